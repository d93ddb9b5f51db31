// Shared pieces of the four-wave kernels with asm-owned accumulators (conv3x3_fat.hip, conv1x1_fat.hip, conv1x1_duo.hip; the seam
// kernel takes the compile-time loops and the MFMA wrappers): compile-time loops, MFMAs on named AGPR accumulator quads, loads / waits /
// LDS-DMA hidden from hipcc's own wait insertion, the weight ring's counted-wait table and drain, and the epilogue arithmetic (bias,
// residual, ReLU, pack). See conv3x3_fat.hip's header. The 1x1 kernels' tile and k-loop are in fat1x1_dev.h.
#pragma once
#include <utility>

#include "igemm_dev.h"

namespace {

template <typename F, int... Is>
__device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sfor(F&& f) {
    sfor_impl(f, std::make_integer_sequence<int, N>{});
}

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) unsigned char lds_u8_t;
typedef __attribute__((address_space(3))) u32x4_t lds_u32x4_t;

template <int AQ>  // AGPR quad AQ += a x b
__device__ __forceinline__ void fat_mfma(const u32x4_t& a, const u32x4_t& b) {
    if constexpr (kLpF16) asm volatile("v_mfma_f32_16x16x32_f16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(a), "v"(b), "n"(4 * AQ), "n"(4 * AQ + 3));
    else asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(a), "v"(b), "n"(4 * AQ), "n"(4 * AQ + 3));
}
template <int AQ>
__device__ __forceinline__ void fat_zero() {
    asm volatile("v_accvgpr_write_b32 a[%c0], 0\n\tv_accvgpr_write_b32 a[%c1], 0\n\tv_accvgpr_write_b32 a[%c2], 0\n\tv_accvgpr_write_b32 a[%c3], 0" ::"n"(4 * AQ),
                 "n"(4 * AQ + 1), "n"(4 * AQ + 2), "n"(4 * AQ + 3));
}
template <int AQ>
__device__ __forceinline__ f32x4_t fat_read() {
    float x, y, z, w;
    asm volatile("v_accvgpr_read_b32 %0, a[%c4]\n\tv_accvgpr_read_b32 %1, a[%c5]\n\tv_accvgpr_read_b32 %2, a[%c6]\n\tv_accvgpr_read_b32 %3, a[%c7]"
                 : "=v"(x), "=v"(y), "=v"(z), "=v"(w)
                 : "n"(4 * AQ), "n"(4 * AQ + 1), "n"(4 * AQ + 2), "n"(4 * AQ + 3));
    return f32x4_t{x, y, z, w};
}
// 16 bytes per lane global -> VGPRs behind hipcc's back: valid only after a counted wait that names the register
template <int IMM>
__device__ __forceinline__ void fat_gload(u32x4_t& dst, unsigned off, const unsigned char* base) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(off), "s"(base), "n"(IMM) : "memory");
}
template <int N>
__device__ __forceinline__ void fat_wait(u32x4_t& a) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N) : "memory"); }
__device__ __forceinline__ void fat_dma(const unsigned char* src, unsigned lds_wave_addr) {  // lane L's 16 bytes -> LDS lds_wave_addr + 16 L
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds_wave_addr)
                 : "memory");
}

// the same with a scalar base and a 32-bit lane offset (one VGPR per request instead of two)
__device__ __forceinline__ void fat_dma_s(const unsigned char* sbase, unsigned voff, unsigned lds_wave_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_wave_addr)
                 : "memory");
}


// ---- the weight ring. A wave streams its weight fragments global -> RING registers: fragment p of a slab (PS fragments) sits in slot
// p % RING, and behind its MFMAs the slot is refilled with fragment p + RING (of the next slab past the end), followed by
// pieces_behind(p) LDS-DMA pieces of a later slab's pixel rows. Every one of these is a vector-memory operation that retires in order,
// so the wait in front of fragment p may leave allowed[p] operations outstanding: those issued AFTER that fragment's load, in the steady
// state (slab 1 of a simulated run of three; the prologues issue the first ring in the same order, so the budget holds from slab 0 on).
template <int RING, int PS>
struct FatRingSched {
    int allowed[PS];
};
template <int RING, int PS, typename F>
constexpr FatRingSched<RING, PS> fat_ring_sched(F pieces_behind) {
    FatRingSched<RING, PS> s{};
    int issued[4][PS] = {};
    int seq = 0;
    for (int p = 0; p < RING; ++p) issued[0][p] = seq++;
    for (int k = 0; k < 3; ++k)
        for (int p = 0; p < PS; ++p) {
            if (k == 1) s.allowed[p] = seq - 1 - issued[k][p];
            const int q = p + RING;
            if (q >= PS) issued[k + 1][q - PS] = seq++;
            else issued[k][q] = seq++;
            seq += pieces_behind(p);
        }
    return s;
}
// behind the k-loop: fragments (and pieces) requested past the end are still landing -- the ring registers stay pinned across the wait,
// and the last MFMAs have left the pipe before the first accumulator read
template <int RING>
__device__ __forceinline__ void fat_ring_drain(u32x4_t (&wr)[RING]) {
#pragma unroll
    for (int i = 0; i < RING; ++i) asm volatile("" : "+v"(wr[i]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < RING; ++i) asm volatile("" : "+v"(wr[i]));
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
}

// ---- epilogue arithmetic on the eight channels a lane holds of one pixel: quads QLO (channels 0 .. 3) and QHI (4 .. 7)
template <int QLO, int QHI>   // v = alpha acc + bias (alpha = 1: acc + bias bit for bit -- one rounding of the same exact sum)
__device__ __forceinline__ void fat_bias8(float (&v)[8], float alpha, const float4& b0, const float4& b1) {
    const f32x4_t lo = fat_read<QLO>(), hi = fat_read<QHI>();
    v[0] = fmaf(alpha, lo[0], b0.x); v[1] = fmaf(alpha, lo[1], b0.y); v[2] = fmaf(alpha, lo[2], b0.z); v[3] = fmaf(alpha, lo[3], b0.w);
    v[4] = fmaf(alpha, hi[0], b1.x); v[5] = fmaf(alpha, hi[1], b1.y); v[6] = fmaf(alpha, hi[2], b1.z); v[7] = fmaf(alpha, hi[3], b1.w);
}
__device__ __forceinline__ void fat_add_lp16x8(float (&v)[8], const u32x4_t& r) {   // v += eight 16-bit values (a residual cell; rounded activations into a pool sum)
    const uint32_t w4[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float l, h;
        unpack_lp16x2(w4[e], l, h);
        v[2 * e] += l;
        v[2 * e + 1] += h;
    }
}
__device__ __forceinline__ void fat_relu8(float (&v)[8], int relu) {
    if (relu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = relu_nan(v[e]);
    }
}
__device__ __forceinline__ uint4 fat_pack8(const float (&v)[8]) {   // one rounding to the 16-bit type
    return make_uint4(pack_lp16x2(v[0], v[1]), pack_lp16x2(v[2], v[3]), pack_lp16x2(v[4], v[5]), pack_lp16x2(v[6], v[7]));
}
// fp32 -> the split-fp16 planes of round 6's conforming mode: hi = fp16(v) (round to nearest), lo = fp16((v - hi) 2^11) -- the difference is
// exact in fp32, the scale keeps lo a NORMAL fp16 wherever hi is one (the consumer's weight segment for the lo plane carries the 2^-11)
__device__ __forceinline__ void split16_pack8(const float (&v)[8], uint4& hi, uint4& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = pack_lp16x2(v[2 * e], v[2 * e + 1]);
        float a, b;
        unpack_lp16x2(h[e], a, b);
        l[e] = pack_lp16x2((v[2 * e] - a) * 2048.f, (v[2 * e + 1] - b) * 2048.f);
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}
// the lane's eight channels of one output pixel, 16-bit or as planes [hi | lo 2^11 | hi] (`o` = the hi plane, `plane` bytes apart)
__device__ __forceinline__ void fat_store8(unsigned char* o, const float (&v)[8]) { *reinterpret_cast<uint4*>(o) = fat_pack8(v); }
__device__ __forceinline__ void fat_store8_split16(unsigned char* o, size_t plane, const float (&v)[8]) {
    uint4 ph, pl;
    split16_pack8(v, ph, pl);
    *reinterpret_cast<uint4*>(o) = ph;
    *reinterpret_cast<uint4*>(o + plane) = pl;
    *reinterpret_cast<uint4*>(o + 2 * plane) = ph;
}

}  // namespace
