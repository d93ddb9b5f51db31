// Split-fp16 stem (round 6, the conforming mode at speed): conv 7x7/2 (3->64, BN folded) + ReLU + maxpool 3x3/2, fused, in the
// arithmetic of agrl_conv2d_bn_act_split16 -- every product as three fp16 MFMAs on fp16 high / low halves, fp32 accumulation -- with
// fp32 NHWC output. vmgn.py:281-284. The exact-fp32 stem (stem.hip, a VALU kernel) takes 1.0 ms of the conforming mode's 12.6 ms
// step; this one runs the 16-bit stem's structure (stem_mfma.hip: the 7x7x3 filter as a K = 7 x 32 contraction straight out of a
// [y][x][4] patch in LDS, no im2col) three times over:
//   patch     39 x 40 x 4 as TWO fp16 images, hi = fp16(x) and lo = fp16(x - hi) (frames are O(1): lo is unscaled; MFMA keeps fp16
//             subnormals, tests/test_gpu_kernels.py::test_fp16_mfma_keeps_subnormal_operands)
//   weights   wh, wl of w 2^k in the 16-bit stem's packed form (64 x 240 fp16 each, resident in LDS); acc += wh xl + wl xh + wh xh
//   conv tile fp32, 17 x 17 positions x 32 channels at a time (two channel halves per tile: 37 KB instead of 74), v = relu(2^-k acc + b)
//   pooling   3 x 3 / 2 max on the fp32 values, fp32 NHWC store
// LDS 25 + 60 + 37 KB: one 512-thread workgroup per CU, persistent over tiles, the next tile's pixels prefetched into registers.
#include <stdlib.h>

#include "stem_dev.h"

namespace {
using namespace stem8;  // tile geometry, tile decode, patch prefetch, weight DMA: shared with stem_mfma.hip

constexpr int CT_BYTES = (NPOS + 3) * 128;     // [pos][32 channels] fp32

__device__ __forceinline__ f32x4_t mfma_f16_16x16x32(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ uint32_t pack_f16x2(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2_t;
    const h2_t v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, v);
}

// TIN = unsigned char (uint8 frames, one trailing FramesU8 argument; stem8::PatchPrefetch): the gather from the 3 KB table is issued
// behind the first channel half's conv-tile barrier (the bytes have had that half's MFMA sweep to land). The rest is the fp32 form's code.
template <typename TIN, typename... EX>
__global__ __launch_bounds__(NTH) void stem_split16_kernel(const TIN* __restrict__ x, const unsigned char* __restrict__ wh_pk,
                                                           const unsigned char* __restrict__ wl_pk, const float* __restrict__ bias,
                                                           float* __restrict__ out, float alpha, int H, int W, int CH, int CW, int PH,
                                                           int PW, int tiles_w, int tiles_hw, int ntiles, EX... ex) {
    constexpr bool U8 = sizeof...(EX) != 0;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * PATCH_BYTES + CT_BYTES + 2 * W_BYTES + 256];
    unsigned char* s_ph = smem;
    unsigned char* s_pl = smem + PATCH_BYTES;
    unsigned char* s_ct = smem + 2 * PATCH_BYTES;
    unsigned char* s_wh = s_ct + CT_BYTES;
    unsigned char* s_wl = s_wh + W_BYTES;
    float* s_bias = reinterpret_cast<float*>(s_wl + W_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;

    weights_to_lds(wh_pk, s_wh, wave, lane);
    weights_to_lds(wl_pk, s_wl, wave, lane);
    if (tid < 64) s_bias[tid] = bias[tid];

    PatchPrefetch<TIN, EX...> pre;
    const int frow = lane & 15, g = lane >> 4;
    int a_off[FPW];
    patch_frag_offsets(wave, frow, g, a_off);

    int q = blockIdx.x;
    if (q < ntiles) {
        pre.load(x, H, W, tile_at(q, tiles_w, tiles_hw), ex...);
        pre.normalize(ex...);
    }
    for (; q < ntiles; q += G) {
        const Tile t = tile_at(q, tiles_w, tiles_hw);
        const int n = t.n, ph0 = t.ph0, pw0 = t.pw0, cr0 = t.cr0, cc0 = t.cc0;
        // ---- this tile's pixels (requested one tile ago) -> fp16 hi / lo patches in LDS
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int e = tid + NTH * i;
            if (e < IT * PWP) {
                typedef __attribute__((ext_vector_type(2))) _Float16 h2_t;
                const h2_t h01 = {(_Float16)pre.pv[i][0], (_Float16)pre.pv[i][1]};
                const _Float16 h2 = (_Float16)pre.pv[i][2];
                uint2 uh, ul;
                uh.x = __builtin_bit_cast(uint32_t, h01);
                uh.y = (uint32_t)__builtin_bit_cast(unsigned short, h2);
                ul.x = pack_f16x2(pre.pv[i][0] - (float)h01[0], pre.pv[i][1] - (float)h01[1]);
                ul.y = (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)(pre.pv[i][2] - (float)h2));
                *reinterpret_cast<uint2*>(s_ph + e * 8) = uh;
                *reinterpret_cast<uint2*>(s_pl + e * 8) = ul;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first tile: the weight DMA (invisible to the compiler) has landed
        __syncthreads();
        if (q + G < ntiles) pre.load(x, H, W, tile_at(q + G, tiles_w, tiles_hw), ex...);  // in flight until the top of the next iteration

        const bool interior = cr0 >= 0 && cc0 >= 0 && cr0 + CT <= CH && cc0 + CT <= CW;
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            f32x4_t acc[FPW][2];
#pragma unroll
            for (int i = 0; i < FPW; ++i)
#pragma unroll
                for (int a = 0; a < 2; ++a) acc[i][a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 7; ++r) {
                uint4 wh[2], wl[2], xh[FPW], xl[FPW];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int o = ((2 * half + a) * 16 + frow) * WROW_BYTES + r * 64 + g * 16;
                    wh[a] = *reinterpret_cast<const uint4*>(s_wh + o);
                    wl[a] = *reinterpret_cast<const uint4*>(s_wl + o);
                }
#pragma unroll
                for (int i = 0; i < FPW; ++i) {
                    xh[i] = *reinterpret_cast<const uint4*>(s_ph + a_off[i] + r * (PWP * 8));
                    xl[i] = *reinterpret_cast<const uint4*>(s_pl + a_off[i] + r * (PWP * 8));
                }
#pragma unroll
                for (int i = 0; i < FPW; ++i)
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        acc[i][a] = mfma_f16_16x16x32(wh[a], xl[i], acc[i][a]);
                        acc[i][a] = mfma_f16_16x16x32(wl[a], xh[i], acc[i][a]);
                        acc[i][a] = mfma_f16_16x16x32(wh[a], xh[i], acc[i][a]);
                    }
            }
            if (half == 1) __syncthreads();  // every thread has pooled half 0: the conv tile may be rewritten
            int fr = frow, gg = g, tq = tid;
            asm volatile("" : "+v"(fr), "+v"(gg), "+v"(tq));
            // conv tile [pos][32 ch] fp32: 16-byte slot s (4 channels) of row p at slot s ^ (p & 7), row p at row index ct_row(p)
            // (stem_mfma.hip's layout with fp32 x 32 channels in place of fp16 x 64: the same 128-byte rows)
#pragma unroll
            for (int i = 0; i < FPW; ++i) {
                const int pos = (wave + NWV * i) * 16 + fr;
                if (pos < NPOS) {
                    const int cy = pos / CT, cx = pos - cy * CT;
                    const bool in = interior || ((unsigned)(cr0 + cy) < (unsigned)CH && (unsigned)(cc0 + cx) < (unsigned)CW);
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const int chl = a * 16 + gg * 4;   // channel inside the half
                        const float4 bv = *reinterpret_cast<const float4*>(s_bias + half * 32 + chl);
                        float4 v = make_float4(relu_nan(fmaf(alpha, acc[i][a][0], bv.x)), relu_nan(fmaf(alpha, acc[i][a][1], bv.y)),
                                               relu_nan(fmaf(alpha, acc[i][a][2], bv.z)), relu_nan(fmaf(alpha, acc[i][a][3], bv.w)));
                        if (!in) v = make_float4(0.f, 0.f, 0.f, 0.f);   // positions outside the conv map count as 0 in the pool (post-ReLU values are >= 0)
                        *reinterpret_cast<float4*>(s_ct + ct_row(pos) * 128 + (((chl >> 2) ^ (pos & 7)) << 4)) = v;
                    }
                }
            }
            __syncthreads();
            if constexpr (U8) {
                if (half == 0 && q + G < ntiles) pre.normalize(ex...);  // the next tile's bytes have landed under the sweep
            }
            // 3x3/2 max pool: thread -> 4 channels (one 16-byte slot) of one pooled pixel
            {
                const int cq = tq & 7;
                const int pp = tq >> 3;
                const int py = pp / PT, px = pp - py * PT;
                const int ph = ph0 + py, pw = pw0 + px;
                if (ph < PH && pw < PW) {
                    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            const int pos = (2 * py + dy) * CT + 2 * px + dx;
                            const float4 u = *reinterpret_cast<const float4*>(s_ct + ct_row(pos) * 128 + ((cq ^ (pos & 7)) << 4));
                            // (NaN-propagating like the ReLU above: an out-of-range activation must reach the embedding)
                            m.x = __builtin_elementwise_maximum(m.x, u.x); m.y = __builtin_elementwise_maximum(m.y, u.y);
                            m.z = __builtin_elementwise_maximum(m.z, u.z); m.w = __builtin_elementwise_maximum(m.w, u.w);
                        }
                    *reinterpret_cast<float4*>(out + (((size_t)n * PH + ph) * PW + pw) * 64 + half * 32 + cq * 4) = m;
                }
            }
        }
        __syncthreads();  // the conv tile and the patches are consumed: the next tile may overwrite them
    }
}
}  // namespace

template <typename TIN, typename... EX>
static int launch_stem_split16(const char* who, const TIN* x, const void* wh_packed, const void* wl_packed, const float* bias, float* out,
                               int N, int H, int W, float w_unscale, agrl_stream_t stream, EX... ex) {
    AGRL_CHECK_ARG(x && wh_packed && wl_packed && bias && out, "%s: null pointer", who);
    StemShape s;
    if (stem_shape(who, N, H, W, PT, PT, &s)) return 1;
    AGRL_CHECK_ARG(((((uintptr_t)wh_packed) | ((uintptr_t)wl_packed) | ((uintptr_t)bias) | ((uintptr_t)out)) & 15) == 0, "%s: misaligned pointer", who);
    AGRL_CHECK_POW2(w_unscale, who, "w_unscale");
    const int cus = agrl_cu_count();
    const unsigned launch = (unsigned)(s.grid < cus ? s.grid : cus);   // one persistent workgroup per CU (123 KB of LDS)
    hipLaunchKernelGGL((stem_split16_kernel<TIN, EX...>), dim3(launch), dim3(NTH), 0, (hipStream_t)stream, x, (const unsigned char*)wh_packed,
                       (const unsigned char*)wl_packed, bias, out, w_unscale, H, W, s.CH, s.CW, s.PH, s.PW, s.tiles_w, s.tiles_h * s.tiles_w, s.grid, ex...);
    AGRL_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int agrl_stem_split16(const float* x, const void* wh_packed, const void* wl_packed, const float* bias, float* out, int N,
                                 int H, int W, float w_unscale, agrl_stream_t stream) {
    return launch_stem_split16("agrl_stem_split16", x, wh_packed, wl_packed, bias, out, N, H, W, w_unscale, stream);
}

extern "C" int agrl_stem_split16_u8(const unsigned char* x, const float* table, int layout, const void* wh_packed, const void* wl_packed,
                                    const float* bias, float* out, int N, int H, int W, float w_unscale, agrl_stream_t stream) {
    FramesU8 u8;
    if (frames_u8_args("agrl_stem_split16_u8", table, layout, H, W, &u8)) return 1;
    return launch_stem_split16("agrl_stem_split16_u8", x, wh_packed, wl_packed, bias, out, N, H, W, w_unscale, stream, u8);
}
