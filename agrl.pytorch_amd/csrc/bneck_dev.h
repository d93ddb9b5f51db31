// Stages shared by the fused Bottleneck kernels (bottleneck_tail.hip, bottleneck_block.hip). Behind its first 1x1 GEMM every
// one of them does the same thing to a 64-pixel tile: bias + residual (in place) + ReLU into the swizzled out tile, drain it to
// HBM, run the next block's conv1 straight from it, stage and drain the z tile -- fed by the same LDS-DMA pieces. Each stage
// is here once, as a plain function template; the kernels keep their own pipelines (what is prefetched how far ahead, which
// wait counts which pieces) and pass in this lane's pixel / channel mapping -- the opaque per-tile copies where a kernel
// keeps its address arithmetic out of scratch that way.
#pragma once
#include <initializer_list>
#include "igemm_dev.h"

// ---- tiles: 64 pixel rows of ROWB bytes (128 / 256 / 512 / 1024 = 64 / 128 / 256 / 512 channels), 16-byte chunk c of row r
// at chunk c ^ (r & mask): conflict-free ds_read_b128 of a fragment (16 rows x 4 chunks). The drains and the residual DMA
// apply the same swizzle on the global side, so both move whole rows.
template <int ROWB>
__device__ __forceinline__ int bneck_swz(int row, int chunk) {  // where chunk `chunk` of row `row` sits in its row
    constexpr int MASK = (ROWB / 16 < 32 ? ROWB / 16 : 32) - 1;
    return chunk ^ (row & MASK);
}
template <int ROWB, typename P>
__device__ __forceinline__ P bneck_chunk(P tile, int row, int chunk) { return tile + row * ROWB + (bneck_swz<ROWB>(row, chunk) << 4); }
template <int ROWB, typename P>
__device__ __forceinline__ P bneck_cell(P tile, int px, int c) {  // channels c .. c + 3 (c a multiple of 4) of pixel px
    return bneck_chunk<ROWB>(tile, px, c >> 3) + ((c & 4) << 1);
}

// ---- per-lane constants. Fragment (a, b) of a wave's accumulator tile covers channels c0 + 16 a .. + 3 (c0 includes
// 4 * (lane >> 4)) of pixel px0 + 16 b (px0 includes lane & 15): the MFMA C layout.
template <bool ADD, int NA>
__device__ __forceinline__ void bneck_bias(float (&b)[NA][4], const float* g, int c0) {  // ADD: the CAT form's b3 + bs
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const float4 t = *reinterpret_cast<const float4*>(g + c0 + a * 16);
        b[a][0] = ADD ? b[a][0] + t.x : t.x; b[a][1] = ADD ? b[a][1] + t.y : t.y;
        b[a][2] = ADD ? b[a][2] + t.z : t.z; b[a][3] = ADD ? b[a][3] + t.w : t.w;
    }
}
// MFMA A fragments of a (N, K) weight matrix for register-resident weights: channel ch0 + 16 a (ch0 includes lane & 15), k-step ks
template <int NA, int NK>
__device__ __forceinline__ void bneck_wfrags(uint4 (&w)[NA][NK], const void* wg, int ch0, int K, int fchunk) {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int ks = 0; ks < NK; ++ks)
            w[a][ks] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(wg) + ((size_t)(ch0 + a * 16) * K + ks * 32 + fchunk * 8) * 2);
}
// opaque from here on: the compiler must keep the values in registers rather than re-load them inside the tile loop (its own
// loads come with vmcnt waits that would drain the DMA queue)
template <int NA, int NK>
__device__ __forceinline__ void bneck_pin(uint4 (&w)[NA][NK]) {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) asm volatile("" : "+v"(w[a][ks].x), "+v"(w[a][ks].y), "+v"(w[a][ks].z), "+v"(w[a][ks].w));
}
template <int NA>
__device__ __forceinline__ void bneck_pin(float (&b)[NA][4]) {
#pragma unroll
    for (int a = 0; a < NA; ++a) asm volatile("" : "+v"(b[a][0]), "+v"(b[a][1]), "+v"(b[a][2]), "+v"(b[a][3]));
}

// ---- LDS-DMA stagers
// one 1 KB piece = eight 128-byte rows of a k-tile in the lds_off layout: this lane brings chunk lchk of row `row`, whose
// k-tile starts at grow (ok = false: zeros)
__device__ __forceinline__ void bneck_dma_rows(const unsigned char* grow, bool ok, int row, int lchk, unsigned char* lds_piece) {
    dma16(ok ? grow + ((lchk ^ ((row >> 1) & 7)) << 4) : reinterpret_cast<const unsigned char*>(&g_zero16), lds_piece);
}
// NP pieces per wave of a residual tile with ROWB-byte rows (whole rows per piece): src(j, row, gch) is the global address of
// the chunk this lane brings for piece j -- chunk gch of the tile's row `row`
template <int ROWB, int NP, typename SRC>
__device__ __forceinline__ void bneck_dma_tile(unsigned char* st, int wave, int lane, SRC&& src) {
    constexpr int CPR = ROWB / 16;  // chunks per row
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int piece = wave * NP + j;
        const int row = piece * (64 / CPR) + (CPR < 64 ? lane / CPR : 0);
        dma16(src(j, row, bneck_swz<ROWB>(row, CPR < 64 ? lane & (CPR - 1) : lane)), st + piece * 1024);
    }
}

// ---- bias + residual (in place) + ReLU -> 16-bit out tile. All residual cells are read before the first is written back (a
// read behind a write to the same array is not hoisted by the compiler: NA * NB LDS round trips in a row otherwise).
template <bool RES, int ROWB, int NA, int NB>
__device__ __forceinline__ void bneck_out_tile(unsigned char* sr, const f32x4_t (&acc)[NA][NB], const float (&bias)[NA][4], int px0, int c0) {
    uint2 rcell[NB][NA];
    if constexpr (RES) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int a = 0; a < NA; ++a) rcell[b][a] = *reinterpret_cast<const uint2*>(bneck_cell<ROWB>(sr, px0 + b * 16, c0 + a * 16));
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            float rr[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (RES) {
                unpack_lp16x2(rcell[b][a].x, rr[0], rr[1]);
                unpack_lp16x2(rcell[b][a].y, rr[2], rr[3]);
            }
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = relu_nan(acc[a][b][r] + bias[a][r] + rr[r]);
            store4<lp16_t>(reinterpret_cast<lp16_t*>(bneck_cell<ROWB>(sr, px0 + b * 16, c0 + a * 16)), v);
        }
}

// ---- tile -> HBM, whole 16-byte chunks: NI per thread, chunk pch0 + PSTEP i of row row0 + RSTEP i. dst(i, row, gch, g) sets
// g to the chunk's global address (it is chunk gch of the global row) and says whether the row exists.
template <int ROWB, int NI, int RSTEP, int PSTEP, typename DST>
__device__ __forceinline__ void bneck_drain(const unsigned char* st, int row0, int pch0, DST&& dst) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int row = row0 + RSTEP * i, pch = pch0 + PSTEP * i;
        unsigned char* g;
        if (dst(i, row, bneck_swz<ROWB>(row, pch), g)) {
            const uint4 v = *reinterpret_cast<const uint4*>(st + row * ROWB + (pch << 4));
            *reinterpret_cast<uint4*>(g) = v;
        }
    }
}

// ---- the next block's conv1, B operand straight from the out tile: K = ROWB / 2, NB pixel fragments from px0, NA channel
// fragments whose A operand wfrag(a, ks) brings (an LDS read or a register). Pixel fragments are read AHEAD k-steps in front
// of their MFMAs; with AHEAD > 0 a sched_barrier per k-step keeps the compiler from hoisting all the reads.
template <int ROWB, int AHEAD, int NA, int NB, typename WF>
__device__ __forceinline__ void bneck_gemm2(const unsigned char* sr, int px0, int fchunk, f32x4_t (&acc)[NA][NB], WF&& wfrag) {
    constexpr int NKS = ROWB / 64, RING = AHEAD + 1;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    uint4 xr[RING][NB];
    auto ld = [&](int ks, int slot) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int px = px0 + b * 16;
            xr[slot][b] = *reinterpret_cast<const uint4*>(bneck_chunk<ROWB>(sr, px, ks * 4 + fchunk));
        }
    };
#pragma unroll
    for (int ks = 0; ks < AHEAD; ++ks) ld(ks, ks);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        uint4 wf[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) wf[a] = wfrag(a, ks);
        if (ks + AHEAD < NKS) ld(ks + AHEAD, (ks + AHEAD) % RING);
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[a][b] = Frag<lp16_t>::mma(wf[a], xr[ks % RING][b], acc[a][b]);
        if constexpr (AHEAD > 0) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- bias + ReLU -> 16-bit z tile of CN channels (rows of 2 CN bytes)
template <int CN, int NA, int NB>
__device__ __forceinline__ void bneck_z_tile(unsigned char* sz, const f32x4_t (&acc)[NA][NB], const float (&bias)[NA][4], int px0, int c0) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = relu_nan(acc[a][b][r] + bias[a][r]);
            store4<lp16_t>(reinterpret_cast<lp16_t*>(bneck_cell<2 * CN>(sz, px0 + b * 16, c0 + a * 16)), v);
        }
}

// ---- host side of the two entry points
// `required` holds no null; exactly one of the residual map and the shortcut conv's input is given, the latter with its weights
static inline int bneck_check_operands(const char* who, std::initializer_list<const void*> required, const void* residual,
                                       const void* x_short, const void* w_short, const void* b_short) {
    bool all = true;
    for (const void* q : required) all = all && q != nullptr;
    AGRL_CHECK_ARG(all, "%s: null pointer", who);
    AGRL_CHECK_ARG((residual != nullptr) != (x_short != nullptr), "%s: pass either the residual map or the downsample conv's input, not both", who);
    AGRL_CHECK_ARG(!x_short || (w_short && b_short), "%s: the downsample form needs its weights and bias", who);
    return 0;
}
static inline int bneck_check_aligned(const char* who, std::initializer_list<const void*> ptrs) {
    uintptr_t al = 0;
    for (const void* q : ptrs) al |= (uintptr_t)q;
    AGRL_CHECK_ARG((al & 15) == 0, "%s: pointers must be 16-byte aligned", who);
    return 0;
}
// persistent workgroups, one per CU
static inline int bneck_grid(int ntiles) { return ntiles < 256 ? ntiles : 256; }
