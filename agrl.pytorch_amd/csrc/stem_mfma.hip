// bf16-MFMA stem: conv 7x7/2 (3->64, BN folded) + ReLU + maxpool 3x3/2, fused. vmgn.py:281-284.
//
// The 7x7x3 filter is turned into a K = 7 x 32 contraction that needs NO im2col: the input patch sits in LDS as
// bf16 [y][x][4] (3 channels + a zero), so for a fixed filter row r the 7 taps x 4 channels an output pixel
// needs are 28 CONTIGUOUS bf16; padding that to 32 (the extra pixel meets zero weights) makes one k-step of
// v_mfma_f32_16x16x32_bf16 per filter row, and every lane's 8-element operand slice is one aligned ds_read_b128
// straight out of the patch. 1.5x redundant MFMA work buys zero gather instructions.
//
// One 512-thread workgroup -> an 8x8 tile of POOLED pixels x 64 channels of one frame:
//   patch 39x40x4 bf16 (12.5 KB) + packed weights 64 x 240 bf16 (30 KB, LDS-DMA)      -> LDS
//   conv tile 17x17 = 289 positions x 64 ch: 19 position fragments over 8 waves, 7 k-steps, +bias, ReLU
//   -> bf16 conv tile in LDS (overlaying patch+weights) -> 3x3/2 max -> NHWC store (128 B per pooled pixel)
// Frames whose pooled row is 17 .. 32 wide (256 x 128 among them) take stem_regpool_kernel below instead (AGRL_STEM_REGPOOL): the same
// contraction with the fragments laid out so that the pool is taken in registers; bit-identical outputs.
#include <stdlib.h>

#include <type_traits>

#include "stem_dev.h"

namespace {
using namespace stem8;  // tile geometry, tile decode, patch prefetch, weight DMA: shared with stem_split16.hip

// Persistent form: a workgroup keeps the packed weights in LDS and walks tiles; the NEXT tile's input pixels are requested
// (12 floats per thread, in registers) right after the current patch has been written to LDS, so the HBM round trip runs
// under the MFMA sweep, the conv-tile epilogue and the pooling of the current tile. The one-tile-per-workgroup form spent
// most of a workgroup's life waiting: for its weights (30 KB per 8 x 8 pooled pixels), its pixels, its three barriers.
// LDS: weights 30 KB + one region that holds the patch, then the conv tile (37 KB) = 67 KB: two workgroups per CU.
constexpr int CT_BYTES = (NPOS + 3) * 128;
constexpr int REGION_BYTES = CT_BYTES > PATCH_BYTES ? CT_BYTES : PATCH_BYTES;

// SPLIT: the patch and the conv tile in SEPARATE LDS regions (12.2 + 36.5 + 30 KB + biases = 78.9 KB: still two workgroups per CU) -- the
// two barriers that guarded the overlay (sweep done -> conv tile may be written; pool done -> next patch may be written) disappear: a wave
// that has finished pooling writes its pixels of the next patch while the others still pool, two barriers per tile instead of four.
//
// TIN = unsigned char (uint8 frames, one trailing FramesU8 argument; stem8::PatchPrefetch): the gather from the 3 KB table (L1-resident;
// in LDS it would cost the SPLIT form its second workgroup per CU) is issued behind the conv-tile barrier, when the bytes have had the
// whole MFMA sweep to land, and is in flight under the pooling. Everything from the LDS write of the patch on is the fp32 form's code.
template <bool SPLIT, typename TIN, typename... EX>
__global__ __launch_bounds__(NTH, 4) void stem_mfma_kernel(const TIN* __restrict__ x, const unsigned char* __restrict__ wpk,
                                                        const float* __restrict__ bias, lp16_t* __restrict__ out, int H,
                                                        int W, int CH, int CW, int PH, int PW, int tiles_w, int tiles_hw,
                                                        int ntiles, int xcd_map, EX... ex) {
    constexpr int TILES_BYTES = SPLIT ? PATCH_BYTES + CT_BYTES : REGION_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILES_BYTES + W_BYTES + 256];
    unsigned char* s_patch = smem;
    unsigned char* s_ct = SPLIT ? smem + PATCH_BYTES : smem;
    unsigned char* s_w = smem + TILES_BYTES;
    float* s_bias = reinterpret_cast<float*>(smem + TILES_BYTES + W_BYTES);  // 64 biases: LDS reads in the epilogue instead
                                                                             // of global loads whose waits also cover the prefetch

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;

    weights_to_lds(wpk, s_w, wave, lane);  // once per workgroup
    if (tid < 64) s_bias[tid] = bias[tid];
    PatchPrefetch<TIN, EX...> pre;  // one pixel (3 channels -> 4 bf16) per thread per pass
    constexpr bool U8 = decltype(pre)::U8;
    const int frow = lane & 15, g = lane >> 4;
    int a_off[FPW];  // byte offset of this lane's patch slice at filter row 0
    patch_frag_offsets(wave, frow, g, a_off);

    // Tile order. Neighbouring tiles share 7 of their 39 input columns / rows, and a 39-pixel row segment of a tile straddles 2-3 of the
    // 4 128-byte lines of its image row: with tile T on workgroup T mod G (XCD T mod 8) the four tiles across an image row sat on four
    // XCDs, each pulling its own copy of the shared lines into its own L2 -- counter fetch 300 MB for 100.7 MB of frames (2.5 x across, 1.22 x
    // down: round-5 PMC pass). Here every FRAME belongs to one XCD (frame n -> XCD n mod 8), whose G / 8 workgroups walk its frames' tiles
    // together (four frames in flight per XCD): the overlaps are L2 hits.
    const int nframes = ntiles / tiles_hw;
    const bool xmap = xcd_map && (G & 7) == 0 && nframes >= 8;
    const int xcd = blockIdx.x & 7;
    const int qstep = xmap ? (G >> 3) : G;
    const int qlimit = xmap ? ((nframes - xcd + 7) >> 3) * tiles_hw : ntiles;
    auto tile_of = [&](int q) {
        if (!xmap) return q;
        const int fl = q / tiles_hw;
        return (xcd + 8 * fl) * tiles_hw + (q - fl * tiles_hw);
    };
    int q = xmap ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (q < qlimit) {
        pre.load(x, H, W, tile_at(tile_of(q), tiles_w, tiles_hw), ex...);
        pre.normalize(ex...);
    }
    for (; q < qlimit; q += qstep) {
        const Tile t = tile_at(tile_of(q), tiles_w, tiles_hw);
        const int n = t.n, ph0 = t.ph0, pw0 = t.pw0, cr0 = t.cr0, cc0 = t.cc0;
        // ---- this tile's pixels (requested one tile ago) -> bf16 patch in LDS
        int tw = tid;
        if constexpr (U8) asm volatile("" : "+v"(tw));  // the uint8 form has no register to spare for hoisted LDS addresses
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int e = tw + NTH * i;
            if (e < IT * PWP) {
                uint2 u;
                u.x = pack_lp16x2(pre.pv[i][0], pre.pv[i][1]);
                u.y = (uint32_t)f32_to_lp16(pre.pv[i][2]);
                *reinterpret_cast<uint2*>(s_patch + e * 8) = u;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first tile: the weight DMA (invisible to the compiler) has landed
        __syncthreads();
        // the next tile's pixels: in flight until the top of the next iteration
        if (q + qstep < qlimit) pre.load(x, H, W, tile_at(tile_of(q + qstep), tiles_w, tiles_hw), ex...);

        f32x4_t acc[FPW][4];
#pragma unroll
        for (int i = 0; i < FPW; ++i)
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[i][a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            uint4 wf[4], xf[FPW];
#pragma unroll
            for (int a = 0; a < 4; ++a)
                wf[a] = *reinterpret_cast<const uint4*>(s_w + (a * 16 + frow) * WROW_BYTES + r * 64 + g * 16);
#pragma unroll
            for (int i = 0; i < FPW; ++i) xf[i] = *reinterpret_cast<const uint4*>(s_patch + a_off[i] + r * (PWP * 8));
#pragma unroll
            for (int i = 0; i < FPW; ++i)
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    acc[i][a] = mfma_lp16_16x16x32(wf[a], xf[i], acc[i][a]);
        }
        if constexpr (!SPLIT) __syncthreads();  // every wave is done with the patch: the conv tile may overlay it
        int fr = frow, gg = g, tq = tid;
        asm volatile("" : "+v"(fr), "+v"(gg), "+v"(tq));  // epilogue / pooling addresses are recomputed per tile

        // conv tile [pos][64 ch] bf16, 8-byte slot s of row p stored at slot s ^ (p & 15); row p lives at row index ct_row(p)
        // = p with bits 0 and 1 swapped: a 32-lane group of the pooling reads below covers two pooled pixels = rows p and
        // p + 2, which would share every bank (rows alternate between the halves of the 256-byte bank window by bit 0)
        // conv positions outside the conv map (only tiles on the top / left image border have any) count as 0 in the pool
        const bool interior = cr0 >= 0 && cc0 >= 0 && cr0 + CT <= CH && cc0 + CT <= CW;
        int rowo[FPW], swz[FPW];
        bool live[FPW], in[FPW];
#pragma unroll
        for (int i = 0; i < FPW; ++i) {
            const int pos = (wave + NWV * i) * 16 + fr;
            const int cy = pos / CT, cx = pos - cy * CT;
            live[i] = pos < NPOS;
            in[i] = interior || ((unsigned)(cr0 + cy) < (unsigned)CH && (unsigned)(cc0 + cx) < (unsigned)CW);
            rowo[i] = ct_row(pos) * 128;
            swz[i] = pos & 7;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int ch = a * 16 + gg * 4;
            const float4 bv = *reinterpret_cast<const float4*>(s_bias + ch);
#pragma unroll
            for (int i = 0; i < FPW; ++i) {
                if (live[i]) {
                    const float v0 = relu_nan(acc[i][a][0] + bv.x), v1 = relu_nan(acc[i][a][1] + bv.y);
                    const float v2 = relu_nan(acc[i][a][2] + bv.z), v3 = relu_nan(acc[i][a][3] + bv.w);
                    uint2 u;
                    u.x = pack_lp16x2(v0, v1);
                    u.y = pack_lp16x2(v2, v3);
                    if (!in[i]) u = make_uint2(0u, 0u);
                    *reinterpret_cast<uint2*>(s_ct + rowo[i] + (((ch >> 3) ^ swz[i]) << 4) + ((ch & 4) << 1)) = u;
                }
            }
        }
        __syncthreads();
        if (q + qstep < qlimit) pre.normalize(ex...);  // uint8 frames: the next tile's bytes have landed under the sweep

        // 3x3/2 max pool: thread -> 8 channels (one 16-byte slot) of ONE pooled pixel. The activations are post-ReLU bf16,
        // i.e. non-negative: their bit patterns order like unsigned 16-bit integers, so the maximum is two v_pk_max_u16 per
        // dword pair instead of unpack + fmax per channel (the kernel is VALU-bound)
        {
            typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
            const int cq = tq & 7;
            const int pp = tq >> 3;
            const int py = pp / PT, px = pp - py * PT;
            const int ph = ph0 + py, pw = pw0 + px;
            if (ph < PH && pw < PW) {
                u16x2_t m[4] = {u16x2_t{0, 0}, u16x2_t{0, 0}, u16x2_t{0, 0}, u16x2_t{0, 0}};
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int pos = (2 * py + dy) * CT + 2 * px + dx;
                        const uint4 u = *reinterpret_cast<const uint4*>(s_ct + ct_row(pos) * 128 + ((cq ^ (pos & 7)) << 4));
                        const uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) m[e] = __builtin_elementwise_max(m[e], __builtin_bit_cast(u16x2_t, w4[e]));
                    }
                const uint4 o = make_uint4(__builtin_bit_cast(uint32_t, m[0]), __builtin_bit_cast(uint32_t, m[1]),
                                           __builtin_bit_cast(uint32_t, m[2]), __builtin_bit_cast(uint32_t, m[3]));
                *reinterpret_cast<uint4*>(out + (((size_t)n * PH + ph) * PW + pw) * 64 + cq * 8) = o;
            }
        }
        if constexpr (!SPLIT) __syncthreads();  // the conv tile is consumed: the next patch may overwrite it
    }
}

// ---- register-pool form: the 3x3/2 maximum is taken on the fp32 accumulators, no conv tile goes through LDS ----------------------
// a -> round16(relu(a + b)) is non-decreasing, so max over a window of round16(relu(acc + b)) = round16(relu(max(acc) + b)) bit for bit
// (and a NaN still wins: every maximum here is the NaN-propagating one). Each conv position is the same 7 k-steps r = 0..6 of the same
// MFMA on the same operands as in stem_mfma_kernel, so the outputs are the conv-tile kernel's.
//
// Mapping (stem_dev.h, namespace stem_rp): a position fragment = 16 adjacent pooled columns px = 16 G + (lane & 15) of ONE conv row at ONE
// column phase (conv column 2 px or 2 px + 1); lanes >> 4 pick 4 channels per channel fragment as before. A wave owns two pooled rows of
// the tile and does column group 0 for both, then group 1. For a pooled row it sweeps conv rows 2 py and 2 py + 1 at both phases (4
// position x 4 channel fragments x 7 k-steps). The window's third row 2 py - 1 is the previous pooled row's 2 py + 1, carried in registers
// (column-maxed, 16 values); it is swept once at the top of the wave's strip: 8.75 MFMAs per pooled pixel where the conv tile took 10.5.
// The third column 2 px - 1 is the left neighbour's odd phase: a DPP row_shr:1 inside the 16-lane row; lane 0 of group 1 takes group 0's
// lane 15, which the wave left in a 1 280-byte LDS slot of its own (20 ds_write_b128 + 20 ds_read_b128 per wave and tile beside 308
// operand reads; kept in registers across group 1's sweep the hand-over spilt). Conv row / column -1 and rows / columns past the conv map
// enter no maximum (-inf). Then once per pooled value: + bias, ReLU, one RNE rounding; two v_permlane16_swap per channel-fragment pair
// give each lane 8 adjacent channels, stored as 16 bytes.
//
// Patch: [39][134][4] 16-bit, plain row-major (row stride 1072 B). Lane (f, g) of a fragment reads 16 B at pixel 4 (16 G + f) + 2 phase +
// 2 g: its 16-byte slot index is 2 f + g + const. A ds_read_b128 is served in groups of 16 lanes holding f in {0-3, 12-15} at chunk g and
// f in {4-11} at chunk g + 1 (or the converse): the first set lands on the 8 slots of one parity mod 16, the second on the other
// parity's 8 -- 0 bank conflicts, with no swizzle. The weight reads are stem_mfma_kernel's (conflict-free, stem_dev.h).
// LDS 41 808 + 30 720 + 256 + 5 120 = 77 904 B: two 256-thread workgroups per CU, two waves per SIMD, so the register budget is 256.
namespace rp = stem_rp;

__device__ __forceinline__ float fmax_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float old, float src) {  // lanes whose source lane lies outside the 16-lane row keep ``old``
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), CTRL, 0xf,
                                                                  0xf, false));
}
constexpr int DPP_ROW_SHR1 = 0x111;

// NR conv rows (patch rows 2 i + r) x both column phases x 64 channels: acc[i][phase][channel fragment]
template <int NR>
__device__ __forceinline__ void rp_sweep(const unsigned char* xb, const unsigned char* wb, f32x4_t (&acc)[NR][2][4]) {
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[i][p][a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // operands of k-step r + 1 are requested before the MFMAs of k-step r; the scheduling fence keeps the compiler from requesting
    // further ahead (at 16 registers a k-step, it spilt)
    uint4 wf[2][4], xf[2][NR][2];
    auto fetch = [&](int r, uint4 (&w)[4], uint4 (&xx)[NR][2]) {
#pragma unroll
        for (int a = 0; a < 4; ++a) w[a] = *reinterpret_cast<const uint4*>(wb + a * 16 * WROW_BYTES + r * 64);
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int p = 0; p < 2; ++p) xx[i][p] = *reinterpret_cast<const uint4*>(xb + (2 * i + r) * rp::ROW_BYTES + p * 16);
    };
    fetch(0, wf[0], xf[0]);
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        if (r < 6) fetch(r + 1, wf[(r + 1) & 1], xf[(r + 1) & 1]);
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int a = 0; a < 4; ++a) acc[i][p][a] = mfma_lp16_16x16x32(wf[r & 1][a], xf[r & 1][i][p], acc[i][p][a]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// maximum over conv columns 2 px - 1, 2 px, 2 px + 1 of one conv row: h = max(even, odd, left neighbour's odd). Lane 0 of each 16-lane
// row has no left neighbour in its fragment: in group 0 that is conv column -1 (-inf); in group 1 it is group 0's lane 15, which group 0
// left in ``edge`` (this wave's 256-byte LDS slot of the conv row: [lane >> 4][16 floats]) -- same wave, program order, no barrier.
template <int GQ>
__device__ __forceinline__ void rp_row_max(const f32x4_t (&even)[4], f32x4_t (&odd)[4], float* edge, int frow, bool odd_all_in,
                                           bool odd_in, f32x4_t (&h)[4]) {
    if (!odd_all_in) {  // a conv map narrower than 64: columns 2 px + 1 >= CW enter no maximum
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) odd[a][j] = odd_in ? odd[a][j] : -INFINITY;
    }
    f32x4_t first[4];
    if constexpr (GQ == 0) {
        if (frow == 15) {
#pragma unroll
            for (int a = 0; a < 4; ++a) *reinterpret_cast<f32x4_t*>(edge + 4 * a) = odd[a];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) first[a] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) first[a] = *reinterpret_cast<const f32x4_t*>(edge + 4 * a);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            h[a][j] = fmax_nan(fmax_nan(even[a][j], odd[a][j]), dpp_mov<DPP_ROW_SHR1>(first[a][j], odd[a][j]));
}

template <typename TIN, typename... EX>
__global__ __launch_bounds__(rp::NTH, 2) void stem_regpool_kernel(const TIN* __restrict__ x, const unsigned char* __restrict__ wpk,
                                                                   const float* __restrict__ bias, lp16_t* __restrict__ out, int H,
                                                                   int W, int CH, int CW, int PH, int PW, int tiles_h, int ntiles,
                                                                   int xcd_map, EX... ex) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[rp::PATCH_BYTES + W_BYTES + 256 + rp::EDGE_BYTES];
    unsigned char* s_patch = smem;
    unsigned char* s_w = smem + rp::PATCH_BYTES;
    float* s_bias = reinterpret_cast<float*>(smem + rp::PATCH_BYTES + W_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;

    weights_to_lds(wpk, s_w, wave, lane, rp::NWV);  // once per workgroup
    if (tid < 64) s_bias[tid] = bias[tid];
    rp::PatchPrefetch<TIN, EX...> pre;
    constexpr int NPASS_RP = decltype(pre)::NPASS;
    const int frow = lane & 15, g = lane >> 4;
    // this lane's patch slice of the strip's first conv row (tile row 4 wave) at filter row 0, group 0, even phase; its weight slice
    const unsigned char* xlane = s_patch + 8 * wave * rp::ROW_BYTES + (4 * frow + 2 * g) * 8;
    const unsigned char* wlane = s_w + frow * WROW_BYTES + g * 16;
    // group 0's lane-15 odd phase of this wave's 5 conv rows, for lane 0 of group 1: [wave][conv row][g][16 floats]
    float* s_edge = reinterpret_cast<float*>(smem + rp::PATCH_BYTES + W_BYTES + 256) + (wave * (2 * rp::RPW + 1) * 4 + g) * 16;

    // tile order: stem_mfma_kernel's (frame n on XCD n mod 8, whose G / 8 workgroups walk its frames' tiles together)
    const int nframes = ntiles / tiles_h;
    const bool xmap = xcd_map && (G & 7) == 0 && nframes >= 8;
    const int xcd = blockIdx.x & 7;
    const int qstep = xmap ? (G >> 3) : G;
    const int qlimit = xmap ? ((nframes - xcd + 7) >> 3) * tiles_h : ntiles;
    auto tile_of = [&](int q) {
        if (!xmap) return q;
        const int fl = q / tiles_h;
        return (xcd + 8 * fl) * tiles_h + (q - fl * tiles_h);
    };
    int q = xmap ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (q < qlimit) pre.load(x, H, W, rp::tile_at(tile_of(q), tiles_h), ex...);
    for (; q < qlimit; q += qstep) {
        const Tile t = rp::tile_at(tile_of(q), tiles_h);
        // ---- this tile's pixels (requested one tile ago) -> 16-bit patch in LDS
        pre.normalize(ex...);  // uint8 frames: the table gather, here so that bytes and values are never both held across the sweeps
        int tw = tid;
        asm volatile("" : "+v"(tw));  // LDS addresses per tile, not hoisted
#pragma unroll
        for (int i = 0; i < NPASS_RP; ++i) {
            const int e = tw + rp::NTH * i;
            if ((i + 1) * rp::NTH <= rp::IT * rp::PWP || e < rp::IT * rp::PWP) {  // only the last pass is partial
                uint2 u;
                u.x = pack_lp16x2(pre.pv[i][0], pre.pv[i][1]);
                u.y = (uint32_t)f32_to_lp16(pre.pv[i][2]);
                *reinterpret_cast<uint2*>(s_patch + e * 8) = u;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first tile: the weight DMA (invisible to the compiler) has landed
        __syncthreads();
        if (q + qstep < qlimit) pre.load(x, H, W, rp::tile_at(tile_of(q + qstep), tiles_h), ex...);

        const int ph_w = t.ph0 + rp::RPW * wave;  // the strip's first pooled row
        if (ph_w < PH) {
            const bool odd_all_in = CW >= 4 * rp::MAX_PW;
            auto group = [&](auto gq_c) {
                constexpr int GQ = decltype(gq_c)::value;
                const unsigned char* xg = xlane + GQ * 512;
                const int px = 16 * GQ + frow;
                const bool odd_in = 2 * px + 1 < CW;
                f32x4_t carry[4];
                {   // conv row 2 ph_w - 1: only its column maxima are kept
                    f32x4_t acc[1][2][4];
                    rp_sweep<1>(xg, wlane, acc);
                    rp_row_max<GQ>(acc[0][0], acc[0][1], s_edge, frow, odd_all_in, odd_in, carry);
                    if (ph_w == 0) {  // conv row -1
#pragma unroll
                        for (int a = 0; a < 4; ++a) carry[a] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    }
                }
#pragma unroll
                for (int sp = 0; sp < rp::RPW; ++sp) {
                    const int ph = ph_w + sp;
                    if (ph < PH) {
                        f32x4_t acc[2][2][4], ha[4], hb[4];
                        rp_sweep<2>(xg + (4 * sp + 2) * rp::ROW_BYTES, wlane, acc);
                        rp_row_max<GQ>(acc[0][0], acc[0][1], s_edge + (2 * sp + 1) * 64, frow, odd_all_in, odd_in, ha);
                        rp_row_max<GQ>(acc[1][0], acc[1][1], s_edge + (2 * sp + 2) * 64, frow, odd_all_in, odd_in, hb);
                        if (2 * ph + 1 >= CH) {  // odd conv height: the last pooled row's window has two rows
#pragma unroll
                            for (int a = 0; a < 4; ++a) hb[a] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                        }
                        // pooled pixel (ph, px): channels 16 a + 4 g + j
                        uint32_t pk[4][2];
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const float4 bv = *reinterpret_cast<const float4*>(s_bias + a * 16 + g * 4);
                            float v[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[j] = fmax_nan(fmax_nan(carry[a][j], ha[a][j]), hb[a][j]);
                            carry[a] = hb[a];
                            pk[a][0] = pack_lp16x2(relu_nan(v[0] + bv.x), relu_nan(v[1] + bv.y));
                            pk[a][1] = pack_lp16x2(relu_nan(v[2] + bv.z), relu_nan(v[3] + bv.w));
                        }
                        // rows of 16 lanes g and g ^ 1 trade halves: afterwards lane g holds channel fragment 2 k + (g & 1), channels
                        // 8 (g >> 1) .. + 7 of it, for k = 0, 1
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
                            const u32x2_t s0 = __builtin_amdgcn_permlane16_swap(pk[2 * k][0], pk[2 * k + 1][0], false, false);
                            const u32x2_t s1 = __builtin_amdgcn_permlane16_swap(pk[2 * k][1], pk[2 * k + 1][1], false, false);
                            if (px < PW) {
                                const int ch = (2 * k + (g & 1)) * 16 + (g >> 1) * 8;
                                *reinterpret_cast<uint4*>(out + (((size_t)t.n * PH + ph) * PW + px) * 64 + ch) =
                                    make_uint4(s0[0], s1[0], s0[1], s1[1]);
                            }
                        }
                    }
                }
            };
            group(std::integral_constant<int, 0>{});
            group(std::integral_constant<int, 1>{});
        }
        __syncthreads();  // every wave is done with the patch: the next tile's may be written
    }
}
}  // namespace

// what an unset AGRL_STEM_REGPOOL selects: the register-pool form (step 3.449 against 3.489 ms, four alternated pairs: DESIGN.md 5.4)
constexpr bool STEM_REGPOOL_DEFAULT = true;

template <typename TIN, typename... EX>
static int launch_stem_mfma(const char* who, const TIN* x, const void* w_packed, const float* bias, void* out, int N, int H, int W,
                            agrl_stream_t stream, EX... ex) {
    AGRL_CHECK_ARG(x && w_packed && bias && out, "%s: null pointer", who);
    StemShape s;
    if (stem_shape(who, N, H, W, PT, PT, &s)) return 1;
    AGRL_CHECK_ARG((((uintptr_t)w_packed) & 15) == 0 && (((uintptr_t)bias) & 15) == 0 && (((uintptr_t)out) & 15) == 0,
                   "%s: misaligned pointer", who);
    // AGRL_STEM_REGPOOL: the register-pool form takes every frame whose pooled row is 17 .. 32 wide (W 65 .. 128), any height
    const int regpool = agrl_opts().stem_regpool;
    if ((agrl_opt_set(regpool) ? regpool != 0 : STEM_REGPOOL_DEFAULT) && s.PW >= stem_rp::MIN_PW && s.PW <= stem_rp::MAX_PW) {
        StemShape r;
        if (stem_shape(who, N, H, W, stem_rp::RT, stem_rp::MAX_PW, &r)) return 1;
        const unsigned launch_rp = (unsigned)(r.grid < 512 ? r.grid : 512);  // two persistent workgroups per CU (76 KB of LDS each)
        hipLaunchKernelGGL((stem_regpool_kernel<TIN, EX...>), dim3(launch_rp), dim3(stem_rp::NTH), 0, (hipStream_t)stream, x,
                           (const unsigned char*)w_packed, bias, (lp16_t*)out, H, W, r.CH, r.CW, r.PH, r.PW, r.tiles_h, r.grid,
                           agrl_opts().stem_xcd_map != 0, ex...);
        AGRL_CHECK_LAUNCH(who);
        return 0;
    }
    const int wgs = 512;  // two persistent workgroups per CU (67 KB of LDS each)
    const unsigned launch = (unsigned)(s.grid < wgs ? s.grid : wgs);
    if (agrl_opts().stem_split_lds != 0)
        hipLaunchKernelGGL((stem_mfma_kernel<true, TIN, EX...>), dim3(launch), dim3(NTH), 0, (hipStream_t)stream, x,
                       (const unsigned char*)w_packed, bias, (lp16_t*)out, H, W, s.CH, s.CW, s.PH, s.PW, s.tiles_w, s.tiles_h * s.tiles_w,
                       s.grid, agrl_opts().stem_xcd_map != 0, ex...);
    else
        hipLaunchKernelGGL((stem_mfma_kernel<false, TIN, EX...>), dim3(launch), dim3(NTH), 0, (hipStream_t)stream, x,
                       (const unsigned char*)w_packed, bias, (lp16_t*)out, H, W, s.CH, s.CW, s.PH, s.PW, s.tiles_w, s.tiles_h * s.tiles_w,
                       s.grid, agrl_opts().stem_xcd_map != 0, ex...);
    AGRL_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int agrl_stem_conv_bn_relu_maxpool_lp16(const float* x, const void* w_packed, const float* bias, void* out,
                                                   int N, int H, int W, agrl_stream_t stream) {
    return launch_stem_mfma("agrl_stem_lp16", x, w_packed, bias, out, N, H, W, stream);
}

extern "C" int agrl_stem_conv_bn_relu_maxpool_lp16_u8(const unsigned char* x, const float* table, int layout, const void* w_packed,
                                                      const float* bias, void* out, int N, int H, int W, agrl_stream_t stream) {
    FramesU8 u8;
    if (frames_u8_args("agrl_stem_lp16_u8", table, layout, H, W, &u8)) return 1;
    return launch_stem_mfma("agrl_stem_lp16_u8", x, w_packed, bias, out, N, H, W, stream, u8);
}
