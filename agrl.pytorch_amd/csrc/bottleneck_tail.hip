// Fused tail of a layer-1 Bottleneck and head of the next one (torchreid/models/vmgn.py:45-65), bf16:
//
//     x_out = relu( W3 y2 + b3 + residual )      1x1 conv   64 -> 256, folded BN, the block's output   (written)
//     z     = relu( W1' x_out + b1' )            1x1 conv  256 ->  64 of the NEXT block, folded BN     (written)
//
// Layer 1 works on 64 x 32 maps (524 288 pixels per 256-frame step) with 64 / 256 channels: every conv there is
// HBM-bound (arithmetic intensity 32-170 flop/B), and the next block's first conv re-reads the 268 MB map the previous
// kernel has just written. Here that conv is computed from the output tile while it is still in LDS: the map is
// written once and not read back (-25 % of a block's HBM bytes, one launch less).
//
//   * persistent workgroups (one per CU, 8 waves), tiles of 64 pixels; BOTH weight matrices stay resident in LDS
//     (32 KB + 32 KB) for the whole kernel
//   * per tile only y2 (8 KB) and the residual (32 KB) come in by LDS-DMA, prefetched one tile ahead (double-buffered);
//     the residual tile is combined in place (fp32 math, one rounding) and IS the out tile: drained to HBM as whole
//     16-byte chunks and re-read as the B operand of the second GEMM (row = pixel, 512 B, chunk c at c ^ (row & 31):
//     conflict-free ds_read_b128)
//   * waits are counted: the prefetch DMA sits in front of the tile's stores in the queue, so waiting for it leaves
//     the stores in flight (loads and stores retire in order on one counter)
//   * everything behind the first GEMM is a stage of bneck_dev.h, shared with the layer-2 form below and bottleneck_block.hip
#include "bneck_dev.h"

namespace {

struct TailParams {
    const void* y2;      // (M, 64)   bf16
    const void* w3;      // (256, 64) bf16, BN folded
    const float* b3;     // (256)
    const void* res;     // (M, 256)  bf16
    void* out;           // (M, 256)  bf16
    const void* w1n;     // (64, 256) bf16, BN folded (next block's conv1)
    const float* b1n;    // (64)
    void* z;             // (M, 64)   bf16
    const void* xs;      // CAT form: (M, 64) bf16 input of the block's 1x1 stride-1 downsample conv (instead of res)
    const void* ws;      // CAT form: (256, 64) bf16 downsample weights, BN folded
    const float* bs;     // CAT form: (256) downsample bias
    int M;
};

constexpr int TBM = 64, TK1 = 64, TN1 = 256, TK2 = 256, TN2 = 64;

// CAT: the residual is the block's own downsample conv (first block of the layer): computed here as a second k-tile,
// out = relu([W3 | Ws] [y2 ; xs] + b3 + bs) -- the 268 MB residual map is neither written nor read.
// CN: output channels of the next block's conv1: 64, or 128 at the layer transition (layer1 -> layer2, 256 -> 128).
template <bool CAT, int CN>
__global__ __launch_bounds__(512) void bottleneck_tail_kernel(const TailParams p, int ntiles) {
    static_assert(CN == 64 || (CN == 128 && !CAT), "next conv1: 64 channels, or 128 with the identity shortcut");
    constexpr int NKT1 = CAT ? 2 : 1;                  // k-tiles of the first GEMM
    constexpr int W3_BYTES = NKT1 * TN1 * 128;         // 32 / 64 KB: [k-tile][256 rows][128 B]
    constexpr int W1_KT = CN * 128;                    // one k-tile of W1': CN rows x 128 B
    constexpr int W1_BYTES = (TK2 / 64) * W1_KT;       // 32 / 64 KB: 4 k-tiles
    constexpr int A_BYTES = NKT1 * TBM * 128;          // 8 / 16 KB input tile
    constexpr int R_BYTES = TBM * TN1 * 2;             // 32 KB residual / out tile, 512-byte rows
    // The LDS budget decides when the residual tile is fetched. CN == 64: two out tile slots fit, the residual comes one
    // tile ahead with y2. CN == 128: the 64 KB of W1' leave room for ONE out tile, so the residual is fetched at the top of
    // its own tile (it lands under the first GEMM's MFMAs); y2 is still prefetched. CAT has no residual tile at all.
    constexpr bool RES_AHEAD = !CAT && CN == 64, RES_OWN = !CAT && CN == 128;
    constexpr int NR = RES_AHEAD ? 2 : 1;              // out tile slots
    constexpr int NA2 = CN / 64;                       // 16-channel fragments of the next conv1 per wave
    constexpr int NST = 4 + NA2;                       // global stores per thread and tile (4 out + 1 or 2 z)
    __shared__ __attribute__((aligned(16))) unsigned char smem[W3_BYTES + W1_BYTES + 2 * A_BYTES + NR * R_BYTES];
    unsigned char* s_w3 = smem;
    unsigned char* s_w1 = s_w3 + W3_BYTES;
    unsigned char* s_a = s_w1 + W1_BYTES;
    unsigned char* s_r = s_a + 2 * A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm2 = wave & 1, wn4 = wave >> 1;  // 2 (pixels) x 4 (channels) wave grid for both GEMMs
    const int frow = lane & 15, fchunk = lane >> 4;
    const int lrow = lane >> 3, lchk = lane & 7;
    const int G = gridDim.x;
    const unsigned char* zsrc = reinterpret_cast<const unsigned char*>(&g_zero16);
    const unsigned char* y2g = reinterpret_cast<const unsigned char*>(p.y2);
    const unsigned char* resg = reinterpret_cast<const unsigned char*>(p.res);

    // ---- resident weights: W3 rows (wave*32 + 8j + lrow), W1' k-tile (kt), rows ((wave + 8h)*8 + lrow)
#pragma unroll
    for (int kt = 0; kt < NKT1; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = wave * 32 + j * 8 + lrow;
            bneck_dma_rows(reinterpret_cast<const unsigned char*>(kt == 0 ? p.w3 : p.ws) + (size_t)row * (TK1 * 2), true, row, lchk,
                           s_w3 + kt * (TN1 * 128) + (wave * 32 + j * 8) * 128);
        }
#pragma unroll
    for (int kt = 0; kt < TK2 / 64; ++kt)
#pragma unroll
        for (int h = 0; h < NA2; ++h) {
            const int row = (wave + 8 * h) * 8 + lrow;
            bneck_dma_rows(reinterpret_cast<const unsigned char*>(p.w1n) + (size_t)row * (TK2 * 2) + kt * 128, true, row, lchk,
                           s_w1 + kt * W1_KT + (wave + 8 * h) * 8 * 128);
        }
    // ---- per-tile DMA: y2 (CAT: and x) piece = rows 8 wave .. +7; residual pieces = rows 2 (4 wave + j) + (lane >> 5)
    auto stage_in = [&](int T, int slot) {
        const int row = wave * 8 + lrow;
        const int gm = T * TBM + row;
        bneck_dma_rows(y2g + (size_t)gm * (TK1 * 2), gm < p.M, row, lchk, s_a + slot * A_BYTES + wave * 1024);
        if constexpr (CAT)
            bneck_dma_rows(reinterpret_cast<const unsigned char*>(p.xs) + (size_t)gm * (TK1 * 2), gm < p.M, row, lchk,
                           s_a + slot * A_BYTES + TBM * 128 + wave * 1024);
    };
    auto stage_res = [&](int T, int slot) {
        bneck_dma_tile<512, 4>(s_r + slot * R_BYTES, wave, lane, [&](int, int row, int gch) {
            const int gm = T * TBM + row;
            return gm < p.M ? resg + ((size_t)gm * TN1 + gch * 8) * 2 : zsrc;
        });
    };
    // biases of this lane's output channels (fixed for the whole kernel)
    float b3v[4][4], b1v[NA2][4];
    bneck_bias<false>(b3v, p.b3, wn4 * 64 + fchunk * 4);
    if constexpr (CAT) bneck_bias<true>(b3v, p.bs, wn4 * 64 + fchunk * 4);
    bneck_bias<false>(b1v, p.b1n, wn4 * (CN / 4) + fchunk * 4);

    int T = blockIdx.x;
    if (T < ntiles) {
        stage_in(T, 0);
        if constexpr (RES_AHEAD) stage_res(T, 0);
    }
    wait_vmcnt<0>();
    wg_barrier();
    int slot = 0;
    for (; T < ntiles; T += G, slot ^= 1) {
        const int m0 = T * TBM;
        const bool has_next = T + G < ntiles;
        // this iteration's queue, oldest first: RES_OWN: 4 residual pieces of THIS tile, then the y2 prefetch (1 piece);
        // otherwise the next tile's 1 + 4 (CAT: 2) pieces; then, below, the tile's NST stores
        if constexpr (RES_OWN) stage_res(T, 0);
        if (has_next) {
            stage_in(T + G, slot ^ 1);
            if constexpr (RES_AHEAD) stage_res(T + G, slot ^ 1);
        }
        const unsigned char* sa = s_a + slot * A_BYTES;
        unsigned char* sr = s_r + (RES_AHEAD ? slot : 0) * R_BYTES;
        // ---- GEMM 1: 64 px x 256 ch, K = 64. Wave tile 32 px x 64 ch.
        f32x4_t acc[4][2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2 * NKT1; ++kk) {
            uint4 xf[2], wf[4];
#pragma unroll
            for (int b = 0; b < 2; ++b)
                xf[b] = *reinterpret_cast<const uint4*>(sa + (kk >> 1) * (TBM * 128) + lds_off(wm2 * 32 + b * 16 + frow, (kk & 1) * 4 + fchunk));
#pragma unroll
            for (int a = 0; a < 4; ++a)
                wf[a] = *reinterpret_cast<const uint4*>(s_w3 + (kk >> 1) * (TN1 * 128) + lds_off(wn4 * 64 + a * 16 + frow, (kk & 1) * 4 + fchunk));
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = Frag<lp16_t>::mma(wf[a], xf[b], acc[a][b]);
        }
        if constexpr (RES_OWN) {
            if (has_next) wait_vmcnt<1>();  // the residual pieces are older than the y2 prefetch
            else wait_vmcnt<0>();
            wg_barrier();                   // everybody's residual pieces are in the out tile
        }
        bneck_out_tile<!CAT, 512>(sr, acc, b3v, wm2 * 32 + frow, wn4 * 64 + fchunk * 4);
        wg_barrier();  // out tile complete; every read of the y2 tile done
        // drain the out tile: 2048 16-byte chunks, 4 per thread, whole 512-byte rows per 32 lanes
        bneck_drain<512, 4, 16, 0>(sr, tid >> 5, tid & 31, [&](int, int row, int gch, unsigned char*& g) {
            const int gm = m0 + row;
            g = reinterpret_cast<unsigned char*>(p.out) + ((size_t)gm * TN1 + gch * 8) * 2;
            return gm < p.M;
        });
        // ---- GEMM 2: 64 px x CN ch, K = 256, B operand straight from the out tile. Wave tile 32 px x CN/4 ch.
        f32x4_t acc2[NA2][2];
        bneck_gemm2<512, 0>(sr, wm2 * 32 + frow, fchunk, acc2, [&](int a, int ks) {
            return *reinterpret_cast<const uint4*>(s_w1 + (ks >> 1) * W1_KT + lds_off(wn4 * (CN / 4) + a * 16 + frow, (ks & 1) * 4 + fchunk));
        });
        // z tile: CN == 64 -> this tile's y2 slot (every wave finished reading it before the barrier above), 128-byte rows;
        //         CN == 128 -> over the out tile once every wave has finished reading it (drain + GEMM 2), 256-byte rows
        unsigned char* sz = CN == 64 ? s_a + slot * A_BYTES : sr;
        if constexpr (CN == 128) wg_barrier();
        bneck_z_tile<CN>(sz, acc2, b1v, wm2 * 32 + frow, wn4 * (CN / 4) + fchunk * 4);
        wg_barrier();  // z tile complete; every read of the out tile done
        bneck_drain<2 * CN, NA2, 0, 1>(sz, tid >> 3, (tid & 7) * NA2, [&](int, int row, int gch, unsigned char*& g) {
            const int gm = m0 + row;
            g = reinterpret_cast<unsigned char*>(p.z) + ((size_t)gm * CN + gch * 8) * 2;
            return gm < p.M;
        });
        // the prefetch DMA (issued in front of them) has landed once at most the NST stores above are still outstanding (a
        // ragged tile issues fewer, but it is the last tile of its workgroup: nothing is in flight then) ...
        wait_vmcnt<NST>();
        wg_barrier();  // ... and nobody still reads the z tile when the next tile's DMA lands on it
    }
}


// ---------------------------------------------------------------------------------------------------------------
// Layer-2 form: conv3 128 -> 512 + residual + ReLU, then the next block's conv1 512 -> 128 (32 x 16 maps, 131 072
// pixels per 256-frame step). The two weight matrices are 128 KB each -- they do not fit the LDS beside the tiles --
// but a wave only ever needs ITS output channels of them: with the eight waves splitting the channels (64 of conv3,
// 16 of the next conv1) each lane keeps its 16 + 16 MFMA weight fragments in 128 VGPRs for the whole kernel, and the
// LDS holds nothing but tiles: y2 (16 KB) and the residual / out tile (64 KB), both double-buffered = 160 KB.
// Per 64-pixel tile the kernel moves 160 KB of HBM traffic (y2, residual in; out, z out) for 2 x 64 MFMAs per wave:
// HBM-bound, like the layer-1 form.
constexpr int L2K1 = 128, L2N1 = 512, L2K2 = 512, L2N2 = 128;

__global__ __launch_bounds__(512) void bottleneck_tail_l2_kernel(const TailParams p, int ntiles) {
    constexpr int A_BYTES = 2 * TBM * 128;      // 16 KB: two 64-channel k-tiles of [64 rows][128 B]
    constexpr int R_BYTES = TBM * L2N1 * 2;     // 64 KB: 1024-byte rows, chunk c at c ^ (row & 31)
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * A_BYTES + 2 * R_BYTES];
    unsigned char* s_a = smem;
    unsigned char* s_r = smem + 2 * A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fchunk = lane >> 4;
    const int G = gridDim.x;
    const unsigned char* zsrc = reinterpret_cast<const unsigned char*>(&g_zero16);
    const unsigned char* y2g = reinterpret_cast<const unsigned char*>(p.y2);
    const unsigned char* resg = reinterpret_cast<const unsigned char*>(p.res);

    // ---- this wave's weight fragments, resident in registers: conv3 channels 64 wave + 16 a + frow, k = 32 kk + 8 fchunk;
    // next conv1 channel 16 wave + frow, k = 32 ks + 8 fchunk (the MFMA A operand: row = lane & 15, k-chunk = lane >> 4)
    uint4 w3f[4][4], w1f[1][16];
    bneck_wfrags(w3f, p.w3, wave * 64 + frow, L2K1, fchunk);
    bneck_wfrags(w1f, p.w1n, wave * 16 + frow, L2K2, fchunk);
    // biases: one value per lane (lane L: conv3 channel 64 wave + L, next conv1 channel 16 wave + (L & 15)), fetched
    // through the cross-lane network where they are used -- 2 registers instead of 20
    float b3l = p.b3[wave * 64 + lane];
    float b1l = p.b1n[wave * 16 + (lane & 15)];
    asm volatile("" : "+v"(b3l), "+v"(b1l));
    auto lane_bias = [&](float held, int src_lane) {
        return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(held)));
    };
    bneck_pin(w3f);
    bneck_pin(w1f);

    // ---- per-tile DMA: 2 y2 pieces (rows 8 wave .. +7 of both k-tiles) + 8 residual pieces (whole rows 8 wave + j)
    auto stage_tile = [&](int T, int slot) {
        const int m0 = T * TBM;
        int ln = lane;
        asm volatile("" : "+v"(ln));  // addresses are recomputed per tile: hoisted out of the loop they end up in scratch
        {
            const int row = wave * 8 + (ln >> 3);
            const int gm = m0 + row;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
                bneck_dma_rows(y2g + (size_t)gm * (L2K1 * 2) + kt * 128, gm < p.M, row, ln & 7, s_a + slot * A_BYTES + kt * (TBM * 128) + wave * 1024);
        }
        bneck_dma_tile<1024, 8>(s_r + slot * R_BYTES, wave, ln, [&](int, int row, int gch) {
            const int gm = m0 + row;
            return gm < p.M ? resg + (size_t)gm * (L2N1 * 2) + (gch << 4) : zsrc;
        });
    };

    int T = blockIdx.x;
    if (T < ntiles) stage_tile(T, 0);
    wait_vmcnt<0>();
    wg_barrier();
    int slot = 0;
    for (; T < ntiles; T += G, slot ^= 1) {
        const int m0 = T * TBM;
        if (T + G < ntiles) stage_tile(T + G, slot ^ 1);  // 10 DMA pieces at the head of this iteration's queue
        const unsigned char* sa = s_a + slot * A_BYTES;
        unsigned char* sr = s_r + slot * R_BYTES;
        // ---- GEMM 1: 64 px x 512 ch, K = 128. Wave tile 64 px x 64 ch, weights from registers; two passes of 32
        // channels (32 accumulator registers at a time beside the 128 weight registers), each followed by its
        // bias + residual (in place) + ReLU -> bf16 out tile
#pragma unroll
        for (int ah = 0; ah < 2; ++ah) {
            f32x4_t acc[2][4];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            uint4 xp[2][4];
            auto ld1 = [&](int kk, int b) {
                return *reinterpret_cast<const uint4*>(sa + (kk >> 1) * (TBM * 128) + lds_off(b * 16 + frow, (kk & 1) * 4 + fchunk));
            };
#pragma unroll
            for (int b = 0; b < 4; ++b) xp[0][b] = ld1(0, b);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (kk + 1 < 4) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) xp[(kk + 1) & 1][b] = ld1(kk + 1, b);
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = Frag<lp16_t>::mma(w3f[2 * ah + a][kk], xp[kk & 1][b], acc[a][b]);
                __builtin_amdgcn_sched_barrier(0);
            }
            float bv[2][4];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) bv[a][r] = lane_bias(b3l, (2 * ah + a) * 16 + fchunk * 4 + r);
            bneck_out_tile<true, 1024>(sr, acc, bv, frow, wave * 64 + 2 * ah * 16 + fchunk * 4);
        }
        wg_barrier();  // out tile complete; every read of the y2 tile done
        // drain the out tile: 4096 16-byte chunks, 8 per thread, one whole 1024-byte row per wave instruction
        int ld = lane, td = tid;
        asm volatile("" : "+v"(ld), "+v"(td));  // store addresses recomputed per tile (see stage_tile)
        bneck_drain<1024, 8, 8, 0>(sr, wave, ld, [&](int, int row, int gch, unsigned char*& g) {
            const int gm = m0 + row;
            g = reinterpret_cast<unsigned char*>(p.out) + ((size_t)gm * L2N1 + gch * 8) * 2;
            return gm < p.M;
        });
        // ---- GEMM 2: 64 px x 128 ch, K = 512, B operand straight from the out tile. Wave tile 64 px x 16 ch.
        f32x4_t acc2[1][4];
        bneck_gemm2<1024, 1>(sr, frow, fchunk, acc2, [&](int a, int ks) { return w1f[a][ks]; });
        // z tile (64 px x 128 ch, 256-byte rows) over this tile's y2 slot
        unsigned char* sz = s_a + slot * A_BYTES;
        float b1v[1][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) b1v[0][r] = lane_bias(b1l, fchunk * 4 + r);
        bneck_z_tile<L2N2>(sz, acc2, b1v, frow, wave * 16 + fchunk * 4);
        wg_barrier();  // z tile complete; every read of the out tile done
        bneck_drain<256, 2, 32, 0>(sz, td >> 4, td & 15, [&](int, int row, int gch, unsigned char*& g) {
            const int gm = m0 + row;
            g = reinterpret_cast<unsigned char*>(p.z) + ((size_t)gm * L2N2 + gch * 8) * 2;
            return gm < p.M;
        });
        // the next tile's DMA (issued first) has landed once at most the 10 stores above are still outstanding (a ragged
        // tile issues fewer, but it is the last tile of its workgroup: nothing is in flight then)
        wait_vmcnt<10>();
        wg_barrier();
    }
}

}  // namespace

extern "C" int agrl_bottleneck_tail(const void* y2, const void* w3, const float* b3, const void* residual,
                                    const void* x_short, const void* w_short, const float* b_short, void* out,
                                    const void* w1_next, const float* b1_next, void* z, int M, int Cmid, int Cout,
                                    int Cnext, int Cshort, agrl_stream_t stream) {
    static const char* who = "agrl_bottleneck_tail";
    if (int e = bneck_check_operands(who, {y2, w3, b3, out, w1_next, b1_next, z}, residual, x_short, w_short, b_short)) return e;
    AGRL_CHECK_ARG(M > 0, "agrl_bottleneck_tail: empty problem");
    const bool layer2 = Cmid == L2K1 && Cout == L2N1 && Cnext == L2N2 && !x_short;
    AGRL_CHECK_ARG(layer2 || (Cmid == TK1 && Cout == TN1 && (Cnext == TN2 || (Cnext == 128 && !x_short)) && (!x_short || Cshort == TK1)),
                   "agrl_bottleneck_tail: built for Cmid=64, Cout=256, Cnext=64 (128 without downsample), Cshort=64 "
                   "(layer 1) and Cmid=128, Cout=512, Cnext=128 without downsample (layer 2), got %d/%d/%d/%d", Cmid, Cout, Cnext, Cshort);
    if (int e = bneck_check_aligned(who, {y2, w3, b3, residual, out, w1_next, b1_next, z, x_short, w_short, b_short})) return e;
    TailParams p;
    p.y2 = y2; p.w3 = w3; p.b3 = b3; p.res = residual; p.out = out; p.w1n = w1_next; p.b1n = b1_next; p.z = z; p.M = M;
    p.xs = x_short; p.ws = w_short; p.bs = b_short;
    const int ntiles = cdiv(M, TBM);
    const int grid = bneck_grid(ntiles);
    if (layer2) hipLaunchKernelGGL(bottleneck_tail_l2_kernel, dim3(grid), dim3(512), 0, (hipStream_t)stream, p, ntiles);
    else if (Cnext == 128) hipLaunchKernelGGL((bottleneck_tail_kernel<false, 128>), dim3(grid), dim3(512), 0, (hipStream_t)stream, p, ntiles);
    else if (x_short) hipLaunchKernelGGL((bottleneck_tail_kernel<true, 64>), dim3(grid), dim3(512), 0, (hipStream_t)stream, p, ntiles);
    else hipLaunchKernelGGL((bottleneck_tail_kernel<false, 64>), dim3(grid), dim3(512), 0, (hipStream_t)stream, p, ntiles);
    AGRL_CHECK_LAUNCH("agrl_bottleneck_tail");
    return 0;
}
