// What the stems share. stem_shape (host) sizes the launch of all three -- stem.hip, stem_mfma.hip, stem_split16.hip; namespace
// stem8 is the device side of the two MFMA-structured ones (stem_mfma.hip: one 16-bit MFMA per product; stem_split16.hip: three fp16
// MFMAs on fp16 high / low halves), which differ from the LDS write of the patch on and are the same before it: one 512-thread
// workgroup -> an 8x8 tile of POOLED pixels x 64 channels of one frame, the 39x40x4 input patch of the NEXT tile prefetched into
// registers, the packed weights resident in LDS. See stem_mfma.hip's header for the K = 7 x 32 contraction both run.
// Namespace stem_rp (end of this file) is the geometry of stem_mfma.hip's register-pool form, which reuses the prefetch and the weight DMA.
#pragma once
#include "agrl_common.h"
#include "frames_u8.h"

// ---- host: output / tile arithmetic of conv 7x7/2 pad 3 + maxpool 3x3/2 pad 1 over pt_h x pt_w tiles of pooled pixels ----------
struct StemShape {
    int CH, CW;            // conv map
    int PH, PW;            // pooled map
    int tiles_h, tiles_w;  // tiles per frame
    int grid;              // tiles of all frames
};

// non-zero (error set) for a shape no stem takes; null-pointer and alignment checks stay with each launcher's own arguments
static inline int stem_shape(const char* who, int N, int H, int W, int pt_h, int pt_w, StemShape* s) {
    AGRL_CHECK_ARG(N > 0 && H >= 7 && W >= 7, "%s: bad shape N=%d H=%d W=%d", who, N, H, W);
    s->CH = (H + 6 - 7) / 2 + 1, s->CW = (W + 6 - 7) / 2 + 1;
    s->PH = (s->CH + 2 - 3) / 2 + 1, s->PW = (s->CW + 2 - 3) / 2 + 1;
    s->tiles_h = cdiv(s->PH, pt_h), s->tiles_w = cdiv(s->PW, pt_w);
    const long long grid = (long long)N * s->tiles_h * s->tiles_w;
    AGRL_CHECK_ARG(grid < (1ll << 31), "%s: grid too large", who);
    s->grid = (int)grid;
    return 0;
}

namespace stem8 {
constexpr int PT = 8;                 // pooled tile edge
constexpr int CT = 2 * PT + 1;        // conv tile edge 17
constexpr int NPOS = CT * CT;         // 289
constexpr int NFRAG = (NPOS + 15) / 16;  // 19
constexpr int NWV = 8;                // waves per workgroup
constexpr int NTH = 64 * NWV;
constexpr int FPW = (NFRAG + NWV - 1) / NWV;  // position fragments per wave: 3
constexpr int IT = 2 * (CT - 1) + 7;  // input patch edge 39
constexpr int PWP = 40;               // padded patch width (pixels)
constexpr int PATCH_BYTES = IT * PWP * 8;      // 12480: [y][x][4] 16-bit elements (3 channels + a zero)
constexpr int NPASS = (IT * PWP + NTH - 1) / NTH;  // patch pixels per thread: 4
// 7*32 bf16 = 448 + 32 pad = 30 sixteen-byte slots per row. A ds_read_b128 is served in groups of 16 lanes: rows
// (lane & 15) 0-3, 12-15 at k-chunk g with rows 4-11 at k-chunk g + 1; 30 r mod 16 sends the first set to the even slots and
// the second (+1) to the odd ones: conflict-free (29 slots, the "odd stride" choice, collides on five of sixteen)
constexpr int WROW_BYTES = 480;
constexpr int W_BYTES = 64 * WROW_BYTES;       // 30720 = 30 KiB

// linear tile index -> frame, pooled origin, conv origin (first conv row / column of the tile; -1 on the top / left image border)
struct Tile {
    int n, ph0, pw0, cr0, cc0;
};
__device__ __forceinline__ Tile tile_at(int T, int tiles_w, int tiles_hw) {
    Tile t;
    t.n = T / tiles_hw;
    const int trem = T - t.n * tiles_hw;
    t.ph0 = (trem / tiles_w) * PT, t.pw0 = (trem % tiles_w) * PT;
    t.cr0 = 2 * t.ph0 - 1, t.cc0 = 2 * t.pw0 - 1;
    return t;
}

// The patch prefetch: one pixel (3 channels) per thread per pass, in registers from the request to the LDS write one tile later.
// TIN = unsigned char (uint8 frames, EX = one trailing FramesU8): load() requests the pixels' BYTES where the fp32 form requests
// floats, and normalize() turns them into the normalised fp32 values one phase later -- a gather from the 3 KB table (L1-resident),
// which a kernel issues once the bytes have had an MFMA sweep to land. From pv on the two forms are the same code on the same values.
// Geometry: a patch of IT_ rows x PWP_ pixels (the first PWV_ of a row are fetched, the rest are padding) over NTH_ threads; the
// patch's first pixel is input pixel (2 t.cr0 - 3, 2 t.cc0 - 3) of frame t.n.
template <int IT_, int PWP_, int PWV_, int NTH_, typename TIN, typename... EX>
struct PatchPrefetchT {
    static constexpr bool U8 = sizeof...(EX) != 0;
    static constexpr int IT = IT_, PWP = PWP_, NTH = NTH_;
    static constexpr int NPASS = (IT_ * PWP_ + NTH_ - 1) / NTH_;  // patch pixels per thread
    uint32_t pb[U8 ? NPASS : 1][3];  // uint8 frames: the raw bytes, FRAMES_U8_PAD (the table's zero entry) outside the frame
    float pv[NPASS][3];              // the pixels as the patch write takes them

    // all loads of all passes are issued together
    __device__ __forceinline__ void load(const TIN* __restrict__ x, int H, int W, const Tile& t, EX... ex) {
        const int iy0 = 2 * t.cr0 - 3, ix0 = 2 * t.cc0 - 3;
        const TIN* xn = x + (size_t)t.n * 3 * H * W;
        int td = threadIdx.x;
        asm volatile("" : "+v"(td));  // per-tile address arithmetic (hoisted out of the tile loop it costs 100 registers)
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int e = td + NTH * i;
            const int py = e / PWP, px = e - py * PWP;
            const int iy = iy0 + py, ix = ix0 + px;
            if constexpr (U8) {
                const FramesU8 u8 = frames_u8_of(ex...);
                pb[i][0] = pb[i][1] = pb[i][2] = FRAMES_U8_PAD;
                if (e < IT * PWP && px < PWV_ && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                    const uint32_t o = (uint32_t)(iy * W + ix) * u8.pixel_stride;   // inside one frame: < 3 H W < 2^31 (frames_u8_args)
                    pb[i][0] = xn[o];
                    pb[i][1] = xn[o + (uint32_t)u8.channel_stride];
                    pb[i][2] = xn[o + 2 * (uint32_t)u8.channel_stride];
                }
            } else {
                pv[i][0] = pv[i][1] = pv[i][2] = 0.f;
                if (e < IT * PWP && px < PWV_ && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                    const size_t o = (size_t)iy * W + ix;
                    pv[i][0] = xn[o];
                    pv[i][1] = xn[(size_t)H * W + o];
                    pv[i][2] = xn[2 * (size_t)H * W + o];
                }
            }
        }
    }
    // uint8 frames: bytes -> table values (the fp32 form's pv); nothing to do for fp32 frames
    __device__ __forceinline__ void normalize(EX... ex) {
        if constexpr (U8) {
            const FramesU8 u8 = frames_u8_of(ex...);
#pragma unroll
            for (int i = 0; i < NPASS; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) pv[i][c] = u8.table[c * FRAMES_U8_ROW + pb[i][c]];
        }
    }
};
template <typename TIN, typename... EX>
using PatchPrefetch = PatchPrefetchT<IT, PWP, IT, NTH, TIN, EX...>;  // the 8x8 tile's 39 x 40 patch over 512 threads

// byte offset, at filter row 0, of this lane's 16-byte patch slice for each of its wave's position fragments
// (frow = lane & 15: position inside the fragment, g = lane >> 4: k-chunk)
__device__ __forceinline__ void patch_frag_offsets(int wave, int frow, int g, int (&a_off)[FPW]) {
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
        int pos = (wave + NWV * i) * 16 + frow;
        pos = pos < NPOS ? pos : NPOS - 1;
        const int cy = pos / CT, cx = pos - cy * CT;
        a_off[i] = ((2 * cy) * PWP + 2 * cx + 2 * g) * 8;
    }
}

// conv-tile row of position p: p with bits 0 and 1 swapped (the kernels' conv-tile comments say what the pooling reads gain)
__device__ __forceinline__ int ct_row(int pos) { return (pos & ~3) | ((pos & 1) << 1) | ((pos >> 1) & 1); }

// one packed weight block (64 rows x WROW_BYTES) -> LDS: 30 one-KiB DMA pieces, contiguous, over the workgroup's waves. The DMA is
// invisible to the compiler: s_waitcnt vmcnt(0) + a barrier before the first read
__device__ __forceinline__ void weights_to_lds(const unsigned char* __restrict__ wpk, unsigned char* s_w, int wave, int lane,
                                               int nwv = NWV) {
    for (int piece = wave; piece < W_BYTES / 1024; piece += nwv)
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(wpk + piece * 1024 + lane * 16), (lds_void_t*)(s_w + piece * 1024), 16, 0, 0);
}
}  // namespace stem8

// ---- the register-pool form of the 16-bit stem (stem_mfma.hip: stem_regpool_kernel) ------------------------------------------
// One 256-thread workgroup -> RT pooled rows x the WHOLE pooled width (at most 16 NG columns) x 64 channels of one frame. A position
// fragment of the MFMA is 16 adjacent pooled columns of one conv row at one column phase (conv column 2 px or 2 px + 1), so a lane's
// accumulators are conv positions of its own pooled pixel; a wave walks RPW pooled rows down and carries the last conv row.
namespace stem_rp {
constexpr int RT = 8;                   // pooled rows per tile
constexpr int NWV = 4;                  // waves per workgroup
constexpr int NTH = 64 * NWV;
constexpr int RPW = RT / NWV;           // pooled rows per wave: 2 (conv rows 4 w .. 4 w + 4 of the tile's 17)
constexpr int NG = 2;                   // 16-column groups per pooled row
constexpr int MAX_PW = 16 * NG;         // widest pooled row the form takes
constexpr int MIN_PW = 16 * (NG - 1) + 1;  // narrower rows leave a whole group idle: the conv-tile kernel takes them
constexpr int IT = 4 * RT + 7;          // input rows of a tile: 39
constexpr int PWP = 4 * MAX_PW + 6;     // input pixels of a row: 134 (conv columns 0 .. 63, 7 taps + the pad pixel of the k-step)
constexpr int ROW_BYTES = PWP * 8;      // 1072 = 67 x 16
constexpr int PATCH_BYTES = IT * ROW_BYTES;  // 41808
constexpr int EDGE_BYTES = NWV * (2 * RPW + 1) * 256;  // group 0 -> group 1 hand-over of the 5 conv rows of each wave: 5120
static_assert(RPW == 2 && NG == 2 && RT % NWV == 0 && ROW_BYTES % 16 == 0, "stem_rp geometry (the kernel's strip walk is written for 2 x 2)");

__device__ __forceinline__ stem8::Tile tile_at(int T, int tiles_h) {
    stem8::Tile t;
    t.n = T / tiles_h;
    t.ph0 = (T - t.n * tiles_h) * RT, t.pw0 = 0;
    t.cr0 = 2 * t.ph0 - 1, t.cc0 = 0;   // conv row -1 heads the first tile's patch (never pooled); conv column -1 is not computed
    return t;
}
template <typename TIN, typename... EX>
using PatchPrefetch = stem8::PatchPrefetchT<IT, PWP, PWP, NTH, TIN, EX...>;
}  // namespace stem_rp
