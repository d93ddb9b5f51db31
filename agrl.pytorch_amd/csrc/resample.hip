// Resize / crop / flip of uint8 channel-last frames on the device, bit-exact with Pillow's Image.crop().resize(size, BILINEAR): the
// rest of the reference's input pipeline (GroupResize, GroupRandomCrop, GroupMisAlignAugment, GroupRandomHorizontalFlip,
// train_vidreid_xent_htri.py:192-217) in front of the stems, which already normalise uint8 frames themselves.
//
// Per frame the host hands over eight ints (src_h, src_w, y0, x0, win_h, win_w, flip, 0): the window [y0, y0+win_h) x [x0, x0+win_w) of
// the frame's valid extent is an image of its own (coordinates outside the extent replicate the nearest edge), resampled to OH x OW in
// Pillow's two integer passes -- horizontal, rounded to uint8, then vertical -- and mirrored if flip is set. The filter taps are Pillow's
// (ImagingResample's precompute_coeffs + normalize_coeffs_8bpc, triangle filter): computed in fp64 and stored as int(0.5 + w 2^22); each
// pass is (2^21 + sum(pixel * k)) >> 22 in int32, clamped to 0..255.
//
// One workgroup per TR x TW output tile of one frame:
//   1. TW + TR threads derive the tile's horizontal / vertical taps from the geometry into LDS (no host tables: nothing on the host
//      depends on the sizes, so ragged batches need no per-shape state and the launch is capturable)
//   2. the window rows the tile's vertical taps reach are staged STAGE_ROWS at a time -- aligned dwords of the source row segment as
//      dword loads, the unaligned head / tail bytewise, never a byte outside the valid extent -- and resampled horizontally into a
//      uint8 LDS tile
//   3. the tile is resampled vertically out of LDS and stored: whole dwords wherever an aligned dword lies inside the tile's row
//      segment, single bytes at a ragged head / tail
// Every index is clamped (source coordinates to the valid extent, tap counts to TAPS, row / column spans to the LDS capacity), so no
// geometry content can make the kernel read or write out of bounds; geometry the host wrapper would reject gives defined garbage.
#include "agrl_common.h"

namespace {
constexpr int NTH = 256;
constexpr int TAPS = 17;                          // taps per output element: a downscale of up to 8 per axis
constexpr int MAX_SCALE = 8;
constexpr int MAX_OUT = 512;
constexpr int PRECISION_BITS = 22;                // Pillow's, for 8-bit channels
constexpr int TR = 16, TW = 64;                   // output tile
constexpr int MAX_ROWS = (TR - 1) * MAX_SCALE + TAPS;   // 137 window rows under one tile
constexpr int SEG = (TW - 1) * MAX_SCALE + TAPS;        // 521 source pixels of a row under one tile
constexpr int SEG_STRIDE = (3 + SEG * 3 + 3) / 4 * 4;   // staged row: the segment behind its pointer's phase (0..3), whole dwords
constexpr int STAGE_ROWS = 8;
constexpr int OUT_DW = (3 + TW * 3 + 3) / 4;            // dwords that cover one output row segment at any phase

// The tap arithmetic must round as the host's C / numpy fp64 does: no fused multiply-add, no fast-math (none is on the command line).
#pragma clang fp contract(off)

__device__ __forceinline__ double tap_weight(int j, double center, double fs) {
    double t = ((double)j - center + 0.5) / fs;
    t = t < 0.0 ? -t : t;
    return t < 1.0 ? 1.0 - t : 0.0;
}

// Taps of output element i of an in -> out axis: k[t * kstride], t = 0..TAPS-1 (zero behind count), first tap lo, count in 1..TAPS.
__device__ __forceinline__ void resample_taps_1d(int in, int out, int i, int* __restrict__ k, int kstride, int* lo_out, int* count_out) {
    if (in == out) {   // Pillow skips the pass
        for (int t = 0; t < TAPS; ++t) k[t * kstride] = t == 0 ? 1 << PRECISION_BITS : 0;
        *lo_out = i;
        *count_out = 1;
        return;
    }
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double center = ((double)i + 0.5) * scale;
    const double lo_d = center - fs + 0.5, hi_d = center + fs + 0.5;   // compared as doubles first: a cast never leaves int's range
    int lo = lo_d < 0.0 ? 0 : (lo_d < (double)in ? (int)lo_d : in);
    const int hi = hi_d < (double)in ? (int)hi_d : in;
    lo = lo > in - 1 ? in - 1 : lo;
    int count = hi - lo;
    count = count < 1 ? 1 : (count > TAPS ? TAPS : count);
    double total = 0.0;
    for (int t = 0; t < count; ++t) total = total + tap_weight(lo + t, center, fs);
    for (int t = 0; t < TAPS; ++t) {
        int v = 0;
        if (t < count && total > 0.0) v = (int)(0.5 + (tap_weight(lo + t, center, fs) / total) * (double)(1 << PRECISION_BITS));
        k[t * kstride] = v;
    }
    *lo_out = lo;
    *count_out = count;
}

__global__ __launch_bounds__(NTH) void resample_taps_kernel(int in, int out, int* __restrict__ k_out, int* __restrict__ bounds_out) {
    const int i = blockIdx.x * NTH + threadIdx.x;
    if (i >= out) return;
    int lo, count;
    resample_taps_1d(in, out, i, k_out + (size_t)i * TAPS, 1, &lo, &count);
    bounds_out[2 * i] = lo;
    bounds_out[2 * i + 1] = count;
}

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }
__device__ __forceinline__ int clip8(int acc) {
    acc >>= PRECISION_BITS;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

__global__ __launch_bounds__(NTH) void clip_resample_kernel(const unsigned char* __restrict__ src, const int* __restrict__ geometry,
                                                            unsigned char* __restrict__ out, int Hs, int Ws, int OH, int OW, int tiles_x,
                                                            int tiles) {
    __shared__ int s_hk[TAPS * TW], s_hlo[TW], s_hcnt[TW];   // taps tap-major: a wave reads consecutive columns
    __shared__ int s_vk[TAPS * TR], s_vlo[TR], s_vcnt[TR];
    __shared__ int s_phase[STAGE_ROWS];
    __shared__ __attribute__((aligned(16))) unsigned char s_stage[STAGE_ROWS * SEG_STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[MAX_ROWS * TW * 3];

    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int r0 = (tile / tiles_x) * TR, c0 = (tile % tiles_x) * TW;
    const int th = OH - r0 < TR ? OH - r0 : TR, tw = OW - c0 < TW ? OW - c0 : TW;
    unsigned char* out_tile = out + (((size_t)n * OH + r0) * OW + c0) * 3;

    const int* g = geometry + (size_t)n * 8;
    const int src_h = g[0] < Hs ? g[0] : Hs, src_w = g[1] < Ws ? g[1] : Ws;
    const long long y0 = g[2], x0 = g[3];
    const int win_h = g[4] < 1 ? 1 : g[4], win_w = g[5] < 1 ? 1 : g[5];
    const bool flip = g[6] != 0;
    if (src_h < 1 || src_w < 1) {   // no valid byte to read (the host wrapper refuses this): a defined output, nothing read
        for (int i = tid; i < th * tw * 3; i += NTH) out_tile[(size_t)(i / (tw * 3)) * OW * 3 + i % (tw * 3)] = 0;
        return;
    }

    // 1. taps. The LDS tile holds UNFLIPPED columns u0 .. u0+tw-1; a flipped frame's output columns c0 .. c0+tw-1 are those, mirrored.
    const int u0 = flip ? OW - c0 - tw : c0;
    if (tid < tw)
        resample_taps_1d(win_w, OW, u0 + tid, s_hk + tid, TW, s_hlo + tid, s_hcnt + tid);
    else if (tid >= TW && tid < TW + th)
        resample_taps_1d(win_h, OH, r0 + (tid - TW), s_vk + (tid - TW), TR, s_vlo + (tid - TW), s_vcnt + (tid - TW));
    __syncthreads();

    // window rows / columns under the tile (lo and lo + count grow with the output index), cut to what LDS holds
    const int ylo = s_vlo[0];
    int nrows = s_vlo[th - 1] + s_vcnt[th - 1] - ylo;
    nrows = nrows < 1 ? 1 : (nrows > MAX_ROWS ? MAX_ROWS : nrows);
    const int sa = clampi(x0 + s_hlo[0], 0, src_w - 1);
    int sb = clampi(x0 + s_hlo[tw - 1] + s_hcnt[tw - 1] - 1, 0, src_w - 1);
    sb = sb < sa ? sa : (sb > sa + SEG - 1 ? sa + SEG - 1 : sb);
    const int seg_bytes = (sb - sa + 1) * 3;
    const int seg_dw = (3 + seg_bytes + 3) / 4;   // dwords that cover the segment at any phase

    // 2. stage source rows, resample them horizontally into s_tile
    for (int rb = 0; rb < nrows; rb += STAGE_ROWS) {
        const int rows_here = nrows - rb < STAGE_ROWS ? nrows - rb : STAGE_ROWS;
        for (int item = tid; item < rows_here * seg_dw; item += NTH) {
            const int q = item / seg_dw, d = item % seg_dw;
            const int sy = clampi(y0 + ylo + rb + q, 0, src_h - 1);
            const unsigned char* row = src + ((size_t)sy * Ws + sa) * 3 + (size_t)n * Hs * Ws * 3;
            const int phase = (int)((uintptr_t)row & 3);
            const unsigned char* gp = row - phase + 4 * d;     // aligned; only bytes [phase, phase + seg_bytes) of the cover are read
            unsigned char* lp = s_stage + q * SEG_STRIDE + 4 * d;
            if (d == 0) s_phase[q] = phase;
            if (4 * d >= phase && 4 * d + 4 <= phase + seg_bytes) {
                *reinterpret_cast<uint32_t*>(lp) = *reinterpret_cast<const uint32_t*>(gp);
            } else {
                for (int b = 0; b < 4; ++b)
                    if (4 * d + b >= phase && 4 * d + b < phase + seg_bytes) lp[b] = gp[b];
            }
        }
        __syncthreads();
        for (int item = tid; item < rows_here * tw * 3; item += NTH) {
            const int q = item / (tw * 3), rem = item % (tw * 3);
            const int col = rem / 3, ch = rem % 3;
            const unsigned char* px = s_stage + q * SEG_STRIDE + s_phase[q] + ch;
            const int lo = s_hlo[col], cnt = s_hcnt[col];
            int acc = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < cnt; ++t) acc += s_hk[t * TW + col] * (int)px[(clampi(x0 + lo + t, sa, sb) - sa) * 3];
            s_tile[((rb + q) * TW + col) * 3 + ch] = (unsigned char)clip8(acc);
        }
        __syncthreads();
    }

    // 3. vertical pass out of s_tile; one aligned dword of an output row segment per thread and step
    for (int item = tid; item < th * OUT_DW; item += NTH) {
        const int r = item / OUT_DW, d = item % OUT_DW;
        unsigned char* orow = out_tile + (size_t)r * OW * 3;
        const int phase = (int)((uintptr_t)orow & 3);
        if (4 * d >= phase + tw * 3) continue;
        const int lo = s_vlo[r] - ylo, cnt = s_vcnt[r];
        uint32_t word = 0;
        int nvalid = 0;
        for (int b = 0; b < 4; ++b) {
            const int off = 4 * d + b - phase;   // byte of the row segment
            if (off < 0 || off >= tw * 3) continue;
            const int col = off / 3, ch = off % 3;
            const unsigned char* px = s_tile + (flip ? tw - 1 - col : col) * 3 + ch;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < cnt; ++t) acc += s_vk[t * TR + r] * (int)px[clampi(lo + t, 0, nrows - 1) * TW * 3];
            word |= (uint32_t)clip8(acc) << (8 * b);
            ++nvalid;
        }
        unsigned char* op = orow - phase + 4 * d;
        if (nvalid == 4) {
            *reinterpret_cast<uint32_t*>(op) = word;
        } else {
            for (int b = 0; b < 4; ++b) {
                const int off = 4 * d + b - phase;
                if (off >= 0 && off < tw * 3) op[b] = (unsigned char)(word >> (8 * b));
            }
        }
    }
}
}  // namespace

extern "C" int agrl_clip_resample_u8(const unsigned char* x, const int* geometry, unsigned char* out, int N, int Hs, int Ws, int OH, int OW,
                                     agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && geometry && out, "agrl_clip_resample_u8: null pointer");
    AGRL_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0, "agrl_clip_resample_u8: bad shape N=%d Hs=%d Ws=%d", N, Hs, Ws);
    AGRL_CHECK_ARG(OH >= 1 && OH <= MAX_OUT && OW >= 1 && OW <= MAX_OUT, "agrl_clip_resample_u8: output size %dx%d, 1..%d each", OH, OW,
                   MAX_OUT);
    const int tiles_x = (OW + TW - 1) / TW, tiles = tiles_x * ((OH + TR - 1) / TR);
    AGRL_CHECK_ARG((long long)N * tiles <= 0x7fffffffLL, "agrl_clip_resample_u8: N=%d frames of %d tiles exceed the grid", N, tiles);
    hipLaunchKernelGGL(clip_resample_kernel, dim3((unsigned)(N * tiles)), dim3(NTH), 0, (hipStream_t)stream, x, geometry, out, Hs, Ws, OH,
                       OW, tiles_x, tiles);
    AGRL_CHECK_LAUNCH("agrl_clip_resample_u8");
    return 0;
}

extern "C" int agrl_resample_taps_u8(int in, int out, int* k_out, int* bounds_out, agrl_stream_t stream) {
    AGRL_CHECK_ARG(k_out && bounds_out, "agrl_resample_taps_u8: null pointer");
    AGRL_CHECK_ARG(in >= 1 && in <= (1 << 30) && out >= 1 && out <= (1 << 20), "agrl_resample_taps_u8: bad sizes in=%d out=%d", in, out);
    hipLaunchKernelGGL(resample_taps_kernel, dim3((unsigned)((out + NTH - 1) / NTH)), dim3(NTH), 0, (hipStream_t)stream, in, out, k_out,
                       bounds_out);
    AGRL_CHECK_LAUNCH("agrl_resample_taps_u8");
    return 0;
}
