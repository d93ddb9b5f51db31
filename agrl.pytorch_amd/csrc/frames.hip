// uint8 frames -> normalised fp32 NCHW frames: the reference's transform_test (ToTensor + Normalize, train_vidreid_xent_htri.py:214-217)
// for the paths that do not fuse it into the stem -- the native train step (its stem reads fp32 through agrl_im2col_rows) and any caller
// that wants the tensor. A streaming kernel: the 3 KB table sits in LDS, a thread turns four bytes into one 16-byte store (frames whose
// H W is a multiple of four, aligned pointers) or one byte into one float (anything else). Not on the eval hot path.
// agrl_frames_normalize_erase_u8 is the same pass with the reference's random erasing in it (second half of this file).
#include "agrl_common.h"
#include "frames_u8.h"

namespace {
constexpr int NTH = 256;

__device__ __forceinline__ void stage_table(float* s_tab, const float* __restrict__ table) {
    for (int i = threadIdx.x; i < 3 * FRAMES_U8_ROW; i += NTH) s_tab[i] = table[i];
    __syncthreads();
}

// NHWC = false: group g = elements 4g .. 4g+3 of the (N,3,H,W) tensor (one channel: H W % 4 == 0), in and out at the same index.
// NHWC = true:  group g = pixels 4g .. 4g+3 of the (N,H,W) grid: 12 bytes in, one float4 per channel plane out.
template <bool NHWC>
__global__ __launch_bounds__(NTH) void frames_normalize_vec4_kernel(const uint32_t* __restrict__ x, const float* __restrict__ table,
                                                                    float* __restrict__ out, long long ngroups, int HW) {
    __shared__ float s_tab[3 * FRAMES_U8_ROW];
    stage_table(s_tab, table);
    for (long long g = (long long)blockIdx.x * NTH + threadIdx.x; g < ngroups; g += (long long)gridDim.x * NTH) {
        if constexpr (!NHWC) {
            const uint32_t u = x[g];
            const float* t = s_tab + (int)((4 * g / HW) % 3) * FRAMES_U8_ROW;
            *reinterpret_cast<float4*>(out + 4 * g) = make_float4(t[u & 255], t[(u >> 8) & 255], t[(u >> 16) & 255], t[u >> 24]);
        } else {
            const uint32_t u0 = x[3 * g], u1 = x[3 * g + 1], u2 = x[3 * g + 2];   // bytes p0c0 p0c1 p0c2 p1c0 | p1c1 p1c2 p2c0 p2c1 | p2c2 p3c0 p3c1 p3c2
            const long long n = 4 * g / HW;
            float* o = out + n * 3 * HW + (4 * g - n * HW);
            const float* t0 = s_tab;
            const float* t1 = s_tab + FRAMES_U8_ROW;
            const float* t2 = s_tab + 2 * FRAMES_U8_ROW;
            *reinterpret_cast<float4*>(o) = make_float4(t0[u0 & 255], t0[u0 >> 24], t0[(u1 >> 16) & 255], t0[(u2 >> 8) & 255]);
            *reinterpret_cast<float4*>(o + HW) = make_float4(t1[(u0 >> 8) & 255], t1[u1 & 255], t1[u1 >> 24], t1[(u2 >> 16) & 255]);
            *reinterpret_cast<float4*>(o + 2 * (long long)HW) = make_float4(t2[(u0 >> 16) & 255], t2[(u1 >> 8) & 255], t2[u2 & 255], t2[u2 >> 24]);
        }
    }
}

// one OUTPUT element (n, c, p) per thread and step: any size, any alignment
template <bool NHWC>
__global__ __launch_bounds__(NTH) void frames_normalize_kernel(const unsigned char* __restrict__ x, const float* __restrict__ table,
                                                               float* __restrict__ out, long long total, int HW) {
    __shared__ float s_tab[3 * FRAMES_U8_ROW];
    stage_table(s_tab, table);
    for (long long i = (long long)blockIdx.x * NTH + threadIdx.x; i < total; i += (long long)gridDim.x * NTH) {
        const long long nc = i / HW;
        const int c = (int)(nc % 3);
        const long long src = NHWC ? ((nc / 3) * HW + (i - nc * HW)) * 3 + c : i;
        out[i] = s_tab[c * FRAMES_U8_ROW + x[src]];
    }
}

// ---- normalise + random erasing (agrl_frames_normalize_erase_u8) ----------------------------------------------------------------------
// The reference's GroupRandomErasing runs behind Normalize and writes a constant per channel into the normalised tensor, so it belongs
// to this pass: out = fill[c] inside any of the frame's rectangles, table[c][x] elsewhere. One workgroup = one chunk of ONE frame, so the
// frame's rectangle list (at most ERASE_MAX_RECTS rows of y, x, h, w) sits in LDS beside the table and every lane reads the same row of
// it (a broadcast). A thread owns PIX consecutive pixels of the frame in all three channels: PIX = 4 is the vectorised form (four bytes
// in and one 16-byte store out per channel plane, or 12 bytes in for channel-last frames), PIX = 1 the element-wise one. A rectangle or
// a count never forms an address: counts are clamped to the list's capacity, rectangles are only compared with the pixel's own (y, x).
// The list loop is what the kernel costs beyond the stream (a frame the reference erases carries ~95 rectangles), so where the thread's
// pixels share a row -- always when W % PIX == 0 -- a rectangle is one row test and one clamped column interval -> PIX bits at once.
constexpr int ERASE_MAX_RECTS = 128;
constexpr int ERASE_STEPS = 4;   // units (PIX pixels) per thread: a workgroup covers NTH * ERASE_STEPS units of its frame

template <bool NHWC, int PIX>
__global__ __launch_bounds__(NTH) void frames_normalize_erase_kernel(const unsigned char* __restrict__ x, const float* __restrict__ table,
                                                                     const int* __restrict__ rects, const int* __restrict__ counts,
                                                                     int max_rects, float fill0, float fill1, float fill2,
                                                                     float* __restrict__ out, int HW, int W, int units, int chunks) {
    __shared__ float s_tab[3 * FRAMES_U8_ROW];
    __shared__ __attribute__((aligned(16))) int s_rect[4 * ERASE_MAX_RECTS];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    int cnt = 0;
    if (max_rects > 0) {
        cnt = counts[n];
        cnt = cnt < 0 ? 0 : (cnt > max_rects ? max_rects : cnt);
    }
    const int* list = rects + (size_t)n * max_rects * 4;
    for (int i = tid; i < 4 * cnt; i += NTH) {   // entries cut to +-2^29 (a frame has fewer pixels), sizes to 0 .. 2^29: the differences
        const int v = list[i];                   // and sums below cannot overflow, and a negative height / width is an empty rectangle
        s_rect[i] = min(max(v, (i & 2) ? 0 : -(1 << 29)), 1 << 29);
    }
    stage_table(s_tab, table);   // ends in the barrier that also publishes s_rect

    const float fill[3] = {fill0, fill1, fill2};
    const size_t frame = (size_t)n * 3 * HW;
    for (int k = 0; k < ERASE_STEPS; ++k) {
        const int u = (chunk * ERASE_STEPS + k) * NTH + tid;
        if (u >= units) break;
        unsigned erased = 0;   // bit j: pixel PIX u + j lies in a rectangle
        if (cnt > 0) {
            const int p0 = PIX * u, y0 = p0 / W, x0 = p0 - y0 * W;
            if (x0 + PIX <= W) {   // the thread's pixels share a row: a rectangle erases the columns [x - x0, x - x0 + w) of them
                for (int r = 0; r < cnt; ++r) {
                    const int4 q = *reinterpret_cast<const int4*>(s_rect + 4 * r);   // y, x, h, w: one address for the whole wave
                    const int lo = min(max(q.y - x0, 0), PIX), hi = min(max(q.y - x0 + q.w, 0), PIX);
                    const unsigned cols = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
                    erased |= (unsigned)(y0 - q.x) < (unsigned)q.z ? cols : 0u;
                }
            } else {   // four consecutive pixels straddle rows (W % 4 != 0; several rows when W < 4): (y, x) per pixel
                int py[PIX], px[PIX];
#pragma unroll
                for (int j = 0; j < PIX; ++j) {
                    py[j] = y0;
                    px[j] = x0 + j;
                    while (px[j] >= W) {
                        px[j] -= W;
                        ++py[j];
                    }
                }
                for (int r = 0; r < cnt; ++r) {
                    const int4 q = *reinterpret_cast<const int4*>(s_rect + 4 * r);
#pragma unroll
                    for (int j = 0; j < PIX; ++j)
                        erased |= (unsigned)((unsigned)(py[j] - q.x) < (unsigned)q.z && (unsigned)(px[j] - q.y) < (unsigned)q.w) << j;
                }
            }
        }
        float* o = out + frame + (size_t)PIX * u;
        if constexpr (PIX == 4) {
            uint32_t b[3];   // b[c]: the four bytes of channel c
            if constexpr (NHWC) {
                const uint32_t* g = reinterpret_cast<const uint32_t*>(x + frame) + 3 * (size_t)u;
                const uint32_t u0 = g[0], u1 = g[1], u2 = g[2];   // bytes p0c0 p0c1 p0c2 p1c0 | p1c1 p1c2 p2c0 p2c1 | p2c2 p3c0 p3c1 p3c2
                b[0] = (u0 & 255) | ((u0 >> 24) << 8) | (((u1 >> 16) & 255) << 16) | (((u2 >> 8) & 255) << 24);
                b[1] = ((u0 >> 8) & 255) | ((u1 & 255) << 8) | ((u1 >> 24) << 16) | (((u2 >> 16) & 255) << 24);
                b[2] = ((u0 >> 16) & 255) | (((u1 >> 8) & 255) << 8) | ((u2 & 255) << 16) | ((u2 >> 24) << 24);
            } else {
                const uint32_t* g = reinterpret_cast<const uint32_t*>(x + frame) + u;
#pragma unroll
                for (int c = 0; c < 3; ++c) b[c] = g[(size_t)c * (HW / 4)];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* t = s_tab + c * FRAMES_U8_ROW;
                const float f = fill[c];
                *reinterpret_cast<float4*>(o + (size_t)c * HW) =
                    make_float4(erased & 1 ? f : t[b[c] & 255], erased & 2 ? f : t[(b[c] >> 8) & 255], erased & 4 ? f : t[(b[c] >> 16) & 255],
                                erased & 8 ? f : t[b[c] >> 24]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned char v = NHWC ? x[frame + 3 * (size_t)u + c] : x[frame + (size_t)c * HW + u];
                o[(size_t)c * HW] = erased ? fill[c] : s_tab[c * FRAMES_U8_ROW + v];
            }
        }
    }
}
}  // namespace

extern "C" int agrl_frames_normalize_u8(const unsigned char* x, const float* table, int layout, float* out, int N, int H, int W,
                                        agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && out, "agrl_frames_normalize_u8: null pointer");
    AGRL_CHECK_ARG(N > 0, "agrl_frames_normalize_u8: bad shape N=%d H=%d W=%d", N, H, W);
    FramesU8 u8;
    if (frames_u8_args("agrl_frames_normalize_u8", table, layout, H, W, &u8)) return 1;
    const int HW = H * W;
    const long long total = (long long)N * 3 * HW;
    const bool nhwc = layout == AGRL_FRAMES_NHWC;
    const bool vec = HW % 4 == 0 && (((uintptr_t)x) & 3) == 0 && (((uintptr_t)out) & 15) == 0;
    const long long work = vec ? (nhwc ? total / 12 : total / 4) : total;
    const long long want = (work + NTH - 1) / NTH;
    const unsigned grid = (unsigned)(want < 4096 ? want : 4096);   // grid-stride: 16 workgroups per CU are plenty for a stream
    hipStream_t s = (hipStream_t)stream;
    if (vec && nhwc)
        hipLaunchKernelGGL(frames_normalize_vec4_kernel<true>, dim3(grid), dim3(NTH), 0, s, (const uint32_t*)x, table, out, work, HW);
    else if (vec)
        hipLaunchKernelGGL(frames_normalize_vec4_kernel<false>, dim3(grid), dim3(NTH), 0, s, (const uint32_t*)x, table, out, work, HW);
    else if (nhwc)
        hipLaunchKernelGGL(frames_normalize_kernel<true>, dim3(grid), dim3(NTH), 0, s, x, table, out, total, HW);
    else
        hipLaunchKernelGGL(frames_normalize_kernel<false>, dim3(grid), dim3(NTH), 0, s, x, table, out, total, HW);
    AGRL_CHECK_LAUNCH("agrl_frames_normalize_u8");
    return 0;
}

extern "C" int agrl_frames_normalize_erase_u8(const unsigned char* x, const float* table, int layout, const int* rects, const int* counts,
                                              int max_rects, float fill0, float fill1, float fill2, float* out, int N, int H, int W,
                                              agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && out, "agrl_frames_normalize_erase_u8: null pointer");
    AGRL_CHECK_ARG(N > 0, "agrl_frames_normalize_erase_u8: bad shape N=%d H=%d W=%d", N, H, W);
    AGRL_CHECK_ARG(max_rects >= 0 && max_rects <= ERASE_MAX_RECTS, "agrl_frames_normalize_erase_u8: max_rects=%d, 0..%d", max_rects,
                   ERASE_MAX_RECTS);
    AGRL_CHECK_ARG(max_rects == 0 || (rects && counts), "agrl_frames_normalize_erase_u8: null pointer (rects / counts with max_rects=%d)",
                   max_rects);
    FramesU8 u8;
    if (frames_u8_args("agrl_frames_normalize_erase_u8", table, layout, H, W, &u8)) return 1;
    const int HW = H * W;
    const bool nhwc = layout == AGRL_FRAMES_NHWC;
    const bool vec = HW % 4 == 0 && (((uintptr_t)x) & 3) == 0 && (((uintptr_t)out) & 15) == 0;
    const int units = vec ? HW / 4 : HW;   // per frame
    const int chunks = (units + NTH * ERASE_STEPS - 1) / (NTH * ERASE_STEPS);
    AGRL_CHECK_ARG((long long)N * chunks <= 0x7fffffffLL, "agrl_frames_normalize_erase_u8: N=%d frames of %d chunks exceed the grid", N,
                   chunks);
    const dim3 grid((unsigned)(N * chunks));
    hipStream_t s = (hipStream_t)stream;
#define AGRL_ERASE_LAUNCH(NHWC_, PIX_)                                                                                               \
    hipLaunchKernelGGL((frames_normalize_erase_kernel<NHWC_, PIX_>), grid, dim3(NTH), 0, s, x, table, rects, counts, max_rects, fill0, \
                       fill1, fill2, out, HW, W, units, chunks)
    if (vec && nhwc)
        AGRL_ERASE_LAUNCH(true, 4);
    else if (vec)
        AGRL_ERASE_LAUNCH(false, 4);
    else if (nhwc)
        AGRL_ERASE_LAUNCH(true, 1);
    else
        AGRL_ERASE_LAUNCH(false, 1);
#undef AGRL_ERASE_LAUNCH
    AGRL_CHECK_LAUNCH("agrl_frames_normalize_erase_u8");
    return 0;
}
