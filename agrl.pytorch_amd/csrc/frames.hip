// uint8 frames -> normalised fp32 NCHW frames: the reference's transform_test (ToTensor + Normalize, train_vidreid_xent_htri.py:214-217)
// for the paths that do not fuse it into the stem -- the native train step (its stem reads fp32 through agrl_im2col_rows) and any caller
// that wants the tensor. A streaming kernel: the 3 KB table sits in LDS, a thread turns four bytes into one 16-byte store (frames whose
// H W is a multiple of four, aligned pointers) or one byte into one float (anything else). Not on the eval hot path.
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
