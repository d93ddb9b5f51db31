// The tails of the STA baselines (sibling models ``sta`` / ``simple_sta``; reference torchreid/models/sta.py:206-245,
// simple_sta.py:202-221). All three kernels are HBM- or latency-bound, plain HIP C++, no atomics: every reduction runs in a fixed
// order, so two runs give the same bits.
//   agrl_sta_frame_stats : one pass over the layer-4 map -> part means, per-bin sums of the pixel norms, per-frame sum of their squares
//   agrl_sta_fuse        : per tracklet: scores -> temporal attention, first-maximum frame per part, cat(selected, attention-weighted)
//   agrl_linear_bn_relu  : skinny Linear + BatchNorm1d + ReLU head, the weight streamed from HBM once whatever M is
#include "agrl_common.h"

namespace {

constexpr int STA_PARTS = 4;

template <typename T>
__device__ inline void sta_load(const T* p, float v[DT<T>::epc]);
template <>
__device__ inline void sta_load<float>(const float* p, float v[4]) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}
template <>
__device__ inline void sta_load<lp16_t>(const lp16_t* p, float v[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) unpack_lp16x2(w[i], v[2 * i], v[2 * i + 1]);
}

// AdaptiveAvgPool2d((4,1)) bin of part q over h rows: [floor(q h / 4), ceil((q + 1) h / 4))
__host__ __device__ inline int sta_bin_start(int q, int h) { return (q * h) / STA_PARTS; }
__host__ __device__ inline int sta_bin_end(int q, int h) { return ((q + 1) * h + STA_PARTS - 1) / STA_PARTS; }

// grid = (F, 4): one workgroup per (frame, part), 256 threads. A lane owns G groups of VEC channels (c = (g * 256 + tid) * VEC) and keeps
// their part sums in registers across the bin's pixels; the pixels go by in batches of PB = 8 / G (eight 16-byte loads in flight per
// lane). Per pixel the sum of squares is a lane's fmaf chain over its channels, the wave's shuffle tree, then the four wave partials
// out of LDS as (w0 + w1) + (w2 + w3) -- read by every thread, so all of them hold the same n_p. LDS partials are double-buffered by
// batch parity: one barrier per batch.
//   nsum[f,q] = sum over the bin's pixels, in memory order, of sqrt(n2_p);  nsq[f,q] = sum of n2_p over the pixels of rows
//   [start_q, start_{q+1}) -- the part of the bin no later bin owns, so that the four add up to the frame's sum with every pixel once.
template <typename T, int G>
__global__ __launch_bounds__(256) void sta_frame_stats_kernel(const T* __restrict__ map, float* __restrict__ vmean,
                                                              float* __restrict__ nsum, float* __restrict__ nsq, int h, int w, int C) {
    constexpr int VEC = DT<T>::epc;
    constexpr int PB = 8 / G;
    __shared__ float s_red[2][4][PB];
    const int frame = blockIdx.x, part = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p_begin = sta_bin_start(part, h) * w, p_end = sta_bin_end(part, h) * w;
    const int p_own = part + 1 < STA_PARTS ? sta_bin_start(part + 1, h) * w : h * w;
    const T* src = map + (size_t)frame * h * w * C;
    float acc[G][VEC];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[g][j] = 0.f;
    float a_nsum = 0.f, a_nsq = 0.f;
    int buf = 0;
    for (int p0 = p_begin; p0 < p_end; p0 += PB, buf ^= 1) {
        float v[PB][G][VEC];
#pragma unroll
        for (int i = 0; i < PB; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int c = (g * 256 + tid) * VEC;
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[i][g][j] = 0.f;
                if (p0 + i < p_end && c < C) sta_load<T>(src + (size_t)(p0 + i) * C + c, v[i][g]);
            }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            float sq = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    acc[g][j] += v[i][g][j];
                    sq = fmaf(v[i][g][j], v[i][g][j], sq);
                }
            sq = wave_sum(sq);
            if (lane == 0) s_red[buf][wave][i] = sq;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const float n2 = (s_red[buf][0][i] + s_red[buf][1][i]) + (s_red[buf][2][i] + s_red[buf][3][i]);
            if (p0 + i < p_end) a_nsum += sqrtf(n2);
            if (p0 + i < p_own) a_nsq += n2;
        }
    }
    const float inv = 1.f / (float)(p_end - p_begin);
    float* dst = vmean + ((size_t)frame * STA_PARTS + part) * C;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = (g * 256 + tid) * VEC;
        if (c < C) {
#pragma unroll
            for (int j = 0; j < VEC; j += 4)
                *reinterpret_cast<float4*>(dst + c + j) =
                    make_float4(acc[g][j] * inv, acc[g][j + 1] * inv, acc[g][j + 2] * inv, acc[g][j + 3] * inv);
        }
    }
    if (tid == 0) {
        nsum[frame * STA_PARTS + part] = a_nsum;
        nsq[frame * STA_PARTS + part] = a_nsq;
    }
}

// grid = (B): one 512-thread workgroup per tracklet. LDS: S * 4 scores / attention weights, 4 selected frames.
//   scores   map : t < 4 S threads, one (s, q) each: (nsum / npix_q) / max(sqrt(((nsq0 + nsq1) + nsq2) + nsq3), 1e-12)
//            norm: a wavefront per node: a lane's fmaf chain over its float4 channel groups, shuffle tree, sqrt
//   t_a, idx     : four threads, one part each: sum_s |score| ascending, the quotient, the FIRST s attaining the maximum
//   f_g          : a thread per four channels: over the parts ascending, the selected frame's mean added up / the fmaf chain over s
//                  ascending added up; ((p0 + p1) + p2) + p3 times 0.25
__global__ __launch_bounds__(512) void sta_fuse_kernel(const float* __restrict__ vmean, const float* __restrict__ nsum,
                                                       const float* __restrict__ nsq, float* __restrict__ f_g, float* __restrict__ t_a,
                                                       int32_t* __restrict__ idx, int S, int C, int h, int w, int mode) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float* s_ta = s_mem;                                      // [S * 4]
    int* s_idx = reinterpret_cast<int*>(s_mem + S * STA_PARTS);  // [4]
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = S * STA_PARTS;
    const float* nodes = vmean + (size_t)b * V * C;
    if (mode == 0) {
        for (int t = tid; t < V; t += 512) {
            const int s = t / STA_PARTS, q = t % STA_PARTS;
            const float* fq = nsq + ((size_t)b * S + s) * STA_PARTS;
            const float tot = ((fq[0] + fq[1]) + fq[2]) + fq[3];
            const float npix = (float)((sta_bin_end(q, h) - sta_bin_start(q, h)) * w);
            s_ta[t] = (nsum[((size_t)b * S + s) * STA_PARTS + q] / npix) / fmaxf(sqrtf(tot), 1e-12f);
        }
    } else {
        for (int v = wave; v < V; v += 8) {
            const float* src = nodes + (size_t)v * C;
            float sq = 0.f;
            for (int c = lane * 4; c < C; c += 256) {
                const float4 x = *reinterpret_cast<const float4*>(src + c);
                sq = fmaf(x.x, x.x, sq); sq = fmaf(x.y, x.y, sq); sq = fmaf(x.z, x.z, sq); sq = fmaf(x.w, x.w, sq);
            }
            sq = wave_sum(sq);
            if (lane == 0) s_ta[v] = sqrtf(sq);
        }
    }
    __syncthreads();
    if (tid < STA_PARTS) {
        const int q = tid;
        float tot = 0.f;
        for (int s = 0; s < S; ++s) tot += fabsf(s_ta[s * STA_PARTS + q]);
        const float den = fmaxf(tot, 1e-12f);
        float best = 0.f;
        int arg = 0;
        for (int s = 0; s < S; ++s) {
            const float a = s_ta[s * STA_PARTS + q] / den;
            s_ta[s * STA_PARTS + q] = a;
            t_a[((size_t)b * S + s) * STA_PARTS + q] = a;
            if (s == 0 || a > best) {
                best = a;
                arg = s;
            }
        }
        s_idx[q] = arg;
        idx[b * STA_PARTS + q] = arg;
    }
    __syncthreads();
    for (int c = tid * 4; c < C; c += 2048) {
        float f1[4] = {0.f, 0.f, 0.f, 0.f}, f2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < STA_PARTS; ++q) {
            const float4 sel = *reinterpret_cast<const float4*>(nodes + ((size_t)s_idx[q] * STA_PARTS + q) * C + c);
            float u[4] = {0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < S; s0 += 8) {
                float4 nv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    nv[i] = s0 + i < S ? *reinterpret_cast<const float4*>(nodes + ((size_t)(s0 + i) * STA_PARTS + q) * C + c)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (s0 + i < S) {
                        const float a = s_ta[(s0 + i) * STA_PARTS + q];
                        u[0] = fmaf(a, nv[i].x, u[0]); u[1] = fmaf(a, nv[i].y, u[1]);
                        u[2] = fmaf(a, nv[i].z, u[2]); u[3] = fmaf(a, nv[i].w, u[3]);
                    }
            }
            f1[0] += sel.x; f1[1] += sel.y; f1[2] += sel.z; f1[3] += sel.w;
#pragma unroll
            for (int j = 0; j < 4; ++j) f2[j] += u[j];
        }
        float* dst = f_g + (size_t)b * 2 * C;
        *reinterpret_cast<float4*>(dst + c) = make_float4(f1[0] * 0.25f, f1[1] * 0.25f, f1[2] * 0.25f, f1[3] * 0.25f);
        *reinterpret_cast<float4*>(dst + C + c) = make_float4(f2[0] * 0.25f, f2[1] * 0.25f, f2[2] * 0.25f, f2[3] * 0.25f);
    }
}

// grid = (ceil(N / 4)): a wavefront per output column n (one row of W), four per workgroup. K goes by in chunks of KC = 256: a lane
// owns four consecutive columns of the row per chunk (16 bytes of an fp32 weight, 8 of a 16-bit one; a wavefront reads 1 KiB / 512 B
// contiguous) and multiplies them with the same columns of all MT rows of x out of LDS (x chunk staged by the whole workgroup, zero
// rows above M, zero columns above K; 2 x 32 x 256 floats = 64 KB at the largest MT, which is what bounds M). Next chunk's weight
// piece and x slice are loaded into registers before this chunk's fmafs; the x slice goes to the other LDS buffer afterwards: one
// barrier per chunk. Per (m, n): a lane's fmaf chain over its K / 64 columns ascending, the shuffle tree, fmaf(acc, scale, shift),
// ReLU (NaN-keeping).
template <typename TW>
__device__ inline void lbr_load_w(const TW* p, float v[4]);
template <>
__device__ inline void lbr_load_w<float>(const float* p, float v[4]) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
}
template <>
__device__ inline void lbr_load_w<lp16_t>(const lp16_t* p, float v[4]) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    unpack_lp16x2(u.x, v[0], v[1]);
    unpack_lp16x2(u.y, v[2], v[3]);
}

constexpr int LBR_KC = 256;

template <typename TW, int MT>
__global__ __launch_bounds__(256) void linear_bn_relu_kernel(const float* __restrict__ x, const TW* __restrict__ wgt,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ out, int M, int K, int N) {
    constexpr int VEC = 4;
    constexpr int KC = LBR_KC;
    constexpr int XN = MT * KC / 4 / 256;   // float4 pieces of an x chunk per thread (MT / 4)
    static_assert(MT % 4 == 0, "whole float4 pieces per thread");
    extern __shared__ __attribute__((aligned(16))) float s_x[];   // [2][MT][KC]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x * 4 + wave;
    const bool has = n < N;
    const TW* wrow = wgt + (size_t)(has ? n : 0) * K;
    const int nchunks = (K + KC - 1) / KC;
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;

    float4 xr[XN];
    float wv[VEC];
    auto load_x = [&](int k0) {
#pragma unroll
        for (int i = 0; i < XN; ++i) {
            const int e = i * 256 + tid;                 // float4 index inside the chunk
            const int m = e / (KC / 4), k = k0 + (e % (KC / 4)) * 4;
            xr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < M && k < K) xr[i] = *reinterpret_cast<const float4*>(x + (size_t)m * K + k);
        }
    };
    auto store_x = [&](float* dstbuf) {
#pragma unroll
        for (int i = 0; i < XN; ++i) {
            const int e = i * 256 + tid;
            *reinterpret_cast<float4*>(dstbuf + e * 4) = xr[i];
        }
    };
    auto load_w = [&](int k0) {
        const int k = k0 + lane * VEC;
#pragma unroll
        for (int j = 0; j < VEC; ++j) wv[j] = 0.f;
        if (has && k < K) lbr_load_w<TW>(wrow + k, wv);
    };

    load_x(0);
    load_w(0);
    store_x(s_x);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        float* cur = s_x + (ch & 1) * MT * KC;
        float wc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) wc[j] = wv[j];
        const bool more = ch + 1 < nchunks;
        if (more) {
            load_x((ch + 1) * KC);
            load_w((ch + 1) * KC);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float* xs = cur + m * KC + lane * VEC;
#pragma unroll
            for (int j = 0; j < VEC; j += 4) {
                const float4 xv = *reinterpret_cast<const float4*>(xs + j);
                acc[m] = fmaf(wc[j], xv.x, acc[m]); acc[m] = fmaf(wc[j + 1], xv.y, acc[m]);
                acc[m] = fmaf(wc[j + 2], xv.z, acc[m]); acc[m] = fmaf(wc[j + 3], xv.w, acc[m]);
            }
        }
        if (more) store_x(s_x + ((ch + 1) & 1) * MT * KC);
        __syncthreads();
    }
    const float sc = has ? scale[n] : 0.f, sh = has ? shift[n] : 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const float t = wave_sum(acc[m]);
        if (has && lane == 0 && m < M) out[(size_t)m * N + n] = relu_nan(fmaf(t, sc, sh));
    }
}

template <typename TW>
int launch_linear_bn_relu(const float* x, const void* w, const float* scale, const float* shift, float* out, int M, int K, int N,
                          hipStream_t st) {
    constexpr int KC = LBR_KC;
    const dim3 grid(cdiv(N, 4));
#define LAUNCH_LBR(MT)                                                                                                         \
    hipLaunchKernelGGL((linear_bn_relu_kernel<TW, MT>), grid, dim3(256), 2 * MT * KC * sizeof(float), st, x, (const TW*)w, scale, \
                       shift, out, M, K, N)
    if (M <= 4) LAUNCH_LBR(4);
    else if (M <= 8) LAUNCH_LBR(8);
    else if (M <= 16) LAUNCH_LBR(16);
    else LAUNCH_LBR(32);
#undef LAUNCH_LBR
    return 0;
}

}  // namespace

extern "C" int agrl_sta_frame_stats(const void* map, float* vmean, float* nsum, float* nsq, int F, int h, int w, int C, int dtype,
                                    agrl_stream_t stream) {
    AGRL_CHECK_ARG(map && vmean && nsum && nsq, "agrl_sta_frame_stats: null pointer");
    AGRL_CHECK_ARG(dtype == AGRL_F32 || dtype == AGRL_LP16, "agrl_sta_frame_stats: bad dtype %d", dtype);
    AGRL_CHECK_ARG(F > 0 && w > 0 && C > 0, "agrl_sta_frame_stats: bad shape");
    AGRL_CHECK_ARG(h >= STA_PARTS, "agrl_sta_frame_stats: h=%d must be at least %d (one row per part)", h, STA_PARTS);
    AGRL_CHECK_ARG(C % 8 == 0, "agrl_sta_frame_stats: C=%d must be a multiple of 8", C);
    const int vec = dtype == AGRL_F32 ? 4 : 8;
    const int groups = cdiv(C, 256 * vec);
    AGRL_CHECK_ARG(groups <= 4, "agrl_sta_frame_stats: C=%d beyond the %d channels a workgroup's registers hold", C, 4 * 256 * vec);
    AGRL_CHECK_ARG((long long)h * w <= (1 << 24), "agrl_sta_frame_stats: map too large");
    AGRL_CHECK_ARG((((uintptr_t)map | (uintptr_t)vmean) & 15) == 0, "agrl_sta_frame_stats: map / vmean must be 16-byte aligned");
    const dim3 grid(F, STA_PARTS);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH_FS(T, G) \
    hipLaunchKernelGGL((sta_frame_stats_kernel<T, G>), grid, dim3(256), 0, st, (const T*)map, vmean, nsum, nsq, h, w, C)
    if (dtype == AGRL_F32) {
        if (groups == 1) LAUNCH_FS(float, 1); else if (groups == 2) LAUNCH_FS(float, 2); else LAUNCH_FS(float, 4);
    } else {
        if (groups == 1) LAUNCH_FS(lp16_t, 1); else if (groups == 2) LAUNCH_FS(lp16_t, 2); else LAUNCH_FS(lp16_t, 4);
    }
#undef LAUNCH_FS
    AGRL_CHECK_LAUNCH("agrl_sta_frame_stats");
    return 0;
}

extern "C" int agrl_sta_fuse(const float* vmean, const float* nsum, const float* nsq, float* f_g, float* t_a, int32_t* idx, int B,
                             int S, int C, int h, int w, int mode, agrl_stream_t stream) {
    AGRL_CHECK_ARG(mode == AGRL_STA_MAP || mode == AGRL_STA_NORM, "agrl_sta_fuse: mode must be 0 (map) or 1 (norm), got %d", mode);
    AGRL_CHECK_ARG(vmean && f_g && t_a && idx, "agrl_sta_fuse: null pointer");
    AGRL_CHECK_ARG(B > 0 && S > 0 && C > 0, "agrl_sta_fuse: bad shape");
    AGRL_CHECK_ARG(C % 4 == 0, "agrl_sta_fuse: C=%d must be a multiple of 4", C);
    AGRL_CHECK_ARG((((uintptr_t)vmean | (uintptr_t)f_g) & 15) == 0, "agrl_sta_fuse: vmean / f_g must be 16-byte aligned");
    if (mode == AGRL_STA_MAP) {
        AGRL_CHECK_ARG(nsum && nsq, "agrl_sta_fuse: the map mode needs nsum and nsq");
        AGRL_CHECK_ARG(h >= STA_PARTS && w > 0, "agrl_sta_fuse: the map mode needs the map's h >= %d and w > 0", STA_PARTS);
    }
    const size_t lds = ((size_t)S * STA_PARTS + STA_PARTS) * sizeof(float);
    AGRL_CHECK_ARG(lds <= 64 * 1024, "agrl_sta_fuse: S=%d too large (4 S + 4 floats must fit 64 KB of LDS)", S);
    hipLaunchKernelGGL(sta_fuse_kernel, dim3(B), dim3(512), lds, (hipStream_t)stream, vmean, nsum, nsq, f_g, t_a, idx, S, C, h, w, mode);
    AGRL_CHECK_LAUNCH("agrl_sta_fuse");
    return 0;
}

extern "C" int agrl_linear_bn_relu(const float* x, const void* w, const float* scale, const float* shift, float* out, int M, int K,
                                   int N, int w_dtype, agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && w && scale && shift && out, "agrl_linear_bn_relu: null pointer");
    AGRL_CHECK_ARG(w_dtype == AGRL_F32 || w_dtype == AGRL_LP16, "agrl_linear_bn_relu: bad weight dtype %d", w_dtype);
    AGRL_CHECK_ARG(M > 0 && K > 0 && N > 0, "agrl_linear_bn_relu: bad shape");
    AGRL_CHECK_ARG(M <= AGRL_LINEAR_BN_RELU_MAX_M, "agrl_linear_bn_relu: M=%d above the %d rows of x the LDS staging holds", M,
                   AGRL_LINEAR_BN_RELU_MAX_M);
    AGRL_CHECK_ARG(K % 4 == 0, "agrl_linear_bn_relu: K=%d must be a multiple of 4", K);
    AGRL_CHECK_ARG((((uintptr_t)x | (uintptr_t)w) & 15) == 0, "agrl_linear_bn_relu: x / w must be 16-byte aligned");
    if (w_dtype == AGRL_F32)
        launch_linear_bn_relu<float>(x, w, scale, shift, out, M, K, N, (hipStream_t)stream);
    else
        launch_linear_bn_relu<lp16_t>(x, w, scale, shift, out, M, K, N, (hipStream_t)stream);
    AGRL_CHECK_LAUNCH("agrl_linear_bn_relu");
    return 0;
}
