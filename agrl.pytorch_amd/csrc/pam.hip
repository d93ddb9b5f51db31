// Position-attention part nodes of the sibling model ganet (torchreid/models/ganet.py:98-136 PAM_Module, :384-400 the
// per-slice use): for every frame and every pyramid slice (rows [start, end) of the h x w map, L = rows * w positions)
//     attention = softmax_q(query_p . key_q)            (L x L, over the key axis)
//     node      = avgpool(gamma * value . attention^T + 2 slice)
// The value conv (C -> C on every position, three times per frame because the pyramid covers the map three times) never
// has to be evaluated per position: average pooling is linear and every attention row sums to one, so
//     avgpool(value . attention^T) = Wv (X abar) + bv,      abar_q = mean_p attention[p][q]
// i.e. ONE matrix-vector product per node on the attention-weighted mean of the slice. This kernel produces the two
// per-node vectors the host needs -- xbar = X abar and xmean = mean of the slice -- from the map and the stacked
// query / key conv output; the host then runs the (F*P, C) x (C, C) Linear on xbar (agrl_linear_nobias) and combines
// (agrl_pam_combine). With the module's gamma == 0 (its value at construction) only xmean is needed.
// grid = (frames, parts), 256 threads. HBM-bound on the map (read once per pyramid level).
//
// Train mode (agrl_pam_pool_train, agrl_pam_pool_backward, agrl_pam_combine_train, agrl_pam_combine_backward, agrl_col_sum) keeps
// the same algebra, so the backward never sees the per-position value conv either. Per node, with A the L x L attention,
// given dxbar = d loss / d xbar (= Wv^T dy, from the Linear node) and dxmean (= 2 dnode):
//     dX[q]   = abar[q] dxbar + dxmean / L                      (needs only abar: pam_dx_kernel, every map element written once,
//                                                                 the pyramid levels summed in level order inside one thread)
//     dabar   = X dxbar                 g = A dabar
//     dE[p,q] = A[p,q] (dabar[q] - g[p]) / L                    (the column mean and the row softmax in one step)
//     dQ      = dE K                    dK = dE^T Q             (pam_backward_kernel: A recomputed in LDS from qk as the forward
//                                                                 does; one launch per pyramid level adding into a zeroed dqk, so
//                                                                 the order of the additions is fixed: no atomics anywhere)
// torchreid.hip_ops.pam_nodes_backward_reference restates this in torch; tests/pam_train_ref.py holds the kernels to it.
#include "agrl_common.h"

namespace {

constexpr int PAM_MAXL = 128;           // positions per slice (16 x 8 map)
constexpr int PAM_ES = PAM_MAXL + 1;    // energy row stride (floats): column sweeps are conflict-free
constexpr int PAM_CH = 32;              // query / key channels staged per step
constexpr int PAM_TS = PAM_CH + 1;

struct PamBins {
    int nparts;
    int start[16], end[16];
};

template <typename T>
__device__ inline float ldf(const T* p);
template <>
__device__ inline float ldf<float>(const float* p) { return *p; }
template <>
__device__ inline float ldf<lp16_t>(const lp16_t* p) { return lp16_to_f32(*p); }

// energies -> softmax over the key axis -> abar, for one slice of L positions: s_e = A (L x L, row stride PAM_ES), s_abar = column
// means of A. qkb: the slice's first row of the stacked query / key map. All 256 threads; ends on a barrier.
template <typename T>
__device__ __forceinline__ void pam_attention(const T* __restrict__ qkb, int L, int Cq, float* s_e, float* s_q, float* s_k, float* s_abar) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int c0 = 0; c0 < Cq; c0 += PAM_CH) {
        for (int e = tid; e < L * PAM_CH; e += 256) {
            const int p = e / PAM_CH, c = e - p * PAM_CH;
            s_q[p * PAM_TS + c] = ldf<T>(qkb + (size_t)p * 2 * Cq + c0 + c);
            s_k[p * PAM_TS + c] = ldf<T>(qkb + (size_t)p * 2 * Cq + Cq + c0 + c);
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < PAM_CH; ++c) {
            float a[8], b[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = s_q[(ty + 16 * i) * PAM_TS + c];
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = s_k[(tx + 16 * j) * PAM_TS + c];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = ty + 16 * i, q = tx + 16 * j;
            if (p < L && q < L) s_e[p * PAM_ES + q] = acc[i][j];
        }
    __syncthreads();
    // softmax over the key axis, one wavefront per query row
    for (int p = wave; p < L; p += 4) {
        const float v0 = lane < L ? s_e[p * PAM_ES + lane] : -INFINITY;
        const float v1 = lane + 64 < L ? s_e[p * PAM_ES + lane + 64] : -INFINITY;
        const float m = wave_max(fmaxf(v0, v1));
        const float e0 = lane < L ? expf(v0 - m) : 0.f, e1 = lane + 64 < L ? expf(v1 - m) : 0.f;
        const float s = wave_sum(e0 + e1);
        if (lane < L) s_e[p * PAM_ES + lane] = e0 / s;
        if (lane + 64 < L) s_e[p * PAM_ES + lane + 64] = e1 / s;
    }
    __syncthreads();
    if (tid < L) {
        float s = 0.f;
        for (int p = 0; p < L; ++p) s += s_e[p * PAM_ES + tid];
        s_abar[tid] = s / (float)L;
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void pam_pool_kernel(const T* __restrict__ x, const T* __restrict__ qk, float* __restrict__ xbar,
                                                       float* __restrict__ xmean, float* __restrict__ abar_out, int h, int w, int C, int Cq,
                                                       PamBins bins, int with_attention) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float* s_e = s_mem;                               // [L][PAM_ES] energy -> attention
    float* s_q = s_e + PAM_MAXL * PAM_ES;             // [L][PAM_TS]
    float* s_k = s_q + PAM_MAXL * PAM_TS;             // [L][PAM_TS]
    float* s_abar = s_k + PAM_MAXL * PAM_TS;          // [L]
    const int frame = blockIdx.x, part = blockIdx.y;
    const int tid = threadIdx.x;
    const int p0 = bins.start[part] * w;
    const int L = (bins.end[part] - bins.start[part]) * w;
    const size_t pix0 = (size_t)frame * h * w + p0;
    if (with_attention) {
        pam_attention<T>(qk + pix0 * (size_t)(2 * Cq), L, Cq, s_e, s_q, s_k, s_abar);
        if (abar_out && tid < PAM_MAXL) abar_out[((size_t)frame * bins.nparts + part) * PAM_MAXL + tid] = tid < L ? s_abar[tid] : 0.f;
    }
    // xbar[c] = sum_q abar[q] x[q][c], xmean[c] = mean_q x[q][c]; thread -> channels c, c + 256, ..: coalesced rows
    const T* xb = x + pix0 * (size_t)C;
    const size_t node = (size_t)frame * bins.nparts + part;
    for (int c = tid; c < C; c += 256) {
        float sb = 0.f, sm = 0.f;
        for (int q0 = 0; q0 < L; q0 += 8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = q0 + i < L ? ldf<T>(xb + (size_t)(q0 + i) * C + c) : 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (q0 + i < L) {
                    sm += v[i];
                    if (with_attention) sb = fmaf(s_abar[q0 + i], v[i], sb);
                }
        }
        xmean[node * C + c] = sm / (float)L;
        if (with_attention) xbar[node * C + c] = sb;
    }
}

// nodes = gamma * (y + bv) + 2 * xmean (y = Wv xbar), + optional bf16 copy (operand of the next Linear)
__global__ __launch_bounds__(256) void pam_combine_kernel(const float* __restrict__ y, const float* __restrict__ bv,
                                                          const float* __restrict__ xmean, float gamma,
                                                          const float* __restrict__ gamma_dev, float* __restrict__ nodes,
                                                          lp16_t* __restrict__ nodes_lp, size_t total, int C) {
    if (gamma_dev) gamma = gamma_dev[0];   // train mode: the parameter itself, no host read
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e % C);
        float v = 2.f * xmean[e];
        if (y) v = fmaf(gamma, y[e] + bv[c], v);
        nodes[e] = v;
        if (nodes_lp) nodes_lp[e] = f32_to_lp16(v);
    }
}

// ---- train mode ---------------------------------------------------------------------------------------------------------------
constexpr int PAM_RC = 64;   // row chunks of the column reductions (agrl_col_sum, agrl_pam_combine_backward)
constexpr size_t PAM_LDS_FWD = (size_t)(PAM_MAXL * PAM_ES + 2 * PAM_MAXL * PAM_TS + PAM_MAXL) * sizeof(float);
constexpr size_t PAM_LDS_BWD = PAM_LDS_FWD + PAM_MAXL * sizeof(float);

struct PamLevels {
    int nlev;
    int step[16], n[16], off[16];   // per pyramid level: rows per slice, slices, index of its first part
};

// One slice: the attention recomputed as in the forward, dabar = X dxbar, dE[p,q] = A[p,q] (dabar[q] - (A dabar)[p]) / L, then
// dQ = dE K and dK = dE^T Q ADDED into dqk (zeroed by the entry point). grid = (frames, slices of ONE pyramid level): the slices of
// a level are disjoint, so every dqk element has exactly one writer per launch and the levels add in launch order.
__global__ __launch_bounds__(256) void pam_backward_kernel(const float* __restrict__ x, const float* __restrict__ qk,
                                                           const float* __restrict__ dxbar, float* __restrict__ dqk,
                                                           float* __restrict__ abar_out, int h, int w, int C, int Cq, PamBins bins, int part0) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float* s_e = s_mem;                               // [L][PAM_ES] attention -> dE
    float* s_q = s_e + PAM_MAXL * PAM_ES;             // [L][PAM_TS]
    float* s_k = s_q + PAM_MAXL * PAM_TS;             // [L][PAM_TS]
    float* s_abar = s_k + PAM_MAXL * PAM_TS;          // [L]
    float* s_dab = s_abar + PAM_MAXL;                 // [L]
    const int frame = blockIdx.x, part = part0 + blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = bins.start[part] * w;
    const int L = (bins.end[part] - bins.start[part]) * w;
    const size_t pix0 = (size_t)frame * h * w + p0;
    const size_t node = (size_t)frame * bins.nparts + part;
    const float* qkb = qk + pix0 * (size_t)(2 * Cq);
    pam_attention<float>(qkb, L, Cq, s_e, s_q, s_k, s_abar);
    if (tid < PAM_MAXL) abar_out[node * PAM_MAXL + tid] = tid < L ? s_abar[tid] : 0.f;
    // dabar[q] = x[q] . dxbar: one wavefront per position, lanes along the channels (coalesced rows)
    const float* xb = x + pix0 * (size_t)C;
    const float* db = dxbar + node * C;
    for (int q = wave; q < L; q += 4) {
        const float* xr = xb + (size_t)q * C;
        float sacc = 0.f;
#pragma unroll 8
        for (int c = lane; c < C; c += 64) sacc = fmaf(xr[c], db[c], sacc);
        sacc = wave_sum(sacc);
        if (lane == 0) s_dab[q] = sacc;
    }
    __syncthreads();
    const float invL = 1.f / (float)L;
    for (int p = wave; p < L; p += 4) {
        const bool in0 = lane < L, in1 = lane + 64 < L;
        const float a0 = in0 ? s_e[p * PAM_ES + lane] : 0.f, a1 = in1 ? s_e[p * PAM_ES + lane + 64] : 0.f;
        const float d0 = in0 ? s_dab[lane] : 0.f, d1 = in1 ? s_dab[lane + 64] : 0.f;
        const float g = wave_sum(fmaf(a0, d0, a1 * d1));
        if (in0) s_e[p * PAM_ES + lane] = (a0 * (d0 - g)) * invL;
        if (in1) s_e[p * PAM_ES + lane + 64] = (a1 * (d1 - g)) * invL;
    }
    __syncthreads();
    // dQ[p][c] = sum_q dE[p][q] K[q][c], dK[q][c] = sum_p dE[p][q] Q[p][c]; thread -> rows pg + 32 i, channels cg .. cg + 3 of the chunk
    const int pg = tid >> 3, cg = (tid & 7) * 4;
    float* dqb = dqk + pix0 * (size_t)(2 * Cq);
    for (int c0 = 0; c0 < Cq; c0 += PAM_CH) {
        for (int e = tid; e < L * PAM_CH; e += 256) {
            const int p = e / PAM_CH, c = e - p * PAM_CH;
            s_q[p * PAM_TS + c] = qkb[(size_t)p * 2 * Cq + c0 + c];
            s_k[p * PAM_TS + c] = qkb[(size_t)p * 2 * Cq + Cq + c0 + c];
        }
        __syncthreads();
        float aq[4][4], ak[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) aq[i][j] = ak[i][j] = 0.f;
#pragma unroll 2
        for (int t = 0; t < L; ++t) {
            float eq[4], ek[4], kv[4], qv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                eq[i] = s_e[(pg + 32 * i) * PAM_ES + t];
                ek[i] = s_e[t * PAM_ES + pg + 32 * i];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kv[j] = s_k[t * PAM_TS + cg + j];
                qv[j] = s_q[t * PAM_TS + cg + j];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    aq[i][j] = fmaf(eq[i], kv[j], aq[i][j]);
                    ak[i][j] = fmaf(ek[i], qv[j], ak[i][j]);
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = pg + 32 * i;
            if (r < L) {
                float* o = dqb + (size_t)r * 2 * Cq + c0 + cg;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o[j] += aq[i][j];
                    o[Cq + j] += ak[i][j];
                }
            }
        }
        __syncthreads();
    }
}

// dX[f][r][col][c] = sum over the pyramid levels whose slices cover row r, in level order, of abar[q] dxbar[c] + dxmean[c] / L
// (q the position inside that level's slice); rows no slice covers get 0. grid = (frames, map rows): every element written once.
__global__ __launch_bounds__(256) void pam_dx_kernel(const float* __restrict__ abar, const float* __restrict__ dxbar,
                                                     const float* __restrict__ dxmean, float* __restrict__ dx, int h, int w, int C, int P,
                                                     PamLevels lv) {
    __shared__ float s_ab[16][PAM_MAXL];
    const int f = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    for (int e = tid; e < lv.nlev * w; e += 256) {
        const int l = e / w, col = e - l * w;
        const int j = r / lv.step[l];
        if (j < lv.n[l]) s_ab[l][col] = abar[((size_t)f * P + lv.off[l] + j) * PAM_MAXL + (r - j * lv.step[l]) * w + col];
    }
    __syncthreads();
    float* out = dx + ((size_t)f * h + r) * w * (size_t)C;
    for (int c = tid; c < C; c += 256) {
        for (int col0 = 0; col0 < w; col0 += 8) {
            float acc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = 0.f;
            for (int l = 0; l < lv.nlev; ++l) {
                const int j = r / lv.step[l];
                if (j >= lv.n[l]) continue;
                const size_t nd = ((size_t)f * P + lv.off[l] + j) * C + c;
                const float db = dxbar[nd], dm = dxmean[nd];
                const float invL = 1.f / (float)(lv.step[l] * w);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (col0 + i < w) acc[i] = fmaf(s_ab[l][col0 + i], db, fmaf(dm, invL, acc[i]));
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (col0 + i < w) out[(size_t)(col0 + i) * C + c] = acc[i];
        }
    }
}

// Column sums in two deterministic stages. Stage 1, grid = (ceil(C / 64), chunks) x 64 threads: a thread adds the rows of its chunk
// for one channel in row order. MODE 0: part[chunk][c] = sum x. MODE 1 (combine backward): also writes dy = gamma dn, dxmean = 2 dn
// and a second partial sum_r dn (y + bv) at part[chunks + chunk][c].
template <int MODE>
__global__ __launch_bounds__(64) void pam_colsum_partial_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ bv, const float* __restrict__ gamma_dev,
                                                                float* __restrict__ dy, float* __restrict__ dxmean, float* __restrict__ part,
                                                                int M, int C, int rpc) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const int chunk = blockIdx.y, r0 = chunk * rpc, r1 = min(M, r0 + rpc);
    float s = 0.f, t = 0.f;
    const float gm = MODE == 1 ? gamma_dev[0] : 0.f, b = MODE == 1 ? bv[c] : 0.f;
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        const size_t e = (size_t)r * C + c;
        const float d = x[e];
        s += d;
        if (MODE == 1) {
            t = fmaf(d, y[e] + b, t);
            dy[e] = gm * d;
            dxmean[e] = 2.f * d;
        }
    }
    part[(size_t)chunk * C + c] = s;
    if (MODE == 1) part[((size_t)gridDim.y + chunk) * C + c] = t;
}

// Stage 2: a thread adds the chunks of one channel in chunk order. MODE 0: out[c]. MODE 1: out[c] = gamma * sum (dbv) and the
// channel's share of dgamma at tcol[c].
template <int MODE>
__global__ __launch_bounds__(64) void pam_colsum_finish_kernel(const float* __restrict__ part, const float* __restrict__ gamma_dev,
                                                               float* __restrict__ out, float* __restrict__ tcol, int chunks, int C) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f, t = 0.f;
    for (int k = 0; k < chunks; ++k) {
        s += part[(size_t)k * C + c];
        if (MODE == 1) t += part[((size_t)chunks + k) * C + c];
    }
    out[c] = MODE == 1 ? gamma_dev[0] * s : s;
    if (MODE == 1) tcol[c] = t;
}

// dgamma = sum_c tcol[c]: one workgroup, a thread's channels in order, then the wavefront and the four wave sums in order
__global__ __launch_bounds__(256) void pam_dgamma_kernel(const float* __restrict__ tcol, float* __restrict__ dgamma, int C) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int c = tid; c < C; c += 256) s += tcol[c];
    s = wave_sum(s);
    if ((tid & 63) == 0) s_red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) dgamma[0] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// the pyramid slices of the splits (ganet.py:387-390: h // n rows per slice, remainder rows dropped); 0 or an error status
int pam_make_bins(const char* who, const int* splits, int n_splits, int h, int w, PamBins* bins, PamLevels* lv) {
    int P = 0;
    AGRL_CHECK_ARG(n_splits > 0 && n_splits <= 16, "%s: 1 to 16 pyramid levels", who);
    for (int i = 0; i < n_splits; ++i) {
        const int n = splits[i];
        AGRL_CHECK_ARG(n > 0 && P + n <= 16 && h / n > 0, "%s: at most 16 parts, each at least one map row", who);
        const int step = h / n;
        AGRL_CHECK_ARG(step * w <= PAM_MAXL, "%s: a slice has %d positions, at most %d supported", who, step * w, PAM_MAXL);
        if (lv) {
            lv->step[i] = step;
            lv->n[i] = n;
            lv->off[i] = P;
        }
        for (int j = 0; j < n; ++j) {
            bins->start[P] = step * j;
            bins->end[P] = step * (j + 1);
            ++P;
        }
    }
    bins->nparts = P;
    for (int i = P; i < 16; ++i) bins->start[i] = bins->end[i] = 0;
    if (lv) {
        lv->nlev = n_splits;
        for (int i = n_splits; i < 16; ++i) {
            lv->step[i] = 1;
            lv->n[i] = lv->off[i] = 0;
        }
    }
    return 0;
}

inline int pam_row_chunks(int M) { return M / 32 < 1 ? 1 : (M / 32 > PAM_RC ? PAM_RC : M / 32); }

}  // namespace

extern "C" int agrl_pam_pool(const void* x, const void* qk, float* xbar, float* xmean, int F, int h, int w, int C, int Cq,
                             const int* splits, int n_splits, int dtype, agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && xmean && splits, "agrl_pam_pool: null pointer");
    AGRL_CHECK_ARG((qk == nullptr) == (xbar == nullptr), "agrl_pam_pool: qk and xbar go together (both NULL when the module's gamma is 0)");
    AGRL_CHECK_ARG(F > 0 && h > 0 && w > 0 && C > 0 && n_splits > 0, "agrl_pam_pool: bad shape");
    AGRL_CHECK_ARG(dtype == AGRL_F32 || dtype == AGRL_LP16, "agrl_pam_pool: bad dtype %d", dtype);
    AGRL_CHECK_ARG(!qk || (Cq > 0 && Cq % PAM_CH == 0), "agrl_pam_pool: Cq=%d must be a multiple of %d", Cq, PAM_CH);
    PamBins bins;
    int P = 0;
    for (int i = 0; i < n_splits; ++i) {
        const int n = splits[i];
        AGRL_CHECK_ARG(n > 0 && P + n <= 16 && h / n > 0, "agrl_pam_pool: at most 16 parts, each at least one map row");
        const int step = h / n;  // ganet.py:387-390: h // n rows per slice, remainder rows dropped
        for (int j = 0; j < n; ++j) {
            bins.start[P] = step * j;
            bins.end[P] = step * (j + 1);
            AGRL_CHECK_ARG(step * w <= PAM_MAXL, "agrl_pam_pool: a slice has %d positions, at most %d supported", step * w, PAM_MAXL);
            ++P;
        }
    }
    bins.nparts = P;
    for (int i = P; i < 16; ++i) bins.start[i] = bins.end[i] = 0;
    const size_t lds = (size_t)(PAM_MAXL * PAM_ES + 2 * PAM_MAXL * PAM_TS + PAM_MAXL) * sizeof(float);
    const int att = qk != nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == AGRL_F32) {
        hipError_t e = hipFuncSetAttribute((const void*)pam_pool_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        AGRL_CHECK_ARG(e == hipSuccess, "agrl_pam_pool: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        hipLaunchKernelGGL(pam_pool_kernel<float>, dim3(F, P), dim3(256), lds, st, (const float*)x, (const float*)qk, xbar, xmean,
                           (float*)nullptr, h, w, C, Cq, bins, att);
    } else {
        hipError_t e = hipFuncSetAttribute((const void*)pam_pool_kernel<lp16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        AGRL_CHECK_ARG(e == hipSuccess, "agrl_pam_pool: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        hipLaunchKernelGGL(pam_pool_kernel<lp16_t>, dim3(F, P), dim3(256), lds, st, (const lp16_t*)x, (const lp16_t*)qk, xbar, xmean,
                           (float*)nullptr, h, w, C, Cq, bins, att);
    }
    AGRL_CHECK_LAUNCH("agrl_pam_pool");
    return 0;
}

extern "C" int agrl_pam_combine(const float* y, const float* bv, const float* xmean, float gamma, float* nodes, void* nodes_lp,
                                int rows, int C, agrl_stream_t stream) {
    AGRL_CHECK_ARG(xmean && nodes && rows > 0 && C > 0, "agrl_pam_combine: bad arguments");
    AGRL_CHECK_ARG((y == nullptr) == (bv == nullptr), "agrl_pam_combine: y and bv go together");
    const size_t total = (size_t)rows * C;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pam_combine_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, y, bv, xmean, gamma,
                       (const float*)nullptr, nodes, (lp16_t*)nodes_lp, total, C);
    AGRL_CHECK_LAUNCH("agrl_pam_combine");
    return 0;
}

extern "C" int agrl_pam_pool_train(const float* x, const float* qk, float* xbar, float* xmean, float* abar, int F, int h, int w, int C,
                                   int Cq, const int* splits, int n_splits, int dtype, agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && qk && xbar && xmean && abar && splits, "agrl_pam_pool_train: null pointer");
    AGRL_CHECK_ARG(dtype == AGRL_F32, "agrl_pam_pool_train: bad dtype %d (the train node is fp32)", dtype);
    AGRL_CHECK_ARG(F > 0 && h > 0 && w > 0 && C > 0, "agrl_pam_pool_train: bad shape");
    AGRL_CHECK_ARG(Cq > 0 && Cq % PAM_CH == 0, "agrl_pam_pool_train: Cq=%d must be a multiple of %d", Cq, PAM_CH);
    PamBins bins;
    if (int rc = pam_make_bins("agrl_pam_pool_train", splits, n_splits, h, w, &bins, nullptr)) return rc;
    hipError_t e = hipFuncSetAttribute((const void*)pam_pool_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAM_LDS_FWD);
    AGRL_CHECK_ARG(e == hipSuccess, "agrl_pam_pool_train: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(pam_pool_kernel<float>, dim3(F, bins.nparts), dim3(256), PAM_LDS_FWD, (hipStream_t)stream, x, qk, xbar, xmean, abar,
                       h, w, C, Cq, bins, 1);
    AGRL_CHECK_LAUNCH("agrl_pam_pool_train");
    return 0;
}

extern "C" int agrl_pam_pool_backward(const float* x, const float* qk, const float* dxbar, const float* dxmean, float* dx, float* dqk,
                                      float* abar, int F, int h, int w, int C, int Cq, const int* splits, int n_splits, int dtype,
                                      agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && qk && dxbar && dxmean && dx && dqk && abar && splits, "agrl_pam_pool_backward: null pointer");
    AGRL_CHECK_ARG(dtype == AGRL_F32, "agrl_pam_pool_backward: bad dtype %d (the train node is fp32)", dtype);
    AGRL_CHECK_ARG(F > 0 && h > 0 && w > 0 && C > 0, "agrl_pam_pool_backward: bad shape");
    AGRL_CHECK_ARG(Cq > 0 && Cq % PAM_CH == 0, "agrl_pam_pool_backward: Cq=%d must be a multiple of %d", Cq, PAM_CH);
    PamBins bins;
    PamLevels lv;
    if (int rc = pam_make_bins("agrl_pam_pool_backward", splits, n_splits, h, w, &bins, &lv)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipFuncSetAttribute((const void*)pam_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAM_LDS_BWD);
    AGRL_CHECK_ARG(e == hipSuccess, "agrl_pam_pool_backward: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    e = hipMemsetAsync(dqk, 0, (size_t)F * h * w * 2 * Cq * sizeof(float), st);
    AGRL_CHECK_ARG(e == hipSuccess, "agrl_pam_pool_backward: cannot clear dqk: %s", hipGetErrorString(e));
    for (int l = 0; l < lv.nlev; ++l)
        hipLaunchKernelGGL(pam_backward_kernel, dim3(F, lv.n[l]), dim3(256), PAM_LDS_BWD, st, x, qk, dxbar, dqk, abar, h, w, C, Cq, bins,
                           lv.off[l]);
    hipLaunchKernelGGL(pam_dx_kernel, dim3(F, h), dim3(256), 0, st, (const float*)abar, dxbar, dxmean, dx, h, w, C, bins.nparts, lv);
    AGRL_CHECK_LAUNCH("agrl_pam_pool_backward");
    return 0;
}

extern "C" int agrl_pam_combine_train(const float* y, const float* bv, const float* xmean, const float* gamma, float* nodes, int rows, int C,
                                      agrl_stream_t stream) {
    AGRL_CHECK_ARG(y && bv && xmean && gamma && nodes, "agrl_pam_combine_train: null pointer");
    AGRL_CHECK_ARG(rows > 0 && C > 0, "agrl_pam_combine_train: bad shape");
    const size_t total = (size_t)rows * C;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pam_combine_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, y, bv, xmean, 0.f, gamma, nodes, (lp16_t*)nullptr,
                       total, C);
    AGRL_CHECK_LAUNCH("agrl_pam_combine_train");
    return 0;
}

extern "C" size_t agrl_col_sum_workspace(int M, int C) {
    if (M <= 0 || C <= 0) return 0;
    return (size_t)(2 * pam_row_chunks(M) + 1) * C * sizeof(float);
}

extern "C" int agrl_pam_combine_backward(const float* dnodes, const float* y, const float* bv, const float* gamma, float* dy, float* dxmean,
                                         float* dgamma, float* dbv, int rows, int C, void* workspace, size_t workspace_bytes,
                                         agrl_stream_t stream) {
    AGRL_CHECK_ARG(dnodes && y && bv && gamma && dy && dxmean && dgamma && dbv && workspace, "agrl_pam_combine_backward: null pointer");
    AGRL_CHECK_ARG(rows > 0 && C > 0, "agrl_pam_combine_backward: bad shape");
    AGRL_CHECK_ARG(workspace_bytes >= agrl_col_sum_workspace(rows, C), "agrl_pam_combine_backward: workspace too small");
    const int chunks = pam_row_chunks(rows), rpc = cdiv(rows, chunks);
    float* part = (float*)workspace;
    float* tcol = part + (size_t)2 * chunks * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pam_colsum_partial_kernel<1>, dim3(cdiv(C, 64), chunks), dim3(64), 0, st, dnodes, y, bv, gamma, dy, dxmean, part, rows, C,
                       rpc);
    hipLaunchKernelGGL(pam_colsum_finish_kernel<1>, dim3(cdiv(C, 64)), dim3(64), 0, st, (const float*)part, gamma, dbv, tcol, chunks, C);
    hipLaunchKernelGGL(pam_dgamma_kernel, dim3(1), dim3(256), 0, st, (const float*)tcol, dgamma, C);
    AGRL_CHECK_LAUNCH("agrl_pam_combine_backward");
    return 0;
}

extern "C" int agrl_col_sum(const float* x, float* out, int M, int C, void* workspace, size_t workspace_bytes, agrl_stream_t stream) {
    AGRL_CHECK_ARG(x && out && workspace, "agrl_col_sum: null pointer");
    AGRL_CHECK_ARG(M > 0 && C > 0, "agrl_col_sum: bad shape");
    AGRL_CHECK_ARG(workspace_bytes >= agrl_col_sum_workspace(M, C), "agrl_col_sum: workspace too small");
    const int chunks = pam_row_chunks(M), rpc = cdiv(M, chunks);
    float* part = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pam_colsum_partial_kernel<0>, dim3(cdiv(C, 64), chunks), dim3(64), 0, st, x, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr, part, M, C, rpc);
    hipLaunchKernelGGL(pam_colsum_finish_kernel<0>, dim3(cdiv(C, 64)), dim3(64), 0, st, (const float*)part, (const float*)nullptr, out,
                       (float*)nullptr, chunks, C);
    AGRL_CHECK_LAUNCH("agrl_col_sum");
    return 0;
}
