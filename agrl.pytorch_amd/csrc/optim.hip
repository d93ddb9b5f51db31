// The optimiser update of the train step (optimizer.step(), train_vidreid_xent_htri.py:411-413, built by optimizers.py:7-23) as ONE
// multi-tensor pass: Adam / AMSGrad, SGD with momentum / Nesterov momentum, RMSprop, AdaBound / AMSBound and RAdam over every
// parameter of a launch class.
//
//   descriptor table  kOptWords int64 words per tensor: {param, grad, state0, state1, state2, numel, vec, 0} (device memory).
//                     Adam: state0 = exp_avg, state1 = exp_avg_sq, state2 = max_exp_avg_sq (AMSGrad, else 0);
//                     SGD:  state0 = momentum_buffer (0 without momentum);
//                     RMSprop: state0 = square_avg, state1 = momentum_buffer (0 without momentum);
//                     AdaBound: as Adam (state2 = max_exp_avg_sq for AMSBound, else 0);  RAdam: state0 = exp_avg, state1 = exp_avg_sq.
//                     vec != 0: param, grad and every state pointer are 16-byte aligned (decided on the host), so every chunk start
//                     is too and the chunk takes 16-byte accesses.
//   chunk table       int32 pairs {tensor, chunk index inside the tensor}: chunk c of tensor t covers the elements
//                     [c * kOptChunk, min(numel, (c + 1) * kOptChunk)).
//
// A workgroup of 256 threads strides over the chunk table (grid = min(n_chunks, kOptGrid)). A chunk is kOptChunk = 4096 elements:
// on the 16-byte path four float4 per lane and stream, on the dword path sixteen floats; all of a chunk's loads are issued before
// its arithmetic. The streams are p, g and the state, read once and written once: 32 bytes per element for Adam with the gradient
// zero-fill (zero_grad != 0 stores +0.0 to every gradient element consumed, in place of a separate memset pass).
//
// Arithmetic per element, IEEE division and square root (no fast-math flag, no approximate intrinsic); every constant derived
// from the hyper-parameters arrives as an fp32 value the host formed in double (1 - beta2 formed in fp32 would alone be off by
// 6e-5 relative):
//   Adam   gd = g + wd p;  m += (1 - beta1) (gd - m);  v = beta2 v + (1 - beta2) gd^2;  [vmax = max(vmax, v), used for v below]
//          p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps)        step_size = lr / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t)
//   SGD    gd = g + wd p;  buf = gd (a tensor's first step) | momentum buf + gd;  d = gd + momentum buf (Nesterov) | buf;  p -= lr d
//   RMSprop  gd = g + wd p;  sq = alpha sq + (1 - alpha) gd^2;  d = gd / (sqrt(sq) + eps);  buf = momentum buf + d, p -= lr buf | p -= lr d
//   AdaBound gd, m, v [, vmax] as Adam;  rate = min(max(step_size / (sqrt(v) + eps), lower), upper);  p -= rate m
//            step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t); no bias correction inside the denominator, eps after the root of the raw v
//   RAdam    v = beta2 v + (1 - beta2) g^2;  m += (1 - beta1) (g - m);  p -= decay p;  p -= step_size m / (sqrt(v) + eps) (adaptive form)
//            | p -= step_size m (momentum-only form); which form runs is decided per launch on the host
// No 16-bit type in this file: both builds of the library get the same code.
#include "agrl_common.h"

namespace {

constexpr int kOptChunk = 4096;   // elements per chunk: 256 threads x 4 x float4
constexpr int kOptGrid = 2048;    // workgroups at most: 256 CUs x 8
constexpr int kOptWords = 8;      // int64 words per descriptor

struct OptTensor {
    float* p;
    float* g;
    float* s0;
    float* s1;
    float* s2;
    long long numel;
    long long vec;
    long long pad;
};
static_assert(sizeof(OptTensor) == kOptWords * 8, "descriptor layout");

struct AdamArgs {
    float wd, omb1, beta2, omb2, step_size, inv_sqrt_bc2, eps;
};

struct SgdArgs {
    float wd, momentum, lr;
    int nesterov;
};

// ---- the per-element updates ---------------------------------------------------------------------------------------------------
template <bool AMS>
struct AdamOp {
    static constexpr int kStates = AMS ? 3 : 2;
    AdamArgs a;
    __device__ inline void operator()(float& p, float g, float* s) const {
        const float gd = g + a.wd * p;
        const float m = s[0] + a.omb1 * (gd - s[0]);
        float v = a.beta2 * s[1] + a.omb2 * (gd * gd);
        s[0] = m;
        s[1] = v;
        if constexpr (AMS) {
            v = fmaxf(s[2], v);
            s[2] = v;
        }
        p = p - a.step_size * m / (sqrtf(v) * a.inv_sqrt_bc2 + a.eps);
    }
};

// MODE 0: no momentum (no state);  1: a tensor's first step with momentum (buf is written, not read);  2: later steps
template <int MODE>
struct SgdOp {
    static constexpr int kStates = MODE == 0 ? 0 : 1;
    static constexpr bool kLoadState = MODE == 2;
    SgdArgs a;
    __device__ inline void operator()(float& p, float g, float* s) const {
        const float gd = g + a.wd * p;
        float d = gd;
        if constexpr (MODE != 0) {
            const float buf = MODE == 1 ? gd : a.momentum * s[0] + gd;
            s[0] = buf;
            d = a.nesterov ? gd + a.momentum * buf : buf;
        }
        p = p - a.lr * d;
    }
};
struct RmspropArgs {
    float wd, alpha, oma, eps, momentum, lr;
};

struct AdaBoundArgs {
    float wd, omb1, beta2, omb2, step_size, eps, lower, upper;
};

struct RAdamArgs {
    float omb1, beta2, omb2, decay, step_size, eps;
};

template <bool MOM>
struct RmspropOp {
    static constexpr int kStates = MOM ? 2 : 1;
    RmspropArgs a;
    __device__ inline void operator()(float& p, float g, float* s) const {
        const float gd = g + a.wd * p;
        const float sq = a.alpha * s[0] + a.oma * (gd * gd);
        s[0] = sq;
        float d = gd / (sqrtf(sq) + a.eps);
        if constexpr (MOM) {
            d = a.momentum * s[1] + d;
            s[1] = d;
        }
        p = p - a.lr * d;
    }
};

template <bool AMS>
struct AdaBoundOp {
    static constexpr int kStates = AMS ? 3 : 2;
    AdaBoundArgs a;
    __device__ inline void operator()(float& p, float g, float* s) const {
        const float gd = g + a.wd * p;
        const float m = s[0] + a.omb1 * (gd - s[0]);
        float v = a.beta2 * s[1] + a.omb2 * (gd * gd);
        s[0] = m;
        s[1] = v;
        if constexpr (AMS) {
            v = fmaxf(s[2], v);
            s[2] = v;
        }
        const float rate = fminf(fmaxf(a.step_size / (sqrtf(v) + a.eps), a.lower), a.upper);
        p = p - rate * m;
    }
};

// ADAPTIVE: the launch takes the adaptive form (N > 4), else the momentum-only form (v is still advanced)
template <bool ADAPTIVE>
struct RAdamOp {
    static constexpr int kStates = 2;
    RAdamArgs a;
    __device__ inline void operator()(float& p, float g, float* s) const {
        const float v = a.beta2 * s[1] + a.omb2 * (g * g);
        const float m = s[0] + a.omb1 * (g - s[0]);
        s[0] = m;
        s[1] = v;
        const float pd = p - a.decay * p;
        if constexpr (ADAPTIVE) {
            p = pd - a.step_size * m / (sqrtf(v) + a.eps);
        } else {
            p = pd - a.step_size * m;
        }
    }
};

template <bool AMS>
constexpr bool loads_state(const AdamOp<AMS>&) { return true; }
template <bool MOM>
constexpr bool loads_state(const RmspropOp<MOM>&) { return true; }
template <bool AMS>
constexpr bool loads_state(const AdaBoundOp<AMS>&) { return true; }
template <bool ADAPTIVE>
constexpr bool loads_state(const RAdamOp<ADAPTIVE>&) { return true; }
template <int MODE>
constexpr bool loads_state(const SgdOp<MODE>&) { return SgdOp<MODE>::kLoadState; }

__device__ inline float* state_ptr(const OptTensor& t, int k) { return k == 0 ? t.s0 : k == 1 ? t.s1 : t.s2; }

// one element through the dword path
template <typename Op>
__device__ inline void update_scalar(const Op& op, const OptTensor& t, long long e, bool zero_grad) {
    constexpr int NS = Op::kStates;
    float p = t.p[e];
    const float g = t.g[e];
    float s[NS > 0 ? NS : 1] = {};
    if (loads_state(op)) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = state_ptr(t, k)[e];
    }
    op(p, g, s);
    t.p[e] = p;
#pragma unroll
    for (int k = 0; k < NS; ++k) state_ptr(t, k)[e] = s[k];
    if (zero_grad) t.g[e] = 0.f;
}

template <typename Op>
__global__ __launch_bounds__(256) void optim_step_kernel(const OptTensor* __restrict__ tensors, const int2* __restrict__ chunks, int n_chunks,
                                                         Op op, int zero_grad) {
    constexpr int NS = Op::kStates;
    constexpr int NSA = NS > 0 ? NS : 1;
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int2 ch = chunks[c];
        const OptTensor t = tensors[ch.x];                      // uniform over the workgroup: scalar loads
        const long long base = (long long)ch.y * kOptChunk;
        const long long left = t.numel - base;                  // > 0 by construction of the chunk table
        const int rem = left < kOptChunk ? (int)left : kOptChunk;
        if (t.vec) {
            // 16-byte path: quad j of this lane = elements base + (j * 256 + tid) * 4 .. + 3, taken while it lies inside the tensor
            float4 p[4], g[4], s[NSA][4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = (j * 256 + tid) * 4;
                ok[j] = e + 4 <= rem;
                p[j] = g[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok[j]) {
                    p[j] = *reinterpret_cast<const float4*>(t.p + base + e);
                    g[j] = *reinterpret_cast<const float4*>(t.g + base + e);
                }
            }
#pragma unroll
            for (int k = 0; k < NSA; ++k) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s[k][j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < NS && loads_state(op) && ok[j]) s[k][j] = *reinterpret_cast<const float4*>(state_ptr(t, k) + base + (j * 256 + tid) * 4);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float sx[NSA], sy[NSA], sz[NSA], sw[NSA];
#pragma unroll
                for (int k = 0; k < NSA; ++k) {
                    sx[k] = s[k][j].x; sy[k] = s[k][j].y; sz[k] = s[k][j].z; sw[k] = s[k][j].w;
                }
                op(p[j].x, g[j].x, sx);
                op(p[j].y, g[j].y, sy);
                op(p[j].z, g[j].z, sz);
                op(p[j].w, g[j].w, sw);
#pragma unroll
                for (int k = 0; k < NSA; ++k) s[k][j] = make_float4(sx[k], sy[k], sz[k], sw[k]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!ok[j]) continue;
                const int e = (j * 256 + tid) * 4;
                *reinterpret_cast<float4*>(t.p + base + e) = p[j];
#pragma unroll
                for (int k = 0; k < NS; ++k) *reinterpret_cast<float4*>(state_ptr(t, k) + base + e) = s[k][j];
                if (zero_grad) *reinterpret_cast<float4*>(t.g + base + e) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            // the ragged tail of the tensor's last chunk: rem % 4 elements through dwords
            if (tid < (rem & 3)) update_scalar(op, t, base + (rem & ~3) + tid, zero_grad != 0);
        } else {
            // dword path: element j of this lane = base + j * 256 + tid
            float p[16], g[16], s[NSA][16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int e = j * 256 + tid;
                p[j] = g[j] = 0.f;
                if (e < rem) {
                    p[j] = t.p[base + e];
                    g[j] = t.g[base + e];
                }
            }
#pragma unroll
            for (int k = 0; k < NSA; ++k) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s[k][j] = 0.f;
                    if (k < NS && loads_state(op) && j * 256 + tid < rem) s[k][j] = state_ptr(t, k)[base + j * 256 + tid];
                }
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float sj[NSA];
#pragma unroll
                for (int k = 0; k < NSA; ++k) sj[k] = s[k][j];
                op(p[j], g[j], sj);
#pragma unroll
                for (int k = 0; k < NSA; ++k) s[k][j] = sj[k];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int e = j * 256 + tid;
                if (e >= rem) continue;
                t.p[base + e] = p[j];
#pragma unroll
                for (int k = 0; k < NS; ++k) state_ptr(t, k)[base + e] = s[k][j];
                if (zero_grad) t.g[base + e] = 0.f;
            }
        }
    }
}

template <typename Op>
int launch(const char* name, const void* tensors, const void* chunks, int n_chunks, const Op& op, int zero_grad, agrl_stream_t stream) {
    const int grid = n_chunks < kOptGrid ? n_chunks : kOptGrid;
    hipLaunchKernelGGL(optim_step_kernel<Op>, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const OptTensor*>(tensors),
                       reinterpret_cast<const int2*>(chunks), n_chunks, op, zero_grad);
    AGRL_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int agrl_optim_geometry(int* chunk_elems, int* max_workgroups, int* descriptor_words) {
    AGRL_CHECK_ARG(chunk_elems && max_workgroups && descriptor_words, "agrl_optim_geometry: null pointer");
    *chunk_elems = kOptChunk;
    *max_workgroups = kOptGrid;
    *descriptor_words = kOptWords;
    return 0;
}

extern "C" int agrl_adam_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, float weight_decay,
                              float one_minus_beta1, float beta2, float one_minus_beta2, float step_size, float inv_sqrt_bc2, float eps,
                              int amsgrad, int zero_grad, agrl_stream_t stream) {
    AGRL_CHECK_ARG(tensors && chunks, "agrl_adam_step: null pointer");
    AGRL_CHECK_ARG(n_tensors > 0 && n_chunks >= n_tensors, "agrl_adam_step: need n_tensors > 0 and at least one chunk per tensor");
    AGRL_CHECK_ARG((((uintptr_t)tensors) & 7) == 0 && (((uintptr_t)chunks) & 7) == 0, "agrl_adam_step: tables must be 8-byte aligned");
    const AdamArgs a = {weight_decay, one_minus_beta1, beta2, one_minus_beta2, step_size, inv_sqrt_bc2, eps};
    if (amsgrad) return launch("agrl_adam_step", tensors, chunks, n_chunks, AdamOp<true>{a}, zero_grad, stream);
    return launch("agrl_adam_step", tensors, chunks, n_chunks, AdamOp<false>{a}, zero_grad, stream);
}

extern "C" int agrl_sgd_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, float weight_decay, float momentum,
                             float lr, int has_momentum, int first_step, int nesterov, int zero_grad, agrl_stream_t stream) {
    AGRL_CHECK_ARG(tensors && chunks, "agrl_sgd_step: null pointer");
    AGRL_CHECK_ARG(n_tensors > 0 && n_chunks >= n_tensors, "agrl_sgd_step: need n_tensors > 0 and at least one chunk per tensor");
    AGRL_CHECK_ARG((((uintptr_t)tensors) & 7) == 0 && (((uintptr_t)chunks) & 7) == 0, "agrl_sgd_step: tables must be 8-byte aligned");
    AGRL_CHECK_ARG(has_momentum || !nesterov, "agrl_sgd_step: Nesterov momentum needs a momentum buffer");
    const SgdArgs a = {weight_decay, momentum, lr, nesterov ? 1 : 0};
    if (!has_momentum) return launch("agrl_sgd_step", tensors, chunks, n_chunks, SgdOp<0>{a}, zero_grad, stream);
    if (first_step) return launch("agrl_sgd_step", tensors, chunks, n_chunks, SgdOp<1>{a}, zero_grad, stream);
    return launch("agrl_sgd_step", tensors, chunks, n_chunks, SgdOp<2>{a}, zero_grad, stream);
}

#define AGRL_OPTIM_TABLE_CHECKS(fn)                                                                                                  \
    AGRL_CHECK_ARG(tensors && chunks, fn ": null pointer");                                                                          \
    AGRL_CHECK_ARG(n_tensors > 0 && n_chunks >= n_tensors, fn ": need n_tensors > 0 and at least one chunk per tensor");             \
    AGRL_CHECK_ARG((((uintptr_t)tensors) & 7) == 0 && (((uintptr_t)chunks) & 7) == 0, fn ": tables must be 8-byte aligned")

extern "C" int agrl_rmsprop_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, float weight_decay, float alpha,
                                 float one_minus_alpha, float eps, float momentum, float lr, int has_momentum, int zero_grad,
                                 agrl_stream_t stream) {
    AGRL_OPTIM_TABLE_CHECKS("agrl_rmsprop_step");
    const RmspropArgs a = {weight_decay, alpha, one_minus_alpha, eps, momentum, lr};
    if (has_momentum) return launch("agrl_rmsprop_step", tensors, chunks, n_chunks, RmspropOp<true>{a}, zero_grad, stream);
    return launch("agrl_rmsprop_step", tensors, chunks, n_chunks, RmspropOp<false>{a}, zero_grad, stream);
}

extern "C" int agrl_adabound_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, float weight_decay,
                                  float one_minus_beta1, float beta2, float one_minus_beta2, float step_size, float eps, float lower,
                                  float upper, int amsbound, int zero_grad, agrl_stream_t stream) {
    AGRL_OPTIM_TABLE_CHECKS("agrl_adabound_step");
    AGRL_CHECK_ARG(lower <= upper, "agrl_adabound_step: need lower <= upper");
    const AdaBoundArgs a = {weight_decay, one_minus_beta1, beta2, one_minus_beta2, step_size, eps, lower, upper};
    if (amsbound) return launch("agrl_adabound_step", tensors, chunks, n_chunks, AdaBoundOp<true>{a}, zero_grad, stream);
    return launch("agrl_adabound_step", tensors, chunks, n_chunks, AdaBoundOp<false>{a}, zero_grad, stream);
}

extern "C" int agrl_radam_step(const void* tensors, int n_tensors, const void* chunks, int n_chunks, float one_minus_beta1, float beta2,
                               float one_minus_beta2, float decay, float step_size, float eps, int adaptive, int zero_grad,
                               agrl_stream_t stream) {
    AGRL_OPTIM_TABLE_CHECKS("agrl_radam_step");
    const RAdamArgs a = {one_minus_beta1, beta2, one_minus_beta2, decay, step_size, eps};
    if (adaptive) return launch("agrl_radam_step", tensors, chunks, n_chunks, RAdamOp<true>{a}, zero_grad, stream);
    return launch("agrl_radam_step", tensors, chunks, n_chunks, RAdamOp<false>{a}, zero_grad, stream);
}
