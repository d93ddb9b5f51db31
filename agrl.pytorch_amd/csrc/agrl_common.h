// Shared device/host helpers for libagrl_hip.so (gfx950 only: 64-lane wavefronts are assumed).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/agrl_hip.h"

#define AGRL_WAVE 64

// ---- the 16-bit storage / MFMA operand type of THIS build. The same sources give two libraries:
//   -DAGRL_LP_F16=1 (default, lib/libagrl_hip.so)       IEEE fp16: 11 significand bits, |x| < 65504
//   -DAGRL_LP_F16=0 (lib/libagrl_hip_bf16.so)           bfloat16:   8 significand bits, fp32 range
// Both feed the same-rate MFMA (v_mfma_f32_16x16x32_f16 / _bf16, fp32 accumulation). fp16 is the default because the path's
// activations stay far inside its range (|x| <= ~15 with the recipe weights, ResNet50 inference in fp16 is routine) and its
// rounding error is 8 x smaller: embedding error 2.5e-4 against 1.7e-3 of the fp32 oracle -- inside the 1e-3 the north
// star allows, which bf16 is not. Every conversion and every 16-bit MFMA in the kernels goes through the helpers below.
#ifndef AGRL_LP_F16
#define AGRL_LP_F16 1
#endif
constexpr bool kLpF16 = AGRL_LP_F16 != 0;
typedef unsigned short lp16_t;  // raw bits of one 16-bit element (fp16 or bfloat16, see above)
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// ---- error plumbing: thread-local message, int status ------------------------------------------
void agrl_set_error(const char* fmt, ...);

#define AGRL_CHECK_ARG(cond, ...)       \
    do {                                \
        if (!(cond)) {                  \
            agrl_set_error(__VA_ARGS__); \
            return 1;                   \
        }                               \
    } while (0)

#define AGRL_CHECK_LAUNCH(name)                                                   \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            agrl_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return 2;                                                             \
        }                                                                         \
    } while (0)

// A positive finite power of two -- what every un-scaling factor of the split-fp16 entry points must be for the un-scaling to be
// exact. NaN, zero, negative, infinite and non-power-of-two values are refused.
static inline bool agrl_is_pow2(float v) {
    int e = 0;
    return v > 0.f && v <= 3.4e38f && frexpf(v, &e) == 0.5f;
}
#define AGRL_CHECK_POW2(value, who, name) \
    AGRL_CHECK_ARG(agrl_is_pow2(value), "%s: %s=%g is not a positive finite power of two", who, name, (double)(value))

// compute units of the current device (256 when the query fails); cached per device ordinal, no lock. Library-internal: not exported
__attribute__((visibility("hidden"))) int agrl_cu_count();

// LDS / global address-space pointers, as __builtin_amdgcn_global_load_lds takes them
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

// ---- 16-bit <-> f32 (round-to-nearest-even, NaN preserved; matches torch .to(float16) / .to(bfloat16)) -------------
__host__ __device__ inline float lp16_to_f32(lp16_t v) {
    if constexpr (kLpF16) {
        return (float)__builtin_bit_cast(_Float16, v);
    } else {
        return __builtin_bit_cast(float, ((uint32_t)v) << 16);
    }
}

__host__ __device__ inline lp16_t f32_to_lp16(float f) {
    if constexpr (kLpF16) {
        return __builtin_bit_cast(unsigned short, (_Float16)f);  // v_cvt_f16_f32, round-to-nearest-even
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        // gfx950 converts in hardware (v_cvt_pk_bf16_f32, round-to-nearest-even); the compiler emits it for this cast
        const __bf16 h = (__bf16)f;
        return __builtin_bit_cast(unsigned short, h);
#else
        uint32_t u = __builtin_bit_cast(uint32_t, f);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (lp16_t)((u >> 16) | 0x40);  // quiet NaN
        u += 0x7fffu + ((u >> 16) & 1u);
        return (lp16_t)(u >> 16);
#endif
    }
}

// two floats -> packed 16-bit pair (lo in bits 0..15): one v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32
__device__ inline uint32_t pack_lp16x2(float lo, float hi) {
    if constexpr (kLpF16) {
        typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
        const f16x2_t v = {(_Float16)lo, (_Float16)hi};
        return __builtin_bit_cast(uint32_t, v);
    } else {
        typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
        const bf16x2_t v = {(__bf16)lo, (__bf16)hi};
        return __builtin_bit_cast(uint32_t, v);
    }
}

// two floats -> packed BFLOAT16 pair whatever the build's 16-bit storage type: the split-bf16 recipe (AGRL_F32X3, Frag<f32s_t>)
// forms its low halves in bf16 and multiplies them with bf16 MFMAs in both builds
__device__ inline uint32_t pack_bf16x2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    const bf16x2_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

// packed 16-bit pair -> two floats (bf16: a shift and a mask; fp16: two v_cvt_f32_f16, the high half through SDWA / op_sel)
__device__ inline void unpack_lp16x2(uint32_t w, float& lo, float& hi) {
    if constexpr (kLpF16) {
        typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
        const f16x2_t v = __builtin_bit_cast(f16x2_t, w);
        lo = (float)v[0];
        hi = (float)v[1];
    } else {
        lo = __uint_as_float(w << 16);
        hi = __uint_as_float(w & 0xffff0000u);
    }
}

// one 16 x 16 x 32 MFMA on two 16-byte chunks of eight 16-bit elements, fp32 accumulation
// (operands: any 16-byte register type -- uint4, a float vector)
template <typename TA, typename TB>
__device__ inline __attribute__((ext_vector_type(4))) float mfma_lp16_16x16x32(const TA& a, const TB& b, __attribute__((ext_vector_type(4))) float c) {
    static_assert(sizeof(TA) == 16 && sizeof(TB) == 16, "16-byte MFMA operands");
    if constexpr (kLpF16) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
}

// ReLU that keeps a NaN: fmaxf(NaN, 0) is 0, which would turn an out-of-range activation of the fp16 build (inf, then
// inf - inf = NaN in the next layer) into a plausible-looking zero; with this form inf / NaN reach the embedding and
// evaluation.extract_features refuses them. One instruction on gfx950: v_maximum3_f32 (IEEE-754-2019 maximum, NaN-propagating).
__device__ inline float relu_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }

// ---- wavefront reductions (64 lanes) -------------------------------------------------------------
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ inline int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <typename T>
struct DT;
template <>
struct DT<float> {
    static constexpr int code = AGRL_F32;
    static constexpr int epc = 4;  // elements per 16-byte chunk
    __device__ static inline float ld(const float* p) { return *p; }
    __device__ static inline void st(float* p, float v) { *p = v; }
};
// fp32 storage, split-bf16 arithmetic (AGRL_F32X3): same layout as float, different MFMA recipe (Frag<f32s_t>)
struct f32s_t {
    float v;
};
template <>
struct DT<f32s_t> {
    static constexpr int code = AGRL_F32X3;
    static constexpr int epc = 4;
};
// fp32 storage, split-FP16 arithmetic (AGRL_F32H3, round 6): same layout as float, Frag<f32h_t>'s recipe
struct f32h_t {
    float v;
};
template <>
struct DT<f32h_t> {
    static constexpr int code = AGRL_F32H3;
    static constexpr int epc = 4;
};
template <>
struct DT<lp16_t> {
    static constexpr int code = AGRL_LP16;
    static constexpr int epc = 8;
    __device__ static inline float ld(const lp16_t* p) { return lp16_to_f32(*p); }
    __device__ static inline void st(lp16_t* p, float v) { *p = f32_to_lp16(v); }
};

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- tuning switches: read from the environment ONCE, when the library is loaded (agrl_reload_options() re-reads them: the
// A/B tools and the kernel tests flip them inside one process). No entry point calls getenv on the launch path.
// AGRL_OPT_UNSET = the variable is not set -> the measured-best default applies. Flags are 1 when set to anything but "0".
#define AGRL_OPT_UNSET (-2147483647 - 1)
struct AgrlOpts {
    int igemm_wide;      // AGRL_IGEMM_WIDE: 0 generic igemm, 1 auto -> wide, 2 / 3 force the 256 x 256 / 256 x 128 tile
    int pool_persist;    // AGRL_POOL_PERSIST: fused pooling through the persistent igemm instead of the wide kernel
    int conv3x3_wide, conv3x3_c64;   // AGRL_CONV3X3_{WIDE,C64}: two-block wide kernel / persistent 64-channel kernel on or off
    int distmat_tiled;   // AGRL_DISTMAT_TILED: tiled igemm (+ split-K) instead of the streaming distance kernel
    int topk_radix;        // AGRL_TOPK_RADIX: every top-k through the five-pass radix kernel
    int graph_linear_mmajor;  // AGRL_GRAPH_LINEAR_MMAJOR: conv-style XCD map for agrl_graph_linear_mix
    int conv3x3_n128;         // AGRL_CONV3X3_N128: conv3x3_wide_kernel with 128-channel tiles also where 256-channel ones apply
    int conv3x3_fat_pb;       // AGRL_CONV3X3_FAT_PB: 1 / 2 forces the pixel blocks per workgroup of conv3x3_fat_kernel (unset: 2 where that still covers the chip)
    int conv3x3_half, conv3x3_half_stagger;   // AGRL_CONV3X3_HALF (0 / 1), AGRL_CONV3X3_HALF_STAGGER (clocks): conv3x3_half_kernel on / off, its start delay
    int stem_split_lds;       // AGRL_STEM_SPLIT_LDS: 0 = patch and conv tile share one LDS region (four barriers per tile; A/B)
    int stem_xcd_map;         // AGRL_STEM_XCD_MAP: 0 = the 16-bit stem's tiles in launch order (A/B); unset / 1: every frame on one XCD
    int stem_regpool;         // AGRL_STEM_REGPOOL: 1 = the 16-bit stem pools its conv accumulators in registers where that form applies, 0 = the conv-tile kernel (unset: stem_mfma.hip's default)
    int distmat_tile_n;       // AGRL_DISTMAT_TILE_N: 192 / 256 forces the column width of the full distance matrix's tile (unset: by round count)
    int split16_ns;           // AGRL_SPLIT16_NS: 2 / 3 forces the LDS ring depth of the in-loop split-fp16 GEMM (unset: 3 for 64-channel tiles, else 2)
    int duo_persist;          // AGRL_DUO_PERSIST: 0 = the 16-bit 1x1 GEMMs of conv1x1_duo.hip through the one-shot form (unset / 1: persistent, round 6)
    int l3_chain;             // AGRL_L3_CHAIN: 1 / 0 = layer 3's middle Bottlenecks through bottleneck_chain_kernel / as separate launches (unset: bottleneck_chain.hip's default)
    int igemm_dbg, conv3x3_dbg;  // ablation masks: parsed only in an -DAGRL_ABLATE build, 0 in the shipped library
};
const AgrlOpts& agrl_opts();
inline bool agrl_opt_set(int v) { return v != AGRL_OPT_UNSET; }

// Ablation bits (skip stores / DMA / waits / MFMA: wrong results by design, profiling only) exist only in a library built
// with -DAGRL_ABLATE (make ABLATE=1 -> lib/libagrl_hip_ablate.so); the shipped object has no switch that removes work.
#ifdef AGRL_ABLATE
#define AGRL_DBG_BITS(p) ((p).dbg)
#else
#define AGRL_DBG_BITS(p) 0
#endif
