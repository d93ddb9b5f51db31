// uint8 frames (include/agrl_hip.h, "uint8 frames"): what the stem kernels and agrl_frames_normalize_u8 share.
//
// The normalised value of byte u in channel c is table[c * FRAMES_U8_ROW + u], the caller's correctly rounded
// (float(u) / 255 - mean[c]) / std[c]; entry FRAMES_U8_PAD of every row is 0, so a kernel that stages a zero-padded patch gives its
// out-of-frame pixels that index instead of keeping a predicate next to the bytes. A lookup cannot differ from the fp32 tensor the
// caller would have built with the same table, which is what the bitwise tests of the uint8 path hold the kernels to.
#pragma once
#include "agrl_common.h"

constexpr int FRAMES_U8_PAD = 256;
constexpr int FRAMES_U8_ROW = 257;

struct FramesU8 {
    const float* table;   // (3, FRAMES_U8_ROW) fp32
    int pixel_stride;     // bytes between horizontally adjacent pixels of a channel: 1 (N,3,H,W) or 3 (N,H,W,3)
    int channel_stride;   // bytes between the channels of a pixel: H * W or 1
};

__device__ __forceinline__ FramesU8 frames_u8_of(const FramesU8& u8) { return u8; }

// validates the uint8-specific arguments of an entry point and fills the kernel argument; non-zero (error set) when they are bad
static inline int frames_u8_args(const char* who, const float* table, int layout, int H, int W, FramesU8* u8) {
    AGRL_CHECK_ARG(table, "%s: null table", who);
    AGRL_CHECK_ARG(layout == AGRL_FRAMES_NCHW || layout == AGRL_FRAMES_NHWC, "%s: bad layout %d", who, layout);
    AGRL_CHECK_ARG(H > 0 && W > 0 && (long long)H * W < (1ll << 29), "%s: bad frame size H=%d W=%d", who, H, W);
    u8->table = table;
    u8->pixel_stride = layout == AGRL_FRAMES_NHWC ? 3 : 1;
    u8->channel_stride = layout == AGRL_FRAMES_NHWC ? 1 : H * W;
    return 0;
}
