// The seam between two Bottlenecks of the MFMA-bound stages (layers 3 / 4), back to back in ONE kernel (16-bit build type):
//   out (M, N1) = relu(y2 (M, K1) @ w3 (N1, K1)^T + b3 + residual)        conv3 / bn3 / += / relu of block i,   vmgn.py:56-64
//   z   (M, N2) = relu(out @ w1n (N2, N1)^T + b1n)                        conv1 / bn1 / relu    of block i + 1, vmgn.py:48-50
// `out` (the 1024- / 2048-channel map) is written once -- it is the next block's residual -- and never read back: as two
// launches it crosses HBM three times (written, read by conv1, read as residual). The two GEMMs run on the same 128-pixel
// tile: conv3's output is produced in 256-channel chunks, each chunk is finished (bias + residual + ReLU, rounded once, stored)
// and at once contracted against the matching 256-deep k-slice of the next conv1 into an accumulator set that lives across
// the chunks (128 x N2 fp32: 64 / 128 registers per lane).
//
// How it works (form 3 of the history below):
//   * The weights are static, so they are packed once (agrl_bottleneck_seam_pack) into the exact order the kernel consumes them:
//     per chunk and wave one contiguous stream of 1-KiB MFMA A-fragments (lane-linear: 16 rows x 64 B of one 32-deep k-step).
//     A wave streams ITS fragments global -> AGPRs with plain 16-byte loads (one KiB per instruction, perfectly coalesced) through
//     a ring of 16 (8) fragments that is refilled the moment a fragment's eight MFMAs have issued: no LDS staging, no barrier.
//   * 256 threads = 4 waves, one per SIMD with 512 registers each. A wave owns 64 conv3 channels of the chunk (GEMM 1: 4 channel
//     fragments x 8 pixel fragments) and N2 / 4 conv1 channels (GEMM 2) of ALL 128 pixels: no weight fragment is needed by two
//     waves, and the 8 pixel fragments of a k-step are read from LDS once per wave and held in registers while the k-step's
//     weight fragments pass (each replaced by its successor right behind its last reader).
//   * LDS holds activations only: the y2 tile (K1 = 256: resident, 64 KB; K1 = 512: 16-KB k-tiles through a 5-slot ring, three
//     tiles ahead, LDS-DMA), the conv3 bias, and the hand-over buffer X (64 KB): a lane's packed epilogue registers (8 consecutive
//     channels of one pixel) ARE the B fragment of one k-step of GEMM 2, so X is an array of 1-KiB fragment blocks [k-step][pixel
//     fragment], written and read lane-linearly, and the same registers go to HBM as 16-byte stores.
//   * The residual never touches LDS: a chunk's accumulators START as residual + bias (16 loads per lane, issued one GEMM 2
//     earlier). Every load of the kernel is inline asm with hand-counted vmcnt waits (hipcc's own waits would drain the ring);
//     the counts come from a constexpr simulation of one chunk's issue order (make_sched).
//
// Round-4 history (every number: rocprofv3 kernel-trace minimum over 10 launches, 256 frames of 16 x 8, fp16, same box):
//   1. BOTH weight matrices staged through an LDS ring (48-KB k-tiles, LDS-DMA, one barrier per k-tile, two tiles ahead -- all
//      that fits beside the 64-KB hand-over buffer): parity-green, layer 4 185 us against 190 us for the two launches. Ablations:
//      171 us without a single MFMA, a lone tile on an idle chip 103 us -- 0.8 us per 32-MFMA step: a chain of barrier-gated
//      LDS-DMA round trips (issue -> landed ~1.1 us) with at most two steps in flight.
//   2. Weights out of the LDS: packed once (agrl_bottleneck_seam_pack) into the order the kernel consumes them and streamed
//      global -> registers; eight waves, each owning 32 channels of all 128 pixels. Same time (layer 3: 52 us, layer 4: 180 us):
//      now every wave reads every pixel fragment from LDS -- 12 MB per layer-4 tile at the ~128 B/clk the LDS delivers = 45 us
//      beside 62 us of MFMA -- and the skeleton without MFMAs, weight loads and HBM traffic still took 50 us.
//   3. This form: FOUR waves of 512 registers (one per SIMD), each owning 64 channels: half the LDS reads, B fragments of a k-step
//      held in registers, weight ring and GEMM 2's accumulators in asm-owned AGPRs. Layer 3 51.4 us against 59.1 us (37.5 + 22.6)
//      for the two launches; layer 4 178 us against 180 us; 256/1024/512 67.5 us against 70 us. What the time is: layer 3 / 4
//      without the chunk epilogues' HBM accesses 36 / 116 us (residual loads 10 / 17 us, out stores 8 / 37 us of the rest),
//      without weight loads as well 29 / 94 us, MFMA alone 16 / 62 us.
//   Tried on top of 3 and withdrawn: the weight ring 32 deep instead of 16 (52.3 us); the chunk's 32 HBM accesses spread one by
//   one behind GEMM 2's fragments instead of in a burst (52.1 us); lanes p / p + 8 swapping a piece by DPP so that every store /
//   load covers 8 pixels x 128 B = whole cache lines instead of 16 half lines (53.2 us); odd tiles starting half a chunk late so
//   that the CUs' bursts interleave (layer 4 +3.5 us with a 9 us delay). The HBM accesses of a chunk cost the same 16 us (layer 3)
//   however they are issued: they do not overlap the matrix work of the wave that issues them, and with one wave per SIMD nothing
//   else does either. The model uses the kernel where it wins (the five seams of layer 3: 3.578 -> 3.552 ms per step, same box).
//
// The tile body lives in seam_dev.h: bottleneck_chain.hip runs it behind a 3x3 phase, four Bottlenecks of layer 3 per launch (which is
// where the model uses it from half a chip of frames on; this kernel keeps the smaller batches, the 256/1024/512 and the layer-4 shapes).
#include "seam_dev.h"

namespace {

template <int K1, int N1, int N2>
__global__ __launch_bounds__(NWV * 64) void bottleneck_seam_kernel(const SeamParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem_[seam_lds_bytes<K1, N1>()];
    seam_tile<K1, N1, N2, false>(p, (lds_u8_t*)smem_, 0);
}

// ---- one-off packing of the two weight matrices into the per-(chunk, wave) fragment streams.
//   GEMM 1 fragment (k-step ks, a < 4):   row i of the MFMA A operand = conv3 channel 256 c + 64 w + sigma(a, i)
//   GEMM 2 fragment (k-step ks, a < FW2): row i = conv1 channel (N2 / 4) w + sigma(a, i)
//   sigma(a, i) = 32 (a >> 1) + 8 (i >> 2) + 4 (a & 1) + (i & 3): the MFMA result rows 4 f + r of a fragment PAIR of a lane are
//   then 8 consecutive channels (one 16-byte piece; igemm_wide.hip)
// lane (i = lane & 15, f = lane >> 4) holds the row's k-elements 32 ks + 8 f .. + 7.
__global__ void seam_pack_kernel(const lp16_t* __restrict__ w3, const lp16_t* __restrict__ w1n, uint4* __restrict__ wpk, int K1, int N1, int N2) {
    const int KS1 = K1 / 32, FW2 = N2 / 64, G1F = FW1 * KS1, FPC = G1F + 8 * FW2;
    const long long total = (long long)(N1 / SCH) * NWV * FPC * 64;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(t & 63);
        long long r = t >> 6;
        const int q = (int)(r % FPC);
        r /= FPC;
        const int w = (int)(r % NWV), c = (int)(r / NWV);
        const int i = lane & 15, f = lane >> 4;
        const lp16_t* src;
        if (q < G1F) {
            const int ks = q / FW1, a = q % FW1;
            const int ch = c * SCH + w * 64 + 32 * (a >> 1) + 8 * (i >> 2) + 4 * (a & 1) + (i & 3);
            src = w3 + (size_t)ch * K1 + ks * 32 + f * 8;
        } else {
            const int g = q - G1F, ks = g / FW2, a = g % FW2;
            const int och = w * (N2 / NWV) + 32 * (a >> 1) + 8 * (i >> 2) + 4 * (a & 1) + (i & 3);
            src = w1n + (size_t)och * N1 + c * SCH + ks * 32 + f * 8;
        }
        wpk[t] = *reinterpret_cast<const uint4*>(src);
    }
}

bool seam_shape_ok(int Cmid, int Cout, int Cnext) {
    return (Cmid == 256 && Cout == 1024 && Cnext == 256) || (Cmid == 512 && Cout == 2048 && Cnext == 512) ||
           (Cmid == 256 && Cout == 1024 && Cnext == 512);
}

}  // namespace

extern "C" long long agrl_bottleneck_seam_packed_bytes(int Cmid, int Cout, int Cnext) {
    if (!seam_shape_ok(Cmid, Cout, Cnext)) return 0;
    return ((long long)Cout * Cmid + (long long)Cnext * Cout) * 2;
}

extern "C" int agrl_bottleneck_seam_pack(const void* w3, const void* w1_next, void* packed, int Cmid, int Cout, int Cnext,
                                         agrl_stream_t stream) {
    AGRL_CHECK_ARG(w3 && w1_next && packed, "agrl_bottleneck_seam_pack: null pointer");
    AGRL_CHECK_ARG(seam_shape_ok(Cmid, Cout, Cnext), "agrl_bottleneck_seam_pack: built for 256/1024/256, 256/1024/512 and 512/2048/512 channels, got %d/%d/%d",
                   Cmid, Cout, Cnext);
    AGRL_CHECK_ARG((((uintptr_t)w3 | (uintptr_t)w1_next | (uintptr_t)packed) & 15) == 0, "agrl_bottleneck_seam_pack: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(seam_pack_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const lp16_t*>(w3),
                       reinterpret_cast<const lp16_t*>(w1_next), reinterpret_cast<uint4*>(packed), Cmid, Cout, Cnext);
    AGRL_CHECK_LAUNCH("agrl_bottleneck_seam_pack");
    return 0;
}

extern "C" int agrl_bottleneck_seam(const void* y2, const void* packed, const float* b3, const void* residual, void* out,
                                    const float* b1_next, void* z, int M, int Cmid, int Cout, int Cnext, agrl_stream_t stream) {
    AGRL_CHECK_ARG(y2 && packed && b3 && residual && out && b1_next && z, "agrl_bottleneck_seam: null pointer");
    AGRL_CHECK_ARG(seam_shape_ok(Cmid, Cout, Cnext), "agrl_bottleneck_seam: built for 256/1024/256, 256/1024/512 and 512/2048/512 channels, got %d/%d/%d",
                   Cmid, Cout, Cnext);
    AGRL_CHECK_ARG(M > 0 && M % SBM == 0, "agrl_bottleneck_seam: the pixel count must be a multiple of %d (whole 16 x 8 frames), got %d", SBM, M);
    AGRL_CHECK_ARG((size_t)M * Cout * 2 < (1ull << 32), "agrl_bottleneck_seam: maps beyond 4 GB are not addressed");
    const uintptr_t al = (uintptr_t)y2 | (uintptr_t)packed | (uintptr_t)b3 | (uintptr_t)residual | (uintptr_t)out | (uintptr_t)b1_next | (uintptr_t)z;
    AGRL_CHECK_ARG((al & 15) == 0, "agrl_bottleneck_seam: pointers must be 16-byte aligned");
    SeamParams p;
    p.y2 = reinterpret_cast<const unsigned char*>(y2);
    p.wpk = reinterpret_cast<const unsigned char*>(packed);
    p.b3 = b3;
    p.res = reinterpret_cast<const unsigned char*>(residual);
    p.out = reinterpret_cast<unsigned char*>(out);
    p.b1n = b1_next;
    p.z = reinterpret_cast<unsigned char*>(z);
    p.M = M;
    const dim3 grid(M / SBM), block(NWV * 64);
    if (Cmid == 256 && Cnext == 256) hipLaunchKernelGGL((bottleneck_seam_kernel<256, 1024, 256>), grid, block, 0, (hipStream_t)stream, p);
    else if (Cmid == 256) hipLaunchKernelGGL((bottleneck_seam_kernel<256, 1024, 512>), grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((bottleneck_seam_kernel<512, 2048, 512>), grid, block, 0, (hipStream_t)stream, p);
    AGRL_CHECK_LAUNCH("agrl_bottleneck_seam");
    return 0;
}
