// The stride-1 middle of layer 3 as ONE kernel per frame (16-bit build type): up to four Bottlenecks chained on the CU that owns
// the frame. A frame of layer 3 is 16 x 8 pixels = exactly one 128-pixel tile, and its 3x3 conv needs no pixel of another frame,
// so everything between the 1024-channel residual-stream maps stays in LDS. For blocks i = 1 .. n (n <= 4):
//   y_i     = relu(conv3x3_i(z_i) + b2_i)            phase A: patch in LDS -> accumulators -> y2 tile in LDS      vmgn.py:52-54
//   a_i     = relu(conv3_i(y_i) + b3_i + a_{i-1})    phase B, GEMM 1: stored to HBM (the next residual)           vmgn.py:56-64
//   z_{i+1} = relu(conv1_{i+1}(a_i) + b1_{i+1})      phase B, GEMM 2: written into the next block's patch in LDS; vmgn.py:48-50
//                                                    the last one goes to HBM instead
// As separate launches (conv3x3_half_kernel + bottleneck_seam_kernel<256,1024,256> per block) y_i and z_{i+1} cross HBM once each
// way, and every launch is a single resident round (256 frames = one workgroup per CU) whose first-load and store bursts are exposed.
//
// How it is put together -- two bodies that exist, composed without changing either's order of operations, so that a_n and
// z_{n+1} are bit-identical to the launches they replace:
//   * phase A is conv3x3_fat_kernel<1>'s slab body (conv3x3_fat.hip): the weight stream global -> 8-fragment VGPR ring behind the
//     counted waits of fat_ring_sched, the shifted frag_px / patch_g reads, the same (slab, tap, k-step, fragment) order. All four
//     64-channel slabs of the halo patch are resident (4 x 23 KiB), so the slab loop has no DMA and no barrier. Its 128 accumulator
//     registers are the AGPR quads a[64 : 192) that GEMM 2 owns in phase B and that are free between blocks.
//   * phase B is the seam's tile body (seam_dev.h, CHAIN = true): the y2 tile is resident, z pieces come back through `zpiece`.
//   * LDS: the patch (92 KB at 0) is dead once the 3x3 loop has ended; y2 (64 KB at 0) and X (64 KB at 64 K) are dead once GEMM 2's
//     last chunk has issued. Each hand-over stands behind one workgroup barrier; the peak is the seam kernel's 132 KB. Because y2
//     and X overwrite the patch, the 52 halo pixels of each slab are zeroed again behind every GEMM 2 (26 KB of LDS writes).
//   * block 1 fills the patch from z_1 in HBM with the fat kernel's LDS-DMA pieces (92 pieces, 23 per wave, zero source for the halo).
//   * every workgroup is self-contained: no flag, no spin-wait, nothing shared between workgroups.
// Measured (256 frames, fp16, one box, one call; profiles/l3_chain_ab.txt, l3_chain_before.txt, l3_chain_kernel_stats.txt): n = 4 takes
// 320 us (rocprofv3 median inside the step, min 315) against 372 us for the four conv3x3_half_kernel + four bottleneck_seam_kernel launches
// it replaces; the step 3.475 against 3.534 ms (medians of five alternated pairs; the slowest run with, 3.486, is ahead of the fastest
// without, 3.524; the spread without is 0.032). The estimate was 10-20 us per block from bursts and drains; the kernels gave 12 us per
// block and the seven launch gaps that went with them another ~3 us per block. The launch behind the chain (block 5's 3x3) lost ~10 us.
// Alone behind a cold conv1 (tools/chain_bench.py, HIP events, arms alternating): n = 1 82 us against 90 for its two launches, n = 2 162
// against 184, n = 4 302 against 362 -- the gain per block grows with the length of the chain (8 / 10 / 15 us), as it should when the
// first patch burst and the last z store are paid once per launch. n = 4 passed the dispatch rule at the first attempt, so n = 1 and
// n = 2 were not A/B-ed inside the step. Kept simple: block 1's whole patch
// is requested up front (92 KB per CU, once per launch) instead of slab by slab under the k-loop as the fat kernel does.
// A first build kept the lane's tap offsets alive across phase B: hipcc parked six values in a[0 : 6) -- the seam body's weight ring;
// tools/seam_check_isa.sh caught it, hence fresh_lane() below (236 VGPRs, no scratch, no compiler-allocated AGPR).
// The weights are the two existing packed forms (agrl_conv3x3_pack of a 256-channel tile, agrl_bottleneck_seam_pack); the launch
// reads a device table of per-block pointers (ChainBlock) that the host builds once at pack time.
#include "fat_dev.h"
#include "seam_dev.h"

namespace {

struct ChainBlock {             // one row of the device table: 8 pointers
    const unsigned char* w2;    // agrl_conv3x3_pack of conv2 (256 -> 256)
    const float* b2;
    const unsigned char* seam;  // agrl_bottleneck_seam_pack of (conv3, the next block's conv1)
    const float* b3;
    const float* b1n;
    const void* unused[3];
};
constexpr int CHAIN_MAX = 4;
struct ChainParams {
    const unsigned char* z1;    // (F, 16, 8, 256): conv1 output of the first chained block
    const ChainBlock* tab;
    unsigned char* a[CHAIN_MAX + 1];   // a[0]: the residual entering the chain; a[i]: block i's output (F, 16, 8, 1024), each its own buffer
    unsigned char* zout;        // (F, 16, 8, 256): conv1 output of the block behind the chain
    int n;
};

constexpr int CRING = 8;                 // weight fragments in flight per wave in phase A
constexpr int CFPS = 9 * 2 * 4;          // weight fragments per slab and wave: 9 taps x 2 k-steps x 4 channel fragments
constexpr int CPATCH = 23 * 1024;        // one slab of the halo patch: 18 x 10 pixels x 128 B, rounded to whole DMA pieces
constexpr int CSLABS = 4;                // 256 input channels
constexpr int CACC = 16;                 // phase A's accumulator quads: AGPR quads [16, 48) = GEMM 2's in phase B
constexpr auto CHAIN_SCHED = fat_ring_sched<CRING, CFPS>([](int) { return 0; });   // nothing but the ring is in flight
constexpr int CHAIN_LDS = seam_lds_bytes<256, 1024>();
static_assert(CSLABS * CPATCH <= CHAIN_LDS && CFPS % CRING == 0, "the patch fits where y2 and X live; a slab is whole ring turns");

__global__ __launch_bounds__(NWV * 64) void bottleneck_chain_kernel(const ChainParams p) {
    using std::integral_constant;
    __shared__ __attribute__((aligned(16))) unsigned char smem_[CHAIN_LDS];
    lds_u8_t* const smem = (lds_u8_t*)smem_;
    const unsigned lds0 = (unsigned)(size_t)smem;

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Lane coordinates are derived afresh wherever they are needed (seam_dev.h's epilogue does the same): phase B leaves no VGPR for
    // a value kept alive across it -- hipcc would park it in an AGPR, i.e. in the seam body's weight ring.
    auto fresh_lane = [] {
        unsigned l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return (int)l;
    };

    // ---- block 1's patch from z_1: piece pi = wave + 4 i of the 4 x 23 pieces (8 patch pixels x 128 B each), halo from the zero source
    {
        const int lane = fresh_lane();
        const unsigned char* zf = p.z1 + (size_t)blockIdx.x * (SBM * 256 * 2);
        const unsigned char* zsrc = reinterpret_cast<const unsigned char*>(&g_zero16);
#pragma unroll
        for (int i = 0; i < 23; ++i) {
            const int pi = wave + 4 * i;
            const int slab = pi / 23, piece = pi - slab * 23;
            const int row = piece * 8 + (lane >> 3);
            const int py = row / 10, px = row - py * 10;
            const bool ok = row < 180 && (unsigned)(py - 1) < 16u && (unsigned)(px - 1) < 8u;
            const unsigned off = (unsigned)(((py - 1) * 8 + (px - 1)) * 512 + slab * 128 + (((lane & 7) ^ patch_g(py, px)) << 4));
            fat_dma(ok ? zf + off : zsrc, __builtin_amdgcn_readfirstlane(lds0 + slab * CPATCH + piece * 1024));
        }
    }

    asm volatile("" ::: "a255");
    for (int i = 0; i < p.n; ++i) {
        const ChainBlock blk = p.tab[i];
        const int lane = fresh_lane();
        const unsigned lane16 = (unsigned)lane * 16u;
        const int frow = lane & 15, fchunk = lane >> 4;
        // pixel fragment b = pixels 16 b + frag_px(lane & 15): patch pixel (2 b + r0 + tr, x0 + ts) at tap (tr, ts) (conv3x3_fat.hip)
        const int fp = frag_px(frow);
        int tbase[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) tbase[t] = patch_off<10>((fp >> 3) + t / 3, (fp & 7) + t % 3, fchunk);

        // ================= phase A: y_i = relu(conv3x3(z_i) + b2) on the resident patch =================
        sfor<32>([&](auto qc) { fat_zero<CACC + decltype(qc)::value>(); });
        const unsigned char* wstream = blk.w2 + (size_t)wave * CSLABS * (CFPS * 1024);
        u32x4_t wr[CRING];
        auto issue_w = [&](auto slot_c, const unsigned char* slab_base, auto pos_c) {
            constexpr int SLOT = decltype(slot_c)::value, POS = decltype(pos_c)::value;
            fat_gload<(POS & 3) * 1024>(wr[SLOT], lane16, slab_base + (POS & ~3) * 1024);
        };
        sfor<CRING>([&](auto ic) { issue_w(ic, wstream, ic); });
        // block 1: this wave's patch pieces are older than the ring; later blocks: its z pieces and halo cells are LDS writes. The
        // barrier covers the other waves'.
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CRING) : "memory");
        wg_barrier();

        u32x4_t xf[8];
#pragma nounroll
        for (int slab = 0; slab < CSLABS; ++slab) {
            const unsigned char* ws = wstream + (size_t)slab * (CFPS * 1024);
            const unsigned char* wsn = wstream + (size_t)(slab + 1 < CSLABS ? slab + 1 : 0) * (CFPS * 1024);  // past the end: slab 0 again (never used)
            const lds_u8_t* sp = smem + slab * CPATCH;
            auto ldx = [&](auto ks_c, auto b_c) {
                constexpr int KS = decltype(ks_c)::value, B = decltype(b_c)::value;
                return *reinterpret_cast<const lds_u32x4_t*>(sp + (tbase[KS >> 1] ^ ((KS & 1) * 64)) + B * 2560);
            };
            sfor<8>([&](auto bc) { xf[decltype(bc)::value] = ldx(integral_constant<int, 0>{}, bc); });
            sfor<CFPS>([&](auto pc) {
                constexpr int P = decltype(pc)::value;
                constexpr int KS = P >> 2, A = P & 3, SL = P % CRING;
                fat_wait<CHAIN_SCHED.allowed[P]>(wr[SL]);
                sfor<8>([&](auto bc) {
                    constexpr int B = decltype(bc)::value;
                    fat_mfma<CACC + A * 8 + B>(wr[SL], xf[B]);
                    if constexpr (A == 3 && KS + 1 < 18) {  // the next k-step's fragment replaces this one right behind its last reader
                        __builtin_amdgcn_sched_barrier(0);
                        xf[B] = ldx(integral_constant<int, KS + 1>{}, bc);
                    }
                });
                __builtin_amdgcn_sched_barrier(0);
                constexpr int Q = P + CRING;
                if constexpr (Q >= CFPS) issue_w(integral_constant<int, SL>{}, wsn, integral_constant<int, Q - CFPS>{});
                else issue_w(integral_constant<int, SL>{}, ws, integral_constant<int, Q>{});
            });
        }
        // The drain's vmcnt(0) is also the residual stream's guard. In phase B this wave loads a_{i-1} at exactly the addresses it
        // stored in the previous block (the seam body gives a wave the same 64 channels of every chunk, as loads and as stores): those
        // stores are acknowledged by L2 once vmcnt has counted them down, and no line of a_{i-1} can sit stale in this CU's vector L1,
        // because every a_i is its own buffer that nothing in this launch has loaded from before it was written.
        fat_ring_drain(wr);

        wg_barrier();   // every wave is past its patch reads: the y2 tile may overwrite the patch
        {
            // + bias, ReLU, round once; lane (f, pixel m = 16 b + fp) holds channels 64 wave + 32 j + 8 f .. + 7: k-tile `wave` of the
            // seam body's resident y2 layout, 128-byte rows, 16-byte piece (4 j + f) ^ ((m >> 1) & 7)
            const lds_u8_t* yw = smem + wave * 16384 + fp * 128;
            const int sw = (fp >> 1) & 7;
            sfor<2>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const float4 b0 = *reinterpret_cast<const float4*>(blk.b2 + wave * 64 + 8 * fchunk + 32 * j);
                const float4 b1 = *reinterpret_cast<const float4*>(blk.b2 + wave * 64 + 8 * fchunk + 32 * j + 4);
                sfor<8>([&](auto bc) {
                    constexpr int B = decltype(bc)::value;
                    float v[8];
                    fat_bias8<CACC + (2 * j) * 8 + B, CACC + (2 * j + 1) * 8 + B>(v, 1.f, b0, b1);
                    fat_relu8(v, 1);
                    const uint4 pk = fat_pack8(v);
                    *reinterpret_cast<lds_u32x4_t*>(const_cast<lds_u8_t*>(yw) + B * 2048 + (((4 * j + fchunk) ^ sw) << 4)) = u32x4_t{pk.x, pk.y, pk.z, pk.w};
                });
            });
        }
        wg_barrier();   // the y2 tile is complete

        // ================= phase B: a_i and z_{i+1} (seam_dev.h) =================
        SeamParams sp;
        sp.y2 = nullptr;
        sp.wpk = blk.seam;
        sp.b3 = blk.b3;
        sp.res = i == 0 ? p.a[0] : i == 1 ? p.a[1] : i == 2 ? p.a[2] : p.a[3];
        sp.out = i == 0 ? p.a[1] : i == 1 ? p.a[2] : i == 2 ? p.a[3] : p.a[4];
        sp.b1n = blk.b1n;
        sp.z = i + 1 == p.n ? p.zout : nullptr;
        sp.M = 0;
        // z_{i+1}: pixel 16 b + frow of the frame = patch pixel (2 b + 1 + (frow >> 3), 1 + (frow & 7)); channels 64 wave + 32 j +
        // 8 fchunk .. + 7 = piece 4 j + fchunk of slab `wave` (the swizzle term does not depend on b: two patch rows per fragment)
        const lds_u8_t* zw = smem + wave * CPATCH;
        seam_tile<256, 1024, 256, true>(sp, smem, [&](auto jc, auto bc, const uint4& pk, int lane_z) {
            constexpr int j = decltype(jc)::value, b = decltype(bc)::value;
            const int frow = lane_z & 15, fchunk = lane_z >> 4;
            *reinterpret_cast<lds_u32x4_t*>(const_cast<lds_u8_t*>(zw) + b * 2560 + patch_off<10>(1 + (frow >> 3), 1 + (frow & 7), 4 * j + fchunk)) =
                u32x4_t{pk.x, pk.y, pk.z, pk.w};
        });
        // y2 and X have overwritten the patch's halo: zero the 52 halo pixels of every slab again (8 16-byte cells each). The cells
        // are disjoint from the z pieces; the barrier at the top of the next phase A publishes both.
        for (int h = wave * 64 + fresh_lane(); h < CSLABS * 52 * 8; h += NWV * 64) {
            const int hp = (h >> 3) % 52, slab = (h >> 3) / 52;
            int py, px;
            if (hp < 20) { py = hp < 10 ? 0 : 17; px = hp < 10 ? hp : hp - 10; }
            else { py = 1 + ((hp - 20) >> 1); px = ((hp - 20) & 1) * 9; }
            *reinterpret_cast<lds_u32x4_t*>(smem + slab * CPATCH + (py * 10 + px) * 128 + (h & 7) * 16) = u32x4_t{0u, 0u, 0u, 0u};
        }
    }
}

}  // namespace

extern "C" int agrl_bottleneck_chain_enabled(int frames) {
    const int want = agrl_opts().l3_chain;
    if (agrl_opt_set(want)) return want != 0;
    // Default: where it was measured and won (256 frames, one workgroup per CU: profiles/l3_chain_ab.txt) down to half a chip of
    // frames; smaller batches keep the separate launches.
    return frames >= agrl_cu_count() / 2;
}

extern "C" int agrl_bottleneck_chain(const void* z1, const void* a0, const void* table, void* const* a_out, void* z_out, int frames, int n,
                                     agrl_stream_t stream) {
    AGRL_CHECK_ARG(z1 && a0 && table && a_out && z_out, "agrl_bottleneck_chain: null pointer");
    AGRL_CHECK_ARG(n >= 1 && n <= CHAIN_MAX, "agrl_bottleneck_chain: 1 to %d chained blocks, got %d", CHAIN_MAX, n);
    AGRL_CHECK_ARG(frames > 0 && (size_t)frames * SBM * 1024 * 2 < (1ull << 32), "agrl_bottleneck_chain: maps beyond 4 GB are not addressed");
    ChainParams p;
    p.z1 = reinterpret_cast<const unsigned char*>(z1);
    p.tab = reinterpret_cast<const ChainBlock*>(table);
    for (int i = 0; i <= CHAIN_MAX; ++i) p.a[i] = nullptr;
    p.a[0] = reinterpret_cast<unsigned char*>(const_cast<void*>(a0));
    for (int i = 0; i < n; ++i) p.a[i + 1] = reinterpret_cast<unsigned char*>(a_out[i]);
    p.zout = reinterpret_cast<unsigned char*>(z_out);
    p.n = n;
    const size_t abytes = (size_t)frames * SBM * 1024 * 2;
    uintptr_t al = (uintptr_t)z1 | (uintptr_t)table | (uintptr_t)z_out;
    for (int i = 0; i <= n; ++i) {
        AGRL_CHECK_ARG(p.a[i], "agrl_bottleneck_chain: null pointer");
        al |= (uintptr_t)p.a[i];
        // a wave reads back only what it stored itself, from a buffer nothing in the launch has loaded before: every a_i on its own
        for (int k = 0; k < i; ++k) {
            const uintptr_t lo = (uintptr_t)p.a[i] < (uintptr_t)p.a[k] ? (uintptr_t)p.a[i] : (uintptr_t)p.a[k];
            const uintptr_t hi = (uintptr_t)p.a[i] < (uintptr_t)p.a[k] ? (uintptr_t)p.a[k] : (uintptr_t)p.a[i];
            AGRL_CHECK_ARG(hi - lo >= abytes, "agrl_bottleneck_chain: the residual-stream buffers must not overlap");
        }
    }
    AGRL_CHECK_ARG((al & 15) == 0, "agrl_bottleneck_chain: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(bottleneck_chain_kernel, dim3(frames), dim3(NWV * 64), 0, (hipStream_t)stream, p);
    AGRL_CHECK_LAUNCH("agrl_bottleneck_chain");
    return 0;
}
