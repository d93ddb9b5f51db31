// The pixel tile and the k-loop of the four-wave 1x1 kernels (conv1x1_fat.hip: 256 pixel rows per workgroup, conv1x1_duo.hip: 128, one-shot
// and persistent), stated once. A workgroup's tile is 16 NB pixel rows x 256 channels: wave w owns 64 channels (4 MFMA A fragments) of all
// rows (NB B fragments of 16 rows), weights from agrl_conv1x1_pack's fragment streams through an 8-fragment VGPR ring, the pixel rows of the
// current / next 128-channel slab in two LDS buffers by LDS-DMA, one barrier per slab. What the kernels keep: the LDS carve-up, the
// prologue, which tile / slab / buffer comes next, and the epilogue's data movement.
#pragma once
#include "fat_dev.h"

namespace {

constexpr int F1RING = 8;        // weight fragments in flight per wave
constexpr int F1PS = 4 * 4;      // weight fragments per 128-channel slab and wave: 4 k-steps x 4 channel fragments
// Slab s is read during the weight fragments 0 .. 15 of slab s -- its LAST k-step's pixel fragments behind fragment 11 -- and the
// first k-step of slab s + 1 behind fragment 15. One barrier per slab, in front of fragment 12: there every wave has issued (and
// waited out) its last reads of slab s's buffer and has waited for its own pieces of slab s + 1 (requested behind fragments
// 12 .. 15 of slab s - 1, i.e. older than the weight fragments it has consumed since), so behind the barrier (a) slab s + 1 is
// complete for everybody and (b) slab s's buffer is free: the pieces of slab s + 2 go into it behind fragments 12 .. 15, a quarter of
// the wave's pieces each. No wave ever waits for LDS data at a slab boundary.
constexpr int F1BARRIER_AT = 12;
// timing ablations of the slab body (results wrong; the kernels map their -DDUO_ABL / -DFAT1_ABL bits onto these)
constexpr int F1_NO_MFMA = 1, F1_NO_WLOAD = 2, F1_NO_DMA = 4, F1_NO_LDSREAD = 8;

template <int NB>   // DMA pieces issued behind weight fragment p: a quarter of the wave's NB behind each of the fragments 12 .. 15
constexpr int f1_pieces_at(int p) { return p >= F1BARRIER_AT ? NB / 4 : 0; }
template <int NB>
constexpr auto F1_SCHED = fat_ring_sched<F1RING, F1PS>(f1_pieces_at<NB>);

template <int NB>   // pixel fragments per wave: 16 (conv1x1_fat_kernel) / 8 (the duo kernels)
struct Fat1x1 {
    static constexpr int ROWS = 16 * NB;        // pixel rows per tile
    static constexpr int HALF = ROWS * 128;     // bytes of one 64-channel half of a slab: ROWS rows x 128 B
    static constexpr int SLAB = 2 * HALF;       // one 128-channel slab of the pixel tile
    static constexpr int PPW = NB;              // DMA pieces (8 rows x 128 B) per wave and slab
    static constexpr int pieces_at(int p) { return f1_pieces_at<NB>(p); }
    static constexpr int piece_first(int p) { int n = 0; for (int q = 0; q < p; ++q) n += pieces_at(q); return n; }

    // rows are 128 bytes of 16-byte chunks, chunk c of row r at c ^ ((r >> 1) & 7) (igemm_kernel's layout): byte offset of chunk c
    static __device__ __forceinline__ unsigned swz(int row, int chunk) { return (unsigned)((chunk ^ ((row >> 1) & 7)) << 4); }
    // pixel fragment b (rows 16 b + (lane & 15)) of k-step kk: half kk >> 1, chunk 4 (kk & 1) + (lane >> 4)
    static __device__ __forceinline__ int xbase(int frow, int fchunk) { return frow * 128 + (int)swz(frow, fchunk); }
    template <int KS, int B>
    static __device__ __forceinline__ u32x4_t ldx(const lds_u8_t* sp, int xb) {
        const lds_u8_t* a = sp + (xb ^ ((KS & 1) * 64));
        return *reinterpret_cast<const lds_u32x4_t*>(a + (KS >> 1) * HALF + B * 2048);
    }
    // piece I = 2 j + h of this wave -> rows (wave + 4 j) * 8 .. + 7 of 64-channel half h of buffer `buf`; lane (lrow = lane >> 3,
    // lchk = lane & 7) brings chunk lchk ^ swizzle(row) of its row: `src` = that chunk's address
    template <int I>
    static __device__ __forceinline__ void stage(const unsigned char* src, unsigned lds0, int buf, int wave) {
        fat_dma(src, __builtin_amdgcn_readfirstlane(lds0 + buf * SLAB + (I & 1) * HALF + (wave + 4 * (I >> 1)) * 1024));
    }
    // weight fragment POS of the slab at slab_base -> ring slot `slot`
    template <int POS>
    static __device__ __forceinline__ void issue_w(u32x4_t& slot, unsigned lane16, const unsigned char* slab_base) {
        fat_gload<(POS & 3) * 1024>(slot, lane16, slab_base + (POS & ~3) * 1024);
    }

    // One slab of the k-loop: the 16 weight fragments of the slab at `ws` against the pixel rows in buffer `sp`; behind each fragment's MFMAs
    // its ring slot is refilled (fragments 8 .. 15 of this slab, then 0 .. 7 of the slab at `wsn`), behind fragments 12 .. 15 stage_piece(ic)
    // requests pieces ic = 0 .. PPW - 1 of the slab after next into the buffer this slab leaves. `spn`: the next slab's buffer (its first
    // k-step's fragments replace this slab's last). The counted waits hold for exactly this issue order. (The two register arrays come by
    // reference into a function that is always inlined; whatever else a kernel's stage_piece reads it must hold in scalars captured by
    // value or element by element -- an array a lambda reaches through a reference or a select between two arrays' elements lives in
    // scratch, and a scratch access is a vector-memory operation that would sit in the counted vmcnt queue: conv1x1_duo_persist_kernel.)
    template <int ABL, typename STAGE>
    static __device__ __forceinline__ void slab(u32x4_t (&wr)[F1RING], u32x4_t (&xf)[NB], const lds_u8_t* sp, const lds_u8_t* spn, int xb,
                                                const unsigned char* ws, const unsigned char* wsn, unsigned lane16, STAGE&& stage_piece) {
        using std::integral_constant;
        sfor<F1PS>([&](auto pc) {
            constexpr int P = decltype(pc)::value;
            constexpr int KS = P >> 2, A = P & 3, SL = P % F1RING;
            fat_wait<F1_SCHED<NB>.allowed[P]>(wr[SL]);
            if constexpr (P == F1BARRIER_AT) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
            sfor<NB>([&](auto bc) {
                constexpr int B = decltype(bc)::value;
                if constexpr (!(ABL & F1_NO_MFMA)) fat_mfma<A * NB + B>(wr[SL], xf[B]);
                if constexpr (A == 3 && !(ABL & F1_NO_LDSREAD)) {  // the next k-step's fragment replaces this one right behind its last reader
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (KS + 1 < 4) xf[B] = ldx<KS + 1, B>(sp, xb);
                    else xf[B] = ldx<0, B>(spn, xb);
                }
            });
            __builtin_amdgcn_sched_barrier(0);
            constexpr int Q = P + F1RING;
            if constexpr (!(ABL & F1_NO_WLOAD)) {
                if constexpr (Q >= F1PS) issue_w<Q - F1PS>(wr[SL], lane16, wsn);
                else issue_w<Q>(wr[SL], lane16, ws);
            }
            if constexpr (!(ABL & F1_NO_DMA))
                sfor<pieces_at(P)>([&](auto ic) { stage_piece(integral_constant<int, piece_first(P) + decltype(ic)::value>{}); });
        });
    }
};

}  // namespace
