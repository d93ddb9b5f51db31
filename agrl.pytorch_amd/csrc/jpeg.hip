// Baseline JPEG decode on the device, bit-exact with Pillow's Image.open().convert('RGB') (libjpeg-turbo): the reference's frame read
// (dataset_loader.py:23-36) in front of the resample / normalise / stem chain. The host (torchreid/device_decode.py) parses headers and
// hands over one byte buffer of entropy-coded scans, one descriptor row per frame and the interned quantisation / Huffman tables; it
// never touches an entropy-coded bit. Three launches, each a function of the descriptor rows alone:
//   1. jpeg_entropy_kernel   one wavefront per frame. The 64 lanes share what is parallel -- staging the frame's Huffman and
//                            quantisation tables into LDS, zero-filling its coefficient blocks -- then ONE lane walks the symbol chain
//                            (serial by construction: a code's position is known only when the one before it is decoded): ITU T.81
//                            Huffman decode with libjpeg's 9-bit look-ahead + maxcode / valoffset tables, DC prediction, run / size AC
//                            with ZRL and EOB, restart intervals; every coefficient dequantised into the int16 workspace
//                            [frame][component][block (raster)][64 (natural order)]
//   2. jpeg_idct_kernel      one 8x8 block per thread: libjpeg's accurate integer IDCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2,
//                            columns then rows in int32, + 128, clamp) into uint8 samples, block-major like the coefficients
//   3. jpeg_colour_kernel    one output pixel per thread: libjpeg's "fancy" (triangle) chroma upsampling on the component planes
//                            cropped to the image, edges replicated, then its 16-bit fixed-point YCbCr -> RGB, channel-last into the
//                            frame's valid extent of the (F, Hc, Wc, 3) container; the rest of the frame's slot is zeroed
// torchreid/hip_ops.py: jpeg_decode_reference is the same arithmetic in numpy, and the definition these kernels are held to.
//
// HARD CONTRACT: no address is formed from stream contents without a range check. The bit reader returns zeros beyond the scan's
// length (and reads the byte buffer only in aligned 8-byte words inside the padding the host checked); a coefficient's index is
// checked against 64; block counts and block positions come from the descriptor's H, W and sampling code, never from the stream; the
// descriptor rows are validated by the entry point on its host copy before any launch and AGAIN by every kernel on the device copy
// (frame_ok): a frame that fails is skipped with status 5. A frame whose status is non-zero has written only inside its own workspace
// slice and its own container slot.
#include "agrl_common.h"

namespace {
constexpr int DESC = 16;            // ints per descriptor row
constexpr int HUFF_WORDS = 360;     // ints per decode-ready Huffman table: look[512] u16 | maxcode[17] | valoffset[17] | huffval[256] u8
constexpr int H_MAXCODE = 256, H_VALOFF = 273, H_VAL = 290;
constexpr int LOOK_BITS = 9;
constexpr int MAX_DIM = 4096;
constexpr int MAX_FRAMES = 65535;   // gridDim.y of the IDCT / colour launches
constexpr int MAX_WS_BLOCKS = 1 << 24;
enum { D_OFF = 0, D_LEN = 1, D_H = 2, D_W = 3, D_SAMP = 4, D_RI = 5, D_Q0 = 6, D_DC0 = 9, D_AC0 = 12, D_WS = 15 };
enum { SAMP_GRAY = 0, SAMP_444 = 1, SAMP_422 = 2, SAMP_420 = 3 };
enum { ST_OK = 0, ST_END = 1, ST_CODE = 2, ST_INDEX = 3, ST_MARKER = 4, ST_DESC = 5 };
enum { STAGE_ENTROPY = 1, STAGE_IDCT = 2, STAGE_COLOUR = 4 };

struct Limits {   // what a descriptor row is checked against
    long long scan_bytes;
    int NQ, NH, ws_blocks, Hc, Wc;
};

struct Geom {
    int ncomp, h0, v0, mx, my;
    int bw[3], bh[3], ph[3], pw[3];   // per component: blocks per row, block rows, cropped plane height / width
    int base[4];                      // first block of each component inside the frame's workspace slice; base[ncomp] = blocks
};

// The one validity predicate of a descriptor row: the entry point applies it to the host copy, every kernel to the device copy.
__host__ __device__ inline bool frame_ok(const int* d, const Limits& lim, Geom& g) {
    const int H = d[D_H], W = d[D_W], samp = d[D_SAMP];
    if (H < 1 || H > MAX_DIM || W < 1 || W > MAX_DIM || samp < SAMP_GRAY || samp > SAMP_420) return false;
    if (H > lim.Hc || W > lim.Wc) return false;
    g.ncomp = samp == SAMP_GRAY ? 1 : 3;
    g.h0 = samp >= SAMP_422 ? 2 : 1;
    g.v0 = samp == SAMP_420 ? 2 : 1;
    g.mx = (W + 8 * g.h0 - 1) / (8 * g.h0);
    g.my = (H + 8 * g.v0 - 1) / (8 * g.v0);
    g.base[0] = 0;
    for (int c = 0; c < 3; ++c) {
        const int hc = c == 0 ? g.h0 : 1, vc = c == 0 ? g.v0 : 1;
        g.bw[c] = g.mx * hc;
        g.bh[c] = g.my * vc;
        g.ph[c] = c == 0 ? H : (H + g.v0 - 1) / g.v0;
        g.pw[c] = c == 0 ? W : (W + g.h0 - 1) / g.h0;
        g.base[c + 1] = g.base[c] + (c < g.ncomp ? g.bw[c] * g.bh[c] : 0);   // at most 3 * 512 * 512 blocks
    }
    const long long off = d[D_OFF], len = d[D_LEN];
    if (off < 0 || len < 0 || (off & 7) != 0 || off + ((len + 7) & ~7LL) + 8 > lim.scan_bytes) return false;   // whole words, one beyond
    if (d[D_RI] < 0 || d[D_RI] > 65535) return false;
    for (int c = 0; c < g.ncomp; ++c) {
        if (d[D_Q0 + c] < 0 || d[D_Q0 + c] >= lim.NQ) return false;
        if (d[D_DC0 + c] < 0 || d[D_DC0 + c] >= lim.NH || d[D_AC0 + c] < 0 || d[D_AC0 + c] >= lim.NH) return false;
    }
    if (d[D_WS] < 0 || (long long)d[D_WS] + g.base[g.ncomp] > lim.ws_blocks) return false;
    return true;
}

// ---- stage 1: the bit reader and the symbol walk (one lane; __host__ too, so that the walk can be checked on a CPU) -------------------
// A 64-bit window refilled bytewise; FF 00 is a stuffed FF. At any other marker and at the end of the scan it stops consuming and feeds
// zero bits, counting them in ``fed``: a symbol that used one of those has passed the end (passed_end()).
struct Bits {
    const unsigned char* d;   // 8-byte aligned; whole words are readable up to the one behind byte n - 1
    int n, p;
    unsigned long long acc, word;
    int nb, fed, widx;
    bool marker;

    __host__ __device__ inline void init(const unsigned char* data, int len) {
        d = data, n = len, p = 0, acc = 0, word = 0, nb = 0, fed = 0, widx = -1, marker = false;
    }
    __host__ __device__ inline unsigned byte(int i) {   // 0 <= i < n, checked by the callers
        const int w = i >> 3;
        if (w != widx) {
            word = *reinterpret_cast<const unsigned long long*>(d + 8 * (size_t)w);
            widx = w;
        }
        return (unsigned)(word >> (8 * (i & 7))) & 255u;
    }
    __host__ __device__ inline void fill() {
        while (nb <= 56) {
            unsigned b = 0;
            if (!marker && p < n) {
                b = byte(p);
                if (b == 0xFFu) {
                    const unsigned nxt = p + 1 < n ? byte(p + 1) : 0xFFu;   // a lone FF at the very end counts as a marker
                    if (nxt == 0) {
                        p += 2;
                    } else {
                        marker = true, b = 0, fed += 8;
                    }
                } else {
                    p += 1;
                }
            } else {
                fed += 8;
            }
            acc = (acc << 8) | b;
            nb += 8;
        }
    }
    __host__ __device__ inline unsigned peek(int k) const { return (unsigned)(acc >> (nb - k)) & ((1u << k) - 1u); }   // k <= 16 <= nb
    __host__ __device__ inline void skip(int k) { nb -= k; }
    __host__ __device__ inline bool passed_end() const { return nb < fed; }
    // byte-align and consume FF D0+index; false when whole bytes still stand in front of the marker or it is not there
    __host__ __device__ inline bool restart(int index) {
        if (nb - fed >= 8 || p + 1 >= n || byte(p) != 0xFFu || byte(p + 1) != 0xD0u + (unsigned)(index & 7)) return false;
        p += 2, acc = 0, nb = 0, fed = 0, marker = false;
        return true;
    }
};

// one Huffman symbol out of a decode-ready table; the code's length, 0 when the next 16 bits are no code of the table
__host__ __device__ inline int huff_symbol(const int* t, unsigned window, unsigned& sym) {
    const unsigned e = reinterpret_cast<const unsigned short*>(t)[window >> (16 - LOOK_BITS)];
    if (e) {
        sym = e & 255u;
        return (int)(e >> 8);
    }
    for (int l = LOOK_BITS + 1; l <= 16; ++l) {
        const int code = (int)(window >> (16 - l));
        if (code <= t[H_MAXCODE + l]) {
            sym = reinterpret_cast<const unsigned char*>(t + H_VAL)[(code + t[H_VALOFF + l]) & 255];
            return l;
        }
    }
    return 0;
}

// The symbol walk of one scan into the frame's coefficient slice (zeroed beforehand). tables: six decode-ready Huffman tables, the
// components' DC tables and then their AC tables; q: their three quantisation tables; zz: the natural index of the k-th coefficient of
// the stream. Returns the frame's status.
__host__ __device__ inline int decode_scan(Bits& br, const Geom& g, int ri, const int* tables, const unsigned short* q,
                                           const unsigned char* zz, short* coef) {
    int pred[3] = {0, 0, 0};
    int since = 0, intervals = 0, mrow = 0, mcol = 0;
    const int mcus = g.mx * g.my;
    for (int m = 0; m < mcus; ++m) {
        if (ri > 0 && since == ri) {
            if (!br.restart(intervals)) return ST_MARKER;
            ++intervals, since = 0;
            pred[0] = pred[1] = pred[2] = 0;
        }
        ++since;
        for (int c = 0; c < g.ncomp; ++c) {
            const int hc = c == 0 ? g.h0 : 1, vc = c == 0 ? g.v0 : 1;
            for (int blk = 0; blk < hc * vc; ++blk) {
                // mrow < my, mcol < mx: the block lies inside the component's bw x bh blocks, whatever the stream holds
                short* out = coef + 64 * (size_t)(g.base[c] + (mrow * vc + blk / hc) * g.bw[c] + mcol * hc + blk % hc);
                int k = 0;
                while (k < 64) {
                    br.fill();
                    unsigned sym = 0;
                    const int l = huff_symbol(tables + (k == 0 ? c : 3 + c) * HUFF_WORDS, br.peek(16), sym);
                    if (l == 0) return ST_CODE;
                    br.skip(l);
                    const int r = k == 0 ? 0 : (int)(sym >> 4), s = (int)(sym & 15u);
                    if (k != 0 && s == 0) {
                        if (br.passed_end()) return br.marker ? ST_MARKER : ST_END;
                        if (r != 15) break;   // EOB
                        k += 16;              // ZRL
                        if (k > 64) return ST_INDEX;
                        continue;
                    }
                    k += r;
                    if (k > 63) return ST_INDEX;
                    int v = 0;
                    if (s) {
                        v = (int)br.peek(s);
                        if (v < (1 << (s - 1))) v = v - (1 << s) + 1;   // EXTEND
                    }
                    br.skip(s);
                    if (br.passed_end()) return br.marker ? ST_MARKER : ST_END;
                    if (k == 0) v = pred[c] = (int)((unsigned)pred[c] + (unsigned)v);
                    const int at = zz[k] & 63;
                    out[at] = (short)(unsigned short)((unsigned)v * (unsigned)q[64 * c + at]);   // stored as int16: the low 16 bits
                    ++k;
                }
            }
        }
        if (++mcol == g.mx) mcol = 0, ++mrow;
    }
    return ST_OK;
}

#define AGRL_JPEG_ZIGZAG                                                                                                              \
    {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, \
     57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
__device__ const unsigned char kZigzag[64] = AGRL_JPEG_ZIGZAG;

__global__ __launch_bounds__(AGRL_WAVE) void jpeg_entropy_kernel(const unsigned char* __restrict__ scans, const int* __restrict__ desc,
                                                                 const unsigned short* __restrict__ quant, const int* __restrict__ huff,
                                                                 short* __restrict__ coef_ws, int* __restrict__ status, Limits lim) {
    __shared__ int s_huff[6][HUFF_WORDS];   // DC tables of the components, then their AC tables
    __shared__ unsigned short s_q[3][64];
    __shared__ unsigned char s_zz[64];
    __shared__ int s_d[DESC];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (lane < DESC) s_d[lane] = desc[(size_t)f * DESC + lane];
    __syncthreads();
    Geom g;
    if (!frame_ok(s_d, lim, g)) {   // wave-uniform
        if (lane == 0) status[f] = ST_DESC;
        return;
    }
    for (int c = 0; c < g.ncomp; ++c) {
        const int* dc = huff + (size_t)s_d[D_DC0 + c] * HUFF_WORDS;
        const int* ac = huff + (size_t)s_d[D_AC0 + c] * HUFF_WORDS;
        for (int i = lane; i < HUFF_WORDS; i += AGRL_WAVE) s_huff[c][i] = dc[i], s_huff[3 + c][i] = ac[i];
        s_q[c][lane] = quant[(size_t)s_d[D_Q0 + c] * 64 + lane];
    }
    s_zz[lane] = kZigzag[lane];
    short* coef = coef_ws + 64 * (size_t)s_d[D_WS];
    uint4* fill = reinterpret_cast<uint4*>(coef);   // 128 bytes per block, the workspace 16-byte aligned
    const int fill_n = g.base[g.ncomp] * 8;
    for (int i = lane; i < fill_n; i += AGRL_WAVE) fill[i] = make_uint4(0, 0, 0, 0);
    __threadfence();   // the zeros have landed before the one lane stores coefficients over them
    __syncthreads();
    if (lane != 0) return;
    Bits br;
    br.init(scans + s_d[D_OFF], s_d[D_LEN]);
    status[f] = decode_scan(br, g, s_d[D_RI], &s_huff[0][0], &s_q[0][0], s_zz, coef);
}

// ---- stage 2: libjpeg's accurate integer IDCT (jidctint.c) ----------------------------------------------------------------------------
// One 1-D pass over x[0..7], descaled by a rounding right shift. Products and sums wrap in 32 bits (unsigned arithmetic: defined), as the
// restatement's int32 arrays do; inside the definition -- coefficients an encoder produces -- nothing comes near the range.
__host__ __device__ inline void idct_pass(int* x, int shift) {
    typedef unsigned U;
    const U x0 = (U)x[0], x1 = (U)x[1], x2 = (U)x[2], x3 = (U)x[3], x4 = (U)x[4], x5 = (U)x[5], x6 = (U)x[6], x7 = (U)x[7];
    U z1 = (x2 + x6) * 4433u;
    U tmp2 = z1 - x6 * 15137u, tmp3 = z1 + x2 * 6270u;
    U tmp0 = (x0 + x4) << 13, tmp1 = (x0 - x4) << 13;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x7, tmp1 = x5, tmp2 = x3, tmp3 = x1;
    z1 = tmp0 + tmp3;
    U z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 *= (U)-7373, z2 *= (U)-20995, z3 = z3 * (U)-16069 + z5, z4 = z4 * (U)-3196 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const U half = 1u << (shift - 1);
    x[0] = (int)(tmp10 + tmp3 + half) >> shift, x[7] = (int)(tmp10 - tmp3 + half) >> shift;
    x[1] = (int)(tmp11 + tmp2 + half) >> shift, x[6] = (int)(tmp11 - tmp2 + half) >> shift;
    x[2] = (int)(tmp12 + tmp1 + half) >> shift, x[5] = (int)(tmp12 - tmp1 + half) >> shift;
    x[3] = (int)(tmp13 + tmp0 + half) >> shift, x[4] = (int)(tmp13 - tmp0 + half) >> shift;
}

// 64 dequantised coefficients (natural order) -> 64 samples, row-major
__host__ __device__ inline void idct_block(const short* in, unsigned char* out) {
    int ws[64];
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = in[8 * r + col];
        idct_pass(x, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[8 * r + col] = x[r];
    }
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        idct_pass(ws + 8 * row, 18);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int v = ws[8 * row + c] + 128;
            out[8 * row + c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    }
}

constexpr int NTH = 256;

__global__ __launch_bounds__(NTH) void jpeg_idct_kernel(const int* __restrict__ desc, const short* __restrict__ coef_ws,
                                                        unsigned char* __restrict__ samples_ws, Limits lim) {
    const int f = blockIdx.y;
    Geom g;
    if (!frame_ok(desc + (size_t)f * DESC, lim, g)) return;
    const int b = blockIdx.x * NTH + threadIdx.x;
    if (b >= g.base[g.ncomp]) return;
    const size_t blk = (size_t)desc[(size_t)f * DESC + D_WS] + b;
    __attribute__((aligned(16))) short in[64];
    __attribute__((aligned(16))) unsigned char out[64];
    const uint4* src = reinterpret_cast<const uint4*>(coef_ws + 64 * blk);
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<uint4*>(in)[i] = src[i];
    idct_block(in, out);
    uint4* dst = reinterpret_cast<uint4*>(samples_ws + 64 * blk);
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = reinterpret_cast<const uint4*>(out)[i];
}

// ---- stage 3: fancy upsampling + colour ------------------------------------------------------------------------------------------------
// sample (yy, xx) of component c: 0 <= yy < ph[c] <= 8 bh[c], 0 <= xx < pw[c] <= 8 bw[c], by the callers' clamps
__host__ __device__ inline int plane_at(const unsigned char* s, const Geom& g, int c, int yy, int xx) {
    return s[64 * (size_t)(g.base[c] + (yy >> 3) * g.bw[c] + (xx >> 3)) + 8 * (yy & 7) + (xx & 7)];
}

// the chroma sample of component c at image pixel (y, x): libjpeg's h2v1 / h2v2 triangle filters, the cropped plane's edges replicated
__host__ __device__ inline int chroma_at(const unsigned char* s, const Geom& g, int samp, int c, int y, int x) {
    if (samp == SAMP_444) return plane_at(s, g, c, y, x);
    const int i = x >> 1, odd = x & 1;
    int ni = odd ? i + 1 : i - 1;
    ni = ni < 0 ? 0 : (ni > g.pw[c] - 1 ? g.pw[c] - 1 : ni);
    if (samp == SAMP_422) return (3 * plane_at(s, g, c, y, i) + plane_at(s, g, c, y, ni) + (odd ? 2 : 1)) >> 2;
    const int r = y >> 1;
    int nr = (y & 1) ? r + 1 : r - 1;
    nr = nr < 0 ? 0 : (nr > g.ph[c] - 1 ? g.ph[c] - 1 : nr);
    const int colsum = 3 * plane_at(s, g, c, r, i) + plane_at(s, g, c, nr, i);
    const int nsum = 3 * plane_at(s, g, c, r, ni) + plane_at(s, g, c, nr, ni);
    return (3 * colsum + nsum + (odd ? 7 : 8)) >> 4;
}

__host__ __device__ inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// pixel (y, x) of the frame -> rgb[3]; s: the frame's samples
__host__ __device__ inline void pixel_rgb(const unsigned char* s, const Geom& g, int samp, int y, int x, unsigned char* rgb) {
    const int Y = plane_at(s, g, 0, y, x);
    if (samp == SAMP_GRAY) {
        rgb[0] = rgb[1] = rgb[2] = (unsigned char)Y;
        return;
    }
    const int cb = chroma_at(s, g, samp, 1, y, x) - 128, cr = chroma_at(s, g, samp, 2, y, x) - 128;
    rgb[0] = (unsigned char)clamp255(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = (unsigned char)clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    rgb[2] = (unsigned char)clamp255(Y + ((116130 * cb + 32768) >> 16));
}

__global__ __launch_bounds__(NTH) void jpeg_colour_kernel(const int* __restrict__ desc, const unsigned char* __restrict__ samples_ws,
                                                          unsigned char* __restrict__ out, Limits lim) {
    const int f = blockIdx.y;
    const int pix = blockIdx.x * NTH + threadIdx.x;   // Hc Wc <= 2^24
    if (pix >= lim.Hc * lim.Wc) return;
    const int y = pix / lim.Wc, x = pix % lim.Wc;
    const int* d = desc + (size_t)f * DESC;
    unsigned char rgb[3] = {0, 0, 0};
    Geom g;
    if (frame_ok(d, lim, g) && y < d[D_H] && x < d[D_W]) pixel_rgb(samples_ws + 64 * (size_t)d[D_WS], g, d[D_SAMP], y, x, rgb);
    unsigned char* o = out + 3 * ((size_t)f * lim.Hc * lim.Wc + pix);
    o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
}
}  // namespace

extern "C" size_t agrl_jpeg_decode_workspace(int ws_blocks) {
    return ws_blocks > 0 && ws_blocks <= MAX_WS_BLOCKS ? (size_t)ws_blocks * (128 + 64) : 0;
}

extern "C" int agrl_jpeg_decode_u8(const unsigned char* scans, long long scan_bytes, const int* desc_host, const int* desc, int F,
                                   const unsigned short* quant, int NQ, const int* huff, int NH, void* workspace, size_t workspace_bytes,
                                   unsigned char* out, int Hc, int Wc, int* status, int stages, agrl_stream_t stream) {
    AGRL_CHECK_ARG(scans && desc_host && desc && quant && huff && workspace && out && status, "agrl_jpeg_decode_u8: null pointer");
    AGRL_CHECK_ARG(F > 0 && F <= MAX_FRAMES, "agrl_jpeg_decode_u8: F=%d frames, 1..%d", F, MAX_FRAMES);
    AGRL_CHECK_ARG(Hc >= 1 && Hc <= MAX_DIM && Wc >= 1 && Wc <= MAX_DIM, "agrl_jpeg_decode_u8: container %dx%d, 1..%d each", Hc, Wc, MAX_DIM);
    AGRL_CHECK_ARG(scan_bytes > 0 && scan_bytes <= 0x7fffffffLL && NQ > 0 && NH > 0, "agrl_jpeg_decode_u8: bad sizes scan_bytes=%lld NQ=%d NH=%d",
                   scan_bytes, NQ, NH);
    AGRL_CHECK_ARG(stages >= 1 && stages <= (STAGE_ENTROPY | STAGE_IDCT | STAGE_COLOUR), "agrl_jpeg_decode_u8: stage mask %d, 1..7", stages);
    AGRL_CHECK_ARG(((uintptr_t)scans & 7) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)quant & 1) == 0 &&
                       ((uintptr_t)huff & 3) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)status & 3) == 0,
                   "agrl_jpeg_decode_u8: misaligned pointer (scans 8, workspace 16, tables and descriptors by their element)");
    const long long ws_cap = (long long)(workspace_bytes / (128 + 64));
    Limits lim = {scan_bytes, NQ, NH, (int)(ws_cap > MAX_WS_BLOCKS ? MAX_WS_BLOCKS : ws_cap), Hc, Wc};
    int max_blocks = 0;
    long long ws_end = 0;
    for (int f = 0; f < F; ++f) {   // every row, before anything is launched
        const int* d = desc_host + (size_t)f * DESC;
        Geom g;
        AGRL_CHECK_ARG(frame_ok(d, lim, g),
                       "agrl_jpeg_decode_u8: descriptor %d is outside its buffers (scan %d+%d of %lld bytes, %dx%d in a %dx%d container, sampling %d, "
                       "restart interval %d, quant %d %d %d of %d, Huffman %d %d %d / %d %d %d of %d, workspace block %d of %d)",
                       f, d[D_OFF], d[D_LEN], scan_bytes, d[D_H], d[D_W], Hc, Wc, d[D_SAMP], d[D_RI], d[D_Q0], d[D_Q0 + 1], d[D_Q0 + 2], NQ,
                       d[D_DC0], d[D_DC0 + 1], d[D_DC0 + 2], d[D_AC0], d[D_AC0 + 1], d[D_AC0 + 2], NH, d[D_WS], lim.ws_blocks);
        AGRL_CHECK_ARG(d[D_WS] >= ws_end, "agrl_jpeg_decode_u8: descriptor %d's workspace slice (block %d) overlaps the one before it (ends at %lld)",
                       f, d[D_WS], ws_end);
        ws_end = (long long)d[D_WS] + g.base[g.ncomp];
        max_blocks = g.base[g.ncomp] > max_blocks ? g.base[g.ncomp] : max_blocks;
    }
    short* coef = reinterpret_cast<short*>(workspace);
    unsigned char* samples = reinterpret_cast<unsigned char*>(workspace) + (size_t)lim.ws_blocks * 128;
    if (stages & STAGE_ENTROPY) {
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)F), dim3(AGRL_WAVE), 0, (hipStream_t)stream, scans, desc, quant, huff, coef,
                           status, lim);
        AGRL_CHECK_LAUNCH("agrl_jpeg_decode_u8 (entropy)");
    }
    if (stages & STAGE_IDCT) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)cdiv(max_blocks, NTH), (unsigned)F), dim3(NTH), 0, (hipStream_t)stream, desc, coef,
                           samples, lim);
        AGRL_CHECK_LAUNCH("agrl_jpeg_decode_u8 (idct)");
    }
    if (stages & STAGE_COLOUR) {
        hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)cdiv(Hc * Wc, NTH), (unsigned)F), dim3(NTH), 0, (hipStream_t)stream, desc, samples,
                           out, lim);
        AGRL_CHECK_LAUNCH("agrl_jpeg_decode_u8 (colour)");
    }
    return 0;
}
