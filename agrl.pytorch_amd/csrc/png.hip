// PNG decode on the device, bit-exact with Pillow's Image.open().convert('RGB'): the reference's frame read (dataset_loader.py:23-36) for
// the two PNG datasets (iLIDS-VID, PRID2011), the sibling of jpeg.hip. The host (torchreid/device_decode.py) walks the chunks, checks
// their CRCs and hands over one byte buffer of zlib streams (the IDAT payloads of a file joined) and one descriptor row per frame; it
// never inflates. ONE launch, ONE wavefront (a one-wave workgroup) per frame, the inflated stream in LDS beside the code tables:
//   1. inflate (RFC 1950 / 1951): stored, fixed and dynamic blocks. The symbol walk is serial by construction, and every lane runs it
//      (wave-uniform: the same window, the same broadcast LDS look-ups), so that each lane knows every match without a hand-over; what
//      is parallel is shared by the 64 lanes -- clearing and filling the code tables, runs of code lengths, stored-block and
//      back-reference copies (a match is up to 258 bytes; where dist < len the source is start + k % dist), the Adler-32 (partial sums
//      modulo 65521: a = 1 + sum d_i, b = N + sum (N - i) d_i, over any partition).
//      The walk reads the stream through a 32-bit window refilled 16 bits at a time out of 8-byte words loaded one ahead; a code is
//      ONE look-up of a merged entry (operation | bits | base value, zlib's ``code``), two for codes longer than the root (9 bits
//      literal/length, 6 distance: zlib's own table shape, whose sizes ENOUGH bounds); no array indexed at run time lives in scratch.
//   2. the five row filters in place, row after row: Up over the lanes, Sub / Average / Paeth one lane per channel along the row
//   3. the expansion to RGB and the store into the frame's slot of the (F, Hc, Wc, 3) container, the rest of the slot zeroed
// torchreid/hip_ops.py: png_decode_reference is the same arithmetic in Python / numpy, and the definition of the status codes.
//
// HARD CONTRACT (jpeg.hip's): no address is formed from stream contents without a range check. The bit reader loads only words the
// descriptor check proved readable and feeds zeros beyond the stream's length; every output position is checked against the frame's
// inflated size (<= the LDS the launch was given), every distance against the output so far, every table index against the table;
// the descriptor rows are validated by the entry point on its host copy before the launch and AGAIN by the kernel on the device copy
// (frame_ok): a frame that fails is skipped with status 5. A frame whose status is non-zero has its slot zeroed and nothing else written.
#include "agrl_common.h"

namespace {
constexpr int DESC = 8;             // ints per descriptor row
constexpr int MAX_DIM = 4096;
constexpr int MAX_FRAMES = 1 << 20;
constexpr int MAX_INFLATED = 131072;   // H * (1 + W * channels): 256 x 128 RGB is 98 560
constexpr int MAX_STREAM = 1 << 27;    // bytes of one zlib stream: bit positions stay inside an int
enum { D_OFF = 0, D_LEN = 1, D_H = 2, D_W = 3, D_CH = 4 };
enum { ST_OK = 0, ST_INPUT = 1, ST_HEADER = 2, ST_BTYPE = 3, ST_STORED = 4, ST_DESC = 5, ST_COUNTS = 6, ST_OVERSUB = 7, ST_INCOMPLETE = 8,
       ST_REPEAT = 9, ST_NOEOB = 10, ST_LITLEN = 11, ST_DISTSYM = 12, ST_DIST = 13, ST_SHORT = 14, ST_LONG = 15, ST_ADLER = 16, ST_FILTER = 17 };
enum { STAGE_INFLATE = 1, STAGE_FILTER = 2, STAGE_STORE = 4 };
enum { KIND_CODES = 0, KIND_LENS = 1, KIND_DISTS = 2 };
// table sizes: root entries plus every second-level table. zlib's ENOUGH (inftrees.h) is 852 for 286 symbols at a 9-bit root and 592
// for 30 symbols at a 6-bit root, 15-bit codes; rounded up here, and the allocation is range-checked whatever the lengths are
constexpr int LIT_ROOT = 9, DIST_ROOT = 6, CL_ROOT = 7;
constexpr int LIT_ENTRIES = 1024, DIST_ENTRIES = 640, CL_ENTRIES = 128;
constexpr int MAX_LENS = 320;       // 288 + 32 code lengths of a fixed block; a dynamic one has at most 286 + 30

// one merged entry per code: op (bits 0-7) | bits of the code at this level (8-15) | value (16-31).
// op 0: literal, value = the byte; 16 + e: length or distance, value = its base, e extra bits; 32: end of block; 64: no code;
// 1..15: the codes with this root continue in a second-level table of 1 << op entries at index ``value``
constexpr unsigned OP_BASE = 16, OP_END = 32, OP_INVALID = 64;
__host__ __device__ inline unsigned entry(unsigned op, unsigned bits, unsigned val) { return op | (bits << 8) | (val << 16); }
__host__ __device__ inline unsigned e_op(unsigned e) { return e & 255u; }
__host__ __device__ inline unsigned e_bits(unsigned e) { return (e >> 8) & 255u; }
__host__ __device__ inline unsigned e_val(unsigned e) { return e >> 16; }
__host__ __device__ inline bool e_link(unsigned e) { return (e & 0xF0u) == 0 && (e & 0x0Fu) != 0; }

struct Limits {   // what a descriptor row is checked against
    long long stream_bytes;
    int Hc, Wc, cap;   // cap: bytes of inflated stream the launch has LDS for
};

struct Work {     // the tables and scratch of one frame, in LDS in front of the inflated stream
    unsigned lit[LIT_ENTRIES];
    unsigned dist[DIST_ENTRIES];
    unsigned cl[CL_ENTRIES];
    unsigned part[2 * AGRL_WAVE];     // the lanes' Adler-32 partial sums
    unsigned short code[MAX_LENS];    // per symbol: its code, bit-reversed (the stream's bit order)
    unsigned short count[16], next[16];
    unsigned char lens[MAX_LENS];
    int desc[DESC];
    int st;
};
constexpr int WORK_BYTES = (sizeof(Work) + 15) & ~15;

// The lanes of the wavefront that decodes a frame. On the host (the CPU check of the walk) there is one.
#ifdef __HIP_DEVICE_COMPILE__
#define PNG_LANE ((int)threadIdx.x)
#define PNG_LANES AGRL_WAVE
#define PNG_SYNC() __syncthreads()
#else
#define PNG_LANE 0
#define PNG_LANES 1
#define PNG_SYNC() ((void)0)
#endif

// The one validity predicate of a descriptor row: the entry point applies it to the host copy, the kernel to the device copy.
__host__ __device__ inline bool frame_ok(const int* d, const Limits& lim) {
    const int H = d[D_H], W = d[D_W], ch = d[D_CH];
    if (H < 1 || H > MAX_DIM || W < 1 || W > MAX_DIM || (ch != 1 && ch != 3)) return false;
    if (H > lim.Hc || W > lim.Wc) return false;
    if ((long long)H * (1 + W * ch) > lim.cap) return false;
    const long long off = d[D_OFF], len = d[D_LEN];
    if (off < 0 || len < 0 || len > MAX_STREAM || (off & 7) != 0 || off + ((len + 7) & ~7LL) + 8 > lim.stream_bytes) return false;   // one word ahead
    return true;
}

// ---- the bit reader: deflate's order, LSB first ---------------------------------------------------------------------------------------
// A 32-bit window refilled 16 bits at a time; the stream is read in aligned 8-byte words, the next one loaded while this one is used.
// Beyond the stream's length it feeds zeros: a field that used one of those has passed the end (over()).
struct Bits {
    const unsigned long long* d;   // 8-byte aligned; words 0 .. (n + 7) / 8 are readable
    int n, lastw;
    unsigned w;
    int cnt, h, widx;              // valid bits in w; next 16-bit unit; index of the word in ``cur``
    unsigned long long cur, nxt;

    __host__ __device__ inline unsigned long long load(int i) const { return i <= lastw ? d[i] : 0ull; }
    __host__ __device__ inline unsigned half() {
        const int hh = h++;
        const int wi = hh >> 2;
        if (wi != widx) cur = nxt, widx = wi, nxt = load(wi + 1);   // units are taken in order: wi == widx + 1
        unsigned v = (unsigned)(cur >> (16 * (hh & 3))) & 0xFFFFu;
        if (2 * hh + 2 > n) v = 2 * hh >= n ? 0u : (v & 0xFFu);
        return v;
    }
    __host__ __device__ inline void seek(int p) {   // 0 <= p <= n
        h = p >> 1, widx = h >> 2, cur = load(widx), nxt = load(widx + 1), w = 0, cnt = 0;
        if (p & 1) w = half() >> 8, cnt = 8;
    }
    __host__ __device__ inline void init(const unsigned char* data, int len) {
        d = reinterpret_cast<const unsigned long long*>(data), n = len, lastw = (len + 7) >> 3;
        seek(0);
    }
    __host__ __device__ inline void refill() {   // at least 16 valid bits afterwards
        if (cnt <= 16) w |= half() << cnt, cnt += 16;
    }
    __host__ __device__ inline unsigned peek(int k) const { return w & ((1u << k) - 1u); }   // k <= 16
    __host__ __device__ inline void drop(int k) { w >>= k, cnt -= k; }
    __host__ __device__ inline unsigned take(int k) {
        refill();
        const unsigned v = peek(k);
        drop(k);
        return v;
    }
    __host__ __device__ inline void align() { drop(cnt & 7); }
    __host__ __device__ inline int bytepos() const { return (16 * h - cnt) >> 3; }
    __host__ __device__ inline bool over() const { return 16 * h - cnt > 8 * n; }
};

// ---- the code tables --------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned symbol_entry(int kind, int sym, unsigned bits) {
    if (kind == KIND_CODES) return entry(0, bits, (unsigned)sym);
    if (kind == KIND_LENS) {
        if (sym < 256) return entry(0, bits, (unsigned)sym);
        if (sym == 256) return entry(OP_END, bits, 0);
        if (sym > 285) return entry(OP_INVALID, bits, 0);
        const int i = sym - 257;
        if (i < 8) return entry(OP_BASE, bits, 3u + i);
        if (i == 28) return entry(OP_BASE, bits, 258u);
        const unsigned extra = (unsigned)(i - 4) >> 2;
        return entry(OP_BASE | extra, bits, 3u + ((4u + (i & 3)) << extra));
    }
    if (sym > 29) return entry(OP_INVALID, bits, 0);
    if (sym < 4) return entry(OP_BASE, bits, 1u + sym);
    const unsigned extra = (unsigned)(sym - 2) >> 1;
    return entry(OP_BASE | extra, bits, 1u + ((2u + (sym & 1)) << extra));
}

// Code lengths (each <= 15) -> the look-up table of their canonical Huffman code, with inflate's own rejections (inftrees.c): an
// over-subscribed set; an incomplete one, except a distance set of one code of length 1; no code at all only for distances.
// Lane 0 counts, assigns the codes and sizes the second-level tables; the lanes clear the table and write the entries.
__host__ __device__ inline int build_table(Work& wk, const unsigned char* lens, int n, int kind, unsigned* tab, int root, int entries) {
    const int lane = PNG_LANE;
    const unsigned mask = (1u << root) - 1u;
    for (int i = lane; i < entries; i += PNG_LANES) tab[i] = entry(OP_INVALID, 1, 0);
    PNG_SYNC();   // the lengths and the cleared table
    if (lane == 0) {
        int st = ST_OK;
        for (int l = 0; l < 16; ++l) wk.count[l] = 0;
        for (int s = 0; s < n; ++s) ++wk.count[lens[s] & 15];
        int maxl = 15;
        while (maxl > 0 && wk.count[maxl] == 0) --maxl;
        if (maxl == 0) {
            st = kind == KIND_DISTS ? ST_OK : ST_INCOMPLETE;
        } else {
            int left = 1;
            unsigned code = 0;
            for (int l = 1; l < 16 && st == ST_OK; ++l) {
                code = (code + (l > 1 ? wk.count[l - 1] : 0u)) << 1;
                wk.next[l] = (unsigned short)code;
                left = 2 * left - wk.count[l];
                if (left < 0) st = ST_OVERSUB;
            }
            if (st == ST_OK && left > 0 && (kind != KIND_DISTS || maxl != 1)) st = ST_INCOMPLETE;
            if (st == ST_OK) {
                for (int s = 0; s < n; ++s) {   // the codes; per root the longest code behind it
                    const int l = lens[s] & 15;
                    if (!l) continue;
                    const unsigned c = wk.next[l]++;
                    const unsigned rev = __builtin_bitreverse32(c) >> (32 - l);
                    wk.code[s] = (unsigned short)rev;
                    if (l > root) {
                        const unsigned e = tab[rev & mask];
                        const unsigned have = e_link(e) ? e_op(e) : 0u;
                        if ((unsigned)(l - root) > have) tab[rev & mask] = entry((unsigned)(l - root), (unsigned)root, 0);
                    }
                }
                int next = 1 << root;
                for (int s = 0; s < n && st == ST_OK; ++s) {   // a second-level table behind each such root
                    const int l = lens[s] & 15;
                    if (l <= root) continue;
                    const unsigned at = wk.code[s] & mask;
                    const unsigned e = tab[at];
                    if (e_val(e) != 0) continue;
                    const int size = 1 << e_op(e);
                    if (next + size > entries) st = ST_OVERSUB;   // beyond what any complete code needs
                    else tab[at] = entry(e_op(e), (unsigned)root, (unsigned)next), next += size;
                }
            }
        }
        wk.st = st;
    }
    PNG_SYNC();
    const int st = wk.st;
    if (st != ST_OK) return st;
    for (int s = lane; s < n; s += PNG_LANES) {
        const int l = lens[s] & 15;
        if (!l) continue;
        const unsigned rev = wk.code[s];
        if (l <= root) {
            const unsigned e = symbol_entry(kind, s, (unsigned)l);
            for (unsigned j = rev; j <= mask; j += 1u << l) tab[j] = e;
        } else {
            const unsigned link = tab[rev & mask];
            const unsigned e = symbol_entry(kind, s, (unsigned)(l - root));
            const unsigned size = 1u << e_op(link);
            for (unsigned j = rev >> root; j < size; j += 1u << (l - root)) {
                const unsigned at = e_val(link) + j;
                if (at < (unsigned)entries) tab[at] = e;
            }
        }
    }
    PNG_SYNC();
    return ST_OK;
}

// one code out of a table at the window's low bits -> its final entry; ``used``: the bits it takes
__host__ __device__ inline unsigned look_up(const unsigned* tab, int root, int entries, unsigned w, int& used) {
    unsigned e = tab[w & ((1u << root) - 1u)];
    used = (int)e_bits(e);
    if (e_link(e)) {
        const unsigned at = e_val(e) + ((w >> root) & ((1u << e_op(e)) - 1u));
        e = at < (unsigned)entries ? tab[at] : entry(OP_INVALID, 1, 0);
        used += (int)e_bits(e);
    }
    return e;
}

// ---- inflate: one zlib stream -> exactly ``expected`` bytes in ``buf`` (LDS), or a status ----------------------------------------------
__host__ __device__ inline int inflate_stream(const unsigned char* src, int n, Work& wk, unsigned char* buf, int expected) {
    const int lane = PNG_LANE;
    Bits br;
    br.init(src, n);
    const unsigned cmf = br.take(8), flg = br.take(8);
    if (br.over()) return ST_INPUT;
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0 || (flg & 32u)) return ST_HEADER;
    int outpos = 0;
    unsigned last = 0;
    while (!last) {
        last = br.take(1);
        const unsigned btype = br.take(2);
        if (br.over()) return ST_INPUT;
        if (btype == 3) return ST_BTYPE;
        if (btype == 0) {
            br.align();
            const unsigned len = br.take(16), inv = br.take(16);
            if (br.over()) return ST_INPUT;
            if (len != (inv ^ 0xFFFFu)) return ST_STORED;
            const int at = br.bytepos();
            if (at + (int)len > n) return ST_INPUT;
            if (outpos + (int)len > expected) return ST_LONG;
            for (int k = lane; k < (int)len; k += PNG_LANES) buf[outpos + k] = src[at + k];
            outpos += (int)len;
            br.seek(at + (int)len);
            continue;
        }
        int nlen = 288, ndist = 32;
        PNG_SYNC();   // nobody still reads the tables or the lengths of the block before
        if (btype == 1) {
            for (int s = lane; s < MAX_LENS; s += PNG_LANES) wk.lens[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        } else {
            nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1;
            const int ncode = (int)br.take(4) + 4;
            if (br.over()) return ST_INPUT;
            if (nlen > 286 || ndist > 30) return ST_COUNTS;
            const unsigned char* order = reinterpret_cast<const unsigned char*>("\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f");
            for (int i = 0; i < 19; ++i) {
                const unsigned v = i < ncode ? br.take(3) : 0u;
                if (lane == 0) wk.lens[order[i]] = (unsigned char)v;
            }
            if (br.over()) return ST_INPUT;
            int st = build_table(wk, wk.lens, 19, KIND_CODES, wk.cl, CL_ROOT, CL_ENTRIES);
            if (st != ST_OK) return st;
            const int total = nlen + ndist;
            int i = 0;
            unsigned prev = 0;
            while (i < total) {
                br.refill();
                int used;
                const unsigned e = look_up(wk.cl, CL_ROOT, CL_ENTRIES, br.w, used);
                br.drop(used);
                if (br.over()) return ST_INPUT;
                if (e_op(e) != 0) return ST_INCOMPLETE;
                const unsigned sym = e_val(e);
                if (sym < 16) {
                    if (lane == 0) wk.lens[i] = (unsigned char)sym;
                    prev = sym, ++i;
                    continue;
                }
                int rep;
                if (sym == 16) {
                    if (i == 0) return ST_REPEAT;
                    rep = 3 + (int)br.take(2);
                } else if (sym == 17) {
                    rep = 3 + (int)br.take(3), prev = 0;
                } else {
                    rep = 11 + (int)br.take(7), prev = 0;
                }
                if (br.over()) return ST_INPUT;
                if (i + rep > total) return ST_REPEAT;
                for (int k = lane; k < rep; k += PNG_LANES) wk.lens[i + k] = (unsigned char)prev;
                i += rep;
            }
            PNG_SYNC();
            if (wk.lens[256] == 0) return ST_NOEOB;
        }
        int st = build_table(wk, wk.lens, nlen, KIND_LENS, wk.lit, LIT_ROOT, LIT_ENTRIES);
        if (st != ST_OK) return st;
        st = build_table(wk, wk.lens + nlen, ndist, KIND_DISTS, wk.dist, DIST_ROOT, DIST_ENTRIES);
        if (st != ST_OK) return st;
        for (;;) {   // the symbol walk
            br.refill();
            int used;
            unsigned e = look_up(wk.lit, LIT_ROOT, LIT_ENTRIES, br.w, used);
            br.drop(used);
            if (br.over()) return ST_INPUT;
            unsigned op = e_op(e);
            if (op == 0) {
                if (outpos >= expected) return ST_LONG;
                if (lane == 0) buf[outpos] = (unsigned char)e_val(e);
                ++outpos;
                continue;
            }
            if (op & OP_END) break;
            if (!(op & OP_BASE)) return ST_LITLEN;
            const int len = (int)(e_val(e) + br.take((int)(op & 15u)));
            if (br.over()) return ST_INPUT;
            br.refill();
            e = look_up(wk.dist, DIST_ROOT, DIST_ENTRIES, br.w, used);
            br.drop(used);
            if (br.over()) return ST_INPUT;
            op = e_op(e);
            if (!(op & OP_BASE)) return ST_DISTSYM;
            const int dist = (int)(e_val(e) + br.take((int)(op & 15u)));
            if (br.over()) return ST_INPUT;
            if (dist > outpos) return ST_DIST;
            if (outpos + len > expected) return ST_LONG;
            PNG_SYNC();   // the bytes before outpos, whichever lane wrote them
            const int start = outpos - dist;   // 0 <= start; start + k % dist < outpos; outpos + k < expected
            if (dist >= len) {
                for (int k = lane; k < len; k += PNG_LANES) buf[outpos + k] = buf[start + k];
            } else {
                for (int k = lane; k < len; k += PNG_LANES) buf[outpos + k] = buf[start + k % dist];
            }
            outpos += len;
        }
    }
    if (outpos < expected) return ST_SHORT;
    br.align();
    const unsigned hi = br.take(16), lo = br.take(16);   // big-endian in the stream
    if (br.over()) return ST_INPUT;
    const unsigned want = ((((hi & 255u) << 8) | (hi >> 8)) << 16) | ((lo & 255u) << 8) | (lo >> 8);
    PNG_SYNC();
    unsigned long long sa = 0, sb = 0;
    for (int i = lane; i < expected; i += PNG_LANES) {
        const unsigned v = buf[i];
        sa += v, sb += (unsigned long long)(expected - i) * v;
    }
    wk.part[lane] = (unsigned)(sa % 65521u), wk.part[PNG_LANES + lane] = (unsigned)(sb % 65521u);
    PNG_SYNC();
    unsigned a = 1, b = (unsigned)expected % 65521u;
    for (int i = 0; i < PNG_LANES; ++i) a += wk.part[i], b += wk.part[PNG_LANES + i];   // 65 terms below 65521 each
    PNG_SYNC();
    return ((b % 65521u) << 16 | (a % 65521u)) == want ? ST_OK : ST_ADLER;
}

// ---- the row filters, undone in place (PNG specification, 9.2); the row above the first one is zeros --------------------------------
__host__ __device__ inline int unfilter(unsigned char* buf, int H, int rb, int bpp) {
    const int lane = PNG_LANE, stride = rb + 1;
    PNG_SYNC();
    for (int y = 0; y < H; ++y) {
        unsigned char* row = buf + (size_t)y * stride + 1;
        const unsigned char* up = y > 0 ? row - stride : row;   // read only where y > 0
        const int ft = row[-1];
        if (ft > 4) return ST_FILTER;
        if (ft == 2) {
            if (y > 0)
                for (int i = lane; i < rb; i += PNG_LANES) row[i] = (unsigned char)(row[i] + up[i]);
        } else if (ft != 0) {
            for (int c0 = lane; c0 < bpp; c0 += PNG_LANES) {   // one lane per channel walks the row
                int a = 0, c = 0;
                for (int i = c0; i < rb; i += bpp) {
                    const int b = y > 0 ? up[i] : 0;
                    int pred;
                    if (ft == 1) {
                        pred = a;
                    } else if (ft == 3) {
                        pred = (a + b) >> 1;
                    } else {
                        const int p = a + b - c;
                        const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
                        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    }
                    a = (row[i] + pred) & 255, c = b;
                    row[i] = (unsigned char)a;
                }
            }
        }
        PNG_SYNC();
    }
    return ST_OK;
}

// the frame's samples (or, with ``buf`` null, nothing) into its slot: grey replicated to RGB, zeros outside H x W
__host__ __device__ inline void store_frame(const unsigned char* buf, int H, int W, int ch, unsigned char* slot, int Hc, int Wc) {
    const int lane = PNG_LANE, stride = 1 + W * ch, row3 = 3 * Wc;
    for (int y = 0; y < Hc; ++y) {
        const bool live = buf != nullptr && y < H;
        const unsigned char* row = live ? buf + (size_t)y * stride + 1 : nullptr;
        unsigned char* o = slot + (size_t)y * row3;
        for (int r = lane; r < row3; r += PNG_LANES) {
            const int x = r / 3;
            o[r] = live && x < W ? row[ch == 3 ? r : x] : (unsigned char)0;
        }
    }
}

// one frame, start to end: what the kernel's wavefront does, and what the CPU check of the walk calls
__host__ __device__ inline int decode_frame(const unsigned char* streams, const int* d, Work& wk, unsigned char* buf, unsigned char* slot, int Hc,
                                            int Wc, int stages) {
    const int H = d[D_H], W = d[D_W], ch = d[D_CH];
    int st = inflate_stream(streams + d[D_OFF], d[D_LEN], wk, buf, H * (1 + W * ch));
    if (st == ST_OK && (stages & STAGE_FILTER)) st = unfilter(buf, H, W * ch, ch);
    if (stages & STAGE_STORE) store_frame(st == ST_OK ? buf : nullptr, H, W, ch, slot, Hc, Wc);
    return st;
}

__global__ __launch_bounds__(AGRL_WAVE) void png_decode_kernel(const unsigned char* __restrict__ streams, const int* __restrict__ desc,
                                                               unsigned char* __restrict__ out, int* __restrict__ status, Limits lim, int stages) {
    extern __shared__ uint4 s_mem[];
    Work& wk = *reinterpret_cast<Work*>(s_mem);
    unsigned char* buf = reinterpret_cast<unsigned char*>(s_mem) + WORK_BYTES;   // lim.cap bytes
    const int f = blockIdx.x, lane = threadIdx.x;
    if (lane < DESC) wk.desc[lane] = desc[(size_t)f * DESC + lane];
    __syncthreads();
    unsigned char* slot = out + (size_t)f * lim.Hc * lim.Wc * 3;
    int st;
    if (!frame_ok(wk.desc, lim)) {   // wave-uniform
        st = ST_DESC;
        if (stages & STAGE_STORE) store_frame(nullptr, 0, 0, 1, slot, lim.Hc, lim.Wc);
    } else {
        st = decode_frame(streams, wk.desc, wk, buf, slot, lim.Hc, lim.Wc, stages);
    }
    if (lane == 0) status[f] = st;
}
}  // namespace

extern "C" int agrl_png_decode_u8(const unsigned char* streams, long long stream_bytes, const int* desc_host, const int* desc, int F,
                                  unsigned char* out, int Hc, int Wc, int* status, int stages, agrl_stream_t stream) {
    AGRL_CHECK_ARG(streams && desc_host && desc && out && status, "agrl_png_decode_u8: null pointer");
    AGRL_CHECK_ARG(F > 0 && F <= MAX_FRAMES, "agrl_png_decode_u8: F=%d frames, 1..%d", F, MAX_FRAMES);
    AGRL_CHECK_ARG(Hc >= 1 && Hc <= MAX_DIM && Wc >= 1 && Wc <= MAX_DIM, "agrl_png_decode_u8: container %dx%d, 1..%d each", Hc, Wc, MAX_DIM);
    AGRL_CHECK_ARG(stream_bytes > 0 && stream_bytes <= 0x7fffffffLL, "agrl_png_decode_u8: bad sizes stream_bytes=%lld", stream_bytes);
    AGRL_CHECK_ARG(stages >= 1 && stages <= (STAGE_INFLATE | STAGE_FILTER | STAGE_STORE) && (stages & STAGE_INFLATE),
                   "agrl_png_decode_u8: stage mask %d: 1 (inflate) | 2 (filters) | 4 (store), inflate always", stages);
    AGRL_CHECK_ARG(((uintptr_t)streams & 7) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)status & 3) == 0,
                   "agrl_png_decode_u8: misaligned pointer (streams 8, descriptors and status 4)");
    Limits lim = {stream_bytes, Hc, Wc, MAX_INFLATED};
    int cap = 16;
    for (int f = 0; f < F; ++f) {   // every row, before anything is launched
        const int* d = desc_host + (size_t)f * DESC;
        AGRL_CHECK_ARG(frame_ok(d, lim),
                       "agrl_png_decode_u8: descriptor %d is outside its buffers (stream %d+%d of %lld bytes, %dx%d in a %dx%d container, %d "
                       "channels, at most %d inflated bytes)",
                       f, d[D_OFF], d[D_LEN], stream_bytes, d[D_H], d[D_W], Hc, Wc, d[D_CH], MAX_INFLATED);
        const int need = d[D_H] * (1 + d[D_W] * d[D_CH]);
        cap = need > cap ? need : cap;
    }
    lim.cap = (cap + 15) & ~15;   // the frames of THIS batch: a batch of small frames leaves the LDS to more workgroups
    const size_t lds = (size_t)WORK_BYTES + (size_t)lim.cap;
    if (lds > 64 * 1024) {   // above the default dynamic-LDS limit of a launch; gfx950 has 160 KB per CU
        hipError_t e = hipFuncSetAttribute((const void*)png_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        AGRL_CHECK_ARG(e == hipSuccess, "agrl_png_decode_u8: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(png_decode_kernel, dim3((unsigned)F), dim3(AGRL_WAVE), lds, (hipStream_t)stream, streams, desc, out, status, lim, stages);
    AGRL_CHECK_LAUNCH("agrl_png_decode_u8");
    return 0;
}
