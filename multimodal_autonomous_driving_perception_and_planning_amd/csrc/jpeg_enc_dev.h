// Baseline JPEG encode, the part host and device share (include/avhot.h: av_jpeg_encode_header / av_jpeg_encode):
// scan geometry, the Annex K Huffman code tables, the per-block entropy coder (one walk, instantiated as bit counter and as bit
// emitter), the byte stuffing, and on the host the quantiser tables and the frame header.  Everything here compiles as plain C++
// too: tests/jpeg_enc_check.cpp runs the same routines on the CPU under the address and undefined-behaviour sanitizers.
// Out of scope: grayscale, progressive, optimised Huffman tables, 16-bit quantisers.
//
// Bounds, by construction: a block is 64 coefficients read with eight 16-byte loads; code_block() makes at most 64 put() calls (plus ZRLs) of at
// most 26 bits; category indices are clamped to the tables; WordSink stores only below the word capacity it was given; stuff_bytes()
// stores only below the limit it was given.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <initializer_list>

#include "avhot.h"
#include "jpeg_dev.h"      // the zigzag order and the Annex K Huffman tables, shared with the decoder

#if defined(__HIPCC__)
#define JPEGE_HD __host__ __device__
#else
#define JPEGE_HD
#endif

namespace jpege {

// ---- scan geometry ------------------------------------------------------------------------------------------------------------------
// The workspace keeps a frame's blocks in the order the scan codes them: block = mcu * bpm + j; j < hs * vs is the luma block
// (j / hs, j % hs) of the MCU, then Cb, then Cr.  Each block: 64 int16 in zigzag order.
constexpr int MAX_BLOCKS = 1 << 21;          // per frame: bit offsets stay below 2^32, frame lengths below 2^31
constexpr int BLOCK_MAX_BYTES = 208;         // 20 bits of DC + 63 x 26 bits of AC = 1658 bits

struct Geom {
    int hs, vs, nl;           // luma sampling, luma blocks per MCU
    int mcus_x, mcus_y, n_mcus;
    int bpm, n_blocks;        // blocks per MCU, blocks per frame
    int nbx, nby;             // luma blocks that hold real pixels: the others of an MCU are dummy blocks
    int cw, ch;               // real chroma extent
    int dri;                  // what the DRI segment says (0: none)
    int ri, n_int;            // MCUs per restart interval as the kernels count them (n_mcus without restarts), intervals per frame
};

// subsampling: AV_JPEG_444 / 422 / 420; restart_mcus: -1 one MCU row, 0 none, else 1..65535 -> false for what is not supported
JPEGE_HD inline bool geom(int h, int w, int subsampling, int restart_mcus, Geom& g) {
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || subsampling < 0 || subsampling > 2 || restart_mcus < -1 || restart_mcus > 65535) return false;
    g.hs = subsampling == AV_JPEG_444 ? 1 : 2, g.vs = subsampling == AV_JPEG_420 ? 2 : 1, g.nl = g.hs * g.vs;
    g.mcus_x = (w + 8 * g.hs - 1) / (8 * g.hs), g.mcus_y = (h + 8 * g.vs - 1) / (8 * g.vs), g.n_mcus = g.mcus_x * g.mcus_y;
    g.bpm = g.nl + 2;
    if (g.n_mcus > MAX_BLOCKS / g.bpm) return false;
    g.n_blocks = g.n_mcus * g.bpm;
    g.nbx = (w + 7) / 8, g.nby = (h + 7) / 8;
    g.cw = (w + g.hs - 1) / g.hs, g.ch = (h + g.vs - 1) / g.vs;
    g.dri = restart_mcus < 0 ? g.mcus_x : restart_mcus;
    g.ri = g.dri > 0 && g.dri < g.n_mcus ? g.dri : g.n_mcus;
    g.n_int = (g.n_mcus + g.ri - 1) / g.ri;
    return true;
}
// bytes the unstuffed streams of one frame can need: every block at its longest, every interval padded to a byte; a multiple of 16
JPEGE_HD inline size_t stream_cap(int n_blocks, int n_mcus) { return ((size_t)n_blocks * BLOCK_MAX_BYTES + (size_t)n_mcus + 4 + 15) & ~(size_t)15; }

// the block whose DC predicts that of `blk`: the previous block of the same component in scan order; -1 at an interval's start
JPEGE_HD inline int pred_block(const Geom& g, int blk) {
    const int m = blk / g.bpm, j = blk - m * g.bpm;
    if (j > 0 && j < g.nl) return blk - 1;
    if (m % g.ri == 0) return -1;
    return j == 0 ? blk - g.bpm + g.nl - 1 : blk - g.bpm;
}

// ---- Huffman code tables: (length << 16) | code per symbol, 0 where the table has no such symbol ----------------------------------
struct Tables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr void fill_codes(uint32_t* out, const uint8_t* bits, const uint8_t* val) {
    uint32_t code = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int k = 0; k < bits[l - 1]; ++k) out[val[p++]] = ((uint32_t)l << 16) | code++;
        code <<= 1;
    }
}
constexpr Tables make_tables() {
    Tables T{};
    for (int t = 0; t < 2; ++t) fill_codes(T.dc[t], jpeg::STD_DC_BITS[t], jpeg::STD_DC_VAL), fill_codes(T.ac[t], jpeg::STD_AC_BITS[t], jpeg::STD_AC_VAL[t]);
    return T;
}

// ---- the per-block coder ------------------------------------------------------------------------------------------------------------
JPEGE_HD inline int category(int v, int cap) {       // bits of |v|, clamped to the table (real coefficients never reach the clamp)
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    const int s = a ? 32 - __builtin_clz(a) : 0;
    return s < cap ? s : cap;
}
struct Vec8 {
    uint32_t w[4];
};
// zz: the block's 64 coefficients, zigzag order, 16-byte aligned; pred: the DC before it; t: 0 luma tables, 1 chroma tables.
// Every code goes to sink.put(bits, length) together with its value bits, length <= 26.
template <class Sink>
JPEGE_HD inline void code_block(const Tables& T, const int16_t* zz, int pred, int t, Sink& sink) {
    int run = 0;
    for (int r = 0; r < 8; ++r) {
        Vec8 v;
        memcpy(&v, __builtin_assume_aligned(zz + 8 * r, 16), 16);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = (int)(int16_t)(uint16_t)(v.w[i >> 1] >> (16 * (i & 1)));
            if (r == 0 && i == 0) {
                const int diff = c - pred, s = category(diff, 11);
                const uint32_t e = T.dc[t][s];
                sink.put(((e & 0xFFFFu) << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1)), (int)(e >> 16) + s);
            } else if (c == 0) {
                ++run;
            } else {
                while (run > 15) {
                    const uint32_t z = T.ac[t][0xF0];
                    sink.put(z & 0xFFFFu, (int)(z >> 16));
                    run -= 16;
                }
                const int s = category(c, 10);
                const uint32_t e = T.ac[t][(run << 4) | s];
                sink.put(((e & 0xFFFFu) << s) | ((uint32_t)(c < 0 ? c - 1 : c) & ((1u << s) - 1)), (int)(e >> 16) + s);
                run = 0;
            }
        }
    }
    if (run > 0) sink.put(T.ac[t][0] & 0xFFFFu, (int)(T.ac[t][0] >> 16));       // EOB
}

struct CountSink {
    uint32_t bits = 0;
    JPEGE_HD void put(uint32_t, int len) { bits += (uint32_t)len; }
};

JPEGE_HD inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// Emits at a bit position of a zeroed byte stream kept as dwords, most significant bit first.  The first and the last dword a block
// touches can be shared with its neighbours (Store::merge: an OR that tolerates concurrent ones); the dwords between are its own.
template <class Store>
struct WordSink {
    Store st;
    uint32_t* words;
    uint32_t word, cap_words;
    uint64_t acc = 0;         // pending bits, left-aligned; the `n` most significant are valid
    int n;
    bool first;
    JPEGE_HD WordSink(Store s, uint32_t* w, uint64_t bitpos, uint32_t cap) : st(s), words(w), word((uint32_t)(bitpos >> 5)), cap_words(cap), n((int)(bitpos & 31)) {
        first = n != 0;
    }
    JPEGE_HD void put(uint32_t bits, int len) {
        if (len <= 0) return;
        acc |= (uint64_t)bits << (64 - n - len);
        n += len;
        if (n >= 32) {
            if (word < cap_words) {
                if (first) st.merge(words + word, bswap32((uint32_t)(acc >> 32)));
                else st.own(words + word, bswap32((uint32_t)(acc >> 32)));
            }
            first = false, ++word, acc <<= 32, n -= 32;
        }
    }
    // pad: fill up to the next byte boundary with 1-bits (the end of a restart interval)
    JPEGE_HD void finish(bool pad) {
        if (pad && (n & 7)) put((1u << (8 - (n & 7))) - 1, 8 - (n & 7));
        if (n > 0 && word < cap_words) st.merge(words + word, bswap32((uint32_t)(acc >> 32)));
    }
};

// ---- byte stuffing -----------------------------------------------------------------------------------------------------------------
JPEGE_HD inline uint32_t count_ff(const uint8_t* src, uint32_t n) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c += src[i] == 0xFF;
    return c;
}
// n bytes of src to dst[pos ...], a 00 behind every FF; nothing is stored at or beyond dst[limit]
JPEGE_HD inline void stuff_bytes(const uint8_t* src, uint32_t n, uint8_t* dst, int64_t pos, int64_t limit) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t b = src[i];
        if (pos < limit) dst[pos] = b;
        ++pos;
        if (b == 0xFF) {
            if (pos < limit) dst[pos] = 0;
            ++pos;
        }
    }
}

// ---- host half: quantiser tables and the frame header (av_jpeg_encode_header) ---------------------------------------------------
inline void quant_tables(int quality, uint8_t qt[2][64]) {
    static const uint8_t base[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (base[t][i] * scale + 50) / 100;
            qt[t][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

constexpr int HEADER_MAX = 640;

// SOI .. the SOS header as libjpeg writes them -> the length, or -1 (bad argument, or cap too small: nothing usable in out)
inline int write_header(int h, int w, int quality, int subsampling, int restart_mcus, uint8_t* out, int cap, uint8_t qt[2][64]) {
    Geom g;
    if (quality < 1 || quality > 100 || !geom(h, w, subsampling, restart_mcus, g)) return -1;
    quant_tables(quality, qt);
    uint8_t b[HEADER_MAX];
    int n = 0;
    auto put = [&](std::initializer_list<int> v) {
        for (int x : v) b[n++] = (uint8_t)x;
    };
    const uint8_t zz[64] = {JPEG_ZIGZAG};
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xDB, 0, 67, t});
        for (int k = 0; k < 64; ++k) b[n++] = qt[t][zz[k]];
    }
    put({0xFF, 0xC0, 0, 17, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, (g.hs << 4) | g.vs, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; ++t)
        for (int cls = 0; cls < 2; ++cls) {
            const int nv = cls ? 162 : 12;
            put({0xFF, 0xC4, (19 + nv) >> 8, (19 + nv) & 255, (cls << 4) | t});
            for (int k = 0; k < 16; ++k) b[n++] = cls ? jpeg::STD_AC_BITS[t][k] : jpeg::STD_DC_BITS[t][k];
            for (int k = 0; k < nv; ++k) b[n++] = cls ? jpeg::STD_AC_VAL[t][k] : jpeg::STD_DC_VAL[k];
        }
    if (g.dri > 0) put({0xFF, 0xDD, 0, 4, g.dri >> 8, g.dri & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    if (n > cap) return -1;
    memcpy(out, b, (size_t)n);
    return n;
}

}  // namespace jpege
