// Baseline JPEG, the part host and device share (include/avhot.h: av_jpeg_parse / av_jpeg_decode): frame geometry, the Huffman
// tables as the entropy kernel keeps them in LDS, the bit reader and the per-segment entropy decode.  Everything here compiles as
// plain C++ too: tests/jpeg_check.cpp runs the same routines on the CPU under the address and undefined-behaviour sanitizers.
//
// Bounds, by construction: decode_segment() loops over n_mcus MCUs x at most 6 blocks x 64 coefficients; the reader never
// fetches a byte outside [begin, end), i.e. never a dword outside the ones enclosing that range; a block address is formed from an
// MCU index below the frame's MCU count only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "avhot.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

namespace jpeg {

// zigzag index -> natural (row-major) index
#define JPEG_ZIGZAG                                                                                                                  \
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, \
        50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63

struct Geom {
    int ncomp, hs, vs;        // luma sampling (1 x 1 for gray)
    int mcus_x, mcus_y, n_mcus;
    int bw[3], bh[3];         // blocks per row / column of each component's (MCU-padded) plane
    int off[3];               // first block of each component in the frame's coefficient / sample area
    int n_blocks;             // blocks of the whole frame
    int cw, ch;               // real chroma extent (what the upsampling filters may touch)
};

// blocks a frame of h x w can need, whatever its subsampling: 3 planes padded to 16 x 16
JPEG_HD inline int cap_blocks(int h, int w) { return 12 * ((w + 15) / 16) * ((h + 15) / 16); }

// The geometry of a frame of h x w, if `d` is a descriptor av_jpeg_parse could have made for that size (false otherwise: the kernels
// then leave the frame undecoded).  Nothing else of `d` is trusted to index memory.
JPEG_HD inline bool geom_from(const av_jpeg_desc& d, int h, int w, Geom& g) {
    if (d.width != w || d.height != h || (d.ncomp != 1 && d.ncomp != 3)) return false;
    const bool gray = d.ncomp == 1;
    if (gray ? (d.hs != 1 || d.vs != 1) : !((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return false;
    for (int c = 0; c < d.ncomp; ++c)
        if (d.tq[c] > 3 || d.td[c] > 1 || d.ta[c] > 1) return false;
    g.ncomp = d.ncomp, g.hs = d.hs, g.vs = d.vs;
    g.mcus_x = (w + 8 * g.hs - 1) / (8 * g.hs), g.mcus_y = (h + 8 * g.vs - 1) / (8 * g.vs);
    g.n_mcus = g.mcus_x * g.mcus_y;
    if (d.restart_interval < 0 || d.restart_interval > 65535 || d.n_segments != (d.restart_interval > 0 ? (g.n_mcus + d.restart_interval - 1) / d.restart_interval : 1)) return false;
    int o = 0;
    for (int c = 0; c < 3; ++c) {
        const bool on = c < g.ncomp;
        g.bw[c] = on ? g.mcus_x * (c == 0 ? g.hs : 1) : 0, g.bh[c] = on ? g.mcus_y * (c == 0 ? g.vs : 1) : 0;
        g.off[c] = o;
        o += g.bw[c] * g.bh[c];
    }
    g.n_blocks = o;
    g.cw = (w + g.hs - 1) / g.hs, g.ch = (h + g.vs - 1) / g.vs;
    return o <= cap_blocks(h, w);
}

// ---- Huffman tables of one frame: DC 0, DC 1, AC 0, AC 1 (5760 bytes; LDS on the device) ---------------------------------------
struct Tables {
    uint16_t look[4][512];    // by the next 9 bits: (code length << 8) | symbol; 0: the code is longer than 9 bits, or none
    int32_t maxcode[4][18];   // largest code of length l (1..16), -1 where there is none
    int32_t valoff[4][18];    // index of that length's first symbol minus its first code
    uint8_t val[4][256];
    uint8_t zz[64];
};

// Table t of `d` into T.  The counts are re-bounded here, so any 928 bytes give tables that index inside themselves.
JPEG_HD inline void build_table(const av_jpeg_desc& d, Tables& T, int t) {
    const uint8_t* bits = t < 2 ? d.dc_bits[t] : d.ac_bits[t - 2];
    const uint8_t* val = t < 2 ? d.dc_val[t] : d.ac_val[t - 2];
    const int nval = t < 2 ? 16 : 256;
    for (int i = 0; i < 256; ++i) T.val[t][i] = i < nval ? val[i] : 0;
    for (int i = 0; i < 512; ++i) T.look[t][i] = 0;
    int code = 0, p = 0;
    T.maxcode[t][0] = -1, T.valoff[t][0] = 0, T.maxcode[t][17] = -1, T.valoff[t][17] = 0;
    for (int l = 1; l <= 16; ++l) {
        int n = bits[l - 1];
        if (n > (1 << l) - code) n = (1 << l) - code;          // av_jpeg_parse refuses such a table; bounded all the same
        if (n > 256 - p) n = 256 - p;
        T.valoff[t][l] = p - code;
        if (n > 0) {
            if (l <= 9)
                for (int k = 0; k < n; ++k) {
                    const uint16_t e = (uint16_t)((l << 8) | T.val[t][p + k]);
                    const int first = (code + k) << (9 - l);
                    for (int j = 0; j < (1 << (9 - l)); ++j) T.look[t][first + j] = e;
                }
            p += n, code += n;
            T.maxcode[t][l] = code - 1;
        } else {
            T.maxcode[t][l] = -1;
        }
        code <<= 1;
    }
}
JPEG_HD inline void build_zigzag(Tables& T) {
    const uint8_t zz[64] = {JPEG_ZIGZAG};
    for (int i = 0; i < 64; ++i) T.zz[i] = zz[i];
}

// ---- bit reader: 64-bit buffer, most significant bit first, bits below `cnt` are zero ------------------------------------------
struct Reader {
    const uint32_t* words;    // the byte buffer as aligned little-endian dwords
    uint32_t pos, end;        // next byte, end of the segment (absolute byte offsets into `words`)
    uint32_t widx, w;         // the dword last fetched
    uint64_t buf;
    int cnt;
};
JPEG_HD inline uint32_t byte_at(Reader& r, uint32_t p) {
    if ((p >> 2) != r.widx) r.widx = p >> 2, r.w = r.words[r.widx];
    return (r.w >> ((p & 3) * 8)) & 255u;
}
JPEG_HD inline void reader_init(Reader& r, const uint32_t* words, uint32_t begin, uint32_t end) {
    r.words = words, r.pos = begin, r.end = end, r.widx = 0xFFFFFFFFu, r.w = 0, r.buf = 0, r.cnt = 0;
}
// top the buffer up to more than 56 bits while bytes last.  FF 00 is the data byte FF; any other FF ends the readable data.
JPEG_HD inline void refill(Reader& r) {
    while (r.cnt <= 56 && r.pos < r.end) {
        const uint32_t b = byte_at(r, r.pos);
        if (b == 0xFF) {
            if (r.pos + 1 < r.end && byte_at(r, r.pos + 1) == 0) r.pos += 2;
            else break;
        } else {
            r.pos += 1;
        }
        r.buf |= (uint64_t)b << (56 - r.cnt);
        r.cnt += 8;
    }
}
// one Huffman symbol of table t -> 0, or the AV_JPEG_E* bit
JPEG_HD inline int get_symbol(Reader& r, const Tables& T, int t, int& sym) {
    if (r.cnt < 16) refill(r);
    const int look = (int)(r.buf >> 48);
    const uint16_t e = T.look[t][look >> 7];
    int l;
    if (e) {
        l = e >> 8, sym = e & 255;
    } else {
        int code = 0;
        for (l = 10; l <= 16; ++l) {
            code = look >> (16 - l);
            if (code <= T.maxcode[t][l]) break;
        }
        if (l > 16) return r.cnt < 16 ? AV_JPEG_EBYTES : AV_JPEG_ECODE;
        sym = T.val[t][(code + T.valoff[t][l]) & 255];
    }
    if (l > r.cnt) return AV_JPEG_EBYTES;
    r.buf <<= l, r.cnt -= l;
    return 0;
}
// s bits (1..15) as the signed value EXTEND makes of them
JPEG_HD inline int get_value(Reader& r, int s, int& v) {
    if (r.cnt < s) refill(r);
    if (r.cnt < s) return AV_JPEG_EBYTES;
    const int u = (int)(r.buf >> (64 - s));
    r.buf <<= s, r.cnt -= s;
    v = u >= (1 << (s - 1)) ? u : u - (1 << s) + 1;
    return 0;
}

// One 8 x 8 block into blk[64] (natural order, zero before the call): only non-zero coefficients are stored.
JPEG_HD inline int decode_block(Reader& r, const Tables& T, int td, int ta, int& pred, int16_t* blk) {
    int sym, v, e;
    if ((e = get_symbol(r, T, td, sym))) return e;
    sym &= 15;
    if (sym) {
        if ((e = get_value(r, sym, v))) return e;
        pred += v;
    }
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        if ((e = get_symbol(r, T, 2 + ta, sym))) return e;
        const int run = sym >> 4, s = sym & 15;
        if (s == 0) {
            if (run != 15) break;                    // EOB
            if (k + 16 > 64) return AV_JPEG_ERUN;
            k += 16;
            continue;
        }
        k += run;
        if (k > 63) return AV_JPEG_ERUN;
        if ((e = get_value(r, s, v))) return e;
        blk[T.zz[k]] = (int16_t)v;
        ++k;
    }
    return 0;
}

// The MCUs [mcu0, mcu0 + n_mcus) of one frame from the bytes [begin, end) into coef (the frame's coefficient area, g.n_blocks x 64,
// zero before the call) -> 0 or one AV_JPEG_E* bit.  On an error the block in progress is zeroed again and the rest stays zero.
JPEG_HD inline int decode_segment(const av_jpeg_desc& d, const Geom& g, const Tables& T, const uint32_t* words, uint32_t begin, uint32_t end,
                                  int mcu0, int n_mcus, int16_t* coef) {
    Reader r;
    reader_init(r, words, begin, end);
    int pred[3] = {0, 0, 0};
    if (mcu0 < 0 || mcu0 >= g.n_mcus) return 0;
    if (n_mcus > g.n_mcus - mcu0) n_mcus = g.n_mcus - mcu0;
    int mx = mcu0 % g.mcus_x, my = mcu0 / g.mcus_x;
    for (int m = 0; m < n_mcus; ++m) {
        for (int c = 0; c < g.ncomp; ++c) {
            const int hsc = c == 0 ? g.hs : 1, vsc = c == 0 ? g.vs : 1;
            for (int v = 0; v < vsc; ++v)
                for (int hh = 0; hh < hsc; ++hh) {
                    int16_t* blk = coef + ((size_t)g.off[c] + (size_t)(my * vsc + v) * g.bw[c] + (mx * hsc + hh)) * 64;
                    const int e = decode_block(r, T, d.td[c] & 1, d.ta[c] & 1, pred[c], blk);
                    if (e) {
                        for (int i = 0; i < 64; ++i) blk[i] = 0;
                        return e;
                    }
                }
        }
        if (++mx == g.mcus_x) mx = 0, ++my;
    }
    return (r.cnt >= 8 || r.pos < r.end) ? AV_JPEG_ELEFT : 0;
}

// ---- host half: the header parse and the segment walk (av_jpeg_parse) --------------------------------------------------------------
// ITU-T T.81 Annex K.3 "typical" Huffman tables: DC luminance, DC chrominance, AC luminance, AC chrominance
static const uint8_t STD_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t STD_DC_VAL[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t STD_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t STD_AC_VAL[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
     130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
     90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149,
     150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199,
     200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247,
     248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10,
     22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
     90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
     149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198,
     199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248,
     249, 250}};

// BITS of a DHT table: a prefix code (no length over-subscribed) of at most `cap` symbols?
inline bool bits_ok(const uint8_t* bits, int cap) {
    int code = 0, n = 0;
    for (int l = 1; l <= 16; ++l) {
        code += bits[l - 1], n += bits[l - 1];
        if (code > (1 << l)) return false;
        code <<= 1;
    }
    return n <= cap;
}

// -> AV_OK or AV_EJPEG_*; *why names the reason.  seg_cap entries of segs may be written.
inline int parse(const uint8_t* p, size_t len, int h, int w, av_jpeg_desc* d, av_jpeg_seg* segs, int seg_cap, int* n_segs, const char** why) {
    const uint8_t zz[64] = {JPEG_ZIGZAG};
#define JPEG_FAIL(code, text) return (*why = (text), (code))
    memset(d, 0, sizeof *d);
    *n_segs = 0;
    if (len > 0x7FFFFFF0u) JPEG_FAIL(AV_EJPEG_FORMAT, "frame of 2 GiB or more");
    if (len < 2) JPEG_FAIL(AV_EJPEG_TRUNCATED, "ends before SOI");
    if (p[0] != 0xFF || p[1] != 0xD8) JPEG_FAIL(AV_EJPEG_FORMAT, "no SOI");
    size_t pos = 2;
    bool have_sof = false, have_dht = false, have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
    uint8_t comp_id[3] = {0, 0, 0};
    const uint8_t* seg = nullptr;
    size_t n = 0;
    for (;;) {
        if (pos + 2 > len) JPEG_FAIL(AV_EJPEG_TRUNCATED, "ends where a marker should be");
        if (p[pos] != 0xFF) JPEG_FAIL(AV_EJPEG_FORMAT, "no marker where one should be");
        const int m = p[pos + 1];
        if (m == 0xFF) {          // fill byte
            pos += 1;
            continue;
        }
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;           // stand-alone markers
        if (m == 0xD9) JPEG_FAIL(AV_EJPEG_FORMAT, "EOI before any scan");
        if (pos + 2 > len) JPEG_FAIL(AV_EJPEG_TRUNCATED, "ends inside a segment length");
        const size_t L = (size_t)p[pos] * 256 + p[pos + 1];
        if (L < 2) JPEG_FAIL(AV_EJPEG_FORMAT, "segment length below 2");
        if (pos + L > len) JPEG_FAIL(AV_EJPEG_TRUNCATED, "ends inside a segment");
        seg = p + pos + 2, n = L - 2;
        pos += L;
        if (m == 0xC0) {
            if (have_sof) JPEG_FAIL(AV_EJPEG_FORMAT, "two frame headers");
            if (n < 6) JPEG_FAIL(AV_EJPEG_FORMAT, "short SOF0");
            if (seg[0] != 8) JPEG_FAIL(AV_EJPEG_PRECISION, "sample precision is not 8 bits");
            const int nc = seg[5];
            if (nc != 1 && nc != 3) JPEG_FAIL(AV_EJPEG_COMPONENTS, "neither 1 nor 3 components");
            if (n < (size_t)(6 + 3 * nc)) JPEG_FAIL(AV_EJPEG_FORMAT, "short SOF0");
            for (int c = 0; c < nc; ++c) {
                const int hv = seg[7 + 3 * c];
                comp_id[c] = seg[6 + 3 * c];
                if (seg[8 + 3 * c] > 3) JPEG_FAIL(AV_EJPEG_TABLE, "quantiser selector above 3");
                d->tq[c] = seg[8 + 3 * c];
                if (nc == 3 && (c == 0 ? (hv != 0x11 && hv != 0x21 && hv != 0x22) : hv != 0x11))
                    JPEG_FAIL(AV_EJPEG_SAMPLING, "sampling is none of 4:4:4, 4:2:2, 4:2:0");
                if (c == 0) d->hs = nc == 3 ? hv >> 4 : 1, d->vs = nc == 3 ? hv & 15 : 1;
            }
            d->height = seg[1] * 256 + seg[2], d->width = seg[3] * 256 + seg[4], d->ncomp = nc;
            if (d->height != h || d->width != w) JPEG_FAIL(AV_EJPEG_SIZE, "the frame has another size than the batch");
            have_sof = true;
        } else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) {
            JPEG_FAIL(AV_EJPEG_ARITH, "arithmetic coding");
        } else if (m >= 0xC1 && m <= 0xC7 && m != 0xC4) {
            JPEG_FAIL(AV_EJPEG_SOF, "not a baseline (SOF0) frame");
        } else if (m == 0xC4) {
            for (size_t i = 0; i < n;) {
                if (i + 17 > n) JPEG_FAIL(AV_EJPEG_FORMAT, "short DHT");
                const int tc = seg[i] >> 4, th = seg[i] & 15;
                if (tc > 1 || th > 1) JPEG_FAIL(AV_EJPEG_TABLE, "Huffman table class or slot above 1");
                const uint8_t* bits = seg + i + 1;
                int cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += bits[l];
                if (!bits_ok(bits, tc ? 256 : 16)) JPEG_FAIL(AV_EJPEG_TABLE, "Huffman table is no prefix code");
                if (i + 17 + (size_t)cnt > n) JPEG_FAIL(AV_EJPEG_FORMAT, "short DHT");
                uint8_t* db = tc ? d->ac_bits[th] : d->dc_bits[th];
                uint8_t* dv = tc ? d->ac_val[th] : d->dc_val[th];
                memset(dv, 0, tc ? 256 : 16);
                for (int l = 0; l < 16; ++l) db[l] = bits[l];
                for (int k = 0; k < cnt; ++k) {
                    if (!tc && seg[i + 17 + k] > 11) JPEG_FAIL(AV_EJPEG_TABLE, "DC category above 11");
                    dv[k] = seg[i + 17 + k];
                }
                have_h[tc * 2 + th] = have_dht = true;
                i += 17 + (size_t)cnt;
            }
        } else if (m == 0xDB) {
            for (size_t i = 0; i < n;) {
                if (seg[i] >> 4) JPEG_FAIL(AV_EJPEG_DQT16, "16-bit quantiser table");
                const int tq = seg[i] & 15;
                if (tq > 3) JPEG_FAIL(AV_EJPEG_TABLE, "quantiser slot above 3");
                if (i + 65 > n) JPEG_FAIL(AV_EJPEG_FORMAT, "short DQT");
                for (int k = 0; k < 64; ++k) d->qt[tq][zz[k]] = seg[i + 1 + k];
                have_q[tq] = true;
                i += 65;
            }
        } else if (m == 0xDD) {
            if (n < 2) JPEG_FAIL(AV_EJPEG_FORMAT, "short DRI");
            d->restart_interval = seg[0] * 256 + seg[1];
        } else if (m == 0xDA) {
            break;
        }                                                       // APPn, COM and anything else: skipped by its length
    }
    if (!have_sof) JPEG_FAIL(AV_EJPEG_FORMAT, "scan before the frame header");
    if (n < 1 || seg[0] != d->ncomp) JPEG_FAIL(AV_EJPEG_MULTISCAN, "the scan does not hold every component");
    if (n < (size_t)(4 + 2 * d->ncomp)) JPEG_FAIL(AV_EJPEG_FORMAT, "short SOS");
    for (int c = 0; c < d->ncomp; ++c) {
        if (seg[1 + 2 * c] != comp_id[c]) JPEG_FAIL(AV_EJPEG_SCAN, "scan components out of order");
        const int td = seg[2 + 2 * c] >> 4, ta = seg[2 + 2 * c] & 15;
        if (td > 1 || ta > 1) JPEG_FAIL(AV_EJPEG_TABLE, "Huffman table selector above 1");
        d->td[c] = (uint8_t)td, d->ta[c] = (uint8_t)ta;
        if (!have_q[d->tq[c]]) JPEG_FAIL(AV_EJPEG_TABLE, "quantiser table missing");
        if (have_dht && (!have_h[td] || !have_h[2 + ta])) JPEG_FAIL(AV_EJPEG_TABLE, "Huffman table missing");
    }
    const uint8_t* sp = seg + 1 + 2 * d->ncomp;
    if (sp[0] != 0 || sp[1] != 63 || sp[2] != 0) JPEG_FAIL(AV_EJPEG_SCAN, "not a sequential full scan (Ss 0, Se 63, Ah 0, Al 0)");
    if (!have_dht)
        for (int t = 0; t < 2; ++t) {
            memcpy(d->dc_bits[t], STD_DC_BITS[t], 16), memcpy(d->dc_val[t], STD_DC_VAL, 12);
            memcpy(d->ac_bits[t], STD_AC_BITS[t], 16), memcpy(d->ac_val[t], STD_AC_VAL[t], 162);
        }
    d->scan_offset = (int32_t)pos;
    const int n_mcus = ((w + 8 * d->hs - 1) / (8 * d->hs)) * ((h + 8 * d->vs - 1) / (8 * d->vs));
    const int want = d->restart_interval > 0 ? (n_mcus + d->restart_interval - 1) / d->restart_interval : 1;
    if (want > seg_cap) JPEG_FAIL(AV_EJPEG_SEGCAP, "more restart intervals than the segment table holds");
    d->n_segments = want;
    int found = 0;
    size_t q = pos, first = pos;
    while (q < len) {
        if (p[q] != 0xFF) {
            ++q;
            continue;
        }
        if (q + 1 >= len) {      // a lone FF at the very end stays data
            q = len;
            break;
        }
        const int m = p[q + 1];
        if (m == 0) {
            q += 2;
        } else if (m >= 0xD0 && m <= 0xD7) {
            if (found < want) segs[found].begin = (uint32_t)first, segs[found].end = (uint32_t)q;
            ++found;
            q += 2, first = q;
        } else if (m == 0xD9) {
            break;
        } else if (m == 0xDA) {
            JPEG_FAIL(AV_EJPEG_MULTISCAN, "a second scan");
        } else {
            ++q;
        }
    }
    if (found < want) segs[found].begin = (uint32_t)first, segs[found].end = (uint32_t)q;
    ++found;
    if (found != want) d->flags |= AV_JPEG_ESEGS;
    for (int i = found; i < want; ++i) segs[i].begin = segs[i].end = (uint32_t)q;
    *n_segs = want;
#undef JPEG_FAIL
    return 0;
}

}  // namespace jpeg
