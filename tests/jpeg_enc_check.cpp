// Stand-alone host program over csrc/jpeg_enc_dev.h for tests/test_mjpeg_encode_host.py, built with the address and undefined-behaviour
// sanitizers: the frame header, the per-block bit count and emit, the interval padding and the byte stuffing the device runs, on the
// CPU in the kernels' order, with every buffer a heap block of exactly the size the code is entitled to.
//   in : int32 n, then per case: int32 h, w, quality, subsampling, restart_mcus, out_cap; n_blocks * 64 int16 coefficients (scan order,
//        zigzag)
//   out: per case: int32 rc (0, or -1 when the parameters are refused); when 0: int32 len, status, then out_cap bytes (the slot)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "jpeg_enc_dev.h"

struct PlainStore {
    void merge(uint32_t* p, uint32_t v) const { *p |= v; }
    void own(uint32_t* p, uint32_t v) const { *p = v; }
};

template <class T>
static T* heap(size_t n) {
    return (T*)std::calloc(n ? n : 1, sizeof(T));
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    static const jpege::Tables T = jpege::make_tables();
    int32_t n = 0;
    if (std::fread(&n, 4, 1, in) != 1 || n < 0) return 1;
    for (int32_t v = 0; v < n; ++v) {
        int32_t hd[6];
        if (std::fread(hd, 4, 6, in) != 6) return 1;
        const int h = hd[0], w = hd[1], quality = hd[2], sub = hd[3], restart = hd[4], out_cap = hd[5];
        jpege::Geom g;
        uint8_t qt[2][64], hbuf[jpege::HEADER_MAX];
        const int header_len = jpege::write_header(h, w, quality, sub, restart, hbuf, (int)sizeof hbuf, qt);
        int32_t rc = header_len > 0 && out_cap >= 0 && jpege::geom(h, w, sub, restart, g) ? 0 : -1;
        std::fwrite(&rc, 4, 1, out);
        if (rc) return 2;                      // the coefficient count is unknown then: the test sends no such case
        uint8_t* header = heap<uint8_t>((size_t)header_len);
        std::memcpy(header, hbuf, (size_t)header_len);
        int16_t* coef = (int16_t*)std::aligned_alloc(16, (size_t)g.n_blocks * 128);
        if (std::fread(coef, 128, (size_t)g.n_blocks, in) != (size_t)g.n_blocks) return 1;
        // size
        uint32_t* bits = heap<uint32_t>((size_t)g.n_blocks);
        for (int b = 0; b < g.n_blocks; ++b) {
            const int pb = jpege::pred_block(g, b);
            jpege::CountSink s;
            jpege::code_block(T, coef + (size_t)b * 64, pb < 0 ? 0 : (int)coef[(size_t)pb * 64], b % g.bpm >= g.nl, s);
            bits[b] = s.bits;
        }
        // scan, prefix
        uint32_t *ubytes = heap<uint32_t>((size_t)g.n_int), *ustart = heap<uint32_t>((size_t)g.n_int);
        uint32_t *sbytes = heap<uint32_t>((size_t)g.n_int), *sstart = heap<uint32_t>((size_t)g.n_int);
        uint32_t utotal = 0;
        for (int i = 0; i < g.n_int; ++i) {
            const int b0 = i * g.ri * g.bpm, b1 = (((i + 1) * g.ri < g.n_mcus) ? (i + 1) * g.ri : g.n_mcus) * g.bpm;
            uint32_t run = 0;
            for (int b = b0; b < b1; ++b) {
                const uint32_t x = bits[b];
                bits[b] = run, run += x;
            }
            ubytes[i] = (run + 7) >> 3, ustart[i] = utotal, utotal += ubytes[i];
        }
        if ((size_t)utotal + 4 > jpege::stream_cap(g.n_blocks, g.n_mcus)) return 3;
        // pack into a zeroed stream of whole dwords
        const uint32_t cap_words = (utotal + 3) / 4;
        uint32_t* words = heap<uint32_t>(cap_words);
        for (int b = 0; b < g.n_blocks; ++b) {
            const int pb = jpege::pred_block(g, b), i = (b / g.bpm) / g.ri;
            const int b1 = (((i + 1) * g.ri < g.n_mcus) ? (i + 1) * g.ri : g.n_mcus) * g.bpm;
            jpege::WordSink<PlainStore> s(PlainStore(), words, (uint64_t)ustart[i] * 8 + bits[b], cap_words);
            jpege::code_block(T, coef + (size_t)b * 64, pb < 0 ? 0 : (int)coef[(size_t)pb * 64], b % g.bpm >= g.nl, s);
            s.finish(b + 1 == b1);
        }
        // the stream as exactly utotal bytes
        uint8_t* stream = heap<uint8_t>(utotal);
        std::memcpy(stream, words, utotal);
        // count, prefix
        uint32_t stotal = 0;
        for (int i = 0; i < g.n_int; ++i) {
            uint32_t ff = 0;
            for (uint32_t off = 0; off < ubytes[i]; off += 4) ff += jpege::count_ff(stream + ustart[i] + off, ubytes[i] - off < 4 ? ubytes[i] - off : 4);
            sbytes[i] = ubytes[i] + ff, sstart[i] = stotal, stotal += sbytes[i] + (i < g.n_int - 1 ? 2 : 0);
        }
        const int64_t L = (int64_t)header_len + stotal + 2, limit = out_cap;
        const int32_t len = (int32_t)L, status = L > out_cap ? AV_JPEG_EFULL : 0;
        // gather
        uint8_t* slot = heap<uint8_t>((size_t)out_cap);
        for (int i = 0; i < g.n_int; ++i) {
            const int64_t pos0 = (int64_t)header_len + sstart[i];
            uint32_t run = 0;
            for (uint32_t off = 0; off < ubytes[i]; off += 4) {
                const uint32_t m = ubytes[i] - off < 4 ? ubytes[i] - off : 4;
                jpege::stuff_bytes(stream + ustart[i] + off, m, slot, pos0 + off + run, limit);
                run += jpege::count_ff(stream + ustart[i] + off, m);
            }
            if (i < g.n_int - 1) {
                const int64_t p = pos0 + sbytes[i];
                if (p < limit) slot[p] = 0xFF;
                if (p + 1 < limit) slot[p + 1] = (uint8_t)(0xD0 + (i & 7));
            }
        }
        for (int k = 0; k < header_len && k < out_cap; ++k) slot[k] = header[k];
        if (L - 2 < limit) slot[L - 2] = 0xFF;
        if (L - 1 < limit) slot[L - 1] = 0xD9;
        std::fwrite(&len, 4, 1, out), std::fwrite(&status, 4, 1, out);
        std::fwrite(slot, 1, (size_t)out_cap, out);
        std::free(slot), std::free(stream), std::free(words), std::free(sstart), std::free(sbytes), std::free(ustart), std::free(ubytes);
        std::free(bits), std::free(coef), std::free(header);
    }
    std::fclose(out);
    std::fclose(in);
    return 0;
}
