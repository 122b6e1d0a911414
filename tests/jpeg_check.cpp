// Stand-alone host program over csrc/jpeg_dev.h for tests/test_mjpeg_host.py, built with the address and undefined-behaviour
// sanitizers: the header parse, the segment walk and the per-segment entropy decode the device runs, on the CPU, with every buffer
// a heap block of exactly the size the decoder is entitled to.
//   in : int32 n, then per frame: int32 h, w, full, len; len bytes
//   out: per frame: int32 rc; when rc == 0: int32 status, n_blocks, uint32 crc32 of the int16 coefficients, and when `full` the
//        n_blocks * 64 coefficients themselves
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_dev.h"

static uint32_t crc32_of(const uint8_t* p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            tab[i] = c;
        }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t n = 0;
    if (std::fread(&n, 4, 1, in) != 1 || n < 0) return 1;
    for (int32_t v = 0; v < n; ++v) {
        int32_t hd[4];
        if (std::fread(hd, 4, 4, in) != 4) return 1;
        const int h = hd[0], w = hd[1], full = hd[2];
        const size_t len = (size_t)hd[3];
        uint8_t* data = (uint8_t*)std::malloc(len ? len : 1);
        if (len && std::fread(data, 1, len, in) != len) return 1;
        const int seg_cap = ((w + 7) / 8) * ((h + 7) / 8);
        av_jpeg_seg* segs = (av_jpeg_seg*)std::malloc(sizeof(av_jpeg_seg) * (size_t)seg_cap);
        av_jpeg_desc* d = (av_jpeg_desc*)std::malloc(sizeof(av_jpeg_desc));
        int n_segs = 0;
        const char* why = "";
        const int32_t rc = jpeg::parse(data, len, h, w, d, segs, seg_cap, &n_segs, &why);
        std::fwrite(&rc, 4, 1, out);
        if (rc == 0) {
            jpeg::Geom g;
            if (!jpeg::geom_from(*d, h, w, g) || n_segs != d->n_segments) return 3;
            // the upload: the frame's bytes, rounded up to whole dwords, plus 8 bytes of padding
            const size_t n_bytes = ((len + 3) & ~(size_t)3) + 8;
            uint32_t* words = (uint32_t*)std::calloc(n_bytes / 4, 4);
            std::memcpy(words, data, len);
            const uint32_t limit = (uint32_t)(n_bytes - 4);
            int16_t* coef = (int16_t*)std::calloc((size_t)g.n_blocks * 64, 2);
            jpeg::Tables* T = (jpeg::Tables*)std::malloc(sizeof(jpeg::Tables));
            for (int t = 0; t < 4; ++t) jpeg::build_table(*d, *T, t);
            jpeg::build_zigzag(*T);
            int32_t status = d->flags;
            const int ri = d->restart_interval;
            for (int i = 0; i < n_segs; ++i) {
                if (segs[i].begin > segs[i].end || segs[i].end > len) return 4;           // the parse bounds every offset
                const uint32_t end = segs[i].end < limit ? segs[i].end : limit, begin = segs[i].begin < end ? segs[i].begin : end;
                status |= jpeg::decode_segment(*d, g, *T, words, begin, end, ri > 0 ? i * ri : 0, ri > 0 ? ri : g.n_mcus, coef);
            }
            const int32_t nb = g.n_blocks;
            const uint32_t crc = crc32_of((const uint8_t*)coef, (size_t)nb * 128);
            std::fwrite(&status, 4, 1, out), std::fwrite(&nb, 4, 1, out), std::fwrite(&crc, 4, 1, out);
            if (full) std::fwrite(coef, 2, (size_t)nb * 64, out);
            std::free(T), std::free(coef), std::free(words);
        }
        std::free(d), std::free(segs), std::free(data);
    }
    std::fclose(out);
    std::fclose(in);
    return 0;
}
