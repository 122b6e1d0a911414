// The bilinear sample of csrc/resample_dev.h in a stand-alone program (tests/test_resample_host.py builds it with
// -fsanitize=address,undefined on the host pass and runs it; no device is touched).  The header has the sample in two forms, the
// packed one (WIDE: two loads per source row, unsigned 32-bit blends) and the tap-by-tap one (rasterdev::resize_channel); here both
// are held against a third evaluation written out below from resize_channel's 64-bit formula, at every position of a grid that
// has both coordinates of every pixel, the last column and the last row exactly, and the weights 0, 1, 32768 and 65535.  The source
// frames are heap blocks of exactly h * w * 3 bytes, so a read past a row's end at the frame's last row, or past the block, is the
// sanitizer's to report.  The host halves of the header (pack_bgr, tile_grid, overlap) are checked on the way.
#include "resample_dev.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static char g_err[512];
void av_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }     // (the HIP runtime's own start-up allocations)

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// the rule, from its statement: bilinear, replicate border, 16-bit weights, 64-bit products, one rounding at the end
static unsigned rule(const uint8_t* src, int sh, int sw, long long tu, long long tv) {
    const long long x0 = tu >> 16, wx = tu & 65535, y0 = tv >> 16, wy = tv & 65535;
    const long long x1 = x0 + 1 < sw ? x0 + 1 : sw - 1, y1 = y0 + 1 < sh ? y0 + 1 : sh - 1;
    unsigned px = 0;
    for (int k = 0; k < 3; ++k) {
        const long long p00 = src[(y0 * sw + x0) * 3 + k], p01 = src[(y0 * sw + x1) * 3 + k];
        const long long p10 = src[(y1 * sw + x0) * 3 + k], p11 = src[(y1 * sw + x1) * 3 + k];
        const long long top = p00 * (65536 - wx) + p01 * wx, bot = p10 * (65536 - wx) + p11 * wx;
        px |= (unsigned)((top * (65536 - wy) + bot * wy + (1LL << 31)) >> 32) << (8 * k);
    }
    return px;
}

// every pixel of an axis of n pixels at the four weights, as far as the last pixel itself
static std::vector<long long> axis(int n) {
    std::vector<long long> t;
    const long long last = (long long)(n - 1) << 16;
    for (int p = 0; p < n; ++p)
        for (long long wgt : {0LL, 1LL, 32768LL, 65535LL})
            if (((long long)p << 16) + wgt <= last) t.push_back(((long long)p << 16) + wgt);
    return t;
}

// -> positions compared
static long long frame(int h, int w, int content) {
    const size_t bytes = (size_t)h * w * 3;
    uint8_t* src = static_cast<uint8_t*>(std::malloc(bytes));
    unsigned s = 12345u + (unsigned)(h * 131 + w);
    for (size_t i = 0; i < bytes; ++i) s = s * 1664525u + 1013904223u, src[i] = content ? 255 : (uint8_t)(s >> 24);
    const std::vector<long long> us = axis(w), vs = axis(h);
    EXPECT(us.front() == 0 && us.back() == (long long)(w - 1) << 16 && vs.front() == 0 && vs.back() == (long long)(h - 1) << 16);
    long long n = 0, bad = 0;
    for (long long tv : vs)
        for (long long tu : us) {
            const unsigned want = rule(src, h, w, tu, tv);
            bool same = resample::bilinear_bgr<false>(src, h, w, tu, tv) == want &&
                        resample::bilinear_bgr<false>(src, h, w, (int32_t)tu, (int32_t)tv) == want;
            if (w >= 2)
                same = same && resample::bilinear_bgr<true>(src, h, w, tu, tv) == want &&
                       resample::bilinear_bgr<true>(src, h, w, (int32_t)tu, (int32_t)tv) == want;
            if (!same && bad++ < 5) std::fprintf(stderr, "%d x %d, content %d: the forms differ at tu %lld, tv %lld\n", h, w, content, tu, tv);
            ++n;
        }
    EXPECT(bad == 0);
    if (content) EXPECT(rule(src, h, w, us.back(), vs.back()) == 0xffffffu);
    std::free(src);
    return n;
}

int main() {
    const int shapes[][2] = {{1, 1}, {5, 1}, {1, 2}, {5, 2}, {2, 3}, {37, 53}};
    long long n = 0;
    for (const auto& hw : shapes)
        for (int content = 0; content < 2; ++content) n += frame(hw[0], hw[1], content);
    // per frame (4 h - 3) x (4 w - 3) positions: a pixel's weights 1, 32768 and 65535 reach past the last pixel and are left out there
    long long want = 0;
    for (const auto& hw : shapes) want += 2LL * (4 * hw[0] - 3) * (4 * hw[1] - 3);
    EXPECT(n == want);

    // the host halves
    const uint8_t fill[3] = {1, 2, 3};
    EXPECT(resample::pack_bgr(fill) == 0x030201u);
    dim3 grid(7, 7, 7);
    EXPECT(resample::tile_grid(65, 17, 3, "entry", "things", &grid) == AV_OK && grid.x == 2 && grid.y == 2 && grid.z == 3);
    EXPECT(resample::tile_grid(2147483647, 65535 * 16, 65535, "entry", "things", &grid) == AV_OK && grid.x == 33554432u && grid.y == 65535u);
    grid = dim3(7, 7, 7);
    EXPECT(resample::tile_grid(4, 65535 * 16 + 1, 1, "entry", "things", &grid) == AV_EINVAL && grid.x == 7 &&
           !std::strcmp(g_err, "entry: more than 65535 things or tile rows"));
    EXPECT(resample::tile_grid(4, 4, 65536, "entry", "things", &grid) == AV_EINVAL && grid.z == 7);
    const char* base = reinterpret_cast<const char*>(uintptr_t(1) << 40);
    EXPECT(resample::overlap(base, 16, base + 15, 1) && !resample::overlap(base, 16, base + 16, 1) && !resample::overlap(base + 1, 1, base, 1));
    EXPECT(resample::overlap(base, ~(unsigned __int128)0 >> 1, base + 100, 1));          // a byte count past 2^64

    if (failures) {
        std::fprintf(stderr, "%d checks failed (last error: %s)\n", failures, g_err);
        return 1;
    }
    std::printf("resample host checks ok (%lld positions)\n", n);
    return 0;
}
