// Stand-alone host program over csrc/fmtnum.h for tests/test_fmtnum_host.py, built with the address and undefined-behaviour
// sanitizers: reads doubles (int64 count, then the values), writes "%.0f", "%.1f" and "%.2f" of each as lines of text, and
// formats every one into a heap buffer of exactly the needed size and into one a byte short (which has to be refused).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fmtnum.h"

static int fail(const char* what, double v, int d) {
    std::fprintf(stderr, "fmtnum_check: %s for %.17g, %d decimals\n", what, v, d);
    return 2;
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "w");
    if (!in || !out) return 1;
    long long n = 0;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0) return 1;
    std::vector<double> v((size_t)n);
    if (n && std::fread(v.data(), sizeof(double), (size_t)n, in) != (size_t)n) return 1;
    for (long long i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) {
            char wide[32];
            const int len = fmtnum::fmt_fixed(v[(size_t)i], d, wide, (int)sizeof wide);
            if (len <= 0 || len > fmtnum::MAX_FIXED) return fail("bad length", v[(size_t)i], d);
            char* exact = (char*)std::malloc((size_t)len);
            if (fmtnum::fmt_fixed(v[(size_t)i], d, exact, len) != len || std::memcmp(exact, wide, (size_t)len)) return fail("exact buffer", v[(size_t)i], d);
            std::free(exact);
            char* tight = (char*)std::malloc((size_t)len - 1 + (len == 1));
            if (fmtnum::fmt_fixed(v[(size_t)i], d, tight, len - 1) != -1) return fail("short buffer accepted", v[(size_t)i], d);
            std::free(tight);
            std::fwrite(wide, 1, (size_t)len, out);
            std::fputc('\n', out);
        }
    // the int32 text: both ends and zero, the same two buffers
    const int32_t ints[] = {0, 7, -7, 2147483647, (-2147483647 - 1), 1000000000, -1000000000, 59};
    for (int32_t x : ints) {
        char wide[16];
        const int len = fmtnum::fmt_int(x, wide, (int)sizeof wide);
        char want[16];
        if (len != std::snprintf(want, sizeof want, "%d", x) || std::memcmp(want, wide, (size_t)len)) return fail("int text", (double)x, 0);
        char* exact = (char*)std::malloc((size_t)len);
        if (fmtnum::fmt_int(x, exact, len) != len) return fail("int exact buffer", (double)x, 0);
        std::free(exact);
        char* tight = (char*)std::malloc((size_t)len - 1 + (len == 1));
        if (fmtnum::fmt_int(x, tight, len - 1) != -1) return fail("int short buffer accepted", (double)x, 0);
        std::free(tight);
    }
    std::fclose(out);
    std::fclose(in);
    return 0;
}
