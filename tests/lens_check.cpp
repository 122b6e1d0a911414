// Host side of the lens model in a stand-alone program (tests/test_lens_host.py builds it with -fsanitize=address,undefined on the
// host pass and runs it; no device is touched): av_lens_make on heap blocks of exactly sizeof(av_lens_cfg), every argument check of
// av_lens_map_rectify, av_lens_map_ground, av_remap and av_track_obstacles_ground_lens, each of which has to return AV_EINVAL
// before anything is launched, and lens_dev.h's model on the host.  The context is a default-constructed dummy: no check may read
// through it.  With the argument "dump" it also prints, as hexadecimal floats, what lens_dev.h computes for a fixed list of
// points and one small map: the test compares them bit for bit with tests/lens_ref.py.
#include "lens.hip"
#include "obstacles.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

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

static int make(const double* K, const double* dist, const double* N, int w, int h, bool* untouched) {
    av_lens_cfg* out = static_cast<av_lens_cfg*>(std::malloc(sizeof(av_lens_cfg)));
    std::memset(out, 0x5A, sizeof *out);
    const int rc = av_lens_make(K, dist, N, w, h, out);
    const unsigned char* b = reinterpret_cast<const unsigned char*>(out);
    *untouched = true;
    for (size_t i = 0; i < sizeof *out; ++i) *untouched = *untouched && b[i] == 0x5A;
    if (rc == AV_OK) {
        const double* n = N ? N : K;
        EXPECT(out->fx == K[0] && out->fy == K[1] && out->cx == K[2] && out->cy == K[3]);
        EXPECT(out->k1 == dist[0] && out->k2 == dist[1] && out->p1 == dist[2] && out->p2 == dist[3] && out->k3 == dist[4]);
        EXPECT(out->nfx == n[0] && out->nfy == n[1] && out->ncx == n[2] && out->ncy == n[3] && out->w == w && out->h == h);
    }
    std::free(out);
    return rc;
}

static void dump() {
    const double K[4] = {1000.0, 1000.0, 640.0, 360.0}, K2[4] = {1400.0, 1400.0, 640.0, 360.0}, N[4] = {900.0, 950.0, 600.0, 380.0};
    const double A[5] = {-0.30, 0.10, 1e-3, -5e-4, -0.02}, Cc[5] = {-0.40, 0.0, 0.0, 0.0, 0.0};
    av_lens_cfg lens[3];
    EXPECT(av_lens_make(K, A, nullptr, 1280, 720, &lens[0]) == AV_OK);
    EXPECT(av_lens_make(K, A, N, 1280, 720, &lens[1]) == AV_OK);
    EXPECT(av_lens_make(K2, Cc, nullptr, 1280, 720, &lens[2]) == AV_OK);
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 9; ++i)
            for (int j = 0; j < 9; ++j) {
                const double u = -40.0 + 200.25 * j, v = -30.5 + 110.125 * i;      // (the far corner lies beyond every fold)
                const lensdev::Undistorted p = lensdev::undistort(&lens[k], u, v);
                const lensdev::LensJac q = lensdev::jacobian(&lens[k], p);
                std::printf("P %d %a %a %a %a %a %a %d %a %a %a %a\n", k, u, v, p.x, p.y, p.u, p.v, p.valid ? 1 : 0, q.juu, q.juv, q.jvu, q.jvv);
            }
    // beyond the third lens's fold: no preimage
    const lensdev::Undistorted far = lensdev::undistort(&lens[2], 1500.0, 800.0);
    EXPECT(!far.valid);
    const double Ks[4] = {40.0, 42.0, 26.3, 18.1}, Ns[4] = {30.0, 32.0, 26.3, 18.1};
    av_lens_cfg small;
    EXPECT(av_lens_make(Ks, A, Ns, 53, 37, &small) == AV_OK);
    for (int r = 0; r < 37; ++r)
        for (int c = 0; c < 53; ++c) {
            int32_t e[2];
            raw_entry(&small, (double)c, (double)r, e);
            std::printf("M %d %d %d %d\n", r, c, e[0], e[1]);
        }
}

int main(int argc, char** argv) {
    static_assert(sizeof(av_lens_cfg) == 112, "av_lens_cfg is 112 bytes");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    bool same;
    const double K[4] = {1000.0, 1000.0, 640.0, 360.0}, K600[4] = {600.0, 600.0, 640.0, 360.0};
    const double A[5] = {-0.30, 0.10, 1e-3, -5e-4, -0.02}, Cc[5] = {-0.40, 0.0, 0.0, 0.0, 0.0}, Z[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    EXPECT(make(K, A, nullptr, 1280, 720, &same) == AV_OK && !same);
    EXPECT(make(K, Z, K600, 1280, 720, &same) == AV_OK && !same);
    EXPECT(make(K, Cc, nullptr, 1280, 720, &same) == AV_OK && !same);             // the fold lies outside the rectified frame
    EXPECT(make(K600, Cc, nullptr, 1280, 720, &same) == AV_EINVAL && same);       // and inside it at the shorter focal length
    EXPECT(make(K, Cc, K600, 1280, 720, &same) == AV_EINVAL && same);             // it is the RECTIFIED frame that counts
    for (int i = 0; i < 4; ++i)
        for (double bad : {inf, -inf, nan}) {
            double k[4];
            std::memcpy(k, K, sizeof k);
            k[i] = bad;
            EXPECT(make(k, A, nullptr, 1280, 720, &same) == AV_EINVAL && same);
            EXPECT(make(K, A, k, 1280, 720, &same) == AV_EINVAL && same);
        }
    for (int i = 0; i < 5; ++i)
        for (double bad : {inf, -inf, nan}) {
            double d[5];
            std::memcpy(d, A, sizeof d);
            d[i] = bad;
            EXPECT(make(K, d, nullptr, 1280, 720, &same) == AV_EINVAL && same);
        }
    for (int i = 0; i < 2; ++i)
        for (double bad : {0.0, -1000.0}) {
            double k[4];
            std::memcpy(k, K, sizeof k);
            k[i] = bad;
            EXPECT(make(k, A, nullptr, 1280, 720, &same) == AV_EINVAL && same);
            EXPECT(make(K, A, k, 1280, 720, &same) == AV_EINVAL && same);
        }
    for (int bad : {0, -1, 32769, 1 << 30}) {
        EXPECT(make(K, A, nullptr, bad, 720, &same) == AV_EINVAL && same);
        EXPECT(make(K, A, nullptr, 1280, bad, &same) == AV_EINVAL && same);
    }
    av_lens_cfg scratch;
    EXPECT(av_lens_make(nullptr, A, nullptr, 8, 8, &scratch) == AV_EINVAL && av_lens_make(K, nullptr, nullptr, 8, 8, &scratch) == AV_EINVAL &&
           av_lens_make(K, A, nullptr, 8, 8, nullptr) == AV_EINVAL);

    // the launching entry points: every call below is refused, so the pointers are never followed (1-byte blocks: a read would trap)
    av_ctx* ctx = new av_ctx();
    unsigned char* p = static_cast<unsigned char*>(std::malloc(1));
    unsigned char* p2 = static_cast<unsigned char*>(std::malloc(1));
    const av_lens_cfg* ln = reinterpret_cast<const av_lens_cfg*>(p);
    const av_ground_cfg* gr = reinterpret_cast<const av_ground_cfg*>(p);
    int32_t* pi = reinterpret_cast<int32_t*>(p);
    double* pd = reinterpret_cast<double*>(p);

    EXPECT(av_lens_map_rectify(nullptr, nullptr, ln, 1, 8, 8, pi) == AV_EINVAL);
    EXPECT(av_lens_map_rectify(ctx, nullptr, nullptr, 1, 8, 8, pi) == AV_EINVAL);
    EXPECT(av_lens_map_rectify(ctx, nullptr, ln, 1, 8, 8, nullptr) == AV_EINVAL);
    for (int bad : {0, -1, 65536, 1 << 30}) EXPECT(av_lens_map_rectify(ctx, nullptr, ln, bad, 8, 8, pi) == AV_EINVAL);
    for (int bad : {0, -1, 32769, 2147483647}) {
        EXPECT(av_lens_map_rectify(ctx, nullptr, ln, 1, bad, 8, pi) == AV_EINVAL);
        EXPECT(av_lens_map_rectify(ctx, nullptr, ln, 1, 8, bad, pi) == AV_EINVAL);
    }

    auto gmap = [&](av_ctx* c, const av_lens_cfg* l, const av_ground_cfg* g, int n, int gh, int gw, double f_far, double m, int32_t* map) {
        return av_lens_map_ground(c, nullptr, l, g, n, gh, gw, f_far, m, map);
    };
    EXPECT(gmap(nullptr, ln, gr, 1, 4, 4, 5.0, 0.5, pi) == AV_EINVAL);
    EXPECT(gmap(ctx, nullptr, gr, 1, 4, 4, 5.0, 0.5, pi) == AV_EINVAL);
    EXPECT(gmap(ctx, ln, nullptr, 1, 4, 4, 5.0, 0.5, pi) == AV_EINVAL);
    EXPECT(gmap(ctx, ln, gr, 1, 4, 4, 5.0, 0.5, nullptr) == AV_EINVAL);
    for (int bad : {0, -1, 65536, 1 << 30}) EXPECT(gmap(ctx, ln, gr, bad, 4, 4, 5.0, 0.5, pi) == AV_EINVAL);
    for (int bad : {0, -1}) {
        EXPECT(gmap(ctx, ln, gr, 1, bad, 4, 5.0, 0.5, pi) == AV_EINVAL);
        EXPECT(gmap(ctx, ln, gr, 1, 4, bad, 5.0, 0.5, pi) == AV_EINVAL);
    }
    EXPECT(gmap(ctx, ln, gr, 1, 2147483647, 4, 5.0, 0.5, pi) == AV_EINVAL);                 // more tile rows than a grid takes
    for (double bad : {0.0, -0.5, inf, nan}) EXPECT(gmap(ctx, ln, gr, 1, 4, 4, 5.0, bad, pi) == AV_EINVAL);
    for (double bad : {inf, -inf, nan}) EXPECT(gmap(ctx, ln, gr, 1, 4, 4, bad, 0.5, pi) == AV_EINVAL);

    const uint8_t fill[3] = {1, 2, 3};
    auto rm = [&](av_ctx* c, const int32_t* map, int n, int stride, int sh, int sw, const uint8_t* src, int dh, int dw, const uint8_t* fl,
                  uint8_t* out) { return av_remap(c, nullptr, map, n, stride, sh, sw, src, dh, dw, fl, out); };
    EXPECT(rm(nullptr, pi, 1, 1, 8, 8, p, 4, 4, fill, p2) == AV_EINVAL);
    EXPECT(rm(ctx, nullptr, 1, 1, 8, 8, p, 4, 4, fill, p2) == AV_EINVAL);
    EXPECT(rm(ctx, pi, 1, 1, 8, 8, nullptr, 4, 4, fill, p2) == AV_EINVAL);
    EXPECT(rm(ctx, pi, 1, 1, 8, 8, p, 4, 4, nullptr, p2) == AV_EINVAL);
    EXPECT(rm(ctx, pi, 1, 1, 8, 8, p, 4, 4, fill, nullptr) == AV_EINVAL);
    for (int bad : {0, -1, 65536, 1 << 30}) EXPECT(rm(ctx, pi, bad, 1, 8, 8, p, 4, 4, fill, p2) == AV_EINVAL);
    for (int bad : {0, -1, -(1 << 30)}) EXPECT(rm(ctx, pi, 2, bad, 8, 8, p, 4, 4, fill, p2) == AV_EINVAL);
    for (int bad : {0, -1, 32769, 2147483647}) {
        EXPECT(rm(ctx, pi, 1, 1, bad, 8, p, 4, 4, fill, p2) == AV_EINVAL);
        EXPECT(rm(ctx, pi, 1, 1, 8, bad, p, 4, 4, fill, p2) == AV_EINVAL);
    }
    for (int bad : {0, -1}) {
        EXPECT(rm(ctx, pi, 1, 1, 8, 8, p, bad, 4, fill, p2) == AV_EINVAL);
        EXPECT(rm(ctx, pi, 1, 1, 8, 8, p, 4, bad, fill, p2) == AV_EINVAL);
    }
    EXPECT(rm(ctx, pi, 1, 1, 8, 8, p, 2147483647, 4, fill, p2) == AV_EINVAL);               // more tile rows than a grid takes
    // out may overlap neither the source nor the table, not even by a byte (a block of its own, never read or written here)
    unsigned char* blk = static_cast<unsigned char*>(std::malloc(8192));
    uint8_t* src = blk + 1000;                                          // 8 x 8 x 3 = 192 bytes
    int32_t* tab = reinterpret_cast<int32_t*>(blk + 4096);              // 4 x 4 x 8 = 128 bytes
    EXPECT(rm(ctx, tab, 1, 1, 8, 8, src, 4, 4, fill, src) == AV_EINVAL);
    EXPECT(rm(ctx, tab, 1, 1, 8, 8, src, 4, 4, fill, src + 191) == AV_EINVAL);                // out starts on the source's last byte
    EXPECT(rm(ctx, tab, 1, 1, 8, 8, src, 4, 4, fill, src - 47) == AV_EINVAL);                 // out ends on the source's first byte
    EXPECT(rm(ctx, tab, 1, 1, 8, 8, src, 4, 4, fill, blk + 4096 + 127) == AV_EINVAL);         // out starts on the table's last byte
    EXPECT(rm(ctx, tab, 2, 2, 8, 8, src, 4, 4, fill, blk + 4096 - 95) == AV_EINVAL);          // two cameras' out ends on the one table
    std::free(blk);

    av_obstacle_cfg ocfg{};
    const av_track_row* snap = reinterpret_cast<const av_track_row*>(p);
    auto obs = [&](av_ctx* c, const av_obstacle_cfg* cfg, const av_ground_cfg* g, const av_lens_cfg* l, int stride, int mode, double rate, int n,
                   int tcap, const av_track_row* s, const int32_t* sn, const double* filt, const double* ps, int ocap, double* o, int32_t* no) {
        return av_track_obstacles_ground_lens(c, nullptr, cfg, g, l, stride, mode, rate, n, tcap, s, sn, filt, ps, ocap, o, no, nullptr);
    };
    for (int mode = 0; mode < 3; ++mode) {
        const double* filt = mode == 2 ? pd : nullptr;
        const double* wrong = mode == 2 ? nullptr : pd;
        EXPECT(obs(nullptr, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, nullptr, gr, ln, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, nullptr, ln, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, nullptr, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 0, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, -1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 0, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 0, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, nullptr, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, snap, nullptr, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, snap, pi, wrong, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, snap, pi, filt, nullptr, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 63, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, nullptr, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, nullptr) == AV_EINVAL);
        if (mode)
            for (double bad : {0.0, -30.0, inf, nan}) EXPECT(obs(ctx, &ocfg, gr, ln, 1, mode, bad, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
    }
    for (int bad : {-1, 3, 1 << 30}) EXPECT(obs(ctx, &ocfg, gr, ln, 1, bad, 30.0, 4, 64, snap, pi, nullptr, pd, 64, pd, pi) == AV_EINVAL);

    if (argc > 1 && std::strcmp(argv[1], "dump") == 0) dump();

    std::free(p);
    std::free(p2);
    delete ctx;
    if (failures) {
        std::fprintf(stderr, "%d checks failed (last error: %s)\n", failures, g_err);
        return 1;
    }
    std::puts("lens host checks ok");
    return 0;
}
