// Host side of the camera model in a stand-alone program (tests/test_ground_host.py builds it with -fsanitize=address,undefined on
// the host pass and runs it; no device is touched): av_ground_make on heap blocks of exactly sizeof(av_ground_cfg), and every
// argument check of av_track_obstacles_ground, av_lane_paths_ground and av_ground_warp, each of which has to return AV_EINVAL
// before anything is launched.  The context is a default-constructed dummy: no check may read through it.
#include "bridge.hip"
#include "ground.hip"
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

static int make(const double* g, double max_range, int anchor, bool* untouched) {
    av_ground_cfg* out = static_cast<av_ground_cfg*>(std::malloc(sizeof(av_ground_cfg)));
    std::memset(out, 0x5A, sizeof *out);
    const int rc = av_ground_make(g, max_range, anchor, out);
    const unsigned char* b = reinterpret_cast<const unsigned char*>(out);
    *untouched = true;
    for (size_t i = 0; i < sizeof *out; ++i) *untouched = *untouched && b[i] == 0x5A;
    if (rc == AV_OK) {
        // g ginv = I to a few ulp of the largest product
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double s = 0.0, mag = 0.0;
                for (int k = 0; k < 3; ++k) s += out->g[r * 3 + k] * out->ginv[k * 3 + c], mag = std::fmax(mag, std::fabs(out->g[r * 3 + k] * out->ginv[k * 3 + c]));
                EXPECT(std::fabs(s - (r == c ? 1.0 : 0.0)) <= 1e-12 * std::fmax(mag, 1.0));
            }
        EXPECT(out->max_range == max_range && out->anchor == anchor && out->reserved == 0);
    }
    std::free(out);
    return rc;
}

int main() {
    static_assert(sizeof(av_ground_cfg) == 160, "av_ground_cfg is 160 bytes");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    bool same;
    const double g0[9] = {0.0, -10.0, 6000.0, 1.0, 0.0, -640.0, 0.0, 1.0, -300.0};
    EXPECT(make(g0, 50.0, 1, &same) == AV_OK && !same);
    const double lin[9] = {0.0, -0.1, 50.0, 0.03, 0.0, -9.6, 0.0, 0.0, 1.0};
    EXPECT(make(lin, 1e9, 0, &same) == AV_OK && !same);
    for (int i = 0; i < 9; ++i)
        for (double bad : {inf, -inf, nan}) {
            double g[9];
            std::memcpy(g, g0, sizeof g);
            g[i] = bad;
            EXPECT(make(g, 50.0, 1, &same) == AV_EINVAL && same);
        }
    const double sing[9] = {1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 1.0, 5.0}, zero[9] = {0.0};
    EXPECT(make(sing, 50.0, 1, &same) == AV_EINVAL && same);
    EXPECT(make(zero, 50.0, 1, &same) == AV_EINVAL && same);
    double tiny[9], huge[9];
    for (int i = 0; i < 9; ++i) tiny[i] = g0[i] * 1e-150, huge[i] = g0[i] * 1e120;
    EXPECT(make(tiny, 50.0, 1, &same) == AV_EINVAL && same);       // the determinant underflows to 0
    EXPECT(make(huge, 50.0, 1, &same) == AV_EINVAL && same);       // the determinant overflows
    for (double bad : {0.0, -1.0, inf, nan}) EXPECT(make(g0, bad, 1, &same) == AV_EINVAL && same);
    for (int bad : {-1, 2, 1 << 30}) EXPECT(make(g0, 50.0, bad, &same) == AV_EINVAL && same);
    av_ground_cfg scratch;
    EXPECT(av_ground_make(nullptr, 50.0, 1, &scratch) == AV_EINVAL && av_ground_make(g0, 50.0, 1, nullptr) == AV_EINVAL);

    // the launching entry points: every call below is refused, so the pointers are never followed (1-byte blocks: a read would trap)
    av_ctx* ctx = new av_ctx();
    unsigned char* p = static_cast<unsigned char*>(std::malloc(1));
    av_obstacle_cfg ocfg{};
    const av_ground_cfg* gr = reinterpret_cast<const av_ground_cfg*>(p);
    const av_track_row* snap = reinterpret_cast<const av_track_row*>(p);
    int32_t* pi = reinterpret_cast<int32_t*>(p);
    double* pd = reinterpret_cast<double*>(p);
    auto obs = [&](av_ctx* c, const av_obstacle_cfg* cfg, const av_ground_cfg* g, int stride, int mode, double rate, int n, int tcap,
                   const av_track_row* s, const int32_t* sn, const double* filt, const double* ps, int ocap, double* o, int32_t* no) {
        return av_track_obstacles_ground(c, nullptr, cfg, g, stride, mode, rate, n, tcap, s, sn, filt, ps, ocap, o, no, nullptr);
    };
    for (int mode = 0; mode < 3; ++mode) {
        const double* filt = mode == 2 ? pd : nullptr;
        const double* wrong = mode == 2 ? nullptr : pd;
        EXPECT(obs(nullptr, &ocfg, gr, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, nullptr, gr, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, nullptr, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 0, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, -1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 0, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 0, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 64, nullptr, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 64, snap, nullptr, filt, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 64, snap, pi, wrong, pd, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 64, snap, pi, filt, nullptr, 64, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 63, pd, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, nullptr, pi) == AV_EINVAL);
        EXPECT(obs(ctx, &ocfg, gr, 1, mode, 30.0, 4, 64, snap, pi, filt, pd, 64, pd, nullptr) == AV_EINVAL);
        if (mode)
            for (double bad : {0.0, -30.0, inf, nan}) EXPECT(obs(ctx, &ocfg, gr, 1, mode, bad, 4, 64, snap, pi, filt, pd, 64, pd, pi) == AV_EINVAL);
    }
    for (int bad : {-1, 3, 1 << 30}) EXPECT(obs(ctx, &ocfg, gr, 1, bad, 30.0, 4, 64, snap, pi, nullptr, pd, 64, pd, pi) == AV_EINVAL);

    auto lanes = [&](av_ctx* c, const av_ground_cfg* g, int S, int h, int w, int np, const double* poly, const int32_t* pts,
                     const int32_t* info, const double* ps, int stride, int rcap, double* ref, int32_t* nref) {
        return av_lane_paths_ground(c, nullptr, g, S, h, w, np, poly, pts, info, ps, stride, rcap, ref, nref, nullptr);
    };
    EXPECT(lanes(nullptr, gr, 2, 720, 1280, 50, pd, pi, pi, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, nullptr, 2, 720, 1280, 50, pd, pi, pi, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, nullptr, pi, pi, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, pd, nullptr, pi, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, pd, pi, nullptr, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, pd, pi, pi, nullptr, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, pd, pi, pi, pd, 1, 50, nullptr, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, pd, pi, pi, pd, 1, 50, pd, nullptr) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 0, 720, 1280, 50, pd, pi, pi, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 0, 1280, 50, pd, pi, pi, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 0, 50, pd, pi, pi, pd, 1, 50, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, pd, pi, pi, pd, 0, 50, pd, pi) == AV_EINVAL);
    for (int bad : {-1, 0, 1, 65, 1 << 30}) EXPECT(lanes(ctx, gr, 2, 720, 1280, bad, pd, pi, pi, pd, 1, 1 << 30, pd, pi) == AV_EINVAL);
    EXPECT(lanes(ctx, gr, 2, 720, 1280, 50, pd, pi, pi, pd, 1, 49, pd, pi) == AV_EINVAL);

    const uint8_t fill[3] = {1, 2, 3};
    auto warp = [&](av_ctx* c, const av_ground_cfg* g, int n, int h, int w, const uint8_t* src, int gh, int gw, double f_far, double m,
                    const uint8_t* fl, uint8_t* out) { return av_ground_warp(c, nullptr, g, n, h, w, src, gh, gw, f_far, m, fl, out); };
    EXPECT(warp(nullptr, gr, 1, 8, 8, p, 4, 4, 5.0, 0.5, fill, p) == AV_EINVAL);
    EXPECT(warp(ctx, nullptr, 1, 8, 8, p, 4, 4, 5.0, 0.5, fill, p) == AV_EINVAL);
    EXPECT(warp(ctx, gr, 1, 8, 8, nullptr, 4, 4, 5.0, 0.5, fill, p) == AV_EINVAL);
    EXPECT(warp(ctx, gr, 1, 8, 8, p, 4, 4, 5.0, 0.5, nullptr, p) == AV_EINVAL);
    EXPECT(warp(ctx, gr, 1, 8, 8, p, 4, 4, 5.0, 0.5, fill, nullptr) == AV_EINVAL);
    for (int bad : {0, -1, 65536, 1 << 30}) EXPECT(warp(ctx, gr, bad, 8, 8, p, 4, 4, 5.0, 0.5, fill, p) == AV_EINVAL);
    for (int bad : {0, -1}) {
        EXPECT(warp(ctx, gr, 1, bad, 8, p, 4, 4, 5.0, 0.5, fill, p) == AV_EINVAL);
        EXPECT(warp(ctx, gr, 1, 8, bad, p, 4, 4, 5.0, 0.5, fill, p) == AV_EINVAL);
        EXPECT(warp(ctx, gr, 1, 8, 8, p, bad, 4, 5.0, 0.5, fill, p) == AV_EINVAL);
        EXPECT(warp(ctx, gr, 1, 8, 8, p, 4, bad, 5.0, 0.5, fill, p) == AV_EINVAL);
    }
    EXPECT(warp(ctx, gr, 1, 8, 8, p, 2147483647, 4, 5.0, 0.5, fill, p) == AV_EINVAL);        // more tile rows than a grid takes
    for (double bad : {0.0, -0.5, inf, nan}) EXPECT(warp(ctx, gr, 1, 8, 8, p, 4, 4, 5.0, bad, fill, p) == AV_EINVAL);
    for (double bad : {inf, -inf, nan}) EXPECT(warp(ctx, gr, 1, 8, 8, p, 4, 4, bad, 0.5, fill, p) == AV_EINVAL);

    std::free(p);
    delete ctx;
    if (failures) {
        std::fprintf(stderr, "%d checks failed (last error: %s)\n", failures, g_err);
        return 1;
    }
    std::puts("ground host checks ok");
    return 0;
}
