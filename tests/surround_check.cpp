// Host side of the surround view in a stand-alone program (tests/test_surround_host.py builds it with -fsanitize=address,undefined
// on the host pass and runs it; no device is touched): every argument check of av_rig_surround and av_rig_view_build, each of
// which has to return AV_EINVAL before anything is launched and before the context is looked at, and av_rig_view_prim_cap.  The
// context is a null pointer or a default-constructed dummy; the other pointers are 1-byte heap blocks: a read through one would trap.
#include "raster.hip"
#include "surround.hip"

#include <cmath>
#include <cstddef>
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

// raster.hip's av_bev_build asks tracker.hip for this; nothing here calls it
extern "C" size_t av_tracker_state_bytes(int, int) { std::abort(); }

extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }     // (the HIP runtime's own start-up allocations)

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// refused, and for the reason named
static bool refused(int rc, const char* why) { return rc == AV_EINVAL && std::strstr(g_err, why) != nullptr; }

int main() {
    static_assert(sizeof(av_surround_cfg) == 24, "av_surround_cfg is 24 bytes");
    static_assert(offsetof(av_surround_cfg, blend) == 16 && offsetof(av_surround_cfg, fill) == 20 && offsetof(av_surround_cfg, reserved) == 23,
                  "av_surround_cfg layout");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    av_ctx* ctx = new av_ctx();
    unsigned char* p = static_cast<unsigned char*>(std::malloc(1));
    unsigned char* far = static_cast<unsigned char*>(std::malloc(1));
    const av_rig_mount* mo = reinterpret_cast<const av_rig_mount*>(p);
    const av_ground_cfg* gr = reinterpret_cast<const av_ground_cfg*>(p);
    // a heap block of exactly sizeof(av_surround_cfg): a read past its end would trap
    av_surround_cfg* cfg = static_cast<av_surround_cfg*>(std::malloc(sizeof(av_surround_cfg)));
    const av_surround_cfg good = {6.0, 0.5, 0, {1, 2, 3}, 0};
    *cfg = good;

    // out and cover far from bgr: addresses only, never followed
    uint8_t* bgr = reinterpret_cast<uint8_t*>(uintptr_t(1) << 40);
    uint8_t* out = reinterpret_cast<uint8_t*>(uintptr_t(2) << 40);
    uint8_t* cov = reinterpret_cast<uint8_t*>(uintptr_t(3) << 40);
    auto sur = [&](av_ctx* c, const av_surround_cfg* cf, int V, int K, const av_rig_mount* m, const av_ground_cfg* g, int h, int w,
                   const uint8_t* src, int gh, int gw, uint8_t* o, uint8_t* cv) {
        g_err[0] = 0;
        return av_rig_surround(c, nullptr, cf, V, K, m, g, h, w, src, gh, gw, o, cv);
    };
    for (av_ctx* c : {static_cast<av_ctx*>(nullptr), ctx}) {
        for (int bad : {0, -1, 65536, 1 << 30}) EXPECT(sur(c, cfg, bad, 4, mo, gr, 8, 8, bgr, 4, 4, out, cov) == AV_EINVAL);
        for (int bad : {0, -1, 9, 1 << 30}) EXPECT(refused(sur(c, cfg, 2, bad, mo, gr, 8, 8, bgr, 4, 4, out, cov), "n_cams"));
        for (int bad : {0, -1, 32769, 1 << 30}) {
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, bad, 8, bgr, 4, 4, out, cov), "frame size"));
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, bad, bgr, 4, 4, out, cov), "frame size"));
        }
        for (int bad : {0, -1}) {
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, bad, 4, out, cov), "panel size"));
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, bad, out, cov), "panel size"));
        }
        EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, 2147483647, 4, out, cov), "tile rows"));      // more tile rows than a grid takes
        EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, 65535 * 16 + 1, 4, out, cov), "tile rows"));
        EXPECT(refused(sur(c, nullptr, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, cov), "null cfg"));
        for (double bad : {0.0, -0.5, inf, nan}) {
            *cfg = good, cfg->m_per_px = bad;
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, cov), "m_per_px"));
        }
        for (double bad : {inf, -inf, nan}) {
            *cfg = good, cfg->x_far = bad;
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, cov), "x_far"));
        }
        for (int bad : {-1, 2, 1 << 30}) {
            *cfg = good, cfg->blend = bad;
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, cov), "blend"));
        }
        for (int bad : {1, 255}) {
            *cfg = good, cfg->reserved = (uint8_t)bad;
            EXPECT(refused(sur(c, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, cov), "reserved"));
        }
        *cfg = good;
    }
    EXPECT(refused(sur(nullptr, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, cov), "null argument"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, nullptr, gr, 8, 8, bgr, 4, 4, out, cov), "null argument"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, nullptr, 8, 8, bgr, 4, 4, out, cov), "null argument"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, gr, 8, 8, nullptr, 4, 4, out, cov), "null argument"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, nullptr, cov), "null argument"));
    // bgr is 2 x 4 x 8 x 8 x 3 = 1536 bytes, out 2 x 4 x 4 x 3 = 96, cover 32
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, bgr, cov), "out overlaps"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, bgr + 1535, cov), "out overlaps"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, bgr - 95, cov), "out overlaps"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, bgr + 1535), "cover overlaps"));
    EXPECT(refused(sur(ctx, cfg, 2, 4, mo, gr, 8, 8, bgr, 4, 4, out, bgr - 31), "cover overlaps"));
    // sizes whose byte counts pass 2^64 are still compared rightly: this panel ends far beyond bgr's address
    EXPECT(refused(sur(ctx, cfg, 65535, 8, mo, gr, 32768, 32768, bgr, 65535 * 16, 2147483647, reinterpret_cast<uint8_t*>(16), nullptr),
                   "out overlaps"));

    // av_rig_view_prim_cap
    EXPECT(av_rig_view_prim_cap(7, 6, 5) == 5 + 4 + 14 + 1 && av_rig_view_prim_cap(1, 1, 1) == 3);
    EXPECT(av_rig_view_prim_cap(512, 50, 51) == 49 + 50 + 1024 + 1);
    EXPECT(av_rig_view_prim_cap(0, 6, 5) == 0 && av_rig_view_prim_cap(7, 0, 5) == 0 && av_rig_view_prim_cap(7, 6, 0) == 0);
    EXPECT(av_rig_view_prim_cap(-1, 6, 5) == 0 && av_rig_view_prim_cap(2147483647, 2147483647, 2147483647) == 0);

    // av_rig_view_build
    const double* pd = reinterpret_cast<const double*>(p);
    const int32_t* pi = reinterpret_cast<const int32_t*>(p);
    av_prim* pp = reinterpret_cast<av_prim*>(far);
    int32_t* np_ = reinterpret_cast<int32_t*>(far);
    const int cap = av_rig_view_prim_cap(7, 6, 5);
    auto view = [&](av_ctx* c, const av_surround_cfg* cf, int V, int gh, int gw, const double* ps, int ncol, int ocap, const double* ob,
                    const int32_t* no, const int32_t* ids, int rcap, const double* ref, const int32_t* nref, int ncand, int npts,
                    const double* wp, const int32_t* ord, av_prim* pr, int pcap, int32_t* npr) {
        g_err[0] = 0;
        return av_rig_view_build(c, nullptr, cf, V, gh, gw, ps, ncol, ocap, ob, no, ids, rcap, ref, nref, ncand, npts, wp, ord, pr, pcap, npr);
    };
    for (av_ctx* c : {static_cast<av_ctx*>(nullptr), ctx}) {
        for (int bad : {0, -1, 65536}) EXPECT(refused(view(c, cfg, bad, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "n_vehicles"));
        for (int bad : {0, -1, 8192}) {
            EXPECT(refused(view(c, cfg, 3, bad, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "panel size"));
            EXPECT(refused(view(c, cfg, 3, 80, bad, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "panel size"));
        }
        for (int bad : {0, 2, 4, 6, -3}) EXPECT(refused(view(c, cfg, 3, 80, 72, pd, bad, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "ncol"));
        for (int bad : {0, -1}) {
            EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, bad, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), ">= 1"));
            EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, bad, pd, pi, 4, 5, pd, pi, pp, cap, np_), ">= 1"));
            EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, bad, 5, pd, pi, pp, cap, np_), ">= 1"));
            EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, bad, pd, pi, pp, cap, np_), ">= 1"));
        }
        EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap - 1, np_), "prim_cap"));
        EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, 65536, np_), "prim_cap"));
        EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 40000, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, 65535, np_), "prim_cap"));
        EXPECT(refused(view(c, nullptr, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "null cfg"));
        for (double bad : {0.0, -0.5, inf, nan}) {
            *cfg = good, cfg->m_per_px = bad;
            EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "m_per_px"));
        }
        for (double bad : {inf, -inf, nan}) {
            *cfg = good, cfg->x_far = bad;
            EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "x_far"));
        }
        *cfg = good;
        EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, nullptr, pi, 4, 5, pd, pi, pp, cap, np_), "come together"));
        EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, nullptr, 4, 5, pd, pi, pp, cap, np_), "come together"));
        EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, nullptr, pi, pp, cap, np_), "come together"));
        EXPECT(refused(view(c, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, nullptr, pp, cap, np_), "come together"));
    }
    EXPECT(refused(view(nullptr, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "null argument"));
    EXPECT(refused(view(nullptr, cfg, 3, 80, 72, pd, 3, 7, pd, pi, nullptr, 6, nullptr, nullptr, 4, 5, nullptr, nullptr, pp, cap, np_), "null argument"));
    EXPECT(refused(view(ctx, cfg, 3, 80, 72, nullptr, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "null argument"));
    EXPECT(refused(view(ctx, cfg, 3, 80, 72, pd, 5, 7, nullptr, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "null argument"));
    EXPECT(refused(view(ctx, cfg, 3, 80, 72, pd, 5, 7, pd, nullptr, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, np_), "null argument"));
    EXPECT(refused(view(ctx, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, nullptr, cap, np_), "null argument"));
    EXPECT(refused(view(ctx, cfg, 3, 80, 72, pd, 5, 7, pd, pi, pi, 6, pd, pi, 4, 5, pd, pi, pp, cap, nullptr), "null argument"));

    std::free(cfg);
    std::free(far);
    std::free(p);
    delete ctx;
    if (failures) {
        std::fprintf(stderr, "%d checks failed (last error: %s)\n", failures, g_err);
        return 1;
    }
    std::puts("surround host checks ok");
    return 0;
}
