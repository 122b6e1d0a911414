// Rig odometry (include/avhot.h: av_rig_egoflow_*): a vehicle's ego motion from the road pixels of all K cameras of its rig, fitted
// together in the vehicle frame.  The patch and match stages are egoflow.hip's over V * K cameras (their ping-pong slot follows the
// vehicle's frame counter); the measure stage is egoflow.hip's over V vehicles.  New here is the solve:
//   one workgroup per vehicle, one wave per camera (at most 8 waves).  Wave k votes and gates camera k's table exactly as
//   av_egoflow_solve does (a histogram of its own in LDS), carries its gated rows through the mount into the vehicle frame and sums
//   them: per lane in tile order, then the wave's fixed tree.  The waves' sums meet in LDS and every wave adds them in the order
//   k = 0 .. K - 1, so all waves hold the same hypotheses -- the pooled fit and one fit per camera --, count their own rows under
//   each, agree on the best through LDS again, and repeat the sums over its inliers for the final fit.
// Every pass reads the camera's rows again (L2 hits: 56 bytes a row, a few rows a lane) and recomputes (X, Y, DX, DY) from them, so
// that nothing per row lives across the workgroup's barriers; no scratch, no global atomics.  The header states the arithmetic;
// DESIGN.md 7t has the layout and the measurements.
#include "egoflow_dev.h"

static_assert(sizeof(av_rig_mount) == 32, "av_rig_mount is 4 doubles (include/avhot.h)");

namespace {

using namespace egoflow;

constexpr int MAX_CAMS = 8;                     // cameras per rig: av_rig_fuse's
constexpr int MAX_HYP = MAX_CAMS + 1;           // the pooled fit and one per camera

// a gated row in the vehicle frame
struct Row {
    double X, Y;
    Disp D;
};
__device__ __forceinline__ Row vehicle_row(const av_egoflow_tile& t, const av_rig_mount& mt, double m_per_px) {
    const Disp d = displacement(t, m_per_px);
    Row r;
    r.X = (mt.x + mt.c * t.f) - mt.s * t.l;
    r.Y = (mt.y + mt.s * t.f) + mt.c * t.l;
    r.D.df = mt.c * d.df - mt.s * d.dl;
    r.D.dl = mt.s * d.df + mt.c * d.dl;
    return r;
}
// the cameras' sums added in the order k = 0 .. K - 1
__device__ __forceinline__ Fit fit_of_cameras(const Sums* part, const int* part_n, int K) {
    Sums s = part[0];
    int n = part_n[0];
    for (int k = 1; k < K; ++k) {
        const Sums p = part[k];
        n += part_n[k], s.sf += p.sf, s.sl += p.sl, s.q += p.q, s.b1 += p.b1, s.b2 += p.b2, s.b3 += p.b3;
    }
    return fit_of_sums(n, s);
}

__global__ void __launch_bounds__(64 * MAX_CAMS) rig_egoflow_solve_kernel(int K, int n_tiles, int R, int gate, double m_per_px,
                                                                           double thr2, int min_inliers,
                                                                           const av_rig_mount* __restrict__ mounts,
                                                                           av_egoflow_tile* __restrict__ tiles,
                                                                           av_egoflow_motion* __restrict__ motion,
                                                                           av_rig_egoflow_info* __restrict__ info) {
    __shared__ int hist[MAX_CAMS][MAX_BINS];
    __shared__ Sums part[2][MAX_CAMS];                              // the gated rows' sums, then the inliers'
    __shared__ int part_n[2][MAX_CAMS], acc_n[MAX_CAMS], vote_bin[MAX_CAMS];
    __shared__ int hyp_n[MAX_HYP][MAX_CAMS];                        // [hypothesis][camera]: the camera's rows within the limit
    __shared__ double part_ss[MAX_CAMS];
    const int v = blockIdx.x, k = (int)(threadIdx.x >> 6), lane = lane_id(), C1 = 2 * R + 1;
    const int cam = v * K + k;
    av_egoflow_tile* tl = tiles + (size_t)cam * n_tiles;
    const av_rig_mount mt = mounts[cam];

    // 1. vote and gate, per camera
    int n_acc;
    const int bin = vote(hist[k], tl, n_tiles, R, lane, n_acc);
    const int my = bin / C1 - R, mx = bin % C1 - R;
    auto gated = [&](const av_egoflow_tile& t) { return accepted(t, R) && abs(t.dy - my) <= gate && abs(t.dx - mx) <= gate; };

    // 2., 3. the camera's gated rows in the vehicle frame, summed
    {
        int n = 0;
        Sums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = lane; i < n_tiles; i += 64) {
            const av_egoflow_tile t = tl[i];
            if (!gated(t)) continue;
            const Row r = vehicle_row(t, mt, m_per_px);
            ++n, add_row(s, r.X, r.Y, r.D);
        }
        n = wave_sum_i(n);
        s = wave_sums(s);
        if (lane == 0) part[0][k] = s, part_n[0][k] = n, acc_n[k] = n_acc, vote_bin[k] = bin;
    }
    __syncthreads();

    // 4. the hypotheses (every wave computes the same ones) and this camera's rows under each
    Fit hyp[MAX_HYP];
    hyp[0] = fit_of_cameras(part[0], part_n[0], K);
#pragma unroll
    for (int i = 1; i < MAX_HYP; ++i) hyp[i] = i <= K ? fit_of_sums(part_n[0][i - 1], part[0][i - 1]) : Fit{0.0, 0.0, 0.0, 0, false};
    {
        int cnt[MAX_HYP];
#pragma unroll
        for (int i = 0; i < MAX_HYP; ++i) cnt[i] = 0;
        for (int i = lane; i < n_tiles; i += 64) {
            const av_egoflow_tile t = tl[i];
            if (!gated(t)) continue;
            const Row r = vehicle_row(t, mt, m_per_px);
#pragma unroll
            for (int j = 0; j < MAX_HYP; ++j)
                if (hyp[j].ok && !(residual2(r.X, r.Y, r.D, hyp[j]) > thr2)) ++cnt[j];
        }
#pragma unroll
        for (int i = 0; i < MAX_HYP; ++i) {
            const int c = wave_sum_i(cnt[i]);
            if (lane == 0) hyp_n[i][k] = c;
        }
    }
    __syncthreads();
    int best = -1, best_n = -1, count[MAX_HYP];
#pragma unroll
    for (int i = 0; i < MAX_HYP; ++i) {
        count[i] = -1;
        if (hyp[i].ok) {                                            // (uniform)
            int c = 0;
            for (int j = 0; j < K; ++j) c += hyp_n[i][j];
            count[i] = c;
            if (c > best_n) best_n = c, best = i;                   // the largest count, among equals the smallest i
        }
    }
    Fit h{0.0, 0.0, 0.0, 0, false};
#pragma unroll
    for (int i = 0; i < MAX_HYP; ++i)
        if (i == best) h = hyp[i];

    // 5. the final fit over the best hypothesis' inliers
    {
        int n = 0;
        Sums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (h.ok)
            for (int i = lane; i < n_tiles; i += 64) {
                const av_egoflow_tile t = tl[i];
                if (!gated(t)) continue;
                const Row r = vehicle_row(t, mt, m_per_px);
                if (residual2(r.X, r.Y, r.D, h) > thr2) continue;
                ++n, add_row(s, r.X, r.Y, r.D);
            }
        n = wave_sum_i(n);
        s = wave_sums(s);
        if (lane == 0) part[1][k] = s, part_n[1][k] = n;
    }
    __syncthreads();
    const Fit B = h.ok ? fit_of_cameras(part[1], part_n[1], K) : Fit{0.0, 0.0, 0.0, 0, false};
    // flags, and the final fit's squared residuals over its rows
    {
        double ss = 0.0;
        for (int i = lane; i < n_tiles; i += 64) {
            const av_egoflow_tile t = tl[i];
            int fl = t.flags & (AV_EGOFLOW_ACCEPTED | AV_EGOFLOW_LIVE);
            if (gated(t)) {
                fl |= AV_EGOFLOW_GATED;
                const Row r = vehicle_row(t, mt, m_per_px);
                if (h.ok && !(residual2(r.X, r.Y, r.D, h) > thr2)) {
                    fl |= AV_EGOFLOW_INLIER;
                    if (B.ok) ss += residual2(r.X, r.Y, r.D, B);
                }
            }
            tl[i].flags = fl;
        }
        ss = wave_sum_dpp(ss);
        if (lane == 0) part_ss[k] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        av_egoflow_motion o;
        av_rig_egoflow_info f;
        double ss = part_ss[0];
        int n_accepted = 0, n_gated = 0, views = 0;
        for (int j = 1; j < K; ++j) ss += part_ss[j];
        for (int j = 0; j < MAX_CAMS; ++j) {
            const bool on = j < K;
            const int b = on ? vote_bin[j] : R * C1 + R;
            f.cam_accepted[j] = on ? acc_n[j] : 0, f.cam_gated[j] = on ? part_n[0][j] : 0, f.cam_inliers[j] = on ? part_n[1][j] : 0;
            f.cam_vote_dy[j] = on ? b / C1 - R : 0, f.cam_vote_dx[j] = on ? b % C1 - R : 0;
            n_accepted += f.cam_accepted[j], n_gated += f.cam_gated[j];
            if (f.cam_inliers[j] > 0) views |= 1 << j;
        }
#pragma unroll
        for (int i = 0; i < MAX_HYP; ++i) f.hyp_count[i] = count[i];
        f.hypothesis = best, f.views = views, f.reserved[0] = f.reserved[1] = 0, f.pad = 0;
        o.t_f = B.ok ? B.tf : 0.0, o.t_l = B.ok ? B.tl : 0.0, o.omega = B.ok ? B.om : 0.0;
        o.rms = B.ok ? sqrt(ss / (double)B.n) : 0.0;
        o.n_accepted = n_accepted, o.n_gated = n_gated, o.n_inliers = h.ok ? B.n : 0;
        o.valid = B.ok && B.n >= min_inliers;
        o.vote_dy = o.vote_dx = 0, o.reserved[0] = o.reserved[1] = 0;
        motion[v] = o;
        info[v] = f;
    }
}

int launch_rig_solve(av_stream_t stream, const av_egoflow_cfg* c, const Geom& g, int n_vehicles, int n_cams, const av_rig_mount* mounts,
                     av_egoflow_tile* tiles, av_egoflow_motion* motion, av_rig_egoflow_info* info) {
    const double thr = c->inlier_px * c->m_per_px;
    hipLaunchKernelGGL(rig_egoflow_solve_kernel, dim3((unsigned)n_vehicles), dim3(64 * (unsigned)n_cams), 0, as_stream(stream), n_cams,
                       g.n_tiles, g.R, c->gate_px, c->m_per_px, thr * thr, c->min_inliers, mounts, tiles, motion, info);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// the header's checks of the rig's shape
int rig_shape(int n_vehicles, int n_cams, const char* who) {
    AV_REQUIRE(n_vehicles >= 1, AV_EINVAL, "%s: n_vehicles must be >= 1", who);
    AV_REQUIRE(n_cams >= 1 && n_cams <= MAX_CAMS, AV_EINVAL, "%s: n_cams must be 1 .. %d", who, MAX_CAMS);
    AV_REQUIRE((long long)n_vehicles * n_cams <= 65535, AV_EINVAL, "%s: more than 65535 cameras", who);
    return AV_OK;
}

}  // namespace

extern "C" int av_rig_egoflow_solve(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_vehicles, int n_cams,
                                    const av_rig_mount* mounts, av_egoflow_tile* tiles, av_egoflow_motion* motion,
                                    av_rig_egoflow_info* info) {
    AV_REQUIRE(ctx && mounts && tiles && motion && info, AV_EINVAL, "av_rig_egoflow_solve: null argument");
    if (int rc = rig_shape(n_vehicles, n_cams, "av_rig_egoflow_solve")) return rc;
    Geom g;
    if (int rc = geometry(cfg, "av_rig_egoflow_solve", &g)) return rc;
    return launch_rig_solve(stream, cfg, g, n_vehicles, n_cams, mounts, tiles, motion, info);
}

extern "C" int av_rig_egoflow_update(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, const av_ground_cfg* ground,
                                     const av_rig_mount* mounts, int n_vehicles, int n_cams, int h, int w, const uint8_t* bgr,
                                     uint8_t* patches, uint32_t* valid, av_egoflow_tile* tiles, av_egoflow_motion* motion,
                                     av_rig_egoflow_info* info, av_egoflow_state* state, double* z, uint8_t* mode) {
    AV_REQUIRE(ctx && ground && mounts && bgr && patches && valid && tiles && motion && info && state && z && mode, AV_EINVAL,
               "av_rig_egoflow_update: null argument");
    if (int rc = rig_shape(n_vehicles, n_cams, "av_rig_egoflow_update")) return rc;
    AV_REQUIRE(h >= 1 && w >= 1, AV_EINVAL, "av_rig_egoflow_update: h and w must be >= 1");
    Geom g;
    if (int rc = geometry(cfg, "av_rig_egoflow_update", &g)) return rc;
    const int n = n_vehicles * n_cams;
    const size_t pair = (size_t)2 * g.gh * g.gw;
    if (int rc = launch_patch(stream, cfg, g, ground, n, h, w, bgr, patches, pair, state, n_cams, valid)) return rc;
    if (int rc = launch_match(stream, cfg, g, n, patches, patches, pair, state, n_cams, valid, tiles)) return rc;
    if (int rc = launch_rig_solve(stream, cfg, g, n_vehicles, n_cams, mounts, tiles, motion, info)) return rc;
    return launch_measure(stream, cfg, n_vehicles, motion, state, z, mode);
}
