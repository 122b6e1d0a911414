// Camera rigs (av_rig_fuse): the obstacle lists of a vehicle's K cameras carried into the vehicle frame and merged where two
// cameras see one object; the piece between the per-camera ground projection (obstacles.hip) and the per-state planner.
//
// The reference has one camera and no fusion; what it does have is the greedy association of its tracker
// (multi_object_tracker.py:136-159: best pair first, each row and each column taken once), which this kernel follows with the
// squared distance on the road in place of the IoU.  Semantics and operation order: include/avhot.h.
//
// Mapping: one 512-thread workgroup per vehicle, cameras visited in turn (a round).  The clusters (at most 8 x 64 = 512, ten
// doubles each, with the class lane's weight and class) and the round's candidates (at most 64) live in LDS, 60 KB in all; the rows themselves are read once, up front,
// wave k taking camera k's list and holding it in registers until its round.  Thread (j, s) = (tid & 63, tid >> 6) owns
// candidate j's view of cluster slice s (clusters s, s + 8, ...): it keeps the nearest admissible cluster of its slice that is
// still free.  A wave therefore reads one cluster at a time, the same for all its lanes (an LDS broadcast).  A match iteration:
// every thread posts its slice's best, wave 0 folds the eight slices per candidate and picks the winner over the candidates with a
// wave reduction on (d2, i, j), and only the threads whose posted cluster was the one just taken scan their slice again -- at most
// 64 clusters each.  A round is bounded by its candidate count (<= 64 iterations), whatever the distances are.
// float64, -ffp-contract=off: every operation rounded on its own.
#include "rig_dev.h"

#include <cmath>

namespace {

constexpr int MAX_CAMS = 8, MAX_IN = 64, MAX_CL = MAX_CAMS * MAX_IN, SLICES = 8, THREADS = SLICES * 64;
constexpr int NONE_KEY = 0x7fffffff;

struct Shared {
    // clusters, in creation order
    double X[MAX_CL], Y[MAX_CL], r[MAX_CL], VX[MAX_CL], VY[MAX_CL];          // where the cluster stands (what distances are taken from)
    double sw[MAX_CL], sx[MAX_CL], sy[MAX_CL], svx[MAX_CL], svy[MAX_CL];     // the weighted sums of its members
    int32_t views[MAX_CL];
    int32_t taken[MAX_CL];                                                   // this round: the cluster has absorbed a candidate
    // the round's candidates, kept rows only, in row order
    double cX[MAX_IN], cY[MAX_IN], cr[MAX_IN], cw[MAX_IN], cVX[MAX_IN], cVY[MAX_IN];
    int32_t match[MAX_IN];                                                   // the cluster that takes candidate j, -1: none
    double best_d2[SLICES][MAX_IN];                                          // what thread (j, s) posts
    int32_t best_i[SLICES][MAX_IN];
    int32_t n_cand, n_clusters, win_i, win_j;
    int32_t skipped[MAX_CAMS];                                               // per camera: rows not taken
    // the class lane (av_rig_fuse_cls): the class of the member with the largest weight, the earliest among equals
    double best_w[MAX_CL];
    int32_t cls[MAX_CL];
    int32_t ccls[MAX_IN];
};
static_assert(sizeof(Shared) <= 64 * 1024, "the fuse kernel's static LDS");

// candidate j against the still-free clusters s, s + 8, ... < m0: the nearest admissible one, the smallest index among equals
__device__ __forceinline__ void scan_slice(const Shared& sh, const av_rig_cfg& cfg, int s, int m0, double x, double y, double r,
                                           double& bd, int& bi) {
    bd = INFINITY, bi = -1;
    for (int i = s; i < m0; i += SLICES) {
        if (sh.taken[i]) continue;
        double d2;
        if (rig_pair(sh.X[i], sh.Y[i], sh.r[i], x, y, r, cfg.merge_min, cfg.merge_scale, d2) && d2 < bd) bd = d2, bi = i;
    }
}

template <int NCOL>
__global__ void __launch_bounds__(THREADS) rig_fuse_kernel(av_rig_cfg cfg, int n_cams, const av_rig_mount* __restrict__ mounts,
                                                           int ocap_in, const double* __restrict__ cam_obs,
                                                           const int32_t* __restrict__ cam_n, const double* __restrict__ plan_state,
                                                           int ocap, double* __restrict__ obstacles, int32_t* __restrict__ n_obs,
                                                           int32_t* __restrict__ views, int32_t* __restrict__ n_skip,
                                                           const int32_t* __restrict__ cam_cls, int32_t* __restrict__ cls) {
    constexpr bool MOVING = NCOL == 5;
    __shared__ Shared sh;
    const int tid = (int)threadIdx.x, j = tid & 63, s = tid >> 6;
    const size_t v = blockIdx.x;
    const double x0 = plan_state[v * 4], y0 = plan_state[v * 4 + 1], h = plan_state[v * 4 + 2];
    const double v0 = MOVING ? plan_state[v * 4 + 3] : 0.0;
    // ---- every camera's rows at once: wave k reads camera k's list, one row per lane, and keeps its kept rows (carried into the
    // vehicle frame) in registers until round k -- one round trip to memory for the whole vehicle ----
    bool keep = false;
    int slot = 0, n_kept = 0;       // the row's place among its camera's kept rows; their number
    double qX = 0.0, qY = 0.0, qr = 0.0, qw = 0.0, qVX = 0.0, qVY = 0.0;
    int qcls = 0;
    if (s < n_cams) {
        const size_t list = v * (size_t)n_cams + (size_t)s;
        int n = cam_n[list];
        n = n < 0 ? 0 : (n > ocap_in ? ocap_in : n);                         // <= ocap_in <= 64: one row per lane
        const av_rig_mount mt = mounts[list];
        if (j < ocap_in) {                                                   // (the row is inside the list whatever n is: its load
            const double* row = cam_obs + (list * (size_t)ocap_in + (size_t)j) * NCOL;       // does not wait for the count's)
            const double x = row[0], y = row[1];
            qr = row[2];
            if (cam_cls) qcls = cam_cls[list * (size_t)ocap_in + (size_t)j];
            keep = j < n && std::isfinite(x) && std::isfinite(y) && std::isfinite(qr) && qr > 0.0;
            double vx = 0.0, vy = 0.0;
            if constexpr (MOVING) {
                vx = row[3], vy = row[4];
                keep = keep && std::isfinite(vx) && std::isfinite(vy);
            }
            const double mm = fmax(x * x + y * y, 1.0);
            qw = 1.0 / (mm * mm);
            qX = (mt.x + mt.c * x) - mt.s * y;
            qY = (mt.y + mt.s * x) + mt.c * y;
            if constexpr (MOVING) {
                qVX = mt.c * vx - mt.s * vy;
                qVY = mt.s * vx + mt.c * vy;
            }
        }
        const unsigned long long km = __ballot(keep);
        slot = __popcll(km & ((1ull << j) - 1ull));                          // < 64
        n_kept = __popcll(km);
        const int skipped = __popcll(__ballot(j < n && !keep));
        if (j == 0) sh.skipped[s] = skipped;
    }
    double sn, cs, s2, c2;          // (the start state's sines here, while the rows are on their way)
    sincos(h, &sn, &cs);
    sincos(h + 1.5707963267948966, &s2, &c2);
    int m = 0;                      // clusters so far (the same in every thread)
    for (int k = 0; k < n_cams; ++k) {
        const int m0 = m;
        // ---- the round's candidates: wave k hands over its kept rows, compacted in row order ----
        if (s == k) {
            if (keep) {
                sh.cX[slot] = qX, sh.cY[slot] = qY, sh.cr[slot] = qr, sh.cw[slot] = qw, sh.ccls[slot] = qcls;
                if constexpr (MOVING) sh.cVX[slot] = qVX, sh.cVY[slot] = qVY;
            }
            sh.match[j] = -1;
            if (j == 0) sh.n_cand = n_kept;
        }
        if (tid < m0) sh.taken[tid] = 0;                                     // m0 <= 512 = the workgroup
        __syncthreads();
        const int nc = sh.n_cand;
        // ---- association against the m0 clusters of the round's start ----
        bool active = j < nc;
        double x = 0.0, y = 0.0, r = 0.0, bd = INFINITY;
        int bi = -1;
        if (active) {
            x = sh.cX[j], y = sh.cY[j], r = sh.cr[j];
            scan_slice(sh, cfg, s, m0, x, y, r, bd, bi);
        }
        for (int it = 0; it < nc; ++it) {                                    // (every thread runs the same iterations: barriers inside)
            sh.best_d2[s][j] = active ? bd : INFINITY;
            sh.best_i[s][j] = active ? bi : -1;
            __syncthreads();
            if (s == 0) {
                double d = INFINITY;
                int key = NONE_KEY;
#pragma unroll
                for (int q = 0; q < SLICES; ++q) {                           // candidate j's nearest over the slices: (d2, i)
                    const double qd = sh.best_d2[q][j];
                    const int qi = sh.best_i[q][j];
                    if (qi >= 0 && (qd < d || (qd == d && ((qi << 6) | j) < key))) d = qd, key = (qi << 6) | j;
                }
                // the winner over the candidates, (d2, i, j): the smallest d2 (never NaN, -0.0 never posted), then the smallest key
                // among the lanes that hold it, both by DPP reductions (common.h)
                const double dmin = -wave_max(-d);
                const unsigned inv = wave_max_u32(key != NONE_KEY && d == dmin ? ~(unsigned)key : 0u);   // keys < 2^15: ~key > 0
                key = inv ? (int)~inv : NONE_KEY;
                if (j == 0) {
                    const bool any = key != NONE_KEY;
                    sh.win_i = any ? key >> 6 : -1, sh.win_j = any ? key & 63 : -1;
                    if (any) sh.taken[key >> 6] = 1, sh.match[key & 63] = key >> 6;       // key >> 6 < m0, key & 63 < nc
                }
            }
            __syncthreads();
            const int wi = sh.win_i, wj = sh.win_j;
            if (wi < 0) break;                                               // (uniform: read behind the barrier)
            if (j == wj) active = false;
            if (active && bi == wi) scan_slice(sh, cfg, s, m0, x, y, r, bd, bi);          // the cluster this thread posted is gone
        }
        // ---- absorption, new clusters (wave 0: a cluster takes at most one candidate per round, so no two lanes meet) ----
        if (s == 0) {
            const bool cand = j < nc;
            const int mi = cand ? sh.match[j] : -1;
            const bool fresh = cand && mi < 0;
            const unsigned long long fm = __ballot(fresh);
            if (cand) {
                const double w = sh.cw[j];
                if (mi >= 0) {
                    const double sw = sh.sw[mi] + w, sx = sh.sx[mi] + w * x, sy = sh.sy[mi] + w * y;
                    sh.sw[mi] = sw, sh.sx[mi] = sx, sh.sy[mi] = sy;
                    sh.X[mi] = sx / sw, sh.Y[mi] = sy / sw;
                    if constexpr (MOVING) {
                        const double svx = sh.svx[mi] + w * sh.cVX[j], svy = sh.svy[mi] + w * sh.cVY[j];
                        sh.svx[mi] = svx, sh.svy[mi] = svy;
                        sh.VX[mi] = svx / sw, sh.VY[mi] = svy / sw;
                    }
                    sh.r[mi] = fmax(sh.r[mi], r);
                    sh.views[mi] |= 1 << k;
                    if (w > sh.best_w[mi]) sh.best_w[mi] = w, sh.cls[mi] = sh.ccls[j];
                } else {
                    const int ni = m0 + __popcll(fm & ((1ull << j) - 1ull));             // < m0 + nc <= (k + 1) * 64 <= 512
                    sh.sw[ni] = w, sh.sx[ni] = w * x, sh.sy[ni] = w * y;
                    sh.X[ni] = x, sh.Y[ni] = y, sh.r[ni] = r, sh.views[ni] = 1 << k;
                    sh.best_w[ni] = w, sh.cls[ni] = sh.ccls[j];
                    if constexpr (MOVING) {
                        const double cvx = sh.cVX[j], cvy = sh.cVY[j];
                        sh.svx[ni] = w * cvx, sh.svy[ni] = w * cvy, sh.VX[ni] = cvx, sh.VY[ni] = cvy;
                    }
                }
            }
            if (j == 0) sh.n_clusters = m0 + __popcll(fm);
        }
        __syncthreads();
        m = sh.n_clusters;
    }
    // ---- cluster i -> row i, in the planner's frame (av_track_obstacles' placement) ----
    if (tid < m) {                                                           // m <= n_cams * ocap_in <= ocap
        const double X = sh.X[tid], Y = sh.Y[tid];
        double* o = obstacles + (v * (size_t)ocap + (size_t)tid) * NCOL;
        o[0] = (x0 + X * cs) + Y * c2;
        o[1] = (y0 + X * sn) + Y * s2;
        o[2] = sh.r[tid];
        if constexpr (MOVING) {
            const double vf = sh.VX[tid] + v0, vl = sh.VY[tid];
            o[3] = vf * cs + vl * c2;
            o[4] = vf * sn + vl * s2;
        }
        if (views) views[v * (size_t)ocap + (size_t)tid] = sh.views[tid];
        if (cls) cls[v * (size_t)ocap + (size_t)tid] = sh.cls[tid];
    }
    if (tid == 0) {
        n_obs[v] = m;
        if (n_skip) {
            int skipped = 0;
            for (int k = 0; k < n_cams; ++k) skipped += sh.skipped[k];       // (written ahead of the rounds' barriers)
            n_skip[v] = skipped;
        }
    }
}

}  // namespace

static int rig_fuse(const char* who, av_ctx* ctx, av_stream_t stream, const av_rig_cfg* cfg, int n_vehicles, int n_cams,
                    const av_rig_mount* mounts, int ncol, int ocap_in, const double* cam_obs, const int32_t* cam_n,
                    const double* plan_state, int ocap, double* obstacles, int32_t* n_obs, int32_t* views, int32_t* n_skip,
                    const int32_t* cam_cls, int32_t* cls) {
    AV_REQUIRE(ctx && cfg && mounts && cam_obs && cam_n && plan_state && obstacles && n_obs, AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE((cam_cls != nullptr) == (cls != nullptr), AV_EINVAL, "%s: cam_cls and cls are given together or not at all", who);
    AV_REQUIRE(n_vehicles >= 1, AV_EINVAL, "%s: n_vehicles must be >= 1", who);
    AV_REQUIRE(n_cams >= 1 && n_cams <= MAX_CAMS, AV_EINVAL, "%s: n_cams %d not in 1..%d", who, n_cams, MAX_CAMS);
    AV_REQUIRE(ocap_in >= 1 && ocap_in <= MAX_IN, AV_EINVAL, "%s: ocap_in %d not in 1..%d", who, ocap_in, MAX_IN);
    AV_REQUIRE(ncol == 3 || ncol == 5, AV_EINVAL, "%s: ncol %d is neither 3 (x, y, r) nor 5 (x, y, r, vx, vy)", who, ncol);
    AV_REQUIRE(ocap >= n_cams * ocap_in, AV_EINVAL, "%s: ocap %d < n_cams * ocap_in = %d (no obstacle is ever dropped)", who, ocap,
               n_cams * ocap_in);
    AV_REQUIRE(std::isfinite(cfg->merge_scale) && std::isfinite(cfg->merge_min) && cfg->merge_scale >= 0.0 && cfg->merge_min >= 0.0,
               AV_EINVAL, "%s: merge_scale and merge_min must be >= 0 and finite", who);
    if (ncol == 5)
        hipLaunchKernelGGL(rig_fuse_kernel<5>, dim3((unsigned)n_vehicles), dim3(THREADS), 0, as_stream(stream), *cfg, n_cams, mounts,
                           ocap_in, cam_obs, cam_n, plan_state, ocap, obstacles, n_obs, views, n_skip, cam_cls, cls);
    else
        hipLaunchKernelGGL(rig_fuse_kernel<3>, dim3((unsigned)n_vehicles), dim3(THREADS), 0, as_stream(stream), *cfg, n_cams, mounts,
                           ocap_in, cam_obs, cam_n, plan_state, ocap, obstacles, n_obs, views, n_skip, cam_cls, cls);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_rig_fuse(av_ctx* ctx, av_stream_t stream, const av_rig_cfg* cfg, int n_vehicles, int n_cams,
                           const av_rig_mount* mounts, int ncol, int ocap_in, const double* cam_obs, const int32_t* cam_n,
                           const double* plan_state, int ocap, double* obstacles, int32_t* n_obs, int32_t* views, int32_t* n_skip) {
    return rig_fuse("av_rig_fuse", ctx, stream, cfg, n_vehicles, n_cams, mounts, ncol, ocap_in, cam_obs, cam_n, plan_state, ocap,
                    obstacles, n_obs, views, n_skip, nullptr, nullptr);
}

extern "C" int av_rig_fuse_cls(av_ctx* ctx, av_stream_t stream, const av_rig_cfg* cfg, int n_vehicles, int n_cams,
                               const av_rig_mount* mounts, int ncol, int ocap_in, const double* cam_obs, const int32_t* cam_n,
                               const int32_t* cam_cls, const double* plan_state, int ocap, double* obstacles, int32_t* n_obs,
                               int32_t* views, int32_t* n_skip, int32_t* cls) {
    return rig_fuse("av_rig_fuse_cls", ctx, stream, cfg, n_vehicles, n_cams, mounts, ncol, ocap_in, cam_obs, cam_n, plan_state, ocap,
                    obstacles, n_obs, views, n_skip, cam_cls, cls);
}
