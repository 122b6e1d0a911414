// Tracker tables -> planner obstacles (av_track_obstacles): the link between the tracking and the planning end of the loop.
//
// The reference has none (MotionPlanner.plan is called without obstacles, demo.py:118-120); what it does have
// is the place where it DRAWS a track in the road plane, BEVRenderer (bev_renderer.py:207-208: forward = 50 - cy * 0.1 m, lateral =
// (cx - 320) * 0.03 m, the constants of av_bev_build in raster.hip), and the way MotionPlanner places a point of lateral offset d at
// arc length s ahead of a start state (motion_planner.py:175-180).  Put together: a confirmed track becomes the obstacle a candidate
// of lateral offset l meets at arc length f.
//
// Mapping: one wave per start state (= one frame of one stream), lane = table row, 64 rows per round.  Confirmed rows whose class has
// a positive radius are compacted in table order by ballot + prefix count; every lane writes its own 24-byte (x, y, radius) row.
// float64 in the operation order include/avhot.h states (-ffp-contract=off: no FMA), the planner's own for a waypoint.
//
// The moving form (av_track_obstacles_moving) adds the track's velocity in the planner's frame to every row: the row's last centre
// difference (px / frame, Track.velocity, multi_object_tracker.py:35-47) scaled like the position and by the frame rate, plus the
// ego's own speed along its heading -- the image is ego-centric, so a track at rest in it moves with the ego.  Same wave per
// state, same compaction; a kept lane writes 40 bytes (x, y, radius, vx, vy).
//
// The filtered form (av_track_obstacles_filtered) is the moving form with the track's centre and velocity taken from the per-track
// Kalman filter's output row (av_track_filter_update, trackfilter.hip) in place of the box and of the last centre difference: a
// coasting track's disc sits where the filter predicts it.  Same selection, order, count and radius.
//
// The ground forms (av_track_obstacles_ground, modes 0..2) are the same kernel with a camera in place of the four linear
// scales: the row's foot point (av_ground_cfg.anchor) goes through the ground-plane homography of the state's camera (entry
// f / cam_stride of a device table), a row whose foot is not on the road is dropped and counted in n_off, and the pixel velocity
// is carried to metres per second by the projection's Jacobian at the foot.  The table entry is the same for a whole wave.
//
// The lens form (av_track_obstacles_ground_lens) takes the rows in RAW pixels: the foot is undistorted first (lens_dev.h: six
// Newton iterations on the Brown-Conrady model of the state's camera), a foot with no valid preimage is off the road, and the
// pixel velocity goes through the undistortion's Jacobian before the projection's.
//
// The class form (av_track_obstacles_ground_cls) is either of the two with an int32 lane beside the obstacle rows: a kept lane also
// writes its row's class, for the fuse and the tracker behind it (rig.hip, rigtrack.hip) to carry on.
#include "common.h"
#include "ground_dev.h"
#include "lens_dev.h"

#include <cmath>
#include <type_traits>

namespace {

enum { STATIC = 0, MOVING_ROWS = 1, FILTERED = 2 };

// what the ground forms take on top of the linear ones; the linear forms carry the empty struct
struct Linear {};
struct Ground {
    const av_ground_cfg* table;     // device [n_cams]
    int cam_stride;                 // state f uses table[f / cam_stride]
    int32_t* n_off;                 // [n_states] or NULL
    int32_t* obs_cls;               // [n_states][ocap] or NULL: the class of the row behind each obstacle
};
struct GroundLens {
    const av_ground_cfg* table;     // as Ground
    int cam_stride;
    int32_t* n_off;
    int32_t* obs_cls;
    const av_lens_cfg* lens;        // device [n_cams], beside table: the rows are raw pixels
};

// MODE != STATIC: rows of 5 doubles, frame_rate in frames per second (unused otherwise); FILTERED: centre and velocity of row i
// from filt [n_states][tcap][6] (cx, cy, vx, vy, ., .), NULL otherwise
// VIA = Ground / GroundLens: cfg's radius[] only, the place and the velocity through the camera VIA names
template <int MODE, typename VIA>
__global__ void __launch_bounds__(256) track_obstacles_kernel(av_obstacle_cfg cfg, double frame_rate, int n_states, int tcap,
                                                              const av_track_row* __restrict__ snap,
                                                              const int32_t* __restrict__ snap_n,
                                                              const double* __restrict__ plan_state, int ocap,
                                                              double* __restrict__ obstacles, int32_t* __restrict__ n_obs,
                                                              const double* __restrict__ filt, VIA via) {
    constexpr bool MOVING = MODE != STATIC;
    constexpr bool GROUND = sizeof(VIA) > 1;
    constexpr bool LENS = std::is_same<VIA, GroundLens>::value;
    const int lane = threadIdx.x & 63;
    const long long fl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fl >= n_states) return;
    const int f = (int)fl;
    int n = snap_n[f];
    n = n < 0 ? 0 : (n > tcap ? tcap : n);
    // the start state is the same for every lane: one sincos pair per wave
    const double x0 = plan_state[(size_t)f * 4], y0 = plan_state[(size_t)f * 4 + 1], h = plan_state[(size_t)f * 4 + 2];
    double sn, cs, s2, c2;
    sincos(h, &sn, &cs);
    sincos(h + 1.5707963267948966, &s2, &c2);                       // heading + np.pi/2  (motion_planner.py:179)
    const av_track_row* rows = snap + (size_t)f * tcap;
    constexpr int OS = MOVING ? 5 : 3;
    const double v0 = MOVING ? plan_state[(size_t)f * 4 + 3] : 0.0;
    double* out = obstacles + (size_t)f * ocap * OS;
    int count = 0;                                                  // obstacles of the rows before this round
    int off = 0;                                                    // GROUND: rows dropped because their foot is not on the road
    const av_ground_cfg* cam = nullptr;
    const av_lens_cfg* lens = nullptr;
    if constexpr (GROUND) cam = via.table + f / via.cam_stride;
    if constexpr (LENS) lens = via.lens + f / via.cam_stride;
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        bool keep = false, off_road = false;
        double ox = 0.0, oy = 0.0, rad = 0.0, ovx = 0.0, ovy = 0.0;
        int cls = 0;
        if (i < n) {
            const av_track_row r = rows[i];
            cls = r.cls;
#pragma unroll
            for (int k = 0; k < 16; ++k) rad = r.cls == k ? cfg.radius[k] : rad;      // (ids outside 0..15 keep 0: no obstacle)
            keep = (r.flags & 1) && rad > 0.0;
            double cx, cy, fvx = 0.0, fvy = 0.0;
            if constexpr (MODE == FILTERED) {
                const double2* fr = reinterpret_cast<const double2*>(filt + ((size_t)f * tcap + i) * 6);
                const double2 c = fr[0], v = fr[1];
                cx = c.x, cy = c.y, fvx = v.x, fvy = v.y;
            } else {
                cx = (double)(r.x1 + r.x2) / 2.0, cy = (double)(r.y1 + r.y2) / 2.0;
            }
            double l, fw;
            grounddev::RoadPoint p;
            lensdev::Undistorted rect;
            if constexpr (GROUND) {
                // the foot point: anchor 1 = bottom centre (filtered: the filter's centre lowered by half the box height)
                double u = cx, v = cy;
                if (cam->anchor != 0) {
                    if constexpr (MODE == FILTERED) v = cy + (double)(r.y2 - r.y1) / 2.0;
                    else v = (double)r.y2;
                }
                if constexpr (LENS) {
                    // (u, v) is a raw pixel: the rectified one stands on the road, if the lens has it at all
                    rect = lensdev::undistort(lens, u, v);
                    u = rect.u, v = rect.v;
                }
                p = grounddev::project(cam->g, cam->max_range, u, v);
                if constexpr (LENS) p.on_road = p.on_road && rect.valid;
                l = p.l, fw = p.f;
                off_road = keep && !p.on_road;
                keep = keep && p.on_road;
            } else {
                l = (cx - cfg.x_center) * cfg.x_scale, fw = cfg.y_far - cy * cfg.y_scale;
            }
            ox = (x0 + fw * cs) + l * c2;
            oy = (y0 + fw * sn) + l * s2;
            if constexpr (MOVING) {
                const bool has_vel = r.hist_len >= 2;               // (vx, vy are valid from the second centre on)
                double rvx = MODE == FILTERED ? fvx : (has_vel ? (double)r.vx : 0.0);   // (a newborn's filtered velocity is 0)
                double rvy = MODE == FILTERED ? fvy : (has_vel ? (double)r.vy : 0.0);
                if constexpr (LENS) {
                    const lensdev::LensJac j = lensdev::jacobian(lens, rect);       // rectified px per raw px at the foot
                    const double qvx = j.juu * rvx + j.juv * rvy, qvy = j.jvu * rvx + j.jvv * rvy;
                    rvx = qvx, rvy = qvy;
                }
                double vl, vf;
                if constexpr (GROUND) {
                    const grounddev::RoadJac j = grounddev::jacobian(cam->g, p);     // metres per pixel at the foot
                    vl = (j.dlu * rvx + j.dlv * rvy) * frame_rate;
                    vf = v0 + (j.dfu * rvx + j.dfv * rvy) * frame_rate;
                } else {
                    vl = (rvx * cfg.x_scale) * frame_rate;                           // lateral, m/s, relative to the ego
                    vf = v0 - (rvy * cfg.y_scale) * frame_rate;                      // forward, m/s: the ego's own speed added
                }
                ovx = vf * cs + vl * c2;
                ovy = vf * sn + vl * s2;
            }
        }
        if constexpr (GROUND) off += __popcll(__ballot(off_road));
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const size_t at = (size_t)(count + __popcll(m & ((1ull << lane) - 1ull)));          // < n <= tcap <= ocap
            double* o = out + at * OS;
            o[0] = ox, o[1] = oy, o[2] = rad;
            if constexpr (MOVING) o[3] = ovx, o[4] = ovy;
            if constexpr (GROUND) {
                if (via.obs_cls) via.obs_cls[(size_t)f * ocap + at] = cls;
            }
        }
        count += __popcll(m);
    }
    if (lane == 0) n_obs[f] = count;
    if constexpr (GROUND) {
        if (lane == 0 && via.n_off) via.n_off[f] = off;
    }
}

}  // namespace

template <int MODE, typename VIA = Linear>
static int track_obstacles_launch(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, double frame_rate, int n_states, int tcap,
                                  const av_track_row* snap, const int32_t* snap_n, const double* plan_state, int ocap,
                                  double* obstacles, int32_t* n_obs, const double* filt, const char* who, VIA via = VIA()) {
    constexpr bool MOVING = MODE != STATIC;
    AV_REQUIRE(ctx && cfg && snap && snap_n && plan_state && obstacles && n_obs, AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE(MODE != FILTERED || filt, AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE(n_states > 0 && tcap > 0, AV_EINVAL, "%s: n_states and tcap must be > 0", who);
    AV_REQUIRE(ocap >= tcap, AV_EINVAL, "%s: ocap %d < tcap %d (no obstacle is ever dropped)", who, ocap, tcap);
    AV_REQUIRE(!MOVING || (frame_rate > 0.0 && std::isfinite(frame_rate)), AV_EINVAL, "%s: frame_rate must be > 0 and finite", who);
    hipLaunchKernelGGL((track_obstacles_kernel<MODE, VIA>), dim3((n_states + 3) / 4), dim3(256), 0, as_stream(stream), *cfg,
                       frame_rate, n_states, tcap, snap, snap_n, plan_state, ocap, obstacles, n_obs, filt, via);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_track_obstacles(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, int n_states, int tcap,
                                  const av_track_row* snap, const int32_t* snap_n, const double* plan_state, int ocap,
                                  double* obstacles, int32_t* n_obs) {
    return track_obstacles_launch<STATIC>(ctx, stream, cfg, 0.0, n_states, tcap, snap, snap_n, plan_state, ocap, obstacles, n_obs,
                                          nullptr, "av_track_obstacles");
}

extern "C" int av_track_obstacles_moving(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, double frame_rate, int n_states,
                                         int tcap, const av_track_row* snap, const int32_t* snap_n, const double* plan_state, int ocap,
                                         double* obstacles, int32_t* n_obs) {
    return track_obstacles_launch<MOVING_ROWS>(ctx, stream, cfg, frame_rate, n_states, tcap, snap, snap_n, plan_state, ocap, obstacles,
                                               n_obs, nullptr, "av_track_obstacles_moving");
}

extern "C" int av_track_obstacles_filtered(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, double frame_rate, int n_states,
                                           int tcap, const av_track_row* snap, const int32_t* snap_n, const double* filt,
                                           const double* plan_state, int ocap, double* obstacles, int32_t* n_obs) {
    return track_obstacles_launch<FILTERED>(ctx, stream, cfg, frame_rate, n_states, tcap, snap, snap_n, plan_state, ocap, obstacles, n_obs,
                                            filt, "av_track_obstacles_filtered");
}

// the three ground entries: lens NULL for rectified rows, obs_cls NULL for no class lane
static int track_obstacles_ground(const char* who, av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg,
                                  const av_ground_cfg* ground, const av_lens_cfg* lens, int cam_stride, int mode, double frame_rate,
                                  int n_states, int tcap, const av_track_row* snap, const int32_t* snap_n, const double* filt,
                                  const double* plan_state, int ocap, double* obstacles, int32_t* n_obs, int32_t* n_off,
                                  int32_t* obs_cls) {
    AV_REQUIRE(ground, AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE(cam_stride >= 1, AV_EINVAL, "%s: cam_stride must be >= 1", who);
    AV_REQUIRE(mode >= STATIC && mode <= FILTERED, AV_EINVAL, "%s: mode %d not in 0..2", who, mode);
    AV_REQUIRE((mode == FILTERED) == (filt != nullptr), AV_EINVAL, "%s: filt goes with mode 2 and with no other", who);
    auto launch = [&](auto via) {
        if (mode == FILTERED)
            return track_obstacles_launch<FILTERED>(ctx, stream, cfg, frame_rate, n_states, tcap, snap, snap_n, plan_state, ocap,
                                                    obstacles, n_obs, filt, who, via);
        if (mode == MOVING_ROWS)
            return track_obstacles_launch<MOVING_ROWS>(ctx, stream, cfg, frame_rate, n_states, tcap, snap, snap_n, plan_state, ocap,
                                                       obstacles, n_obs, nullptr, who, via);
        return track_obstacles_launch<STATIC>(ctx, stream, cfg, 0.0, n_states, tcap, snap, snap_n, plan_state, ocap, obstacles, n_obs,
                                              nullptr, who, via);
    };
    if (lens) return launch(GroundLens{ground, cam_stride, n_off, obs_cls, lens});
    return launch(Ground{ground, cam_stride, n_off, obs_cls});
}

extern "C" int av_track_obstacles_ground(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, const av_ground_cfg* ground,
                                         int cam_stride, int mode, double frame_rate, int n_states, int tcap, const av_track_row* snap,
                                         const int32_t* snap_n, const double* filt, const double* plan_state, int ocap,
                                         double* obstacles, int32_t* n_obs, int32_t* n_off) {
    return track_obstacles_ground("av_track_obstacles_ground", ctx, stream, cfg, ground, nullptr, cam_stride, mode, frame_rate, n_states,
                                  tcap, snap, snap_n, filt, plan_state, ocap, obstacles, n_obs, n_off, nullptr);
}

extern "C" int av_track_obstacles_ground_lens(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, const av_ground_cfg* ground,
                                              const av_lens_cfg* lens, int cam_stride, int mode, double frame_rate, int n_states,
                                              int tcap, const av_track_row* snap, const int32_t* snap_n, const double* filt,
                                              const double* plan_state, int ocap, double* obstacles, int32_t* n_obs, int32_t* n_off) {
    AV_REQUIRE(lens, AV_EINVAL, "av_track_obstacles_ground_lens: null argument");
    return track_obstacles_ground("av_track_obstacles_ground_lens", ctx, stream, cfg, ground, lens, cam_stride, mode, frame_rate,
                                  n_states, tcap, snap, snap_n, filt, plan_state, ocap, obstacles, n_obs, n_off, nullptr);
}

extern "C" int av_track_obstacles_ground_cls(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, const av_ground_cfg* ground,
                                             const av_lens_cfg* lens, int cam_stride, int mode, double frame_rate, int n_states,
                                             int tcap, const av_track_row* snap, const int32_t* snap_n, const double* filt,
                                             const double* plan_state, int ocap, double* obstacles, int32_t* n_obs, int32_t* n_off,
                                             int32_t* obs_cls) {
    return track_obstacles_ground("av_track_obstacles_ground_cls", ctx, stream, cfg, ground, lens, cam_stride, mode, frame_rate,
                                  n_states, tcap, snap, snap_n, filt, plan_state, ocap, obstacles, n_obs, n_off, obs_cls);
}
