/*
 * avhot.h -- C ABI of libavhot.so: the MI355X (gfx950) hot path of the
 * per-frame detect -> lane -> track -> Kalman -> plan loop.
 *
 * The reference (bhavyageethika/multimodal_autonomous_driving_perception_and_planning)
 * is pure Python and has no FFI; the drop-in boundary is its five classes
 * (SURVEY.md section 8b).  This header is what those classes' replacements
 * bind through ctypes; each entry point names the reference method it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions
 *   - Every function returns 0 (AV_OK) or a negative AV_E* code and never
 *     throws; av_last_error_string() describes the last failure on this thread.
 *   - All data pointers are DEVICE pointers unless the parameter is documented
 *     as host.  The caller owns every buffer; the library owns only av_ctx
 *     (constant tables, one side stream, captured graphs).  No allocation
 *     happens on the per-frame path.
 *   - `stream` is a hipStream_t passed as void*.  Calls are asynchronous and
 *     stream-ordered.  An av_ctx is bound to one device and is not thread-safe.
 *   - Batched layout: S independent video streams x W consecutive frames per
 *     call ("window").  Sequential state (track table, Kalman state, detector
 *     frame counter) lives in caller-owned device buffers and is advanced
 *     in place; S=1, W=1 is the reference's per-frame call.
 *   - Arithmetic that feeds a comparison is done in the reference's type and
 *     operation order (int32 boxes, float64 everywhere else, no FMA contraction).
 */
#ifndef AVHOT_H
#define AVHOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AV_VERSION 103

enum {
    AV_OK = 0,
    AV_EINVAL = -1,     /* bad argument (null pointer, capacity out of range, ...) */
    AV_EHIP = -2,       /* a HIP runtime call failed; see av_last_error_string()     */
    AV_ENODEV = -3,     /* no usable gfx950 device                                    */
    AV_ESTATE = -4,     /* call order violated (e.g. planner used before configure)   */
    AV_ENOMEM = -5
};

typedef struct av_ctx av_ctx;
typedef void* av_stream_t;          /* hipStream_t */

/* ---- context --------------------------------------------------------------------------------- */
int av_version(void);
const char* av_last_error_string(void);
int av_device_count(int* count);                      /* host out */
int av_ctx_create(int device, av_ctx** out);          /* fails with AV_ENODEV when no GPU is present */
int av_ctx_destroy(av_ctx* ctx);
int av_ctx_device(const av_ctx* ctx, int* device);

/* Side stream for fork/join of independent stages (tracker || Kalman->planner), also valid inside
 * a stream capture.  av_fork makes the side stream wait for everything enqueued on `main` so far;
 * av_join makes `main` wait for the side stream. */
int av_side_stream(av_ctx* ctx, av_stream_t* side);
int av_fork(av_ctx* ctx, av_stream_t main);
int av_join(av_ctx* ctx, av_stream_t main);

/* hipGraph capture of a sequence of av_* calls issued on `stream` (must not be the null stream). */
int av_graph_begin(av_ctx* ctx, av_stream_t stream);
int av_graph_end(av_ctx* ctx, av_stream_t stream, int* graph_id);
int av_graph_launch(av_ctx* ctx, int graph_id, av_stream_t stream);
int av_graph_destroy(av_ctx* ctx, int graph_id);

/* HIP events on arbitrary streams (bench.py times kernels on the stream they run on). */
int av_event_create(void** ev);
int av_event_destroy(void* ev);
int av_event_record(void* ev, av_stream_t stream);
int av_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on `stop` */
int av_stream_sync(av_stream_t stream);
int av_stream_sync_spin(av_stream_t stream);                   /* the same, polling (no interrupt wake-up latency) */

/* Pinned host staging buffers and stream-ordered copies for the per-frame class surfaces (one packed upload and
 * one packed download per detect() / update() / step() / plan() call; demo.py:107-120 calls them once per frame).
 * av_copy_d2h with sync != 0 also waits for the stream, i.e. for the results. */
int av_host_alloc(void** p, size_t bytes);
int av_host_free(void* p);
int av_copy_h2d(void* dst_dev, const void* src_host, size_t bytes, av_stream_t stream);
int av_copy_d2h(void* dst_host, const void* src_dev, size_t bytes, av_stream_t stream, int sync);

/* ---- D1: simulated detector -------------------------------------------------------------------
 * Replaces ObjectDetector.detect -> _detect_simulated (src/perception/detector.py:86-101,125-169).
 * Detections are a pure function of (frame_count, h, w): the reference reseeds NumPy's legacy
 * MT19937 with frame_count % 1000 per frame (:134).  The kernel re-derives that stream on device.
 * frame_count[s] is the detector's counter BEFORE the window; frames frame_count[s]+1 .. +W are
 * generated and frame_count[s] += W (detector.py:96).
 *   det_n   [S][W]            number of detections (3..7)
 *   det_box [S][W][dcap][4]   x1,y1,x2,y2 (int32)
 *   det_cls [S][W][dcap]      class id 0..7
 *   det_conf[S][W][dcap]      float64
 * dcap >= 7.  status[s] != 0 if the MT19937 draw budget (227 words) was exceeded (never observed). */
int av_simdet_generate(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, int h, int w,
                       int dcap, int32_t* frame_count, int32_t* det_n, int32_t* det_box,
                       int32_t* det_cls, double* det_conf, int32_t* status);

/* ---- K1-K3: IoU tracker -----------------------------------------------------------------------
 * Replaces MultiObjectTracker.update/_associate/_compute_iou
 * (src/tracking/multi_object_tracker.py:84-105,113-164,166-241). */
typedef struct {
    double iou_threshold;        /* 0.3  (:62) ; must be >= 0 */
    int32_t max_age;             /* 30   (:63) */
    int32_t min_hits;            /* 3    (:64) */
    int32_t trajectory_length;   /* 50   (:65) ; capacity of the per-track history ring */
} av_tracker_cfg;

/* One row of a track table, in dict-insertion (= ascending id) order.  64 bytes. */
typedef struct {
    int32_t id;
    int32_t x1, y1, x2, y2;      /* last matched bbox (:192) */
    int32_t cls;                 /* class at birth; never updated on match (:216-221) */
    int32_t age, hits, misses;
    int32_t slot;                /* index of this track's history ring in the stream's pool */
    int32_t hist_len;            /* centres appended so far (birth included); ring index = k % L */
    int32_t flags;               /* bit0: confirmed (hits >= min_hits) */
    double conf;
    float vx, vy;            /* last centre velocity (the Track.velocity property), valid when hist_len >= 2;
                                differences of half-integers, so exact in float32 */
} av_track_row;

/* Persistent per-stream tracker state (device).  Layout, for stream s with capacity tcap, L =
 * trajectory_length, all 16-byte aligned:
 *   int32 hdr[16]                  hdr[0]=n_tracks hdr[1]=next_id hdr[2]=frame_count hdr[3]=status
 *   av_track_row rows[tcap]
 *   double hist[tcap][L][4]        ring per slot: (cx, cy, vx, vy); entry k at k % L
 * trajectory  = entries max(0,hist_len-L) .. hist_len-1        (cx, cy)
 * velocities  = entries max(1,hist_len-L) .. hist_len-1        (vx, vy)
 * status bit0: table overflow (more than tcap live tracks; births were dropped, parity lost). */
size_t av_tracker_state_bytes(int tcap, int trajectory_length);
int av_tracker_reset(av_ctx* ctx, av_stream_t stream, int n_streams, int tcap, int trajectory_length,
                     void* state);
/* tcap in {64,128,...,1024}; dcap <= 64.
 *   snap    [S][W][tcap]   table after each frame (rows >= snap_n are unspecified); may be NULL
 *   snap_n  [S][W]         live rows after each frame; may be NULL iff snap is NULL
 *   det2trk [S][W][dcap]   id of the track detection j was matched to or born as (-1 beyond det_n)
 * Test hooks, read from the environment on every call (they choose the kernel; outputs stay bit-identical, which is what
 * tests/test_gpu_kernels.py and tests/test_gpu_more.py assert with them): AVHOT_TRACKER_REP=1 (tcap 64, dcap <= 8: the one-wave
 * kernel, not eight waves that split the association by detection column), AVHOT_TRACKER_PIPE=0 / 1 (the column waves without /
 * with the ninth wave that keeps the complete rows one frame behind them; unset: with it for windows of 16 frames or more).
 * The library reads no other variable for this stage. */
int av_tracker_update(av_ctx* ctx, av_stream_t stream, const av_tracker_cfg* cfg, int n_streams,
                      int n_frames, int dcap, const int32_t* det_n, const int32_t* det_box,
                      const int32_t* det_cls, const double* det_conf, int tcap, void* state,
                      av_track_row* snap, int32_t* snap_n, int32_t* det2trk);

/* Wire format of a track table for the all-gather of per-frame track tables across ranks (BASELINE config 5,
 * SURVEY.md section 8e; the reference has no multi-process code, F9).  What travels is what a consumer of
 * MultiObjectTracker.update()'s return value reads (multi_object_tracker.py:236-241): a 16-byte header and tcap
 * 32-byte rows, rows >= n_rows zero-filled.  Lossy against av_track_row only in `conf` (float32), `misses`
 * (saturates at 65535) and coordinates (int16: frames up to 32767 px); slot / hist_len stay local. */
#define AV_WIRE_HDR_BYTES 16
#define AV_WIRE_ROW_BYTES 32
typedef struct {
    int32_t n_rows, stream, frame, reserved;   /* global stream id; frame: see av_pack_tracks */
} av_wire_hdr;
typedef struct {
    int32_t id;
    int16_t x1, y1, x2, y2;
    int32_t age, hits;
    uint16_t misses;
    uint8_t cls, flags;          /* flags bit0: confirmed */
    float conf;
    int16_t vx2, vy2;            /* 2 x the last centre velocity (half-integers, so exact) */
} av_wire_row;
size_t av_wire_table_bytes(int tcap);          /* AV_WIRE_HDR_BYTES + tcap * AV_WIRE_ROW_BYTES */
/* Packs the tables of frames [frame_lo, frame_lo + n_sel) of every stream of a window into
 *   wire [n_streams][n_sel][av_wire_table_bytes(tcap)]
 * (n_sel = 1, frame_lo = n_frames - 1: the end-of-window table; n_sel = n_frames: every frame's table).
 * header.stream = stream0 + s (this rank's first global stream id).  header.frame = frame0 + the stream's DETECTOR FRAME COUNT
 * at that frame (ObjectDetector.frame_count after detect(), detector.py:96; 1 for a stream's first frame, plus whatever offset
 * the counter was reset to) when `frame_count` [n_streams] -- the detector's counters after the window's last frame, as
 * av_simdet_generate / av_hot_step leave them -- is given: the same value av_hot_step stamps.  frame_count NULL: frame0 + the
 * frame's index within the window.  The gather itself is torch.distributed's all_gather_into_tensor on `wire`
 * (RCCL over xGMI; distributed.TrackTableExchange). */
int av_pack_tracks(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, int tcap, int frame_lo, int n_sel,
                   int stream0, int frame0, const av_track_row* snap, const int32_t* snap_n, const int32_t* frame_count, void* wire);

/* The all-gather itself as a library call on an RCCL communicator (av_allgather_tracks(ctx, ncclComm_t, ...);
 * the reference has no counterpart).  `comm` is an ncclComm_t: the caller's own, or one made by av_comm_create from a
 * 128-byte ncclUniqueId that rank 0 obtained with av_comm_unique_id and handed to the other ranks by any means (the Python class
 * broadcasts it with torch.distributed).  librccl is opened with dlopen at the first of these calls: the library has no link-time
 * dependency on it, and a process that never gathers never loads it.
 *   send [bytes_per_rank] this rank's packed tables; recv [world * bytes_per_rank] every rank's, in rank order; stream-ordered. */
int av_comm_unique_id(void* id128);
int av_comm_create(av_ctx* ctx, const void* id128, int rank, int world, void** comm);
int av_comm_destroy(void* comm);
int av_allgather_tracks(av_ctx* ctx, void* comm, av_stream_t stream, const void* send, void* recv, size_t bytes_per_rank);

/* ---- E1-E3: vehicle state estimator ------------------------------------------------------------
 * Replaces VehicleStateEstimator.predict/update/step/_extract_state
 * (src/state_estimation/vehicle_state.py:68-198) incl. filterpy's predict/update equations. */
typedef struct {
    double dt;                   /* 0.033 (:49) */
    double process_noise;        /* 0.1   (:50) */
    double measurement_noise;    /* 1.0   (:51) */
} av_kf_cfg;

#define AV_KF_STATE_DOUBLES 48   /* x[6], P[36] row-major, prev_heading, prev_speed, time, 3 spare */
#define AV_VSTATE_DOUBLES 12     /* x y vx vy heading speed acceleration yaw_rate timestamp
                                    pos_uncertainty vel_uncertainty heading_uncertainty(=0) */
int av_kf_reset(av_ctx* ctx, av_stream_t stream, int n_streams, double* kf_state);
/* mode per (stream, frame): 0 = predict only (VehicleStateEstimator.predict)
 *                           1 = step(z)      (predict + update)
 *                           2 = step(None)   (predict + second extract)
 *                           3 = update(z) only
 * mode == NULL means 1 everywhere.
 *   z          [S][W][4]
 *   out_state  [S][W][12]
 *   plan_state [S][W][4]   (x, y, heading, speed) = the tuple demo.py:118-119 builds; may be NULL */
int av_kf_step(av_ctx* ctx, av_stream_t stream, const av_kf_cfg* cfg, int n_streams, int n_frames,
               const double* z, const uint8_t* mode, double* kf_state, double* out_state,
               double* plan_state);

/* ---- P1-P3: motion planner ---------------------------------------------------------------------
 * Replaces MotionPlanner.generate_polynomial_trajectory / evaluate_trajectory_cost / plan
 * (src/planning/motion_planner.py:126-204,206-262,264-303). */
typedef struct {
    double planning_horizon;     /* 5.0 (:69) */
    double dt;                   /* 0.1 (:70) */
    int32_t num_samples;         /* 7   (:71) lateral samples; candidates = 3 * num_samples */
    int32_t reserved;
    double w_lateral, w_velocity, w_acceleration, w_curvature;   /* 1.0 0.5 0.3 0.4 (:85-89) */
} av_planner_cfg;

#define AV_WP_DOUBLES 6          /* x y heading velocity timestamp curvature */
/* Builds the per-configuration constant tables (timestamps, 1-exp(-t), quintic blend, lateral
 * offsets) on the host and uploads them.  n_points = int(H/dt)+1 <= 256, candidates <= 192;
 * av_planner_plan plans every configuration this call accepts. */
int av_planner_configure(av_ctx* ctx, const av_planner_cfg* cfg);
int av_planner_dims(const av_ctx* ctx, int* n_points, int* n_candidates);   /* host out */
/* The launch av_planner_plan / _plan_each / _plan_moving make for n_states start states of a configuration with n_points
 * waypoints and n_candidates candidates; extra != 0: a reference path or obstacles are given (_plan_each / _plan_moving: a list
 * pointer is).  Needs neither a context nor a device: it is the library's own launch plan, asked without launching.
 *   out[0]  0: planner_kernel<G, NW> (a workgroup of NW waves plans G start states), 1: planner_wave_kernel (every wave on its own;
 *           with `extra` its form that reads the lists)
 *   out[1]  G; for the wave kernel the start states per wave        out[2]  NW, waves per workgroup
 *   out[3]  dynamic LDS bytes of a workgroup (<= 65 536)
 * AV_EINVAL outside what av_planner_configure accepts (n_points in [1,256], n_candidates = 3 * num_samples in [3,192]) and for
 * n_states <= 0. */
int av_planner_launch_shape(int n_points, int n_candidates, int n_states, int extra, int32_t out[4]);   /* host out */
/* One plan() per start state.  n_states = S*W.
 *   state     [n_states][4]          x, y, heading, speed
 *   ref_path  [n_ref][2] or NULL     shared by all states of this call (set_reference_path, :93-124)
 *   obstacles [n_obs][3] or NULL     (x, y, radius), shared by all states of this call
 *   waypoints [n_states][C][n][6]    GENERATION order (lateral outer, speed inner); may be NULL
 *   cost      [n_states][C]          generation order
 *   order     [n_states][C]          order[r] = generation index of the r-th cheapest (stable sort) */
int av_planner_plan(av_ctx* ctx, av_stream_t stream, int n_states, const double* state,
                    const double* ref_path, int n_ref, const double* obstacles, int n_obs,
                    double* waypoints, double* cost, int32_t* order);

/* av_planner_plan with per-state inputs: S x W start states are S x W independent MotionPlanners, each with its own
 * set_reference_path (:93-124) and its own plan(state, obstacles) argument (:264-303).  State f reads obstacle list f and
 * reference path f / ref_stride (ref_stride = W: one path per stream).
 *   ref_path  [n_paths][rcap][2], n_ref [n_paths], n_paths = ceil(n_states / ref_stride); both NULL = no paths;
 *             n_ref[p] < 2 = no path for that group (set_reference_path ignores shorter lists, :100-101); clamped to rcap
 *   obstacles [n_states][ocap][3], n_obs [n_states] clamped to 0..ocap; both NULL = no obstacles
 *   waypoints / cost / order as av_planner_plan.  Same kernels and dispatch as av_planner_plan: a state's results are those of
 *   av_planner_plan with its path and list shared, bit for bit. */
int av_planner_plan_each(av_ctx* ctx, av_stream_t stream, int n_states, const double* state,
                         const double* ref_path, const int32_t* n_ref, int rcap, int ref_stride,
                         const double* obstacles, const int32_t* n_obs, int ocap,
                         double* waypoints, double* cost, int32_t* order);

/* av_planner_plan_each around MOVING obstacles: rows of five doubles (x, y, radius, vx, vy), position and velocity in the
 * planner's frame (m, m/s).  For the waypoint with timestamp t (waypoint field 4, the configuration's table value) the disc is at
 *   px = x + vx * t,  py = y + vy * t           (float64, two roundings each: no FMA)
 * and the rest of the cost is av_planner_plan's unchanged: dist = sqrt((wx - px)^2 + (wy - py)^2), the < 2r and < 4r branches
 * (:253-259), per waypoint over the list in order.  vx = vy = 0 is av_planner_plan_each's term, bit for bit.
 *   obstacles [n_states][ocap][5], n_obs [n_states] clamped to 0..ocap; both NULL = no obstacles
 * Every other argument, the clamping, the NULL rules, the error codes and the dispatch are av_planner_plan_each's. */
int av_planner_plan_moving(av_ctx* ctx, av_stream_t stream, int n_states, const double* state,
                           const double* ref_path, const int32_t* n_ref, int rcap, int ref_stride,
                           const double* obstacles, const int32_t* n_obs, int ocap,
                           double* waypoints, double* cost, int32_t* order);

/* The tracker's tables as the planner's obstacles: every confirmed track (flags bit0) of a frame, in table order, at the place
 * the BEV panel draws it (av_bev_build; bev_renderer.py:207-208), carried into the planner's frame by the frame's start state
 * (x0, y0, h, .) the way a candidate is placed (motion_planner.py:175-180):
 *   cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;  l = (cx - x_center) * x_scale, f = y_far - cy * y_scale
 *   ox = (x0 + f cos h) + l cos(h + pi/2), oy = (y0 + f sin h) + l sin(h + pi/2), r = radius[cls]
 * so an obstacle at (f, l) lies where a candidate of lateral offset l is at arc length f. */
typedef struct {
    double x_center, x_scale;   /* 320.0, 0.03: lateral = (cx - x_center) * x_scale   (bev_renderer.py:208) */
    double y_far, y_scale;      /* 50.0, 0.1:   forward = y_far - cy * y_scale        (bev_renderer.py:207) */
    double radius[16];          /* per class id; <= 0, or an id outside 0..15: that track is no obstacle */
} av_obstacle_cfg;              /* 160 bytes */
/*   snap [n_states][tcap], snap_n [n_states] (av_tracker_update), plan_state [n_states][4] (av_kf_step)
 *   obstacles [n_states][ocap][3] (x, y, radius), n_obs [n_states]; ocap >= tcap (nothing is ever dropped);
 *   rows >= n_obs[f] are unspecified */
int av_track_obstacles(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, int n_states, int tcap,
                       const av_track_row* snap, const int32_t* snap_n, const double* plan_state,
                       int ocap, double* obstacles, int32_t* n_obs);
/* av_track_obstacles with the tracks' velocities, for av_planner_plan_moving: the same rows in the same order at the same place
 * with the same radius (columns 0..2 and n_obs are av_track_obstacles' output), and in columns 3..4 the constant velocity the
 * track's last centre difference predicts (Track.velocity, what predict_next_position uses, multi_object_tracker.py:35-47), in
 * the planner's frame.  With the frame's start state (x0, y0, h, v0) and frame_rate in frames per second (> 0, finite):
 *   rvx, rvy = row.vx, row.vy if row.hist_len >= 2, else 0, 0        (px per frame)
 *   vl = (rvx * x_scale) * frame_rate                                  lateral, m/s, relative to the ego
 *   vf = v0 - (rvy * y_scale) * frame_rate                             forward, m/s: the image is ego-centric, so the ego's
 *                                                                      own speed is added (a track at rest in it moves with the ego)
 *   vx = vf cos h + vl cos(h + pi/2), vy = vf sin h + vl sin(h + pi/2)
 *   obstacles [n_states][ocap][5] (x, y, radius, vx, vy); everything else as av_track_obstacles */
int av_track_obstacles_moving(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, double frame_rate, int n_states,
                              int tcap, const av_track_row* snap, const int32_t* snap_n, const double* plan_state,
                              int ocap, double* obstacles, int32_t* n_obs);

/* ---- Per-track Kalman filter over the snapshot tables (the SORT filter; the reference has none: Track.velocity is the last
 * centre difference, multi_object_tracker.py:35-47) -------------------------------------------------------------------------
 * A constant-velocity filter per track, fed the matched centres, predicting through misses.  State x = (cx, cy, vx, vy) in
 * pixels and pixels per frame, one frame as the time step:
 *   F = [[1,0,1,0],[0,1,0,1],[0,0,1,0],[0,0,0,1]],  Q = q_accel G G^T with G = [[1/2,0],[0,1/2],[1,0],[0,1]]
 *   (per axis [[q/4, q/2], [q/2, q]]),  H = [I2 0],  R = r_meas I2
 * One frame after the other per stream; for every live row i < clamp(snap_n, 0, tcap) of the frame, with
 * z = ((x1 + x2) / 2, (y1 + y2) / 2) and k = row.slot (unique among live rows, inside [0, tcap), stable for a track's life):
 *   birth   (state[k].id != row.id): x = (z, 0, 0), P = diag(p0_pos, p0_pos, p0_vel, p0_vel), state[k].id = row.id; no prediction
 *   else    x <- F x, P <- F P F^T + Q
 *   then    if row.misses == 0: the Kalman update with measurement z
 *   filt row = (x, sqrt(P00 + P11), sqrt(P22 + P33))        the two uncertainties VehicleState carries
 * Slots that no live row of a frame names keep their state.  A row whose slot lies outside [0, tcap) (a hand-made table) is
 * skipped: its filt row is zeros and status bit 0 is set; no index leaves the state buffer.  float64 throughout. */
typedef struct {
    double q_accel;   /* 1.0   white-noise acceleration, px^2 / frame^4; finite, >= 0 */
    double r_meas;    /* 4.0   measurement variance of a centre coordinate, px^2; finite, > 0 */
    double p0_pos;    /* 4.0   initial variance of cx, cy; finite, >= 0 */
    double p0_vel;    /* 100.0 initial variance of vx, vy; finite, >= 0 */
} av_track_filter_cfg;           /* 32 bytes */
/* Persistent per-stream filter state (device).  Layout, for stream s with capacity tcap, 16-byte aligned:
 *   int32 hdr[16]                  hdr[0]=status; the rest 0
 *   slot[tcap], 64 bytes each:     int32 id (-1: free), int32 reserved (0), double x[4] (cx, cy, vx, vy),
 *                                  double p[3] (P00 = P11, P02 = P13, P22 = P33)
 * x and y never mix and share F, Q, H, R and the initial variances, so P is two equal 2 x 2 blocks, one per axis, that depend
 * only on the track's hit / miss pattern; every other entry of P is 0.  The three numbers ARE the covariance.
 * status bit0: a row named a slot outside [0, tcap) and was skipped.
 * av_track_filter_reset sets every id to -1 and every other byte, the status word included, to 0. */
size_t av_track_filter_state_bytes(int tcap);          /* 0 for tcap <= 0 */
int av_track_filter_reset(av_ctx* ctx, av_stream_t stream, int n_streams, int tcap, void* state);
/*   snap [S][W][tcap], snap_n [S][W]   av_tracker_update's outputs
 *   filt [S][W][tcap][6]               (cx, cy, vx, vy, pos_sigma, vel_sigma) aligned with the snapshot rows; rows at index
 *                                      clamp(snap_n) and beyond are not written
 * tcap as av_tracker_update's; n_streams, n_frames >= 1; cfg inside the ranges above: AV_EINVAL otherwise, before any launch. */
int av_track_filter_update(av_ctx* ctx, av_stream_t stream, const av_track_filter_cfg* cfg, int n_streams, int n_frames, int tcap,
                           const av_track_row* snap, const int32_t* snap_n, void* state, double* filt);
/* av_track_obstacles_moving on the filtered tracks: row selection, order, count and radius are av_track_obstacles', position and
 * velocity av_track_obstacles_moving's formulas in its operation order, with
 *   cx, cy   = filt[f][i][0..1]     instead of the box centre
 *   rvx, rvy = filt[f][i][2..3]     instead of row.vx, row.vy; no hist_len test (a newborn's filtered velocity is 0)
 * so a coasting track's disc sits where the filter predicts it, not where it was last seen.
 *   filt [n_states][tcap][6] (av_track_filter_update); everything else as av_track_obstacles_moving */
int av_track_obstacles_filtered(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, double frame_rate, int n_states, int tcap,
                                const av_track_row* snap, const int32_t* snap_n, const double* filt, const double* plan_state,
                                int ocap, double* obstacles, int32_t* n_obs);

/* The YOLO-mode detector's output (av_yolo_forward: float32 boxes and confidences, the model's class ids, confidence-descending)
 * as the tracker's input (av_tracker_update), on the device; what ObjectDetector._detect_yolo does per box on the host
 * (detector.py:111-121: map(int, xyxy), float(conf), int(cls)), plus an optional class table.  Per frame f:
 *   n = clamp(src_n[f], 0, max_det); entries 0 .. n-1 are visited in order
 *   class_map given: entry i is kept when 0 <= src_cls[i] < n_map and class_map[src_cls[i]] >= 0; its class is class_map[src_cls[i]]
 *   class_map NULL:  every entry is kept with its raw class id
 *   the first dcap kept entries are written in order: det_n[f] = min(kept, dcap), dropped[f] = kept - det_n[f]
 *   det_box = the four coordinates truncated toward zero (int(x)); saturated to the int32 range, NaN -> 0
 *   det_conf = (double)src_conf
 *   rows at or past det_n[f] are not written
 *   src_n [F], src_box [F][max_det][4], src_conf [F][max_det], src_cls [F][max_det]; class_map [n_map] or NULL
 *   det_n [F], det_box [F][dcap][4], det_cls [F][dcap], det_conf [F][dcap]; dropped [F] or NULL
 * 1 <= dcap <= 64 (the tracker's limit), max_det >= 1, n_frames >= 1: AV_EINVAL otherwise. */
int av_dets_to_tracker(av_ctx* ctx, av_stream_t stream, int n_frames, int max_det, const int32_t* src_n,
                       const float* src_box, const float* src_conf, const int32_t* src_cls, const int32_t* class_map,
                       int n_map, int dcap, int32_t* det_n, int32_t* det_box, int32_t* det_cls, double* det_conf,
                       int32_t* dropped);

/* The lane detector's fits (av_lane_detect) as the planner's reference path, one per stream (av_planner_plan_each with
 * ref_stride = the window), and as the maneuver tagger's lane offset in metres (av_maneuver_detect).  cfg's four scale fields
 * are av_track_obstacles' (the radii are ignored), so tracks and lanes land in one road plane.  Stream s uses start state
 * s * ref_stride (x0, y0, h0, .), the first frame of its window.  Where info[s][0] and info[s][1] are both non-zero, for
 * i = 0 .. n_points - 1 (float64, every operation rounded on its own: no FMA):
 *   y  = (double)h - (double)i * ((0.4 * (double)h) / (double)(n_points - 1))     rows h .. 0.6 h, nearest first
 *                                                                                  (lane_detector.py:164)
 *   x_side = (c2 * y + c1) * y + c0 for side 0 (left) and 1 (right) of poly;  xc = (x_left + x_right) / 2
 *   l = (xc - x_center) * x_scale,  f = y_far - y * y_scale
 *   ref_path[s][i] = ((x0 + f cos h0) + l cos(h0 + pi/2), (y0 + f sin h0) + l sin(h0 + pi/2))
 *   n_ref[s] = n_points
 *   lane_offset[s] = ((double)w / 2 - (double)(pts[s][0][49][0] + pts[s][1][49][0]) / 2) * x_scale
 *                                                                  (get_lane_center_offset, lane_detector.py:253-272, in metres)
 * otherwise n_ref[s] = 0, lane_offset[s] = NaN and no path row is written.  Rows at or past n_ref[s] are never written.
 *   poly [S][2][3], pts [S][2][50][2], info [S][8] (av_lane_detect); plan_state [S * ref_stride][4] (av_kf_step)
 *   ref_path [S][rcap][2], n_ref [S]; lane_offset [S] or NULL
 * 2 <= n_points <= rcap and n_points <= 64 (one wave per stream); n_streams, h, w, ref_stride >= 1: AV_EINVAL otherwise. */
int av_lane_paths(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, int n_streams, int h, int w, int n_points,
                  const double* poly, const int32_t* pts, const int32_t* info, const double* plan_state, int ref_stride,
                  int rcap, double* ref_path, int32_t* n_ref, double* lane_offset);

/* ---- The camera model: a ground-plane homography per camera (opt-in; the reference has no camera, and av_obstacle_cfg's four
 * numbers are the BEV panel's drawing convention) ----------------------------------------------------------------------------
 * A flat road seen by a pinhole camera is a plane-to-plane projection: image (u, v, 1) -> g (u, v, 1)^T = (F, L, D),
 * forward = F / D, lateral = L / D in metres.  (u, v) is a RECTIFIED pixel; for raw frames see av_lens_cfg below.
 * Projection of an image point (float64, every operation rounded on its own: no FMA):
 *   F = (g0*u + g1*v) + g2;  L = (g3*u + g4*v) + g5;  D = (g6*u + g7*v) + g8
 *   f = F / D;  l = L / D
 *   on_road = D > 0 && f >= 0 && f <= max_range        (a NaN fails)
 *   dfu = (g0 - f*g6) / D;  dfv = (g1 - f*g7) / D;  dlu = (g3 - l*g6) / D;  dlv = (g4 - l*g7) / D      (the Jacobian, m / px) */
typedef struct {
    double g[9];       /* row-major; image (u, v, 1) -> (F, L, D): forward = F / D, lateral = L / D, metres, lateral > 0 towards image right */
    double ginv[9];    /* the inverse: road (f, l, 1) -> (U, V, D'): u = U / D', v = V / D' */
    double max_range;  /* metres, > 0, finite */
    int32_t anchor;    /* 0: box centre ((x1+x2)/2, (y1+y2)/2); 1: bottom centre ((x1+x2)/2, y2) -- the default */
    int32_t reserved;  /* 0 */
} av_ground_cfg;       /* 160 bytes */
/* Fills *out from g: ginv = adj(g) / det(g), the TRUE inverse (D' = 1 / D), so one sign convention holds in both directions:
 * D > 0 = below the horizon and in front of the camera.  AV_EINVAL, *out untouched: an entry of g not finite; det == 0 or an
 * entry of ginv not finite; max_range not > 0 and finite; anchor not 0 or 1.  Host only: no context, no GPU. */
int av_ground_make(const double g[9], double max_range, int anchor, av_ground_cfg* out);

/* av_track_obstacles / _moving / _filtered (mode 0 / 1 / 2) through a camera.  ground is a DEVICE table; state f uses entry
 * f / cam_stride (ref_stride's convention).  cfg gives radius[] only.  Row selection, order, compaction and radius are
 * av_track_obstacles'; in addition the row's foot point (u, v) must be on_road:
 *   anchor 0: (cx, cy);  anchor 1: (cx, (double)y2), in mode 2 (filt cx, filt cy + (double)(y2 - y1) / 2.0)
 *   with (cx, cy) the box centre (modes 0, 1) or filt[f][i][0..1] (mode 2)
 * A confirmed row of a class with positive radius whose foot is not on_road is counted in n_off[f] and not written.
 *   position: ox = (x0 + f cos h) + l cos(h + pi/2), oy likewise, with (f, l) the foot's projection
 *   velocity (modes 1, 2; rvx, rvy as av_track_obstacles_moving / _filtered take them):
 *     vl = (dlu*rvx + dlv*rvy) * frame_rate;  vf = v0 + (dfu*rvx + dfv*rvy) * frame_rate;  then the rotation by h as there
 *   obstacles [n_states][ocap][3] (mode 0) or [5]; n_off [n_states] or NULL; filt non-NULL exactly in mode 2
 * cam_stride >= 1, mode in 0..2, and the checks of the linear forms: AV_EINVAL otherwise, before any launch. */
int av_track_obstacles_ground(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, const av_ground_cfg* ground,
                              int cam_stride, int mode, double frame_rate, int n_states, int tcap, const av_track_row* snap,
                              const int32_t* snap_n, const double* filt, const double* plan_state, int ocap, double* obstacles,
                              int32_t* n_obs, int32_t* n_off);

/* av_lane_paths through a camera: ground is a DEVICE table, stream s uses ground[s].  Rows y_i and centre abscissa xc_i as in
 * av_lane_paths; (f_i, l_i) = the projection of (xc_i, y_i); the path is the longest prefix i = 0 .. m-1 whose points are all
 * on_road: n_ref[s] = m if m >= 2, else 0 (the planner takes fewer than two points as no path); rows at or past n_ref[s] are
 * not written.
 *   lane_offset[s] = l((double)w / 2, (double)h) - l(xm, (double)h),  xm = (double)(pts[s][0][49][0] + pts[s][1][49][0]) / 2
 *   NaN if either point is not on_road or the lane pair is missing (info[s][0] or info[s][1] zero; then n_ref[s] = 0 too).
 * Every other argument and check as av_lane_paths. */
int av_lane_paths_ground(av_ctx* ctx, av_stream_t stream, const av_ground_cfg* ground, int n_streams, int h, int w, int n_points,
                         const double* poly, const int32_t* pts, const int32_t* info, const double* plan_state, int ref_stride,
                         int rcap, double* ref_path, int32_t* n_ref, double* lane_offset);

/* The bird's-eye view of the frames: panel pixel (r, c) of camera k shows the road point
 *   f = f_far - ((double)r + 0.5) * m_per_px;   l = (((double)c + 0.5) - (double)gw / 2.0) * m_per_px
 * seen through ground[k].ginv = q (float64, no FMA):
 *   U = (q0*f + q1*l) + q2;  V = (q3*f + q4*l) + q5;  D = (q6*f + q7*l) + q8;   !(D > 0): fill
 *   u = U / D; v = V / D;   tu = floor(u * 65536.0 + 0.5), tv = floor(v * 65536.0 + 0.5)   (doubles)
 *   !(0 <= tu <= (w-1) * 65536 && 0 <= tv <= (h-1) * 65536): fill
 *   x0 = tu >> 16, wx = tu & 65535, x1 = min(x0 + 1, w - 1); y likewise; each channel by the bilinear rule of the side-by-side
 *   view's resize: ((p00 (65536-wx) + p01 wx) (65536-wy) + (p10 (65536-wx) + p11 wx) wy + 2^31) >> 32
 *   ground DEVICE [n_cams], bgr [n_cams][h][w][3], fill: three HOST bytes (b, g, r), out [n_cams][gh][gw][3]
 * n_cams, h, w, gh, gw >= 1 (any width: no multiple-of-four rule); m_per_px > 0 and finite, f_far finite; n_cams and
 * ceil(gh / 16) <= 65535: AV_EINVAL otherwise. */
int av_ground_warp(av_ctx* ctx, av_stream_t stream, const av_ground_cfg* ground, int n_cams, int h, int w, const uint8_t* bgr,
                   int gh, int gw, double f_far, double m_per_px, const uint8_t fill[3], uint8_t* out);

/* ---- Lens distortion (opt-in): OpenCV's five-coefficient Brown-Conrady model in front of the ground-plane homography ---------
 * A raw pixel (u, v) has normalised coordinates (xd, yd) = ((u - cx) / fx, (v - cy) / fy); the undistorted point (x, y) is shown
 * at the rectified pixel (nfx*x + ncx, nfy*y + ncy).  Pixel c sits at u = c, as av_ground_warp indexes.  float64, every operation
 * rounded on its own (no FMA), in exactly this order:
 *   r2   = x*x + y*y
 *   rad  = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *   xd   = x*rad + (2*p1*x*y + p2*(r2 + 2*x*x))          2*p1*x*y = ((2*p1)*x)*y, 2*x*x = (2*x)*x, and so on, left to right
 *   yd   = y*rad + (p1*(r2 + 2*y*y) + 2*p2*x*y)
 *   drad = k1 + r2*(2*k2 + r2*(3*k3))                    d rad / d r2
 *   a = rad + 2*x*x*drad + (2*p1*y + 6*p2*x)             d xd / dx      (a = (rad + ((2*x)*x)*drad) + (..))
 *   b = 2*x*y*drad + (2*p1*x + 2*p2*y)                   d xd / dy = d yd / dx
 *   d = rad + 2*y*y*drad + (6*p1*y + 2*p2*x)             d yd / dy
 * Undistorting a raw pixel: Newton's method from (x, y) = (xd, yd), exactly six iterations of
 *   ex = xd(x, y) - xd;  ey = yd(x, y) - yd;  det = a*d - b*b
 *   x' = x - (d*ex - b*ey) / det;  y' = y - (a*ey - b*ex) / det
 * then the model once more at the result: valid = det > 0 at all seven points && ex*ex + ey*ey <= 1e-20   (a NaN fails).
 * The Jacobian raw pixel -> rectified pixel at the result is the inverse of [[a, b], [b, d]], scaled:
 *   juu = (d / det) * (nfx / fx);  juv = (-b / det) * (nfx / fy);  jvu = (-b / det) * (nfy / fx);  jvv = (a / det) * (nfy / fy) */
typedef struct {
    double fx, fy, cx, cy;          /* the raw frame's intrinsics */
    double k1, k2, p1, p2, k3;      /* OpenCV's order */
    double nfx, nfy, ncx, ncy;      /* the rectified picture's intrinsics */
    int32_t w, h;                   /* frame size, raw and rectified */
} av_lens_cfg;                      /* 112 bytes */
/* Fills *out.  K = (fx, fy, cx, cy); dist = (k1, k2, p1, p2, k3); new_K = the rectified picture's four, or NULL for K.
 * AV_EINVAL, *out untouched: an entry not finite; a focal length not > 0; w or h not in 1 .. 32768; a model that folds over inside
 * the rectified frame: q = 1 + r2*(3*k1 + r2*(5*k2 + r2*(7*k3))) <= 0 (the radial map's derivative) at r = rmax * i / 1024 for any
 * i = 1 .. 1024, rmax the largest normalised radius of the rectified frame's four corner pixels.  Host only: no context, no GPU. */
int av_lens_make(const double K[4], const double dist[5], const double new_K[4], int w, int h, av_lens_cfg* out);

/* The table that rectifies a frame (cold path, once per lens): map int32 [n_maps][h][w][2], lens DEVICE [n_maps].  Rectified
 * pixel (r, c) of map k, through lens[k]:
 *   x = ((double)c - ncx) / nfx;  y = ((double)r - ncy) / nfy;  (xd, yd) as above;  u = fx*xd + cx;  v = fy*yd + cy
 *   tu = floor(u * 65536.0 + 0.5);  tv likewise
 *   entry = (tu, tv) if 0 <= tu <= (w-1) * 65536 && 0 <= tv <= (h-1) * 65536, else (-1, -1)
 * A table entry whose own w, h are not the arguments' gives a map of (-1, -1) throughout.
 * n_maps >= 1, 1 <= h, w <= 32768, n_maps and ceil(h / 16) <= 65535: AV_EINVAL otherwise. */
int av_lens_map_rectify(av_ctx* ctx, av_stream_t stream, const av_lens_cfg* lens, int n_maps, int h, int w, int32_t* map);

/* The table of the bird's-eye view taken straight from RAW frames (cold path): map [n_maps][gh][gw][2].  Panel pixel (r, c) of
 * map k: the road point and ground[k].ginv exactly as av_ground_warp, !(D > 0): (-1, -1); the rectified (u, v) = (U / D, V / D);
 * then x = (u - ncx) / nfx, y = (v - ncy) / nfy through lens[k] to the raw frame as av_lens_map_rectify, within lens[k]'s w, h.
 * gh, gw >= 1, m_per_px > 0 and finite, f_far finite, n_maps and ceil(gh / 16) <= 65535: AV_EINVAL otherwise. */
int av_lens_map_ground(av_ctx* ctx, av_stream_t stream, const av_lens_cfg* lens, const av_ground_cfg* ground, int n_maps, int gh,
                       int gw, double f_far, double m_per_px, int32_t* map);

/* The hot path: out pixel (r, c) of camera k is the source picture at map[k / cam_stride][r][c] = (tu, tv), 1/65536 pixels:
 *   x0 = tu >> 16, wx = tu & 65535, x1 = min(x0 + 1, sw - 1); y likewise; each channel by av_ground_warp's bilinear rule
 *   an entry outside [0, (sw-1) * 65536] x [0, (sh-1) * 65536] (a builder's (-1, -1), or anything else): fill
 *   map DEVICE [ceil(n_cams / cam_stride)][dh][dw][2], bgr [n_cams][sh][sw][3], fill: three HOST bytes, out [n_cams][dh][dw][3]
 * Integer arithmetic only.  n_cams, dh, dw >= 1 (any width), 1 <= sh, sw <= 32768, cam_stride >= 1, n_cams and ceil(dh / 16)
 * <= 65535, out overlapping neither bgr nor map: AV_EINVAL otherwise, before any launch. */
int av_remap(av_ctx* ctx, av_stream_t stream, const int32_t* map, int n_cams, int cam_stride, int sh, int sw, const uint8_t* bgr,
             int dh, int dw, const uint8_t fill[3], uint8_t* out);

/* av_track_obstacles_ground for tracks given in RAW pixels: lens is a DEVICE table beside ground, under the same cam_stride.
 * The foot point (u, v) of av_track_obstacles_ground is undistorted as above and the rectified pixel is projected; a foot that is
 * not valid counts as not on_road (n_off).  The pixel velocity goes through the undistortion's Jacobian first,
 *   qvx = juu*rvx + juv*rvy;  qvy = jvu*rvx + jvv*rvy
 * and (qvx, qvy) through the ground Jacobian at the rectified foot.  Everything else, and every check, as there. */
int av_track_obstacles_ground_lens(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, const av_ground_cfg* ground,
                                   const av_lens_cfg* lens, int cam_stride, int mode, double frame_rate, int n_states, int tcap,
                                   const av_track_row* snap, const int32_t* snap_n, const double* filt, const double* plan_state,
                                   int ocap, double* obstacles, int32_t* n_obs, int32_t* n_off);
/* av_track_obstacles_ground (lens NULL) or av_track_obstacles_ground_lens (lens given) with a class lane: the same kernel, which
 * writes beside every obstacle row o of state f the class of the tracker row behind it, obs_cls[f][o] = row.cls, whatever its
 * value.  obs_cls int32 [n_states][ocap] or NULL (then exactly the call without it); entries at or past n_obs[f] are not written.
 * Every other argument, output and check as there. */
int av_track_obstacles_ground_cls(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, const av_ground_cfg* ground,
                                  const av_lens_cfg* lens, int cam_stride, int mode, double frame_rate, int n_states, int tcap,
                                  const av_track_row* snap, const int32_t* snap_n, const double* filt, const double* plan_state,
                                  int ocap, double* obstacles, int32_t* n_obs, int32_t* n_off, int32_t* obs_cls);

/* ---- Camera rigs (opt-in): K cameras per vehicle, their obstacle lists fused on the road ------------------------------------------
 * A mount places a camera's road frame (x forward, y lateral from the camera's ground point) in the vehicle's: a rotation by the
 * mount's yaw (from the vehicle's forward axis towards +lateral) and a shift.  The table holds cos and sin, not the angle, so a
 * quarter turn can be written exactly. */
typedef struct {
    double c, s;           /* cos(yaw), sin(yaw) */
    double x, y;           /* the camera's ground point in the vehicle frame, metres */
} av_rig_mount;            /* 32 bytes */
typedef struct {
    double merge_scale;    /* 1.0: the gate in units of the larger of the two radii */
    double merge_min;      /* 1.0: the smallest gate, metres */
} av_rig_cfg;              /* 16 bytes; both finite and >= 0 */
/* The obstacle lists of every vehicle's K cameras -> one list per vehicle, in the planner's frame, objects seen by several cameras
 * merged.  cam_obs holds each camera's obstacles in that camera's own road frame, columns (x, y, r) or (x, y, r, vx, vy) with the
 * velocity relative to the vehicle: what av_track_obstacles_ground / _ground_lens write when their plan_state rows are
 * (0, 0, 0, 0).  Camera k of vehicle v is list v * n_cams + k.  float64, every operation rounded on its own (no FMA), in the
 * order written.  Per vehicle, cameras in the order k = 0 .. n_cams - 1 (a round), clusters kept in creation order:
 *   candidates of camera k: rows 0 .. clamp(cam_n, 0, ocap_in) - 1 in order; a row with x, y or r not finite, r <= 0 or (ncol 5)
 *     vx or vy not finite is skipped and counted in n_skip[v].  For a kept row, with the mount (c, s, mx, my):
 *       m = max(x*x + y*y, 1.0);  w = 1.0 / (m*m)          (a pixel's footprint grows with the squared distance from the camera,
 *                                                            so the variance of a ground position with its fourth power)
 *       X = (mx + c*x) - s*y;  Y = (my + s*x) + c*y;  VX = c*vx - s*vy;  VY = s*vx + c*vy
 *   association, against the clusters that existed when the round began (two rows of one camera never merge): for cluster i and
 *     candidate j
 *       dx = X_i - X_j;  dy = Y_i - Y_j;  d2 = dx*dx + dy*dy;  gate = max(merge_min, merge_scale * max(r_i, r_j))
 *     the pair is admissible when d2 <= gate*gate (and d2 is finite).  Repeatedly the admissible pair with the smallest d2 among
 *     the clusters and candidates not yet taken in this round is taken -- equal d2: the smallest i, then the smallest j -- until
 *     none remains (multi_object_tracker.py:136-159, with the distance in place of the IoU).
 *   absorption: sw += w; sx += w*X; sy += w*Y; svx += w*VX; svy += w*VY; r = max(r, r_j); views |= 1 << k; then
 *     X = sx / sw, and Y, VX, VY likewise: the next round measures from the fused position.
 *   new clusters: the candidates left over, in candidate order, behind the existing ones: sw = w, sx = w*X, ..., views = 1 << k;
 *     a cluster with one member stands at that member's X, Y, VX, VY themselves.
 *   output, cluster i = row i, placed as av_track_obstacles places a track, (x0, y0, h, v0) = plan_state[v]:
 *       ox = (x0 + X cos h) + Y cos(h + pi/2);  oy = (y0 + X sin h) + Y sin(h + pi/2);  r
 *       VF = VX + v0;  vx = VF cos h + VY cos(h + pi/2);  vy = VF sin h + VY sin(h + pi/2)                       (ncol 5)
 *     n_obs[v] = the number of clusters, views[v][i] = the mask of the cameras that saw cluster i; rows at or past n_obs[v] are
 *     not written.
 *   mounts DEVICE [V][K]; cam_obs [V*K][ocap_in][ncol], cam_n [V*K]; plan_state [V][4] (av_kf_step's)
 *   obstacles [V][ocap][ncol], n_obs [V]; views [V][ocap] or NULL; n_skip [V] or NULL
 * AV_EINVAL before any launch: a null pointer other than views and n_skip; n_vehicles < 1; n_cams not in 1..8; ocap_in not in
 * 1..64; ncol not 3 or 5; ocap < n_cams * ocap_in (nothing is ever dropped); cfg outside its ranges. */
int av_rig_fuse(av_ctx* ctx, av_stream_t stream, const av_rig_cfg* cfg, int n_vehicles, int n_cams, const av_rig_mount* mounts,
                int ncol, int ocap_in, const double* cam_obs, const int32_t* cam_n, const double* plan_state, int ocap,
                double* obstacles, int32_t* n_obs, int32_t* views, int32_t* n_skip);
/* av_rig_fuse with a class lane: cam_cls int32 [V*K][ocap_in] beside cam_obs (av_track_obstacles_ground_cls's obs_cls), cls int32
 * [V][ocap] beside obstacles, given together or both NULL (then exactly av_rig_fuse).  The association does not look at the classes:
 * obstacles, n_obs, views and n_skip are av_rig_fuse's bit for bit.  A cluster carries (best_w, cls): a new cluster takes its
 * member's w and class; an absorbed candidate with w > best_w (strictly) replaces both -- the class comes from the camera that sees
 * the object nearest, from the earlier camera among equals.  Class values travel as they are, negatives included; cls[v][i] is
 * cluster i's, entries at or past n_obs[v] are not written. */
int av_rig_fuse_cls(av_ctx* ctx, av_stream_t stream, const av_rig_cfg* cfg, int n_vehicles, int n_cams, const av_rig_mount* mounts,
                    int ncol, int ocap_in, const double* cam_obs, const int32_t* cam_n, const int32_t* cam_cls,
                    const double* plan_state, int ocap, double* obstacles, int32_t* n_obs, int32_t* views, int32_t* n_skip,
                    int32_t* cls);

/* ---- Vehicle-frame tracks (opt-in): av_rig_fuse's lists followed over time -------------------------------------------------------
 * A multi-object tracker in the planner's frame, one frame per call, with a state of its own per vehicle and a constant-velocity
 * Kalman filter per track: a fused obstacle keeps its id from frame to frame and from camera to camera, and a track that no row
 * matches coasts at its predicted place until max_age misses have passed.  The planner's frame is the ego filter's world frame:
 * the ego's own motion is already out of the positions (and, with five columns, out of the velocities), so constant velocity is
 * the right model there.  The greedy association is the reference tracker's (multi_object_tracker.py:136-159) with av_rig_fuse's
 * distance and gate in place of the IoU; max_age and min_hits are that tracker's.  float64, every operation rounded on its own (no
 * FMA), in the order written. */
typedef struct {
    double dt;            /* 1/30   seconds per frame; finite, > 0 */
    double q_accel;       /* 4.0    white-noise acceleration, m^2 / s^4; finite, >= 0 */
    double r_meas;        /* 0.25   measurement variance of a coordinate, m^2; finite, > 0 */
    double r_range;       /* 1e-6   the range term of the measurement variance (below); finite, >= 0; 0: the plain SORT filter */
    double p0_pos;        /* 1.0    initial variance of x, y; finite, >= 0 */
    double p0_vel;        /* 25.0   initial variance of vx, vy; finite, >= 0 */
    double gate_scale;    /* 2.0    the gate in units of the larger of the two radii; finite, >= 0 */
    double gate_min;      /* 2.0    the smallest gate, metres; finite, >= 0 */
    int32_t max_age;      /* 30     a track with more consecutive misses than this is freed; >= 0 */
    int32_t min_hits;     /* 3      a track is confirmed (written to the output) from this many hits on; >= 1 */
} av_rig_track_cfg;       /* 72 bytes */
/* Persistent per-vehicle state (device).  Layout, for vehicle v with capacity tcap (1 .. 512), 16-byte aligned:
 *   int32 hdr[16]                  hdr[0] = status, hdr[1] = the next id (1 after a reset), hdr[2] = frames seen,
 *                                  hdr[3] = live tracks; the rest 0
 *   slot[tcap], 96 bytes each:     int32 id (-1: free), hits, misses, age, views, views_ever, reserved[2] (0; the first is
 *                                  av_rig_track_cls's class word, class id + 1, which av_rig_track carries unchanged);
 *                                  double x[4] (x, y, vx, vy); double p[3] (P_pos, P_pos,vel, P_vel); double r (the radius)
 * x and y never mix and share F, Q, R and the initial variances, so the covariance is two equal 2 x 2 blocks, one per axis, as in
 * av_track_filter_update.  status bit0: a row found no free slot and was dropped (sticky until the next reset).
 * av_rig_track_reset sets every id to -1, hdr[1] to 1 and every other byte to 0. */
size_t av_rig_track_state_bytes(int tcap);             /* 64 + 96 * tcap; 0 for tcap outside 1 .. 512 */
int av_rig_track_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int tcap, void* state);
/* One frame per vehicle, (x0, y0, ., .) = plan_state[v], (a, b, c) = p, in this order:
 *   1 predict, every live slot:   x = x + vx*dt;  y = y + vy*dt;  age += 1
 *       bc = b + dt*c;  a' = ((a + dt*b) + dt*bc) + q11;  b' = bc + q12;  c' = c + q22            (P <- F P F^T + Q)
 *       q11 = q_accel * (((dt*dt)*(dt*dt)) / 4.0);  q12 = q_accel * (((dt*dt)*dt) / 2.0);  q22 = q_accel * (dt*dt)
 *   2 candidates: rows 0 .. clamp(n_in[v], 0, ocap_in) - 1 of obs_in[v]; a row with x, y or r not finite, r <= 0 or (ncol 5) vx
 *       or vy not finite is skipped: counted in n_skip[v], match = -1.
 *   3 association, live slot i (predicted) against candidate row j, stated as av_rig_fuse states it:
 *       dx = x_i - x_j;  dy = y_i - y_j;  d2 = dx*dx + dy*dy;  gate = max(gate_min, gate_scale * max(r_i, r_j))
 *     the pair is admissible when d2 <= gate*gate (and d2 is finite).  Repeatedly the admissible pair with the smallest d2 among
 *     the slots and rows not yet taken is taken -- equal d2: the smallest slot, then the smallest row -- until none remains.
 *   4 update of a matched slot with its row (zx, zy, r_j, views_j; views_j = 0 without views_in):
 *       ex = zx - x0;  ey = zy - y0;  m = max(ex*ex + ey*ey, 1.0);  R = r_meas + r_range * (m*m)   (av_rig_fuse's fourth power
 *                                                                                                   of the range from the vehicle)
 *       S = a + R;  k0 = a / S;  k1 = b / S
 *       per axis: y = z - x;  x = x + k0*y;  v = v + k1*y
 *       a' = a - k0*a;  b' = b - k0*b;  c' = c - k1*b
 *       r = r_j;  hits += 1;  misses = 0;  views = views_j;  views_ever |= views_j;  match[j] = id
 *   5 live slots left unmatched: misses += 1; views = 0; with misses > max_age the slot is freed (id = -1, everything else 0).
 *   6 births: the kept rows left unmatched, in row order, into the free slots in ascending order (those freed in step 5 among
 *       them): id = hdr[1]++;  x = (zx, zy, vx_j, vy_j) (velocities 0 with ncol 3);  p = (p0_pos, 0, p0_vel);  r = r_j;  hits = 1;
 *       misses = 0;  age = 0;  views = views_ever = views_j;  match[j] = id.  Without a free slot the row is dropped:
 *       match[j] = -2, counted in n_drop[v], status bit0 set.
 *   7 output: every live slot with hits >= min_hits, in slot order, compacted: (x, y, r) or (x, y, r, vx, vy) into obstacles[v],
 *       its slot into obs_slot[v]; n_obs[v] = their number.  A coasting slot is written at its predicted place.
 *   then hdr[2] += 1 and hdr[3] = the live slots.
 *   obs_in [V][ocap_in][ncol], n_in [V], views_in [V][ocap_in] or NULL (av_rig_fuse's obstacles, n_obs, views); plan_state [V][4]
 *   state  [V] x av_rig_track_state_bytes(tcap)
 *   obstacles [V][ocap_out][ncol], n_obs [V]; obs_slot [V][ocap_out], match [V][ocap_in], n_skip [V], n_drop [V]: each or NULL
 *   Rows of obstacles and obs_slot at or past n_obs[v], and entries of match at or past clamp(n_in[v]), are not written.
 * AV_EINVAL before any launch and before the context is looked at: n_vehicles < 1; tcap or ocap_in not in 1..512; ncol not 3 or 5;
 * ocap_out < tcap; cfg outside its ranges; a null pointer other than views_in, obs_slot, match, n_skip, n_drop and stream. */
int av_rig_track(av_ctx* ctx, av_stream_t stream, const av_rig_track_cfg* cfg, int n_vehicles, int tcap, int ncol, int ocap_in,
                 const double* obs_in, const int32_t* n_in, const int32_t* views_in, const double* plan_state, void* state,
                 int ocap_out, double* obstacles, int32_t* n_obs, int32_t* obs_slot, int32_t* match, int32_t* n_skip,
                 int32_t* n_drop);
/* av_rig_track with a class lane: cls_in int32 [V][ocap_in] beside obs_in (av_rig_fuse_cls's cls), cls_out int32 [V][ocap_out]
 * beside obstacles, each or NULL; with both NULL exactly av_rig_track.  The slot's first reserved word holds cls1 = class id + 1,
 * 0: no class known.  With cls_in given: a matched slot (step 4) or a birth (step 6) whose row has class c >= 0 sets cls1 = c + 1
 * (the latest observation wins); a row with c < 0 leaves a matched slot's word alone and gives a newborn 0.  A slot freed in step 5
 * gets 0 like its other words.  With cls_in NULL the word is carried unchanged.  Step 7 writes cls_out[v][o] = cls1 - 1 beside
 * output row o (-1: no class known).  The association does not look at the classes. */
int av_rig_track_cls(av_ctx* ctx, av_stream_t stream, const av_rig_track_cfg* cfg, int n_vehicles, int tcap, int ncol, int ocap_in,
                     const double* obs_in, const int32_t* n_in, const int32_t* views_in, const int32_t* cls_in,
                     const double* plan_state, void* state, int ocap_out, double* obstacles, int32_t* n_obs, int32_t* obs_slot,
                     int32_t* match, int32_t* n_skip, int32_t* n_drop, int32_t* cls_out);

/* ---- The rig's surround view (opt-in): a vehicle's K rectified frames stitched into one top-down panel --------------------------
 * av_ground_warp gives one panel per camera, each in its own camera's road frame.  av_rig_surround gives one panel per VEHICLE in
 * the vehicle's frame: every pixel from the cameras that see that road point, through the mounts and the cameras' ginv.  float64,
 * every operation rounded on its own (no FMA), in the order written.  Panel pixel (r, c) of vehicle v shows the vehicle-frame
 * road point
 *   X = x_far - ((double)r + 0.5) * m_per_px;   Y = (((double)c + 0.5) - (double)gw / 2.0) * m_per_px
 * For camera k = 0 .. n_cams - 1 of the vehicle (entry v * n_cams + k of mounts, ground and bgr: av_rig_fuse's convention), with
 * the mount (cs, sn, mx, my) and q = ground[v * n_cams + k].ginv:
 *   dx = X - mx;  dy = Y - my;  f = cs*dx + sn*dy;  l = cs*dy - sn*dx              (CameraRig.from_vehicle's order)
 *   U, V, D, u, v, tu, tv exactly as av_ground_warp has them for the road point (f, l)
 *   camera k CONTRIBUTES when D > 0 && f >= 0 && f <= max_range && 0 <= tu <= (w-1) * 65536 && 0 <= tv <= (h-1) * 65536
 *   (a NaN fails); its channels p_k are av_ground_warp's bilinear taps at (tu, tv)
 * blend 0, feather -- a weight that is the distance to the frame's border in whole pixels, plus one, in integers:
 *   bu = min(tu, (w-1) * 65536 - tu);  bv = min(tv, (h-1) * 65536 - tv);  wt_k = (min(bu, bv) >> 16) + 1
 *   per channel  out = (2 * sum(wt_k * p_k) + sum(wt_k)) / (2 * sum(wt_k))   over the contributing cameras, integer division
 *   (the sums fit 32 bits: 8 cameras x 16384 x 255)
 * blend 1, nearest -- the contributing camera with the smallest d2 = f*f + l*l gives the pixel; equal d2: the smallest k.
 * No contributing camera: fill.  cover[v][r][c] has bit k set where camera k contributes (under either blend), 0 where none does. */
typedef struct {
    double x_far;        /* vehicle-frame forward coordinate of the panel's top edge, metres; finite */
    double m_per_px;     /* > 0, finite */
    int32_t blend;       /* 0: feather, 1: nearest */
    uint8_t fill[3];     /* b, g, r where no camera sees the road point */
    uint8_t reserved;    /* 0 */
} av_surround_cfg;       /* 24 bytes */
/*   mounts DEVICE [V][K]; ground DEVICE [V*K]; bgr [V*K][h][w][3]: RECTIFIED frames; out [V][gh][gw][3]; cover [V][gh][gw] or NULL
 * AV_EINVAL before any launch and before the context is looked at: a null pointer other than cover and stream; n_vehicles < 1;
 * n_cams not in 1..8; h or w not in 1..32768; gh or gw < 1; n_vehicles or ceil(gh / 16) above 65535; m_per_px not > 0 and finite;
 * x_far not finite; blend not 0 or 1; reserved not 0; out or cover overlapping bgr. */
int av_rig_surround(av_ctx* ctx, av_stream_t stream, const av_surround_cfg* cfg, int n_vehicles, int n_cams,
                    const av_rig_mount* mounts, const av_ground_cfg* ground, int h, int w, const uint8_t* bgr, int gh, int gw,
                    uint8_t* out, uint8_t* cover);

/* generate_polynomial_trajectory for arbitrary (lateral offset, target speed) pairs (:126-204).
 *   state [n_traj][4], end_lateral_offset [n_traj], target_velocity [n_traj] -> waypoints [n_traj][n][6] */
int av_planner_generate(av_ctx* ctx, av_stream_t stream, int n_traj, const double* state,
                        const double* end_lateral_offset, const double* target_velocity,
                        double* waypoints);
/* evaluate_trajectory_cost for caller-supplied trajectories of any length (:206-262), accumulated
 * strictly left to right like the reference.  waypoints [n_traj][n_wp][6]; n_wp == 0 -> +inf (:218). */
int av_planner_evaluate(av_ctx* ctx, av_stream_t stream, int n_traj, int n_wp, const double* waypoints,
                        const double* ref_path, int n_ref, const double* obstacles, int n_obs,
                        double* cost);
/* av_planner_evaluate around moving obstacles [n_obs][5] (x, y, radius, vx, vy): the same strict order (obstacle outer,
 * waypoint inner), each disc at x + vx * t, y + vy * t for t = that waypoint's own field 4. */
int av_planner_evaluate_moving(av_ctx* ctx, av_stream_t stream, int n_traj, int n_wp, const double* waypoints,
                               const double* ref_path, int n_ref, const double* obstacles, int n_obs,
                               double* cost);

/* ---- L1-L7: lane detector ----------------------------------------------------------------------
 * Replaces LaneDetector.detect and its private stages (src/perception/lane_detector.py:47-218):
 * cvtColor(BGR2GRAY) + GaussianBlur 5x5 (:66-74), median-adaptive Canny (:76-84), trapezoid ROI
 * (:47-64,86-90), HoughLinesP(1, pi/180, 50, minLineLength=50, maxLineGap=150) (:92-103), slope split
 * (:105-134), polyfit + EMA + 50-point resampling (:136-176). */
typedef struct {
    int32_t hough_threshold;     /* 50  (:98)  */
    int32_t min_line_length;     /* 50  (:99)  */
    int32_t max_line_gap;        /* 150 (:100) */
    int32_t max_segments;        /* capacity of the per-frame segment list */
    double smoothing_factor;     /* 0.7 (:45)  */
} av_lane_cfg;

/* Scratch the caller allocates once (blurred image, NMS map, union-find labels, edge maps, point list,
 * Hough accumulator, segments).  av_lane_workspace_init zero-fills it (required before first use). */
size_t av_lane_workspace_bytes(int n_streams, int h, int w, int max_segments);
int av_lane_workspace_init(av_ctx* ctx, av_stream_t stream, int n_streams, int h, int w, int max_segments,
                           void* workspace);
/* Byte range of an intermediate inside the workspace (tests, visualisation, the scene stage); `what` is one of: */
#define AV_LANE_VIEW_BLUR 0         /* blurred u8[S][h][w]; widths that are multiples of 16 write it only with AV_LANE_KEEP_EDGES
                                       (with AV_LANE_GIVEN_GRAY: the caller's gray image) */
#define AV_LANE_VIEW_NMS 1          /* NMS map u8[S][h][w] */
#define AV_LANE_VIEW_EDGES 2        /* Canny edges u8[S][h][w], only written with AV_LANE_KEEP_EDGES */
#define AV_LANE_VIEW_MASKED 3       /* ROI-masked edges (consumed by the Hough stage: lines it finds are erased) */
#define AV_LANE_VIEW_THRESHOLDS 4   /* double[S][4]: lo, hi, median, spare */
#define AV_LANE_VIEW_SEGMENTS 5     /* int32[S][max_segments][4] */
#define AV_LANE_VIEW_NSEG 6         /* segment counts int32[S] */
#define AV_LANE_VIEW_ACCUM 7        /* Hough accumulator */
#define AV_LANE_VIEW_HOUGH_PATH 8   /* int32[S], after the Hough stage: the kernel that made the frame's segments -- 1 the
                                       theta-sharded kernel, 2 the single-workgroup kernel, 3 the generic kernel */
#define AV_LANE_VIEW_POINTS 9       /* uint32[S][h*w], after the pixel stages: frame s's ROI edge points x | y << 16, row-major,
                                       from [s][0] (the Hough stage reorders them) */
#define AV_LANE_VIEW_NPOINTS 10     /* point counts int32[S] */
int av_lane_workspace_view(int what, int n_streams, int h, int w, int max_segments, size_t* offset,
                           size_t* bytes);
/*   bgr        u8 [S][h][w][3]
 *   roi_rows   int32 [h][2] inclusive column range kept per row, or NULL for the default trapezoid
 *   lane_state double [S][8]   previous smoothed fit per side: c2 c1 c0 has_prev (prev_left_fit/prev_right_fit)
 *   poly       double [S][2][3]   x = c2*y^2 + c1*y + c0   (side 0 = left, 1 = right)
 *   pts        int32 [S][2][50][2]
 *   info       int32 [S][8]    valid_left valid_right n_left_segments n_right_segments n_segments n_points lo hi
 *   conf       double [S][2]   min(1, n_side_segments / 10)
 *   stages     0 = the whole chain, or a sum of the AV_LANE_* bits below */
#define AV_LANE_KEEP_EDGES 1        /* also write the pre-ROI Canny edge map (view 2) */
#define AV_LANE_PIXELS_ONLY 2       /* stop after the pixel stages (no Hough, no fit): the point lists stay in the workspace */
#define AV_LANE_RESERVED 4          /* ignored */
#define AV_LANE_GENERIC_HOUGH 8     /* Hough by the generic PPHT kernel alone, then the fit (no theta-sharded or single-workgroup
                                       LDS kernel): the Hough kernels' test hook */
#define AV_LANE_HOUGH_ONLY 16       /* skip the pixel stages and run Hough + fit on what the last AV_LANE_PIXELS_ONLY call left in
                                       the workspace -- the two halves of a frame can then be enqueued apart, e.g. the Hough half
                                       beside the next frame's LDS-free kernels (it holds most of a CU's LDS) */
#define AV_LANE_FIT_ONLY 32         /* (with AV_LANE_HOUGH_ONLY) fit only, on the segment list already in the workspace (views
                                       5 / 6): a test hook for the least-squares stage */
#define AV_LANE_GIVEN_GRAY 64       /* Canny of the u8 image the caller left in view 0 (no gray / blur / median) with the thresholds
                                       it left in view 4 (lo, hi as doubles), then the ROI and compaction as usual (the scene
                                       stage: full-frame roi_rows) */
int av_lane_detect(av_ctx* ctx, av_stream_t stream, const av_lane_cfg* cfg, int n_streams, int h, int w,
                   const uint8_t* bgr, const int32_t* roi_rows, void* workspace, double* lane_state,
                   double* poly, int32_t* pts, int32_t* info, double* conf, int stages);

/* ---- D2: YOLO-mode detector ---------------------------------------------------------------------
 * Replaces ObjectDetector._detect_yolo (src/perception/detector.py:103-123), i.e. ultralytics
 * YOLO(model)(frame): letterbox -> YOLOv8n graph (Conv/BN/SiLU, C2f, SPPF, Detect+DFL) -> best-class
 * confidence filter -> class-aware NMS -> boxes scaled back to the frame.  `weights` is a HOST array in
 * the parameter order documented in perception/yolo.py (per conv: weight[cout][cin][k][k], then BN
 * gamma, beta, running_mean, running_var or, for the two plain Conv2d of each head branch, bias);
 * BatchNorm is folded and everything is converted to IEEE half at creation (float32 accumulation).  All activation and NMS scratch
 * is allocated here, once, and the launches of a forward are planned here: a shape that no kernel serves fails at creation.
 * Test hooks, read from the environment once per forward (a change re-plans the launches; outputs stay bit-identical, which is what
 * tests/test_gpu_yolo.py asserts with them): AVHOT_YOLO_NO_FUSE (one launch per layer: no fused front end, no fused C2f blocks, no
 * virtual Upsample + Concat), AVHOT_CONV_GENERIC80 (the 80-channel layers of the class branch on the generic kernels, which have no
 * decode epilogue: the class candidates and with them the detections are not written, the logits of av_yolo_keep_logits are),
 * AVHOT_CONV_NO_GEMM (no GEMM-form convolution), AVHOT_CONV_NO_GEMM_1X1 (none for the 1x1 layers), AVHOT_YOLO_GENERIC_PRE (the
 * generic letterbox kernel for every frame shape).  The library reads no other variable for this stage. */
typedef struct av_yolo av_yolo;
size_t av_yolo_param_count(void);
int av_yolo_create(av_ctx* ctx, int batch, int in_h, int in_w, const float* weights, size_t n_weights,
                   av_yolo** out);
/* The same with a choice of arithmetic.  AV_YOLO_FP16 (av_yolo_create): IEEE-half tensors, weights and MFMA operands, float32
 * accumulation -- the fused production path.  AV_YOLO_FP32: the reference's own precision (ultralytics runs torch float32,
 * detector.py:103-123): float32 tensors, weights and MFMA operands (v_mfma_f32_16x16x4_f32), one generic convolution kernel, no
 * fusion, no deferred tail -- the checking mode for the half-precision path and a second bench figure.  Same entry points otherwise;
 * av_yolo_tensor then returns float32 data. */
#define AV_YOLO_FP16 0
#define AV_YOLO_FP32 1
int av_yolo_create_ex(av_ctx* ctx, int batch, int in_h, int in_w, const float* weights, size_t n_weights, int precision,
                      av_yolo** out);
/* The model family: YOLOv8 Detect models of yolov8.yaml.  av_yolo_model is everything the graph builder reads -- no table per scale
 * exists anywhere else: ch = the widths of the five stages (layers 0/1/3/5/7), rep = the bottleneck pairs of the backbone's C2f blocks
 * (layers 2/4/6/8), neck_rep = those of the neck's (12/15/18/21), nc = classes.  Derived: SPPF ch[4] -> ch[4]/2, 4 ch[4]/2 -> ch[4];
 * Detect box branch ch -> hb -> hb -> 64 with hb = max(16, ch[2]/4, 64), class branch ch -> hc -> hc -> nc with
 * hc = max(ch[2], min(nc, 100)).  Channel counts of the class branch that are no multiple of 16 are padded with zero filters and zero
 * biases up to one (a padded hidden channel is silu(0) = 0 and meets zero weight columns; a padded logit is exactly 0.0f, lies at
 * channels [nc, cstride) of the class logits and is never read by a decode).  av_yolo_model_preset fills a model for scale 'n', 's'
 * or 'm' and 1 <= nc <= 256 (anything else: AV_EINVAL naming it; scales 'l' and 'x' are refused by name).  av_yolo_create_model and
 * av_yolo_model_param_count take exactly what the preset gives for one of those three scales (reserved words zero): any other struct --
 * an l- or x-shaped one, other widths or repeats -- is AV_EINVAL / 0, because only the presets' layer shapes have kernels.  av_yolo_create /
 * av_yolo_create_ex / av_yolo_param_count are the ('n', 80) preset. */
typedef struct av_yolo_model {
    int32_t ch[5];
    int32_t rep[4];
    int32_t neck_rep;
    int32_t nc;
    int32_t reserved[5];            /* zero */
} av_yolo_model;
int av_yolo_model_preset(int scale_char, int nc, av_yolo_model* model);
size_t av_yolo_model_param_count(const av_yolo_model* model);                      /* 0: not a preset of n, s or m */
int av_yolo_create_model(av_ctx* ctx, int batch, int in_h, int in_w, const av_yolo_model* model, const float* weights,
                         size_t n_weights, int precision, av_yolo** out);
int av_yolo_model_of(const av_yolo* h, av_yolo_model* model);                      /* host out */
int av_yolo_destroy(av_yolo* h);
int av_yolo_dims(const av_yolo* h, int* net_h, int* net_w, int* n_anchors);        /* host out */
/*   bgr      u8 [batch][in_h][in_w][3] (device)
 *   det_n    int32 [batch]; det_box float [batch][max_det][4] xyxy in frame pixels (not truncated);
 *   det_conf float [batch][max_det]; det_cls int32 [batch][max_det]; rows in descending confidence */
int av_yolo_forward(av_yolo* h, av_stream_t stream, const uint8_t* bgr, float conf_thres, float iou_thres,
                    int max_det, int32_t* det_n, float* det_box, float* det_conf, int32_t* det_cls);
/* Throughput mode: with the tail deferred, av_yolo_forward enqueues decode + sort + NMS on a stream of its own behind the
 * head convolutions, so that they run beside the NEXT forward's convolutions (one workgroup per image for ~0.25 ms is the
 * latency-bound end of the chain).  Same kernels and results; det_* are complete once `stream` has passed
 * av_yolo_join_tail().  Forwards of one handle still execute in call order. */
int av_yolo_defer_tail(av_yolo* h, int enable);
int av_yolo_join_tail(av_yolo* h, av_stream_t stream);
/* The Detect head's decode (DFL expectation, best class, sigmoid; reference: ultralytics' Detect via detector.py:103-123)
 * runs in the epilogue of the head's last convolutions: the float32 logits are normally neither written nor read.  With
 * keep_logits the head writes them as well and the stand-alone decode kernel runs on them into buffers of its own
 * (tensor ids 120-122), which is how the tests show that both decodes give the same candidates bit for bit. */
int av_yolo_keep_logits(av_yolo* h, int enable);
/* Test hook: device pointer + geometry of an intermediate NHWC tensor (IEEE half; ids = yolov8.yaml layer
 * numbers, 0 = network input: RGB in 4-channel pixels inside a one-pixel frame of zeros, [H+2][W+2]; 100+2i / 101+2i =
 * float32 box / class logits of level i, valid after av_yolo_keep_logits(h, 1); 110 / 111 / 112 = the candidates of every
 * anchor as the head wrote them: box float32 [A][4], confidence float32 [A], class int32 [A]; 120-122 = the same from the
 * stand-alone decode of the kept logits). */
int av_yolo_tensor(const av_yolo* h, int id, void** ptr, int* H, int* W, int* C, int* cstride, int* coff);
/* Test hook: the tail of av_yolo_forward on the caller's candidates instead of the head's.  cand_box float32 [batch][n_anchors][4]
 * (xyxy in network pixels), cand_conf float32 [batch][n_anchors], cand_cls int32 [batch][n_anchors], all on the device, in the
 * handle's geometry (av_yolo_dims); conf_thres / iou_thres / max_det and det_* as in av_yolo_forward, with its argument checks.
 * The launches are the forward's own (one internal function serves both): the same sort kernel by anchor count, the same gain and
 * padding, the handle's sort scratch -- hence AV_ESTATE while a deferred tail of the handle is pending (av_yolo_join_tail first).
 * What the tail computes, here as in the forward: a confidence outside (conf_thres, 1], NaN included, is not a candidate; the
 * candidates are taken in descending confidence, equal confidences in ascending anchor order; a box is dropped when an earlier KEPT box
 * of its class has IoU > iou_thres with it (0/0 of two zero-area boxes is NaN: not dropped); the first max_det kept boxes are
 * mapped back to the frame.  det_n[b] rows of image b are written; rows at and beyond det_n[b] are not written. */
int av_yolo_tail(av_yolo* h, av_stream_t stream, const float* cand_box, const float* cand_conf, const int32_t* cand_cls,
                 float conf_thres, float iou_thres, int max_det, int32_t* det_n, float* det_box, float* det_conf, int32_t* det_cls);
/* Test hook: the ops of the network as av_yolo_create built them, one per layer in execution order (what a forward under
 * AVHOT_YOLO_NO_FUSE launches one by one), so that a test can read one layer's operands and output back and evaluate that layer alone
 * (tests/test_gpu_yolo_layers.py does, in float64).  The query reads host memory only: it launches nothing, copies nothing and does
 * not touch the plan.  A slice is `c` channels from channel `coff` of an NHWC map of `cstride` elements per pixel, H x W per image,
 * image b at ptr + b H W cstride elements; ptr = NULL: the op has no such operand.  Convolutions (AV_YOLO_OP_CONV): weights with
 * BatchNorm folded, half [cout][kpad] with k = tap cin + ci (tap = ky ksz + kx) and zeros from kreal on -- or, with wgt_f32 (the
 * AV_YOLO_FP32 mode), float32 [cout][tap][cin] --, a float32 bias [cout], zero padding ksz / 2, out = act ? silu(.) : (.), then
 * + res.  `out` is float32 for the head's last convolutions (written only with keep_logits or in float32 mode).  in2: the
 * half-resolution map from which the default plan reads input channels [0, in2.c) of this 1x1 layer itself (virtual Upsample + Concat),
 * instead of their upsampled copy in `in`.  AV_YOLO_OP_STEM: `in` is the network input WITH its one-pixel frame of zeros
 * (in_frame = 1: no further padding), 4 channels per pixel, weights half [cout][64] with k = 16 ky + 4 kx + c.  AV_YOLO_OP_POOLS:
 * out channels [i in.c, (i + 1) in.c) = the 5x5 stride-1 maximum applied i + 1 times; AV_YOLO_OP_MAXPOOL: applied once;
 * AV_YOLO_OP_UPSAMPLE: nearest neighbour x2. */
#define AV_YOLO_OP_CONV 0
#define AV_YOLO_OP_STEM 1
#define AV_YOLO_OP_POOLS 2
#define AV_YOLO_OP_MAXPOOL 3
#define AV_YOLO_OP_UPSAMPLE 4
typedef struct av_yolo_slice {
    const void* ptr;
    int32_t H, W, cstride, coff, c;
    int32_t f32;                    /* 1: float32 elements, 0: IEEE half */
} av_yolo_slice;
typedef struct av_yolo_op_info {
    int32_t kind;                   /* AV_YOLO_OP_* */
    int32_t ksz, stride, act, cin, cout;
    int32_t kpad, kreal;            /* row length of the weight matrix, and how much of a row is used */
    int32_t in_frame, wgt_f32;
    av_yolo_slice in, in2, out, res;
    const void* wgt;
    const float* bias;
} av_yolo_op_info;
int av_yolo_op_count(const av_yolo* h, int* n_ops);                                /* host out */
int av_yolo_op(const av_yolo* h, int k, av_yolo_op_info* info);                    /* host out */
/* With a padded class branch (av_yolo_model) an op's cout / out.c and a tensor's C are the REAL channel counts and cstride the padded
 * one; cin / in.c of a convolution that reads a padded map count the operand's channels, zero padding included (the weights' K layout
 * is tap cin + ci with that cin; the padding channels hold zeros on both sides).
 *
 * Test hook: the launches of a forward as they are planned now (for the hooks and keep_logits in force), in order.  family: which
 * kernel family runs the launch; first_op / n_ops: the ops of av_yolo_op it covers (a fused block covers several; an upsample whose
 * reader fetches the source itself is covered by that reader's launch; n_ops = 0: the letterbox); when: AV_YOLO_WHEN_*, the frame
 * pointer alignment the launch is for (both forms of the front end are planned; a forward runs one).  Reads host memory only. */
#define AV_YOLO_K_MFMA 0            /* conv_mfma_kernel: no LDS, one weight stream per wave -- the fallback for any shape */
#define AV_YOLO_K_GEMM128 1
#define AV_YOLO_K_LDS 2
#define AV_YOLO_K_WS3 3
#define AV_YOLO_K_WS1 4
#define AV_YOLO_K_GEMM_F32 5
#define AV_YOLO_K_STEM_F32 6        /* conv_f32_kernel: the float32 chain's no-LDS kernel (its 3-channel stem) */
#define AV_YOLO_K_FIXED 7           /* a fused block, the half-precision stem, pools, upsample, letterbox */
#define AV_YOLO_WHEN_ALWAYS 0
#define AV_YOLO_WHEN_BGR_ALIGNED 1
#define AV_YOLO_WHEN_BGR_UNALIGNED 2
typedef struct av_yolo_step_info {
    int32_t family, first_op, n_ops, when;
    int32_t grid[3], block[3];
    int32_t lds_bytes, lane;
    int32_t variant[6];             /* the family's template parameters */
} av_yolo_step_info;
int av_yolo_plan_count(const av_yolo* h, int* n_steps);                            /* host out */
int av_yolo_plan_step(const av_yolo* h, int k, av_yolo_step_info* info);           /* host out */

/* ---- T3: scene classifier (road type, conditions, lane count) -------------------------------------------
 * Replaces SceneClassifier.classify and its helpers (src/tagging/scene_classifier.py:76-303): BGR2GRAY, Canny(50, 150)
 * and HoughLinesP(1, pi/180, 100, minLineLength=100, maxLineGap=10) on the whole frame, the BGR2HSV green mask
 * inRange((35,40,40), (85,255,255)), np.mean(gray), Laplacian(ksize=1, BORDER_REFLECT_101).var(), the road-type scores
 * and decision rules (:128-202), conditions (:231-259), lane count (:261-280) and the 5-deep road-type vote (:282-298).
 * Per call and stream: scene_front (one read of the frame: gray into the lane workspace, integer pixel sums), the lane
 * chain's Canny with stages bit 6 on the full-frame ROI, the centre edge count on its point list, the lane chain's
 * PPHT, scene_decide.  Enum indices below follow the reference's definition order:
 *   road type  0 unknown 1 intersection 2 highway 3 urban 4 residential 5 parking
 *   condition  0 clear 1 congested 2 night 3 day 4 rain 5 fog */
#define AV_SCENE_STATE_BYTES 64            /* per stream: frame_count, history length, road types of the last 5 frames */
#define AV_SCENE_CAT_TRAFFIC 1             /* category bits of av_scene_classify's per-class table */
#define AV_SCENE_CAT_VEHICLE 2
#define AV_SCENE_CAT_PEDESTRIAN 4
typedef struct av_scene_row {
    uint64_t gray_sum;                     /* sum of the gray image                     */
    uint64_t green_count;                  /* pixels inside the HSV green range         */
    int64_t lap_sum;                       /* sum and sum of squares of the Laplacian   */
    uint64_t lap_sumsq;
    int32_t center_count;                  /* edge pixels in [h/3, 2h/3) x [w/3, 2w/3)  */
    int32_t n_lines;                       /* len(lines) (at most max_segments)         */
    double avg_length;                     /* np.mean of the line lengths (0 without lines) */
    double mean, green_ratio, center_density, lap_var;
    double scores[6];                      /* normalised road-type scores               */
    int32_t road_type_raw;                 /* this frame's decision before the vote      */
    int32_t road_type;                     /* after the vote                             */
    double confidence;
    int32_t n_conditions;
    int32_t conditions[3];
    double condition_conf[3];
    int32_t lane_count;
    int32_t has_pedestrian;
    int32_t n_traffic;                     /* detections of a traffic class (traffic_light / stop_sign) */
    int32_t overflow;                      /* 1: the segment list filled up; the line statistics may be short */
    double timestamp;                      /* frame_count / 30.0                         */
    int32_t frame_count;
    int32_t history_len;
    int32_t history[5];                    /* the vote's history after this frame, oldest first */
    int32_t reserved;
} av_scene_row;                            /* 240 bytes */
size_t av_scene_state_bytes(int n_streams);
int av_scene_reset(av_ctx* ctx, av_stream_t stream, int n_streams, void* state);
/* Scratch of one scene stage: its own lane workspace (views of av_lane_workspace_view with the same S, h, w, max_segments),
 * the pixel sums and the lane outputs it does not use.  av_scene_workspace_init zero-fills it (required before first use). */
size_t av_scene_workspace_bytes(int n_streams, int h, int w, int max_segments);
int av_scene_workspace_init(av_ctx* ctx, av_stream_t stream, int n_streams, int h, int w, int max_segments, void* workspace);
/*   bgr         u8 [S][h][w][3]
 *   max_segments  capacity of the per-frame segment list (OpenCV has none; a full list sets row.overflow)
 *   det_n       int32 [S] (0: detections empty or None); det_cls int32 [S][max_det]; cat u8 [n_cat] AV_SCENE_CAT_* bits per
 *               class id (ids outside the table: no category).  det_n may be NULL (no detections).
 *   speed       f64 [S] ego speed, NaN = no vehicle_state; NULL = none for every stream
 *   lanes       f64 [S][4] {mode, left_x, right_x, 0}: mode 0 = lanes falsy, 1 = a lane is None, 2 = both present with the
 *               lanes' x at the bottom row; ignored when lane_info is given
 *   lane_info, lane_poly   the lane detector's info [S][8] / poly [S][2][3] (av_lane_detect): mode 2 when both sides are
 *               valid, else 1; x = (c2 h + c1) h + c0.  May be NULL.
 *   state       av_scene_state_bytes(S), advanced in place;  rows  av_scene_row [S] */
int av_scene_classify(av_ctx* ctx, av_stream_t stream, int n_streams, int h, int w, const uint8_t* bgr, void* workspace,
                      int max_segments, const int32_t* det_n, const int32_t* det_cls, int max_det, const uint8_t* cat, int n_cat,
                      const double* speed, const double* lanes, const int32_t* lane_info, const double* lane_poly, void* state,
                      av_scene_row* rows);

/* ---- T1: maneuver tags ------------------------------------------------------
 * Replaces ManeuverDetector.detect (src/tagging/maneuver_detector.py:105-262): lateral / longitudinal /
 * turning maneuver of every frame from the current and the 14 previous vehicle states (the reference looks
 * at the newest 10 yaw rates and 15 headings of its 30-deep deques).  Enum fields are indices into the
 * reference's Enum definition order (:18-41).  `state` carries the 14 states before the window per stream. */
#define AV_MANEUVER_STATE_DOUBLES 32   /* frames seen, 14 yaw rates, 14 headings (oldest first), 3 spare */
typedef struct av_maneuver_row {
    int32_t lateral, longitudinal, turning, reserved;
    double lateral_confidence, longitudinal_confidence, turning_confidence;
    double speed_kmh, acceleration, yaw_rate_deg, timestamp;
} av_maneuver_row;                      /* 72 bytes */
int av_maneuver_reset(av_ctx* ctx, av_stream_t stream, int n_streams, double* state);
/*   vstate      f64 [n_streams][n_frames][AV_VSTATE_DOUBLES]  (the out_state of av_kf_step)
 *   lane_offset f64 [n_streams][n_frames], NaN = none for that frame; may be NULL (:197-203)
 *   out         av_maneuver_row [n_streams][n_frames] */
int av_maneuver_detect(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const double* vstate,
                       const double* lane_offset, double* state, av_maneuver_row* out);

/* ---- T2: interaction tags ----------------------------------------------------
 * Replaces InteractionDetector.detect (src/tagging/interaction_detector.py:132-222) and its helpers
 * (_estimate_distance :224, _estimate_relative_speed :250, _calculate_ttc :262, _analyze_interaction :270,
 * _calculate_overall_risk :374): the consumer of the per-frame track tables.  The reference is handed the
 * tracker's returned (confirmed) tracks in order; here those are the snapshot rows with flags bit0 set.  A
 * track's centre-x history (deque of 30, needed by the cut-in rule) lives in `state`, indexed by the row's
 * history slot, which is stable for a track's lifetime.  Types / risks are indices into the reference's Enum
 * definition order (:20-40); type -1 = no interaction for that row. */
typedef struct {
    int32_t frame_h, frame_w;        /* frame_shape (:135), e.g. 720, 1280 */
    int32_t class_kind[16];          /* per class id: 0 other, 1 pedestrian, 2 cyclist/bicycle, 3 car/truck/bus,
                                        4 motorcycle (counted as a vehicle, :160, but outside the vehicle rules) */
} av_interaction_cfg;
typedef struct av_interaction_row {
    int32_t type, risk, agent_id, cls;
    double confidence, distance, relative_speed, ttc;       /* ttc NaN = None */
} av_interaction_row;                /* 48 bytes */
typedef struct av_interaction_summary {
    int32_t agent_count, pedestrian_count, cyclist_count, vehicle_count;
    int32_t n_interactions, primary_type, overall_risk, primary_row;   /* primary_type -1 = None */
    double closest_distance, min_ttc, timestamp;                        /* min_ttc NaN = None */
} av_interaction_summary;            /* 56 bytes */
size_t av_interaction_state_bytes(int tcap);
int av_interaction_reset(av_ctx* ctx, av_stream_t stream, int n_streams, int tcap, void* state);
/*   snap, snap_n   the tracker's per-frame tables (av_tracker_update), tcap == 64.  Windows longer than 64 frames
 *                  are evaluated as independent 64-frame chunks that rebuild the 30-deep histories from the 29
 *                  frames before them; this relies on what the tracker guarantees -- a returned track is returned
 *                  in every frame until it is deleted.  Tables without that property: windows of <= 64 frames.
 *   vstate         f64 [S][W][AV_VSTATE_DOUBLES] (ego speed = element 5); NULL = 10.0 (:166)
 *   has_state      u8 [S][W], 0 = vehicle_state was None for that frame; NULL = always given
 *   vy             f64 [S][W][tcap] image-space y velocity per row instead of the row's float vy; may be NULL
 *   rows           av_interaction_row [S][W][tcap], aligned with the snapshot rows
 *   summary        av_interaction_summary [S][W] */
int av_interaction_detect(av_ctx* ctx, av_stream_t stream, const av_interaction_cfg* cfg, int n_streams, int n_frames,
                          int tcap, const av_track_row* snap, const int32_t* snap_n, const double* vstate,
                          const uint8_t* has_state, const double* vy, void* state, av_interaction_row* rows,
                          av_interaction_summary* summary);

/* ---- Interaction tags of a rig (opt-in): the rules above on av_rig_track's vehicle-frame tracks -----------------------------------
 * av_interaction_detect guesses a distance from the box height and "in front" from the image centre.  Behind av_rig_track the
 * quantities themselves are there -- a position in metres, a filtered velocity on the road, an id that survives camera hand-overs,
 * objects beside and behind the vehicle -- so this tagger is the library's own: the reference's types, confidences, risk levels and
 * thresholds (interaction_detector.py:117-125: 3 / 10 / 8 / 15 / 5 / 30 m, 3.0 s / 1.5 s) on metric inputs, plus the four types a
 * forward camera can never produce (being_followed, vehicle_cut_out, passing, being_passed).  yielding and merging are not produced.
 * Cut-in is tested ahead of following, unlike the reference: a vehicle that has just entered the corridor is a cut-in for as long as
 * its oldest remembered offset lies outside the corridor, and is followed after that.  float64, every operation rounded on its own
 * (no FMA), in the order written. */
typedef struct {
    double dt;                /* 1/30   seconds per frame */
    double corridor_half;     /* 1.75   |lateral| below this is the ego's path, metres */
    double adjacent_half;     /* 5.25   |lateral| below this (and not in the path) is the neighbouring lane, metres */
    double alongside;         /* 10.0   |forward| below this is beside the ego, metres */
    double pass_speed;        /* 1.0    forward speed difference that counts as passing, m/s; all five finite and > 0 */
    int32_t min_hits;         /* the tracker's (av_rig_track_cfg); >= 1 */
    int32_t reserved;
    int32_t class_kind[16];   /* av_interaction_cfg's table and meaning, indexed by the track's class id */
} av_rig_interact_cfg;        /* 112 bytes */
/* Persistent per-vehicle state (device), for capacity tcap (1 .. 512): int64 frames, 8 bytes of 0, then per slot of the tracker
 * { int32 id, int32 cnt, double lat[30] } (248 bytes): the ring of the slot's lateral offsets.  av_rig_interact_reset sets frames
 * to 0, every id to -1 and every other byte to 0. */
size_t av_rig_interact_state_bytes(int tcap);          /* 16 + 248 * tcap; 0 for tcap outside 1 .. 512 */
int av_rig_interact_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int tcap, void* state);
/* One frame per vehicle.  track_state is av_rig_track's state of the same tcap, read only; (x0, y0, h, v0) = plan_state[v].  Slot t
 * of the tracker (id, hits, cls1 = its class word, x, y, vx, vy) is an agent when id >= 0 and hits >= min_hits (coasting tracks
 * included: the planner sees them too).  Per agent:
 *   cs = cos h;  sn = sin h;  c2 = cos(h + pi/2);  s2 = sin(h + pi/2)                                      (av_rig_fuse's)
 *   ex = x - x0;  ey = y - y0;  X = ex*cs + ey*sn;  Y = ex*c2 + ey*s2                                      forward, lateral
 *   rvx = vx - v0*cs;  rvy = vy - v0*sn;  RVX = rvx*cs + rvy*sn                                            relative to the ego
 *   d = sqrt(ex*ex + ey*ey);  closing = d > 0 ? -((ex*rvx + ey*rvy) / d) : 0                               > 0: the range shrinks
 *   ttc = closing > 0.1 ? d / closing : none                                                               (_calculate_ttc)
 *   ring: c = (stored id == id) ? cnt : 0;  lat[c % 30] = Y;  cnt = c + 1;  stored id = id;  hl = min(cnt, 30);
 *         Y0 = the oldest of the last hl entries (lat[0] while cnt <= 30, else lat[cnt % 30])
 *   ahead = X > 0;  in_path = |Y| < corridor_half;  beside = !in_path && |Y| < adjacent_half
 *   kind = class_kind[cls1 - 1] for cls1 in 1..16, else 0
 * Rules, the first hit wins (type, confidence, risk; risk 0 low, 1 medium, 2 high, 3 critical):
 *   1   d < 3                                                        near_miss 9, 0.9, critical
 *   2a  kind 1, d < 10, ahead && in_path                             pedestrian_crossing 6, 0.8, high if d < 8 else medium
 *   2b  kind 1, d < 10, otherwise                                    pedestrian_waiting 7, 0.6, low; relative_speed 0, no ttc
 *   3   kind 2, d < 15                                               cyclist_nearby 8, 0.7, medium if d < 8 else low; no ttc
 *   4a  kind 3, hl >= 10, d < 15, ahead, in_path, |Y0| >= corridor_half    vehicle_cut_in 4, 0.7, medium
 *   4b  kind 3, hl >= 10, d < 15, ahead, !in_path, |Y0| < corridor_half    vehicle_cut_out 5, 0.7, low
 *   4c  kind 3, in_path, 5 < d < 30, ahead                           following_vehicle 1, 0.75, medium if d < 10 else low; high if
 *                                                                    ttc given and < 3
 *   4d  kind 3, in_path, 5 < d < 30, not ahead                       being_followed 2, 0.75, low; high if ttc given and < 3
 *   4e  kind 3, beside, |X| < alongside, RVX < -pass_speed           passing 11, 0.7, low
 *   4f  kind 3, beside, |X| < alongside, RVX > pass_speed            being_passed 12, 0.7, low
 * rows[v][t], slot-indexed: an agent's row holds type (-1: no rule hit), risk, agent_id = id, cls = cls1 - 1, confidence,
 * distance = d, and with a type relative_speed = closing and ttc (NaN: none) unless the rule says otherwise; without a type
 * relative_speed 0, ttc NaN.  A slot that is no agent gets type -1, risk 0, agent_id -1, cls -1, 0.0 and ttc NaN.
 * summary[v]: the counts by kind as av_interaction_detect counts them (vehicle_count: kinds 3 and 4); n_interactions = the rows
 * with a type; closest_distance = the smallest d, inf without agents; min_ttc = the smallest ttc over the agents, NaN when none has
 * one; primary_row / primary_type = the interaction with the highest risk, then the highest confidence, then the smallest slot (-1, -1
 * without one) -- a numeric order, not the reference's sort on the risk's name, because this tagger is the library's own;
 * overall_risk = 3 when an interaction exists and min_ttc < 1.5, else the largest risk (0 without interactions);
 * timestamp = (double)frames * dt, then frames += 1.
 *   track_state [V] x av_rig_track_state_bytes(tcap); plan_state [V][4]; state [V] x av_rig_interact_state_bytes(tcap)
 *   rows av_interaction_row [V][tcap]; summary av_interaction_summary [V]
 * AV_EINVAL before any launch and before the context is looked at: n_vehicles < 1; tcap not in 1..512; a cfg double that is not
 * finite and > 0 (the message names the field); min_hits < 1; a null pointer other than stream. */
int av_rig_interact(av_ctx* ctx, av_stream_t stream, const av_rig_interact_cfg* cfg, int n_vehicles, int tcap, const void* track_state,
                    const double* plan_state, void* state, av_interaction_row* rows, av_interaction_summary* summary);

/* ---- tag log: per-frame tag masks, search, event segments, statistics -----------------------------------------
 * Replaces AutoTagger's bookkeeping (src/tagging/auto_tagger.py:112-310: all_tags, tag_counts, search_by_tag(s),
 * get_high_risk_frames, get_event_segments, get_tag_statistics) for S streams, on the device.  A logged frame is one 64-bit mask
 * over the vocabulary below plus the frame's speed; the tags are laid out in the reference's Enum definition order (the indices
 * the three taggers' rows carry), each group at its base bit.  A frame's tags are a set: the reference's first-seen order inside
 * all_tags is not kept. */
#define AV_TAG_ROAD_TYPE 0            /* 6: unknown intersection highway urban residential parking          */
#define AV_TAG_ELEMENT 6              /* 5: traffic_light stop_sign crosswalk yield_sign speed_limit         */
#define AV_TAG_CONDITION 11           /* 6: clear congested night day rain fog                               */
#define AV_TAG_PEDESTRIAN_AREA 17
#define AV_TAG_LATERAL 18             /* 4 */
#define AV_TAG_LONGITUDINAL 22        /* 5 */
#define AV_TAG_TURNING 27             /* 6 */
#define AV_TAG_INTERACTION 33         /* 13; no_interaction is bit 33 */
#define AV_TAG_RISK 46                /* 3: risk_medium risk_high risk_critical (RiskLevel index - 1) */
#define AV_TAG_COUNT 49               /* bits 49..60 are zero */
#define AV_TAG_HAS_SCENE 61           /* presence flags, not tags: the frame had a scene row / a maneuver row / an */
#define AV_TAG_HAS_MANEUVER 62        /* interaction summary (get_tag_statistics' `if ft.maneuver`, `if ft.interaction`) */
#define AV_TAG_HAS_INTERACTION 63
/* The three taggers' rows of n_streams x n_frames frames as masks and speeds (the get_tags_list of scene_classifier.py:66,
 * maneuver_detector.py:71, interaction_detector.py:95).  Each input group may be NULL; its presence flag is then clear.
 *   maneuver       av_maneuver_row [S][W]: the three enum bits; out_speed = speed_kmh (NaN without maneuver rows)
 *   inter_rows     av_interaction_row [S][W][tcap], inter_summary [S][W], snap_n [S][W] (given together), tcap == 64: the type bit
 *                  of every row below clamp(snap_n, 0, tcap) with 0 <= type < 13 and confidence > 0.5 (exactly 0.5 is no tag);
 *                  risk_<overall_risk> when overall_risk is 1..3
 *   scene          av_scene_row [S][W]: road_type (after the vote), conditions[k] for k < clamp(n_conditions, 0, 3),
 *                  pedestrian_area when has_pedestrian != 0
 *   det_n [S][W], det_cls [S][W][max_det], elem_table u8 [n_elem] (given together, only with scene rows: traffic elements are scene
 *                  tags): per class id 0 = none, else TrafficElement index + 1; one element bit per detection
 *                  i < clamp(det_n, 0, max_det) whose class id lies inside the table and whose entry is 1..5
 * An enum index outside its range sets no bit.   out_mask u64 [S][W], out_speed f64 [S][W] */
int av_tags_pack(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const av_maneuver_row* maneuver,
                 const av_interaction_row* inter_rows, const av_interaction_summary* inter_summary, const int32_t* snap_n, int tcap,
                 const av_scene_row* scene, const int32_t* det_n, const int32_t* det_cls, int max_det, const uint8_t* elem_table,
                 int n_elem, uint64_t* out_mask, double* out_speed);
/* av_tags_pack's maneuver and interaction groups for slot-indexed rows (av_rig_interact's): inter_rows [S][W][tcap] with any tcap in
 * 1..512 and no snap_n -- every row with 0 <= type < 13 and confidence > 0.5 sets its bit, a row of type -1 none.  No scene group.
 * The same kernel.  AV_EINVAL: n_streams or n_frames < 1; inter_rows and inter_summary not given together; tcap outside 1..512
 * with them; a null ctx, out_mask or out_speed. */
int av_tags_pack_slots(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const av_maneuver_row* maneuver,
                       const av_interaction_row* inter_rows, const av_interaction_summary* inter_summary, int tcap,
                       uint64_t* out_mask, double* out_speed);
/* The log: log_mask u64 [S][cap], log_speed f64 [S][cap], log_n int32 [S], dropped int32 [S], the caller's, zeroed to start with.
 * An append copies mask / speed [S][W] behind log_n[s] and advances log_n on the device (no host synchronisation: it can
 * sit in a step).  A frame that does not fit is not written and counted in dropped[s]; log_n never exceeds cap. */
/* av_taglog_append_ex (below) with cols = log_cols = NULL. */
int av_taglog_append(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const uint64_t* mask, const double* speed,
                     int cap, uint64_t* log_mask, double* log_speed, int32_t* log_n, int32_t* dropped);
/* Queries cut a stream's log into chunks of AV_TAGLOG_CHUNK frames, one wave each, and hand what a chunk needs of the chunks before
 * it from launch to launch through `workspace` (av_taglog_workspace_bytes(S, cap) bytes, 8-byte aligned, contents irrelevant
 * between calls; one query at a time per workspace).
 * Frame i of stream s matches when (m & all) == all, (any == 0 or (m & any) != 0) and (m & none) == 0, and first <= i < last;
 * the range is clamped to [0, log_n[s]) (first = 0, last = cap: the whole log). */
#define AV_TAGLOG_CHUNK 1024
size_t av_taglog_workspace_bytes(int n_streams, int cap);
/* A search leaves out_idx int32 [S][out_cap], the matching frame indices, increasing, and out_n [S], the number of matches, which
 * may exceed out_cap; rows at or past min(out_n, out_cap) are not written. */
/* av_taglog_search_where (below) with the three masks, no numeric bound and log_speed = log_cols = NULL. */
int av_taglog_search(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask, const int32_t* log_n,
                     uint64_t all, uint64_t any, uint64_t none, int first, int last, void* workspace, int out_cap,
                     int32_t* out_idx, int32_t* out_n);
/* get_event_segments (auto_tagger.py:281-310): the maximal runs of matching frames with last - first + 1 >= min_duration, in
 * order, as out_seg int32 [S][seg_cap][2] (first, last); a run that reaches the end of the range is closed there.  out_n [S] is
 * the number of such runs, which may exceed seg_cap; rows at or past min(out_n, seg_cap) are not written. */
/* av_taglog_segments_where (below) with the three masks, no numeric bound and log_speed = log_cols = NULL. */
int av_taglog_segments(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask, const int32_t* log_n,
                       uint64_t all, uint64_t any, uint64_t none, int first, int last, int min_duration, void* workspace,
                       int seg_cap, int32_t* out_seg, int32_t* out_n);
/* get_tag_statistics (auto_tagger.py:210-250) of every stream's whole log.  Integer fields and min / max are exact; the partial
 * sums of the chunks are folded in a fixed order, so speed_sum is the same on every call. */
typedef struct av_taglog_stats_row {
    int64_t tag_count[64];          /* frames carrying each bit (the presence flags included) */
    int64_t n_frames, n_maneuver;   /* log_n; frames with AV_TAG_HAS_MANEUVER */
    int64_t risk_count[4];          /* low (AV_TAG_HAS_INTERACTION and none of the risk bits), medium, high, critical */
    double speed_min, speed_max;    /* over the frames with AV_TAG_HAS_MANEUVER; +inf / -inf without one */
    double speed_sum;
} av_taglog_stats_row;              /* 584 bytes */
int av_taglog_stats(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask, const double* log_speed,
                    const int32_t* log_n, void* workspace, av_taglog_stats_row* out);
/* Per-frame records: the numbers of the taggers' rows that a mask cannot hold, kept beside mask and speed as a third log array
 * log_cols av_taglog_cols [S][cap] (array of structs).  They fill the reference's `frames` table (src/database/tag_database.py)
 * and answer numeric queries.  Every value is copied bit for bit from its row; nothing is computed. */
typedef struct av_taglog_cols {
    double road_type_confidence;                       /* av_scene_row.confidence; 0 without a scene row     */
    double lateral_confidence, longitudinal_confidence, turning_confidence;   /* maneuver row; 0 without     */
    double acceleration, yaw_rate_deg;                 /* maneuver row; 0 without                             */
    double min_ttc, closest_distance;                  /* summary, bit for bit (NaN = None); NaN without one  */
    int32_t agent_count, pedestrian_count, cyclist_count, vehicle_count;      /* summary; 0 without          */
} av_taglog_cols;                                      /* 80 bytes */
/* The records of n_streams x n_frames frames from the same three row arrays as av_tags_pack (each may be NULL).
 *   out_cols  av_taglog_cols [S][W] */
int av_tags_cols(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const av_maneuver_row* maneuver,
                 const av_interaction_summary* inter_summary, const av_scene_row* scene, av_taglog_cols* out_cols);
/* The append, with the records moved in the same launch to the same positions.  cols [S][W] and log_cols [S][cap] are both NULL
 * (a log without records) or both given. */
int av_taglog_append_ex(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const uint64_t* mask, const double* speed,
                        const av_taglog_cols* cols, int cap, uint64_t* log_mask, double* log_speed, av_taglog_cols* log_cols,
                        int32_t* log_n, int32_t* dropped);
/* A query over masks, speeds and records.  The mask part is that of av_taglog_search.  A NaN bound is unset and imposes nothing; a
 * set bound is an inclusive comparison with the stored value, hence false where the stored value is NaN (a frame whose min_ttc is
 * None never matches a ttc_max).  A count bound <= 0 imposes nothing. */
typedef struct av_taglog_where {
    uint64_t all, any, none;
    double speed_min, speed_max;        /* log_speed                          */
    double accel_min, accel_max;        /* av_taglog_cols.acceleration        */
    double ttc_max, distance_max;       /* min_ttc, closest_distance          */
    int32_t agents_min, pedestrians_min, cyclists_min, vehicles_min;
} av_taglog_where;                      /* 88 bytes */
/* av_taglog_search / av_taglog_segments with an av_taglog_where in place of the three masks: the same workspace, outputs and
 * out_n contract.  log_speed is loaded only when a speed bound is set, a record's fields only when a bound on them is set;
 * log_cols (or log_speed) may be NULL when no bound needs it, and is refused when one does. */
int av_taglog_search_where(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask, const double* log_speed,
                           const av_taglog_cols* log_cols, const int32_t* log_n, const av_taglog_where* where, int first, int last,
                           void* workspace, int out_cap, int32_t* out_idx, int32_t* out_n);
int av_taglog_segments_where(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask,
                             const double* log_speed, const av_taglog_cols* log_cols, const int32_t* log_n,
                             const av_taglog_where* where, int first, int last, int min_duration, void* workspace, int seg_cap,
                             int32_t* out_seg, int32_t* out_n);
/* The logged frames idx[s][i], i < min(idx_n[s], idx_cap), as out_mask u64 / out_speed f64 / out_cols av_taglog_cols [S][idx_cap];
 * idx int32 [S][idx_cap] and idx_n [S] are what a search left (its out_n may exceed its out_cap, hence the clamp).  An index
 * outside [0, log_n[s]) gives an all-zero record and is never read; rows at or past min(idx_n, idx_cap) are not written;
 * out_cols is written only when log_cols is given. */
int av_taglog_gather(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask, const double* log_speed,
                     const av_taglog_cols* log_cols, const int32_t* log_n, const int32_t* idx, const int32_t* idx_n, int idx_cap,
                     uint64_t* out_mask, double* out_speed, av_taglog_cols* out_cols);

/* ---- rendering ----------------------------------------------------------------
 * Replaces the cv2 drawing behind BEVRenderer.render (src/visualization/bev_renderer.py:286-348 and its helpers
 * :92-284,350-364), OverlayRenderer (src/visualization/overlays.py:26-210) and the draw_* methods of the four hot-path
 * classes (detector.py:171, lane_detector.py:220, multi_object_tracker.py:251, motion_planner.py:305).  A picture is an
 * ORDERED list of primitives (later ones paint over earlier ones), rasterised per pixel by exact integer tests -- the
 * geometry of the reference's calls, not OpenCV's scan conversion, labels in a 5x7 bitmap font: parity unpinned
 * (OpenCV absent), bit-exact against oracle/raster_ref.py. */
enum {
    AV_PRIM_RECT = 1,        /* filled, corners (x0,y0)-(x1,y1) inclusive                                   */
    AV_PRIM_SEG = 2,         /* segment (x0,y0)-(x1,y1), thickness p: pixels within p/2 of it               */
    AV_PRIM_QUAD = 3,        /* filled convex quadrilateral (x0,y0) (x1,y1) (x2,y2) (x3,y3), edges included */
    AV_PRIM_DISC = 4,        /* filled circle, centre (x0,y0), radius p                                     */
    AV_PRIM_RING = 5,        /* circle outline of thickness 1, centre (x0,y0), radius p                     */
    AV_PRIM_GLYPH = 6,       /* character p (ASCII 32..126) of the 5x7 font, top-left (x0,y0), scale x1     */
    AV_PRIM_BLEND_RECT = 7,  /* rectangle blended 0.7 picture + 0.3 colour (cv2.addWeighted panels)         */
    AV_PRIM_POLY_BLEND = 8   /* polygon verts[x0 .. x0+y0), even-odd, blended the same; (x2,y2)-(x3,y3) = its bounding box */
};
typedef struct {
    int32_t type;
    int32_t x0, y0, x1, y1, x2, y2, x3, y3;
    int32_t p;
    uint8_t b, g, r, a;      /* colour in OpenCV's channel order; a unused */
    int32_t reserved;
} av_prim;                   /* 48 bytes */
/*   img     u8 [n_images][h][w][3], drawn in place
 *   prims   av_prim [n_images][prim_cap], n_prims int32 [n_images]
 *   verts   int32 [n_images][vert_cap][2] polygon vertices (x, y); may be NULL when no POLY primitive is used */
int av_raster_draw(av_ctx* ctx, av_stream_t stream, int n_images, int h, int w, uint8_t* img, const av_prim* prims, int prim_cap,
                   const int32_t* n_prims, const int32_t* verts, int vert_cap);
/* The BEV panel of BEVRenderer.render (bev_renderer.py:286-348) as a primitive list built ON THE DEVICE from the hot
 * loop's tables -- planner waypoints + stable order, tracker snapshot rows + history rings, Kalman output -- for frame
 * `frame` of the window of every stream; paint it with av_raster_draw over the road image.  Layering as the reference:
 * candidates of rank 1 .. n_candidates-1 (grey), the planned path (rank 0, green, a disc on every third waypoint), the
 * confirmed tracks (footprint, outline, heading arrow, "ID:n", trail), the ego vehicle + uncertainty circle, the legend.
 * The list has a fixed layout of av_bev_prim_cap() slots per stream; unused slots are type 0. */
typedef struct {
    int32_t width, height;          /* 600, 600 (bev_renderer.py:29-33) */
    double pixels_per_meter;        /* 10.0 */
    double x_min, x_max, y_min, y_max;   /* (-30, 30), (-10, 50) */
    int32_t n_candidates;           /* how many of the ranked candidates to show (demo.py:143 passes candidate_trajs[:10]) */
    int32_t reserved;
} av_bev_cfg;
int av_bev_prim_cap(const av_bev_cfg* cfg, int tcap, int n_points);
/*   snap, snap_n   [S][W][tcap], [S][W] of av_tracker_update; tracker_state its persistent state (history rings)
 *   vstate         [S][W][AV_VSTATE_DOUBLES] of av_kf_step, or NULL (no ego vehicle)
 *   waypoints      [S*W][C][n][6], order [S*W][C] of av_planner_plan
 *   prims          av_prim [S][prim_cap], n_prims int32 [S]
 * The history rings hold the trails as of the END of the window: build panels for frame = W-1 (or run W = 1). */
int av_bev_build(av_ctx* ctx, av_stream_t stream, const av_bev_cfg* cfg, int n_streams, int n_frames, int frame, int tcap,
                 int trajectory_length, const av_track_row* snap, const int32_t* snap_n, const void* tracker_state,
                 const double* vstate, const double* waypoints, const int32_t* order, av_prim* prims, int prim_cap, int32_t* n_prims);
/* Bilinear resize (half-pixel centres) of src [sh][sw][3] into the dh x dw window at column dst_x0 of a picture whose
 * rows hold dst_pitch_px pixels: OverlayRenderer.create_side_by_side's cv2.resize + hstack (overlays.py:187-196). */
int av_resize_into(av_ctx* ctx, av_stream_t stream, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, int dst_pitch_px,
                   int dst_x0);

/* The source / destination form of av_raster_draw: the h x w pictures src [n_images][h][src_pitch_px][3] are painted into the h x w
 * window at column dst_x0 of dst [n_images][h][dst_pitch_px][3]; every pixel is read once and written once, the source stays as it
 * is.  src == dst with equal pitches and dst_x0 = 0 is av_raster_draw; any other overlap of the two is refused (AV_EINVAL). */
int av_raster_draw_to(av_ctx* ctx, av_stream_t stream, int n_images, int h, int w, const uint8_t* src, int src_pitch_px, uint8_t* dst,
                      int dst_pitch_px, int dst_x0, const av_prim* prims, int prim_cap, const int32_t* n_prims, const int32_t* verts,
                      int vert_cap);

/* The overlay of a rig's surround view: what the ego loop planned around as a primitive list over av_rig_surround's panel (paint it
 * with av_raster_draw).  A fixed layout of
 * av_rig_view_prim_cap() slots per vehicle, unused slots type 0, n_prims[v] = that number; in order:
 *   rcap - 1      the reference path: segment i joins ref_path[v][i] and [i + 1], i + 1 < clamp(n_ref[v], 0, rcap); AV_PRIM_SEG,
 *                 thickness 1, (b, g, r) = (0, 255, 255).  ref_path and n_ref may be NULL (together)
 *   n_points - 1  the planned trajectory: the waypoints of candidate order[v][0] (an index outside 0 .. n_cand - 1: none), fields 0
 *                 and 1 of consecutive ones joined; thickness 3, green (0, 255, 0).  waypoints and order may be NULL (together)
 *   2 * ocap      per obstacle row i < clamp(n_obs[v], 0, ocap) of (x, y, r[, vx, vy]): slot 2i an AV_PRIM_RING about (x, y) of
 *                 radius p = max(1, (int)floor(r / m_per_px + 0.5)) (type 0 unless that floor is <= 32767; a NaN fails), slot
 *                 2i + 1 with ncol 5 an AV_PRIM_SEG of thickness 1 from (x, y) to where the obstacle is one second on,
 *                 (x + vx, y + vy), with ncol 3 type 0.  Colour: av_bev_build's agent colour ((ids[v][i] % 6) + 6) % 6, without
 *                 ids red (0, 0, 255)
 *   1             the ego vehicle: an AV_PRIM_QUAD with the vehicle-frame corners (2.25, -0.9) (2.25, 0.9) (-2.25, 0.9)
 *                 (-2.25, -0.9), white
 * A world point (wx, wy) is placed with (x0, y0, hd, .) = plan_state[v] (float64, no FMA):
 *   dx = wx - x0;  dy = wy - y0;  ch = cos(hd);  sh = sin(hd);  X = dx*ch + dy*sh;  Y = dy*ch - dx*sh       (the vehicle frame)
 *   pc = floor(Y / m_per_px + (double)gw / 2.0);  pr = floor((x_far - X) / m_per_px)                        (column, row)
 * and is drawable when pc and pr are both finite and within -32768 .. 32767; a primitive with an undrawable point is type 0.
 *   plan_state [V][4]; obstacles [V][ocap][ncol], n_obs [V], ids [V][ocap] or NULL; ref_path [V][rcap][2], n_ref [V];
 *   waypoints [V][n_cand][n_points][6], order [V][n_cand] (av_planner_plan's, one state per vehicle); prims [V][prim_cap]
 * Only cfg's x_far and m_per_px are read.  AV_EINVAL before any launch and before the context is looked at: n_vehicles not in
 * 1..65535; gh or gw not in 1..8191; ncol not 3 or 5; ocap, rcap, n_cand or n_points < 1; prim_cap below av_rig_view_prim_cap() or
 * above 65535; m_per_px not > 0 and finite, x_far not finite; one of ref_path / n_ref or of waypoints / order without the other;
 * any other null pointer except ids and stream. */
int av_rig_view_prim_cap(int ocap, int rcap, int n_points);    /* (rcap-1) + (n_points-1) + 2*ocap + 1; 0 for an argument < 1 */
int av_rig_view_build(av_ctx* ctx, av_stream_t stream, const av_surround_cfg* cfg, int n_vehicles, int gh, int gw,
                      const double* plan_state, int ncol, int ocap, const double* obstacles, const int32_t* n_obs,
                      const int32_t* ids, int rcap, const double* ref_path, const int32_t* n_ref,
                      int n_cand, int n_points, const double* waypoints, const int32_t* order,
                      av_prim* prims, int prim_cap, int32_t* n_prims);

/* ---- the demo's annotated view (demo.py:122-150), composed on the device ---------------------------------------------------------
 * av_camview_build writes, one workgroup per camera, the primitive list of the camera view from what a camera loop's step left in
 * HBM, in the order and with the arithmetic of the class methods demo.py calls; `flags` selects the layers:
 *   AV_VIEW_DETECTIONS  ObjectDetector.draw_detections: every box of det_* in order (float32 coordinates truncated toward zero),
 *                       colour det_colors[cls] (white outside the table), outline 2, label box, "name 0.87" ("unknown" outside
 *                       the name table; the confidence is "%.2f" of the float32 widened to double)
 *   AV_VIEW_LANES       LaneDetector.draw_lanes: the blended area left + reversed right when both sides exist (lane_info[s][0],
 *                       [1]), then the left and the right polyline, thickness 3
 *   AV_VIEW_TRACKS      MultiObjectTracker.draw_tracks (defaults): confirmed rows of the snapshot in table order, palette[id % 8],
 *                       "ID:n name" (the class id in decimal outside trk_names), the trail from the history ring
 *   AV_VIEW_INFO        OverlayRenderer.draw_info_panel: "Frame: n" (the tracker's frame counter - 1), "FPS: %.1f" (fps), and from
 *                       vstate speed * 3.6, heading * (180 / pi), acceleration, position (vstate NULL: the first two lines only)
 *   AV_VIEW_SUMMARY     draw_detection_summary, top right: a count per class name in order of first appearance (names are told
 *                       apart by their id: two ids with one name would be listed twice; ids outside the table are one "unknown")
 *   AV_VIEW_GAUGE       draw_lane_offset_indicator of get_lane_center_offset (the empty gauge without a lane pair)
 * The list is compacted: n_prims[s] primitives, no empty slots.  Number text is that of Python's % operator (csrc/fmtnum.h).
 * Name tables: char [n][AV_NAME_BYTES] plus int32 lengths [n] (negative: no such id), at most max_name (< AV_NAME_BYTES) characters
 * are drawn; det_colors u8 [n_det_colors][3] in B, G, R order. */
#define AV_NAME_BYTES 24
enum {
    AV_VIEW_DETECTIONS = 1, AV_VIEW_LANES = 2, AV_VIEW_TRACKS = 4, AV_VIEW_INFO = 8, AV_VIEW_SUMMARY = 16, AV_VIEW_GAUGE = 32,
    AV_VIEW_DEMO = 31,       /* the layers demo.py draws */
    AV_VIEW_ALL = 63
};
typedef struct {
    int32_t n_streams, h, w;                /* cameras, frame size */
    int32_t flags;                          /* AV_VIEW_* */
    int32_t n_frames, frame;                /* snap / snap_n / vstate are [S][n_frames][..]; the frame of the window to draw */
    int32_t max_det, tcap, trajectory_length, max_name;
    int32_t n_det_names, n_det_colors, n_trk_names, reserved;
    double fps;
    const int32_t* det_n;                   /* [S] */
    const float* det_box;                   /* [S][max_det][4] x1 y1 x2 y2 */
    const float* det_conf;                  /* [S][max_det] */
    const int32_t* det_cls;                 /* [S][max_det] */
    const char* det_names;                  /* [n_det_names][AV_NAME_BYTES] */
    const int32_t* det_name_len;            /* [n_det_names] */
    const uint8_t* det_colors;              /* [n_det_colors][3] */
    const int32_t* lane_pts;                /* [S][2][50][2] of av_lane_detect */
    const int32_t* lane_info;               /* [S][8] of av_lane_detect */
    const av_track_row* snap;               /* [S][n_frames][tcap] */
    const int32_t* snap_n;                  /* [S][n_frames] */
    const void* tracker_state;              /* the tracker's persistent state: frame counter and history rings */
    const char* trk_names;                  /* [n_trk_names][AV_NAME_BYTES] */
    const int32_t* trk_name_len;            /* [n_trk_names] */
    const double* vstate;                   /* [S][n_frames][AV_VSTATE_DOUBLES] or NULL */
} av_camview_args;
/* slots a camera's list can need; 0 for arguments out of range (max_det, tcap <= 1024, max_name < AV_NAME_BYTES) */
int av_camview_prim_cap(int max_det, int tcap, int trajectory_length, int max_name);
/*   prims  av_prim [S][prim_cap], n_prims int32 [S]; verts int32 [S][vert_cap][2], vert_cap >= 100 with AV_VIEW_LANES
 * AV_EINVAL when av_camview_prim_cap() exceeds the rasteriser's 65535 or prim_cap is below it. */
int av_camview_build(av_ctx* ctx, av_stream_t stream, const av_camview_args* args, av_prim* prims, int prim_cap, int32_t* n_prims,
                     int32_t* verts, int vert_cap);

/* OverlayRenderer.create_side_by_side for n_images pairs in one launch: both pictures at the taller one's height th, the one that
 * keeps its height copied, the other resized by av_resize_into's rule to int(w * (th / h)) columns (overlays.py:88-90), the labels
 * at (10, 25) and (nw1 + 10, 25) in the doubled font.   cam u8 [n][h1][w1][3], bev u8 [n][h2][w2][3], out u8 [n][th][nw1 + nw2][3].
 * cam (or bev) may be NULL when that half keeps its size and is already in place in `out` (painted there by av_raster_draw_to):
 * the call then writes the other half and the labels only.  Labels: at most AV_VIEW_LABEL_BYTES - 1 characters. */
#define AV_VIEW_LABEL_BYTES 32
int av_view_compose_size(int h1, int w1, int h2, int w2, int* th, int* nw1, int* nw2);
int av_view_compose(av_ctx* ctx, av_stream_t stream, int n_images, const uint8_t* cam, int h1, int w1, const uint8_t* bev, int h2, int w2,
                    uint8_t* out, const char* label1, const char* label2);

/* "%.{decimals}f" % v as Python writes it, decimals 0 .. 2 (csrc/fmtnum.h, the formatter the view builder runs on the device): exact
 * for |v| < 1e9, "nan" / "inf" / "-inf", and "inf" / "-inf" for a finite |v| >= 1e9.  `cap` characters fit in out, no terminator is
 * written.  -> the length, or AV_EINVAL (bad argument, or the text does not fit: nothing is written).  Needs no context. */
int av_format_fixed(double v, int decimals, char* out, int cap);

/* Interleaved BGR -> planar YUV 4:2:0 (I420), the inverse direction of av_i420_to_bgr, for writing uncompressed video: BT.601 limited
 * range in OpenCV's 20-bit constants (Y = (269484 R + 528482 G + 102760 B + 2^19 >> 20) + 16; U, V from -155188 / -305135 / 460324
 * and 460324 / -385875 / -74448, + 128), chroma from the rounded mean colour of each 2 x 2 block.  Parity unpinned (OpenCV absent).
 *   bgr u8 [n_frames][h][w][3];  yuv u8 [n_frames][h*w*3/2];  h and w even (AV_EINVAL otherwise) */
int av_bgr_to_i420(av_ctx* ctx, av_stream_t stream, int n_frames, int h, int w, const uint8_t* bgr, uint8_t* yuv);

/* ---- video ingest ----------------------------------------------------------------
 * The pixel half of VideoDataLoader.read_frame / read_frame_at (data/loaders/video_loader.py:88-131): what a decoder hands over
 * as planar YUV 4:2:0 becomes the BGR frame cv2.VideoCapture.read returns, then av_resize_into scales it to target_size
 * (:103-104).  Baseline JPEG (Motion-JPEG) is decoded by av_jpeg_decode below; no other bitstream decoder is here.
 *   yuv  u8 [n_frames][h*w*3/2]  I420: Y plane, then U, then V (each (h/2) x (w/2));   bgr  u8 [n_frames][h][w][3] */
int av_i420_to_bgr(av_ctx* ctx, av_stream_t stream, int n_frames, int h, int w, const uint8_t* yuv, uint8_t* bgr);

/* Baseline JPEG (Motion-JPEG in AVI, or a raw .mjpeg stream) decoded on the device: the one compressed format this library opens.
 * Supported: one SOF0 frame (8-bit, Huffman), one interleaved scan (Ss 0, Se 63, Ah = Al = 0), 1 component (gray) or 3 (YCbCr) with
 * luma sampling 1x1, 2x1 or 2x2 and 1x1 chroma (4:4:4 / 4:2:2 / 4:2:0), 8-bit DQT, DHT in the frame or absent (then the four "typical"
 * tables of ITU-T T.81 Annex K, as AVI MJPEG frames expect), optional DRI with RST0-7; APPn / COM are skipped by their length.
 *
 * The pixels are those of libjpeg's default path (what Pillow / libjpeg-turbo produce; tests/golden/mjpeg.npz pins them bit for bit):
 *   entropy   EXTEND(v, s) = v if v >= 2^(s-1) else v - 2^s + 1; the DC predictors are 0 at the start of every restart segment.
 *   IDCT      jidctint "islow": CONST_BITS 13, PASS1_BITS 2, columns first, on coefficient * quantiser, with the constants
 *             2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172.  Even part: z1 = (in2 + in6) * 4433;
 *             tmp2 = z1 - in6 * 15137; tmp3 = z1 + in2 * 6270; tmp0 = (in0 + in4) << 13; tmp1 = (in0 - in4) << 13.  Odd part from
 *             in7, in5, in3, in1 with z5 = (z3 + z4) * 9633 and the multipliers 2446, 16819, 25172, 12299, -7373, -20995, -16069,
 *             -3196.  Descale with rounding by 11 after the columns and by 18 after the rows, + 128, clamp to 0..255.  (32-bit
 *             two's-complement arithmetic throughout: what a damaged stream's coefficients overflow wraps.)
 *   chroma    libjpeg's "fancy" triangle filters over the real chroma extent ceil(w/2) x ceil(h/2) (x h for 4:2:2); edge samples
 *             stand in for neighbours outside it.  2x1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2.
 *             2x2: t[i] = 3 near[i] + far[i] (far: the chroma row above for the upper output row, below for the lower one), then
 *             out[2i] = (3 t[i] + t[i-1] + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4.
 *   colour    cb, cr centred by -128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 *             G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), arithmetic shifts, clamped.  Gray goes to all three channels.
 * Parity with OpenCV's FFmpeg-based MJPEG decoder is unpinned (neither is in this image).
 *
 * av_jpeg_desc: what av_jpeg_parse reads from one frame's headers (928 bytes; quantisers in natural order, Huffman tables as BITS /
 * HUFFVAL, selectors per component).  seg_base and byte_base are the caller's: where this frame's segments start in the batch's
 * segment table and where its bytes start in the batch's byte buffer.  av_jpeg_seg: the byte range [begin, end) of one restart
 * interval's entropy data, relative to the frame's first byte; segment i holds the MCUs [i * restart_interval, ...) (without DRI:
 * one segment, the whole scan). */
typedef struct av_jpeg_desc {
    int32_t width, height, ncomp;       /* ncomp 1 or 3 */
    int32_t hs, vs;                     /* luma sampling factors: 1x1, 2x1 or 2x2 (1x1 for gray) */
    int32_t restart_interval;           /* MCUs per segment; 0: no DRI */
    int32_t n_segments;                 /* ceil(MCUs / restart_interval), or 1 */
    int32_t flags;                      /* AV_JPEG_ESEGS when the scan held another number of restart intervals; goes into status */
    int32_t scan_offset;                /* first byte of entropy data */
    int32_t seg_base;                   /* caller: index of this frame's first av_jpeg_seg in the batch's table */
    uint32_t byte_base;                 /* caller: offset of this frame's first byte in the batch's byte buffer */
    int32_t reserved;
    uint8_t tq[4], td[4], ta[4], pad[4];/* per component: quantiser, DC table, AC table */
    uint8_t qt[4][64];                  /* natural (row-major) order */
    uint8_t dc_bits[2][16], dc_val[2][16], ac_bits[2][16], ac_val[2][256];
} av_jpeg_desc;
typedef struct av_jpeg_seg {
    uint32_t begin, end;
} av_jpeg_seg;
#define AV_JPEG_DESC_BYTES 928

/* status bits of a decoded frame (0: every segment decoded cleanly).  A segment that hits one of the first four stops there: its
 * block in progress and all its later blocks decode as all-zero coefficients (mid-gray); other segments and frames are unaffected. */
#define AV_JPEG_ECODE 1   /* a bit pattern that is no Huffman code */
#define AV_JPEG_ERUN 2    /* a zero run past coefficient 63 */
#define AV_JPEG_EBYTES 4  /* the segment's bytes ran out (also: a 0xFF not followed by 0x00 inside it) */
#define AV_JPEG_ELEFT 8   /* whole bytes left over after the segment's last block */
#define AV_JPEG_ESEGS 16  /* the scan held fewer or more restart intervals than the frame size asks for (set by av_jpeg_parse) */
#define AV_JPEG_EDESC 32  /* the descriptor is not one av_jpeg_parse makes for this h x w: nothing decoded, the frame is mid-gray */

/* av_jpeg_parse refuses what is not supported, each kind with its own code (and av_last_error_string): */
#define AV_EJPEG_TRUNCATED (-101)  /* the bytes end inside the headers */
#define AV_EJPEG_FORMAT (-102)     /* no SOI, a malformed segment, no frame header before the scan */
#define AV_EJPEG_SOF (-103)        /* SOF1/2/3/5/6/7: extended, progressive, lossless, hierarchical */
#define AV_EJPEG_ARITH (-104)      /* SOF9..15 or DAC: arithmetic coding */
#define AV_EJPEG_PRECISION (-105)  /* sample precision other than 8 */
#define AV_EJPEG_COMPONENTS (-106) /* neither 1 nor 3 components */
#define AV_EJPEG_SAMPLING (-107)   /* sampling factors other than 4:4:4, 4:2:2, 4:2:0 */
#define AV_EJPEG_DQT16 (-108)      /* a 16-bit quantiser table */
#define AV_EJPEG_MULTISCAN (-109)  /* a scan that does not hold every component, or a second scan */
#define AV_EJPEG_SIZE (-110)       /* the frame is not h x w */
#define AV_EJPEG_TABLE (-111)      /* a table that is missing, out of range or no prefix code */
#define AV_EJPEG_SCAN (-112)       /* scan parameters other than Ss 0, Se 63, Ah 0, Al 0 */
#define AV_EJPEG_SEGCAP (-113)     /* more restart intervals than seg_cap */

/* Host half, needs no context and no device.  Reads one frame (`len` bytes from SOI) that has to be h x w, fills *desc (seg_base and
 * byte_base left 0) and segs[0 .. desc->n_segments), found by walking the scan for FF D0-D7 / FF D9 (FF 00 is stuffing; a scan that
 * ends without EOI ends at `len`).  Every offset is <= len.  -> AV_OK, AV_EINVAL (null / non-positive argument) or AV_EJPEG_*. */
int av_jpeg_parse(const uint8_t* data, size_t len, int h, int w, av_jpeg_desc* desc, av_jpeg_seg* segs, int seg_cap, int* n_segs);

/* Device half.  Decodes n_frames frames of one h x w in one call into bgr u8 [n_frames][h][w][3] and status i32 [n_frames] (AV_JPEG_E*
 * bits).  desc [n_frames], segs [n_segs_total] and bytes [n_bytes] are DEVICE copies; bytes is 4-byte aligned and n_bytes includes at
 * least 8 bytes of padding behind the last frame.  A batch may mix frames of different files, tables, subsampling and restart
 * intervals.  max_segs sizes the entropy launch (one lane per frame and restart segment): a frame whose n_segments exceeds it is not
 * decoded (AV_JPEG_EDESC, mid-gray).  The kernels
 * bound every descriptor field, segment index and byte offset themselves (AV_JPEG_EDESC / clamped to n_bytes), so a wrong table
 * cannot make them read or write outside the buffers given here.  workspace: av_jpeg_workspace_bytes(n_frames, h, w) bytes, 16-byte
 * aligned, contents irrelevant before and after.  Enqueues four kernels on `stream`; no host synchronisation, no allocation. */
size_t av_jpeg_workspace_bytes(int n_frames, int h, int w);
int av_jpeg_decode(av_ctx* ctx, av_stream_t stream, int n_frames, int h, int w, const av_jpeg_desc* desc, const av_jpeg_seg* segs,
                   int n_segs_total, int max_segs, const uint8_t* bytes, size_t n_bytes, void* workspace, uint8_t* bgr, int32_t* status);

/* ---- video output: baseline JPEG (Motion-JPEG) encoded on the device ------------------------------------
 * Frames of BGR u8 become baseline JPEG frames that equal, byte for byte, what libjpeg's default compress path writes (Pillow /
 * libjpeg-turbo; tests/golden/mjpeg_encode.npz pins them): three components (Y, Cb, Cr), 4:2:0, 4:2:2 or 4:4:4, any h, w >= 1, the
 * Annex K Huffman tables, quantisers from `quality`, optional restart intervals.  Grayscale, progressive, optimised Huffman tables
 * and 16-bit quantisers are out of scope.  All arithmetic is 32-bit integer:
 *   colour    FIX(x) = int(x * 65536 + 0.5): Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16,
 *             Cb = (-FIX(.168735892) R - FIX(.331264108) G + FIX(.5) B + (128 << 16) + 32767) >> 16,
 *             Cr = (FIX(.5) R - FIX(.418687589) G - FIX(.081312411) B + (128 << 16) + 32767) >> 16.
 *   edges     luma is edge-replicated to whole MCUs.  Full-resolution chroma is replicated to the right to whole MCUs and at the
 *             bottom only to a multiple of the vertical sampling factor, then downsampled (4:2:2: (a + b + bias) >> 1, bias 0, 1, 0,
 *             1 .. along the output row; 4:2:0: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ..); the downsampled plane is then
 *             replicated down to whole MCUs.
 *   DCT       jfdctint "islow" on samples - 128: CONST_BITS 13, PASS1_BITS 2, the constants of the decoder's IDCT; rows first
 *             (outputs scaled up by 4, the odd part descaled by 11), then columns (even terms descaled by 2, the rest by 15).
 *   quantise  sign(c) * ((|c| + (8 q >> 1)) / (8 q)).  Tables: scale = 5000 / quality below 50, else 200 - 2 quality;
 *             (base * scale + 50) / 100 clamped to 1..255 over the Annex K luminance and chrominance tables.
 *   dummies   blocks of an MCU wholly outside ceil(w/8) x ceil(h/8) luma blocks take no pixels: AC 0, DC of the block coded before
 *             them in the MCU.
 *   entropy   differential DC per component (0 at every restart), run/size symbols with ZRL and EOB, bits MSB first, the last byte
 *             of every restart interval and of the scan padded with 1-bits, FF followed by 00, RST(k mod 8) between intervals.
 *   layout    SOI, APP0 JFIF 1.01 (units 0, density 1 x 1), DQT luma, DQT chroma, SOF0, DHT DC0, AC0, DC1, AC1, DRI when a restart
 *             interval is set, SOS, data, EOI. */
#define AV_JPEG_444 0
#define AV_JPEG_422 1
#define AV_JPEG_420 2
#define AV_JPEG_EFULL 64  /* status bit of an encoded frame: it needs more than out_cap bytes (len tells how many) */

/* Host half, needs no context and no device.  Writes SOI .. the SOS header of an h x w frame into out (cap bytes; 640 always
 * suffice) and the two quantiser tables, natural order, into qt (what av_jpeg_encode takes).  restart_mcus: -1 one MCU row per
 * restart interval, 0 no restart markers, else MCUs per interval, 1..65535.  -> the header's length, or AV_EINVAL (null pointer,
 * h or w outside 1..65535 or more than 2^21 blocks, quality outside 1..100, unknown subsampling, bad restart_mcus, cap too small). */
int av_jpeg_encode_header(int h, int w, int quality, int subsampling, int restart_mcus, uint8_t* out, int cap, uint8_t qt[2][64]);

/* Device half.  Encodes n_frames frames bgr u8 [n_frames][h][w][3] in one call.  qt (u8 [2][64]) and header (header_len bytes, as
 * av_jpeg_encode_header made them for the same h, w, subsampling and restart_mcus) are DEVICE copies.  Frame k is written
 * contiguously at out + k * out_cap: header, scan, EOI.  len[k] (i32, device) is the length the frame needs whether or not it
 * fitted; status[k] is 0, or AV_JPEG_EFULL when len[k] > out_cap: then nothing is written at or beyond out + (k + 1) * out_cap and
 * the content of that slot is unspecified.  workspace: av_jpeg_encode_workspace_bytes(n_frames, h, w, subsampling) bytes, 16-byte
 * aligned, contents irrelevant before and after (0: bad arguments).  The kernels index the caller's buffers by the geometry of the
 * arguments checked here only.  Enqueues nine kernels on `stream`; no host synchronisation, no allocation. */
size_t av_jpeg_encode_workspace_bytes(int n_frames, int h, int w, int subsampling);
int av_jpeg_encode(av_ctx* ctx, av_stream_t stream, int n_frames, int h, int w, const uint8_t* bgr, const uint8_t* qt, int subsampling,
                   int restart_mcus, const uint8_t* header, int header_len, void* workspace, uint8_t* out, int out_cap, int32_t* len,
                   int32_t* status);

/* ---- synthetic input ---------------------------------------------------
 * Deterministic 8-bit BGR road scenes generated on the device, standing in for the reference's lost
 * SyntheticDataGenerator (data/generators, source absent).  Frame (stream0+s, frame) is bit-identical to
 * oracle/lane_ref.py: synthetic_frame().   bgr: u8 [n_streams][h][w][3] */
int av_synth_frames(av_ctx* ctx, av_stream_t stream, int n_streams, int h, int w, int stream0, int frame,
                    uint8_t* bgr);

/* ---- one launch per time-step (BASELINE config 4, window 1; the reference's per-frame cadence, demo.py:97-120) -----------
 * av_hot_step = av_simdet_generate + av_tracker_update + av_kf_step + av_planner_plan (no reference path / obstacles) for ONE
 * frame of every stream, as a single kernel with role-split workgroups that run the stage kernels' own device code: the
 * results are those of the four calls bit for bit.  A step's arguments are two structs -- av_step_loop: what all steps of a
 * loop share (the configurations, the shapes, the persistent state); av_step_set: the buffers one step reads and writes -- plus
 * the wire tables.  Buffers as in the stage calls with n_frames = 1:
 *   frame_count [S]; det_n [S], det_box [S][dcap][4], det_cls / det_conf [S][dcap], det_status [S] or NULL;
 *   tracker_state as av_tracker_update; snap [S][tcap] + snap_n [S] (or both NULL); det2trk [S][dcap];
 *   z [S][4]; kf_state [S][AV_KF_STATE_DOUBLES]; vstate [S][AV_VSTATE_DOUBLES]; plan_state [S][4];
 *   waypoints [S][C][n][6] or NULL; cost, order [S][C];
 *   wire: NULL, or [S][av_wire_table_bytes(tcap)] -- every stream's table in the all-gather's wire format (av_pack_tracks with
 *   n_sel = 1), written by the same launch (needs snap); header.stream = stream0 + s, header.frame = frame0 + frame_count[s]
 *   after the step (the stream's own detector frame count, read on the device: a captured graph stamps every replay correctly).
 * Built for tcap 64, dcap 7..8, iou_threshold > 0 (AV_EINVAL otherwise: use the stage calls). */
typedef struct av_step_set {
    int32_t *det_n, *det_box, *det_cls;
    double* det_conf;
    av_track_row* snap;
    int32_t *snap_n, *det2trk;
    const double* z;
    double *vstate, *plan_state, *waypoints, *cost;
    int32_t* order;
} av_step_set;
typedef struct av_step_loop {
    av_tracker_cfg tracker_cfg;
    av_kf_cfg kf_cfg;
    int32_t n_streams, h, w, dcap, tcap, reserved;      /* (reserved: the pointers start 8-byte aligned) */
    int32_t* frame_count;
    int32_t* det_status;
    void* tracker_state;
    double* kf_state;
} av_step_loop;
int av_hot_step(av_ctx* ctx, av_stream_t stream, const av_step_loop* loop, const av_step_set* set, void* wire, int stream0,
                int frame0);
/* AV_OK when the one-launch step can run n_streams streams with the planner configured now and `depth` launches in flight (1 for
 * av_hot_step, D for av_hot_step_seq); AV_EINVAL where it cannot (the planner's per-wave tiles do not fit the LDS even with eight
 * waves per workgroup, e.g. 126 waypoints at 21 candidates), and the caller keeps the four stage calls. */
int av_hot_step_fits(av_ctx* ctx, int n_streams, int dcap, int tcap, int depth);
/* The launch shape av_hot_step_fits decides on, under the same conditions and with the same return codes: waves per workgroup of
 * the step kernel (16, 12 or 8: sixteen where `depth` launches of 2 S sixteen-wave workgroups are all resident, else twelve, else
 * eight; AVHOT_STEP_PW=8|12|16 forces one), the workgroups per CU the occupancy query answered for that kernel (0 at depth 1, where
 * it is not asked) and the dynamic LDS bytes of a launch.  Any of the three pointers may be NULL.  Launches nothing. */
int av_hot_step_plan(av_ctx* ctx, int n_streams, int dcap, int tcap, int depth, int* waves, int* per_cu, size_t* lds_bytes);

/* Consecutive time-steps OVERLAPPED (still one launch per step, same results bit for bit).  The reference's loop runs frame t + 1
 * after frame t (demo.py:97-120); what frame t + 1 needs of frame t is the stream's tracker table (tracker role) and its filter
 * state (Kalman role), not the planner's output.  The caller launches step `seq` (0, 1, 2, ... since the state was reset) on HIP
 * stream seq % D of D = 2 .. 4 streams -- so that step seq + D follows step seq in stream order -- and gives the D steps that may
 * be in flight DIFFERENT per-step buffers (an av_step_set each, and a wire buffer each); the av_step_loop -- the persistent
 * buffers (frame_count, det_status, tracker_state, kf_state) -- and seq_flags are shared.  On the device a role of step `seq` waits
 * until seq_flags says its stream's role of step seq - 1 has finished and published its state:
 *   seq_flags  int32 [AV_STEP_FLAG_INTS(S)], set up when the state is reset: [32 (2 s + r)] = 0, the steps done by role r (0 tracker,
 *              1 Kalman) of stream s, a 128-byte line each; [64 S] = 0, the fault word -- bit 0: a workgroup's wait ran out
 *              (AVHOT_STEP_SPIN polls, default 2^22: a predecessor that was never launched) and it left without running its step,
 *              bit 1: frame_count[s] was not base + seq; check it after synchronising; [64 S + 32 + s] = frame_count[s] at the
 *              reset (the detections of step seq are made for frame count base + seq + 1 without waiting for step seq - 1);
 *              the last 64 ints (at an even word -- one word of padding in front of them for odd S -- so that seq_flags has to be 8-byte
 *              aligned): phase clocks summed by the kernel when AVHOT_STEP_FENCE=8 (tools/steptime.py), otherwise unused.  (For odd S
 *              this is one word more than the earlier 65 S + 96: a caller that still allocates that is only overrun with
 *              AVHOT_STEP_FENCE=8 set.)
 * Step numbers are 32-bit and wrap (a signed int carrying an unsigned count: 2^31 - 1 is followed by -2^31, -1 by 0); the stream and
 * buffer set of step seq are those of (uint32_t)seq % D.
 * `depth` = D: up to D launches may be in flight, each possibly waiting for the one before it, so all of them must be RESIDENT
 * together: the call picks sixteen, twelve or eight waves per workgroup accordingly (av_hot_step_plan says which) and returns
 * AV_EINVAL when D launches of 2 S workgroups cannot fit (64 streams: D <= 2 with sixteen waves, <= 4 with twelve or eight).
 * HotLoop(window=1, overlap=D) drives it. */
#define AV_STEP_FLAG_INTS(n_streams) (65 * (n_streams) + ((n_streams) & 1) + 32 + 64)
#define AV_STEP_MAX_DEPTH 4
int av_hot_step_seq(av_ctx* ctx, av_stream_t stream, const av_step_loop* loop, const av_step_set* set, void* wire, int stream0,
                    int frame0, int32_t* seq_flags, int seq, int depth);

/* n_steps consecutive overlapped steps (seq0, seq0 + 1, ...) enqueued by ONE call: the launch loop of av_hot_step_seq in C (a Python
 * caller spends 8 us per launch, the device 6-7), with `depth` (2 .. AV_STEP_MAX_DEPTH) steps in flight: step q runs on
 * streams[q % depth] and writes sets[q % depth], so after the call the sets hold the outputs of the last `depth` steps.  All launches
 * in flight have to fit on the device together (depth * 2 S workgroups, two per CU): AV_EINVAL otherwise.
 *   z_steps     NULL (every step reads its set's z), or [n_steps][S][4]: the measurements of step seq0 + i at z_steps + i * S * 4
 *   wire_steps  NULL, or [n_steps][S][av_wire_table_bytes(tcap)]: every step's wire tables (the per-frame all-gather's payload) */
int av_hot_steps_seq(av_ctx* ctx, int depth, const av_stream_t* streams, const av_step_loop* loop, const av_step_set* sets,
                     const double* z_steps, void* wire_steps, int stream0, int frame0, int32_t* seq_flags, int seq0, int n_steps);

/* ---- Ground odometry (opt-in): the ego measurement of av_kf_step from the road pixels of two consecutive frames -----------------
 * The reference synthesises z = [x, y, vx, vy] on the host (video_loader.py:166-205: generate_ego_motion); recorded video has no
 * such array.  Four stages, each an entry of its own, and av_egoflow_update, which enqueues all four for a loop.
 *
 * Geometry: a gray bird's-eye patch uint8 [gh][gw] per camera, av_ground_warp's: pixel (r, c) shows the road point
 *   f = f_far - ((double)r + 0.5) * m_per_px;   l = (((double)c + 0.5) - (double)gw / 2.0) * m_per_px
 * Tiles of T x T pixels (T = tile) with a search range of R pixels (R = search): tile (ty, tx) has its first pixel at
 *   y0 = R + ty * T, x0 = R + tx * T;   tiles_y = (gh - 2 R) / T, tiles_x = (gw - 2 R) / T (integer division),
 *   n_tiles = tiles_y * tiles_x, tile index = ty * tiles_x + tx; its centre is the road point
 *   f = f_far - ((double)y0 + (double)T / 2.0) * m_per_px;   l = (((double)x0 + (double)T / 2.0) - (double)gw / 2.0) * m_per_px
 * Checked by every entry (AV_EINVAL, before any launch): gh, gw in 1 .. 4096; T a multiple of 4, 4 <= T <= 32; 1 <= R <= 15; at least one
 * tile fits (tiles_y, tiles_x >= 1) and n_tiles <= 65535; m_per_px > 0 and finite, f_far finite; frame_rate > 0 and finite;
 * min_texture >= 0; 0 <= gate_px <= 2 R; inlier_px > 0 and finite; min_inliers >= 1; n_cams in 1 .. 65535. */
typedef struct {
    int32_t gh, gw;            /* patch rows, columns (256, 256) */
    int32_t tile, search;      /* T (16), R (12) */
    double f_far, m_per_px;    /* row 0's far edge in metres ahead; metres per patch pixel (0.1) */
    double frame_rate;         /* frames / s (30): z's velocity = displacement * frame_rate */
    int32_t min_texture;       /* a tile with less texture is not accepted (2 T T) */
    int32_t gate_px;           /* the vote's gate (3) */
    double inlier_px;          /* residual limit of the fit, patch pixels (1.0) */
    int32_t min_inliers;       /* fewer inliers: not valid (8) */
    int32_t reserved;          /* 0 */
} av_egoflow_cfg;              /* 64 bytes */

/* One row per tile.  flags bit 0: accepted (match), bit 1: live (match), bit 2: inside the vote's gate (solve), bit 3: inlier of the
 * final fit (solve).  A tile that is not live has every other field of the match 0 except f, l. */
#define AV_EGOFLOW_ACCEPTED 1
#define AV_EGOFLOW_LIVE 2
#define AV_EGOFLOW_GATED 4
#define AV_EGOFLOW_INLIER 8
typedef struct {
    int32_t flags;
    int32_t dy, dx;            /* the best candidate, patch pixels */
    int32_t sad;               /* its sum of absolute differences */
    int32_t texture;
    int32_t reserved;          /* 0 */
    double sub_dy, sub_dx;     /* sub-pixel offsets to add to dy, dx; in [-0.5, 0.5], 0 where not defined */
    double f, l;               /* the tile's centre, metres */
} av_egoflow_tile;             /* 56 bytes */

typedef struct {
    double t_f, t_l, omega;    /* the camera's motion between the two frames in the PREVIOUS frame's road frame: metres, radians */
    double rms;                /* of the inliers' residuals, metres */
    int32_t n_accepted, n_gated, n_inliers, valid;
    int32_t vote_dy, vote_dx;  /* the vote's mode (0, 0 where no tile is accepted) */
    int32_t reserved[2];
} av_egoflow_motion;           /* 64 bytes */

/* Persistent per-camera state (device; settable from the host between calls): the pose of the camera's ground point in the world
 * and the number of frames seen since the reset.  All zero = reset. */
typedef struct {
    double x, y, psi;
    int32_t frames, reserved;
} av_egoflow_state;            /* 32 bytes */

int av_egoflow_tiles(const av_egoflow_cfg* cfg, int* tiles_y, int* tiles_x);   /* host only: the checks above and the tile grid */

/* Stage 1, patch: per patch pixel the road point as above, then through ground[k].ginv exactly av_ground_warp's position rule (U, V,
 * D, u, v, tu, tv and its two refusals) and its bilinear sample (b, g, r); then the lane front end's gray
 *   gray = (1868 b + 9617 g + 4899 r + 8192) >> 14
 * A pixel the position rule refuses is INVALID: its gray is 0 and its validity bit is 0.
 *   ground DEVICE [n_cams]; bgr [n_cams][h][w][3] RECTIFIED frames; patch [n_cams][gh][gw];
 *   valid uint32 [n_cams][gh][vw], vw = (gw + 31) / 32: bit (c & 31) of word c >> 5 is pixel (r, c)'s; bits at c >= gw are 0 */
int av_egoflow_patch(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, const av_ground_cfg* ground, int n_cams, int h,
                     int w, const uint8_t* bgr, uint8_t* patch, uint32_t* valid);

/* Stage 2, match (the hot kernel): cur, prev [n_cams][gh][gw] gray patches (any bytes: hand-made ones are fine), valid as above,
 * tiles [n_cams][n_tiles].  Per tile, integers throughout:
 *   live     = every pixel of rows y0 - R .. y0 + T + R - 1, columns x0 - R .. x0 + T + R - 1 is valid
 *   SAD(dy, dx) = sum over i, j in 0 .. T-1 of |cur[y0+i][x0+j] - prev[y0+dy+i][x0+dx+j]|,   dy, dx in -R .. R
 *   best     = the smallest SAD; among equals the first in row-major (dy, dx) order (dy = -R first, then dx = -R first)
 *   texture  = sum over i in 0 .. T-1, j in 0 .. T-2 of |cur[y0+i][x0+j] - cur[y0+i][x0+j+1]|
 *            + sum over i in 0 .. T-2, j in 0 .. T-1 of |cur[y0+i][x0+j] - cur[y0+i+1][x0+j]|
 *   accepted = live && texture >= min_texture && |dy| < R && |dx| < R
 *   sub-pixel, per axis, only where the best is not on that axis's border (|d| < R; else 0), float64:
 *     sm = SAD at d - 1, s0 = the best SAD, sp = SAD at d + 1 (the other axis at the best);
 *     den = (double)(sm - 2 s0 + sp) * 2.0;   sub = den > 0 ? (double)(sm - sp) / den : 0
 * So the road texture under cur's pixel (y, x) was under prev's pixel (y + dy + sub_dy, x + dx + sub_dx). */
int av_egoflow_match(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_cams, const uint8_t* cur, const uint8_t* prev,
                     const uint32_t* valid, av_egoflow_tile* tiles);

/* Stage 3, solve: one wave per camera; reads the match's fields of tiles, sets flag bits 2 and 3, writes motion [n_cams].
 *   vote: the histogram of the ACCEPTED tiles' (dy, dx); the mode (my, mx) is the fullest bin, among equals the first in row-major
 *         (dy, dx) order.  No accepted tile: motion all 0.
 *   gate: gated = accepted && |dy - my| <= gate_px && |dx - mx| <= gate_px
 *   a tile's displacement in metres (the road point seen at p = (f, l) now was at p + d in the previous frame's road frame):
 *         d_f = -((double)dy + sub_dy) * m_per_px;   d_l = ((double)dx + sub_dx) * m_per_px
 *   fit over a set of tiles, the small-angle rigid motion d = t + omega J p, J p = (-l, f), float64:
 *         n = the count; Sf = sum f; Sl = sum l; Q = sum (f f + l l); B1 = sum d_f; B2 = sum d_l; B3 = sum (f d_l - l d_f)
 *         (each lane sums its own tiles in index order, then a fixed tree over the 64 lanes: sums may differ from a sequential
 *         sum in the last bits)
 *         elimination, t first: den = (Q - (Sl Sl) / n) - (Sf Sf) / n;   singular unless n >= 1 and den > 1e-9 * Q   (the pivot test)
 *         omega = ((B3 + (Sl B1) / n) - (Sf B2) / n) / den;   t_f = (B1 + omega Sl) / n;   t_l = (B2 - omega Sf) / n
 *   first fit over the gated tiles; residual r_f = d_f - (t_f - omega l), r_l = d_l - (t_l + omega f);
 *   inlier = gated && !(r_f r_f + r_l r_l > (inlier_px m_per_px)^2);  second fit over the inliers: t_f, t_l, omega;
 *   rms = sqrt(sum over the inliers of the second fit's (r_f r_f + r_l r_l) / n_inliers)
 *   valid = neither fit singular && n_inliers >= min_inliers.  A singular first fit: no inliers, t_f = t_l = omega = rms = 0; a
 *   singular second fit leaves them 0 too. */
int av_egoflow_solve(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_cams, av_egoflow_tile* tiles,
                     av_egoflow_motion* motion);

/* Stage 4, measure: state [n_cams] is advanced, z [n_cams][4] and mode [n_cams] are what av_kf_step reads (window 1).
 *   use = motion.valid && state.frames >= 1       (the first frame after a reset has no predecessor)
 *   use: c = cos(psi), s = sin(psi);  Dx = t_f c - t_l s;  Dy = t_f s + t_l c;  x += Dx;  y += Dy;  psi += omega;
 *        z = [x, y, Dx * frame_rate, Dy * frame_rate];  mode = 1
 *   else: the pose stays;  z = [x, y, 0, 0];  mode = 2 (the filter predicts)
 *   frames += 1 either way. */
int av_egoflow_measure(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_cams, const av_egoflow_motion* motion,
                       av_egoflow_state* state, double* z, uint8_t* mode);

/* All four stages, enqueued on `stream`; no allocation, no host round trip.  patches [n_cams][2][gh][gw] is the ping-pong pair:
 * frame number state[k].frames of camera k is written to slot frames & 1 and matched against the other slot (on the first frame
 * that slot holds whatever it held; the measure stage ignores the outcome).  valid, tiles, motion as in the stages. */
int av_egoflow_update(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, const av_ground_cfg* ground, int n_cams, int h,
                      int w, const uint8_t* bgr, uint8_t* patches, uint32_t* valid, av_egoflow_tile* tiles, av_egoflow_motion* motion,
                      av_egoflow_state* state, double* z, uint8_t* mode);

/* ---- Rig odometry (opt-in): a vehicle's ego motion from the road pixels of all K cameras of its rig ------------------------------
 * The patch and match stages are av_egoflow_patch and av_egoflow_match over V * K cameras (camera k of vehicle v is camera
 * v * K + k, as in av_rig_fuse).  The solve below fits every camera's tiles together in the VEHICLE frame: a wide baseline for the
 * yaw, the motion of the vehicle's origin rather than of a camera's ground point (the lever arm falls out of the algebra), a
 * measurement when no single camera has enough tiles, and a camera whose whole patch shows another vehicle is dropped.
 *
 * av_rig_egoflow_solve: one workgroup per vehicle, one wave per camera; reads the match's fields of tiles [V*K][n_tiles], sets flag
 * bits 2 and 3, writes motion [V] and info [V].  float64, every operation rounded on its own (no FMA), in the order written.
 *   1. vote and gate, per camera: exactly av_egoflow_solve's vote, mode and gate on that camera's table, its "accepted" included
 *      (the (dy, dx) of cameras with different yaws cannot share a histogram).  Bit 2 on the gated tiles; info.cam_accepted[k],
 *      cam_gated[k], cam_vote_dy[k], cam_vote_dx[k].
 *   2. rows in the vehicle frame: a gated tile with centre (f, l) and av_egoflow_solve's displacement (d_f, d_l) under the mount
 *      (c, s, mx, my) of its camera, as av_rig_fuse writes it:
 *        X = (mx + c*f) - s*l;   Y = (my + s*f) + c*l;   DX = c*d_f - s*d_l;   DY = s*d_f + c*d_l
 *      The model is D = T + Omega J P, the camera's small-angle form: with d = t + omega J p in the camera's frame and
 *      P = M + R p, D = R d, it gives T = R t - omega J M and Omega = omega.
 *   3. fit(set): av_egoflow_solve's fit with (X, Y, DX, DY) for (f, l, d_f, d_l) and the same pivot test.  Each camera's sums as
 *      there (per lane in tile order, then the wave's fixed tree); the cameras' sums added in the order k = 0 .. K - 1.
 *   4. hypotheses: h_0 = fit(all gated rows of the vehicle), h_(1+k) = fit(camera k's gated rows); singular ones are dropped.
 *      count_i = the number of the vehicle's gated rows with !(r_X r_X + r_Y r_Y > (inlier_px m_per_px)^2) under h_i, where
 *      r_X = DX - (T_f - Omega Y), r_Y = DY - (T_l + Omega X).  info.hyp_count[i] = count_i, or -1 where h_i was dropped or is
 *      absent (i > K).  The best hypothesis has the largest count, among equals the smallest i: info.hypothesis.  None regular:
 *      motion all 0 except n_accepted and n_gated, info.hypothesis = -1, no bit 3.
 *   5. final fit: inliers = the gated rows within the limit under the best hypothesis (bit 3); info.cam_inliers[k]; info.views
 *      has bit k set when camera k has at least one inlier.  B = fit(inliers): t_f, t_l, omega (the motion of the vehicle's origin
 *      in the previous frame's VEHICLE frame); rms over the inliers under B (the cameras' sums of squares added in the order
 *      k = 0 .. K - 1); n_inliers the count; valid = B regular && n_inliers >= min_inliers.  B singular: t_f = t_l = omega = rms = 0.
 *      n_accepted and n_gated are the cameras' sums; vote_dy = vote_dx = 0.
 * With K = 1 and the identity mount (1, 0, 0, 0) this is av_egoflow_solve step for step: X = f and DX = d_f exactly, h_0 = h_1.
 *   mounts DEVICE [V][K]; tiles [V*K][n_tiles]; motion [V]; info [V]
 * AV_EINVAL before any launch: a null pointer; n_vehicles < 1; n_cams not in 1 .. 8; n_vehicles * n_cams > 65535; a cfg that
 * av_egoflow_tiles refuses. */
typedef struct {
    int32_t hypothesis;        /* the best hypothesis: 0 pooled, 1 + k camera k's, -1 none regular */
    int32_t views;             /* bit k: camera k has an inlier */
    int32_t reserved[2];       /* 0 */
    int32_t cam_accepted[8], cam_gated[8], cam_inliers[8];     /* per camera; 0 at k >= K */
    int32_t cam_vote_dy[8], cam_vote_dx[8];                    /* every camera's own mode; 0 at k >= K */
    int32_t hyp_count[9];      /* count_i; -1: dropped or absent */
    int32_t pad;               /* 0 */
} av_rig_egoflow_info;         /* 216 bytes */
#ifdef __cplusplus
static_assert(sizeof(av_rig_egoflow_info) == 216, "av_rig_egoflow_info is 54 int32");
#else
_Static_assert(sizeof(av_rig_egoflow_info) == 216, "av_rig_egoflow_info is 54 int32");
#endif
int av_rig_egoflow_solve(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_vehicles, int n_cams,
                         const av_rig_mount* mounts, av_egoflow_tile* tiles, av_egoflow_motion* motion, av_rig_egoflow_info* info);

/* av_egoflow_update for a rig, enqueued on `stream`; no allocation, no host round trip: the patch and match stages over the V * K
 * cameras, av_rig_egoflow_solve, and av_egoflow_measure's stage over the V vehicles.  state [V], z [V][4] and mode [V] are the
 * VEHICLE's: the pose is that of the vehicle's origin.  patches [V*K][2][gh][gw] is the ping-pong pair; every camera's slot follows
 * its vehicle's frame counter, state[cam / K].frames & 1.  ground DEVICE [V*K], bgr [V*K][h][w][3] RECTIFIED frames, valid
 * [V*K][gh][vw], tiles [V*K][n_tiles], motion [V], info [V].  The solve's checks, and h, w >= 1. */
int av_rig_egoflow_update(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, const av_ground_cfg* ground,
                          const av_rig_mount* mounts, int n_vehicles, int n_cams, int h, int w, const uint8_t* bgr, uint8_t* patches,
                          uint32_t* valid, av_egoflow_tile* tiles, av_egoflow_motion* motion, av_rig_egoflow_info* info,
                          av_egoflow_state* state, double* z, uint8_t* mode);

/* ---- Road memory (opt-in): the surround panel's unseen pixels from earlier frames, through the measured pose --------------------
 * av_rig_surround stitches what the cameras see NOW; where none looks (under the vehicle, beside its sills) the panel has a hole.
 * The road there was in view some frames ago.  Per vehicle a WORLD-anchored rolling canvas takes every frame's seen panel pixels
 * through the pose the odometry integrated (av_egoflow_state), and the panel's unseen pixels are read back out of it: a pixel is
 * resampled exactly twice, whatever its age.  Three stages, each an entry of its own, and av_roadmem_step, which enqueues all
 * three.  All positions float64, every operation rounded on its own (no FMA), in the order written.
 *
 * World cells of pitch m = cfg.m_per_px: cell (i, j), i and j integers of either sign, has its centre at
 *   xc = ((double)i + 0.5) * m;   yc = ((double)j + 0.5) * m
 * Canvas, per vehicle: canvas uint8 [V][N][N][4] (b, g, r, 0: a cell is one aligned 32-bit word) and stamp uint32 [V][N][N]
 * (0: never seen; else the vehicle's frame counter when the cell was last written).  Cell (i, j) lives at [i mod N][j mod N], the
 * mathematical (non-negative) mod.  The window of a vehicle is i in i0 .. i0 + N - 1, j in j0 .. j0 + N - 1, with
 *   i0 = (int32)floor(x / m) - N / 2;   j0 = (int32)floor(y / m) - N / 2          (x, y: the pose of this frame)
 * The panel is av_rig_surround's: gh x gw pixels of pm = cfg.panel_m_per_px metres, row 0 at x_far metres ahead. */
typedef struct {
    int32_t n;                 /* N: a multiple of 16 in 16 .. 4096 */
    int32_t max_age;           /* a cell older than this many frames is not read back; >= 0 */
    double m_per_px;           /* the cells' pitch m, metres; > 0, finite */
    int32_t gh, gw;            /* the panel's rows and columns; >= 1 */
    double x_far;              /* the panel's x_far; finite */
    double panel_m_per_px;     /* the panel's pitch pm; > 0, finite */
    uint8_t fill[3];           /* b, g, r of an unseen pixel that is not remembered */
    uint8_t reserved[5];       /* 0 */
} av_roadmem_cfg;              /* 48 bytes */
/* Persistent per-vehicle state (device): the window's origin, the frame counter F and the status.  All zero = reset.  status bit 0:
 * the pose was out of range on the last frame: !(|x / m| <= 2^30 && |y / m| <= 2^30), a NaN among them.  Such a frame is a reset:
 * nothing is written to canvas or stamp, and the state becomes {0, 0, 0, 1}. */
typedef struct {
    int32_t i0, j0, frames, status;
} av_roadmem_state;            /* 16 bytes */
typedef struct {
    double x, y, cs, sn;       /* the vehicle origin's place in the world, cos and sin of its heading */
    int32_t reset, reserved;   /* reset != 0: what the canvas holds no longer lies where the pose says */
} av_roadmem_pose;             /* 40 bytes */

/* Host only.  AV_EINVAL for a null cfg, n not a multiple of 16 in 16 .. 4096, max_age < 0, m_per_px or panel_m_per_px not > 0 and
 * finite, x_far not finite, gh or gw < 1, a reserved byte not 0.  Every device entry below makes these checks before any launch and
 * before the context is looked at, and refuses a null pointer other than stream (and mode), n_vehicles outside 1 .. 65535, and a
 * panel that shares a byte with canvas or stamp. */
int av_roadmem_check(const av_roadmem_cfg* cfg);

/* Stage 1, pose: pose[v] = {x, y copied from state[v]; cs = cos(psi); sn = sin(psi); reset = (mode != NULL && mode[v] == 2); 0}.
 * The frame on which the odometry measured nothing (av_egoflow_measure's mode 2, the first frame among them) is a reset: the
 * integrated pose did not follow the vehicle over it.  The only transcendental calls of the road memory are here; the pixel stages
 * take (x, y, cs, sn) as given, the way av_rig_surround takes the mounts'.
 *   state [V] (the odometry's, read), mode [V] or NULL, pose [V] */
int av_roadmem_pose_from(av_ctx* ctx, av_stream_t stream, int n_vehicles, const av_egoflow_state* state, const uint8_t* mode,
                         av_roadmem_pose* pose);

/* Stage 2, update (the hot kernel).  Per vehicle, with the state {i0, j0, frames, status} of the previous frame and this frame's
 * pose: out of range (above): state = {0, 0, 0, 1}, nothing else.  Otherwise
 *   fresh = reset || frames == 0;   F = fresh ? 1 : frames + 1;   (i0n, j0n) = the window's origin from the pose
 * and for every cell (i, j) of the NEW window:
 *   1 entered = fresh || i < i0 || i >= i0 + N || j < j0 || j >= j0 + N        (the OLD origin); entered: stamp = 0
 *   2 dx = xc - x;  dy = yc - y;  X = cs*dx + sn*dy;  Y = cs*dy - sn*dx             (av_rig_surround's mount order)
 *   3 pr = (x_far - X) / pm - 0.5;  pc = Y / pm + (double)gw / 2.0 - 0.5;  tr = floor(pr * 65536.0 + 0.5);  tc likewise
 *     inside = 0 <= tr <= (gh-1) * 65536 && 0 <= tc <= (gw-1) * 65536               (a NaN fails)
 *   4 r0 = tr >> 16, wr = tr & 65535, r1 = min(r0 + 1, gh - 1); c0, wc, c1 likewise
 *     seen = inside && cover[r0][c0] != 0 && cover[r0][c1] != 0 && cover[r1][c0] != 0 && cover[r1][c1] != 0
 *   5 seen: each channel av_ground_warp's bilinear rule on the four panel taps,
 *       ((p00 (65536-wc) + p01 wc)(65536-wr) + (p10 (65536-wc) + p11 wc) wr + 2^31) >> 32,
 *     byte 3 = 0, stamp = F (a cell that entered and is seen on the same frame ends with F).  Not seen: the colour stays.
 * then state = {i0n, j0n, F, 0}.
 *   pose [V]; panel [V][gh][gw][3]: the stitched panel BEFORE any fill, read; cover [V][gh][gw], read; state [V]; canvas; stamp
 * The counter is 32 bits: a vehicle is reset before 2^31 frames. */
int av_roadmem_update(av_ctx* ctx, av_stream_t stream, const av_roadmem_cfg* cfg, int n_vehicles, const av_roadmem_pose* pose,
                      const uint8_t* panel, const uint8_t* cover, av_roadmem_state* state, uint8_t* canvas, uint32_t* stamp);

/* Stage 3, fill: the state is the one av_roadmem_update left for this frame (i0, j0, F = frames), the pose the same.  For every
 * panel pixel (r, c):
 *   cover != 0: age = 0, the pixel is not touched.
 *   cover == 0:
 *   1 X = x_far - ((double)r + 0.5) * pm;   Y = (((double)c + 0.5) - (double)gw / 2.0) * pm         (av_rig_surround's)
 *   2 xw = (x + cs*X) - sn*Y;   yw = (y + sn*X) + cs*Y
 *   3 ti = floor((xw / m - 0.5) * 65536.0 + 0.5);  tj likewise from yw;  ia = ti >> 16 (arithmetic, of a 64-bit integer: the floor
 *     for negatives), wi = ti & 65535;  ja, wj likewise
 *   4 remembered = F != 0 && ia >= i0 && ia + 1 < i0 + N && ja >= j0 && ja + 1 < j0 + N    (tested on ti, tj as doubles: a NaN or a
 *       position outside 64 bits fails) && the four cells (ia | ia + 1, ja | ja + 1) have stamp != 0
 *       && F - min(stamp) <= max_age
 *   5 remembered: each channel the bilinear rule above on the four cells, weights wj across and wi down;
 *       age = min(F - min(stamp), 254)
 *   6 else: the pixel becomes fill, age = 255
 *   panel [V][gh][gw][3] in place; age [V][gh][gw].  Also AV_EINVAL: ceil(gh / 16) above 65535 (av_rig_surround's tile mapping). */
int av_roadmem_fill(av_ctx* ctx, av_stream_t stream, const av_roadmem_cfg* cfg, int n_vehicles, const av_roadmem_pose* pose,
                    const av_roadmem_state* state, const uint8_t* canvas, const uint32_t* stamp, const uint8_t* cover, uint8_t* panel,
                    uint8_t* age);

/* Stages 1 - 3 enqueued on `stream`; no allocation, no host round trip.  ego_state [V] and mode [V] (or NULL) are the odometry's
 * (av_rig_egoflow_update's or av_egoflow_update's state and mode), pose [V] is written and then read. */
int av_roadmem_step(av_ctx* ctx, av_stream_t stream, const av_roadmem_cfg* cfg, int n_vehicles, const av_egoflow_state* ego_state,
                    const uint8_t* mode, av_roadmem_pose* pose, uint8_t* panel, const uint8_t* cover, av_roadmem_state* state,
                    uint8_t* canvas, uint32_t* stamp, uint8_t* age);
/* Zeroes the state of vehicle `vehicle` (0 .. n_vehicles - 1), or of every vehicle with -1: one hipMemsetAsync on `stream`.  The
 * canvas needs no clearing: after a reset every cell enters. */
int av_roadmem_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int vehicle, av_roadmem_state* state);

/* ---- Road lanes (opt-in): the lane boundaries in metres from the Hough segments of all K cameras of a rig ------------------------
 * Every camera's lane chain leaves its Hough segments in the lane workspace (AV_LANE_VIEW_SEGMENTS / _NSEG).  av_road_lanes carries
 * them onto the road and through the mounts into the VEHICLE frame (av_rig_fuse's: X forward, Y lateral, positive towards image
 * right), pools them over the cameras, finds the lane boundaries Y = a0 + a1 X + a2 X^2 there by two votes and a gated refit,
 * picks the ego lane, follows it from frame to frame through the measured ego motion and writes the planner's reference path and
 * the maneuver tagger's offset; no host round trip.  One workgroup per vehicle, one wave per camera.  float64, every operation
 * rounded on its own (no FMA), in the order written; model(a, X) = (a0 + a1*X) + a2*(X*X).
 *
 * Sums: a "sum over the rows" below is taken per lane (lane = i & 63 of the row index i, rows of a lane in ascending i, starting
 * from the first term), then over the 64 lanes of the camera's wave by the fixed tree of av_egoflow_solve (adjacent pairs, six
 * levels; a lane without a term holds 0.0), then over the cameras in the order k = 0 .. K - 1 starting from camera 0's sum. */
typedef struct {
    double min_len;            /* 0.5   m: a shorter segment is no row */
    double slope_max;          /* 0.5:  |dY| <= slope_max dX */
    double vote_len;           /* 0.25  m per vote */
    double x_vote;             /* 15    m: the rows that vote have Xm <= x_vote */
    double slope_tol;          /* 0.15 */
    double y_max;              /* 8     m: the offset histogram covers [-y_max, y_max) */
    double min_sep;            /* 2.0   m between accepted offset peaks */
    double gate;               /* 0.4   m */
    double span_quad;          /* 10    m: the X extent from which a boundary is fitted as a quadratic */
    double w_min, w_max;       /* 2.5, 5.0 m: a lane's width */
    double default_width;      /* 3.5   m */
    double alpha;              /* 0.7:  the weight of the prediction in the smoothed fit */
    double jump;               /* 1.0   m */
    double path_near, path_far;/* 2, 40 m */
    int32_t min_votes;         /* 16 */
    int32_t max_coast;         /* 10 frames */
    int32_t one_sided;         /* 1: a lone side gives the other at the last width */
    int32_t n_points;          /* 50; 2 .. 64 */
} av_road_lanes_cfg;           /* 144 bytes */
#define AV_ROAD_LANES_MAX_BOUNDS 8
#define AV_ROAD_BOUND_QUAD 1       /* av_road_lane_bound.flags: the last fit was quadratic */
#define AV_ROAD_BOUND_KEPT 2       /* in some round the fit was singular or the boundary had no member: it kept its model */
#define AV_ROAD_BOUND_LEFT 4       /* the ego lane's measured left boundary */
#define AV_ROAD_BOUND_RIGHT 8      /* the ego lane's measured right boundary */
typedef struct {
    double a0, a1, a2;
    double x_min, x_max;       /* of its members' end points */
    double length;             /* the members' summed length, metres */
    int32_t n_members;
    int32_t views;             /* bit k: camera k contributed a member */
    int32_t flags;
    int32_t reserved;          /* 0 */
} av_road_lane_bound;          /* 64 bytes */
#define AV_ROAD_LANE 1             /* av_road_lanes_row.status: there is a lane (both sides) */
#define AV_ROAD_ONE_SIDED 2        /* one side is the other shifted by the width */
#define AV_ROAD_COAST_LEFT 4       /* the left side is its prediction */
#define AV_ROAD_COAST_RIGHT 8
#define AV_ROAD_CHANGE_LEFT 16     /* both sides jumped towards -Y by a lane's width */
#define AV_ROAD_CHANGE_RIGHT 32
#define AV_ROAD_NO_VOTER 64        /* the frame had no voter: no measurement */
typedef struct {
    double left[3], right[3], centre[3];
    double width;
    double lane_offset;        /* -centre[0]; NaN without a lane */
    double heading;            /* -atan(centre[1]) */
    double curvature;          /* (2 centre[2]) / (q sqrt(q)), q = 1 + centre[1]^2 */
    int32_t n_bounds, lane_count, lane_index, views, status, reserved;
} av_road_lanes_row;           /* 128 bytes */
typedef struct {
    int32_t cam_rows[8];       /* rows per camera; 0 at k >= K */
    int32_t n_over;            /* segments beyond scap */
    int32_t n_off;             /* segments with an end point not on_road */
    int32_t n_short;           /* on the road, shorter than min_len */
    int32_t n_steep;           /* long enough, dX == 0 or |dY| > slope_max dX */
    int32_t n_voters;          /* rows with Xm <= x_vote */
    int32_t dir_bin;           /* the direction vote's peak, -1 without a voter */
    int32_t n_cand;            /* the offset vote's candidate peaks */
    int32_t n_peaks;           /* ... accepted (<= 8) */
    double m_star;             /* 0 without a voter */
} av_road_lanes_info;          /* 72 bytes */
/* Persistent per-vehicle state (device).  All zero = reset. */
typedef struct {
    double left[3], right[3];  /* the smoothed polynomials */
    double width;              /* the last smoothed width of a measured pair */
    double xmax_left, xmax_right;
    int32_t has_left, has_right, miss_left, miss_right, has_width, frames;
} av_road_lanes_state;         /* 96 bytes */

/* The stage per vehicle v, camera k of it being list v * n_cams + k (ground, segments, nseg) with the mount mounts[v][k]:
 * 1 rows.  n = clamp(nseg, 0, max_segments); camera k contributes segments i = 0 .. min(n, scap) - 1; info.n_over sums
 *   max(n - scap, 0).  A segment (x1, y1, x2, y2), int32 rectified pixels taken as doubles: both end points by av_ground_cfg's
 *   projection (f, l, on_road), then X = (mx + c*f) - s*l;  Y = (my + s*f) + c*l.  The end points are swapped when X2 < X1; then
 *     dX = X2 - X1;  dY = Y2 - Y1;  len = sqrt(dX*dX + dY*dY)
 *   not both on_road: n_off.  Else !(len >= min_len): n_short.  Else !(dX > 0 && |dY| <= slope_max*dX): n_steep.  Else a row:
 *     m = dY / dX;  Xm = (X1 + X2) * 0.5;  Ym = (Y1 + Y2) * 0.5;  w = (int)min(max(floor(len / vote_len), 1.0), 255.0)
 * 2 direction vote.  voters = rows with Xm <= x_vote.  bin_m = clamp((int)floor((m + slope_max) * (32.0 / slope_max)), 0, 63);
 *   h[bin_m] += w;  h'[i] = h[i-1] + 2 h[i] + h[i+1] (zeros outside);  the peak pm: the largest h', among equals the smallest i.
 *   m* = (sum over the voters with |bin_m - pm| <= 1 of (double)w * m) / (double)(the sum of their w).  No voter: no boundary,
 *   status bit AV_ROAD_NO_VOTER, step 6 with neither side measured.
 * 3 offset vote.  Voters with |m - m*| <= slope_tol:  b = Ym - m* * Xm;  t = (b + y_max) * (32.0 / y_max);  they vote when
 *   t >= 0 && t < 64, bin_b = (int)floor(t), with w; h' as above.  Candidates: h'[i] >= min_votes && h'[i] > h'[i-1] &&
 *   h'[i] >= h'[i+1].  Repeatedly the candidate with the largest h' (among equals the smallest i) is accepted and every candidate
 *   j with (double)|j - i| * (y_max / 32.0) < min_sep leaves, until none remains or 8 are accepted.  Boundaries p = 0 .. in
 *   ascending bin:  a0 = (sum over those voters with |bin_b - peak_p| <= 1 of (double)w * b) / (double)(sum of their w), a1 = m*,
 *   a2 = 0.
 * 4 grow and refit, rounds r = 0, 1, 2 with the range x_vote, 2.0 * x_vote, unbounded.  A row with Xm <= range (round 2: every
 *   row) is admissible for p when r1 = |Y1 - model(p, X1)| <= gate and r2 = |Y2 - model(p, X2)| <= gate; it joins the admissible
 *   p with the smallest max(r1, r2), among equals the smallest p.  Per boundary, the sums over its members, each member adding its
 *   two end points in the order 1, 2 with the weight len:
 *     S0 += len; S1 += len*X; S2 += len*(X*X); S3 += len*((X*X)*X); S4 += len*((X*X)*(X*X)); T0 += len*Y; T1 += len*(X*Y);
 *     T2 += len*((X*X)*Y)
 *   n = its members, x_min = min X1, x_max = max X2, views.  n == 0: the model stays, AV_ROAD_BOUND_KEPT.  Else, quadratic when
 *   n >= 3 && x_max - x_min >= span_quad:
 *     c11 = S2 - (S1*S1)/S0;  c12 = S3 - (S1*S2)/S0;  c22 = S4 - (S2*S2)/S0;  d1 = T1 - (S1*T0)/S0;  d2 = T2 - (S2*T0)/S0
 *     singular unless c11 > 1e-9 * S2;   e22 = c22 - (c12*c12)/c11;   singular unless e22 > 1e-9 * S4   (av_egoflow_solve's test)
 *     a2 = (d2 - (c12*d1)/c11) / e22;   a1 = (d1 - c12*a2) / c11;   a0 = ((T0 - a1*S1) - a2*S2) / S0
 *   else a line: c11, d1 and its pivot test as above;  a1 = d1 / c11;  a0 = (T0 - a1*S1) / S0;  a2 = 0.
 *   Singular: the model stays, AV_ROAD_BOUND_KEPT.  After round 2 a boundary with n == 0 is dropped, the others keep their order:
 *   bounds[v][0 .. n_bounds-1] with length = S0 * 0.5; entries at or past n_bounds are zero.
 * 5 the ego lane.  L = the boundary with the largest a0 < 0, R = the one with the smallest a0 >= 0 (among equals the smallest
 *   index).  With both and !(w_min <= a0_R - a0_L <= w_max) the farther one is not measured: R when -a0_L <= a0_R, else L.
 *   A measured side's flags take AV_ROAD_BOUND_LEFT / _RIGHT.
 * 6 following.  mv = motion != NULL && motion[v].valid != 0.  pred(a) with (t_f, t_l, omega) of motion[v] when mv:
 *     a0' = ((a0 + a1*t_f) + a2*(t_f*t_f)) - t_l;   a1' = (a1 + (2.0*a2)*t_f) - omega;   a2' = a2;   xmax' = xmax - t_f
 *   else a and xmax themselves.  Per side, left first:
 *     measured, has history: d = new_a0 - a0';  |d| <= jump: a_i = alpha*a_i' + (1.0 - alpha)*new_a_i;  else a = new, the side
 *       "jumped by d".  Measured without history: a = new.  Either way xmax = the boundary's x_max, has = 1, miss = 0.
 *     not measured, has history: miss += 1;  miss > max_coast: the side is gone (all its fields 0);  else a = a', xmax = xmax',
 *       AV_ROAD_COAST_LEFT / _RIGHT.
 *   Both measured: state.width = right a0 - left a0 (smoothed), has_width = 1.  Both jumped, both d < 0 (left) or both d > 0
 *   (right), and both |d| in [w_min, w_max]: AV_ROAD_CHANGE_LEFT / _RIGHT.  frames += 1.
 *   Exactly one side measured, the other without history after the above, and cfg.one_sided: the other side of the OUTPUT (not of
 *   the state) is the measured side's smoothed fit with a0 -/+ W (left = right - W, right = left + W), W = state.width if has_width
 *   else default_width, and its xmax; AV_ROAD_ONE_SIDED.  There is a lane (AV_ROAD_LANE) when both sides of the output exist.
 * 7 outputs.  row: left, right (zeros for a missing side), and with a lane centre_i = (left_i + right_i) * 0.5, width =
 *   right_0 - left_0, lane_offset, heading, curvature as in the struct (without: 0, lane_offset NaN); n_bounds; views = the OR of the
 *   measured sides' boundaries' views.  The chain: from a measured L the boundaries at index L-1, L-2, ... continue it while
 *   a0[j+1] - a0[j] lies in [w_min, w_max]; from a measured R likewise upwards; lane_index = the left count,
 *   lane_count = 1 + both counts with a lane, else both 0.
 *   The path: x_end = min(path_far, min(xmax_left, xmax_right));  n_ref = n_points when there is a lane and
 *   x_end - path_near >= 1.0, else 0;  step = (x_end - path_near) / (double)(n_points - 1);  X_i = path_near + (double)i*step;
 *   Y_i = model(centre, X_i), placed as av_rig_fuse places a cluster with (x0, y0, h) = plan_state[v]:
 *     ref_path[v][i] = ((x0 + X cos h) + Y cos(h + pi/2), (y0 + X sin h) + Y sin(h + pi/2));  rows at or past n_ref are not written.
 *   lane_offset[v] = row.lane_offset.  bounds [V][8], info [V], row [V], n_ref [V], lane_offset [V] are always written.
 *
 *   ground DEVICE [V*K]; mounts DEVICE [V][K]; segments int32 [V*K][max_segments][4]; nseg int32 [V*K]; motion [V] or NULL;
 *   plan_state [V][4]; state [V]; bounds [V][8]; info [V]; row [V]; ref_path [V][rcap][2]; n_ref [V]; lane_offset [V]
 * AV_EINVAL before any launch: a null pointer other than motion; n_vehicles outside 1 .. 65535; n_cams outside 1 .. 8;
 * max_segments < 1; scap outside 1 .. 256; cfg.n_points outside 2 .. min(rcap, 64); a cfg that av_road_lanes_check refuses.  The
 * arguments are checked before the context is looked at. */
/* Host only.  AV_EINVAL for a null cfg; a double not finite; min_len, vote_len, x_vote, slope_tol, y_max, min_sep, gate, span_quad,
 * w_min, default_width, jump not > 0; slope_max not in (0, 4]; w_max < w_min; alpha not in [0, 1); path_near < 0 or path_far <=
 * path_near; min_votes < 1; max_coast < 0; one_sided not 0 or 1; n_points not in 2 .. 64. */
int av_road_lanes_check(const av_road_lanes_cfg* cfg);
size_t av_road_lanes_state_bytes(void);        /* sizeof(av_road_lanes_state) */
int av_road_lanes(av_ctx* ctx, av_stream_t stream, const av_road_lanes_cfg* cfg, int n_vehicles, int n_cams,
                  const av_ground_cfg* ground, const av_rig_mount* mounts, int max_segments, int scap, const int32_t* segments,
                  const int32_t* nseg, const av_egoflow_motion* motion, const double* plan_state, av_road_lanes_state* state,
                  av_road_lane_bound* bounds, av_road_lanes_info* info, av_road_lanes_row* row, int rcap, double* ref_path,
                  int32_t* n_ref, double* lane_offset);
/* Zeroes the state of vehicle `vehicle` (0 .. n_vehicles - 1), or of every vehicle with -1: one hipMemsetAsync on `stream`. */
int av_road_lanes_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int vehicle, av_road_lanes_state* state);

/* ---- Road marks (opt-in): what each lane boundary is -- solid or dashed, white or yellow -- read from the pictures ----------------
 * av_road_lanes knows where every boundary lies; av_road_marks walks along each of them in the rectified frames of the rig's K
 * cameras and reads the paint.  Positions are float64, every operation rounded on its own (no FMA), in the order written; every
 * decision is taken in integers.  The host turns the four lengths of the settings into sample counts once:
 *   count(len) = (int)floor(len / ds + 0.5)                 (gap_solid_n, gap_dash_n, min_seen_n, min_paint_n; each 1 .. 65536) */
typedef struct {
    double x_near;             /* 4.0   m: the near edge of the first sample, ahead of the vehicle's origin */
    double ds;                 /* 0.1   m: sample spacing along X */
    double dl;                 /* 0.05  m: tap spacing across the line */
    double gap_solid;          /* 0.5   m: a boundary without a measured gap this long is solid */
    double gap_dash;           /* 1.5   m: a dashed boundary has a measured gap at least this long */
    double min_seen;           /* 8.0   m of seen samples, below which the type is unknown */
    double min_paint;          /* 2.0   m of paint samples, likewise */
    int32_t n_samples;         /* 210;  1 .. 512 */
    int32_t core;              /* 5:    taps |j| <= core belong to the marking; >= 0 */
    int32_t shoulder0;         /* 9 */
    int32_t shoulder1;         /* 13:   core < shoulder0 <= shoulder1 <= 16; taps shoulder0 <= |j| <= shoulder1 are the background */
    int32_t contrast;          /* 40    gray levels; 1 .. 255 */
    int32_t yellow_tenths;     /* 7;    0 .. 10 */
    int32_t hold;              /* 3     frames; >= 1 */
    int32_t forget;            /* 30    frames; >= 1 */
} av_road_marks_cfg;           /* 88 bytes */
#define AV_ROAD_MARKS_MAX_SAMPLES 512
#define AV_ROAD_MARK_UNKNOWN 0     /* av_road_mark.type */
#define AV_ROAD_MARK_SOLID 1
#define AV_ROAD_MARK_DASHED 2
#define AV_ROAD_MARK_WHITE 1       /* av_road_mark.colour; 0 with type UNKNOWN */
#define AV_ROAD_MARK_YELLOW 2
#define AV_ROAD_MARK_AMBIGUOUS 1   /* av_road_mark.flags: enough paint, a measured gap of gap_solid or more, and not dashed */
typedef struct {
    int32_t type, colour, flags;
    int32_t n_seen, n_paint;   /* samples */
    int32_t n_runs;            /* paint runs */
    int32_t longest_gap;       /* the longest measured gap, samples */
    int32_t n_gaps;            /* measured gaps */
    int32_t n_dashes;          /* complete paint runs */
    int32_t contrast;          /* the rounded mean of peak - bg over the paint samples; 0 without one */
    int32_t views;             /* bit k: a seen sample was read from camera k */
    int32_t reserved;          /* 0 */
    double dash_m, gap_m;      /* the mean complete run and the mean measured gap, metres; 0 without one */
} av_road_mark;                /* 64 bytes */
typedef struct {
    int32_t type, colour;      /* published */
    int32_t observed, observed_colour;     /* this frame's */
    int32_t run;               /* how many frames in a row the candidate pair has been observed */
    int32_t bound;             /* the boundary observed, -1 without one */
} av_road_marks_side;          /* 24 bytes */
typedef struct {
    av_road_marks_side left, right;
    int32_t may_change_left, may_change_right;     /* 1: the published type is dashed, 0: solid, -1: unknown */
    int32_t reserved[2];       /* 0 */
} av_road_marks_row;           /* 64 bytes */
/* Persistent per-vehicle state (device).  All zero = reset. */
typedef struct {
    int32_t type, colour;      /* published */
    int32_t cand_type, cand_colour, run;           /* the last non-UNKNOWN observation and its run length */
    int32_t since;             /* frames since the last non-UNKNOWN observation */
} av_road_marks_side_state;    /* 24 bytes */
typedef struct {
    av_road_marks_side_state left, right;
    int32_t frames;
    int32_t reserved[3];       /* 0 */
} av_road_marks_state;         /* 64 bytes */

/* The stage for vehicle v, boundary b < nb = clamp(lanes[v].n_bounds, 0, 8) with (a0, a1, a2, x_min, x_max) = bounds[v][b], camera k
 * of the vehicle being entry v * n_cams + k of mounts, ground and bgr (av_rig_surround's convention):
 * 1 per sample i = 0 .. n_samples - 1:
 *     X = x_near + ((double)i + 0.5) * ds;   Yc = (a0 + a1*X) + a2*(X*X);   tap j = -shoulder1 .. shoulder1:  Y_j = Yc + (double)j * dl
 *   A tap in camera k, with the mount (cs, sn, mx, my), q = ground.ginv: av_rig_surround's
 *     dx = X - mx;  dy = Y_j - my;  f = cs*dx + sn*dy;  l = cs*dy - sn*dx
 *   and av_ground_warp's U, V, D, u, v, tu, tv for the road point (f, l); it PASSES when D > 0 && 0 <= tu <= (w-1) * 65536 &&
 *   0 <= tv <= (h-1) * 65536 (a NaN fails).  Camera k SEES the sample when both end taps j = -shoulder1 and j = shoulder1 pass and
 *   have 0 <= f <= max_range.  The taps lie on one straight line of the road, so they lie on one in the picture, and the frame is
 *   convex: every tap between two that pass passes too.  (Only the roundings of u, v could break this, along the frame's very
 *   border; a tap between the ends that does not pass reads as b = g = r = 0, so nothing outside the frame is ever read.)
 *   The sample is read from the seeing camera with the smallest d2 = f*f + l*l of the centre tap j = 0; equal d2: the smallest k
 *   (av_rig_surround's nearest blend).  seen_i = some camera sees it && X >= x_min && X <= x_max.
 *   A seen sample's taps with |j| <= core or shoulder0 <= |j| <= shoulder1 are av_ground_warp's bilinear taps (b, g, r) at
 *   (tu, tv) of that camera, and  gray = (1868*b + 9617*g + 4899*r + 8192) >> 14   (the lane front end's luma).
 *     peak = the largest gray over |j| <= core, among equals the smallest j; (pb, pg, pr) that tap's channels
 *     bg   = (2 * S + n) / (2 * n), S the sum of gray over the n = 2 * (shoulder1 - shoulder0 + 1) shoulder taps, integer division
 *     paint_i = seen_i && peak - bg >= contrast
 *   Over the paint samples: sum_b += pb; sum_g += pg; sum_r += pr; sum_c += peak - bg.  views: bit k where a seen sample was read
 *   from camera k.
 * 2 per boundary, on the bit strings seen and paint.  n_seen, n_paint: their counts.  A paint RUN is a maximal run of paint
 *   samples; n_runs.  A GAP is the stretch between two consecutive runs; it is MEASURED when every sample of it is seen (a gap
 *   across a stretch no camera sees is no gap): n_gaps, longest_gap, gap_m = ((double)(sum of their lengths) / (double)n_gaps) * ds.
 *   A run is COMPLETE when the sample before its first and the sample after its last exist and are seen (they are not paint):
 *   n_dashes, dash_m = ((double)(sum of their lengths) / (double)n_dashes) * ds.  Without one, 0.0.
 *     type = UNKNOWN                            when n_seen < min_seen_n || n_paint < min_paint_n
 *            else SOLID                         when longest_gap < gap_solid_n
 *            else DASHED                        when n_runs >= 2 && longest_gap >= gap_dash_n
 *            else UNKNOWN, flags AMBIGUOUS
 *     colour = 0 with type UNKNOWN, else YELLOW when 10 * sum_b < yellow_tenths * min(sum_g, sum_r), else WHITE
 *     contrast = (2 * sum_c + n_paint) / (2 * n_paint), 0 without paint.
 *   marks[v][b]; profile[v][b][0] = the seen bits, [v][b][1] = the paint bits, sample i in bit i & 31 of word i >> 5.  Rows at
 *   b >= nb (marks and profile) are zero.
 * 3 per vehicle, from frame to frame.  If lanes[v].status has AV_ROAD_CHANGE_LEFT (the vehicle entered the lane on its left: its
 *   old left boundary is now its right one), state.right = state.left and state.left = zero; else with AV_ROAD_CHANGE_RIGHT the
 *   mirror image.  A side observes the first boundary b < nb whose flags carry AV_ROAD_BOUND_LEFT (_RIGHT): its (type, colour);
 *   without one (coasting, the derived side of a one-sided lane, no lane) it observes UNKNOWN.  Then, per side:
 *     observed type != UNKNOWN:  since = 0;  the pair equals (cand_type, cand_colour): run = min(run + 1, 1 << 30);  else cand =
 *       the pair, run = 1.  run >= hold: (type, colour) = cand.
 *     observed UNKNOWN:  since = min(since + 1, 1 << 30);  since >= forget: the side's state is zero (it publishes UNKNOWN).
 *       Otherwise nothing changes: the candidate and its run survive the frame.
 *   frames += 1.  sides[v]: per side the published pair, the observed pair, run and the boundary's index;
 *   may_change_left / _right from the published type of that side.
 *
 *   mounts DEVICE [V][K]; ground DEVICE [V*K]; bgr [V*K][h][w][3]: RECTIFIED frames; bounds [V][8]; lanes [V]; state [V];
 *   marks [V][8]; sides [V]; profile uint32 [V][8][2][16] or NULL.  Two launches on `stream`: one workgroup per (vehicle, boundary)
 *   with one thread per sample (two rounds above 256), then one thread per vehicle.
 * AV_EINVAL before any launch and before the context is looked at: a cfg that av_road_marks_check refuses; n_vehicles outside
 * 1 .. 65535; n_cams outside 1 .. 8; h or w outside 1 .. 32768; a null pointer other than profile and stream. */
/* Host only.  AV_EINVAL for a null cfg; a double not finite; ds, dl, gap_solid, gap_dash, min_seen, min_paint not > 0; gap_dash <
 * gap_solid; a count(len) outside 1 .. 65536; n_samples outside 1 .. 512; core < 0; not core < shoulder0 <= shoulder1 <= 16;
 * contrast outside 1 .. 255; yellow_tenths outside 0 .. 10; hold or forget < 1. */
int av_road_marks_check(const av_road_marks_cfg* cfg);
size_t av_road_marks_state_bytes(void);        /* sizeof(av_road_marks_state) */
int av_road_marks(av_ctx* ctx, av_stream_t stream, const av_road_marks_cfg* cfg, int n_vehicles, int n_cams,
                  const av_rig_mount* mounts, const av_ground_cfg* ground, int h, int w, const uint8_t* bgr,
                  const av_road_lane_bound* bounds, const av_road_lanes_row* lanes, av_road_marks_state* state, av_road_mark* marks,
                  av_road_marks_row* sides, uint32_t* profile);
/* Zeroes the state of vehicle `vehicle` (0 .. n_vehicles - 1), or of every vehicle with -1: one hipMemsetAsync on `stream`. */
int av_road_marks_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int vehicle, av_road_marks_state* state);

/* ---- Lane planner (opt-in): the planner's candidates ranked against the lane boundaries and their marks ---------------------------
 * av_planner_plan_each / _plan_moving know a reference path and obstacle discs.  av_lane_plan is a post-pass over what they wrote:
 * it charges every candidate for the lines it crosses, by their type (av_road_marks'), for the waypoints it spends on a line and
 * for ending on one, ranks the candidates again and says what the chosen one does.  It reads waypoints and cost and writes
 * neither; one launch, one workgroup per vehicle.  float64, every operation rounded on its own (no FMA), in the order written;
 * every comparison with a NaN is false. */
typedef struct {
    double half_width;         /* 0.9   m: the vehicle's half width (av_rig_view_build's ego quad) */
    double x_far;              /* 40.0  m: no line is tested beyond it */
    double w_cross[3];         /* by av_road_mark.type UNKNOWN, SOLID, DASHED: 300, 1000, 0 */
    double w_on[3];            /* 2, 5, 0: per waypoint closer to the line than half_width */
    double w_end;              /* 500:  where the candidate ends it stands inside a lane, whatever the line's type */
    int32_t follow;            /* 1:    lines are taken relative to the ego lane's course */
    int32_t reserved;          /* 0 */
} av_lane_plan_cfg;            /* 80 bytes */
#define AV_LANEPLAN_MAX_LINES 10
#define AV_LANEPLAN_MAX_CAND 192
#define AV_LANEPLAN_MAX_POINTS 256
#define AV_LANEPLAN_SRC_LEFT 8    /* av_lane_plan_line.source: the ego lane's left side itself (coasting or derived) */
#define AV_LANEPLAN_SRC_RIGHT 9
typedef struct {
    double a0, a1, a2;         /* as published: the course is not subtracted here */
    double xe;                 /* the line is tested for 0 <= X <= xe (and x_far) */
    int32_t type;              /* AV_ROAD_MARK_UNKNOWN / _SOLID / _DASHED */
    int32_t source;            /* the boundary's index b, AV_LANEPLAN_SRC_LEFT / _RIGHT, -1 for an unused row */
    int32_t reserved[2];       /* 0 */
} av_lane_plan_line;           /* 48 bytes */
#define AV_LANEPLAN_KEEP 0        /* av_lane_plan_row.maneuver */
#define AV_LANEPLAN_LEFT 1
#define AV_LANEPLAN_RIGHT 2
#define AV_LANEPLAN_FOLLOW 1      /* av_lane_plan_row.flags: a course was subtracted */
#define AV_LANEPLAN_CHANGED 2     /* best != base_best */
#define AV_LANEPLAN_FORCED 4      /* the best candidate crosses a solid or an unknown line */
#define AV_LANEPLAN_NO_LINES 8
typedef struct {
    int32_t best;              /* order[v][0] */
    int32_t base_best;         /* the index of the smallest cost, among equals the smallest index */
    int32_t maneuver;          /* from the sign of delta: 0 keep, < 0 left, > 0 right */
    int32_t delta;             /* delta[v][best] */
    uint32_t crossed;          /* the crossed bits (0 .. 9) of cross[v][best] */
    uint32_t crossed_solid;    /* ... those of its lines of type SOLID */
    uint32_t crossed_unknown;  /* ... of type UNKNOWN */
    int32_t n_lines;
    int32_t flags;
    int32_t reserved;          /* 0 */
    double base_cost, lane_cost, total;            /* cost, lane_cost and total of best */
} av_lane_plan_row;            /* 64 bytes */

/* The stage for vehicle v with (x0, y0, h) = plan_state[v][0 .. 2]:
 * 1 the lines, at most 10, in this order.  For b < nb = clamp(lanes[v].n_bounds, 0, 8): (a0, a1, a2) and xe = x_max of bounds[v][b],
 *   source = b; its type is sides[v].left.type (the published one: av_road_marks' hold / forget) when the boundary's flags carry
 *   AV_ROAD_BOUND_LEFT, else sides[v].right.type with _RIGHT, else marks[v][b].type.  Then, when lanes[v].status has AV_ROAD_LANE:
 *   if no boundary b < nb carries _LEFT, the ego side itself (coasting, or derived from the other): lanes[v].left, xe = x_far, type
 *   sides[v].left.type, source 8; likewise the right side with source 9.  A type outside 0 .. 2 reads as UNKNOWN; with marks and
 *   sides NULL every type is UNKNOWN.  lines[v][0 .. n_lines-1]; the rows behind are zero with source -1.
 * 2 the course.  (c1, c2) = (lanes[v].centre[1], lanes[v].centre[2]) when cfg.follow and the status has AV_ROAD_LANE (row flag
 *   FOLLOW), else (0, 0).  Line j is used as b1 = a1 - c1, b2 = a2 - c2: the planner's candidates are straight in the ego heading,
 *   and their lateral profile is read as an offset from the lane's course.
 * 3 per candidate c and line j, over the waypoints (wx, wy) = waypoints[v][c][i][0 .. 1] in ascending i, placed as av_rig_view_build
 *   places them:
 *     dx = wx - x0;  dy = wy - y0;  X = dx*cos h + dy*sin h;  Y = dy*cos h - dx*sin h
 *   Waypoint i is VALID for line j when X >= 0 && X <= xe && X <= x_far.  For a valid one
 *     e = Y - ((a0 + b1*X) + b2*(X*X));   side = e > 0;   d = half_width - |e|
 *   crossed: two consecutive valid waypoints (in index order) differ in side.  on = the sum from 0.0, in ascending i, of
 *   w_on[type] * (d*d) over the valid waypoints with d > 0.  end = w_end * (d*d) of the last valid waypoint when its d > 0, else 0.
 *     term_j = ((crossed ? w_cross[type] : 0.0) + on) + end;   delta_j = side_last - side_first   (0 without a valid waypoint)
 * 4 per candidate.  lane_cost[v][c] = 0.0 + term_0 + term_1 + ... in ascending j;  total[v][c] = cost[v][c] + lane_cost[v][c];
 *   cross[v][c]: bit j when crossed, bit 16 + j when some valid waypoint had d > 0;  delta[v][c] = the sum of delta_j (negative: the
 *   candidate ends further left, a lateral offset below 0 being left);  order[v][.] = the stable ascending rank of total, the
 *   planner's own rule (a smaller total first, among equals the smaller index).  Without a line every lane cost is exactly 0.0:
 *   total is cost and order is the planner's.
 * 5 row[v]: see the struct; flags FOLLOW, CHANGED, FORCED (crossed_solid | crossed_unknown != 0), NO_LINES (n_lines == 0).
 *
 *   plan_state [V][4]; waypoints [V][C][n][6] (fields 0 and 1 are read); cost [V][C]; bounds [V][8]; lanes [V]; marks [V][8] and
 *   sides [V], NULL only together; lines [V][10]; lane_cost, total [V][C]; order int32 [V][C]; cross uint32 [V][C]; delta int32
 *   [V][C]; row [V].  All device memory, the outputs always written.
 * AV_EINVAL before any launch and before the context is looked at: a cfg that av_lane_plan_check refuses; n_vehicles outside
 * 1 .. 65535; n_cand outside 1 .. 192; n_points outside 1 .. 256; one of marks / sides without the other; any other null pointer
 * except the stream. */
/* Host only.  AV_EINVAL for a null cfg; a double not finite; a weight < 0; half_width or x_far not > 0; follow not 0 or 1. */
int av_lane_plan_check(const av_lane_plan_cfg* cfg);
int av_lane_plan(av_ctx* ctx, av_stream_t stream, const av_lane_plan_cfg* cfg, int n_vehicles, int n_cand, int n_points,
                 const double* plan_state, const double* waypoints, const double* cost, const av_road_lane_bound* bounds,
                 const av_road_lanes_row* lanes, const av_road_mark* marks, const av_road_marks_row* sides, av_lane_plan_line* lines,
                 double* lane_cost, double* total, int32_t* order, uint32_t* cross, int32_t* delta, av_lane_plan_row* row);

#ifdef __cplusplus
}
#endif
#endif /* AVHOT_H */
