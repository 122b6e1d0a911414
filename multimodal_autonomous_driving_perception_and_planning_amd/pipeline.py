"""Batched hot loop: S independent video streams x W frames per launch, all state resident in HBM.

This is the host-side driver of the simulated-detection configuration (BASELINE configs 2/4/5):

    detect (av_simdet_generate) -> track (av_tracker_update)          side stream
                                   Kalman (av_kf_step) -> plan (av_planner_plan)   main stream

in the reference's per-frame call order (demo.py:97-120).  Tracker and Kalman/planner are
independent (the planner never consumes tracks), so they run as two branches
of one fork/join, optionally captured into a hipGraph.  PyTorch only provides device memory and
the stream; every kernel is in libavhot.so.

Opt-in (HotLoop(obstacles="tracks"), set_obstacles, set_reference_paths): every frame plans with its own obstacle
list and every stream with its own reference path (av_planner_plan_each); with "tracks" the lists are the frame's
confirmed tracks (av_track_obstacles), and the planner then runs behind the tracker.  With "moving_tracks" every such
obstacle also carries the velocity its track's last centre difference predicts (av_track_obstacles_moving), and each waypoint
meets it where it is at that waypoint's time (av_planner_plan_moving).  With "filtered_tracks" the tables first pass through a
per-track Kalman filter (av_track_filter_update, behind the tracker on the side stream) and the obstacles take the filter's
centre and velocity (av_track_obstacles_filtered): smoothed, right after a gap, and predicted forward while a track coasts.

Opt-in (set_detections, set_lane_inputs, CameraLoop): the tracker is fed by a real detector's output left in HBM
(av_dets_to_tracker instead of the simulated detector) and every stream's reference path is its own lane fit
(av_lane_paths); CameraLoop wires a PerceptionLoop to a HotLoop that way, S cameras from pixels to ranked trajectories
with no host round trip.

Opt-in (calibration=, HotLoop and CameraLoop): a camera model per stream (perception.CameraCalibration, a ground-plane
homography) in place of the linear pixel-to-metre scales: tracks stand where their boxes' feet meet the road
(av_track_obstacles_ground), lane paths end at the horizon (av_lane_paths_ground), and CameraLoop.enqueue_ground_view warps the
frames to a bird's-eye view (av_ground_warp).  Calibrations with a lens (perception.LensModel, Brown-Conrady): a HotLoop takes its
tracker's boxes as raw pixels (av_track_obstacles_ground_lens); a CameraLoop rectifies every fed frame through a table built
once (av_lens_map_rectify, av_remap: cam.raw -> cam.frames) and everything behind it sees rectified pixels.

Opt-in (RigLoop): V vehicles with K cameras each (perception.CameraRig).  A CameraLoop of V * K cameras runs up to the per-camera
obstacle lists, av_rig_fuse carries them through the mounts into the vehicle frame and merges what several cameras see, and a
HotLoop of V ego states plans around the fused lists -- one plan per vehicle, no host round trip.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as nat


class HotLoop:
    def __init__(self, n_streams=1, window=1, h=720, w=1280, tcap=64, dcap=8, device=0,
                 tracker_kw=None, kf_kw=None, planner_kw=None, keep_waypoints=True, keep_snapshots=True,
                 ctx=None, fused_step=None, overlap=1, obstacles=None, obstacle_kw=None, track_filter_kw=None, calibration=None):
        """fused_step: with window 1, run a time-step as ONE launch (av_hot_step: role-split workgroups running the stage
        kernels' own device code, same results bit for bit) instead of the four stage launches.  None = whenever the
        configuration allows it (window 1, tcap 64, dcap 7..8, iou_threshold > 0, and planner settings whose tiles fit the
        step's LDS: av_hot_step_fits); True where it does not raises ValueError.
        overlap=2 (fused step only): consecutive steps are launched alternately on two HIP streams and ordered per stream and
        role on the device (av_hot_step_seq), so step t + 1 starts while step t's planner is still writing.  The per-step
        buffers (det_*, snap, snap_n, det2trk, z, vstate, plan_state, wp, cost, order) are kept as `overlap` buffer sets (one
        at overlap=1), each with its av_step_set made once; the attributes always name the set of the step enqueued LAST (for
        `z`: the set the NEXT step will read), and that set is next written by the step `overlap` steps on.  Same results as
        overlap=1 bit for bit.
        obstacles="tracks": every frame's confirmed tracks become that frame's planner obstacles (av_track_obstacles: where the
        BEV panel draws them, in the planner's frame) and the planner runs per state (av_planner_plan_each) behind the tracker;
        self.obstacles [S, W, tcap, 3] / self.n_obs [S, W].  obstacle_kw overrides av_obstacle_cfg's fields (x_center, x_scale,
        y_far, y_scale, radius: up to 16 per-class radii, default 1.5 for ids 0..5 = car, truck, pedestrian, cyclist, motorcycle,
        bus and 0 = no obstacle for the rest).  Needs keep_snapshots=True and the stage launches (no fused step, overlap 1).
        obstacles="moving_tracks": the same obstacles, each with the constant velocity of its track in the planner's frame
        (av_track_obstacles_moving: the last centre difference at obstacle_kw's frame_rate, default 30 frames/s, plus the ego's
        own speed), planned around where they are at each waypoint's time (av_planner_plan_moving); self.obstacles
        [S, W, tcap, 5] (x, y, radius, vx, vy).  frame_rate is accepted only in this mode and the next.
        obstacles="filtered_tracks": "moving_tracks" with every track's centre and velocity taken from a per-track constant-velocity
        Kalman filter over the snapshot tables (av_track_filter_update, then av_track_obstacles_filtered): self.track_filt
        [S, W, tcap, 6] (cx, cy, vx, vy, pos_sigma, vel_sigma; px and px / frame) aligned with the snapshot rows.  The filter's state
        (self.track_filter, a tracking.TrackFilter) persists across windows and is cleared by reset().  track_filter_kw: its settings
        (q_accel, r_meas, p0_pos, p0_vel), accepted only in this mode.
        calibration: one perception.CameraCalibration, or one per stream -- the camera model (a ground-plane homography,
        av_ground_cfg) in place of av_obstacle_cfg's four linear scales: the obstacle stage becomes av_track_obstacles_ground in the
        mode `obstacles` names (a track stands where its box's foot meets the road, a foot off the road is no obstacle and is
        counted in self.n_off [S, W], pixel velocities go through the projection's Jacobian), set_lane_inputs' paths go through
        av_lane_paths_ground.  obstacle_kw may then carry radius and frame_rate only.  Needs the stage launches like obstacles=.
        Calibrations with a lens (all streams, or none): the tracker's boxes are RAW pixels, the obstacle stage is
        av_track_obstacles_ground_lens (self.lens: the device table beside self.ground), and set_lane_inputs is refused -- lane
        fits come from rectified frames, which CameraLoop provides."""
        if not torch.cuda.is_available():
            raise RuntimeError("HotLoop needs a HIP device; this package has no CPU path")
        self.S, self.W, self.h, self.w, self.tcap, self.dcap = n_streams, window, h, w, tcap, dcap
        self.overlap = int(overlap)
        if self.overlap not in (1, 2, 3, 4):
            raise ValueError("overlap is 1 .. 4")
        self.dev = torch.device("cuda", device)
        self.ctx = ctx or nat.Context(device)
        self.L = nat.lib()
        tk = dict(iou_threshold=0.3, max_age=30, min_hits=3, trajectory_length=50)
        tk.update(tracker_kw or {})
        kk = dict(dt=0.033, process_noise=0.1, measurement_noise=1.0)
        kk.update(kf_kw or {})
        pk = dict(planning_horizon=5.0, dt=0.1, num_samples=7, w_lateral=1.0, w_velocity=0.5,
                  w_acceleration=0.3, w_curvature=0.4)
        pk.update(planner_kw or {})
        self.pcfg = nat.PlannerCfg(reserved=0, **pk)
        nat.check(self.L.av_planner_configure(self.ctx.handle, C.byref(self.pcfg)))
        n, c = C.c_int(), C.c_int()
        nat.check(self.L.av_planner_dims(self.ctx.handle, C.byref(n), C.byref(c)))
        self.n_points, self.n_cand = n.value, c.value

        S, W, d = n_streams, window, self.dev
        i32, f64 = torch.int32, torch.float64
        self.frame_count = torch.zeros(S, dtype=i32, device=d)
        self.det_status = torch.zeros(S, dtype=i32, device=d)
        self.trk_bytes = int(self.L.av_tracker_state_bytes(tcap, tk["trajectory_length"]))
        self.trk_state = torch.zeros(S, self.trk_bytes, dtype=torch.uint8, device=d)
        self.kf_state = torch.zeros(S, nat.KF_STATE_DOUBLES, dtype=f64, device=d)
        # what all steps share, as the one-launch step takes it (av_step_loop); tcfg / kcfg are its members, not copies
        self._cloop = nat.StepLoop(nat.TrackerCfg(**tk), nat.KfCfg(**kk), S, h, w, dcap, tcap, 0, self.frame_count.data_ptr(),
                                   self.det_status.data_ptr(), self.trk_state.data_ptr(), self.kf_state.data_ptr())
        self.tcfg, self.kcfg = self._cloop.tracker_cfg, self._cloop.kf_cfg
        self.keep_snapshots, self.keep_waypoints = keep_snapshots, keep_waypoints
        # the per-step buffers: `overlap` sets, each with its av_step_set; the attributes name one of them (reset(): the first)
        self._sets = [self._new_set() for _ in range(self.overlap)]
        self._csets = (nat.StepSet * self.overlap)(*[nat.StepSet(*[t.data_ptr() if t is not None else None for t in b.values()])
                                                     for b in self._sets])
        self.__dict__.update(self._sets[0])
        self._use_streams([torch.cuda.Stream(device=d) for _ in range(self.overlap)])
        self.graph_id = None
        self._graphs = {}
        if obstacles not in (None, "tracks", "moving_tracks", "filtered_tracks"):
            raise ValueError('obstacles is None, "tracks", "moving_tracks" or "filtered_tracks"')
        if track_filter_kw is not None and obstacles != "filtered_tracks":
            raise ValueError('track_filter_kw belongs to obstacles="filtered_tracks"')
        if obstacles is not None and (fused_step or overlap != 1 or not keep_snapshots):
            raise ValueError('obstacles="%s" needs keep_snapshots=True and the stage launches (fused_step=True and overlap > 1 '
                             'plan without obstacles)' % obstacles)
        if calibration is not None and (fused_step or overlap != 1):
            raise ValueError("calibration= needs the stage launches (fused_step=True and overlap > 1 plan without obstacles and "
                             "lane paths)")
        self._obs_mode = obstacles                # None | "tracks" | "moving_tracks" | "filtered_tracks" | "given" (set_obstacles)
        self.track_filter = self.track_filt = None
        self.obstacles = self.n_obs = self.ref_paths = self.n_ref = None
        self._obstacle_kw = dict(obstacle_kw or {})
        self._src = self._class_map = self.det_dropped = None       # set_detections
        self._lanes = self.lane_offset = None                       # set_lane_inputs
        self._meas = None                                           # set_measurement_source
        self._ext_streams = {}
        self.tag_log = None                                         # enable_tag_log
        self.calibration = self.ground = self.n_off = self.lens = self.lenses = None
        if calibration is not None:
            from .perception.calibration import ground_table, lens_table, lenses_of
            scales = sorted(k for k in ("x_center", "x_scale", "y_far", "y_scale") if k in self._obstacle_kw)
            if scales:
                raise ValueError("obstacle_kw: %s belong to the linear map; with calibration= only radius and frame_rate are taken"
                                 % ", ".join(scales))
            self.ground, self.calibration = ground_table(calibration, S, d)         # uint8 [S, 160]: av_ground_cfg per stream
            self.lenses = lenses_of(self.calibration, S)
            if self.lenses is not None:
                self.lens = lens_table(self.lenses, S, d)[0]                        # uint8 [S, 112]: av_lens_cfg per stream
            fused_step = False
        if obstacles is not None:
            self.ocfg = self._make_ocfg(obstacles)
            self.obstacles = torch.zeros(S, W, tcap, 3 if obstacles == "tracks" else 5, dtype=f64, device=d)
            self.n_obs = torch.zeros(S, W, dtype=i32, device=d)
            if self.ground is not None:
                self.n_off = torch.zeros(S, W, dtype=i32, device=d)
            if obstacles == "filtered_tracks":
                from .tracking.track_filter import TrackFilter
                self.track_filter = TrackFilter(S, tcap, ctx=self.ctx, **(track_filter_kw or {}))
                self.track_filt = torch.zeros(S, W, tcap, 6, dtype=f64, device=d)
            fused_step = False
        can_fuse = window == 1 and tcap == 64 and 7 <= dcap <= 8 and self.tcfg.iou_threshold > 0
        if fused_step and not can_fuse:
            raise ValueError("fused_step needs window 1, tcap 64, dcap 7..8 and iou_threshold > 0")
        if can_fuse and fused_step is not False:
            # the planner's settings decide whether its tiles fit the one-launch step's LDS: decided here, not at the first step()
            # (whether overlap=D launches are all resident is the trial step's question below)
            rc = self.L.av_hot_step_fits(self.ctx.handle, S, dcap, tcap, 1)
            if rc != 0:
                if fused_step:
                    raise ValueError("fused_step: %s" % self.L.av_last_error_string().decode())
                can_fuse = False
        self.fused_step = can_fuse if fused_step is None else bool(fused_step)
        self.wire = None                  # set_wire(): the fused step also writes every stream's table in wire format
        self._wire_ids = (0, 0)
        self._seq, self._stepped = 0, False
        if self.overlap > 1:
            if not self.fused_step:
                raise ValueError("overlap=2 needs the fused step (window 1, tcap 64, dcap 7..8, iou_threshold > 0)")
            self.seq_flags = torch.zeros(nat.step_flag_ints(S), dtype=i32, device=d)
            self.reset()
            try:                              # (one step now: the library refuses a depth whose launches would not all be resident)
                self._enqueue_step_seq()
                self.synchronize()
            except RuntimeError as e:
                raise ValueError("overlap=%d: %s" % (self.overlap, e)) from None
        self.reset()

    def _make_ocfg(self, mode):
        """av_obstacle_cfg from the constructor's obstacle_kw over the BEV panel's defaults; frame_rate (-> self.frame_rate) is
        accepted with modes "moving_tracks" and "filtered_tracks" only."""
        ok = dict(x_center=320.0, x_scale=0.03, y_far=50.0, y_scale=0.1, radius=[1.5] * 6 + [0.0] * 10)
        ok.update(self._obstacle_kw)
        if mode in ("moving_tracks", "filtered_tracks"):
            self.frame_rate = float(ok.pop("frame_rate", 30.0))
            if not (self.frame_rate > 0.0 and np.isfinite(self.frame_rate)):
                raise ValueError("obstacle_kw: frame_rate must be > 0 and finite")
        elif "frame_rate" in ok:
            raise ValueError('obstacle_kw: frame_rate belongs to obstacles="moving_tracks" / "filtered_tracks"')
        rad = [float(r) for r in ok.pop("radius")]
        if len(rad) > 16:
            raise ValueError("obstacle_kw: at most 16 per-class radii")
        return nat.ObstacleCfg(radius=(C.c_double * 16)(*(rad + [0.0] * (16 - len(rad)))), **ok)

    def _new_set(self):
        """One set of the per-step buffers, attribute name -> tensor (None: not kept), in av_step_set's member order (wp is its
        `waypoints`)."""
        S, W, d, i32, f64 = self.S, self.W, self.dev, torch.int32, torch.float64
        zeros = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=d)
        return dict(det_n=zeros(S, W, dtype=i32), det_box=zeros(S, W, self.dcap, 4, dtype=i32), det_cls=zeros(S, W, self.dcap, dtype=i32),
                    det_conf=zeros(S, W, self.dcap, dtype=f64),
                    snap=zeros(S, W, self.tcap, nat.TRACK_ROW_BYTES, dtype=torch.uint8) if self.keep_snapshots else None,
                    snap_n=zeros(S, W, dtype=i32) if self.keep_snapshots else None, det2trk=zeros(S, W, self.dcap, dtype=i32),
                    z=zeros(S, W, 4, dtype=f64), vstate=zeros(S, W, nat.VSTATE_DOUBLES, dtype=f64), plan_state=zeros(S, W, 4, dtype=f64),
                    wp=zeros(S * W, self.n_cand, self.n_points, nat.WP_DOUBLES, dtype=f64) if self.keep_waypoints else None,
                    cost=zeros(S * W, self.n_cand, dtype=f64), order=zeros(S * W, self.n_cand, dtype=i32))

    def _use_streams(self, streams):
        """The HIP streams the steps run on: step q on streams[q % overlap]; `stream` is the first."""
        self._pstreams, self.stream = list(streams), streams[0]
        self._cstreams = (C.c_void_p * self.overlap)(*[st.cuda_stream for st in streams])

    # ------------------------------------------------------------------------------------------
    @property
    def _s(self):
        return C.c_void_p(self.stream.cuda_stream)

    _i32 = staticmethod(nat.step_i32)

    @property
    def step_waves(self):
        """Waves per workgroup of the one-launch step as the library launches it for this loop (av_hot_step_plan at the loop's
        overlap depth: 16, 12 or 8; AVHOT_STEP_PW is read at every launch, and here); None without the fused step."""
        if not self.fused_step:
            return None
        rc, waves, _, _ = nat.step_plan(self.ctx.handle, self.S, self.dcap, self.tcap, self.overlap)
        nat.check(rc)
        return waves

    def _serial_only(self, what):
        if self.overlap != 1:
            raise RuntimeError("%s is not available with overlap=2.. (only the one-launch step is ordered across the loop's streams)" % what)

    def reset(self, frame_offsets=None):
        """Resets every stream (tracker.reset(), state_estimator.reset(), detector.reset())."""
        h, L = self.ctx.handle, self.L
        for st in self._pstreams:
            st.synchronize()
        nat.check(L.av_tracker_reset(h, self._s, self.S, self.tcap, self.tcfg.trajectory_length, nat.ptr(self.trk_state)))
        nat.check(L.av_kf_reset(h, self._s, self.S, nat.ptr(self.kf_state)))
        if self.track_filter is not None:
            self.track_filter.reset(self._s)
        with torch.cuda.stream(self.stream):
            if frame_offsets is None:
                self.frame_count.zero_()
            else:
                self.frame_count.copy_(torch.as_tensor(np.asarray(frame_offsets, np.int32)), non_blocking=False)
            if self.overlap > 1:
                self.seq_flags.zero_()
                self.seq_flags[64 * self.S + 32:65 * self.S + 32].copy_(self.frame_count)
        self._seq, self._stepped = 0, False
        self.__dict__.update(self._sets[0])
        self.stream.synchronize()

    def load_measurements(self, z, all_sets=False):
        """z: float64 [S, W, 4] ego measurements for the next window (host array).  overlap=2..: for the next STEP (its buffer
        set, on its stream); all_sets=True: for every step from now on (all sets)."""
        zt = torch.as_tensor(np.ascontiguousarray(z, np.float64)).view(self.S, self.W, 4)
        nxt = self._seq % self.overlap
        for k in (range(self.overlap) if all_sets else (nxt,)):
            with torch.cuda.stream(self._pstreams[k]):
                self._sets[k]["z"].copy_(zt)
            self._pstreams[k].synchronize()
        self.z = self._sets[nxt]["z"]

    # ---- individual stages (enqueue only) --------------------------------------------------------
    def enqueue_detect(self, stream=None):
        self._serial_only("enqueue_detect")
        if self._src is not None:
            # set_detections: the caller's detector output -> det_* (av_dets_to_tracker); the frame counters advance as they do
            # with the simulated detector, on the same stream
            n, box, conf, cls = self._src
            nat.check(self.L.av_dets_to_tracker(self.ctx.handle, stream or self._s, self.S * self.W, int(box.shape[2]), nat.ptr(n),
                                                nat.ptr(box), nat.ptr(conf), nat.ptr(cls), nat.ptr(self._class_map),
                                                0 if self._class_map is None else int(self._class_map.numel()), self.dcap,
                                                nat.ptr(self.det_n), nat.ptr(self.det_box), nat.ptr(self.det_cls),
                                                nat.ptr(self.det_conf), nat.ptr(self.det_dropped)))
            with torch.cuda.stream(self._torch_stream(stream)):
                self.frame_count.add_(self.W)
            return
        nat.check(self.L.av_simdet_generate(self.ctx.handle, stream or self._s, self.S, self.W, self.h, self.w,
                                            self.dcap, nat.ptr(self.frame_count), nat.ptr(self.det_n),
                                            nat.ptr(self.det_box), nat.ptr(self.det_cls), nat.ptr(self.det_conf),
                                            nat.ptr(self.det_status)))

    def enqueue_track(self, stream=None):
        self._serial_only("enqueue_track")
        nat.check(self.L.av_tracker_update(self.ctx.handle, stream or self._s, C.byref(self.tcfg), self.S, self.W,
                                           self.dcap, nat.ptr(self.det_n), nat.ptr(self.det_box),
                                           nat.ptr(self.det_cls), nat.ptr(self.det_conf), self.tcap,
                                           nat.ptr(self.trk_state), nat.ptr(self.snap), nat.ptr(self.snap_n),
                                           nat.ptr(self.det2trk)))

    def set_measurement_source(self, z, mode, producer=None):
        """The Kalman stage reads the ego measurement from the caller's device tensors instead of load_measurements' buffer: z
        float64 [S, W, 4] and mode uint8 [S, W] (av_kf_step's: 1 = step(z), 2 = step(None), ...), written on the device by a stage
        ahead of it (perception.GroundOdometry).  producer: a callable(stream) that enqueues that stage; enqueue_kf calls it on
        its own stream in front of av_kf_step, so the stage runs beside the tracker's branch.  (None, None) puts the loop's own
        buffer back.  The one-launch step and the overlapped loop read their own buffer sets: refused there."""
        if z is None and mode is None:
            self._meas = None
            self._drop_graphs()
            return
        if self.fused_step or self.overlap != 1:
            raise RuntimeError("set_measurement_source needs the stage launches, HotLoop(fused_step=False): the one-launch step and "
                               "overlap > 1 read the ego measurement from their own buffer sets (load_measurements)")
        if (z is None or mode is None or z.dtype != torch.float64 or mode.dtype != torch.uint8 or z.device != self.dev
                or mode.device != self.dev or tuple(z.shape) != (self.S, self.W, 4) or tuple(mode.shape) != (self.S, self.W)
                or not z.is_contiguous() or not mode.is_contiguous()):
            raise ValueError("set_measurement_source: device tensors z float64 [%d, %d, 4] and mode uint8 [%d, %d], contiguous"
                             % (self.S, self.W, self.S, self.W))
        self._meas = (z, mode, producer)
        self._drop_graphs()

    def enqueue_kf(self, stream=None):
        self._serial_only("enqueue_kf")
        z, mode = self.z, None
        if self._meas is not None:
            z, mode, producer = self._meas
            if producer is not None:
                producer(stream or self._s)
        nat.check(self.L.av_kf_step(self.ctx.handle, stream or self._s, C.byref(self.kcfg), self.S, self.W,
                                    nat.ptr(z), nat.ptr(mode), nat.ptr(self.kf_state), nat.ptr(self.vstate),
                                    nat.ptr(self.plan_state)))

    def enqueue_maneuver(self, stream=None, lane_offset=None):
        """Maneuver tags of every frame of the window from the Kalman output (ManeuverDetector.detect,
        maneuver_detector.py:105-262); call after enqueue_kf on the same stream.  Results: self.maneuver
        (uint8 view of av_maneuver_row [S][W])."""
        self._serial_only("enqueue_maneuver")
        if not hasattr(self, "mv_state"):
            self.mv_state = torch.zeros(self.S, nat.MANEUVER_STATE_DOUBLES, dtype=torch.float64, device=self.dev)
            self.maneuver = torch.zeros(self.S, self.W, nat.MANEUVER_ROW_BYTES, dtype=torch.uint8, device=self.dev)
        nat.check(self.L.av_maneuver_detect(self.ctx.handle, stream or self._s, self.S, self.W, nat.ptr(self.vstate),
                                            nat.ptr(lane_offset), nat.ptr(self.mv_state), nat.ptr(self.maneuver)))

    def enqueue_interactions(self, stream=None, frame_shape=None, class_names=None):
        """Interaction tags of every frame of the window from the tracker's snapshot tables and the Kalman output
        (InteractionDetector.detect, interaction_detector.py:132-222); call where both are complete (after the
        join).  Results: self.inter_rows (av_interaction_row [S][W][tcap]), self.inter_summary ([S][W])."""
        self._serial_only("enqueue_interactions")
        from .perception.detector import ObjectDetector
        from .tagging.interaction_detector import interaction_cfg
        if self.tcap != 64 or self.snap is None:
            raise RuntimeError("enqueue_interactions needs keep_snapshots=True and tcap 64")
        if not hasattr(self, "inter_state"):
            self.inter_state = torch.zeros(self.S * int(self.L.av_interaction_state_bytes(self.tcap)), dtype=torch.uint8,
                                           device=self.dev)
            nat.check(self.L.av_interaction_reset(self.ctx.handle, stream or self._s, self.S, self.tcap, nat.ptr(self.inter_state)))
            self.inter_rows = torch.zeros(self.S, self.W, self.tcap, nat.INTERACTION_ROW_BYTES, dtype=torch.uint8, device=self.dev)
            self.inter_summary = torch.zeros(self.S, self.W, nat.INTERACTION_SUMMARY_BYTES, dtype=torch.uint8, device=self.dev)
        cfg = interaction_cfg(frame_shape or (self.h, self.w), class_names or [ObjectDetector.CLASSES[k] for k in range(8)])
        nat.check(self.L.av_interaction_detect(self.ctx.handle, stream or self._s, C.byref(cfg), self.S, self.W, self.tcap,
                                               nat.ptr(self.snap), nat.ptr(self.snap_n), nat.ptr(self.vstate), None, None,
                                               nat.ptr(self.inter_state), nat.ptr(self.inter_rows), nat.ptr(self.inter_summary)))

    def enable_tag_log(self, capacity, columns=False):
        """A device-resident tag log of `capacity` frames per stream (tagging.tag_log.TagLog, self.tag_log) for enqueue_tags;
        columns=True: with the per-frame records (TagLog(columns=True))."""
        self._serial_only("enable_tag_log")
        from .tagging.tag_log import TagLog
        self.tag_log = TagLog(self.S, capacity, device=self.dev.index, ctx=self.ctx, stream=self.stream, columns=columns)
        return self.tag_log

    def enqueue_tags(self, stream=None, scene_rows=None, det=None, elem_table=None):
        """This window's tags into self.tag_log (av_tags_pack + av_taglog_append): the maneuver rows and the interaction rows /
        summaries, whichever enqueue_maneuver / enqueue_interactions have produced -- call it after them on the same stream --
        plus, when given, scene_rows (av_scene_row [S][W] as uint8) with det = (det_n [S][W], det_cls [S][W][max_det]) and
        elem_table (tagging.tag_log.element_table) for the traffic elements."""
        self._serial_only("enqueue_tags")
        if self.tag_log is None:
            raise RuntimeError("enqueue_tags needs enable_tag_log(capacity)")
        inter = hasattr(self, "inter_rows")
        det_n, det_cls = det if det is not None else (None, None)
        self.tag_log.pack_and_append(self.W, maneuver=getattr(self, "maneuver", None),
                                     inter_rows=self.inter_rows if inter else None,
                                     inter_summary=self.inter_summary if inter else None, snap_n=self.snap_n if inter else None,
                                     scene_rows=scene_rows, det_n=det_n, det_cls=det_cls, elem_table=elem_table,
                                     stream=stream or self._s)

    def enqueue_bev(self, stream=None, frame=None, n_candidates=10):
        """BEV panels of every stream (BEVRenderer.render, bev_renderer.py:286-348) for one frame of the window, built and
        painted on the device from the tables the step left in HBM; call where tracker, Kalman and planner outputs are
        complete (after the join).  Results: self.bev (uint8 [S, 600, 600, 3]).  The trails come from the tracker's
        history rings, i.e. they are those of the window's last frame (the default)."""
        self._serial_only("enqueue_bev")
        from .visualization.bev_renderer import BEVRenderer
        if not (self.keep_waypoints and self.keep_snapshots):
            raise RuntimeError("enqueue_bev needs keep_waypoints=True and keep_snapshots=True")
        if not hasattr(self, "bev"):
            r = BEVRenderer(device=self.dev.index)
            self._bev_cfg = nat.BevCfg(r.width, r.height, r.pixels_per_meter, r.x_range[0], r.x_range[1], r.y_range[0], r.y_range[1],
                                       n_candidates, 0)
            self._bev_cap = int(self.L.av_bev_prim_cap(C.byref(self._bev_cfg), self.tcap, self.n_points))
            self._bev_base = torch.as_tensor(r.create_base_image()).to(self.dev)
            self.bev = torch.empty(self.S, r.height, r.width, 3, dtype=torch.uint8, device=self.dev)
            self._bev_prims = torch.zeros(self.S, self._bev_cap, nat.PRIM_BYTES, dtype=torch.uint8, device=self.dev)
            self._bev_n = torch.zeros(self.S, dtype=torch.int32, device=self.dev)
        st = stream or self._s
        f = self.W - 1 if frame is None else frame
        # the base image is copied on the stream the kernels run on (a caller-supplied stream must not race with it)
        ts = self.stream if stream is None else torch.cuda.ExternalStream(stream.value if hasattr(stream, "value") else int(stream), device=self.dev)
        with torch.cuda.stream(ts):
            self.bev.copy_(self._bev_base.unsqueeze(0).expand_as(self.bev))
        nat.check(self.L.av_bev_build(self.ctx.handle, st, C.byref(self._bev_cfg), self.S, self.W, f, self.tcap,
                                      self.tcfg.trajectory_length, nat.ptr(self.snap), nat.ptr(self.snap_n), nat.ptr(self.trk_state),
                                      nat.ptr(self.vstate), nat.ptr(self.wp), nat.ptr(self.order), nat.ptr(self._bev_prims),
                                      self._bev_cap, nat.ptr(self._bev_n)))
        nat.check(self.L.av_raster_draw(self.ctx.handle, st, self.S, self._bev_cfg.height, self._bev_cfg.width, nat.ptr(self.bev),
                                        nat.ptr(self._bev_prims), self._bev_cap, nat.ptr(self._bev_n), None, 0))

    def enqueue_plan(self, stream=None):
        self._serial_only("enqueue_plan")
        nat.check(self.L.av_planner_plan(self.ctx.handle, stream or self._s, self.S * self.W,
                                         nat.ptr(self.plan_state), None, 0, None, 0, nat.ptr(self.wp),
                                         nat.ptr(self.cost), nat.ptr(self.order)))

    # ---- per-state planner inputs -------------------------------------------------------------------
    def _per_state(self):
        return self._obs_mode is not None or self.ref_paths is not None

    def _need_stage_launches(self, what):
        if self.overlap != 1 or self.fused_step:
            raise RuntimeError("%s needs the stage launches, HotLoop(fused_step=False): the one-launch step plans without reference "
                               "paths and obstacles" % what)

    def _drop_graphs(self):
        # a captured step has the planner call it makes, and the buffers it reads, baked in
        for gid in self._graphs.values():
            nat.check(self.L.av_graph_destroy(self.ctx.handle, gid))
        self._graphs, self.graph_id = {}, None

    def _torch_stream(self, stream):
        """The torch stream object of a raw stream handle (None: the loop's own stream)."""
        if stream is None:
            return self.stream
        h = stream.value if hasattr(stream, "value") else int(stream)
        if h not in self._ext_streams:
            self._ext_streams[h] = torch.cuda.ExternalStream(h, device=self.dev)
        return self._ext_streams[h]

    def set_detections(self, src_n, src_box=None, src_conf=None, src_cls=None, class_map=None):
        """A real detector's output as the tracker's input, read in place by every step from now on: device tensors int32 [S, W]
        counts, float32 [S, W, max_det, 4] boxes (x1, y1, x2, y2), float32 [S, W, max_det] confidences and int32 [S, W, max_det]
        class ids, in the detector's (confidence-descending) order -- PerceptionLoop's det_* viewed as [S, 1, ...].
        enqueue_detect then calls av_dets_to_tracker into the loop's own det_* instead of the simulated detector: coordinates
        truncated like int(), at most dcap entries per frame, the surplus counted in self.det_dropped [S, W].  class_map: None
        (raw class ids) or an int32 table detector id -> tracker id, negative = skip the entry (host array or device tensor).
        set_detections(None): the simulated detector again."""
        if src_n is None:
            if not (src_box is None and src_conf is None and src_cls is None):
                raise ValueError("set_detections: the four detector tensors go together")
            self._src = self._class_map = self.det_dropped = None
            self._drop_graphs()
            return
        self._need_stage_launches("set_detections")
        if src_box is None or src_conf is None or src_cls is None:
            raise ValueError("set_detections: the four detector tensors go together")
        ok = lambda t, dt, shape: (t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.is_cuda
                                   and t.device == self.dev)
        if not (torch.is_tensor(src_box) and src_box.dim() == 4 and src_box.shape[2] >= 1
                and ok(src_box, torch.float32, (self.S, self.W, src_box.shape[2], 4))):
            raise ValueError("set_detections: src_box is a contiguous float32 device tensor [S, W, max_det, 4]")
        md = int(src_box.shape[2])
        if not (torch.is_tensor(src_n) and ok(src_n, torch.int32, (self.S, self.W))):
            raise ValueError("set_detections: src_n is a contiguous int32 device tensor [S, W]")
        if not (torch.is_tensor(src_conf) and ok(src_conf, torch.float32, (self.S, self.W, md))):
            raise ValueError("set_detections: src_conf is a contiguous float32 device tensor [S, W, max_det]")
        if not (torch.is_tensor(src_cls) and ok(src_cls, torch.int32, (self.S, self.W, md))):
            raise ValueError("set_detections: src_cls is a contiguous int32 device tensor [S, W, max_det]")
        if not 1 <= self.dcap <= 64:
            raise ValueError("set_detections: dcap %d not in 1 .. 64 (the tracker's limit)" % self.dcap)
        if class_map is not None:
            if not torch.is_tensor(class_map):
                class_map = torch.as_tensor(np.ascontiguousarray(class_map, np.int32))
            if class_map.dtype != torch.int32 or class_map.dim() != 1 or class_map.numel() == 0:
                raise ValueError("set_detections: class_map is a one-dimensional int32 table")
            class_map = class_map.to(self.dev).contiguous()
        self._src, self._class_map = (src_n, src_box, src_conf, src_cls), class_map
        self.det_dropped = torch.zeros(self.S, self.W, dtype=torch.int32, device=self.dev)
        self._drop_graphs()

    def set_lane_inputs(self, poly, pts=None, info=None, n_points=50):
        """The lane detector's fits as every stream's reference path, rebuilt every step: device tensors float64 [S, 2, 3],
        int32 [S, 2, 50, 2] and int32 [S, 8] (av_lane_detect's poly / pts / info, PerceptionLoop's attributes), read in place.
        enqueue_step then runs av_lane_paths behind the Kalman stage into self.ref_paths [S, n_points, 2] / self.n_ref [S] /
        self.lane_offset [S] (metres, NaN without a lane pair: what enqueue_maneuver(lane_offset=...) takes when the window is
        1) and plans per state (av_planner_plan_each).  The image -> road scales are the loop's av_obstacle_cfg (obstacle_kw).
        Not together with set_reference_paths.  set_lane_inputs(None): no lane paths."""
        if poly is None:
            if not (pts is None and info is None):
                raise ValueError("set_lane_inputs: poly, pts and info go together")
            if self._lanes is not None:
                self._lanes = self.ref_paths = self.n_ref = self.lane_offset = None
                self._drop_graphs()
            return
        if self.lens is not None:
            raise ValueError("set_lane_inputs: this loop's calibration has a lens, so its pixels are raw, and lane fits come from "
                             "rectified frames -- CameraLoop rectifies the frames and feeds both")
        self._need_stage_launches("set_lane_inputs")
        if self._lanes is None and self.ref_paths is not None:
            raise RuntimeError("set_lane_inputs: this loop has caller-supplied reference paths (set_reference_paths)")
        if not 2 <= int(n_points) <= 64:
            raise ValueError("set_lane_inputs: n_points is 2 .. 64")
        ok = lambda t, dt, shape: (torch.is_tensor(t) and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()
                                   and t.is_cuda and t.device == self.dev)
        if not ok(poly, torch.float64, (self.S, 2, 3)):
            raise ValueError("set_lane_inputs: poly is a contiguous float64 device tensor [S, 2, 3]")
        if not ok(pts, torch.int32, (self.S, 2, 50, 2)):
            raise ValueError("set_lane_inputs: pts is a contiguous int32 device tensor [S, 2, 50, 2]")
        if not ok(info, torch.int32, (self.S, 8)):
            raise ValueError("set_lane_inputs: info is a contiguous int32 device tensor [S, 8]")
        if not hasattr(self, "ocfg"):
            self.ocfg = self._make_ocfg(None)
        self._lanes = (poly, pts, info, int(n_points))
        self.ref_paths = torch.zeros(self.S, int(n_points), 2, dtype=torch.float64, device=self.dev)
        self.n_ref = torch.zeros(self.S, dtype=torch.int32, device=self.dev)
        self.lane_offset = torch.full((self.S,), float("nan"), dtype=torch.float64, device=self.dev)
        self._drop_graphs()

    def enqueue_lane_paths(self, stream=None):
        """set_lane_inputs: the lane fits and the window's first start states -> self.ref_paths / self.n_ref / self.lane_offset
        (av_lane_paths); call behind enqueue_kf on the same stream."""
        if self._lanes is None:
            raise RuntimeError("enqueue_lane_paths needs set_lane_inputs")
        poly, pts, info, n_points = self._lanes
        if self.ground is not None:
            nat.check(self.L.av_lane_paths_ground(self.ctx.handle, stream or self._s, nat.ptr(self.ground), self.S, self.h, self.w,
                                                  n_points, nat.ptr(poly), nat.ptr(pts), nat.ptr(info), nat.ptr(self.plan_state),
                                                  self.W, int(self.ref_paths.shape[1]), nat.ptr(self.ref_paths), nat.ptr(self.n_ref),
                                                  nat.ptr(self.lane_offset)))
            return
        nat.check(self.L.av_lane_paths(self.ctx.handle, stream or self._s, C.byref(self.ocfg), self.S, self.h, self.w, n_points,
                                       nat.ptr(poly), nat.ptr(pts), nat.ptr(info), nat.ptr(self.plan_state), self.W,
                                       int(self.ref_paths.shape[1]), nat.ptr(self.ref_paths), nat.ptr(self.n_ref),
                                       nat.ptr(self.lane_offset)))

    def set_obstacles(self, obstacles, n_obs):
        """Caller-supplied obstacles for every frame of the window: float64 device tensor [S, W, ocap, 3] (x, y, radius) or, moving,
        [S, W, ocap, 5] (x, y, radius, vx, vy), and int32 [S, W] counts, read by every step from now on; None, None: none.  Not
        together with obstacles="tracks" / "moving_tracks" / "filtered_tracks"."""
        if self._obs_mode in ("tracks", "moving_tracks", "filtered_tracks"):
            raise RuntimeError('set_obstacles: this loop takes its obstacles from the tracker (obstacles="%s")' % self._obs_mode)
        if (obstacles is None) != (n_obs is None):
            raise ValueError("set_obstacles: the list and its counts go together")
        if obstacles is not None:
            self._need_stage_launches("set_obstacles")
            if not (obstacles.dtype == torch.float64 and obstacles.dim() == 4 and tuple(obstacles.shape[:2]) == (self.S, self.W)
                    and obstacles.shape[3] in (3, 5) and obstacles.is_contiguous() and obstacles.is_cuda):
                raise ValueError("set_obstacles: obstacles is a contiguous float64 device tensor [S, W, ocap, 3] or [S, W, ocap, 5]")
            if not (n_obs.dtype == torch.int32 and tuple(n_obs.shape) == (self.S, self.W) and n_obs.is_contiguous() and n_obs.is_cuda):
                raise ValueError("set_obstacles: n_obs is a contiguous int32 device tensor [S, W]")
        self.obstacles, self.n_obs = obstacles, n_obs
        self._obs_mode = None if obstacles is None else "given"
        self._drop_graphs()

    def set_reference_paths(self, paths, n_ref):
        """One reference path per stream (each stream's MotionPlanner.set_reference_path, motion_planner.py:93-124): float64
        device tensor [S, rcap, 2] and int32 [S] point counts (fewer than two points: no path for that stream); None, None: none."""
        if (paths is None) != (n_ref is None):
            raise ValueError("set_reference_paths: the paths and their counts go together")
        if self._lanes is not None:
            raise RuntimeError("set_reference_paths: this loop builds its reference paths from the lane fits (set_lane_inputs)")
        if paths is not None:
            self._need_stage_launches("set_reference_paths")
            if not (paths.dtype == torch.float64 and paths.dim() == 3 and paths.shape[0] == self.S and paths.shape[2] == 2
                    and paths.is_contiguous() and paths.is_cuda):
                raise ValueError("set_reference_paths: paths is a contiguous float64 device tensor [S, rcap, 2]")
            if not (n_ref.dtype == torch.int32 and tuple(n_ref.shape) == (self.S,) and n_ref.is_contiguous() and n_ref.is_cuda):
                raise ValueError("set_reference_paths: n_ref is a contiguous int32 device tensor [S]")
        self.ref_paths, self.n_ref = paths, n_ref
        self._drop_graphs()

    def enqueue_obstacles(self, stream=None, obs_cls=None):
        """obstacles="tracks" / "moving_tracks" / "filtered_tracks": the window's snapshot tables and start states (and, filtered,
        self.track_filt) -> self.obstacles / self.n_obs (av_track_obstacles / _moving / _filtered); call where the tracker's, the
        track filter's and the Kalman filter's outputs are complete (after the join).  obs_cls (a loop with a calibration only):
        int32 [S, W, tcap], filled with the class of the track behind every obstacle row (av_track_obstacles_ground_cls)."""
        if obs_cls is not None and self.ground is None:
            raise RuntimeError("enqueue_obstacles(obs_cls=...) needs a loop with a calibration")
        if self._obs_mode not in ("tracks", "moving_tracks", "filtered_tracks"):
            raise RuntimeError('enqueue_obstacles needs HotLoop(obstacles="tracks"), "moving_tracks" or "filtered_tracks"')
        if self.ground is not None:
            mode = ("tracks", "moving_tracks", "filtered_tracks").index(self._obs_mode)
            tail = (self.W, mode, self.frame_rate if mode else 0.0, self.S * self.W, self.tcap, nat.ptr(self.snap), nat.ptr(self.snap_n),
                    nat.ptr(self.track_filt) if mode == 2 else None, nat.ptr(self.plan_state), self.tcap, nat.ptr(self.obstacles),
                    nat.ptr(self.n_obs), nat.ptr(self.n_off))
            head = (self.ctx.handle, stream or self._s, C.byref(self.ocfg), nat.ptr(self.ground))
            if obs_cls is not None:
                nat.check(self.L.av_track_obstacles_ground_cls(*head, nat.ptr(self.lens), *tail, nat.ptr(obs_cls)))
            elif self.lens is not None:
                nat.check(self.L.av_track_obstacles_ground_lens(*head, nat.ptr(self.lens), *tail))
            else:
                nat.check(self.L.av_track_obstacles_ground(*head, *tail))
            return
        if self._obs_mode == "filtered_tracks":
            nat.check(self.L.av_track_obstacles_filtered(self.ctx.handle, stream or self._s, C.byref(self.ocfg), self.frame_rate,
                                                         self.S * self.W, self.tcap, nat.ptr(self.snap), nat.ptr(self.snap_n),
                                                         nat.ptr(self.track_filt), nat.ptr(self.plan_state), self.tcap,
                                                         nat.ptr(self.obstacles), nat.ptr(self.n_obs)))
            return
        tail = (self.S * self.W, self.tcap, nat.ptr(self.snap), nat.ptr(self.snap_n), nat.ptr(self.plan_state), self.tcap,
                nat.ptr(self.obstacles), nat.ptr(self.n_obs))
        if self._obs_mode == "moving_tracks":
            nat.check(self.L.av_track_obstacles_moving(self.ctx.handle, stream or self._s, C.byref(self.ocfg), self.frame_rate, *tail))
        else:
            nat.check(self.L.av_track_obstacles(self.ctx.handle, stream or self._s, C.byref(self.ocfg), *tail))

    def enqueue_track_filter(self, stream=None):
        """obstacles="filtered_tracks": the window's snapshot tables -> self.track_filt, advancing the per-track filters' state
        (av_track_filter_update); call behind the tracker, on its stream."""
        if self.track_filter is None:
            raise RuntimeError('enqueue_track_filter needs HotLoop(obstacles="filtered_tracks")')
        self.track_filter.update(self.snap, self.snap_n, out=self.track_filt, stream=stream or self._s)

    def enqueue_plan_each(self, stream=None):
        """The planner with per-state inputs (av_planner_plan_each; av_planner_plan_moving where the obstacle rows carry a
        velocity): frame (s, f) reads obstacle list (s, f) and stream s's reference path."""
        self._serial_only("enqueue_plan_each")
        rcap = 0 if self.ref_paths is None else int(self.ref_paths.shape[1])
        ocap = 0 if self.obstacles is None else int(self.obstacles.shape[2])
        moving = self.obstacles is not None and int(self.obstacles.shape[3]) == 5
        plan = self.L.av_planner_plan_moving if moving else self.L.av_planner_plan_each
        nat.check(plan(self.ctx.handle, stream or self._s, self.S * self.W, nat.ptr(self.plan_state),
                       nat.ptr(self.ref_paths), nat.ptr(self.n_ref), rcap, self.W,
                       nat.ptr(self.obstacles), nat.ptr(self.n_obs), ocap,
                       nat.ptr(self.wp), nat.ptr(self.cost), nat.ptr(self.order)))

    def set_wire(self, wire, stream0=0, frame0=0):
        """Fused step only: `wire` (uint8 device tensor [S, av_wire_table_bytes(tcap)], or None) receives every stream's
        track table in the all-gather's wire format from the same launch; header.stream = stream0 + s, header.frame =
        frame0 + the stream's detector frame count after the step."""
        if wire is not None and not (self.fused_step and self.keep_snapshots):
            raise RuntimeError("set_wire needs the fused step and keep_snapshots=True")
        self.wire, self._wire_ids = wire, (int(stream0), int(frame0))

    def enqueue_step_fused(self, stream=None):
        """Window 1: detect + track + Kalman + plan of one frame of every stream as ONE launch."""
        if self.overlap > 1:
            return self._enqueue_step_seq(stream)
        nat.check(self.L.av_hot_step(self.ctx.handle, stream or self._s, self._cloop, self._csets[0], nat.ptr(self.wire), *self._wire_ids))

    def _enqueue_step_seq(self, stream=None):
        """overlap=D: step number self._seq on stream seq % D with buffer set seq % D, ordered behind step seq - 1 per stream and
        role by the sequence flags (av_hot_step_seq)."""
        if stream is not None:
            raise RuntimeError("overlap=2.. launches on the loop's own streams")
        k = self._seq % self.overlap         # (_seq is kept modulo 2^32: the library's step numbers are 32-bit and wrap)
        self.__dict__.update(self._sets[k])  # the attributes name the set of the step enqueued last
        nat.check(self.L.av_hot_step_seq(self.ctx.handle, C.c_void_p(self._pstreams[k].cuda_stream), self._cloop, self._csets[k],
                                         nat.ptr(self.wire), *self._wire_ids, nat.ptr(self.seq_flags), self._i32(self._seq), self.overlap))
        self._seq = (self._seq + 1) & 0xFFFFFFFF
        self._stepped = True

    def enqueue_steps(self, n_steps, z_steps=None, wire_steps=None):
        """overlap=2: n_steps consecutive steps enqueued by one library call (av_hot_steps_seq: the launch loop in C).
        z_steps: None (every step reads its buffer set's z) or a float64 device tensor [n_steps, S, 4], the measurements of each
        step; wire_steps: None or a uint8 device tensor [n_steps, S, av_wire_table_bytes(tcap)] that receives every step's
        wire tables (set_wire's stream0 / frame0 apply)."""
        if self.overlap < 2:
            raise RuntimeError("enqueue_steps needs overlap=2..")
        if n_steps <= 0:
            return
        if z_steps is not None and (z_steps.dtype != torch.float64 or z_steps.numel() != n_steps * self.S * 4 or not z_steps.is_contiguous()):
            raise ValueError("z_steps: contiguous float64 [n_steps, S, 4]")
        if wire_steps is not None:
            wb = int(self.L.av_wire_table_bytes(self.tcap))
            if not (self.keep_snapshots and wire_steps.dtype == torch.uint8 and wire_steps.numel() == n_steps * self.S * wb and wire_steps.is_contiguous()):
                raise ValueError("wire_steps: contiguous uint8 [n_steps, S, %d] (and keep_snapshots=True)" % wb)
        nat.check(self.L.av_hot_steps_seq(self.ctx.handle, self.overlap, self._cstreams, self._cloop, self._csets, nat.ptr(z_steps),
                                          nat.ptr(wire_steps), *self._wire_ids, nat.ptr(self.seq_flags), self._i32(self._seq), int(n_steps)))
        self._seq = (self._seq + int(n_steps)) & 0xFFFFFFFF
        self._stepped = True
        self.__dict__.update(self._sets[((self._seq - 1) & 0xFFFFFFFF) % self.overlap])

    def tune_streams(self, pool=8, candidates=12, steps=600):
        """overlap=D: pick the D HIP streams the overlapped steps run on.  The runtime serves a process's streams from a few hardware
        queues, assigned by the process's whole stream history; launches on streams that share a queue do not overlap, and the same
        64-stream loop at depth 4 was measured at 4.9 us per step in one process and 10 us in another.  There is no way to ask for a
        queue, so the loop measures: `steps` steps (one library call) on each of `candidates` sets of D streams drawn from `pool`
        fresh ones, and keeps the fastest set.  Call it before reset() / loading state: the measured steps advance the streams'
        state, and the loop is reset afterwards.  -> us per step of every candidate set."""
        import time
        if self.overlap < 2:
            return []
        self.synchronize(check=False)
        D = self.overlap
        fresh = [torch.cuda.Stream(device=self.dev) for _ in range(max(pool, D))]
        rs = np.random.RandomState(12345)
        sets = [list(self._pstreams)] + [fresh[i:i + D] for i in range(0, len(fresh) - D + 1, D)]
        while len(sets) < candidates:
            sets.append([fresh[i] for i in sorted(rs.choice(len(fresh), D, replace=False))])
        tried = []
        for cand in sets:
            self._use_streams(cand)
            self.reset()
            self.enqueue_steps(64)
            self.synchronize()
            t0 = time.perf_counter()
            self.enqueue_steps(steps)
            self.synchronize()
            tried.append(((time.perf_counter() - t0) / steps * 1e6, cand))
        best = min(tried, key=lambda x: x[0])
        self._use_streams(best[1])
        self.reset()
        return [round(t, 2) for t, _ in tried]

    def step_stream(self):
        """The torch stream the step enqueued last runs on (overlap=2 alternates between two)."""
        return self._pstreams[((self._seq - 1) & 0xFFFFFFFF) % self.overlap] if self.overlap > 1 and self._stepped else self.stream

    def enqueue_step(self):
        """One window of the whole loop: fork{detect; track} || {kf; plan}; join.  Detections only feed the
        tracker, so both sit on the side stream and the Kalman/planner chain starts at once.  With window 1 and
        fused_step the whole step is one launch instead.  With per-state planner inputs (obstacles="tracks", set_obstacles,
        set_reference_paths) the planner runs behind the join as av_planner_plan_each."""
        if self.fused_step:
            return self.enqueue_step_fused()
        h, L, s = self.ctx.handle, self.L, self._s
        nat.check(L.av_fork(h, s))
        self.enqueue_detect(self.ctx.side_stream)
        self.enqueue_track(self.ctx.side_stream)
        if self._obs_mode == "filtered_tracks":
            self.enqueue_track_filter(self.ctx.side_stream)
        self.enqueue_kf()
        if self._per_state():
            # per-state planner inputs: fork{detect; track} || {kf}; join; [lanes -> paths]; [tracks -> obstacles]; plan.  With obstacles from the
            # tracker the planner consumes the tables, so it moves behind the join
            nat.check(L.av_join(h, s))
            if self._lanes is not None:
                self.enqueue_lane_paths()
            if self._obs_mode in ("tracks", "moving_tracks", "filtered_tracks"):
                self.enqueue_obstacles()
            self.enqueue_plan_each()
            return
        self.enqueue_plan()
        nat.check(L.av_join(h, s))

    def capture(self):
        """Capture enqueue_step() into a hipGraph (replayed by step(graph=True)).  (overlap=2: not available -- a graph would
        replay one step number.)  The fused step bakes the wire buffer's
        address into its kernel arguments, so graphs are kept per wire buffer (the exchange alternates between two)."""
        self._serial_only("capture()")
        gid = C.c_int(-1)
        nat.check(self.L.av_graph_begin(self.ctx.handle, self._s))
        try:
            self.enqueue_step()
        finally:
            nat.check(self.L.av_graph_end(self.ctx.handle, self._s, C.byref(gid)))
        self.graph_id = gid.value
        self._graphs[self._graph_key()] = gid.value
        return self.graph_id

    def _graph_key(self):
        return (self.wire.data_ptr(), self._wire_ids) if self.wire is not None else None

    def step(self, graph=False, sync=False):
        if graph:
            gid = self._graphs.get(self._graph_key())
            if gid is None:
                gid = self.capture()
            nat.check(self.L.av_graph_launch(self.ctx.handle, gid, self._s))
        else:
            self.enqueue_step()
        if sync:
            self.synchronize()

    def synchronize(self, check=True):
        for st in self._pstreams:
            st.synchronize()
        if self.overlap > 1 and check and int(self.seq_flags[64 * self.S].item()) != 0:
            raise RuntimeError("HotLoop(overlap=%d): a step waited in vain for its predecessor (sequence flags: fault word set); "
                               "the state is no longer that of a serial run -- reset()" % self.overlap)

    # ---- host views of the last window -------------------------------------------------------------
    def snapshots(self):
        """-> (rows structured array [S,W,tcap], n [S,W]) for the last window."""
        self.synchronize()
        raw = self.snap.cpu().numpy()
        rows = raw.view(np.dtype(nat.TRACK_ROW_FIELDS)).reshape(self.S, self.W, self.tcap)
        return rows, self.snap_n.cpu().numpy()

    def tracker_tables(self):
        """Persistent per-stream state: (hdr int32[S,16], rows [S,tcap], hist float64[S,tcap,L,4])."""
        self.synchronize()
        raw = self.trk_state.cpu().numpy()
        L = self.tcfg.trajectory_length
        hdr = raw[:, :nat.TRACKER_HDR_BYTES].copy().view(np.int32)
        ro = nat.TRACKER_HDR_BYTES
        rows = raw[:, ro:ro + self.tcap * 64].copy().view(np.dtype(nat.TRACK_ROW_FIELDS)).reshape(self.S, self.tcap)
        hist = raw[:, ro + self.tcap * 64:].copy().view(np.float64).reshape(self.S, self.tcap, L, 4)
        return hdr, rows, hist

    def results(self):
        self.synchronize()
        out = dict(det_n=self.det_n.cpu().numpy(), det_box=self.det_box.cpu().numpy(),
                   det_cls=self.det_cls.cpu().numpy(), det_conf=self.det_conf.cpu().numpy(),
                   det2trk=self.det2trk.cpu().numpy(), vstate=self.vstate.cpu().numpy(),
                   cost=self.cost.cpu().numpy().reshape(self.S, self.W, self.n_cand),
                   order=self.order.cpu().numpy().reshape(self.S, self.W, self.n_cand))
        if self.keep_waypoints:
            out["wp"] = self.wp.cpu().numpy().reshape(self.S, self.W, self.n_cand, self.n_points, 6)
        if self._obs_mode is not None:
            out["obstacles"], out["n_obs"] = self.obstacles.cpu().numpy(), self.n_obs.cpu().numpy()
        if self.n_off is not None:
            out["n_off"] = self.n_off.cpu().numpy()
        if self.track_filt is not None:
            out["track_filt"] = self.track_filt.cpu().numpy()
        if self._src is not None:
            out["det_dropped"] = self.det_dropped.cpu().numpy()
        if self._lanes is not None:
            out["ref_paths"], out["n_ref"] = self.ref_paths.cpu().numpy(), self.n_ref.cpu().numpy()
            out["lane_offset"] = self.lane_offset.cpu().numpy()
        return out

    # algorithmic HBM bytes of one planner launch: per start state
    # 32 B read + C*n*48 B waypoints + C*8 B costs + C*4 B order
    def planner_bytes_per_state(self):
        c, n = self.n_cand, self.n_points
        return 32 + c * n * 48 + c * 8 + c * 4


class PerceptionLoop:
    """BASELINE config 3: S camera streams, frames generated on the device, YOLO-mode detector (MFMA conv
    path) + lane detector per frame.  Everything stays in HBM; one enqueue per stage per step."""

    def __init__(self, n_streams=16, h=720, w=1280, device=0, model="random:0", max_segments=512, ctx=None, precision="fp16", names=None,
                 lens=None):
        """model: a YOLOv8 n / s / m state_dict file, a flat parameter vector or "random[:seed[:scale[:nc]]]" (perception/yolo.py);
        names: its class names, if the file carries none.  lens: one perception.LensModel or one per stream (size = (w, h)) -- the
        step's input (generated, copied or decoded) then lands in self.raw and av_remap writes its rectified picture into
        self.frames on the loop's stream before the detector, through a table built here (av_lens_map_rectify: self.lens_map
        int32 [n_maps, h, w, 2], one map if every stream has the same lens); everything behind sees rectified pixels."""
        if not torch.cuda.is_available():
            raise RuntimeError("PerceptionLoop needs a HIP device; this package has no CPU path")
        from .perception.yolo import MAX_DET, YoloV8
        self.S, self.h, self.w, self.ms = n_streams, h, w, max_segments
        self.dev = torch.device("cuda", device)
        self.L = nat.lib()
        self.yolo = YoloV8(model, device=device, batch=n_streams, precision=precision, names=names)
        self.ctx = self.yolo._dev.ctx
        self.yolo._prepare(h, w)
        # the detector chain is the critical path when the lane chain runs beside it: higher queue priority
        self.stream = torch.cuda.Stream(device=self.dev, priority=-1)
        S, d = n_streams, self.dev
        self.frames = torch.empty(S, h, w, 3, dtype=torch.uint8, device=d)
        self.raw = self.lens = self.lenses = self.lens_map = None
        self.lens_fill = (0, 0, 0)              # rectified pixels that show nothing of the raw frame
        if lens is not None:
            self._setup_lens(lens)
        self.ws = torch.empty(int(self.L.av_lane_workspace_bytes(S, h, w, max_segments)), dtype=torch.uint8, device=d)
        nat.check(self.L.av_lane_workspace_init(self.ctx.handle, self._s, S, h, w, max_segments, nat.ptr(self.ws)))
        self.lane_state = torch.zeros(S, 8, dtype=torch.float64, device=d)
        self.poly = torch.zeros(S, 2, 3, dtype=torch.float64, device=d)
        self.pts = torch.zeros(S, 2, 50, 2, dtype=torch.int32, device=d)
        self.info = torch.zeros(S, 8, dtype=torch.int32, device=d)
        self.conf = torch.zeros(S, 2, dtype=torch.float64, device=d)
        self.det_n = torch.zeros(S, dtype=torch.int32, device=d)
        self.det_box = torch.zeros(S, MAX_DET, 4, dtype=torch.float32, device=d)
        self.det_conf = torch.zeros(S, MAX_DET, dtype=torch.float32, device=d)
        self.det_cls = torch.zeros(S, MAX_DET, dtype=torch.int32, device=d)
        self.lcfg = nat.LaneCfg(50, 50, 150, max_segments, 0.7)
        self.max_det = MAX_DET
        net_h, net_w, _ = self.yolo.dims()
        # 2*MACs of every convolution at the letterboxed resolution (the figure the MFMA roofline is priced on)
        self.flops_per_frame = _yolo_flops(net_h, net_w, self.yolo.scale, self.yolo.nc)
        # HBM bytes per pixel the lane pixel stages have to move (bench.py): read BGR 3, write the non-maximum-suppressed
        # magnitudes 1, read them for the hysteresis pass 1 (the resolve / compaction passes only touch the ROI box: +0.3).
        # SURVEY 8d's 7*W*H per frame assumed the blurred image goes out to memory and back; the fused front end keeps it
        # in registers, so the chain as a whole is priced on 7*W*H and this stage on what it really needs
        self.lane_pixel_bytes_per_px = 5
        self.lane_pixel_kernels = ("front_pack (gray+blur+hist+Sobel+NMS) + thresholds + ccl_tile + ccl_border + "
                                   "finalize_fast + compact_box")
        self.frame_idx = 0
        self._lanes_pending = False
        self._tail_deferred = False
        self.stream.synchronize()

    @property
    def _s(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _setup_lens(self, lens):
        from .perception.calibration import lens_table
        S, h, w, d = self.S, self.h, self.w, self.dev
        table, self.lenses = lens_table(lens, S, d)
        for l in self.lenses:
            if l.size != (w, h):
                raise ValueError("lens: size %r is not the loop's frame size %r" % (l.size, (w, h)))
        self.lens = table                                                           # uint8 [S, 112]: av_lens_cfg per stream
        shared = all(l == self.lenses[0] for l in self.lenses)
        self.lens_stride = S if shared else 1                                       # camera k reads map k // lens_stride
        n_maps = 1 if shared else S
        with torch.cuda.stream(self.stream):
            self.raw = torch.zeros(S, h, w, 3, dtype=torch.uint8, device=d)
            self.lens_map = torch.empty(n_maps, h, w, 2, dtype=torch.int32, device=d)
            nat.check(self.L.av_lens_map_rectify(self.ctx.handle, self._s, nat.ptr(table), n_maps, h, w, nat.ptr(self.lens_map)))

    def enqueue_rectify(self):
        """self.raw -> self.frames through self.lens_map on the loop's stream (av_remap)."""
        nat.check(self.L.av_remap(self.ctx.handle, self._s, nat.ptr(self.lens_map), self.S, self.lens_stride, self.h, self.w,
                                  nat.ptr(self.raw), self.h, self.w, (C.c_uint8 * 3)(*self.lens_fill), nat.ptr(self.frames)))

    def enqueue_generate(self, stream0=0):
        nat.check(self.L.av_synth_frames(self.ctx.handle, self._s, self.S, self.h, self.w, stream0, self.frame_idx,
                                         nat.ptr(self.raw if self.lens is not None else self.frames)))
        if self.lens is not None:
            self.enqueue_rectify()
        self.frame_idx += 1

    def enqueue_frames(self, frames=None):
        """The step's input on the loop's stream.  None: generate (enqueue_generate).  A uint8 device tensor [S, h, w, 3]: copied into
        self.frames (nothing is enqueued when it IS self.frames); the caller orders whatever produced it before the loop's stream.
        An object with read_into(dst, stream) -- a loaders.VideoFeed -- decodes straight into self.frames.  frame_idx advances.
        With a lens all of that lands in self.raw (the camera's raw frames), and self.frames is its rectified picture."""
        if frames is None:
            return self.enqueue_generate()
        dst = self.raw if self.lens is not None else self.frames
        if hasattr(frames, "read_into"):
            frames.read_into(dst, self.stream)
        else:
            if (not torch.is_tensor(frames) or frames.device != dst.device or frames.dtype != torch.uint8
                    or tuple(frames.shape) != tuple(dst.shape)):
                raise ValueError("frames must be a uint8 tensor %s on %s, or an object with read_into()" % (
                    tuple(dst.shape), dst.device))
            if self.lens is not None and frames.data_ptr() == self.frames.data_ptr():
                raise ValueError("frames is the loop's rectified buffer; give raw frames (cam.raw, or a tensor of your own)")
            if frames.data_ptr() != dst.data_ptr() or not frames.is_contiguous():
                with torch.cuda.stream(self.stream):
                    dst.copy_(frames, non_blocking=True)
        if self.lens is not None:
            self.enqueue_rectify()
        self.frame_idx += 1

    def enqueue_detect(self):
        nat.check(self.L.av_yolo_forward(self.yolo._h, self._s, nat.ptr(self.frames), 0.25, 0.7, self.max_det,
                                         nat.ptr(self.det_n), nat.ptr(self.det_box), nat.ptr(self.det_conf),
                                         nat.ptr(self.det_cls)))

    def enqueue_lanes(self, stream=None, stages=0):
        """stages 0: the whole chain; nat.LANE_PIXELS_ONLY: pixel stages only (edge points left in the workspace);
        nat.LANE_HOUGH_ONLY: Hough + fit of what the last pixel-stage call left there."""
        nat.check(self.L.av_lane_detect(self.ctx.handle, stream or self._s, C.byref(self.lcfg), self.S, self.h, self.w,
                                        nat.ptr(self.frames), None, nat.ptr(self.ws), nat.ptr(self.lane_state),
                                        nat.ptr(self.poly), nat.ptr(self.pts), nat.ptr(self.info), nat.ptr(self.conf), stages))

    def step(self, sync=False, frames=None):
        """generate (or take `frames`: see enqueue_frames); fork{lanes} || {detect}; join.  The detector and the lane chain only
        share the frames: the lane chain (mostly the sequential per-frame PPHT, one CU per frame) runs beside the convolutions."""
        h = self.ctx.handle
        self.enqueue_frames(frames)
        nat.check(self.L.av_fork(h, self._s))
        self.enqueue_lanes(self.ctx.side_stream)
        self.enqueue_detect()
        nat.check(self.L.av_join(h, self._s))
        if sync:
            self.stream.synchronize()

    def tune_streams(self, candidates=8, steps=4):
        """Pick the main stream the step overlaps best on.  A step is four chains on four streams (detector main chain, Detect
        head's class branch, lane chain, deferred detector tail); the HIP runtime serves a process's streams from a few hardware
        queues per priority class, assigned by the process's whole stream history, and WHICH queues the four chains got decides
        how they overlap -- measured on MI355X / ROCm 7.2: the same 64-camera step takes 1.55 ms or 2.9 ms (tools/c3seq.py: fresh
        process 1.55; after any HotLoop was closed 2.9; with four more highest-priority streams created first 1.55 again).  The
        runtime offers no way to ask for a queue, so the loop measures: `steps` pipelined steps on each of `candidates`
        highest-priority streams (PyTorch hands its pool out round-robin), keeps the fastest.  Results do not depend on the
        stream; the generator's frame counter and the lanes' EMA state are put back afterwards.  -> ms per step of every candidate."""
        import time
        state0, idx0 = self.lane_state.clone(), self.frame_idx
        deferred = bool(self._tail_deferred)
        self.synchronize()
        tried = []
        for _ in range(max(1, candidates)):
            st = torch.cuda.Stream(device=self.dev, priority=-1)
            self.stream = st
            self._lanes_pending = False
            for _ in range(2):
                self.step_deferred()
            self.flush_lanes()
            self.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                self.step_deferred()
            self.flush_lanes()
            self.synchronize()
            tried.append(((time.perf_counter() - t0) / steps * 1e3, st))
        best = min(tried, key=lambda x: x[0])
        self.stream = best[1]
        self._lanes_pending = False
        self.lane_state.copy_(state0)
        self.frame_idx = idx0
        self.synchronize()
        self.defer_detector_tail(deferred)
        return [round(t, 4) for t, _ in tried]

    def defer_detector_tail(self, enable=True):
        """Throughput mode of the detector: decode + sort + NMS of step k beside the convolutions of step k+1
        (av_yolo_defer_tail); det_* are complete after flush_lanes() / join_detector_tail()."""
        if enable and self.yolo.precision == "fp32":
            raise RuntimeError("the float32 detector mode has no deferred tail")
        nat.check(self.L.av_yolo_defer_tail(self.yolo._h, 1 if enable else 0))
        self._tail_deferred = bool(enable)

    def join_detector_tail(self):
        nat.check(self.L.av_yolo_join_tail(self.yolo._h, self._s))

    def step_deferred(self, frames=None):
        """Throughput variant of step(): the Hough + fit half of a frame's lane chain is enqueued one step late, ahead
        of the next frame's pixel stages on the side stream.  The sharded PPHT holds 158 KB of LDS on every CU it
        runs on, which keeps the LDS-tiled convolutions off those CUs; one step late it runs beside the detector's
        preprocess + stem + first stride-2 convolution, which use no LDS.  Same kernels, same per-stream order, same
        results; the lane outputs (poly / pts / info / conf) describe the PREVIOUS frame until flush_lanes()."""
        h = self.ctx.handle
        self.enqueue_frames(frames)
        nat.check(self.L.av_fork(h, self._s))
        if self._lanes_pending:
            self.enqueue_lanes(self.ctx.side_stream, stages=nat.LANE_HOUGH_ONLY)
        self.enqueue_lanes(self.ctx.side_stream, stages=nat.LANE_PIXELS_ONLY)
        self._lanes_pending = True
        self.enqueue_detect()
        nat.check(self.L.av_join(h, self._s))

    def flush_lanes(self):
        """Hough + fit of the last frame step_deferred() left pending."""
        if self._lanes_pending:
            self.enqueue_lanes(stages=nat.LANE_HOUGH_ONLY)
            self._lanes_pending = False
        self.join_detector_tail()

    def synchronize(self):
        self.stream.synchronize()

    def enqueue_scene(self, stream=None, speeds=None, max_segments=4096):
        """Opt-in scene stage (SceneClassifier.classify for every camera, av_scene_classify) on the frames, detections and
        lane outputs in HBM: call it after step() (after flush_lanes() in the deferred mode), so that det_* and info / poly
        describe the current frames.  speeds: ego speed per camera (NaN = no vehicle state; a host array, or a float64 device
        tensor [S], which is read on the stream the stage runs on), or None for none.  The stage
        has its own workspace and 5-deep road-type history per camera; rows land in self.scene_rows."""
        from .tagging.scene_classifier import category_table
        S, d = self.S, self.dev
        if getattr(self, "scene_ws", None) is None or self.scene_cap != max_segments:
            self.scene_cap = int(max_segments)
            self.scene_ws = torch.empty(int(self.L.av_scene_workspace_bytes(S, self.h, self.w, self.scene_cap)), dtype=torch.uint8,
                                        device=d)
            nat.check(self.L.av_scene_workspace_init(self.ctx.handle, stream or self._s, S, self.h, self.w, self.scene_cap,
                                                     nat.ptr(self.scene_ws)))
            if getattr(self, "scene_state", None) is None:
                self.scene_state = torch.zeros(int(self.L.av_scene_state_bytes(S)), dtype=torch.uint8, device=d)
                self.scene_rows = torch.zeros(S, nat.SCENE_ROW_BYTES, dtype=torch.uint8, device=d)
                cat = category_table(self.yolo.names)
                self.scene_cat = torch.as_tensor(cat).to(d)
                self.scene_speed = torch.full((S,), float("nan"), dtype=torch.float64, device=d)
        sp = None
        if isinstance(speeds, torch.Tensor) and speeds.is_cuda:
            # a device tensor (e.g. the Kalman output's speed column): copied on the stream the stage runs on, no host round trip
            if speeds.dtype != torch.float64 or tuple(speeds.shape) != (S,):
                raise ValueError("speeds on the device: a float64 tensor [n_streams]")
            ts = self.stream if stream is None else torch.cuda.ExternalStream(stream.value if hasattr(stream, "value") else int(stream),
                                                                              device=d)
            with torch.cuda.stream(ts):
                self.scene_speed.copy_(speeds)
            sp = nat.ptr(self.scene_speed)
        elif speeds is not None:
            with torch.cuda.stream(self.stream):
                self.scene_speed.copy_(torch.as_tensor(np.asarray(speeds, np.float64).reshape(S)))
            sp = nat.ptr(self.scene_speed)
        nat.check(self.L.av_scene_classify(self.ctx.handle, stream or self._s, S, self.h, self.w, nat.ptr(self.frames),
                                           nat.ptr(self.scene_ws), self.scene_cap, nat.ptr(self.det_n), nat.ptr(self.det_cls),
                                           self.max_det, nat.ptr(self.scene_cat), int(self.scene_cat.numel()), sp, None,
                                           nat.ptr(self.info), nat.ptr(self.poly), nat.ptr(self.scene_state),
                                           nat.ptr(self.scene_rows)))

    def scene_results(self):
        """The last enqueue_scene's av_scene_row per camera (structured NumPy array; synchronises)."""
        self.synchronize()
        return self.scene_rows.cpu().numpy().view(nat.SCENE_ROW_FIELDS).reshape(self.S)

    def reset_scene(self):
        if getattr(self, "scene_state", None) is not None:
            nat.check(self.L.av_scene_reset(self.ctx.handle, self._s, self.S, nat.ptr(self.scene_state)))


def _yolo_flops(H, W, scale="n", nc=80):
    """2*MACs of the YOLOv8 graph (scale, nc) at input H x W (per frame), walking the same layer list as the library."""
    from .perception.yolo import conv_specs, model_dims
    specs = conv_specs(scale, nc)
    _, rep, nr, _, _ = model_dims(scale, nc)
    # downscale of every conv's OUTPUT, in execution order (a C2f block with n bottleneck pairs has 2 + 2 n convolutions)
    def c2f(n, d):
        return [d] * (2 + 2 * n)
    div = [2, 4] + c2f(rep[0], 4) + [8] + c2f(rep[1], 8) + [16] + c2f(rep[2], 16) + [32] + c2f(rep[3], 32) + [32, 32]     # backbone + SPPF
    div += c2f(nr, 16) + c2f(nr, 8) + [16] + c2f(nr, 16) + [32] + c2f(nr, 32)                                              # neck
    for d in (8, 16, 32):
        div += [d] * 6
    assert len(div) == len(specs)
    fl = 0
    for (cin, cout, k, s, _), d in zip(specs, div):
        fl += 2 * cin * cout * k * k * (H // d) * (W // d)
    return fl


# detector class name -> the reference's class id (ObjectDetector.CLASSES: the ids av_obstacle_cfg.radius and the interaction tagger
# expect); "_" in a name reads as " "
_REFERENCE_IDS = {"car": 0, "truck": 1, "person": 2, "pedestrian": 2, "bicycle": 3, "cyclist": 3, "motorcycle": 4, "bus": 5,
                  "traffic light": 6, "stop sign": 7}


def reference_class_map(names):
    """names: the detector's {id: name} dict or name list -> int32 table detector id -> reference id, -1 where the reference has
    no such class (av_dets_to_tracker's class_map)."""
    items = names.items() if isinstance(names, dict) else enumerate(names)
    items = [(int(k), str(v)) for k, v in items]
    table = np.full(max(k for k, _ in items) + 1, -1, np.int32)
    for k, v in items:
        table[k] = _REFERENCE_IDS.get(v.strip().lower().replace("_", " "), -1)
    return table


class CameraLoop:
    """S cameras from pixels to ranked trajectories with no host round trip: a PerceptionLoop (self.cam: frames -> YOLO-mode
    detector + lane detector) feeding a HotLoop of window 1 on the stage launches (self.hot: tracker -> Kalman -> planner) through
    av_dets_to_tracker and av_lane_paths.  The tracker sees the detector's boxes, the planner avoids the tracks
    (obstacles="moving_tracks" / "filtered_tracks" / "tracks" / None) and follows each camera's own lane centre line."""

    def __init__(self, n_streams, h=720, w=1280, model="random:0", precision="fp16", dcap=64, obstacles="moving_tracks",
                 class_map="reference", device=0, tracker_kw=None, kf_kw=None, planner_kw=None, obstacle_kw=None, tags=None,
                 tag_capacity=4096, view=None, tag_columns=False, names=None, track_filter_kw=None, calibration=None, ego=None,
                 ego_kw=None):
        """model, names: PerceptionLoop's (any YOLOv8 n / s / m model, e.g. "random:0:s"; names for a checkpoint without them).
        class_map: "reference" (the detector's class names -> the reference's eight ids, everything else skipped:
        reference_class_map), None (raw ids) or an explicit int table.  With names that match none of the reference's eight (a
        fine-tuned model's own classes, or the "class<i>" defaults) "reference" therefore skips EVERY detection: the tracker sees
        nothing -- pass class_map=None or a table for such a model.  obstacle_kw: HotLoop's; the defaults stretch the BEV
        panel's 640 x 500 px convention to the frame (x_center = w / 2, x_scale = 0.03 * 640 / w, y_far = 50,
        y_scale = 50 / h).  calibration: HotLoop's (one CameraCalibration or one per camera); the stretched defaults are then not
        built and obstacle_kw takes radius and frame_rate only.  enqueue_ground_view warps the frames to a bird's-eye view through
        it.  Calibrations with a lens (all cameras, or none): the step's input is the cameras' RAW frames (cam.raw), cam.frames is
        their rectified picture (av_remap through a table built once), and the detector, lanes, scene, views, tracker and the
        ground kernels see rectified pixels as without a lens.
        obstacles="filtered_tracks" and track_filter_kw: HotLoop's (the per-track Kalman filter; self.hot.track_filt).
        tags: None, "motion" or "all" -- every step() also tags its frame behind hot.step() on the hot stream and appends it to
        self.tag_log (a TagLog of tag_capacity frames per camera): "motion" runs the maneuver tagger (with the lanes' offset), the
        interaction tagger (class_map="reference" only: it needs the reference's class ids) and enqueue_tags; "all" runs the scene
        stage ahead of them (cam.enqueue_scene with the Kalman speed, read on the device) and adds its tags and the detector's
        traffic elements.  The scene stage is the expensive one, hence not the default of `tags`.
        tag_columns: the tag log also keeps the per-frame records (TagLog(columns=True)).
        view: None, "camera" or "demo" -- every step() also renders the frame it processed, behind the hot half on the hot stream
        (enqueue_view): "camera" leaves self.view_cam (uint8 [S, h, w, 3]: the frames with detections, lane area, tracks,
        info panel and detection summary as demo.py:124-136 draws them), "demo" leaves self.view (uint8 [S, th, tw, 3]: that picture
        beside the BEV panel, labelled, as create_side_by_side joins them).  The frames themselves are not touched.  The info
        panel's "FPS" line shows self.view_fps (0.0 until set).
        ego: None -- the Kalman stage's measurement is the caller's (load_measurements) -- or "ground_flow": it is measured from
        the road pixels of consecutive rectified frames (self.ego, a perception.GroundOdometry with ego_kw's settings, DESIGN 7s;
        needs calibration=).  The stage runs on the hot stream behind the wait for the camera half, in front of the Kalman stage,
        which reads its z and mode in place; load_measurements then raises, and results() has ego_motion [S, 3], ego_valid [S],
        ego_pose [S, 3] and ego_inliers [S]."""
        if tags not in (None, "motion", "all"):
            raise ValueError('tags is None, "motion" or "all"')
        if view not in (None, "camera", "demo"):
            raise ValueError('view is None, "camera" or "demo"')
        if ego not in (None, "ground_flow"):
            raise ValueError('ego is None or "ground_flow"')
        if ego is None and ego_kw is not None:
            raise ValueError('ego_kw belongs to ego="ground_flow"')
        if ego is not None and calibration is None:
            raise ValueError('ego="ground_flow" needs calibration=: the road is seen through the camera model')
        self.S, self.h, self.w = n_streams, h, w
        lenses = None
        if calibration is not None:
            from .perception.calibration import CameraCalibration, lenses_of
            lenses = lenses_of(calibration, n_streams)
            if lenses is not None:      # behind the rectification the hot half works on rectified pixels: the cameras without their lenses
                calibration = (calibration.rectified() if isinstance(calibration, CameraCalibration)
                               else [c.rectified() for c in calibration])
        self.cam = PerceptionLoop(n_streams=n_streams, h=h, w=w, device=device, model=model, precision=precision, names=names,
                                  lens=lenses)
        ok = {} if calibration is not None else dict(x_center=w / 2.0, x_scale=0.03 * 640.0 / w, y_far=50.0, y_scale=50.0 / h)
        ok.update(obstacle_kw or {})
        self.hot = HotLoop(n_streams=n_streams, window=1, h=h, w=w, dcap=dcap, device=device, tracker_kw=tracker_kw, kf_kw=kf_kw,
                           planner_kw=planner_kw, ctx=self.cam.ctx, fused_step=False, obstacles=obstacles, obstacle_kw=ok,
                           keep_waypoints=True, keep_snapshots=True, track_filter_kw=track_filter_kw,
                           calibration=calibration)          # what enqueue_bev / enqueue_view read
        if isinstance(class_map, str):
            if class_map != "reference":
                raise ValueError('class_map is "reference", None or an int table')
            class_map = reference_class_map(self.cam.yolo.names)
        self.class_map = class_map
        c, S = self.cam, n_streams
        self.hot.set_detections(c.det_n.view(S, 1), c.det_box.view(S, 1, c.max_det, 4), c.det_conf.view(S, 1, c.max_det),
                                c.det_cls.view(S, 1, c.max_det), class_map=class_map)
        self.hot.set_lane_inputs(c.poly, c.pts, c.info)
        self.ego = None
        if ego is not None:
            from .perception.ground_odometry import GroundOdometry
            self.ego = GroundOdometry(calibration, n_streams, h, w, device=device, ctx=self.cam.ctx, **(ego_kw or {}))
            self.hot.set_measurement_source(self.ego.z.view(S, 1, 4), self.ego.mode.view(S, 1),
                                            producer=lambda stream: self.ego.enqueue(c.frames, stream))
        self._stepped = False
        self.tags, self.tag_log = tags, None
        if tags is not None:
            from .perception.detector import ObjectDetector
            from .tagging.tag_log import element_table
            self.tag_log = self.hot.enable_tag_log(tag_capacity, columns=tag_columns)
            self._tag_interactions = isinstance(class_map, np.ndarray) and np.array_equal(class_map, reference_class_map(c.yolo.names))
            self._tag_classes = [ObjectDetector.CLASSES[k] for k in range(8)]
            self._elem_table = torch.as_tensor(element_table(c.yolo.names)).to(self.hot.dev) if tags == "all" else None
        self.view_mode, self.view_fps = view, 0.0
        self.view = self.view_cam = None
        self.ground_view = None                 # enqueue_ground_view
        self._ground_map = None                 # (geometry, av_lens_map_ground's table): enqueue_ground_view(source="raw")
        if view is not None:
            self._setup_view()

    VIEW_LABELS = ("Camera View", "Bird's Eye View")         # demo.py:149

    def _setup_view(self):
        """Device tables and buffers of enqueue_view: the name and colour tables go up once, the argument block is made once."""
        from .perception.detector import ObjectDetector
        cam, hot, S, d = self.cam, self.hot, self.S, self.hot.dev
        is_ref = isinstance(self.class_map, np.ndarray) and np.array_equal(self.class_map, reference_class_map(cam.yolo.names))
        det_tab, det_len = nat.name_table(cam.yolo.names, "detector class names")
        trk_tab, trk_len = nat.name_table(ObjectDetector.CLASSES if is_ref else cam.yolo.names, "track class names")
        colors = np.array([ObjectDetector.CLASS_COLORS[k] for k in range(len(ObjectDetector.CLASS_COLORS))], np.uint8)
        max_name = int(max(det_len.max(), trk_len.max(), 0))
        L = hot.tcfg.trajectory_length
        cap = int(self.hot.L.av_camview_prim_cap(cam.max_det, hot.tcap, L, max_name))
        if cap <= 0 or cap > 65535:
            raise ValueError("view: a camera's list may need %d primitives (max_det %d, tcap %d, trajectory_length %d), the rasteriser "
                             "takes 65535" % (cap, cam.max_det, hot.tcap, L))
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(d)       # noqa: E731
        self._view_tabs = [up(a) for a in (det_tab, det_len, colors, trk_tab, trk_len)]
        self._view_cap, self._view_vcap = cap, 128
        self._view_prims = torch.zeros(S, cap, nat.PRIM_BYTES, dtype=torch.uint8, device=d)
        self._view_n = torch.zeros(S, dtype=torch.int32, device=d)
        self._view_verts = torch.zeros(S, self._view_vcap, 2, dtype=torch.int32, device=d)
        tabs = self._view_tabs
        self._view_args = nat.CamviewArgs(
            n_streams=S, h=self.h, w=self.w, flags=nat.VIEW_DEMO, n_frames=1, frame=0, max_det=cam.max_det, tcap=hot.tcap,
            trajectory_length=L, max_name=max_name, n_det_names=len(det_len), n_det_colors=len(colors), n_trk_names=len(trk_len),
            fps=0.0, det_n=cam.det_n.data_ptr(), det_box=cam.det_box.data_ptr(), det_conf=cam.det_conf.data_ptr(),
            det_cls=cam.det_cls.data_ptr(), det_names=tabs[0].data_ptr(), det_name_len=tabs[1].data_ptr(), det_colors=tabs[2].data_ptr(),
            lane_pts=cam.pts.data_ptr(), lane_info=cam.info.data_ptr(), snap=hot.snap.data_ptr(), snap_n=hot.snap_n.data_ptr(),
            tracker_state=hot.trk_state.data_ptr(), trk_names=tabs[3].data_ptr(), trk_name_len=tabs[4].data_ptr(),
            vstate=hot.vstate.data_ptr())
        self._view_geom = None
        if self.view_mode == "demo":
            from .visualization.bev_renderer import BEVRenderer
            r = BEVRenderer(device=d.index)
            th, nw1, nw2 = C.c_int(), C.c_int(), C.c_int()
            nat.check(hot.L.av_view_compose_size(self.h, self.w, r.height, r.width, C.byref(th), C.byref(nw1), C.byref(nw2)))
            self._view_geom = (th.value, nw1.value, nw2.value, r.height, r.width)
            self.view = torch.zeros(S, th.value, nw1.value + nw2.value, 3, dtype=torch.uint8, device=d)
        if self.view_mode == "camera" or self._view_geom[0] != self.h:
            # "demo" with a camera picture shorter than the panel: the painted frames are resized, so they are staged here
            self.view_cam = torch.zeros(S, self.h, self.w, 3, dtype=torch.uint8, device=d)
        torch.cuda.current_stream(d).synchronize()          # the buffers are zero-filled before the hot stream writes them

    def enqueue_view(self, fps=0.0, layers=None):
        """Render what the last step() left in HBM, on the hot stream (call it behind hot.step(); step() does when `view` is
        set): av_camview_build writes every camera's primitive list, the rasteriser paints it from cam.frames into self.view_cam
        or straight into the camera half of self.view (av_raster_draw_to: the frames are read, never written), and for "demo"
        HotLoop.enqueue_bev and av_view_compose add the panel and the labels.  layers: a sum of nat.VIEW_* bits, None = the
        layers demo.py draws (nat.VIEW_DEMO: no lane-offset gauge)."""
        if self.view_mode is None:
            raise RuntimeError('enqueue_view needs CameraLoop(view="camera") or view="demo"')
        hot, cam, L, a = self.hot, self.cam, self.hot.L, self._view_args
        a.fps, a.flags = float(fps), nat.VIEW_DEMO if layers is None else int(layers)
        h, st, S = hot.ctx.handle, hot._s, self.S
        nat.check(L.av_camview_build(h, st, C.byref(a), nat.ptr(self._view_prims), self._view_cap, nat.ptr(self._view_n),
                                     nat.ptr(self._view_verts), self._view_vcap))
        staged = self.view_cam is not None
        dst, pitch = (self.view_cam, self.w) if staged else (self.view, self.view.shape[2])
        nat.check(L.av_raster_draw_to(h, st, S, self.h, self.w, nat.ptr(cam.frames), self.w, nat.ptr(dst), pitch, 0,
                                      nat.ptr(self._view_prims), self._view_cap, nat.ptr(self._view_n), nat.ptr(self._view_verts),
                                      self._view_vcap))
        if self.view_mode == "demo":
            _, _, _, bh, bw = self._view_geom
            with torch.cuda.stream(hot.stream):             # the panel's buffers, made at the first call, are filled on that stream too
                hot.enqueue_bev()
            nat.check(L.av_view_compose(h, st, S, nat.ptr(self.view_cam) if staged else None, self.h, self.w, nat.ptr(hot.bev), bh, bw,
                                        nat.ptr(self.view), self.VIEW_LABELS[0].encode(), self.VIEW_LABELS[1].encode()))

    def enqueue_ground_view(self, gh=500, gw=640, f_far=50.0, m_per_px=0.1, fill=(0, 0, 0), source="frames"):
        """The frames of the last step() seen from above, on the hot stream (call it behind step(); the next cam.step() waits for
        that stream): self.ground_view uint8 [S, gh, gw, 3], row 0 at f_far metres ahead, m_per_px metres per pixel, the camera's
        axis down the middle column (av_ground_warp through every camera's own calibration; `fill` where the road point is above
        the horizon or outside the frame).  cam.frames is read, never written.
        source="raw" (a loop with lenses only): the view is taken straight from cam.raw through the composed table road point ->
        rectified pixel -> raw position (av_lens_map_ground, built at the first call with a geometry, then av_remap): one
        interpolation instead of two."""
        hot = self.hot
        if hot.ground is None:
            raise RuntimeError("enqueue_ground_view needs CameraLoop(calibration=...)")
        if source not in ("frames", "raw"):
            raise ValueError('source is "frames" or "raw"')
        if source == "raw" and self.cam.lens is None:
            raise ValueError('enqueue_ground_view(source="raw") needs calibrations with a lens; without one cam.frames IS the raw frame')
        gh, gw = int(gh), int(gw)
        if self.ground_view is None or tuple(self.ground_view.shape[1:3]) != (gh, gw):
            with torch.cuda.stream(hot.stream):         # zero-filled on the stream that writes it
                self.ground_view = torch.zeros(self.S, gh, gw, 3, dtype=torch.uint8, device=hot.dev)
        if source == "raw":
            geom = (gh, gw, float(f_far), float(m_per_px))
            if self._ground_map is None or self._ground_map[0] != geom:
                with torch.cuda.stream(hot.stream):
                    table = torch.empty(self.S, gh, gw, 2, dtype=torch.int32, device=hot.dev)
                nat.check(hot.L.av_lens_map_ground(hot.ctx.handle, hot._s, nat.ptr(self.cam.lens), nat.ptr(hot.ground), self.S, gh, gw,
                                                   geom[2], geom[3], nat.ptr(table)))
                self._ground_map = (geom, table)
            nat.check(hot.L.av_remap(hot.ctx.handle, hot._s, nat.ptr(self._ground_map[1]), self.S, 1, self.h, self.w,
                                     nat.ptr(self.cam.raw), gh, gw, (C.c_uint8 * 3)(*[int(c) for c in fill]),
                                     nat.ptr(self.ground_view)))
            return
        nat.check(hot.L.av_ground_warp(hot.ctx.handle, hot._s, nat.ptr(hot.ground), self.S, self.h, self.w, nat.ptr(self.cam.frames),
                                       gh, gw, float(f_far), float(m_per_px), (C.c_uint8 * 3)(*[int(c) for c in fill]),
                                       nat.ptr(self.ground_view)))

    def load_measurements(self, z):
        """z: float64 [S, 1, 4] (or [S, 4]) ego measurements of the next step (HotLoop.load_measurements)."""
        if self.ego is not None:
            raise RuntimeError('CameraLoop(ego="ground_flow") measures the ego motion from the frames: there is nothing to load')
        self.hot.load_measurements(z)

    def step(self, sync=False, frames=None):
        """cam.step(frames=frames); hot.step() behind it.  The camera half of the next step overwrites what the hot half reads (det_*,
        poly, pts, info -- and cam.frames, which the view and the scene stage read there), so it first waits for the hot half of this
        one; the decode or copy of given `frames` (PerceptionLoop.enqueue_frames) is enqueued behind that wait like the generator."""
        if self.cam._tail_deferred or self.cam._lanes_pending:
            raise RuntimeError("CameraLoop steps the plain PerceptionLoop.step(): with a deferred detector tail or a pending lane "
                               "half det_* / poly describe the previous frame")
        if self._stepped:
            self.cam.stream.wait_stream(self.hot.stream)
        self.cam.step(frames=frames)
        self.hot.stream.wait_stream(self.cam.stream)
        self.hot.step()
        if self.tags is not None:
            self._enqueue_tags()
        if self.view_mode is not None:
            self.enqueue_view(fps=self.view_fps)
        self._stepped = True
        if sync:
            self.synchronize()

    def _enqueue_tags(self):
        """The taggers and the log append behind hot.step(), all on the hot stream: it has waited for the camera half, and the next
        cam.step() waits for it, so the scene stage may read the frames, detections and lane fits there."""
        hot, cam, S = self.hot, self.cam, self.S
        scene = det = None
        with torch.cuda.stream(hot.stream):         # the stages' buffers, made at the first call, are zero-filled on that stream too
            if self.tags == "all":
                cam.enqueue_scene(stream=hot._s, speeds=hot.vstate[:, 0, 5])
                scene, det = cam.scene_rows.view(S, 1, -1), (cam.det_n.view(S, 1), cam.det_cls.view(S, 1, cam.max_det))
            hot.enqueue_maneuver(lane_offset=hot.lane_offset)
            if self._tag_interactions:
                hot.enqueue_interactions(frame_shape=(self.h, self.w), class_names=self._tag_classes)
            hot.enqueue_tags(scene_rows=scene, det=det, elem_table=self._elem_table)

    def synchronize(self):
        self.cam.synchronize()
        self.hot.synchronize()

    def results(self):
        """HotLoop.results() of the last step: with det_dropped [S, 1], ref_paths [S, 50, 2], n_ref [S] and lane_offset [S]; with
        ego="ground_flow" also ego_motion [S, 3] (t_f, t_l, omega), ego_valid [S], ego_pose [S, 3] and ego_inliers [S]."""
        out = self.hot.results()
        if self.ego is not None:
            e = self.ego.results()
            out["ego_motion"], out["ego_valid"], out["ego_pose"], out["ego_inliers"] = e["motion"], e["valid"], e["pose"], e["n_inliers"]
        return out


class RigLoop:
    """V vehicles with K cameras each (perception.CameraRig), one plan per vehicle around everything any of its cameras sees, with
    no host round trip: a CameraLoop of V * K cameras driven stage by stage up to the per-camera obstacle lists (self.cams: camera
    v * K + k is camera k of vehicle v; its start states are held at zero, so the lists stand in each camera's own road frame, and
    its Kalman and planner stages are never enqueued), av_rig_fuse carrying them through the mounts into the vehicle frame and
    merging the objects seen by several cameras, and a HotLoop of V ego states (self.ego) that plans around the fused lists."""

    _OUT_OF_SCOPE = {"fused_step": "the one-launch step plans without obstacles", "overlap": "the overlapped loop plans without obstacles",
                     "graph": "graph capture of a RigLoop is not supported", "graphs": "graph capture of a RigLoop is not supported",
                     "view": "the annotated views describe one camera, not a rig",
                     "views": "the annotated views describe one camera, not a rig"}

    def __init__(self, n_vehicles, rig, h=720, w=1280, model="random:0", precision="fp16", dcap=64, obstacles="moving_tracks",
                 class_map="reference", lane_camera=0, fuse_kw=None, tracker_kw=None, kf_kw=None, planner_kw=None, obstacle_kw=None,
                 track_filter_kw=None, names=None, device=0, track=False, rig_track_kw=None, tags=None, tag_capacity=4096,
                 tag_columns=False, ego=None, ego_kw=None, lanes=None, lanes_kw=None, marks=False, marks_kw=None, plan=None, lane_plan_kw=None,
                 **other):
        """rig: a perception.CameraRig.  obstacles: "moving_tracks", "filtered_tracks" or "tracks", CameraLoop's modes (a rig
        without obstacles has nothing to fuse).  lane_camera: the index of the camera whose lane fit is the vehicle's reference path
        (av_lane_paths_ground through rig.vehicle_calibration(lane_camera)), None for no path; its mount may not be yawed beyond
        +-pi/2, since a path behind the vehicle is none.  fuse_kw: av_rig_cfg's merge_scale and merge_min (1.0, 1.0 m).  Everything
        else is CameraLoop's; kf_kw and planner_kw go to the ego loop.  The one-launch step, the overlapped loop, graph capture
        and the per-camera annotated views are refused by name; the rig's own picture is enqueue_surround_view().
        track=True: a tracking.RigTracker follows the fused lists (av_rig_track behind av_rig_fuse, on the ego stream) and the
        ego loop plans around its confirmed tracks -- ids that persist across frames and cameras, coasting through the frames in
        which no camera sees an object.  rig_track_kw: RigTracker's settings (av_rig_track_cfg's fields; dt defaults to the ego
        Kalman filter's) and tcap (default min(512, K * the cameras' tcap)).
        tags="motion" (with track=True only: the rig's taggers read the vehicle-frame tracks): every step logs one tag mask per
        vehicle into self.tag_log (a TagLog of tag_capacity frames per vehicle on the ego stream; tag_columns: with the per-frame
        records), with no host round trip -- the class of every track travels beside the obstacle rows through the cameras' lists,
        the fuse and the tracker (the _cls entry points), the maneuver tagger runs on the ego filter's output with the lane
        camera's offset, and, when class_map is the reference map (CameraLoop's rule), av_rig_interact tags the tracks
        (self.tagger, a tagging.RigInteractionDetector).  tags="all" is refused: the scene classifier describes one camera.
        ego: None -- the ego Kalman stage's measurement is the caller's (load_measurements) -- or "ground_flow": it is measured
        from the road pixels of all K cameras' consecutive rectified frames, fitted together in the vehicle frame
        (self.odometry, a perception.RigOdometry with ego_kw's settings; a rig with lenses is refused, as
        CameraLoop(ego=) refuses one).  The stages are enqueued on the ego stream in front of av_kf_step, which reads their z and
        mode in place; load_measurements then raises, and results() has ego_motion [V, 3], ego_valid [V], ego_pose [V, 3] (the
        vehicle origin's), ego_inliers [V] and ego_views [V] (bit k: camera k has an inlier).
        lanes: None -- the reference path is the lane camera's, above -- or "road": the lane boundaries are found in metres in the
        vehicle frame from the Hough segments of all K cameras (self.road_lanes, a perception.RoadLanes with lanes_kw's settings:
        av_road_lanes_cfg's fields and scap), read in place from the cameras' lane workspace and followed from frame to
        frame through the measured ego motion when ego="ground_flow".  It fills ref_paths / n_ref / lane_offset in the lane camera's
        place, so lane_camera stays None or its default, and results() gains lane_bounds, lane_left, lane_right, lane_width,
        lane_heading, lane_curvature, lane_count, lane_index, lane_views and lane_status.  A rig with lenses is welcome: the lane
        chain sees rectified frames, so its segments are rectified pixels.
        marks=True (with lanes="road" only: the marks are read along its boundaries): every boundary is classified solid or dashed,
        white or yellow, from the rectified frames of all K cameras, and the ego lane's two sides are held over frames
        (self.road_marks, a perception.RoadMarks with marks_kw's settings: av_road_marks_cfg's fields), on the ego stream
        behind the road lanes.  results() gains lane_mark_left / _right, lane_colour_left / _right, may_change_left / _right and
        bound_marks.
        plan: None -- the plan is the planner's own ranking -- or "lanes" (with lanes="road" only; with or without marks=True: without,
        every line's type is unknown): behind the planner every candidate is charged for the lane boundaries it crosses, by their
        marks, and the candidates are ranked again (self.lane_plan, a planning.LanePlanner with lane_plan_kw's settings:
        av_lane_plan_cfg's fields).  The planner's wp, cost and order are read and never written; results() gains lane_cost,
        plan_total, plan_order, plan_best, plan_maneuver, plan_delta, plan_crossed, plan_flags and plan_lines, and the surround view's
        overlay draws the trajectory chosen here."""
        from .perception.calibration import CameraRig, ground_table
        from .tracking.rig_tracker import RigTracker, check_shape, rig_track_cfg
        for k in other:
            if k in self._OUT_OF_SCOPE:
                raise ValueError("RigLoop: %s is out of scope (%s)" % (k, self._OUT_OF_SCOPE[k]))
            raise TypeError("RigLoop() got an unexpected keyword argument %r" % k)
        if not isinstance(rig, CameraRig):
            raise ValueError("RigLoop: rig is a perception.CameraRig")
        if ego not in (None, "ground_flow"):
            raise ValueError('RigLoop: ego is None or "ground_flow"')
        if ego is None and ego_kw is not None:
            raise ValueError('RigLoop: ego_kw belongs to ego="ground_flow"')
        if ego is not None:
            from .perception.ground_odometry import egoflow_cfg
            egoflow_cfg(**(ego_kw or {}))                                           # (ValueError for a bad geometry)
        if obstacles not in ("moving_tracks", "filtered_tracks", "tracks"):
            raise ValueError('RigLoop: obstacles is "moving_tracks", "filtered_tracks" or "tracks"')
        V, K = int(n_vehicles), rig.K
        if V < 1:
            raise ValueError("RigLoop: n_vehicles must be >= 1")
        if lanes not in (None, "road"):
            raise ValueError('RigLoop: lanes is None or "road"')
        if lanes is None and lanes_kw is not None:
            raise ValueError('RigLoop: lanes_kw belongs to lanes="road"')
        if lanes is not None:
            from .perception.road_lanes import check_shape as check_lanes_shape, road_lanes_cfg
            if lanes_kw is not None and not isinstance(lanes_kw, dict):
                raise ValueError("RigLoop: lanes_kw is None or a dict of av_road_lanes_cfg's fields and scap")
            if lane_camera is not None and not (isinstance(lane_camera, (int, np.integer)) and not isinstance(lane_camera, bool)
                                                and lane_camera == 0):
                raise ValueError('RigLoop: lanes="road" takes the lanes from every camera and lane_camera=%r asks for one camera\'s: '
                                 "leave lane_camera at None or its default" % (lane_camera,))
            lane_camera = None
            lkw = dict(lanes_kw or {})
            lanes_scap = lkw.pop("scap", None)
            road_lanes_cfg(**lkw)                                                   # (ValueError for a setting outside its range)
            if lanes_scap is not None:
                check_lanes_shape(V, K, 1 << 20, lanes_scap)
        if not isinstance(marks, (bool, np.bool_)):
            raise ValueError("RigLoop: marks is True or False")
        if marks and lanes is None:
            raise ValueError('RigLoop: marks=True needs lanes="road": the marks are read along the road lanes\' boundaries')
        if marks_kw is not None and not marks:
            raise ValueError("RigLoop: marks_kw belongs to marks=True")
        if marks:
            from .perception.road_marks import check_shape as check_marks_shape, road_marks_cfg
            if marks_kw is not None and not isinstance(marks_kw, dict):
                raise ValueError("RigLoop: marks_kw is None or a dict of av_road_marks_cfg's fields")
            road_marks_cfg(**(marks_kw or {}))                                      # (ValueError for a setting outside its range)
            check_marks_shape(V, K, h, w)
        if plan not in (None, "lanes"):
            raise ValueError('RigLoop: plan is None or "lanes"')
        if plan is not None and lanes is None:
            raise ValueError('RigLoop: plan="lanes" needs lanes="road": the candidates are ranked against the road lanes\' boundaries')
        if lane_plan_kw is not None and plan is None:
            raise ValueError('RigLoop: lane_plan_kw belongs to plan="lanes"')
        if plan is not None:
            from .planning.lane_planner import lane_plan_cfg
            if lane_plan_kw is not None and not isinstance(lane_plan_kw, dict):
                raise ValueError("RigLoop: lane_plan_kw is None or a dict of av_lane_plan_cfg's fields")
            lane_plan_cfg(**(lane_plan_kw or {}))                                   # (ValueError for a setting outside its range)
        if lane_camera is not None:
            if not (isinstance(lane_camera, (int, np.integer)) and 0 <= lane_camera < K):
                raise ValueError("RigLoop: lane_camera is None or a camera index 0 .. %d" % (K - 1))
            yaw = float(np.arctan2(np.sin(rig.mounts[lane_camera, 2]), np.cos(rig.mounts[lane_camera, 2])))
            if abs(yaw) > np.pi / 2:
                raise ValueError("RigLoop: lane_camera %d is yawed %.1f degrees from the vehicle's forward axis, beyond +-90: its lane "
                                 "lies behind the vehicle, and a reference path there is no path (on_road wants forward >= 0)"
                                 % (lane_camera, np.degrees(yaw)))
        fk = dict(merge_scale=1.0, merge_min=1.0)
        fk.update(fuse_kw or {})
        if sorted(fk) != ["merge_min", "merge_scale"]:
            raise ValueError("RigLoop: fuse_kw takes merge_scale and merge_min")
        if not all(np.isfinite(float(v)) and float(v) >= 0.0 for v in fk.values()):
            raise ValueError("RigLoop: merge_scale and merge_min must be >= 0 and finite")
        self.fcfg = nat.RigCfg(float(fk["merge_scale"]), float(fk["merge_min"]))
        if not isinstance(track, (bool, np.bool_)):
            raise ValueError("RigLoop: track is True or False")
        if rig_track_kw is not None and not track:
            raise ValueError("RigLoop: rig_track_kw needs track=True")
        tkw = dict(rig_track_kw or {})
        track_tcap = tkw.pop("tcap", None)
        if track:
            rig_track_cfg(**tkw)                                                    # (ValueError for a setting outside its range)
            if track_tcap is not None:
                if isinstance(track_tcap, bool) or not isinstance(track_tcap, (int, np.integer)):
                    raise ValueError("RigLoop: rig_track_kw's tcap is an integer")
                check_shape(V, track_tcap, 3)
        if tags not in (None, "motion", "all"):
            raise ValueError('RigLoop: tags is None or "motion"')
        if tags == "all":
            raise ValueError('RigLoop: tags="all" is out of scope (the scene classifier describes one camera, not a rig)')
        if tags is not None and not track:
            raise ValueError("RigLoop: tags need track=True: the rig's taggers read the vehicle-frame tracks")
        if tags is not None and (isinstance(tag_capacity, bool) or not isinstance(tag_capacity, (int, np.integer)) or tag_capacity < 1):
            raise ValueError("RigLoop: tag_capacity is an integer >= 1")
        self.V, self.K, self.rig, self.h, self.w, self.lane_camera = V, K, rig, h, w, lane_camera
        self.cams = CameraLoop(V * K, h=h, w=w, model=model, precision=precision, dcap=dcap, obstacles=obstacles, class_map=class_map,
                               device=device, tracker_kw=tracker_kw, planner_kw=planner_kw, obstacle_kw=obstacle_kw, names=names,
                               track_filter_kw=track_filter_kw, calibration=rig.calibrations(V))
        hot = self.cams.hot
        self.ego = HotLoop(V, window=1, h=h, w=w, device=device, kf_kw=kf_kw, planner_kw=planner_kw, ctx=self.cams.cam.ctx,
                           fused_step=False, keep_waypoints=True)
        self.L, self.dev, self.tcap = self.ego.L, self.ego.dev, hot.tcap
        self.cols = int(hot.obstacles.shape[3])
        d, i32, f64 = self.dev, torch.int32, torch.float64
        if K * self.tcap > 512:
            raise ValueError("RigLoop: %d cameras x %d tracks exceed av_rig_fuse's 512 clusters" % (K, self.tcap))
        self.mounts = rig.mounts_table(V, d)                                        # float64 [V, K, 4]
        self.obstacles = torch.zeros(V, 1, K * self.tcap, self.cols, dtype=f64, device=d)
        self.n_obs = torch.zeros(V, 1, dtype=i32, device=d)
        self.views = torch.zeros(V, K * self.tcap, dtype=i32, device=d)
        self.n_skip = torch.zeros(V, dtype=i32, device=d)
        self.tracker = None
        if track:
            tkw.setdefault("dt", float(self.ego.kcfg.dt))
            self.tracker = RigTracker(V, tcap=min(512, K * self.tcap) if track_tcap is None else int(track_tcap), ncol=self.cols,
                                      ctx=self.ego.ctx, **tkw)
            self.tracker.match = torch.full((V, K * self.tcap), -1, dtype=i32, device=d)      # (results() may come before a step)
            self.ego.set_obstacles(self.tracker.obstacles.view(V, 1, self.tracker.tcap, self.cols), self.tracker.n_obs.view(V, 1))
        else:
            self.ego.set_obstacles(self.obstacles, self.n_obs)
        self.ref_paths = self.n_ref = self.lane_offset = self.lane_ground = None
        if lane_camera is not None:
            # the frames behind a lens are rectified before the lane detector sees them: the vehicle calibration without its lens
            self.lane_ground = ground_table(rig.vehicle_calibration(lane_camera).rectified(), V, d)[0]
            self._lane_idx = torch.arange(V, dtype=torch.int64, device=d) * K + int(lane_camera)
            self._poly = torch.zeros(V, 2, 3, dtype=f64, device=d)
            self._pts = torch.zeros(V, 2, 50, 2, dtype=i32, device=d)
            self._info = torch.zeros(V, 8, dtype=i32, device=d)
            self.ref_paths = torch.zeros(V, 50, 2, dtype=f64, device=d)
            self.n_ref = torch.zeros(V, dtype=i32, device=d)
            self.lane_offset = torch.full((V,), float("nan"), dtype=f64, device=d)
            self.ego.set_reference_paths(self.ref_paths, self.n_ref)
        self.road_lanes = None
        if lanes is not None:
            from .perception.road_lanes import RoadLanes
            cam = self.cams.cam
            self.road_lanes = RoadLanes(rig, V, h, w, max_segments=cam.ms, scap=min(256, cam.ms) if lanes_scap is None else int(lanes_scap),
                                        ctx=self.ego.ctx, device=device, **lkw)
            # the cameras' segment lists and counts where the lane chain leaves them: views into its workspace, no copy
            off, nb = C.c_size_t(), C.c_size_t()
            nat.check(self.L.av_lane_workspace_view(nat.LANE_VIEW_SEGMENTS, V * K, h, w, cam.ms, C.byref(off), C.byref(nb)))
            self.lane_segments = cam.ws[off.value:off.value + nb.value].view(i32).view(V * K, cam.ms, 4)
            nat.check(self.L.av_lane_workspace_view(nat.LANE_VIEW_NSEG, V * K, h, w, cam.ms, C.byref(off), C.byref(nb)))
            self.lane_nseg = cam.ws[off.value:off.value + nb.value].view(i32).view(V * K)
            self.ref_paths, self.n_ref, self.lane_offset = self.road_lanes.ref_paths, self.road_lanes.n_ref, self.road_lanes.lane_offset
            self.ego.set_reference_paths(self.ref_paths, self.n_ref)
        self.road_marks = None
        if marks:
            from .perception.road_marks import RoadMarks
            self.road_marks = RoadMarks(rig, V, h, w, ctx=self.ego.ctx, device=device, **(marks_kw or {}))
        self.lane_plan = None
        if plan is not None:
            from .planning.lane_planner import LanePlanner
            self.lane_plan = LanePlanner(V, self.ego.n_cand, self.ego.n_points, ctx=self.ego.ctx, device=device, **(lane_plan_kw or {}))
        self.surround_view = self.surround_cover = None     # enqueue_surround_view
        self._surround = self._surround_key = self._surround_ids = None
        self.surround_age = self.road_memory = None         # enqueue_surround_view(memory=True)
        self._stepped = False
        self.odometry = None
        if ego is not None:
            from .perception.rig_odometry import RigOdometry
            self.odometry = RigOdometry(rig, V, h, w, device=device, ctx=self.ego.ctx, **(ego_kw or {}))
            self.ego.set_measurement_source(self.odometry.z.view(V, 1, 4), self.odometry.mode.view(V, 1),
                                            producer=lambda stream: self.odometry.enqueue(self.cams.cam.frames, stream))
        self.tags, self.tag_log, self.tagger = tags, None, None
        if tags is not None:
            from .perception.detector import ObjectDetector
            from .tagging.rig_interaction_detector import RigInteractionDetector
            from .tagging.tag_log import TagLog
            # the class lanes beside the cameras' lists and the fused list (the tracker holds its own, tracker.cls)
            self.cam_cls = torch.full((V * K, 1, self.tcap), -1, dtype=i32, device=d)
            self.fused_cls = torch.full((V, K * self.tcap), -1, dtype=i32, device=d)
            cm = self.cams.class_map
            if isinstance(cm, np.ndarray) and np.array_equal(cm, reference_class_map(self.cams.cam.yolo.names)):
                self.tagger = RigInteractionDetector(V, self.tracker.tcap, class_names=ObjectDetector.CLASSES, ctx=self.ego.ctx,
                                                     dt=float(self.ego.kcfg.dt), min_hits=int(self.tracker.cfg.min_hits))
            self.tag_log = TagLog(V, int(tag_capacity), device=d.index, ctx=self.ego.ctx, stream=self.ego.stream,
                                  columns=bool(tag_columns))
        torch.cuda.current_stream(d).synchronize()          # the buffers are filled before the loops' streams touch them

    def load_measurements(self, z):
        """z: float64 [V, 1, 4] (or [V, 4]) ego measurements of the next step (HotLoop.load_measurements)."""
        if self.odometry is not None:
            raise RuntimeError('RigLoop(ego="ground_flow") measures the ego motion from the frames: there is nothing to load')
        self.ego.load_measurements(z)

    def enqueue_fuse(self, stream=None):
        """The cameras' lists (self.cams.hot.obstacles / n_obs) and the ego start states -> self.obstacles / n_obs / views / n_skip
        (av_rig_fuse); call behind the cameras' enqueue_obstacles and the ego's enqueue_kf.  With tags also self.cam_cls ->
        self.fused_cls (av_rig_fuse_cls)."""
        hot, ego = self.cams.hot, self.ego
        if self.tags is not None:
            nat.check(self.L.av_rig_fuse_cls(ego.ctx.handle, stream or ego._s, C.byref(self.fcfg), self.V, self.K, nat.ptr(self.mounts),
                                             self.cols, self.tcap, nat.ptr(hot.obstacles), nat.ptr(hot.n_obs), nat.ptr(self.cam_cls),
                                             nat.ptr(ego.plan_state), self.K * self.tcap, nat.ptr(self.obstacles), nat.ptr(self.n_obs),
                                             nat.ptr(self.views), nat.ptr(self.n_skip), nat.ptr(self.fused_cls)))
            return
        nat.check(self.L.av_rig_fuse(ego.ctx.handle, stream or ego._s, C.byref(self.fcfg), self.V, self.K, nat.ptr(self.mounts), self.cols,
                                     self.tcap, nat.ptr(hot.obstacles), nat.ptr(hot.n_obs), nat.ptr(ego.plan_state), self.K * self.tcap,
                                     nat.ptr(self.obstacles), nat.ptr(self.n_obs), nat.ptr(self.views), nat.ptr(self.n_skip)))

    def enqueue_rig_track(self, stream=None):
        """track=True: the fused lists, their views and the ego start states -> self.tracker's obstacles / n_obs / obs_slot / match /
        n_skip / n_drop (av_rig_track); call behind enqueue_fuse on the same stream."""
        if self.tracker is None:
            raise RuntimeError("enqueue_rig_track needs RigLoop(track=True)")
        self.tracker.update(self.obstacles, self.n_obs, self.ego.plan_state, views=self.views, stream=stream or self.ego._s,
                            cls=self.fused_cls if self.tags is not None else None)

    def enqueue_tags(self, stream=None):
        """tags="motion": the maneuver tagger on the ego filter's output (with the lane camera's offset), the rig tagger on the
        tracker's state, and one mask (and record) per vehicle into self.tag_log; call behind enqueue_rig_track and
        enqueue_lane_paths on the same stream."""
        if self.tags is None:
            raise RuntimeError('enqueue_tags needs RigLoop(track=True, tags="motion")')
        ego, s = self.ego, stream or self.ego._s
        with torch.cuda.stream(ego._torch_stream(stream)):      # the maneuver stage's buffers, made at the first call, are filled there
            ego.enqueue_maneuver(stream=s, lane_offset=self.lane_offset)
        rows = summary = None
        if self.tagger is not None:
            rows, summary = self.tagger.detect(self.tracker, ego.plan_state, stream=s)
        self.tag_log.pack_and_append(1, maneuver=ego.maneuver, inter_rows=rows, inter_summary=summary, stream=s)

    def enqueue_lane_paths(self, stream=None):
        """The lane camera's fits, gathered on the device, and the ego start states -> self.ref_paths / n_ref / lane_offset
        (av_lane_paths_ground through the lane camera's vehicle calibration); call behind the camera half and the ego's enqueue_kf."""
        if self.lane_camera is None:
            raise RuntimeError("enqueue_lane_paths needs RigLoop(lane_camera=...)")
        cam, ego = self.cams.cam, self.ego
        with torch.cuda.stream(ego._torch_stream(stream)):
            torch.index_select(cam.poly, 0, self._lane_idx, out=self._poly)
            torch.index_select(cam.pts, 0, self._lane_idx, out=self._pts)
            torch.index_select(cam.info, 0, self._lane_idx, out=self._info)
        nat.check(self.L.av_lane_paths_ground(ego.ctx.handle, stream or ego._s, nat.ptr(self.lane_ground), self.V, self.h, self.w, 50,
                                              nat.ptr(self._poly), nat.ptr(self._pts), nat.ptr(self._info), nat.ptr(ego.plan_state), 1,
                                              50, nat.ptr(self.ref_paths), nat.ptr(self.n_ref), nat.ptr(self.lane_offset)))

    def enqueue_road_lanes(self, stream=None):
        """lanes="road": every camera's Hough segments (read in place from the lane workspace), the mounts, the odometry's motion
        (ego="ground_flow") and the ego start states -> self.ref_paths / n_ref / lane_offset and self.road_lanes' rows
        (av_road_lanes); call behind the camera half and the ego's enqueue_kf."""
        if self.road_lanes is None:
            raise RuntimeError('enqueue_road_lanes needs RigLoop(lanes="road")')
        self.road_lanes.update(self.lane_segments, self.lane_nseg, plan_state=self.ego.plan_state,
                               motion=self.odometry.motion if self.odometry is not None else None, stream=stream or self.ego._s)

    def enqueue_road_marks(self, stream=None):
        """marks=True: the boundaries enqueue_road_lanes() left and the cameras' rectified frames (cams.cam.frames, read and never
        written) -> self.road_marks' rows (av_road_marks); call behind enqueue_road_lanes() on the same stream.  The next camera half
        waits for the ego stream before it overwrites the frames, as it does for the surround view."""
        if self.road_marks is None:
            raise RuntimeError('enqueue_road_marks needs RigLoop(lanes="road", marks=True)')
        self.road_marks.update(self.cams.cam.frames, self.road_lanes.bound_rows, self.road_lanes.rows, stream=stream or self.ego._s)

    def enqueue_lane_plan(self, stream=None):
        """plan="lanes": the planner's candidates (ego.wp, ego.cost: read and never written), the boundaries enqueue_road_lanes() left
        and, with marks=True, the marks of enqueue_road_marks() -> self.lane_plan's outputs (av_lane_plan); call behind
        ego.enqueue_plan_each() on the same stream."""
        if self.lane_plan is None:
            raise RuntimeError('enqueue_lane_plan needs RigLoop(lanes="road", plan="lanes")')
        ego, rm = self.ego, self.road_marks
        self.lane_plan.rank(ego.plan_state, ego.wp, ego.cost, self.road_lanes.bound_rows, self.road_lanes.rows,
                            marks=rm.mark_rows if rm is not None else None, sides=rm.side_rows if rm is not None else None,
                            stream=stream or ego._s)

    def step(self, frames=None, sync=False):
        """The camera half for V * K frames (frames: PerceptionLoop.enqueue_frames', [V * K, h, w, 3]); then on the ego loop's
        stream the cameras' detections -> tracker [-> track filter] -> camera-frame obstacle lists, the ego Kalman stage, av_rig_fuse,
        the lane camera's reference path and the per-state planner.  The camera half of the next step overwrites what this one
        reads, so it first waits for the ego stream, as CameraLoop.step does."""
        cams, ego = self.cams, self.ego
        cam, hot = cams.cam, cams.hot
        if cam._tail_deferred or cam._lanes_pending:
            raise RuntimeError("RigLoop steps the plain PerceptionLoop.step(): with a deferred detector tail or a pending lane half "
                               "det_* / poly describe the previous frame")
        if self._stepped:
            cam.stream.wait_stream(ego.stream)
        cam.step(frames=frames)
        ego.stream.wait_stream(cam.stream)
        s = ego._s
        hot.enqueue_detect(s)
        hot.enqueue_track(s)
        if hot.track_filter is not None:
            hot.enqueue_track_filter(s)
        # hot.plan_state is zero: every list in its camera's own road frame
        hot.enqueue_obstacles(s, obs_cls=self.cam_cls if self.tags is not None else None)
        ego.enqueue_kf()
        self.enqueue_fuse()
        if self.tracker is not None:
            self.enqueue_rig_track()
        if self.lane_camera is not None:
            self.enqueue_lane_paths()
        if self.road_lanes is not None:
            self.enqueue_road_lanes()
        if self.road_marks is not None:
            self.enqueue_road_marks()
        ego.enqueue_plan_each()
        if self.lane_plan is not None:
            self.enqueue_lane_plan()
        if self.tags is not None:
            self.enqueue_tags()
        self._stepped = True
        if sync:
            self.synchronize()

    def enqueue_surround_view(self, gh=800, gw=800, x_far=40.0, m_per_px=0.1, fill=(0, 0, 0), blend="feather", overlay=True,
                              memory=False, memory_kw=None):
        """The rig's own picture of the last step(), on the ego stream (call it behind step(); the next camera half waits for that
        stream): self.surround_view uint8 [V, gh, gw, 3], every vehicle's K frames (cams.cam.frames: rectified, read and never
        written) stitched into one top-down panel in the vehicle's frame -- row 0 at x_far metres ahead, m_per_px metres per pixel,
        the forward axis down the middle column, `fill` where no camera sees the road, blend "feather" or "nearest"
        (visualization.SurroundView, av_rig_surround) -- and self.surround_cover uint8 [V, gh, gw], bit k where camera k saw the
        pixel.  overlay: what the ego loop planned around is drawn over the panel (av_rig_view_build, av_raster_draw): the tracked
        list coloured by track id with track=True, else the fused list, each obstacle a ring of its radius and, with velocities, its
        way in one second; the lane camera's reference path; the best trajectory; the ego vehicle.
        memory=True (with ego="ground_flow" only: the measured pose anchors it): the pixels no camera sees -- the road under the
        vehicle, beside its sills -- are filled from earlier frames between the stitch and the overlay (self.road_memory, a
        visualization.RoadMemory with memory_kw's size, cell_m, max_age and fill: a world-anchored canvas per vehicle, DESIGN 7u;
        av_roadmem_step on the odometry's own state and mode, no host round trip), and self.surround_age uint8 [V, gh, gw] is 0
        where a camera sees the pixel, its age in frames where it is remembered, 255 where it is `fill`; surround_cover stays the
        cameras'.  The frame on which the odometry measured nothing starts the canvas anew.  While memory is on neither the
        geometry nor fill, blend or memory_kw may change between calls."""
        from .visualization.surround_view import SurroundView, check_panel, surround_cfg
        if not isinstance(memory, (bool, np.bool_)):
            raise ValueError("RigLoop: memory is True or False")
        if memory_kw is not None and not memory:
            raise ValueError("RigLoop: memory_kw belongs to memory=True")
        if memory_kw is not None and not (isinstance(memory_kw, dict) and set(memory_kw) <= {"size", "cell_m", "max_age", "fill"}):
            raise ValueError("RigLoop: memory_kw is None or a dict of size, cell_m, max_age and fill")
        if memory and self.odometry is None:
            raise ValueError('RigLoop: memory=True needs ego="ground_flow": there is no measured pose to anchor the road memory to')
        if not self._stepped:
            raise RuntimeError("enqueue_surround_view draws what a step() left behind: call it after one")
        if not isinstance(overlay, (bool, np.bool_)):
            raise ValueError("RigLoop: overlay is True or False")
        check_panel(self.V, self.h, self.w, gh, gw)
        surround_cfg(x_far, m_per_px, fill, blend)                                  # (ValueError for a setting outside its range)
        ego, V = self.ego, self.V
        key = (int(gh), int(gw), float(x_far), float(m_per_px), tuple(int(c) for c in fill), blend)
        if memory:
            from .visualization.road_memory import roadmem_cfg
            mkw = dict(dict(fill=key[4]), **(memory_kw or {}))
            roadmem_cfg(key[0], key[1], key[2], key[3], **mkw)                      # (ValueError for a bad geometry)
            key = key + (tuple(sorted((k, tuple(v) if k == "fill" else v) for k, v in mkw.items())),)
            if getattr(self, "_surround_key", None) is not None and len(self._surround_key) == len(key) and self._surround_key != key:
                raise ValueError("RigLoop: the surround view's settings (geometry, fill, blend, memory_kw) may not change while memory is "
                                 "on: the canvas and what it remembers belong to them")
        with torch.cuda.stream(ego.stream):                 # the view's buffers and the ids below are made on the stream that fills them
            if getattr(self, "_surround_key", None) != key:
                self._surround = SurroundView(self.rig, V, self.h, self.w, gh=key[0], gw=key[1], x_far=key[2], m_per_px=key[3],
                                              fill=key[4], blend=blend, ctx=ego.ctx, memory=mkw if memory else None)
                self._surround_key = key
            sv = self._surround
            sv.render(self.cams.cam.frames, stream=ego._s, ego=(self.odometry.state, self.odometry.mode) if memory else None)
            self.surround_view, self.surround_cover = sv.panel, sv.cover
            self.surround_age, self.road_memory = sv.age, sv.memory
            if not overlay:
                return
            ids = None
            if self.tracker is not None:
                t = self.tracker
                obstacles, n_obs = t.obstacles, t.n_obs
                # the id of the slot behind each row (RigTracker.tracks()' first field), gathered on the device
                slot_ids = t.state[:, nat.RIG_TRACK_HDR_BYTES:].reshape(V, t.tcap, nat.RIG_TRACK_SLOT_BYTES)[:, :, :4].contiguous()
                slot_ids = slot_ids.view(torch.int32).reshape(V, t.tcap)
                ids = self._surround_ids = torch.gather(slot_ids, 1, t.obs_slot.clamp(0, t.tcap - 1).long()).contiguous()
            else:
                obstacles, n_obs = self.obstacles, self.n_obs.view(V)
            sv.draw(ego.plan_state, obstacles, n_obs, ids=ids, ref_path=self.ref_paths, n_ref=self.n_ref, waypoints=ego.wp,
                    order=self.lane_plan.order if self.lane_plan is not None else ego.order, stream=ego._s)

    def capture(self):
        raise RuntimeError("RigLoop: graph capture is out of scope")

    def synchronize(self):
        self.cams.synchronize()
        self.ego.synchronize()

    def results(self):
        """The ego loop's results() of the last step (obstacles [V, 1, K * tcap, cols] and n_obs [V, 1] are the fused lists -- with track=True
        the tracked lists [V, 1, tcap, cols], beside fused_obstacles / fused_n_obs (the fused lists), track_ids [V, tcap] (the id behind
        each obstacle row, -1 past n_obs), match [V, K * tcap] (the id each fused row went to), n_drop [V] and rig_tracks
        (RigTracker.tracks())) plus
        cam_obstacles [V, K, tcap, cols], cam_n_obs [V, K], n_off [V, K] (the cameras' own lists), views [V, K * tcap] (the mask of the
        cameras that saw each fused obstacle), n_skip [V] and, with a lane camera or lanes="road", ref_paths [V, 50, 2] (n_points
        of them with lanes="road"), n_ref [V], lane_offset [V]; with lanes="road" also lane_bounds [V, 8] (av_road_lane_bound),
        lane_left / lane_right [V, 3], lane_width, lane_heading, lane_curvature, lane_count, lane_index, lane_views, lane_status [V].
        With marks=True: lane_mark_left / _right [V] (the ego lane's sides: 0 unknown, 1 solid, 2 dashed), lane_colour_left / _right
        [V] (0, 1 white, 2 yellow), may_change_left / _right [V] (1 over a dashed line, 0 not over a solid one, -1 unknown) and
        bound_marks [V, 8] (av_road_mark, beside lane_bounds).
        With plan="lanes": lane_cost and plan_total [V, C], plan_order [V, C] (cost and order stay the planner's), plan_best,
        plan_maneuver (0 keep, 1 left, 2 right), plan_delta, plan_crossed (bit j: line j), plan_flags [V] (av_lane_plan_row's) and
        plan_lines [V, 10] (av_lane_plan_line).
        With tags: track_cls [V, tcap] and fused_cls [V, K * tcap] (the class id behind each tracked / fused row, -1 past the count),
        interactions (one tagging.InteractionTags per vehicle) and interaction_summary (av_interaction_summary [V]); the last two are
        None when class_map is not the reference map.
        With ego="ground_flow": ego_motion [V, 3] (t_f, t_l, omega), ego_valid [V], ego_pose [V, 3], ego_inliers [V], ego_views [V]."""
        self.synchronize()
        hot, V, K = self.cams.hot, self.V, self.K
        out = self.ego.results()
        if self.odometry is not None:
            e = self.odometry.results()
            out["ego_motion"], out["ego_valid"], out["ego_pose"] = e["motion"], e["valid"], e["pose"]
            out["ego_inliers"], out["ego_views"] = e["n_inliers"], e["views"]
        out["cam_obstacles"] = hot.obstacles.cpu().numpy().reshape(V, K, self.tcap, self.cols)
        out["cam_n_obs"] = hot.n_obs.cpu().numpy().reshape(V, K)
        out["n_off"] = hot.n_off.cpu().numpy().reshape(V, K)
        out["views"], out["n_skip"] = self.views.cpu().numpy(), self.n_skip.cpu().numpy()
        if self.tracker is not None:
            # obstacles / n_obs above are the tracked lists the ego loop planned around
            t = self.tracker
            out["fused_obstacles"], out["fused_n_obs"] = self.obstacles.cpu().numpy(), self.n_obs.cpu().numpy()
            out["rig_tracks"] = t.tracks()
            slot, n = t.obs_slot.cpu().numpy(), t.n_obs.cpu().numpy()
            written = np.arange(t.tcap)[None, :] < n[:, None]
            out["track_ids"] = np.where(written, np.take_along_axis(out["rig_tracks"]["id"], np.where(written, slot, 0), axis=1), -1)
            out["match"], out["n_drop"] = t.match.cpu().numpy(), t.n_drop.cpu().numpy()
            if self.tags is not None:
                # the class behind each tracked / fused obstacle row, -1 past the counts (and for a track whose class is not known)
                out["track_cls"] = np.where(written, t.cls.cpu().numpy(), -1)
                fused = np.arange(K * self.tcap)[None, :] < out["fused_n_obs"].reshape(V, 1)
                out["fused_cls"] = np.where(fused, self.fused_cls.cpu().numpy(), -1)
                out["interactions"] = out["interaction_summary"] = None
                if self.tagger is not None:
                    out["interactions"] = self.tagger.results()
                    out["interaction_summary"] = (self.tagger.summary.cpu().numpy().reshape(V, -1)
                                                  .view(np.dtype(nat.INTERACTION_SUMMARY_FIELDS)).reshape(V))
        if self.lane_camera is not None or self.road_lanes is not None:
            out["ref_paths"], out["n_ref"] = self.ref_paths.cpu().numpy(), self.n_ref.cpu().numpy()
            out["lane_offset"] = self.lane_offset.cpu().numpy()
        if self.road_lanes is not None:
            rows = self.road_lanes.lanes()
            out["lane_bounds"] = self.road_lanes.bounds()
            out["lane_left"], out["lane_right"], out["lane_width"] = rows["left"].copy(), rows["right"].copy(), rows["width"].copy()
            out["lane_heading"], out["lane_curvature"] = rows["heading"].copy(), rows["curvature"].copy()
            out["lane_count"], out["lane_index"] = rows["lane_count"].copy(), rows["lane_index"].copy()
            out["lane_views"], out["lane_status"] = rows["views"].copy(), rows["status"].copy()
        if self.road_marks is not None:
            sides = self.road_marks.sides()
            out["bound_marks"] = self.road_marks.marks()
            out["lane_mark_left"], out["lane_mark_right"] = sides["left"]["type"].copy(), sides["right"]["type"].copy()
            out["lane_colour_left"], out["lane_colour_right"] = sides["left"]["colour"].copy(), sides["right"]["colour"].copy()
            out["may_change_left"], out["may_change_right"] = sides["may_change_left"].copy(), sides["may_change_right"].copy()
        if self.lane_plan is not None:
            p = self.lane_plan.results()
            out["lane_cost"], out["plan_total"], out["plan_order"] = p["lane_cost"], p["total"], p["order"]
            out["plan_best"], out["plan_maneuver"] = p["rows"]["best"].copy(), p["rows"]["maneuver"].copy()
            out["plan_delta"], out["plan_crossed"] = p["rows"]["delta"].copy(), p["rows"]["crossed"].copy()
            out["plan_flags"], out["plan_lines"] = p["rows"]["flags"].copy(), p["lines"]
        return out
