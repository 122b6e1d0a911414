"""Road lanes: the lane boundaries in metres from the Hough segments of every camera of a rig (include/avhot.h: av_road_lanes*,
csrc/roadlanes.hip)."""
import ctypes as C

import numpy as np

from .. import _native as nat
from .calibration import CameraRig, ground_table


def road_lanes_cfg(**kw):
    """av_road_lanes_cfg from nat.ROAD_LANES_DEFAULTS and the given fields, checked by the library's own rule (av_road_lanes_check:
    host only, no GPU); ValueError with the library's message where it refuses, or for a field there is not."""
    vals = dict(nat.ROAD_LANES_DEFAULTS)
    for k, v in kw.items():
        if k not in vals:
            raise ValueError("road lanes: no setting %r (av_road_lanes_cfg has %s)" % (k, ", ".join(vals)))
        vals[k] = v
    ints = ("min_votes", "max_coast", "one_sided", "n_points")
    for k in ints:
        v = vals[k]
        if isinstance(v, (bool, np.bool_)) and k == "one_sided":
            v = vals[k] = int(v)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("road lanes: %s is an integer" % k)
    try:
        vals = {k: (int(v) if k in ints else float(v)) for k, v in vals.items()}
    except (TypeError, ValueError):
        raise ValueError("road lanes: the settings other than %s are numbers" % ", ".join(ints)) from None
    cfg = nat.RoadLanesCfg(**vals)
    if nat.lib().av_road_lanes_check(C.byref(cfg)) != 0:
        raise ValueError(nat.lib().av_last_error_string().decode())
    return cfg


def check_shape(n_vehicles, n_cams, max_segments, scap, n_points=None, rcap=None):
    """av_road_lanes' shape rules without a GPU: ValueError naming the argument."""
    for name, v in (("n_vehicles", n_vehicles), ("max_segments", max_segments), ("scap", scap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("road lanes: %s is an integer" % name)
    if not 1 <= n_vehicles <= 65535:
        raise ValueError("road lanes: n_vehicles %d not in 1..65535" % n_vehicles)
    if not 1 <= n_cams <= 8:
        raise ValueError("road lanes: n_cams %d not in 1..8" % n_cams)
    if max_segments < 1:
        raise ValueError("road lanes: max_segments must be >= 1")
    if not 1 <= scap <= nat.ROAD_LANES_MAX_SCAP:
        raise ValueError("road lanes: scap %d not in 1..%d" % (scap, nat.ROAD_LANES_MAX_SCAP))
    if n_points is not None and rcap is not None and n_points > rcap:
        raise ValueError("road lanes: n_points %d exceeds rcap %d" % (n_points, rcap))


class RoadLanes:
    """n_vehicles rigs' lane boundaries, ego lane and reference path, frame to frame, on the device.

    rig: a perception.CameraRig (a camera behind a lens contributes through its rectified calibration: the lane chain sees
    rectified frames).  h, w: the frames' size (kept for the caller; the stage reads segments, not pixels).  max_segments: the rows of
    every camera's segment list; scap <= 256: how many of them the stage reads.  **cfg: av_road_lanes_cfg's fields
    (nat.ROAD_LANES_DEFAULTS).  It owns the state and the outputs: ref_paths float64 [V, n_points, 2], n_ref int32 [V],
    lane_offset float64 [V] (NaN without a lane) are what the planner and the maneuver tagger take."""

    def __init__(self, rig, n_vehicles, h, w, max_segments, scap=256, ctx=None, device=0, **cfg):
        self.cfg = road_lanes_cfg(**cfg)                    # checked first: a bad one is refused without a GPU
        if not isinstance(rig, CameraRig):
            raise ValueError("RoadLanes: rig is a perception.CameraRig")
        check_shape(n_vehicles, rig.K, max_segments, scap)
        self.rig, self.V, self.K, self.h, self.w = rig, int(n_vehicles), rig.K, int(h), int(w)
        self.max_segments, self.scap, self.n = int(max_segments), int(scap), int(n_vehicles) * rig.K
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("RoadLanes needs a HIP device; this package has no CPU path")
        self.dev = torch.device("cuda", device)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        cals = [c.rectified() if c.lens is not None else c for c in rig.calibrations(self.V)]
        self.ground, self.calibration = ground_table(cals, self.n, self.dev)
        self.mounts = rig.mounts_table(self.V, self.dev)                                # float64 [V, K, 4]
        V, d, u8 = self.V, self.dev, torch.uint8
        self.state = torch.zeros(V, nat.ROAD_LANES_STATE_BYTES, dtype=u8, device=d)
        self.bound_rows = torch.zeros(V, nat.ROAD_LANES_MAX_BOUNDS, nat.ROAD_LANE_BOUND_BYTES, dtype=u8, device=d)
        self.info_rows = torch.zeros(V, nat.ROAD_LANES_INFO_BYTES, dtype=u8, device=d)
        self.rows = torch.zeros(V, nat.ROAD_LANES_ROW_BYTES, dtype=u8, device=d)
        self.ref_paths = torch.zeros(V, self.cfg.n_points, 2, dtype=torch.float64, device=d)
        self.n_ref = torch.zeros(V, dtype=torch.int32, device=d)
        self.lane_offset = torch.full((V,), float("nan"), dtype=torch.float64, device=d)
        self._zero_plan = torch.zeros(V, 4, dtype=torch.float64, device=d)
        torch.cuda.current_stream(d).synchronize()

    def update(self, segments, nseg, plan_state=None, motion=None, stream=None):
        """One frame, enqueued on `stream` (a hipStream_t as c_void_p; default: torch's current stream); no allocation, no host round
        trip.  segments: device int32 [V * K, max_segments, 4] and nseg int32 [V * K], read in place (views into a lane workspace
        are fine).  plan_state: device float64 [V, 4] (None: zeros, the path stands in the vehicle frame itself).  motion: a device
        tensor of V av_egoflow_motion entries (RigOdometry.motion) or None."""
        import torch

        if (tuple(segments.shape) != (self.n, self.max_segments, 4) or segments.dtype != torch.int32 or not segments.is_contiguous()
                or segments.device != self.dev):
            raise ValueError("segments: contiguous device int32 [%d, %d, 4]" % (self.n, self.max_segments))
        if tuple(nseg.shape) != (self.n,) or nseg.dtype != torch.int32 or not nseg.is_contiguous() or nseg.device != self.dev:
            raise ValueError("nseg: contiguous device int32 [%d]" % self.n)
        if plan_state is None:
            plan_state = self._zero_plan
        elif (plan_state.dtype != torch.float64 or plan_state.numel() != self.V * 4 or not plan_state.is_contiguous()
              or plan_state.device != self.dev):
            raise ValueError("plan_state: contiguous device float64 [%d, 4]" % self.V)
        if motion is not None and (motion.numel() * motion.element_size() != self.V * nat.EGOFLOW_MOTION_BYTES
                                   or not motion.is_contiguous() or motion.device != self.dev):
            raise ValueError("motion: %d av_egoflow_motion entries on the device" % self.V)
        nat.check(self.L.av_road_lanes(self.ctx.handle, stream or nat.stream_handle(), C.byref(self.cfg), self.V, self.K,
                                       nat.ptr(self.ground), nat.ptr(self.mounts), self.max_segments, self.scap, nat.ptr(segments),
                                       nat.ptr(nseg), nat.ptr(motion), nat.ptr(plan_state), nat.ptr(self.state), nat.ptr(self.bound_rows),
                                       nat.ptr(self.info_rows), nat.ptr(self.rows), int(self.ref_paths.shape[1]), nat.ptr(self.ref_paths),
                                       nat.ptr(self.n_ref), nat.ptr(self.lane_offset)))

    def reset(self, vehicle=None, stream=None):
        """Forget the lane of one vehicle (None: of all): the next frame's fit is taken as it is."""
        nat.check(self.L.av_road_lanes_reset(self.ctx.handle, stream or nat.stream_handle(), self.V, -1 if vehicle is None else int(vehicle),
                                             nat.ptr(self.state)))

    def _host(self, t, fields, shape):
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        return t.cpu().numpy().view(np.dtype(fields)).reshape(shape)

    def lanes(self):
        """The last frame's av_road_lanes_row per vehicle: a structured array [V] (nat.ROAD_LANES_ROW_FIELDS).  Synchronises."""
        return self._host(self.rows, nat.ROAD_LANES_ROW_FIELDS, self.V)

    def bounds(self):
        """The last frame's boundaries: a structured array [V, 8] (nat.ROAD_LANE_BOUND_FIELDS), lanes()["n_bounds"] of them live."""
        return self._host(self.bound_rows, nat.ROAD_LANE_BOUND_FIELDS, (self.V, nat.ROAD_LANES_MAX_BOUNDS))

    def info(self):
        """The last frame's av_road_lanes_info per vehicle (nat.ROAD_LANES_INFO_FIELDS)."""
        return self._host(self.info_rows, nat.ROAD_LANES_INFO_FIELDS, self.V)

    def states(self):
        """The state per vehicle (nat.ROAD_LANES_STATE_FIELDS)."""
        return self._host(self.state, nat.ROAD_LANES_STATE_FIELDS, self.V)
