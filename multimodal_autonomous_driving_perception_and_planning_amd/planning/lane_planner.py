"""Lane planner: the planner's candidates charged for the lane boundaries they cross, by the boundaries' marks, and ranked again
(include/avhot.h: av_lane_plan*, csrc/laneplan.hip).  A post-pass over what the planner wrote: it reads the
waypoints and costs of perception-side planning (av_planner_plan_each / _plan_moving), the boundaries of perception.RoadLanes and
the marks of perception.RoadMarks, all in place on the device."""
import ctypes as C

import numpy as np

from .. import _native as nat

_TRIPLES = ("w_cross", "w_on")


def lane_plan_cfg(**kw):
    """av_lane_plan_cfg from nat.LANEPLAN_DEFAULTS and the given fields (w_cross and w_on: three numbers, by mark type unknown,
    solid, dashed), checked by the library's own rule (av_lane_plan_check: host only, no GPU); ValueError with the library's message
    where it refuses, or for a field there is not."""
    vals = dict(nat.LANEPLAN_DEFAULTS)
    for k, v in kw.items():
        if k not in vals:
            raise ValueError("lane planner: no setting %r (av_lane_plan_cfg has %s)" % (k, ", ".join(vals)))
        vals[k] = v
    v = vals["follow"]
    if isinstance(v, (bool, np.bool_)):
        v = int(v)
    if not isinstance(v, (int, np.integer)) or not -2 ** 31 <= v < 2 ** 31:
        raise ValueError("lane planner: follow is 0 or 1")
    cfg = nat.LanePlanCfg()
    cfg.follow, cfg.reserved = int(v), 0
    try:
        for k in _TRIPLES:
            t = tuple(float(x) for x in vals[k])
            if len(t) != 3:
                raise ValueError
            setattr(cfg, k, (C.c_double * 3)(*t))
        cfg.half_width, cfg.x_far, cfg.w_end = float(vals["half_width"]), float(vals["x_far"]), float(vals["w_end"])
    except (TypeError, ValueError):
        raise ValueError("lane planner: half_width, x_far and w_end are numbers, w_cross and w_on three numbers each") from None
    if nat.lib().av_lane_plan_check(C.byref(cfg)) != 0:
        raise ValueError(nat.lib().av_last_error_string().decode())
    return cfg


def check_shape(n_vehicles, n_cand, n_points):
    """av_lane_plan's shape rules without a GPU: ValueError naming the argument."""
    for name, v, hi in (("n_vehicles", n_vehicles, 65535), ("n_cand", n_cand, nat.LANEPLAN_MAX_CAND),
                        ("n_points", n_points, nat.LANEPLAN_MAX_POINTS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("lane planner: %s is an integer" % name)
        if not 1 <= v <= hi:
            raise ValueError("lane planner: %s %d not in 1..%d" % (name, v, hi))


class LanePlanner:
    """n_vehicles planners' candidates ([n_cand] trajectories of n_points waypoints each) ranked against the lane boundaries.

    **cfg: av_lane_plan_cfg's fields (nat.LANEPLAN_DEFAULTS).  It owns the outputs: lines uint8 [V, 10, 48] (av_lane_plan_line),
    lane_cost and total float64 [V, C], order int32 [V, C], cross int32 [V, C] (the bits of a uint32), delta int32 [V, C] and rows
    uint8 [V, 64] (av_lane_plan_row)."""

    def __init__(self, n_vehicles, n_cand, n_points, ctx=None, device=0, **cfg):
        self.cfg = lane_plan_cfg(**cfg)                     # checked first: a bad one is refused without a GPU
        check_shape(n_vehicles, n_cand, n_points)
        self.V, self.C, self.n = int(n_vehicles), int(n_cand), int(n_points)
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("LanePlanner needs a HIP device; this package has no CPU path")
        self.dev = torch.device("cuda", device)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        V, Cn, d, f64, i32 = self.V, self.C, self.dev, torch.float64, torch.int32
        self.lines = torch.zeros(V, nat.LANEPLAN_MAX_LINES, nat.LANEPLAN_LINE_BYTES, dtype=torch.uint8, device=d)
        self.lane_cost, self.total = torch.zeros(V, Cn, dtype=f64, device=d), torch.zeros(V, Cn, dtype=f64, device=d)
        self.order, self.cross, self.delta = (torch.zeros(V, Cn, dtype=i32, device=d) for _ in range(3))
        self.rows = torch.zeros(V, nat.LANEPLAN_ROW_BYTES, dtype=torch.uint8, device=d)
        torch.cuda.current_stream(d).synchronize()

    def rank(self, plan_state, waypoints, cost, bounds, lanes, marks=None, sides=None, stream=None):
        """One frame, enqueued on `stream` (a hipStream_t as c_void_p; default: torch's current stream); no allocation, no host round
        trip.  plan_state float64 [V, 4], waypoints float64 [V, C, n, 6] and cost float64 [V, C] are the planner's (read, never
        written); bounds and lanes RoadLanes.bound_rows (uint8 [V, 8, 64]) and RoadLanes.rows (uint8 [V, 128]); marks and sides
        RoadMarks.mark_rows (uint8 [V, 8, 64]) and .side_rows (uint8 [V, 64]), or both None: lanes without marks, every type unknown.
        Tensors of those layouts are read in place; a contiguous view into a larger tensor is fine."""
        import torch

        if (marks is None) != (sides is None):
            raise ValueError("marks and sides come together, or neither")
        V, Cn, n = self.V, self.C, self.n
        for name, t, count in (("plan_state", plan_state, V * 4), ("waypoints", waypoints, V * Cn * n * nat.WP_DOUBLES),
                               ("cost", cost, V * Cn)):
            if t.dtype != torch.float64 or t.numel() != count or not t.is_contiguous() or t.device != self.dev:
                raise ValueError("%s: %d contiguous float64 on the device" % (name, count))
        rows = [("bounds", bounds, V * nat.ROAD_LANES_MAX_BOUNDS * nat.ROAD_LANE_BOUND_BYTES), ("lanes", lanes, V * nat.ROAD_LANES_ROW_BYTES)]
        if marks is not None:
            rows += [("marks", marks, V * nat.ROAD_LANES_MAX_BOUNDS * nat.ROAD_MARK_BYTES), ("sides", sides, V * nat.ROAD_MARKS_ROW_BYTES)]
        for name, t, nbytes in rows:
            if t.numel() * t.element_size() != nbytes or not t.is_contiguous() or t.device != self.dev or t.data_ptr() % 8:
                raise ValueError("%s: %d contiguous bytes on the device, 8-byte aligned" % (name, nbytes))
        nat.check(self.L.av_lane_plan(self.ctx.handle, stream or nat.stream_handle(), C.byref(self.cfg), V, Cn, n, nat.ptr(plan_state),
                                      nat.ptr(waypoints), nat.ptr(cost), nat.ptr(bounds), nat.ptr(lanes), nat.ptr(marks), nat.ptr(sides),
                                      nat.ptr(self.lines), nat.ptr(self.lane_cost), nat.ptr(self.total), nat.ptr(self.order),
                                      nat.ptr(self.cross), nat.ptr(self.delta), nat.ptr(self.rows)))

    def results(self):
        """The last frame on the host: lines (a structured array [V, 10], nat.LANEPLAN_LINE_FIELDS), lane_cost, total [V, C], order
        [V, C], cross uint32 [V, C], delta [V, C] and rows (a structured array [V], nat.LANEPLAN_ROW_FIELDS).  Synchronises."""
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        host = lambda t: t.cpu().numpy()
        return dict(lines=host(self.lines).view(np.dtype(nat.LANEPLAN_LINE_FIELDS)).reshape(self.V, nat.LANEPLAN_MAX_LINES),
                    lane_cost=host(self.lane_cost), total=host(self.total), order=host(self.order),
                    cross=host(self.cross).view(np.uint32), delta=host(self.delta),
                    rows=host(self.rows).view(np.dtype(nat.LANEPLAN_ROW_FIELDS)).reshape(self.V))
