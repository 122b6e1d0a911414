"""Vehicle-frame tracks over av_rig_fuse's lists (av_rig_track).

av_rig_fuse gives a fresh, unlabelled list per frame.  RigTracker follows it over time on the device: a fused obstacle keeps one
id from frame to frame and from camera to camera, a track that nobody sees for a while coasts at its predicted place, and its
velocity is filtered in the planner's frame by a constant-velocity Kalman filter per track.  Every kernel is in libavhot.so; this
class owns the state and the output buffers and checks shapes.
"""
import ctypes as C

import numpy as np

from .. import _native as nat

_DEFAULTS = dict(dt=1.0 / 30.0, q_accel=4.0, r_meas=0.25, r_range=1e-6, p0_pos=1.0, p0_vel=25.0, gate_scale=2.0, gate_min=2.0,
                 max_age=30, min_hits=3)
_INTS = ("max_age", "min_hits")


def rig_track_cfg(**cfg):
    """av_rig_track_cfg from keyword overrides of its defaults; ValueError outside the ranges the library accepts."""
    unknown = set(cfg) - set(_DEFAULTS)
    if unknown:
        raise ValueError("rig tracker: unknown setting(s) %s (known: %s)" % (sorted(unknown), sorted(_DEFAULTS)))
    c = dict(_DEFAULTS)
    c.update(cfg)
    for k in _INTS:
        if isinstance(c[k], bool) or not isinstance(c[k], (int, np.integer)):
            raise ValueError("rig tracker: %s is an integer" % k)
        c[k] = int(c[k])
    for k in c:
        if k not in _INTS:
            c[k] = float(c[k])
            if not np.isfinite(c[k]) or c[k] < 0.0:
                raise ValueError("rig tracker: %s must be finite and >= 0" % k)
    if not (c["dt"] > 0.0 and c["r_meas"] > 0.0):
        raise ValueError("rig tracker: dt and r_meas must be > 0")
    if c["max_age"] < 0 or c["min_hits"] < 1 or c["max_age"] > 2**31 - 2 or c["min_hits"] > 2**31 - 1:
        raise ValueError("rig tracker: max_age must be >= 0 and min_hits >= 1")
    return nat.RigTrackCfg(**c)


def check_shape(n_vehicles, tcap, ncol):
    """ValueError for a tracker shape av_rig_track refuses."""
    if int(n_vehicles) < 1:
        raise ValueError("RigTracker: n_vehicles must be >= 1")
    if not 1 <= int(tcap) <= nat.RIG_TRACK_MAX:
        raise ValueError("RigTracker: tcap is 1 .. %d" % nat.RIG_TRACK_MAX)
    if ncol not in (3, 5):
        raise ValueError("RigTracker: ncol is 3 (x, y, r) or 5 (x, y, r, vx, vy)")


class RigTracker:
    def __init__(self, n_vehicles, tcap=128, ncol=5, ctx=None, device=0, **cfg):
        """n_vehicles track tables of tcap slots each (1 .. 512) over obstacle lists of ncol columns.  cfg: av_rig_track_cfg's
        fields -- dt (1/30 s), q_accel (4.0 m^2/s^4), r_meas (0.25 m^2), r_range (1e-6: the measurement variance grows with the
        fourth power of the range from the vehicle; 0 for the plain SORT filter), p0_pos (1.0), p0_vel (25.0), gate_scale (2.0 radii),
        gate_min (2.0 m), max_age (30 misses), min_hits (3)."""
        import torch
        check_shape(n_vehicles, tcap, ncol)
        self.cfg = rig_track_cfg(**cfg)
        if not torch.cuda.is_available():
            raise RuntimeError("RigTracker needs a HIP device; this package has no CPU path")
        self.V, self.tcap, self.ncol = int(n_vehicles), int(tcap), int(ncol)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.dev = torch.device("cuda", self.ctx.device)
        self.state_bytes = int(self.L.av_rig_track_state_bytes(self.tcap))
        d, i32 = self.dev, torch.int32
        self.state = torch.zeros(self.V, self.state_bytes, dtype=torch.uint8, device=d)
        self.obstacles = torch.zeros(self.V, self.tcap, self.ncol, dtype=torch.float64, device=d)
        self.n_obs = torch.zeros(self.V, dtype=i32, device=d)
        self.obs_slot = torch.zeros(self.V, self.tcap, dtype=i32, device=d)
        self.n_skip = torch.zeros(self.V, dtype=i32, device=d)
        self.n_drop = torch.zeros(self.V, dtype=i32, device=d)
        self.match = None                                   # int32 [V, ocap_in], sized by the first update
        self.cls = torch.full((self.V, self.tcap), -1, dtype=i32, device=d)     # update(cls=...): the class behind each output row
        self.reset()

    @staticmethod
    def _stream(stream):
        return stream if isinstance(stream, C.c_void_p) else nat.stream_handle(stream)

    def reset(self, stream=None):
        """Every slot free, the next id 1, status 0 (stream-ordered)."""
        nat.check(self.L.av_rig_track_reset(self.ctx.handle, self._stream(stream), self.V, self.tcap, nat.ptr(self.state)))

    def update(self, obstacles, n_obs, plan_state, views=None, stream=None, cls=None):
        """One frame.  obstacles: float64 [V, ocap_in, ncol] (or av_rig_fuse's [V, 1, ocap_in, ncol]), n_obs int32 [V] (or [V, 1]),
        plan_state float64 [V, 4] (or [V, 1, 4]), views int32 [V, ocap_in] or None: contiguous device tensors.  Fills
        self.obstacles [V, tcap, ncol] / n_obs [V] (the confirmed tracks, coasting ones at their predicted place), obs_slot
        [V, tcap] (the slot behind each row), match [V, ocap_in] (the id each input row went to; -1: skipped, -2: dropped for want
        of a slot), n_skip and n_drop [V]; rows past a count keep what they held.  Enqueued on `stream` (a torch stream or a raw
        handle; default: the current one).  cls: int32 [V, ocap_in], the rows' class ids (av_rig_fuse_cls's), or None: with it the
        tracks carry the class of their latest classified row (av_rig_track_cls) and self.cls [V, tcap] holds the class behind each
        output row, -1 for none known; without it the call is av_rig_track and self.cls is not written.  Returns self.obstacles,
        self.n_obs."""
        import torch
        f64, i32 = torch.float64, torch.int32
        ok = lambda t, dt: torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dtype == dt          # noqa: E731
        if ok(obstacles, f64) and obstacles.dim() == 4 and obstacles.shape[1] == 1:
            obstacles = obstacles[:, 0]
        if not (ok(obstacles, f64) and obstacles.dim() == 3 and obstacles.shape[0] == self.V and obstacles.shape[2] == self.ncol
                and 1 <= obstacles.shape[1] <= nat.RIG_TRACK_MAX):
            raise ValueError("RigTracker.update: obstacles is a contiguous float64 device tensor [V, ocap_in, %d], ocap_in 1 .. %d"
                             % (self.ncol, nat.RIG_TRACK_MAX))
        ocap_in = int(obstacles.shape[1])
        if not (ok(n_obs, i32) and n_obs.numel() == self.V and n_obs.shape[0] == self.V):
            raise ValueError("RigTracker.update: n_obs is a contiguous int32 device tensor [V]")
        if not (ok(plan_state, f64) and plan_state.numel() == self.V * 4 and plan_state.shape[0] == self.V and plan_state.shape[-1] == 4):
            raise ValueError("RigTracker.update: plan_state is a contiguous float64 device tensor [V, 4]")
        if views is not None and not (ok(views, i32) and tuple(views.shape) == (self.V, ocap_in)):
            raise ValueError("RigTracker.update: views is None or a contiguous int32 device tensor [V, ocap_in]")
        if cls is not None and not (ok(cls, i32) and tuple(cls.shape) == (self.V, ocap_in)):
            raise ValueError("RigTracker.update: cls is None or a contiguous int32 device tensor [V, ocap_in]")
        if self.match is None or self.match.shape[1] != ocap_in:
            self.match = torch.full((self.V, ocap_in), -1, dtype=i32, device=self.dev)
        if cls is not None:
            nat.check(self.L.av_rig_track_cls(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.V, self.tcap, self.ncol,
                                              ocap_in, nat.ptr(obstacles), nat.ptr(n_obs), nat.ptr(views), nat.ptr(cls),
                                              nat.ptr(plan_state), nat.ptr(self.state), self.tcap, nat.ptr(self.obstacles),
                                              nat.ptr(self.n_obs), nat.ptr(self.obs_slot), nat.ptr(self.match), nat.ptr(self.n_skip),
                                              nat.ptr(self.n_drop), nat.ptr(self.cls)))
            return self.obstacles, self.n_obs
        nat.check(self.L.av_rig_track(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.V, self.tcap, self.ncol, ocap_in,
                                      nat.ptr(obstacles), nat.ptr(n_obs), nat.ptr(views), nat.ptr(plan_state), nat.ptr(self.state),
                                      self.tcap, nat.ptr(self.obstacles), nat.ptr(self.n_obs), nat.ptr(self.obs_slot),
                                      nat.ptr(self.match), nat.ptr(self.n_skip), nat.ptr(self.n_drop)))
        return self.obstacles, self.n_obs

    def _host_state(self):
        import torch
        torch.cuda.synchronize(self.dev)
        return self.state.cpu().numpy()

    def status(self):
        """int32 [V]: the vehicles' status words (bit 0: a row found no free slot and was dropped).  Synchronises."""
        return self._host_state()[:, :4].copy().view(np.int32).reshape(self.V)

    def header(self):
        """int32 [V, 4]: status, the next id, frames seen, live tracks.  Synchronises."""
        return self._host_state()[:, :16].copy().view(np.int32).reshape(self.V, 4)

    def tracks(self):
        """Host view of the state: structured array [V, tcap] with the slot's fields (id, hits, misses, age, views, views_ever,
        reserved, x[4], p[3], r) and pos_sigma = sqrt(2 P_pos), vel_sigma = sqrt(2 P_vel), the two uncertainties VehicleState
        carries, and cls, the track's class id (reserved[0] - 1; -1: none known).  id -1: a free slot.  Synchronises."""
        raw = self._host_state()[:, nat.RIG_TRACK_HDR_BYTES:].copy().view(np.dtype(nat.RIG_TRACK_SLOT_FIELDS)).reshape(self.V, self.tcap)
        out = np.zeros(raw.shape, np.dtype(nat.RIG_TRACK_SLOT_FIELDS + [("pos_sigma", "<f8"), ("vel_sigma", "<f8"), ("cls", "<i4")]))
        for name in raw.dtype.names:
            out[name] = raw[name]
        out["pos_sigma"], out["vel_sigma"] = np.sqrt(2.0 * raw["p"][..., 0]), np.sqrt(2.0 * raw["p"][..., 2])
        out["cls"] = raw["reserved"][..., 0] - 1
        return out
