"""Per-track constant-velocity Kalman filter over the tracker's snapshot tables (av_track_filter_update).

The reference's Track.velocity is the last centre difference (multi_object_tracker.py:35-47): noisy, wrong after a gap and
stale while a track coasts.  TrackFilter keeps one small Kalman filter per track on the device, fed the matched centres and
predicting through misses; its state persists from window to window, keyed by the rows' slots.  Every kernel is in
libavhot.so; this class owns the state buffer and checks shapes.
"""
import ctypes as C

import numpy as np
import torch

from .. import _native as nat

_DEFAULTS = dict(q_accel=1.0, r_meas=4.0, p0_pos=4.0, p0_vel=100.0)


def filter_cfg(**cfg):
    """av_track_filter_cfg from keyword overrides of its defaults; ValueError outside the ranges the library accepts."""
    unknown = set(cfg) - set(_DEFAULTS)
    if unknown:
        raise ValueError("track filter: unknown setting(s) %s (known: %s)" % (sorted(unknown), sorted(_DEFAULTS)))
    c = dict(_DEFAULTS)
    c.update({k: float(v) for k, v in cfg.items()})
    if not all(np.isfinite(v) for v in c.values()):
        raise ValueError("track filter: every setting must be finite")
    if c["q_accel"] < 0 or c["p0_pos"] < 0 or c["p0_vel"] < 0 or not c["r_meas"] > 0:
        raise ValueError("track filter: q_accel, p0_pos, p0_vel must be >= 0 and r_meas > 0")
    return nat.TrackFilterCfg(**c)


class TrackFilter:
    def __init__(self, n_streams, tcap=64, ctx=None, device=0, **cfg):
        """n_streams filter banks of tcap slots each (tcap as the tracker's: a multiple of 64 in [64, 1024]).  cfg: q_accel (1.0,
        white-noise acceleration, px^2 / frame^4), r_meas (4.0, variance of a measured centre coordinate, px^2), p0_pos (4.0) and
        p0_vel (100.0), the initial variances of a newborn track."""
        if not torch.cuda.is_available():
            raise RuntimeError("TrackFilter needs a HIP device; this package has no CPU path")
        if n_streams <= 0 or tcap < 64 or tcap > 1024 or tcap % 64:
            raise ValueError("TrackFilter: n_streams >= 1 and tcap a multiple of 64 in [64, 1024]")
        self.S, self.tcap = int(n_streams), int(tcap)
        self.cfg = filter_cfg(**cfg)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.dev = torch.device("cuda", self.ctx.device)
        self.state_bytes = int(self.L.av_track_filter_state_bytes(self.tcap))
        self.state = torch.zeros(self.S, self.state_bytes, dtype=torch.uint8, device=self.dev)
        self.reset()

    @staticmethod
    def _stream(stream):
        return stream if isinstance(stream, C.c_void_p) else nat.stream_handle(stream)

    def reset(self, stream=None):
        """Every slot free, status 0 (stream-ordered)."""
        nat.check(self.L.av_track_filter_reset(self.ctx.handle, self._stream(stream), self.S, self.tcap, nat.ptr(self.state)))

    def update(self, snap, snap_n, out=None, stream=None):
        """snap: av_tracker_update's tables, uint8 [S, W, tcap, 64]; snap_n int32 [S, W] (device tensors) -> filt float64
        [S, W, tcap, 6] (cx, cy, vx, vy, pos_sigma, vel_sigma), aligned with the rows; rows at and past a frame's count are not
        written (a fresh `out` holds NaN there).  Enqueued on `stream` (a torch stream or a raw handle; default: the current one)."""
        if not (snap.is_cuda and snap.is_contiguous() and snap.dtype == torch.uint8 and snap.dim() == 4
                and snap.shape[0] == self.S and snap.shape[2] == self.tcap and snap.shape[3] == nat.TRACK_ROW_BYTES):
            raise ValueError("TrackFilter.update: snap is a contiguous uint8 device tensor [S, W, tcap, %d]" % nat.TRACK_ROW_BYTES)
        W = int(snap.shape[1])
        if not (snap_n.is_cuda and snap_n.is_contiguous() and snap_n.dtype == torch.int32 and tuple(snap_n.shape) == (self.S, W)):
            raise ValueError("TrackFilter.update: snap_n is a contiguous int32 device tensor [S, W]")
        if out is None:
            out = torch.full((self.S, W, self.tcap, 6), float("nan"), dtype=torch.float64, device=self.dev)
        elif not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (self.S, W, self.tcap, 6)):
            raise ValueError("TrackFilter.update: out is a contiguous float64 device tensor [S, W, tcap, 6]")
        nat.check(self.L.av_track_filter_update(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.S, W, self.tcap,
                                                nat.ptr(snap), nat.ptr(snap_n), nat.ptr(self.state), nat.ptr(out)))
        return out

    @property
    def status(self):
        """int32 [S]: the streams' status words (bit 0: a row named a slot outside [0, tcap) and was skipped).  Synchronises."""
        torch.cuda.synchronize(self.dev)
        return self.state[:, :4].cpu().numpy().view(np.int32).reshape(self.S).copy()

    def slots(self):
        """Host view of the state: structured array [S, tcap] (id, reserved, x[4], p[3]).  Synchronises."""
        torch.cuda.synchronize(self.dev)
        raw = self.state[:, nat.TRACK_FILTER_HDR_BYTES:].cpu().numpy()
        return raw.view(np.dtype(nat.TRACK_FILTER_SLOT_FIELDS)).reshape(self.S, self.tcap)
