"""Road marks: what each lane boundary is -- solid or dashed, white or yellow -- read from the rig's rectified frames along the
boundaries of perception.RoadLanes (include/avhot.h: av_road_marks*, csrc/roadmarks.hip)."""
import ctypes as C

import numpy as np

from .. import _native as nat
from .calibration import CameraRig, ground_table

_INTS = ("n_samples", "core", "shoulder0", "shoulder1", "contrast", "yellow_tenths", "hold", "forget")


def road_marks_cfg(**kw):
    """av_road_marks_cfg from nat.ROAD_MARKS_DEFAULTS and the given fields, checked by the library's own rule (av_road_marks_check:
    host only, no GPU); ValueError with the library's message where it refuses, or for a field there is not."""
    vals = dict(nat.ROAD_MARKS_DEFAULTS)
    for k, v in kw.items():
        if k not in vals:
            raise ValueError("road marks: no setting %r (av_road_marks_cfg has %s)" % (k, ", ".join(vals)))
        vals[k] = v
    for k in _INTS:
        v = vals[k]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("road marks: %s is an integer" % k)
    try:
        vals = {k: (int(v) if k in _INTS else float(v)) for k, v in vals.items()}
    except (TypeError, ValueError):
        raise ValueError("road marks: the settings other than %s are numbers" % ", ".join(_INTS)) from None
    cfg = nat.RoadMarksCfg(**vals)
    if nat.lib().av_road_marks_check(C.byref(cfg)) != 0:
        raise ValueError(nat.lib().av_last_error_string().decode())
    return cfg


def check_shape(n_vehicles, n_cams, h, w):
    """av_road_marks' shape rules without a GPU: ValueError naming the argument."""
    for name, v in (("n_vehicles", n_vehicles), ("h", h), ("w", w)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("road marks: %s is an integer" % name)
    if not 1 <= n_vehicles <= 65535:
        raise ValueError("road marks: n_vehicles %d not in 1..65535" % n_vehicles)
    if not 1 <= n_cams <= 8:
        raise ValueError("road marks: n_cams %d not in 1..8" % n_cams)
    if not (1 <= h <= 32768 and 1 <= w <= 32768):
        raise ValueError("road marks: frame size h %d, w %d not in 1..32768" % (h, w))


class RoadMarks:
    """n_vehicles rigs' lane boundaries classified frame by frame on the device, and the ego lane's two sides held over frames.

    rig: a perception.CameraRig (a camera behind a lens contributes through its rectified calibration: the stage reads rectified
    frames).  h, w: the frames' size.  **cfg: av_road_marks_cfg's fields (nat.ROAD_MARKS_DEFAULTS).  It owns the state and the
    outputs: mark_rows [V, 8] (av_road_mark), side_rows [V] (av_road_marks_row) and profile uint32 [V, 8, 2, 16] (the seen and the
    paint bits of every sample)."""

    def __init__(self, rig, n_vehicles, h, w, ctx=None, device=0, **cfg):
        self.cfg = road_marks_cfg(**cfg)                    # checked first: a bad one is refused without a GPU
        if not isinstance(rig, CameraRig):
            raise ValueError("RoadMarks: rig is a perception.CameraRig")
        check_shape(n_vehicles, rig.K, h, w)
        self.rig, self.V, self.K, self.h, self.w, self.n = rig, int(n_vehicles), rig.K, int(h), int(w), int(n_vehicles) * rig.K
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("RoadMarks needs a HIP device; this package has no CPU path")
        self.dev = torch.device("cuda", device)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        cals = [c.rectified() if c.lens is not None else c for c in rig.calibrations(self.V)]
        self.ground, self.calibration = ground_table(cals, self.n, self.dev)
        self.mounts = rig.mounts_table(self.V, self.dev)                                # float64 [V, K, 4]
        V, d, u8 = self.V, self.dev, torch.uint8
        self.state = torch.zeros(V, nat.ROAD_MARKS_STATE_BYTES, dtype=u8, device=d)
        self.mark_rows = torch.zeros(V, nat.ROAD_LANES_MAX_BOUNDS, nat.ROAD_MARK_BYTES, dtype=u8, device=d)
        self.side_rows = torch.zeros(V, nat.ROAD_MARKS_ROW_BYTES, dtype=u8, device=d)
        self.profile = torch.zeros(V, nat.ROAD_LANES_MAX_BOUNDS, 2, nat.ROAD_MARKS_PROFILE_WORDS, dtype=torch.int32, device=d)
        torch.cuda.current_stream(d).synchronize()

    def update(self, frames, bounds, lanes, stream=None):
        """One frame, enqueued on `stream` (a hipStream_t as c_void_p; default: torch's current stream); no allocation, no host round
        trip.  frames: device uint8 [V * K, h, w, 3], rectified, read in place (a contiguous view into a larger tensor is fine).
        bounds, lanes: RoadLanes.bound_rows (uint8 [V, 8, 64]) and RoadLanes.rows (uint8 [V, 128]) of the same frame, or tensors of
        their layout, read in place."""
        import torch

        if (tuple(frames.shape) != (self.n, self.h, self.w, 3) or frames.dtype != torch.uint8 or not frames.is_contiguous()
                or frames.device != self.dev):
            raise ValueError("frames: contiguous device uint8 [%d, %d, %d, 3]" % (self.n, self.h, self.w))
        for name, t, nbytes in (("bounds", bounds, self.V * nat.ROAD_LANES_MAX_BOUNDS * nat.ROAD_LANE_BOUND_BYTES),
                                ("lanes", lanes, self.V * nat.ROAD_LANES_ROW_BYTES)):
            if t.numel() * t.element_size() != nbytes or not t.is_contiguous() or t.device != self.dev or t.data_ptr() % 8:
                raise ValueError("%s: %d contiguous bytes on the device, 8-byte aligned" % (name, nbytes))
        nat.check(self.L.av_road_marks(self.ctx.handle, stream or nat.stream_handle(), C.byref(self.cfg), self.V, self.K,
                                       nat.ptr(self.mounts), nat.ptr(self.ground), self.h, self.w, nat.ptr(frames), nat.ptr(bounds),
                                       nat.ptr(lanes), nat.ptr(self.state), nat.ptr(self.mark_rows), nat.ptr(self.side_rows),
                                       nat.ptr(self.profile)))

    def reset(self, vehicle=None, stream=None):
        """Forget what the sides of one vehicle's lane were (None: of all)."""
        nat.check(self.L.av_road_marks_reset(self.ctx.handle, stream or nat.stream_handle(), self.V, -1 if vehicle is None else int(vehicle),
                                             nat.ptr(self.state)))

    def _host(self, t, fields, shape):
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        return t.cpu().numpy().view(np.dtype(fields)).reshape(shape)

    def marks(self):
        """The last frame's av_road_mark per boundary: a structured array [V, 8] (nat.ROAD_MARK_FIELDS).  Synchronises."""
        return self._host(self.mark_rows, nat.ROAD_MARK_FIELDS, (self.V, nat.ROAD_LANES_MAX_BOUNDS))

    def sides(self):
        """The ego lane's sides per vehicle: a structured array [V] (nat.ROAD_MARKS_ROW_FIELDS)."""
        return self._host(self.side_rows, nat.ROAD_MARKS_ROW_FIELDS, self.V)

    def states(self):
        """The state per vehicle (nat.ROAD_MARKS_STATE_FIELDS)."""
        return self._host(self.state, nat.ROAD_MARKS_STATE_FIELDS, self.V)

    def profiles(self):
        """The last frame's bit strings: bool [V, 8, 2, n_samples], [..., 0, :] seen and [..., 1, :] paint."""
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        words = self.profile.cpu().numpy().view(np.uint32)
        bits = (words[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1
        return bits.reshape(self.V, nat.ROAD_LANES_MAX_BOUNDS, 2, -1)[..., :self.cfg.n_samples].astype(bool)
