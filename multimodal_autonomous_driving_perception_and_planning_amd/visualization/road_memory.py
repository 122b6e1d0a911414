"""Road memory: the surround panel's unseen pixels -- the road under the vehicle, beside its sills, between two fields of view --
from earlier frames (include/avhot.h: av_roadmem_*, csrc/roadmem.hip).

A world-anchored rolling canvas per vehicle takes every frame's seen panel pixels through the pose the odometry integrated on the
device (perception.RigOdometry / GroundOdometry: their `state` tensor), and the panel's unseen pixels are read back out of it.  The
canvas is anchored in the world, not in the vehicle, so a pixel is resampled exactly twice whatever its age; it is a small local
road map of its own (`canvas`, `stamp`).  Every kernel is in libavhot.so; this class owns the buffers and checks shapes.
"""
import ctypes as C

import numpy as np

from .. import _native as nat


def roadmem_cfg(gh, gw, x_far, m_per_px, size=512, cell_m=None, max_age=90, fill=(0, 0, 0)):
    """av_roadmem_cfg for a panel of gh x gw pixels of m_per_px metres with x_far metres at its top edge (SurroundView's geometry),
    checked by the library's own rule (av_roadmem_check: host only, no GPU); ValueError with the library's message where it
    refuses.  size: the canvas' cells a side; cell_m: their pitch in metres (None: the panel's); max_age in frames."""
    try:
        f = [int(c) for c in fill]
    except (TypeError, ValueError):
        raise ValueError("road memory: fill is three bytes (b, g, r)") from None
    if len(f) != 3 or not all(0 <= c <= 255 for c in f):
        raise ValueError("road memory: fill is three bytes (b, g, r)")
    ints = (gh, gw, size, max_age)
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 31 <= v < 2 ** 31 for v in ints):
        raise ValueError("road memory: gh, gw, size and max_age are integers")
    try:
        x_far, m_per_px = float(x_far), float(m_per_px)
        cell_m = m_per_px if cell_m is None else float(cell_m)
    except (TypeError, ValueError):
        raise ValueError("road memory: x_far, m_per_px and cell_m are numbers") from None
    cfg = nat.RoadmemCfg(n=int(size), max_age=int(max_age), m_per_px=cell_m, gh=int(gh), gw=int(gw), x_far=x_far,
                         panel_m_per_px=m_per_px, fill=(C.c_uint8 * 3)(*f), reserved=(C.c_uint8 * 5)())
    if nat.lib().av_roadmem_check(C.byref(cfg)) != 0:
        raise ValueError(nat.lib().av_last_error_string().decode())
    return cfg


class RoadMemory:
    def __init__(self, n_vehicles, gh, gw, x_far, m_per_px, size=512, cell_m=None, max_age=90, fill=(0, 0, 0), ctx=None, device=0):
        """n_vehicles canvases of size x size cells of cell_m metres (None: the panel's pitch) for panels of gh x gw pixels of
        m_per_px metres, x_far metres at the top edge.  A cell last written more than max_age frames ago is not read back; an
        unseen pixel that is not remembered becomes fill (b, g, r)."""
        import torch
        # the geometry is checked first: a bad one is refused without a GPU
        self.cfg = roadmem_cfg(gh, gw, x_far, m_per_px, size, cell_m, max_age, fill)
        if isinstance(n_vehicles, bool) or not isinstance(n_vehicles, (int, np.integer)) or not 1 <= n_vehicles <= 65535:
            raise ValueError("road memory: n_vehicles is an integer 1 .. 65535")
        if (gh + 15) // 16 > 65535:
            raise ValueError("road memory: more than 65535 tile rows")
        if not torch.cuda.is_available():
            raise RuntimeError("RoadMemory needs a HIP device; this package has no CPU path")
        self.V, self.gh, self.gw, self.N = int(n_vehicles), int(gh), int(gw), int(size)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.dev = d = torch.device("cuda", self.ctx.device)
        V, N, u8 = self.V, self.N, torch.uint8
        self.canvas = torch.zeros(V, N, N, 4, dtype=u8, device=d)                       # b, g, r, 0 per world cell, on the torus
        self.stamp = torch.zeros(V, N, N, dtype=torch.int32, device=d)                  # (uint32 bits) 0: never seen, else the frame
        self.age = torch.full((V, self.gh, self.gw), 255, dtype=u8, device=d)
        self.state = torch.zeros(V, nat.ROADMEM_STATE_BYTES, dtype=u8, device=d)
        self.poses = torch.zeros(V, nat.ROADMEM_POSE_BYTES, dtype=u8, device=d)
        torch.cuda.current_stream(d).synchronize()          # the buffers are filled before another stream writes them

    @staticmethod
    def _stream(stream):
        return stream if isinstance(stream, C.c_void_p) else nat.stream_handle(stream)

    def _tensor(self, t, shape, what, dtype=None):
        import torch
        if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dtype == (dtype or torch.uint8) and tuple(t.shape) == shape):
            raise ValueError("RoadMemory: %s is a contiguous uint8 device tensor %s" % (what, list(shape)))
        return t

    def _panel_cover(self, panel, cover):
        return (self._tensor(panel, (self.V, self.gh, self.gw, 3), "panel"), self._tensor(cover, (self.V, self.gh, self.gw), "cover"))

    def _ego(self, state, mode):
        self._tensor(state, (self.V, nat.EGOFLOW_STATE_BYTES), "state (the odometry's)")
        if mode is not None:
            self._tensor(mode, (self.V,), "mode")

    def pose_from(self, state, mode=None, stream=None):
        """Stage 1: the odometry's state tensor uint8 [V, 32] (x, y, psi) and mode uint8 [V] (2: it measured nothing on this frame,
        which resets the vehicle's canvas; None: never) -> self.poses."""
        self._ego(state, mode)
        nat.check(self.L.av_roadmem_pose_from(self.ctx.handle, self._stream(stream), self.V, nat.ptr(state), nat.ptr(mode),
                                              nat.ptr(self.poses)))
        return self.poses

    def update(self, panel, cover, stream=None):
        """Stage 2: the seen pixels (cover != 0) of panel uint8 [V, gh, gw, 3], the stitched panel before any fill, into the canvas
        through self.poses."""
        panel, cover = self._panel_cover(panel, cover)
        nat.check(self.L.av_roadmem_update(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.V, nat.ptr(self.poses),
                                           nat.ptr(panel), nat.ptr(cover), nat.ptr(self.state), nat.ptr(self.canvas), nat.ptr(self.stamp)))

    def fill(self, panel, cover, stream=None):
        """Stage 3: the unseen pixels (cover == 0) of panel, in place, out of the canvas; self.age uint8 [V, gh, gw]: 0 seen now,
        1 .. 254 frames since the oldest of the four cells was seen, 255 not remembered (the pixel is `fill`).  Returns panel."""
        panel, cover = self._panel_cover(panel, cover)
        nat.check(self.L.av_roadmem_fill(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.V, nat.ptr(self.poses),
                                         nat.ptr(self.state), nat.ptr(self.canvas), nat.ptr(self.stamp), nat.ptr(cover), nat.ptr(panel),
                                         nat.ptr(self.age)))
        return panel

    def step(self, panel, cover, state, mode=None, stream=None):
        """All three stages on `stream` (a torch stream or a raw handle; default: the current one): no allocation, no host round
        trip.  Returns panel, filled in place."""
        panel, cover = self._panel_cover(panel, cover)
        self._ego(state, mode)
        nat.check(self.L.av_roadmem_step(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.V, nat.ptr(state), nat.ptr(mode),
                                         nat.ptr(self.poses), nat.ptr(panel), nat.ptr(cover), nat.ptr(self.state), nat.ptr(self.canvas),
                                         nat.ptr(self.stamp), nat.ptr(self.age)))
        return panel

    def reset(self, v=None, stream=None):
        """Forget what vehicle v (None: every vehicle) has seen: its next frame starts a new canvas."""
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < self.V):
            raise ValueError("RoadMemory.reset: v is None or a vehicle index 0 .. %d" % (self.V - 1))
        nat.check(self.L.av_roadmem_reset(self.ctx.handle, self._stream(stream), self.V, -1 if v is None else int(v), nat.ptr(self.state)))

    def results(self):
        """What the last call left (synchronises): dict(state, poses: structured arrays [V] of nat.ROADMEM_STATE_FIELDS /
        ROADMEM_POSE_FIELDS; canvas [V, N, N, 4]; stamp uint32 [V, N, N]; age [V, gh, gw])."""
        import torch
        torch.cuda.synchronize(self.dev)
        return dict(state=self.state.cpu().numpy().view(np.dtype(nat.ROADMEM_STATE_FIELDS)).reshape(self.V),
                    poses=self.poses.cpu().numpy().view(np.dtype(nat.ROADMEM_POSE_FIELDS)).reshape(self.V),
                    canvas=self.canvas.cpu().numpy(), stamp=self.stamp.cpu().numpy().view(np.uint32), age=self.age.cpu().numpy())
