"""A rig's surround view: the K cameras of a vehicle stitched into one top-down panel in the vehicle's frame (av_rig_surround), with
what the planner steered around drawn over it (av_rig_view_build + av_raster_draw).

CameraLoop.enqueue_ground_view gives one bird's-eye panel per camera, each in its own camera's road frame.  SurroundView takes the
same rectified frames through the rig's mounts instead: every panel pixel comes from the cameras that see that road point, blended
with weights that fade towards each frame's border ("feather") or taken from the nearest camera ("nearest").  Every kernel is in
libavhot.so; this class owns the tables and the output buffers and checks shapes.
"""
import ctypes as C

import numpy as np

from .. import _native as nat

MAX_PANEL = 8191            # the rasteriser's largest picture side


def surround_cfg(x_far=40.0, m_per_px=0.1, fill=(0, 0, 0), blend="feather"):
    """av_surround_cfg from the panel's settings; ValueError outside what the library accepts."""
    if blend not in nat.SURROUND_BLENDS:
        raise ValueError('surround view: blend is "feather" or "nearest"')
    try:
        x_far, m_per_px = float(x_far), float(m_per_px)
    except (TypeError, ValueError):
        raise ValueError("surround view: x_far and m_per_px are numbers") from None
    if not np.isfinite(x_far):
        raise ValueError("surround view: x_far must be finite")
    if not (m_per_px > 0.0 and np.isfinite(m_per_px)):
        raise ValueError("surround view: m_per_px must be > 0 and finite")
    try:
        f = [int(c) for c in fill]
    except (TypeError, ValueError):
        raise ValueError("surround view: fill is three bytes (b, g, r)") from None
    if len(f) != 3 or not all(0 <= c <= 255 for c in f):
        raise ValueError("surround view: fill is three bytes (b, g, r)")
    return nat.SurroundCfg(x_far, m_per_px, nat.SURROUND_BLENDS[blend], (C.c_uint8 * 3)(*f), 0)


def check_panel(n_vehicles, h, w, gh, gw):
    """ValueError for a shape av_rig_surround or the rasteriser refuses."""
    ints = (n_vehicles, h, w, gh, gw)
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in ints):
        raise ValueError("surround view: n_vehicles, h, w, gh and gw are integers")
    if not 1 <= n_vehicles <= 65535:
        raise ValueError("surround view: n_vehicles is 1 .. 65535")
    if not (1 <= h <= 32768 and 1 <= w <= 32768):
        raise ValueError("surround view: h and w are 1 .. 32768")
    if not (1 <= gh <= MAX_PANEL and 1 <= gw <= MAX_PANEL):
        raise ValueError("surround view: gh and gw are 1 .. %d" % MAX_PANEL)


class SurroundView:
    def __init__(self, rig, n_vehicles, h, w, gh=800, gw=800, x_far=40.0, m_per_px=0.1, fill=(0, 0, 0), blend="feather", ctx=None,
                 device=0, memory=None):
        """rig: a perception.CameraRig; n_vehicles rigs of it, frames of h x w pixels (RECTIFIED: a camera's lens plays no part
        here).  The panel is gh x gw pixels of m_per_px metres, its top edge x_far metres ahead of the vehicle's origin and the
        vehicle's forward axis down the middle column (so x_far = gh * m_per_px / 2 puts the vehicle in the centre).  fill: (b, g, r)
        where no camera sees the road; blend: "feather" or "nearest".  memory: None, or a dict of RoadMemory's settings (size,
        cell_m, max_age, fill -- the panel's by default; {} for the defaults): render(..., ego=) then fills the pixels no camera
        sees from earlier frames (self.memory, a visualization.RoadMemory) and self.age says how old each pixel is."""
        import torch
        from ..perception.calibration import CameraRig, ground_table
        if not isinstance(rig, CameraRig):
            raise ValueError("SurroundView: rig is a perception.CameraRig")
        check_panel(n_vehicles, h, w, gh, gw)
        self.cfg = surround_cfg(x_far, m_per_px, fill, blend)
        if memory is not None:
            from .road_memory import roadmem_cfg
            if not isinstance(memory, dict) or not set(memory) <= {"size", "cell_m", "max_age", "fill"}:
                raise ValueError("SurroundView: memory is None or a dict of size, cell_m, max_age and fill")
            memory = dict(dict(fill=fill), **memory)
            roadmem_cfg(gh, gw, x_far, m_per_px, **memory)                         # (ValueError for a bad geometry, without a GPU)
        if not torch.cuda.is_available():
            raise RuntimeError("SurroundView needs a HIP device; this package has no CPU path")
        self.rig, self.V, self.K, self.h, self.w, self.gh, self.gw = rig, int(n_vehicles), rig.K, int(h), int(w), int(gh), int(gw)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.dev = d = torch.device("cuda", self.ctx.device)
        self.mounts = rig.mounts_table(self.V, d)                                                       # float64 [V, K, 4]
        self.ground = ground_table([c.rectified() for c in rig.calibrations(self.V)], self.V * self.K, d)[0]
        self.panel = torch.zeros(self.V, self.gh, self.gw, 3, dtype=torch.uint8, device=d)
        self.cover = torch.zeros(self.V, self.gh, self.gw, dtype=torch.uint8, device=d)
        self.prims = self.n_prims = None                    # the overlay's list, sized by the first draw()
        self._prim_shape = None
        self.memory = self.age = None
        if memory is not None:
            from .road_memory import RoadMemory
            self.memory = RoadMemory(self.V, self.gh, self.gw, x_far, m_per_px, ctx=self.ctx, **memory)
            self.age = self.memory.age
        torch.cuda.current_stream(d).synchronize()          # the buffers are zero-filled before another stream writes them

    @staticmethod
    def _stream(stream):
        return stream if isinstance(stream, C.c_void_p) else nat.stream_handle(stream)

    def render(self, frames, stream=None, ego=None):
        """frames: a contiguous uint8 device tensor [V * K, h, w, 3] (camera k of vehicle v is frame v * K + k), read and never
        written.  Fills self.panel [V, gh, gw, 3] and self.cover [V, gh, gw] (bit k: camera k saw the pixel).  Enqueued on `stream`
        (a torch stream or a raw handle; default: the current one).  Returns self.panel.
        With memory=: ego = (state, mode), the odometry's device tensors of these frames (RigOdometry.state uint8 [V, 32] and
        .mode uint8 [V], or None for mode); the pixels no camera sees are then filled from the road memory and self.age uint8
        [V, gh, gw] is 0 where a camera sees the pixel, its age in frames where it is remembered and 255 where it is `fill`;
        self.cover stays the cameras' cover."""
        import torch
        if (ego is not None) != (self.memory is not None):
            raise ValueError("SurroundView.render: ego=(state, mode) comes with memory=, and memory= needs it")
        if ego is not None and not (isinstance(ego, (tuple, list)) and len(ego) == 2):
            raise ValueError("SurroundView.render: ego is (state, mode)")
        if not (torch.is_tensor(frames) and frames.is_cuda and frames.is_contiguous() and frames.dtype == torch.uint8
                and tuple(frames.shape) == (self.V * self.K, self.h, self.w, 3)):
            raise ValueError("SurroundView.render: frames is a contiguous uint8 device tensor [%d, %d, %d, 3]"
                             % (self.V * self.K, self.h, self.w))
        nat.check(self.L.av_rig_surround(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.V, self.K, nat.ptr(self.mounts),
                                         nat.ptr(self.ground), self.h, self.w, nat.ptr(frames), self.gh, self.gw, nat.ptr(self.panel),
                                         nat.ptr(self.cover)))
        if self.memory is not None:
            self.memory.step(self.panel, self.cover, ego[0], mode=ego[1], stream=self._stream(stream))
        return self.panel

    def draw(self, plan_state, obstacles, n_obs, ids=None, ref_path=None, n_ref=None, waypoints=None, order=None, stream=None):
        """The overlay over self.panel: the reference path (ref_path float64 [V, rcap, 2] with n_ref int32 [V], or neither), the
        planned trajectory (waypoints float64 [V, n_cand, n_points, 6] with order int32 [V, n_cand], or neither), a ring and, with
        five columns, a one-second velocity segment per obstacle (obstacles float64 [V, ocap, 3 or 5] -- or the loops'
        [V, 1, ocap, cols] --, n_obs int32 [V], coloured by ids int32 [V, ocap] when given) and the ego vehicle.  plan_state: float64
        [V, 4] (x, y, heading, speed), the frame the world points are seen from.  Contiguous device tensors.  Returns self.panel."""
        import torch
        f64, i32 = torch.float64, torch.int32
        ok = lambda t, dt: torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.dtype == dt          # noqa: E731
        V = self.V
        if not (ok(plan_state, f64) and plan_state.numel() == V * 4 and plan_state.shape[0] == V and plan_state.shape[-1] == 4):
            raise ValueError("SurroundView.draw: plan_state is a contiguous float64 device tensor [V, 4]")
        if ok(obstacles, f64) and obstacles.dim() == 4 and obstacles.shape[1] == 1:
            obstacles = obstacles[:, 0]
        if not (ok(obstacles, f64) and obstacles.dim() == 3 and obstacles.shape[0] == V and obstacles.shape[1] >= 1
                and obstacles.shape[2] in (3, 5)):
            raise ValueError("SurroundView.draw: obstacles is a contiguous float64 device tensor [V, ocap, 3 or 5]")
        ocap, ncol = int(obstacles.shape[1]), int(obstacles.shape[2])
        if not (ok(n_obs, i32) and n_obs.numel() == V and n_obs.shape[0] == V):
            raise ValueError("SurroundView.draw: n_obs is a contiguous int32 device tensor [V]")
        if ids is not None and not (ok(ids, i32) and tuple(ids.shape) == (V, ocap)):
            raise ValueError("SurroundView.draw: ids is None or a contiguous int32 device tensor [V, ocap]")
        if (ref_path is None) != (n_ref is None):
            raise ValueError("SurroundView.draw: ref_path and n_ref come together")
        rcap = 1
        if ref_path is not None:
            if not (ok(ref_path, f64) and ref_path.dim() == 3 and ref_path.shape[0] == V and ref_path.shape[1] >= 1
                    and ref_path.shape[2] == 2 and ok(n_ref, i32) and tuple(n_ref.shape) == (V,)):
                raise ValueError("SurroundView.draw: ref_path is a contiguous float64 device tensor [V, rcap, 2], n_ref int32 [V]")
            rcap = int(ref_path.shape[1])
        if (waypoints is None) != (order is None):
            raise ValueError("SurroundView.draw: waypoints and order come together")
        n_cand = n_points = 1
        if waypoints is not None:
            if not (ok(waypoints, f64) and waypoints.dim() == 4 and waypoints.shape[0] == V and waypoints.shape[1] >= 1
                    and waypoints.shape[2] >= 1 and waypoints.shape[3] == 6 and ok(order, i32)
                    and tuple(order.shape) == (V, waypoints.shape[1])):
                raise ValueError("SurroundView.draw: waypoints is a contiguous float64 device tensor [V, n_cand, n_points, 6], order "
                                 "int32 [V, n_cand]")
            n_cand, n_points = int(waypoints.shape[1]), int(waypoints.shape[2])
        cap = int(self.L.av_rig_view_prim_cap(ocap, rcap, n_points))
        if cap <= 0 or cap > 65535:
            raise ValueError("SurroundView.draw: the overlay needs %d primitives (ocap %d, rcap %d, n_points %d), the rasteriser takes "
                             "65535" % (cap, ocap, rcap, n_points))
        st = self._stream(stream)
        if self._prim_shape != cap:
            ts = torch.cuda.ExternalStream(st.value, device=self.dev) if st.value else torch.cuda.default_stream(self.dev)
            with torch.cuda.stream(ts):                     # zero-filled on the stream that writes them
                self.prims = torch.zeros(V, cap, nat.PRIM_BYTES, dtype=torch.uint8, device=self.dev)
                self.n_prims = torch.zeros(V, dtype=i32, device=self.dev)
            self._prim_shape = cap
        nat.check(self.L.av_rig_view_build(self.ctx.handle, st, C.byref(self.cfg), V, self.gh, self.gw, nat.ptr(plan_state), ncol, ocap,
                                           nat.ptr(obstacles), nat.ptr(n_obs), nat.ptr(ids), rcap, nat.ptr(ref_path), nat.ptr(n_ref),
                                           n_cand, n_points, nat.ptr(waypoints), nat.ptr(order), nat.ptr(self.prims), cap,
                                           nat.ptr(self.n_prims)))
        nat.check(self.L.av_raster_draw(self.ctx.handle, st, V, self.gh, self.gw, nat.ptr(self.panel), nat.ptr(self.prims), cap,
                                        nat.ptr(self.n_prims), None, 0))
        return self.panel
