"""Ground odometry: the ego motion of a camera from the road pixels of two consecutive frames (include/avhot.h: av_egoflow_*,
csrc/egoflow.hip).  The reference has no counterpart: it synthesises the ego measurement on the host
(video_loader.py:166-205)."""
import ctypes as C

import numpy as np

from .. import _native as nat
from .calibration import ground_table

NEAR_EDGE_M = 4.0       # f_far=None: the patch's near edge lies this many metres ahead of the camera's ground point


def egoflow_cfg(gh=256, gw=256, f_far=None, m_per_px=0.1, tile=16, search=12, frame_rate=30.0, min_texture=None, gate_px=3,
                inlier_px=1.0, min_inliers=8):
    """-> (nat.EgoflowCfg, tiles_y, tiles_x), checked by the library's own rule (av_egoflow_tiles: host only, no GPU); ValueError
    with the library's message where it refuses."""
    gh, gw, tile, search = int(gh), int(gw), int(tile), int(search)
    m_per_px = float(m_per_px)
    cfg = nat.EgoflowCfg(gh=gh, gw=gw, tile=tile, search=search,
                         f_far=NEAR_EDGE_M + gh * m_per_px if f_far is None else float(f_far), m_per_px=m_per_px,
                         frame_rate=float(frame_rate), min_texture=2 * tile * tile if min_texture is None else int(min_texture),
                         gate_px=int(gate_px), inlier_px=float(inlier_px), min_inliers=int(min_inliers), reserved=0)
    ty, tx = C.c_int(), C.c_int()
    if nat.lib().av_egoflow_tiles(C.byref(cfg), C.byref(ty), C.byref(tx)) != 0:
        raise ValueError(nat.lib().av_last_error_string().decode())
    return cfg, ty.value, tx.value


class GroundOdometry:
    """n cameras' planar ego motion, frame to frame, and the Kalman stage's measurement from it -- all on the device.

    Per update: a gray bird's-eye patch of every frame (gh x gw pixels of m_per_px metres, row 0 at f_far metres ahead, the
    camera's axis on the middle column: av_ground_warp's geometry), block matching of tile x tile tiles against the previous
    patch over +-search pixels, a vote, a gate and a least-squares rigid motion (t_f, t_l, omega) with one rejection round, and
    the pose (x, y, psi) of the camera's ground point integrated from it.  Other vehicles on the patch are outliers of the fit.

    The largest measurable speed is search * m_per_px * frame_rate: 36 m/s at the defaults (12 px of 0.1 m at 30 frames/s); a
    faster road leaves the tiles' best match on the search border, no tile is accepted, and the filter predicts (mode 2).

    f_far=None puts the patch's near edge NEAR_EDGE_M = 4 m ahead.  min_texture=None is 2 * tile * tile."""

    def __init__(self, calibration, n_cams, h, w, gh=256, gw=256, f_far=None, m_per_px=0.1, tile=16, search=12, frame_rate=30.0,
                 min_texture=None, gate_px=3, inlier_px=1.0, min_inliers=8, device=0, ctx=None):
        # the geometry is checked first: a bad one is refused without a GPU
        self.cfg, self.tiles_y, self.tiles_x = egoflow_cfg(gh, gw, f_far, m_per_px, tile, search, frame_rate, min_texture, gate_px,
                                                           inlier_px, min_inliers)
        self.n, self.h, self.w = int(n_cams), int(h), int(w)
        if self.n < 1 or self.h < 1 or self.w < 1:
            raise ValueError("n_cams, h and w must be >= 1")
        self.n_tiles = self.tiles_y * self.tiles_x
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("GroundOdometry needs a HIP device; this package has no CPU path")
        self.dev = torch.device("cuda", device)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.ground, self.calibration = ground_table(calibration, self.n, self.dev)
        if any(c.lens is not None for c in self.calibration):
            raise ValueError("GroundOdometry reads RECTIFIED frames: pass calibration.rectified() and rectify the frames first")
        n, d, u8 = self.n, self.dev, torch.uint8
        gh, gw = self.cfg.gh, self.cfg.gw
        self.patches = torch.zeros(n, 2, gh, gw, dtype=u8, device=d)                    # the ping-pong pair
        self.valid = torch.zeros(n, gh, (gw + 31) // 32, dtype=torch.int32, device=d)   # a bit per patch pixel
        self.tile_rows = torch.zeros(n, self.n_tiles, nat.EGOFLOW_TILE_BYTES, dtype=u8, device=d)
        self.motion = torch.zeros(n, nat.EGOFLOW_MOTION_BYTES, dtype=u8, device=d)
        self.state = torch.zeros(n, nat.EGOFLOW_STATE_BYTES, dtype=u8, device=d)
        self.z = torch.zeros(n, 4, dtype=torch.float64, device=d)                       # what av_kf_step reads, window 1
        self.mode = torch.full((n,), 2, dtype=u8, device=d)
        self._staged = None
        torch.cuda.current_stream(d).synchronize()

    # ---- the per-frame path: enqueue only ------------------------------------------------------------------------------------------
    def enqueue(self, frames, stream=None):
        """All four stages for device frames uint8 [n, h, w, 3] (rectified) on `stream` (a hipStream_t as c_void_p; default: torch's
        current stream).  self.z and self.mode then hold the Kalman stage's measurement; no allocation, no host round trip."""
        if tuple(frames.shape) != (self.n, self.h, self.w, 3) or frames.dtype != self.patches.dtype or not frames.is_contiguous():
            raise ValueError("frames: contiguous uint8 [%d, %d, %d, 3]" % (self.n, self.h, self.w))
        nat.check(self.L.av_egoflow_update(self.ctx.handle, stream or nat.stream_handle(), C.byref(self.cfg), nat.ptr(self.ground), self.n,
                                           self.h, self.w, nat.ptr(frames), nat.ptr(self.patches), nat.ptr(self.valid),
                                           nat.ptr(self.tile_rows), nat.ptr(self.motion), nat.ptr(self.state), nat.ptr(self.z),
                                           nat.ptr(self.mode)))

    # ---- the class surface -----------------------------------------------------------------------------------------------------------
    def update(self, frames):
        """frames: device or host uint8 [n, h, w, 3] rectified frames, the next one of every camera.  -> dict(motion [n, 3] (t_f, t_l,
        omega: metres and radians in the previous frame's road frame), valid [n], n_tiles [n] (accepted tiles), n_inliers [n],
        rms [n] (metres), pose [n, 3] (x, y, psi), z [n, 4], mode [n]: 1 = the filter takes z, 2 = it predicts)."""
        import torch

        if not isinstance(frames, torch.Tensor):
            frames = torch.as_tensor(np.ascontiguousarray(frames, np.uint8))
        if frames.device != self.dev:
            if self._staged is None:
                self._staged = torch.empty(self.n, self.h, self.w, 3, dtype=torch.uint8, device=self.dev)
            if tuple(frames.shape) != tuple(self._staged.shape):
                raise ValueError("frames: uint8 [%d, %d, %d, 3]" % (self.n, self.h, self.w))
            self._staged.copy_(frames)
            frames = self._staged
        self.enqueue(frames.contiguous())
        return self.results()

    def results(self):
        """What the last enqueue() left (synchronises)."""
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        mo = self.motion.cpu().numpy().view(np.dtype(nat.EGOFLOW_MOTION_FIELDS)).reshape(self.n)
        st = self.state.cpu().numpy().view(np.dtype(nat.EGOFLOW_STATE_FIELDS)).reshape(self.n)
        return dict(motion=np.stack([mo["t_f"], mo["t_l"], mo["omega"]], axis=1), valid=mo["valid"].astype(bool),
                    n_tiles=mo["n_accepted"].copy(), n_inliers=mo["n_inliers"].copy(), rms=mo["rms"].copy(),
                    pose=np.stack([st["x"], st["y"], st["psi"]], axis=1), z=self.z.cpu().numpy(), mode=self.mode.cpu().numpy())

    def tiles(self):
        """The last tile table: a structured array [n, tiles_y * tiles_x] of av_egoflow_tile rows (nat.EGOFLOW_TILE_FIELDS; flags:
        nat.EGOFLOW_ACCEPTED / _LIVE / _GATED / _INLIER)."""
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        return self.tile_rows.cpu().numpy().view(np.dtype(nat.EGOFLOW_TILE_FIELDS)).reshape(self.n, self.n_tiles)

    def set_pose(self, pose):
        """pose: [n, 3] (or [3] for all) -- x, y, psi of every camera's ground point in the world; the frame count stays."""
        import torch

        p = np.broadcast_to(np.asarray(pose, np.float64), (self.n, 3))
        torch.cuda.current_stream(self.dev).synchronize()
        st = self.state.cpu().numpy().view(np.dtype(nat.EGOFLOW_STATE_FIELDS)).reshape(self.n).copy()
        st["x"], st["y"], st["psi"] = p[:, 0], p[:, 1], p[:, 2]
        self.state.copy_(torch.as_tensor(st.view(np.uint8).reshape(self.n, nat.EGOFLOW_STATE_BYTES)))
        torch.cuda.current_stream(self.dev).synchronize()

    def reset(self):
        """Pose (0, 0, 0), no previous frame: the next update measures nothing (mode 2)."""
        import torch

        self.state.zero_()
        self.z.zero_()
        self.mode.fill_(2)
        torch.cuda.current_stream(self.dev).synchronize()
