"""Rig odometry: a vehicle's ego motion from the road pixels of all K cameras of its rig, fitted together in the vehicle frame
(include/avhot.h: av_rig_egoflow_*, csrc/rigflow.hip).  GroundOdometry's patch and match stages per camera;
the solve pools every camera's tiles through the mounts."""
import ctypes as C

import numpy as np

from .. import _native as nat
from .calibration import CameraRig, ground_table
from .ground_odometry import egoflow_cfg


class RigOdometry:
    """n_vehicles rigs' planar ego motion, frame to frame, and the Kalman stage's measurement from it -- all on the device.

    Shaped like GroundOdometry, whose geometry and settings it takes (gh, gw, f_far, m_per_px, tile, search, frame_rate,
    min_texture, gate_px, inlier_px, min_inliers: one patch of that geometry per camera).  Camera k of vehicle v is frame
    v * K + k.  The motion (t_f, t_l, omega) and the pose (x, y, psi) are those of the VEHICLE's origin: every camera's gated
    tiles are carried through its mount into the vehicle frame and fitted together, so a camera's lever arm falls out, the yaw
    has the rig's whole baseline, cameras with too few tiles each still measure together, and a camera whose whole patch shows
    something else than the road is dropped (results()' views and hypothesis say which cameras the fit rests on)."""

    def __init__(self, rig, n_vehicles, h, w, gh=256, gw=256, f_far=None, m_per_px=0.1, tile=16, search=12, frame_rate=30.0,
                 min_texture=None, gate_px=3, inlier_px=1.0, min_inliers=8, device=0, ctx=None):
        # the geometry is checked first: a bad one is refused without a GPU
        self.cfg, self.tiles_y, self.tiles_x = egoflow_cfg(gh, gw, f_far, m_per_px, tile, search, frame_rate, min_texture, gate_px,
                                                           inlier_px, min_inliers)
        if not isinstance(rig, CameraRig):
            raise ValueError("RigOdometry: rig is a perception.CameraRig")
        self.rig, self.V, self.K, self.h, self.w = rig, int(n_vehicles), rig.K, int(h), int(w)
        if self.V < 1 or self.h < 1 or self.w < 1:
            raise ValueError("n_vehicles, h and w must be >= 1")
        if self.V * self.K > 65535:
            raise ValueError("RigOdometry: more than 65535 cameras")
        if any(c.lens is not None for c in rig.cameras):
            raise ValueError("GroundOdometry reads RECTIFIED frames: pass calibration.rectified() and rectify the frames first")
        self.n, self.n_tiles = self.V * self.K, self.tiles_y * self.tiles_x
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("RigOdometry needs a HIP device; this package has no CPU path")
        self.dev = torch.device("cuda", device)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.ground, self.calibration = ground_table(rig.calibrations(self.V), self.n, self.dev)
        self.mounts = rig.mounts_table(self.V, self.dev)                                # float64 [V, K, 4]
        n, V, d, u8 = self.n, self.V, self.dev, torch.uint8
        gh, gw = self.cfg.gh, self.cfg.gw
        self.patches = torch.zeros(n, 2, gh, gw, dtype=u8, device=d)                    # the ping-pong pairs, one per camera
        self.valid = torch.zeros(n, gh, (gw + 31) // 32, dtype=torch.int32, device=d)   # a bit per patch pixel
        self.tile_rows = torch.zeros(n, self.n_tiles, nat.EGOFLOW_TILE_BYTES, dtype=u8, device=d)
        self.motion = torch.zeros(V, nat.EGOFLOW_MOTION_BYTES, dtype=u8, device=d)
        self.info = torch.zeros(V, nat.RIG_EGOFLOW_INFO_BYTES, dtype=u8, device=d)
        self.state = torch.zeros(V, nat.EGOFLOW_STATE_BYTES, dtype=u8, device=d)        # one per vehicle
        self.z = torch.zeros(V, 4, dtype=torch.float64, device=d)                       # what av_kf_step reads, window 1
        self.mode = torch.full((V,), 2, dtype=u8, device=d)
        self._staged = None
        torch.cuda.current_stream(d).synchronize()

    # ---- the per-frame path: enqueue only ------------------------------------------------------------------------------------------
    def enqueue(self, frames, stream=None):
        """All stages for device frames uint8 [V * K, h, w, 3] (rectified) on `stream` (a hipStream_t as c_void_p; default: torch's
        current stream).  self.z and self.mode then hold the Kalman stage's measurement; no allocation, no host round trip."""
        if tuple(frames.shape) != (self.n, self.h, self.w, 3) or frames.dtype != self.patches.dtype or not frames.is_contiguous():
            raise ValueError("frames: contiguous uint8 [%d, %d, %d, 3]" % (self.n, self.h, self.w))
        nat.check(self.L.av_rig_egoflow_update(self.ctx.handle, stream or nat.stream_handle(), C.byref(self.cfg), nat.ptr(self.ground),
                                               nat.ptr(self.mounts), self.V, self.K, self.h, self.w, nat.ptr(frames),
                                               nat.ptr(self.patches), nat.ptr(self.valid), nat.ptr(self.tile_rows), nat.ptr(self.motion),
                                               nat.ptr(self.info), nat.ptr(self.state), nat.ptr(self.z), nat.ptr(self.mode)))

    # ---- the class surface -----------------------------------------------------------------------------------------------------------
    def update(self, frames):
        """frames: device or host uint8 [V * K, h, w, 3] rectified frames, the next one of every camera.  -> results()."""
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
        """What the last enqueue() left (synchronises): dict(motion [V, 3] (t_f, t_l, omega of the vehicle's origin: metres and
        radians in the previous frame's vehicle frame), valid [V], n_tiles [V] (accepted tiles of all cameras), n_inliers [V],
        rms [V] (metres), pose [V, 3] (x, y, psi of the vehicle's origin), z [V, 4], mode [V] (1 = the filter takes z, 2 = it
        predicts), views [V] (bit k: camera k has an inlier), hypothesis [V] (what the inliers were chosen by: 0 the pooled fit,
        1 + k camera k's own, -1 none) and cam_inliers [V, K])."""
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        V = self.V
        mo = self.motion.cpu().numpy().view(np.dtype(nat.EGOFLOW_MOTION_FIELDS)).reshape(V)
        st = self.state.cpu().numpy().view(np.dtype(nat.EGOFLOW_STATE_FIELDS)).reshape(V)
        inf = self.info.cpu().numpy().view(np.dtype(nat.RIG_EGOFLOW_INFO_FIELDS)).reshape(V)
        return dict(motion=np.stack([mo["t_f"], mo["t_l"], mo["omega"]], axis=1), valid=mo["valid"].astype(bool),
                    n_tiles=mo["n_accepted"].copy(), n_inliers=mo["n_inliers"].copy(), rms=mo["rms"].copy(),
                    pose=np.stack([st["x"], st["y"], st["psi"]], axis=1), z=self.z.cpu().numpy(), mode=self.mode.cpu().numpy(),
                    views=inf["views"].copy(), hypothesis=inf["hypothesis"].copy(), cam_inliers=inf["cam_inliers"][:, :self.K].copy())

    def tiles(self):
        """The last tile tables: a structured array [V, K, tiles_y * tiles_x] of av_egoflow_tile rows (nat.EGOFLOW_TILE_FIELDS; flags:
        nat.EGOFLOW_ACCEPTED / _LIVE / _GATED / _INLIER)."""
        import torch

        torch.cuda.current_stream(self.dev).synchronize()
        return self.tile_rows.cpu().numpy().view(np.dtype(nat.EGOFLOW_TILE_FIELDS)).reshape(self.V, self.K, self.n_tiles)

    def set_pose(self, pose):
        """pose: [V, 3] (or [3] for all) -- x, y, psi of every vehicle's origin in the world; the frame count stays."""
        import torch

        p = np.broadcast_to(np.asarray(pose, np.float64), (self.V, 3))
        torch.cuda.current_stream(self.dev).synchronize()
        st = self.state.cpu().numpy().view(np.dtype(nat.EGOFLOW_STATE_FIELDS)).reshape(self.V).copy()
        st["x"], st["y"], st["psi"] = p[:, 0], p[:, 1], p[:, 2]
        self.state.copy_(torch.as_tensor(st.view(np.uint8).reshape(self.V, nat.EGOFLOW_STATE_BYTES)))
        torch.cuda.current_stream(self.dev).synchronize()

    def reset(self):
        """Pose (0, 0, 0), no previous frame: the next update measures nothing (mode 2)."""
        import torch

        self.state.zero_()
        self.z.zero_()
        self.mode.fill_(2)
        torch.cuda.current_stream(self.dev).synchronize()
