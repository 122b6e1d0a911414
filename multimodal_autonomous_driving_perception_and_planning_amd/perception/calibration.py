"""CameraCalibration: one camera's ground-plane homography (include/avhot.h: av_ground_cfg).

A flat road seen by a pinhole camera is a plane-to-plane projection, so image (u, v) and road (forward, lateral) in metres are
related by a 3 x 3 matrix g up to scale: g (u, v, 1)^T = (F, L, D), forward = F / D, lateral = L / D, lateral > 0 towards the
image's right.  D > 0 means below the horizon and in front of the camera.  Frames are taken as rectified (no lens distortion).

The reference has no camera model; its BEVRenderer places a track by forward = 50 - cy * 0.1, lateral = (cx - 320) * 0.03
(bev_renderer.py:207-208), which from_linear restates as a (degenerate) homography.
"""
import ctypes as C

import numpy as np

from .. import _native as nat

_ANCHORS = {"centre": 0, "center": 0, "bottom": 1}
LINEAR_MAX_RANGE = 1.0e9        # from_linear: the linear map has no horizon and no range limit; av_ground_cfg wants a finite one


class CameraCalibration:
    def __init__(self, g, max_range=80.0, anchor="bottom"):
        """g: 3 x 3, image (u, v, 1) -> (F, L, D).  max_range: metres, > 0 and finite; a foot point farther ahead is off the
        road.  anchor: which point of a box touches the road, "bottom" (bottom centre) or "centre"."""
        g = np.asarray(g, dtype=np.float64)
        if g.shape != (3, 3):
            raise ValueError("g is a 3 x 3 matrix")
        if anchor not in _ANCHORS:
            raise ValueError('anchor is "bottom" or "centre"')
        self.g = g.copy()
        self.max_range = float(max_range)
        self.anchor = "centre" if _ANCHORS[anchor] == 0 else "bottom"
        self._cfg = self._make()            # (validates: singular g, non-finite entries, max_range)
        self.ginv = np.array(self._cfg.ginv, dtype=np.float64).reshape(3, 3)

    def _make(self):
        out = nat.GroundCfg()
        flat = (C.c_double * 9)(*self.g.reshape(9))
        rc = nat.lib().av_ground_make(flat, self.max_range, _ANCHORS[self.anchor], C.byref(out))
        if rc != 0:
            raise ValueError(nat.lib().av_last_error_string().decode())
        return out

    def cfg(self):
        """A fresh nat.GroundCfg (av_ground_make's output) for this camera."""
        return self._make()

    # ---- constructors ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_pose(cls, fx, fy, cx, cy, height, pitch=0.0, max_range=80.0, anchor="bottom"):
        """A pinhole camera (focal lengths fx, fy and principal point cx, cy in pixels) `height` metres above a flat road,
        pitched down by `pitch` radians (positive = down); no roll, no yaw.  g = inv(P), P the road -> image matrix
          [[cx cos t, fx, cx H sin t], [cy cos t - fy sin t, 0, (fy cos t + cy sin t) H], [cos t, 0, H sin t]]."""
        fx, fy, cx, cy, H, t = (float(x) for x in (fx, fy, cx, cy, height, pitch))
        if not (H > 0.0 and fx > 0.0 and fy > 0.0):
            raise ValueError("from_pose: height, fx and fy must be > 0")
        c, s = np.cos(t), np.sin(t)
        P = np.array([[cx * c, fx, cx * H * s], [cy * c - fy * s, 0.0, (fy * c + cy * s) * H], [c, 0.0, H * s]])
        return cls(np.linalg.inv(P), max_range=max_range, anchor=anchor)

    @classmethod
    def from_points(cls, image_pts, ground_pts, max_range=80.0, anchor="bottom"):
        """g from at least four correspondences image (u, v) <-> road (forward, lateral), by the direct linear transform
        (normalised coordinates, NumPy's SVD).  The sign is chosen so that D > 0 at the given image points; ValueError if they
        disagree about it or the points are degenerate (fewer than four, three on a line, ...)."""
        ip = np.asarray(image_pts, dtype=np.float64)
        gp = np.asarray(ground_pts, dtype=np.float64)
        if ip.ndim != 2 or ip.shape[1] != 2 or ip.shape != gp.shape or ip.shape[0] < 4:
            raise ValueError("from_points: at least 4 pairs of (u, v) and (forward, lateral)")
        if not (np.isfinite(ip).all() and np.isfinite(gp).all()):
            raise ValueError("from_points: non-finite coordinates")

        def normalise(p):
            m, d = p.mean(0), np.sqrt(((p - p.mean(0)) ** 2).sum(1)).mean()
            if not d > 0.0:
                raise ValueError("from_points: degenerate points")
            k = np.sqrt(2.0) / d
            T = np.array([[k, 0.0, -k * m[0]], [0.0, k, -k * m[1]], [0.0, 0.0, 1.0]])
            return (p - m) * k, T

        a, Ta = normalise(ip)
        b, Tb = normalise(gp)
        rows = []
        for (u, v), (f, l) in zip(a, b):
            rows.append([u, v, 1.0, 0.0, 0.0, 0.0, -f * u, -f * v, -f])
            rows.append([0.0, 0.0, 0.0, u, v, 1.0, -l * u, -l * v, -l])
        _, sv, vt = np.linalg.svd(np.asarray(rows))
        # one null direction only: the eighth singular value of the 2n x 9 system must stand clear of zero
        if not sv[7] > 1e-9 * sv[0]:
            raise ValueError("from_points: degenerate points (the correspondences do not fix a homography)")
        g = np.linalg.inv(Tb) @ vt[-1].reshape(3, 3) @ Ta
        if not abs(np.linalg.det(g)) > 0.0:
            raise ValueError("from_points: degenerate points")
        D = ip @ g[2, :2] + g[2, 2]
        if (D > 0.0).all():
            pass
        elif (D < 0.0).all():
            g = -g
        else:
            raise ValueError("from_points: the image points lie on both sides of the horizon of the fitted model")
        # a scale that keeps the entries readable: D = 1 at the image points' centroid
        g = g / (ip.mean(0) @ g[2, :2] + g[2, 2])
        return cls(g, max_range=max_range, anchor=anchor)

    @classmethod
    def from_linear(cls, x_center, x_scale, y_far, y_scale, max_range=LINEAR_MAX_RANGE):
        """The linear map of av_obstacle_cfg, lateral = (cx - x_center) * x_scale, forward = y_far - cy * y_scale, at the box
        centre: no horizon (D = 1 everywhere) and, in place of no range limit, a large finite one."""
        xc, xs, yf, ys = (float(x) for x in (x_center, x_scale, y_far, y_scale))
        return cls([[0.0, -ys, yf], [xs, 0.0, -xc * xs], [0.0, 0.0, 1.0]], max_range=max_range, anchor="centre")

    # ---- the projection in NumPy (vectorised; the operation order is the header's) --------------------------------------------
    def image_to_ground(self, uv):
        """[..., 2] image points -> ([..., 2] (forward, lateral), [...] on_road)."""
        uv = np.asarray(uv, dtype=np.float64)
        g = self.g.reshape(9)
        u, v = uv[..., 0], uv[..., 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            F, L, D = (g[0] * u + g[1] * v) + g[2], (g[3] * u + g[4] * v) + g[5], (g[6] * u + g[7] * v) + g[8]
            f, l = F / D, L / D
            on = (D > 0.0) & (f >= 0.0) & (f <= self.max_range)
        return np.stack([f, l], axis=-1), on

    def ground_to_image(self, fl):
        """[..., 2] road points (forward, lateral) -> ([..., 2] (u, v), [...] visible: in front of the camera, D' > 0)."""
        fl = np.asarray(fl, dtype=np.float64)
        q = self.ginv.reshape(9)
        f, l = fl[..., 0], fl[..., 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            U, V, D = (q[0] * f + q[1] * l) + q[2], (q[3] * f + q[4] * l) + q[5], (q[6] * f + q[7] * l) + q[8]
            uv = np.stack([U / D, V / D], axis=-1)
        return uv, D > 0.0

    def __repr__(self):
        return "CameraCalibration(g=%r, max_range=%r, anchor=%r)" % (self.g.tolist(), self.max_range, self.anchor)


def ground_table(calibrations, n, device):
    """One CameraCalibration, or a sequence of n of them -> a device uint8 tensor [n, 160] of av_ground_cfg entries."""
    import torch

    cals = [calibrations] * n if isinstance(calibrations, CameraCalibration) else list(calibrations)
    if len(cals) != n or not all(isinstance(c, CameraCalibration) for c in cals):
        raise ValueError("calibration is one CameraCalibration or one per stream (%d)" % n)
    raw = b"".join(bytes(c.cfg()) for c in cals)
    host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(n, C.sizeof(nat.GroundCfg))
    return host.to(device), cals
