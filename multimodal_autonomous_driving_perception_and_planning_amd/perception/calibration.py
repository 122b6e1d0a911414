"""CameraCalibration: one camera's ground-plane homography (include/avhot.h: av_ground_cfg).

A flat road seen by a pinhole camera is a plane-to-plane projection, so image (u, v) and road (forward, lateral) in metres are
related by a 3 x 3 matrix g up to scale: g (u, v, 1)^T = (F, L, D), forward = F / D, lateral = L / D, lateral > 0 towards the
image's right.  D > 0 means below the horizon and in front of the camera.  g is defined on RECTIFIED pixels; a LensModel
(OpenCV's five-coefficient Brown-Conrady distortion, include/avhot.h: av_lens_cfg) beside it says how the raw frame's pixels
relate to them.

The reference has no camera model; its BEVRenderer places a track by forward = 50 - cy * 0.1, lateral = (cx - 320) * 0.03
(bev_renderer.py:207-208), which from_linear restates as a (degenerate) homography.
"""
import ctypes as C

import numpy as np

from .. import _native as nat

_ANCHORS = {"centre": 0, "center": 0, "bottom": 1}
LINEAR_MAX_RANGE = 1.0e9        # from_linear: the linear map has no horizon and no range limit; av_ground_cfg wants a finite one


_OTHER_MODELS = {8: "rational (k4..k6)", 12: "thin-prism (s1..s4)", 14: "tilted-sensor (tau)"}


class LensModel:
    """OpenCV's five-coefficient Brown-Conrady lens: raw pixel <-> rectified pixel (av_lens_cfg; the operation order is the
    header's, every operation rounded on its own)."""

    def __init__(self, fx, fy, cx, cy, dist=(0.0, 0.0, 0.0, 0.0, 0.0), size=None, new_K=None, model="brown"):
        """fx, fy, cx, cy: the raw frame's intrinsics (pixel c sits at u = c).  dist: (k1, k2, p1, p2, k3), OpenCV's order.
        size: (w, h) of the frames.  new_K: (fx, fy, cx, cy) of the rectified picture, None for the raw ones."""
        if model != "brown":
            raise ValueError('LensModel: the %s model is not supported (the five-coefficient "brown" model only: no rational, '
                             "thin-prism or fisheye terms)" % (model,))
        dist = np.asarray(dist, dtype=np.float64).reshape(-1)
        if dist.size != 5:
            raise ValueError("LensModel: dist is (k1, k2, p1, p2, k3); %d coefficients%s" % (
                dist.size, " are OpenCV's %s model, which is not supported" % _OTHER_MODELS[dist.size]
                if dist.size in _OTHER_MODELS else (" could be OpenCV's fisheye model, which is not supported" if dist.size == 4 else "")))
        if size is None or len(size) != 2:
            raise ValueError("LensModel: size=(w, h) of the frames is needed")
        self.K = tuple(float(v) for v in (fx, fy, cx, cy))
        self.dist = tuple(float(v) for v in dist)
        self.size = (int(size[0]), int(size[1]))
        if new_K is not None and len(new_K) != 4:
            raise ValueError("LensModel: new_K is (fx, fy, cx, cy)")
        self.new_K = self.K if new_K is None else tuple(float(v) for v in new_K)
        self._cfg = self._make()            # (validates: av_lens_make's refusals, with its messages)

    def _make(self):
        out = nat.LensCfg()
        rc = nat.lib().av_lens_make((C.c_double * 4)(*self.K), (C.c_double * 5)(*self.dist), (C.c_double * 4)(*self.new_K),
                                    self.size[0], self.size[1], C.byref(out))
        if rc != 0:
            raise ValueError(nat.lib().av_last_error_string().decode())
        return out

    def cfg(self):
        """A fresh nat.LensCfg (av_lens_make's output)."""
        return self._make()

    def key(self):
        return (self.K, self.dist, self.new_K, self.size)

    def __eq__(self, other):
        return isinstance(other, LensModel) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    # ---- the model in NumPy (vectorised) ----------------------------------------------------------------------------------
    def _model(self, x, y):
        k1, k2, p1, p2, k3 = (np.float64(v) for v in self.dist)
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + (2 * p1 * x * y + p2 * (r2 + 2 * x * x))
        yd = y * rad + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
        drad = k1 + r2 * (2 * k2 + r2 * (3 * k3))
        a = rad + 2 * x * x * drad + (2 * p1 * y + 6 * p2 * x)
        b = 2 * x * y * drad + (2 * p1 * x + 2 * p2 * y)
        d = rad + 2 * y * y * drad + (6 * p1 * y + 2 * p2 * x)
        return xd, yd, a, b, d

    def distort(self, uv):
        """[..., 2] rectified pixels -> [..., 2] raw pixels (the forward model)."""
        uv = np.asarray(uv, dtype=np.float64)
        fx, fy, cx, cy = (np.float64(v) for v in self.K)
        nfx, nfy, ncx, ncy = (np.float64(v) for v in self.new_K)
        xd, yd = self._model((uv[..., 0] - ncx) / nfx, (uv[..., 1] - ncy) / nfy)[:2]
        return np.stack([fx * xd + cx, fy * yd + cy], axis=-1)

    def _newton(self, uv):
        uv = np.asarray(uv, dtype=np.float64)
        fx, fy, cx, cy = (np.float64(v) for v in self.K)
        xd, yd = (uv[..., 0] - cx) / fx, (uv[..., 1] - cy) / fy
        x, y = xd.copy(), yd.copy()
        ok = np.ones(x.shape, dtype=bool)
        with np.errstate(all="ignore"):
            for _ in range(6):
                mx, my, a, b, d = self._model(x, y)
                ex, ey = mx - xd, my - yd
                det = a * d - b * b
                ok &= det > 0.0
                x, y = x - (d * ex - b * ey) / det, y - (a * ey - b * ex) / det
            mx, my, a, b, d = self._model(x, y)
            ex, ey = mx - xd, my - yd
            det = a * d - b * b
            ok &= (det > 0.0) & (ex * ex + ey * ey <= 1e-20)
        return x, y, a, b, d, det, ok

    def undistort(self, uv):
        """[..., 2] raw pixels -> ([..., 2] rectified pixels, [...] valid): six Newton iterations, as the device does."""
        nfx, nfy, ncx, ncy = (np.float64(v) for v in self.new_K)
        x, y, _, _, _, _, ok = self._newton(uv)
        return np.stack([nfx * x + ncx, nfy * y + ncy], axis=-1), ok

    def jacobian(self, uv):
        """[..., 2] raw pixels -> [..., 2, 2]: d(rectified pixel) / d(raw pixel) at each."""
        fx, fy = (np.float64(v) for v in self.K[:2])
        nfx, nfy = (np.float64(v) for v in self.new_K[:2])
        _, _, a, b, d, det, _ = self._newton(uv)
        with np.errstate(all="ignore"):
            J = np.stack([np.stack([(d / det) * (nfx / fx), (-b / det) * (nfx / fy)], axis=-1),
                          np.stack([(-b / det) * (nfy / fx), (a / det) * (nfy / fy)], axis=-1)], axis=-2)
        return J

    def __repr__(self):
        return "LensModel(K=%r, dist=%r, size=%r, new_K=%r)" % (self.K, self.dist, self.size, self.new_K)


class CameraCalibration:
    def __init__(self, g, max_range=80.0, anchor="bottom", lens=None):
        """g: 3 x 3, RECTIFIED image (u, v, 1) -> (F, L, D).  max_range: metres, > 0 and finite; a foot point farther ahead is off
        the road.  anchor: which point of a box touches the road, "bottom" (bottom centre) or "centre".  lens: a LensModel, if the
        camera's frames (and the boxes found in them) are raw, None if they are rectified."""
        if lens is not None and not isinstance(lens, LensModel):
            raise ValueError("lens is a LensModel or None")
        self.lens = lens
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
    def from_pose(cls, fx, fy, cx, cy, height, pitch=0.0, max_range=80.0, anchor="bottom", dist=None, size=None):
        """A pinhole camera (focal lengths fx, fy and principal point cx, cy in pixels) `height` metres above a flat road,
        pitched down by `pitch` radians (positive = down); no roll, no yaw.  g = inv(P), P the road -> image matrix
          [[cx cos t, fx, cx H sin t], [cy cos t - fy sin t, 0, (fy cos t + cy sin t) H], [cos t, 0, H sin t]].
        dist = (k1, k2, p1, p2, k3) with size = (w, h): the frames are raw, lens = LensModel(fx, fy, cx, cy, dist, size), and g
        is defined on the pixels rectified to the same intrinsics."""
        fx, fy, cx, cy, H, t = (float(x) for x in (fx, fy, cx, cy, height, pitch))
        if not (H > 0.0 and fx > 0.0 and fy > 0.0):
            raise ValueError("from_pose: height, fx and fy must be > 0")
        c, s = np.cos(t), np.sin(t)
        P = np.array([[cx * c, fx, cx * H * s], [cy * c - fy * s, 0.0, (fy * c + cy * s) * H], [c, 0.0, H * s]])
        lens = None if dist is None else LensModel(fx, fy, cx, cy, dist=dist, size=size)
        return cls(np.linalg.inv(P), max_range=max_range, anchor=anchor, lens=lens)

    def rectified(self):
        """The same camera on rectified pixels: this calibration without its lens."""
        return self if self.lens is None else CameraCalibration(self.g, max_range=self.max_range, anchor=self.anchor)

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
    def image_to_ground(self, uv, raw=False):
        """[..., 2] image points -> ([..., 2] (forward, lateral), [...] on_road).  raw: the points are raw pixels, undistorted
        through self.lens first (a point with no valid preimage is not on the road)."""
        uv = np.asarray(uv, dtype=np.float64)
        valid = True
        if raw:
            if self.lens is None:
                raise ValueError("image_to_ground(raw=True) needs a calibration with a lens")
            uv, valid = self.lens.undistort(uv)
        g = self.g.reshape(9)
        u, v = uv[..., 0], uv[..., 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            F, L, D = (g[0] * u + g[1] * v) + g[2], (g[3] * u + g[4] * v) + g[5], (g[6] * u + g[7] * v) + g[8]
            f, l = F / D, L / D
            on = (D > 0.0) & (f >= 0.0) & (f <= self.max_range) & valid
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
        return "CameraCalibration(g=%r, max_range=%r, anchor=%r%s)" % (self.g.tolist(), self.max_range, self.anchor,
                                                                       "" if self.lens is None else ", lens=%r" % (self.lens,))


MAX_RIG_CAMERAS = 8             # av_rig_fuse's n_cams


class CameraRig:
    """K calibrated cameras on one vehicle: each camera's road frame (forward, lateral from its own ground point) placed in the
    vehicle's by a mount (x, y, yaw) -- a rotation by yaw, measured from the vehicle's forward axis towards +lateral, and a shift
    (include/avhot.h: av_rig_mount).  pipeline.RigLoop fuses the cameras' obstacle lists through it (av_rig_fuse)."""

    def __init__(self, cameras, mounts):
        """cameras: K CameraCalibrations, each in its own road frame; all of them carry a lens, or none does.
        mounts: K triples (x, y, yaw): metres in the vehicle frame (x forward, y lateral, the library's sense) and radians."""
        cams = list(cameras)
        if not 1 <= len(cams) <= MAX_RIG_CAMERAS or not all(isinstance(c, CameraCalibration) for c in cams):
            raise ValueError("CameraRig: cameras is a list of 1 .. %d CameraCalibrations" % MAX_RIG_CAMERAS)
        try:
            m = np.asarray(mounts, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("CameraRig: mounts is one (x, y, yaw) triple per camera") from None
        if m.shape != (len(cams), 3):
            raise ValueError("CameraRig: mounts is one (x, y, yaw) triple per camera (%d), not an array of shape %r"
                             % (len(cams), m.shape))
        if not np.isfinite(m).all():
            raise ValueError("CameraRig: a mount is not finite")
        lenses_of(cams, len(cams))              # (refuses a rig where some cameras have a lens and some have none)
        self.cameras, self.mounts = cams, m.copy()
        # (cos, sin, x, y) per camera: what the device table holds
        self._csxy = np.array([[np.cos(yaw), np.sin(yaw), x, y] for x, y, yaw in m], dtype=np.float64).reshape(len(cams), 4)

    @classmethod
    def from_poses(cls, poses):
        """One dict per camera: fx, fy, cx, cy, height, and optionally pitch=0.0, yaw=0.0, x=0.0, y=0.0, max_range=80.0,
        anchor="bottom", dist=None, size=None -- CameraCalibration.from_pose's arguments plus the mount."""
        cams, mounts = [], []
        for i, p in enumerate(poses):
            p = dict(p)
            try:
                mounts.append((float(p.pop("x", 0.0)), float(p.pop("y", 0.0)), float(p.pop("yaw", 0.0))))
                cams.append(CameraCalibration.from_pose(**p))
            except TypeError as e:
                raise ValueError("CameraRig.from_poses: camera %d: %s" % (i, e)) from None
        return cls(cams, mounts)

    @property
    def K(self):
        return len(self.cameras)

    def calibrations(self, n_vehicles):
        """The per-camera list of n_vehicles rigs: camera k of vehicle v is entry v * K + k."""
        return list(self.cameras) * int(n_vehicles)

    def mounts_table(self, n_vehicles, device=None):
        """float64 [V, K, 4] of (cos, sin, x, y): av_rig_fuse's `mounts` (device None: a host tensor)."""
        import torch

        t = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(self._csxy, (int(n_vehicles),) + self._csxy.shape)))
        return t if device is None else t.to(device)

    def to_vehicle(self, k, fl):
        """[..., 2] (forward, lateral) in camera k's road frame -> [..., 2] in the vehicle frame (av_rig_fuse's operation order)."""
        fl = np.asarray(fl, dtype=np.float64)
        c, s, mx, my = self._csxy[k]
        f, l = fl[..., 0], fl[..., 1]
        return np.stack([(mx + c * f) - s * l, (my + s * f) + c * l], axis=-1)

    def from_vehicle(self, k, FL):
        """[..., 2] vehicle-frame road points -> [..., 2] in camera k's road frame."""
        FL = np.asarray(FL, dtype=np.float64)
        c, s, mx, my = self._csxy[k]
        dx, dy = FL[..., 0] - mx, FL[..., 1] - my
        return np.stack([c * dx + s * dy, c * dy - s * dx], axis=-1)

    def image_to_vehicle(self, k, uv, raw=False):
        """[..., 2] pixels of camera k -> ([..., 2] vehicle-frame road points, [...] on that camera's road)."""
        fl, on = self.cameras[k].image_to_ground(uv, raw=raw)
        return self.to_vehicle(k, fl), on

    def mount_matrix(self, k):
        """The mount as a homography of the road plane: (F, L, D) in camera k's frame -> the vehicle's."""
        c, s, mx, my = self._csxy[k]
        return np.array([[c, -s, mx], [s, c, my], [0.0, 0.0, 1.0]])

    def vehicle_calibration(self, k):
        """Camera k with the mount folded into its homography, g = M_k g_k: image -> the VEHICLE's (forward, lateral).  Meaningful
        only for a camera whose view lies ahead of the vehicle: on_road wants forward >= 0, which is why av_rig_fuse takes the
        mounts beside the cameras instead of folded into every g."""
        cam = self.cameras[k]
        return CameraCalibration(self.mount_matrix(k) @ cam.g, max_range=cam.max_range, anchor=cam.anchor, lens=cam.lens)

    def __repr__(self):
        return "CameraRig(K=%d, mounts=%r)" % (self.K, self.mounts.tolist())


def ground_table(calibrations, n, device):
    """One CameraCalibration, or a sequence of n of them -> a device uint8 tensor [n, 160] of av_ground_cfg entries."""
    import torch

    cals = [calibrations] * n if isinstance(calibrations, CameraCalibration) else list(calibrations)
    if len(cals) != n or not all(isinstance(c, CameraCalibration) for c in cals):
        raise ValueError("calibration is one CameraCalibration or one per stream (%d)" % n)
    raw = b"".join(bytes(c.cfg()) for c in cals)
    host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(n, C.sizeof(nat.GroundCfg))
    return host.to(device), cals


def lens_table(lenses, n, device):
    """One LensModel, or a sequence of n of them -> (a device uint8 tensor [n, 112] of av_lens_cfg entries, the list)."""
    import torch

    ls = [lenses] * n if isinstance(lenses, LensModel) else list(lenses)
    if len(ls) != n or not all(isinstance(l, LensModel) for l in ls):
        raise ValueError("lens is one LensModel or one per stream (%d)" % n)
    raw = b"".join(bytes(l.cfg()) for l in ls)
    host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(n, C.sizeof(nat.LensCfg))
    return host.to(device), ls


def lenses_of(calibrations, n):
    """The lenses of one calibration or of n of them: None if none has one, a list of n if all have; mixed is refused."""
    cals = [calibrations] * n if isinstance(calibrations, CameraCalibration) else list(calibrations)
    have = [getattr(c, "lens", None) is not None for c in cals]
    if not any(have):
        return None
    if not all(have):
        raise ValueError("calibration: every stream has a lens or none has (streams %s have none)"
                         % ", ".join(str(i) for i, h in enumerate(have) if not h))
    return [c.lens for c in cals]
