"""Host-side restatements for the view tests (tests/test_fmtnum_host.py, test_view_host.py, test_gpu_view.py): the number-text
cases and their expected strings, the worst-case primitive count of the camera view, BGR -> I420 in NumPy."""
import math

import numpy as np


def fmt_expected(v, d):
    """What av_format_fixed documents: Python's % operator, and "inf" / "-inf" for a finite |v| >= 1e9."""
    if math.isfinite(v) and abs(v) >= 1e9:
        return "-inf" if v < 0 else "inf"
    return "%.*f" % (d, v)


def fmt_values():
    """The values every decimals setting is checked on (about 47 000; times d = 0, 1, 2)."""
    rng = np.random.RandomState(11)
    k = np.arange(4000, dtype=np.float64)
    parts = [
        k + 0.05, -(k + 0.05), k + 0.005, k + 0.5, k * 0.1 + 0.05,                       # decimal ties (most are not exact in binary)
        np.array([0.125, 2.675, 1.005, 0.375, 0.995, 1.115, 8.345, 0.045, 0.5, 1.5, 2.5, 0.25, 0.35]),
        (2 * k + 1) / 2, (2 * k + 1) / 20, -(2 * k + 1) / 2, (2 * k + 1) / 8, (2 * k + 1) / 200,   # binary ties where the quotient is exact
        rng.rand(6000).astype(np.float32).astype(np.float64),                            # detector confidences
        (np.arange(1001) / 1000.0).astype(np.float32).astype(np.float64),
        np.float32([0.995, 0.125, 0.375, 0.005, 0.015]).astype(np.float64),
        rng.uniform(-1e9, 1e9, 6000), rng.uniform(-1e3, 1e3, 4000), rng.uniform(-1.0, 1.0, 2000),
        999999999.0 + rng.rand(200), -(999999999.0 + rng.rand(200)),
        np.array([0.0, -0.0, -0.04, 0.04, -0.004, -0.5, -0.05, -0.005, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310,
                  float("nan"), -float("nan"), float("inf"), -float("inf"), 1e9, -1e9, 1e9 + 1, 1e300, -1e300,
                  np.nextafter(1e9, 0), -np.nextafter(1e9, 0), 999999999.995, 999999999.5, 123456.78, 100000.05, -100000.05]),
    ]
    return np.concatenate([np.asarray(p, np.float64).ravel() for p in parts])


def camview_prim_cap(max_det, tcap, L, max_name):
    """Slots a camera's list can need, counted from the layers' definitions: a number is at most 14 characters
    ("-1000000000.00"), an int32 at most 11."""
    num, integer = 14, 11
    det_name = max(max_name, len("unknown"))
    det = 4 + 1 + (det_name + 1 + num)                                     # outline, label box, "name 0.87"
    lanes = 1 + 2 * 49                                                      # area, two polylines of 50 points
    trk = 4 + (len("ID:") + integer + 1 + max(max_name, integer)) + (L - 1)   # outline, "ID:n name", trail
    info = 1 + (len("Frame: ") + integer) + (len("FPS: ") + num) + (len("Speed: ") + num + len(" km/h")) + (
        len("Heading: ") + num + len(" deg")) + (len("Accel: ") + num + len(" m/s2")) + (len("Pos: (, )") + 2 * num)
    summary = 1 + len("Detections:") + max_det * (len("  : ") + det_name + integer)
    gauge = 1 + 4 + 1 + 1 + (len("Offset: px") + num)
    return max_det * det + lanes + tcap * trk + info + summary + gauge


def bgr_to_i420(bgr):
    """uint8 [h, w, 3] (even sizes) -> I420 bytes [h * w * 3 / 2]: BT.601 limited range in OpenCV's 20-bit constants, chroma from the
    rounded mean colour of every 2 x 2 block (av_bgr_to_i420's statement in include/avhot.h)."""
    h, w = bgr.shape[:2]
    p = bgr.astype(np.int64)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    y = (269484 * r + 528482 * g + 102760 * b + (16 << 20) + (1 << 19)) >> 20
    m = (p.reshape(h // 2, 2, w // 2, 2, 3).sum(axis=(1, 3)) + 2) >> 2
    b, g, r = m[..., 0], m[..., 1], m[..., 2]
    u = (-155188 * r - 305135 * g + 460324 * b + (128 << 20) + (1 << 19)) >> 20
    v = (460324 * r - 385875 * g - 74448 * b + (128 << 20) + (1 << 19)) >> 20
    return np.concatenate([np.clip(a, 0, 255).astype(np.uint8).ravel() for a in (y, u, v)])
