"""CPU restatement of SceneClassifier (src/tagging/scene_classifier.py:76-303), test infrastructure.

The OpenCV calls it makes come from the oracle's C restatements where they exist (oracle.lane_ref.gray / canny /
houghp: BGR2GRAY, Canny, HoughLinesP); BGR2HSV + inRange and the ksize=1 Laplacian are restated here in NumPy.  The
decision rules follow the reference line by line; tests/golden/scene.npz (recorded from the reference itself) pins them.
`scene_frame` is the fixture's frame generator: oracle.lane_ref.synthetic_frame plus a small variant id.
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import lane_ref  # noqa: E402

ROAD_TYPES = ["unknown", "intersection", "highway", "urban", "residential", "parking"]
CONDITIONS = ["clear", "congested", "night", "day", "rain", "fog"]
ELEMENTS = ["traffic_light", "stop_sign", "crosswalk", "yield_sign", "speed_limit"]
UNKNOWN, INTERSECTION, HIGHWAY, URBAN, RESIDENTIAL, PARKING = range(6)
CLEAR, CONGESTED, NIGHT, DAY, RAIN, FOG = range(6)

# frame variants of the fixture (restated by the GPU tests from the same parameters)
V_PLAIN, V_DARK, V_GREEN, V_FLAT, V_LINES, V_CENTER, V_BRIGHT = range(7)


def scene_frame(h, w, stream, frame, variant=V_PLAIN):
    """synthetic_frame(h, w, stream, frame) modified by `variant` (pure integer arithmetic)."""
    img = lane_ref.synthetic_frame(h, w, stream, frame).astype(np.int64)
    y, x = np.mgrid[0:h, 0:w]
    if variant == V_DARK:
        img = img // 4
    elif variant == V_GREEN:
        on = x < (3 * w) // 10
        img[on] = (40, 140 + (frame % 8), 50)
    elif variant == V_FLAT:
        img = 100 + (img - 100) // 16
    elif variant == V_LINES:
        img[:] = 90
        for k in range(8):
            y0 = (h * (k + 1)) // 10
            img[(y >= y0) & (y < y0 + 3)] = 230
    elif variant == V_CENTER:
        on = (y >= h // 3) & (y < 2 * h // 3) & (x >= w // 3) & (x < 2 * w // 3)
        chk = (((y // 4) + (x // 4)) % 2) * 255
        for c in range(3):
            img[..., c] = np.where(on, chk, img[..., c])
    elif variant == V_BRIGHT:
        img = 128 + img // 2
    return img.astype(np.uint8)


def bgr2hsv(bgr):
    """cv2.cvtColor(bgr, COLOR_BGR2HSV) for u8 (OpenCV RGB2HSV_b: hsv_shift 12, rounded division tables)."""
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    i = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sdiv = np.where(i > 0, np.rint((255 << 12) / i), 0).astype(np.int64)
        hdiv = np.where(i > 0, np.rint((180 << 12) / (6.0 * i)), 0).astype(np.int64)
    v = np.maximum(b, np.maximum(g, r))
    vmin = np.minimum(b, np.minimum(g, r))
    diff = v - vmin
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], -1).astype(np.uint8)


def in_range(hsv, lo, hi):
    """cv2.inRange with inclusive per-channel bounds -> u8 mask of 0 / 255."""
    ok = np.ones(hsv.shape[:2], bool)
    for c in range(3):
        ok &= (hsv[..., c] >= lo[c]) & (hsv[..., c] <= hi[c])
    return ok.astype(np.uint8) * 255


def laplacian(gray):
    """cv2.Laplacian(gray, CV_64F) (ksize=1: [0,1,0; 1,-4,1; 0,1,0], BORDER_REFLECT_101) as exact int64."""
    p = np.pad(gray.astype(np.int64), 1, mode="reflect")
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * p[1:-1, 1:-1]


def hough_lines(edges, cap=4096):
    """cv2.HoughLinesP(edges, 1, pi/180, 100, minLineLength=100, maxLineGap=10) -> int32 [n, 4] (at most cap)."""
    return lane_ref.houghp(edges.copy(), 100, 100, 10, max_lines=cap)


def frame_stats(bgr, cap=4096):
    """Everything the classifier reads from the pixels, in the device's terms (exact sums) and NumPy's."""
    h, w = bgr.shape[:2]
    gray = lane_ref.gray(bgr)
    edges = lane_ref.canny(gray, 50, 150)
    center = edges[h // 3:2 * h // 3, w // 3:2 * w // 3]
    lines = hough_lines(edges, cap)
    lens = [np.sqrt((l[2] - l[0]) ** 2 + (l[3] - l[1]) ** 2) for l in lines]
    green = in_range(bgr2hsv(bgr), (35, 40, 40), (85, 255, 255))
    lap = laplacian(gray)
    n = h * w
    ls, lq = int(lap.sum()), int((lap * lap).sum())
    return dict(
        gray_sum=int(gray.sum(dtype=np.int64)), green_count=int(np.sum(green > 0)), lap_sum=ls, lap_sumsq=lq,
        center_count=int(np.sum(center > 0)), n_lines=len(lines), overflow=int(len(lines) >= cap),
        avg_length=float(np.mean(lens)) if len(lens) else 0.0, mean=float(np.mean(gray)),
        green_ratio=float(np.sum(green > 0) / green.size), center_density=float(np.sum(center > 0) / center.size),
        lap_var=(n * lq - ls * ls) / (n * n), lap_var_np=float(lap.astype(np.float64).var()), lines=lines)


def lane_input(frame_shape, lanes):
    """(mode, left_x, right_x) of a `lanes` argument: mode 0 = falsy, 1 = a lane is None, 2 = both present.
    Sequences: the reference's lanes[k][1] * h + lanes[k][0], or w//3 / 2w//3 when shorter than 2 (:271-272); objects
    with a `polynomial` (LaneLine): np.polyval(polynomial, h) -- the port's documented deviation (the reference raises
    TypeError on len(LaneLine))."""
    if not lanes:
        return 0, 0.0, 0.0
    if lanes[0] is None or lanes[1] is None:
        return 1, 0.0, 0.0
    h, w = frame_shape[:2]

    def x_at(lane, fallback):
        if hasattr(lane, "polynomial"):
            return float(np.polyval(lane.polynomial, h))
        return lane[1] * h + lane[0] if len(lane) >= 2 else fallback

    return 2, x_at(lanes[0], w // 3), x_at(lanes[1], 2 * w // 3)


def lane_count(mode, lx, rx):
    if mode == 0:
        return 0
    if mode == 1:
        return 2
    lw = abs(rx - lx)
    return 3 if lw > 200 else (2 if lw > 100 else 1)


def decide(st, detections, mode, speed):
    """_classify_road_type's rules (:128-202) and _analyze_conditions (:231-259) from the pixel statistics.
    detections: list of class names (None for an object without class_name); speed None = no vehicle_state."""
    sc = [0.0] * 6
    if st["center_density"] > 0.15:
        sc[INTERSECTION] += 0.4
    if st["n_lines"] > 5 and st["avg_length"] > 150:
        sc[HIGHWAY] += 0.5
    elements, has_ped = [], False
    if detections:
        traffic = sum(1 for c in detections if c in ("traffic_light", "stop_sign"))
        if traffic > 0:
            sc[INTERSECTION] += 0.3
            sc[URBAN] += 0.2
        veh = sum(1 for c in detections if c in ("car", "truck", "bus"))
        if veh > 3:
            sc[URBAN] += 0.3
            sc[HIGHWAY] += 0.2
        elif veh <= 1:
            sc[RESIDENTIAL] += 0.3
        has_ped = any(c == "pedestrian" for c in detections)
        elements = [ELEMENTS.index(c) for c in detections if c in ("traffic_light", "stop_sign")]
    if st["green_ratio"] > 0.15:
        sc[RESIDENTIAL] += 0.3
    if mode == 2:
        sc[HIGHWAY] += 0.2
        sc[URBAN] += 0.1
    total = sum(sc) + 0.001
    norm = [v / total for v in sc]
    best = max(range(6), key=lambda k: norm[k])
    conf = norm[best]
    if conf < 0.3:
        best, conf = URBAN, 0.3
    cond = []
    if st["mean"] < 60:
        cond.append((NIGHT, 0.8))
    elif st["mean"] > 120:
        cond.append((DAY, 0.8))
    else:
        cond.append((DAY, 0.5))
    if speed is not None:
        if speed < 2.0:
            cond.append((CONGESTED, 0.7))
        elif speed > 15.0:
            cond.append((CLEAR, 0.7))
    if st["lap_var_np"] < 100:
        cond.append((FOG, 0.3))
    return dict(road_type_raw=best, confidence=conf, scores=norm, conditions=cond, elements=elements, has_pedestrian=has_ped)


class SceneRef:
    """Stateful restatement: timestamp, the 5-deep history and the vote of _smooth_tags."""

    def __init__(self, cap=4096):
        self.cap = cap
        self.frame_count = 0
        self.history = []

    def classify_stats(self, st, frame_shape, detections=None, lanes_in=(0, 0.0, 0.0), speed=None):
        d = decide(st, detections, lanes_in[0], speed)
        d["lane_count"] = lane_count(*lanes_in)
        d["timestamp"] = self.frame_count / 30.0
        rec = [d["road_type_raw"]]
        self.history.append(rec)
        if len(self.history) > 5:
            self.history.pop(0)
        self.frame_count += 1
        if len(self.history) >= 2:
            votes = {}
            for r in self.history:
                votes[r[0]] = votes.get(r[0], 0) + 1
            win = max(votes, key=votes.get)
            if votes[win] > len(self.history) // 2:
                rec[0] = win
        d["road_type"] = rec[0]
        d["history"] = [r[0] for r in self.history]
        return d

    def classify(self, frame, detections=None, lanes=None, speed=None):
        st = frame_stats(frame, self.cap)
        d = self.classify_stats(st, frame.shape, detections, lane_input(frame.shape, lanes), speed)
        d["stats"] = st
        return d
