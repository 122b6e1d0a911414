"""CPU restatements of av_dets_to_tracker and av_lane_paths (include/avhot.h), test infrastructure.

The detector's float32 boxes become the tracker's int32 boxes the way ObjectDetector._detect_yolo makes them (detector.py:111-121:
map(int, xyxy), float(conf), int(cls)), through an optional class table; the lane fits become a reference path at the reference's
own rows (lane_detector.py:164), placed like a track's centre (tests/obstacles_ref.py), and the lane-centre offset in metres
(get_lane_center_offset, lane_detector.py:253-272).  Plain NumPy scalar arithmetic in the operation order the header states.
"""
import numpy as np

from tests.obstacles_ref import DEFAULT_CFG

# detector name -> the reference's class id (ObjectDetector.CLASSES); names are compared with "_" read as " "
REFERENCE_IDS = {"car": 0, "truck": 1, "person": 2, "pedestrian": 2, "bicycle": 3, "cyclist": 3, "motorcycle": 4, "bus": 5,
                 "traffic light": 6, "stop sign": 7}
# COCO ids of the eight reference classes (car, truck, person, bicycle, motorcycle, bus, traffic light, stop sign)
COCO_OF_REFERENCE = [2, 7, 0, 1, 3, 5, 9, 11]


def coco_class_map():
    """The 80-entry table COCO id -> reference id (-1: no reference class), from the ids alone."""
    m = np.full(80, -1, np.int32)
    for ref_id, coco_id in enumerate(COCO_OF_REFERENCE):
        m[coco_id] = ref_id
    return m


def trunc_sat(x):
    """int(x) saturated to the int32 range, NaN -> 0."""
    x = np.float32(x)
    if np.isnan(x):
        return 0
    if x >= np.float32(2147483648.0):
        return 2147483647
    if x <= np.float32(-2147483648.0):
        return -2147483648
    return int(x)


def dets_to_tracker(src_n, src_box, src_conf, src_cls, class_map, dcap, sentinel=(-9, -9, -9.0)):
    """src_n [F], src_box f32 [F, max_det, 4], src_conf f32 [F, max_det], src_cls i32 [F, max_det], class_map int array or None
    -> det_n i32 [F], det_box i32 [F, dcap, 4], det_cls i32 [F, dcap], det_conf f64 [F, dcap], dropped i32 [F]; rows at or past
    det_n hold `sentinel` (box, class, confidence): the kernel does not write them."""
    src_box, src_conf, src_cls = np.asarray(src_box, np.float32), np.asarray(src_conf, np.float32), np.asarray(src_cls)
    F, max_det = src_cls.shape
    det_n, dropped = np.zeros(F, np.int32), np.zeros(F, np.int32)
    det_box = np.full((F, dcap, 4), sentinel[0], np.int32)
    det_cls = np.full((F, dcap), sentinel[1], np.int32)
    det_conf = np.full((F, dcap), sentinel[2], np.float64)
    for f in range(F):
        n = min(max(int(src_n[f]), 0), max_det)
        kept = 0
        for i in range(n):
            cls = int(src_cls[f, i])
            if class_map is not None:
                if not (0 <= cls < len(class_map)) or int(class_map[cls]) < 0:
                    continue
                cls = int(class_map[cls])
            if kept < dcap:
                det_box[f, kept] = [trunc_sat(v) for v in src_box[f, i]]
                det_cls[f, kept] = cls
                det_conf[f, kept] = np.float64(src_conf[f, i])
            kept += 1
        det_n[f] = min(kept, dcap)
        dropped[f] = kept - det_n[f]
    return det_n, det_box, det_cls, det_conf, dropped


def lane_rows(h, n_points):
    """The image rows the path is sampled at: h down to 0.6 h, nearest first."""
    step = (np.float64(0.4) * np.float64(h)) / np.float64(n_points - 1)
    return np.array([np.float64(h) - np.float64(i) * step for i in range(n_points)], np.float64)


def lane_paths(poly, pts, info, plan_state, ref_stride, h, w, n_points, cfg=None):
    """poly f64 [S, 2, 3], pts i32 [S, 2, 50, 2], info i32 [S, 8], plan_state f64 [S * ref_stride, 4]
    -> (paths: list of S float64 [n_ref, 2] arrays, n_ref i32 [S], lane_offset f64 [S])."""
    c = dict(DEFAULT_CFG)
    c.update(cfg or {})
    x_center, x_scale = np.float64(c["x_center"]), np.float64(c["x_scale"])
    y_far, y_scale = np.float64(c["y_far"]), np.float64(c["y_scale"])
    poly, pts, info = np.asarray(poly, np.float64), np.asarray(pts), np.asarray(info)
    plan_state = np.asarray(plan_state, np.float64).reshape(-1, 4)
    S = len(info)
    paths, n_ref, off = [], np.zeros(S, np.int32), np.full(S, np.nan)
    ys = lane_rows(h, n_points)
    for s in range(S):
        if not (info[s, 0] != 0 and info[s, 1] != 0):
            paths.append(np.zeros((0, 2)))
            continue
        x0, y0, hd = (np.float64(v) for v in plan_state[s * ref_stride][:3])
        cs, sn = np.cos(hd), np.sin(hd)
        c2, s2 = np.cos(hd + np.pi / 2), np.sin(hd + np.pi / 2)
        out = []
        for y in ys:
            xl = (poly[s, 0, 0] * y + poly[s, 0, 1]) * y + poly[s, 0, 2]
            xr = (poly[s, 1, 0] * y + poly[s, 1, 1]) * y + poly[s, 1, 2]
            xc = (xl + xr) / 2.0
            lat = (xc - x_center) * x_scale
            fwd = y_far - y * y_scale
            out.append(((x0 + fwd * cs) + lat * c2, (y0 + fwd * sn) + lat * s2))
        paths.append(np.asarray(out, np.float64))
        n_ref[s] = n_points
        off[s] = (np.float64(w) / 2.0 - np.float64(int(pts[s, 0, 49, 0]) + int(pts[s, 1, 49, 0])) / 2.0) * x_scale
    return paths, n_ref, off


# ---- the golden tracker input as a detector would have produced it ------------------------------------------------------------------

UNMAPPED = [4, 6, 8, 10, 12, 79]              # COCO ids without a reference class (airplane, train, boat, ...)


def floatified_golden(g, frames=None, max_det=16):
    """tests/golden/tracker_sim720.npz's tracker input (in_n / in_box / in_cls / in_conf, the real reference's detector output) as
    float32 detector output: fractions from {0.25, 0.5, 0.75} added to every coordinate (int() removes them), the classes sent
    through the inverse of the COCO table, and an entry of an unmapped class interleaved ahead of every real one and behind the
    last.  -> src_n i32 [F], src_box f32 [F, max_det, 4], src_conf f32 [F, max_det], src_cls i32 [F, max_det]."""
    F = len(g["in_n"]) if frames is None else frames
    rng = np.random.default_rng(720)
    src_n = np.zeros(F, np.int32)
    src_box = np.zeros((F, max_det, 4), np.float32)
    src_conf = np.zeros((F, max_det), np.float32)
    src_cls = np.zeros((F, max_det), np.int32)
    for f in range(F):
        k = 0
        for i in range(int(g["in_n"][f])):
            src_box[f, k] = rng.uniform(0, 1280, 4)
            src_conf[f, k], src_cls[f, k] = 0.99, UNMAPPED[(f + i) % len(UNMAPPED)]
            k += 1
            src_box[f, k] = g["in_box"][f, i].astype(np.float32) + rng.choice([0.25, 0.5, 0.75], 4).astype(np.float32)
            src_conf[f, k], src_cls[f, k] = np.float32(g["in_conf"][f, i]), COCO_OF_REFERENCE[int(g["in_cls"][f, i])]
            k += 1
        src_box[f, k] = rng.uniform(0, 1280, 4)
        src_conf[f, k], src_cls[f, k] = 0.5, UNMAPPED[f % len(UNMAPPED)]
        src_n[f] = k + 1
    assert src_n.max() <= max_det
    return src_n, src_box, src_conf, src_cls
