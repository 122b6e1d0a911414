#!/usr/bin/env python3
"""Generate tests/golden/scene.npz by running the REAL reference SceneClassifier and AutoTagger.

Runs only where the reference checkout is available (AV_REFERENCE, default: a `reference` directory beside this
repository); only the .npz is committed.
`cv2` is not installed, so a stand-in module is registered under that name, backed by the CPU restatements in
tests/scene_ref.py (oracle.lane_ref's gray / Canny / PPHT, NumPy HSV / inRange / Laplacian).  That pins the reference's
decision logic; the OpenCV primitives themselves stay unpinned, as they are for the lane detector.

scene_classifier.py, maneuver_detector.py, interaction_detector.py and auto_tagger.py are loaded from their files under
a stub `src.tagging` package: the real package __init__ imports the VLM tagger.  Frames are stored as generator
parameters (scene_ref.scene_frame(h, w, stream, frame, variant)), not as pixels.

Usage:  python tests/golden/make_golden_scene.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AV_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))
sys.path.insert(0, os.path.dirname(OUT))
import scene_ref as sr  # noqa: E402

H, W = 360, 640
NAMES = ["car", "truck", "bus", "pedestrian", "traffic_light", "stop_sign", "cyclist", "person"]
KMAX = 8
LANE_CASES = {          # kind -> lanes argument (sequences as the reference indexes them: lanes[k][1] * h + lanes[k][0])
    0: None,
    1: (None, None),
    2: ((120.0, 0.2), None),
    3: ((100.0, 0.0), (150.0, 0.05)),      # width 68  -> 1 lane
    4: ((100.0, 0.1), (250.0, 0.0)),       # width 114 -> 2
    5: ((50.0, 0.0), (400.0, 0.0)),        # width 350 -> 3
    6: ((5.0,), (7.0,)),                   # len < 2 -> w//3, 2w//3
}


def _cv2_standin():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2GRAY, cv2.COLOR_BGR2HSV, cv2.CV_64F = 6, 40, 6

    def cvtColor(img, code):
        if code == cv2.COLOR_BGR2GRAY:
            return sr.lane_ref.gray(img)
        if code == cv2.COLOR_BGR2HSV:
            return sr.bgr2hsv(img)
        raise NotImplementedError(code)

    def Canny(img, lo, hi):
        return sr.lane_ref.canny(img, int(lo), int(hi))

    def HoughLinesP(edges, rho, theta, threshold, minLineLength=0, maxLineGap=0):
        assert rho == 1 and abs(theta - np.pi / 180) < 1e-15
        lines = sr.lane_ref.houghp(edges.copy(), int(threshold), int(minLineLength), int(maxLineGap), max_lines=1 << 16)
        return None if len(lines) == 0 else lines.reshape(-1, 1, 4)

    def inRange(img, lo, hi):
        return sr.in_range(img, lo, hi)

    def Laplacian(img, ddepth):
        assert ddepth == cv2.CV_64F
        return sr.laplacian(img).astype(np.float64)

    cv2.cvtColor, cv2.Canny, cv2.HoughLinesP, cv2.inRange, cv2.Laplacian = cvtColor, Canny, HoughLinesP, inRange, Laplacian
    return cv2


def _load_reference():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not found at %s" % REF)
    sys.modules["cv2"] = _cv2_standin()
    src = types.ModuleType("src")
    src.__path__ = [os.path.join(REF, "src")]
    pkg = types.ModuleType("src.tagging")
    pkg.__path__ = [os.path.join(REF, "src", "tagging")]
    sys.modules["src"], sys.modules["src.tagging"] = src, pkg
    mods = {}
    for name in ("scene_classifier", "maneuver_detector", "interaction_detector", "auto_tagger"):
        full = "src.tagging." + name
        spec = importlib.util.spec_from_file_location(full, os.path.join(REF, "src", "tagging", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def plan():
    """Per frame: (stream, frame, variant, detections [(name index, conf)], speed or NaN (= vehicle_state None), lane kind,
    reset).  The vote counts smoothed road types, so the first majority of a sequence sticks: every clip (add call) starts
    with the scene classifier reset, except where `cont` continues the previous clip."""
    P = []

    def add(n, variant, dets, speed, lane_kinds, stream=0, cont=False):
        for i in range(n):
            f = len(P)
            P.append((stream, f, variant, dets(i) if callable(dets) else dets, speed(i) if callable(speed) else speed,
                      lane_kinds[i % len(lane_kinds)], int(i == 0 and not cont)))

    TL, SS, CAR, TRUCK, BUS, PED, CYC, PERSON = (NAMES.index(n) for n in
                                                 ("traffic_light", "stop_sign", "car", "truck", "bus", "pedestrian", "cyclist", "person"))
    add(5, sr.V_CENTER, [(TL, 0.91), (CAR, 0.8)], 10.0, [3, 4], stream=1)           # intersection (+ traffic element)
    add(2, sr.V_GREEN, [(CAR, 0.7)], 10.0, [0], stream=2, cont=True)                # residential raw, voted back to intersection
    add(2, sr.V_PLAIN, [(CAR, 0.7)], 10.0, [1], stream=2)                           # a tie in the vote (first frames differ)
    add(3, sr.V_GREEN, [], 10.0, [1], stream=2, cont=True)
    add(6, sr.V_LINES, [], 20.0, [5, 4, 3])                                         # highway (long lines + lanes), CLEAR
    add(6, sr.V_GREEN, lambda i: [(CAR, 0.6)] if i % 2 else [], 8.0, [1, 2], stream=3)      # residential
    add(6, sr.V_PLAIN, [(CAR, 0.9), (TRUCK, 0.85), (BUS, 0.8), (CAR, 0.7), (PED, 0.66), (SS, 0.55)], 1.0, [6, 5],
        stream=4)                                                                   # urban, CONGESTED, pedestrians, stop sign
    add(5, sr.V_DARK, [], np.nan, [0, 1], stream=5)                                 # NIGHT, no vehicle_state, urban default
    add(5, sr.V_FLAT, [(PERSON, 0.5), (CYC, 0.4)], 5.0, [4], stream=6)              # FOG, DAY 0.5
    add(5, sr.V_BRIGHT, lambda i: [(TL, 0.5 + 0.1 * i), (TL, 0.3)], 16.0, [3, 6], stream=7)    # DAY 0.8
    add(4, sr.V_PLAIN, None, 12.0, [2, 5], stream=8)                                # detections None
    add(4, sr.V_LINES, [(CAR, 0.9)] * 5, 30.0, [5], stream=9)                       # highway with > 3 vehicles
    return P


def main():
    mods = _load_reference()
    scm, atm = mods["scene_classifier"], mods["auto_tagger"]
    road = list(scm.RoadType)
    cond = list(scm.Condition)
    elem = list(scm.TrafficElement)
    assert [r.value for r in road] == sr.ROAD_TYPES and [c.value for c in cond] == sr.CONDITIONS
    assert [e.value for e in elem] == sr.ELEMENTS
    P = plan()
    n = len(P)
    out = dict(h=np.int32(H), w=np.int32(W), names=np.array(NAMES),
               stream=np.array([p[0] for p in P], np.int32), frame=np.array([p[1] for p in P], np.int32),
               variant=np.array([p[2] for p in P], np.int32), speed=np.array([p[4] for p in P], np.float64),
               lane_kind=np.array([p[5] for p in P], np.int32), reset=np.array([p[6] for p in P], np.int32), det_n=np.full(n, -1, np.int32),
               det_cls=np.zeros((n, KMAX), np.int32), det_conf=np.zeros((n, KMAX), np.float64),
               road_type=np.zeros(n, np.int32), confidence=np.zeros(n), lane_count=np.zeros(n, np.int32),
               has_ped=np.zeros(n, np.int32), timestamp=np.zeros(n), n_cond=np.zeros(n, np.int32),
               cond=np.full((n, 3), -1, np.int32), cond_conf=np.zeros((n, 3)), n_elem=np.zeros(n, np.int32),
               elem=np.full((n, KMAX), -1, np.int32), elem_conf=np.zeros((n, KMAX)),
               history=np.full((n, 5), -1, np.int32), frame_count=np.zeros(n, np.int32))
    sc = scm.SceneClassifier()
    at = atm.AutoTagger(video_path="fixture.mp4", fps=30.0)
    x = 0.0
    frames_tags = []
    for i, (stream, f, variant, dets, speed, lk, rs) in enumerate(P):
        img = sr.scene_frame(H, W, stream, f, variant)
        if rs:
            sc.reset()
            at.scene_classifier.reset()
        if dets is None:
            det_objs = None
        else:
            det_objs = [types.SimpleNamespace(class_name=NAMES[c], confidence=float(cf)) for c, cf in dets]
            out["det_n"][i] = len(dets)
            for k, (c, cf) in enumerate(dets):
                out["det_cls"][i, k], out["det_conf"][i, k] = c, cf
        vs = None
        if not np.isnan(speed):
            x += speed / 30.0
            vs = types.SimpleNamespace(speed=float(speed), heading=0.0, acceleration=0.0, yaw_rate=0.0, x=x, y=0.0)
        lanes = LANE_CASES[lk]
        t = sc.classify(img, det_objs, lanes, vs)
        out["road_type"][i] = road.index(t.road_type)
        out["confidence"][i] = t.road_type_confidence
        out["lane_count"][i] = t.lane_count
        out["has_ped"][i] = int(t.has_pedestrian_area)
        out["timestamp"][i] = t.timestamp
        out["n_cond"][i] = len(t.conditions)
        for k, (c, cf) in enumerate(t.conditions):
            out["cond"][i, k], out["cond_conf"][i, k] = cond.index(c), cf
        out["n_elem"][i] = len(t.traffic_elements)
        for k, (e, cf) in enumerate(t.traffic_elements):
            out["elem"][i, k], out["elem_conf"][i, k] = elem.index(e), cf
        for k, hh in enumerate(sc.history):
            out["history"][i, k] = road.index(hh.road_type)
        out["frame_count"][i] = sc.frame_count
        ft = at.tag_frame(img, det_objs, None, lanes, vs)
        frames_tags.append(dict(all_tags=ft.all_tags, tag_confidences=ft.tag_confidences, frame_idx=ft.frame_idx,
                                timestamp=ft.timestamp))
    at.finalize()
    stats = at.get_tag_statistics()
    stats.pop("session_info")
    stats["speed_stats"] = {k: float(v) for k, v in stats["speed_stats"].items()}
    searches = dict(
        by_tag={t: [ft.frame_idx for ft in at.search_by_tag(t)] for t in ("intersection", "highway", "fog", "night", "clear")},
        all_=[ft.frame_idx for ft in at.search_by_tags(["day", "residential"], match_all=True)],
        any_=[ft.frame_idx for ft in at.search_by_tags(["night", "congested"], match_all=False)],
        high_risk=[ft.frame_idx for ft in at.get_high_risk_frames()],
        segments={t: at.get_event_segments(t, d) for t, d in (("day", 5), ("highway", 3), ("night", 5), ("residential", 8))})
    auto = dict(frames=frames_tags, statistics=stats, searches=searches, csv=at.export_tags("csv"))
    out["auto_json"] = np.array(json.dumps(auto))
    out["elem_names"] = np.array(sr.ELEMENTS)
    np.savez_compressed(os.path.join(OUT, "scene.npz"), **out)
    raw = []
    ref = sr.SceneRef()
    for i, (stream, f, variant, dets, speed, lk, rs) in enumerate(P):
        img = sr.scene_frame(H, W, stream, f, variant)
        if rs:
            ref = sr.SceneRef()
        d = ref.classify(img, None if dets is None else [NAMES[c] for c, _ in dets], LANE_CASES[lk],
                         None if np.isnan(speed) else speed)
        raw.append(d["road_type_raw"])
        assert d["road_type"] == out["road_type"][i], (i, d["road_type"], out["road_type"][i])
    raw = np.array(raw)
    print("scene.npz: %d frames, %d B" % (n, os.path.getsize(os.path.join(OUT, "scene.npz"))))
    print("  raw road types %s, smoothed %s, overrides %d" % (np.bincount(raw, minlength=6), np.bincount(out["road_type"], minlength=6),
                                                          int((raw != out["road_type"]).sum())))
    print("  conditions %s; lane counts %s" % (np.bincount(out["cond"][out["cond"] >= 0], minlength=6),
                                               np.bincount(out["lane_count"], minlength=4)))
    print("  DAY-0.8 %d DAY-0.5 %d; traffic elements %d; pedestrian frames %d" % (
        int(((out["cond"][:, 0] == sr.DAY) & (out["cond_conf"][:, 0] == 0.8)).sum()),
        int(((out["cond"][:, 0] == sr.DAY) & (out["cond_conf"][:, 0] == 0.5)).sum()), int(out["n_elem"].sum()), int(out["has_ped"].sum())))


if __name__ == "__main__":
    main()
