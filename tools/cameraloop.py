#!/usr/bin/env python3
"""CameraLoop: what a step from pixels to ranked trajectories costs, and what its parts cost.

  perception    PerceptionLoop(S).step() alone
  hot           HotLoop(S, window=1, fused_step=False, obstacles="moving_tracks") step alone (simulated detector)
  camera        CameraLoop(S).step(): the two wired through av_dets_to_tracker and av_lane_paths
  bridge        av_dets_to_tracker and av_lane_paths on their own, on the camera loop's tensors
  classes       the same S cameras frame by frame through the five drop-in classes (ObjectDetector in YOLO mode, LaneDetector,
                MultiObjectTracker, VehicleStateEstimator, MotionPlanner): wall clock per step of S frames, downloads included

HIP events on the stream the work runs on (the camera step: from the camera half's stream to the hot half's), median of --reps
steps after --warm warm-up steps, the whole measurement --rounds times (the spread between rounds is the figure's own noise).
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.harness import generate_ego_motion, synthetic_frame  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import CameraLoop, HotLoop, PerceptionLoop  # noqa: E402


def timed(L, s0, s1, fn, reps, warm, sync):
    """Median us of fn() between an event on stream s0 ahead of it and one on s1 behind it; every step is waited for."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    nat.check(L.av_event_create(C.byref(e0)))
    nat.check(L.av_event_create(C.byref(e1)))
    ms, out = C.c_float(), []
    for k in range(warm + reps):
        nat.check(L.av_event_record(e0, s0))
        fn()
        nat.check(L.av_event_record(e1, s1))
        sync()
        nat.check(L.av_event_elapsed_ms(e0, e1, C.byref(ms)))
        if k >= warm:
            out.append(ms.value * 1e3)
    L.av_event_destroy(e0), L.av_event_destroy(e1)
    return round(float(np.median(out)), 1)


def figures(S, reps, warm, what):
    L, out = nat.lib(), {}
    z = np.stack([np.asarray(generate_ego_motion(1, seed=k)) for k in range(S)])
    if "perception" in what:
        cam = PerceptionLoop(n_streams=S)
        out["perception"] = timed(L, cam._s, cam._s, cam.step, reps, warm, cam.synchronize)
        del cam
    if "hot" in what:
        hot = HotLoop(n_streams=S, window=1, fused_step=False, obstacles="moving_tracks")
        hot.load_measurements(z)
        out["hot"] = timed(L, hot._s, hot._s, hot.step, reps, warm, hot.synchronize)
        del hot
    if "camera" in what or "bridge" in what:
        loop = CameraLoop(S)
        loop.load_measurements(z)
        if "camera" in what:
            out["camera"] = timed(L, loop.cam._s, loop.hot._s, loop.step, reps, warm, loop.synchronize)
        if "bridge" in what:
            loop.step(sync=True)
            hot = loop.hot
            out["av_dets_to_tracker"] = timed(L, hot._s, hot._s, hot.enqueue_detect, reps, warm, hot.synchronize)
            out["av_lane_paths"] = timed(L, hot._s, hot._s, hot.enqueue_lane_paths, reps, warm, hot.synchronize)
            r = loop.results()
            out["kept / dropped / lanes"] = (int(r["det_n"].sum()), int(r["det_dropped"].sum()), int((r["n_ref"] > 0).sum()))
        del loop
    if "classes" in what:
        import src.perception as P
        import src.planning as PL
        import src.state_estimation as SE
        import src.tracking as T
        frames = [synthetic_frame(720, 1280, s, 0) for s in range(S)]
        cams = [(P.ObjectDetector(mode="yolo"), P.LaneDetector(), T.MultiObjectTracker(), SE.VehicleStateEstimator(), PL.MotionPlanner())
                for _ in range(S)]
        t = []
        for k in range(max(2, warm // 5) + max(3, reps // 5)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s, (det, lane, trk, est, pl) in enumerate(cams):
                trk.update(det.detect(frames[s]))
                lane.detect(frames[s])
                st = est.step(z[s, 0])
                pl.plan((st.x, st.y, st.heading, st.speed))
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e6)
        out["classes (wall clock)"] = round(float(np.median(t[max(2, warm // 5):])), 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", default="perception,hot,camera,bridge,classes")
    a = ap.parse_args()
    for r in range(a.rounds):
        print("us per step of %d cameras:" % a.streams, figures(a.streams, a.reps, a.warm, a.what.split(",")), flush=True)
