#!/usr/bin/env python3
"""Rig tags: what the class lanes and the rig tagger cost.

  stages        for --vehicles rigs of 4 cameras with 8 obstacles per camera: av_rig_fuse and av_rig_fuse_cls, av_rig_track and
                av_rig_track_cls on the fused lists (--tcap slots, steady state), av_rig_interact on the tracker's state with --tcap
                and with 512 slots, and av_track_obstacles_ground beside av_track_obstacles_ground_cls on 4 x --vehicles tables of 64
                rows -- each pair in the same process, on the same inputs
  loop          RigLoop(--rigs, a four-camera rig, track=True).step() without and with tags="motion", in one process

HIP events on the stream the work runs on, median of --reps steps after --warm warm-up steps, every step waited for, the whole
measurement --rounds times (the spread between rounds is the figure's own noise), as tools/rigtrack.py measures.
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.harness import generate_ego_motion  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.perception import CameraCalibration  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import RigLoop  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.tagging import RigInteractionDetector  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.tracking import RigTracker  # noqa: E402

from cameraloop import timed  # noqa: E402
from rigloop import rig4  # noqa: E402


def stage_legs(L, ctx, V, tcap, reps, warm, per_cam=8, ocap_in=64, ncol=5):
    """tools/rigtrack.py's load with a class per row -> {figure: us}."""
    rig, K = rig4(), 4
    rng = np.random.default_rng(per_cam)
    d, a = rng.uniform(3.0, 45.0, (V * K, per_cam)), rng.uniform(-math.pi / 3, math.pi / 3, (V * K, per_cam))
    obs = np.zeros((V * K, ocap_in, ncol))
    obs[:, :per_cam, 0], obs[:, :per_cam, 1] = d * np.cos(a), d * np.sin(a)
    obs[:, :per_cam, 2] = rng.choice([0.5, 0.75, 1.0, 1.5, 2.0, 2.5], (V * K, per_cam))
    obs[:, :per_cam, 3:] = rng.uniform(-8.0, 8.0, (V * K, per_cam, 2))
    dev = torch.device("cuda", 0)
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    t_obs, t_n = up(obs), up(np.full(V * K, per_cam, np.int32))
    t_cls = up(rng.integers(0, 6, (V * K, ocap_in)).astype(np.int32))
    ps = up(np.stack([np.asarray(generate_ego_motion(1, seed=k))[0] for k in range(V)]))
    mounts = rig.mounts_table(V, dev)
    i32 = torch.int32
    fused = torch.zeros(V, K * ocap_in, ncol, dtype=torch.float64, device=dev)
    n_obs, n_skip = torch.zeros(V, dtype=i32, device=dev), torch.zeros(V, dtype=i32, device=dev)
    views, fcls = torch.zeros(V, K * ocap_in, dtype=i32, device=dev), torch.zeros(V, K * ocap_in, dtype=i32, device=dev)
    st = torch.cuda.Stream(device=dev)
    s = C.c_void_p(st.cuda_stream)
    cfg = nat.RigCfg(1.0, 1.0)
    trk, trk_cls = (RigTracker(V, tcap=tcap, ncol=ncol, ctx=ctx) for _ in range(2))
    big = RigTracker(V, tcap=512, ncol=ncol, ctx=ctx)
    names = {0: "car", 1: "truck", 2: "pedestrian", 3: "cyclist", 4: "motorcycle", 5: "bus"}
    tag, tag_big = RigInteractionDetector(V, tcap, class_names=names, ctx=ctx), RigInteractionDetector(V, 512, class_names=names, ctx=ctx)
    torch.cuda.synchronize()
    head = (ctx.handle, s, C.byref(cfg), V, K, nat.ptr(mounts), ncol, ocap_in, nat.ptr(t_obs), nat.ptr(t_n))
    tail = (nat.ptr(ps), K * ocap_in, nat.ptr(fused), nat.ptr(n_obs), nat.ptr(views), nat.ptr(n_skip))
    out = {}
    run = lambda f: timed(L, s, s, f, reps, warm, st.synchronize)         # noqa: E731
    out["av_rig_fuse"] = run(lambda: nat.check(L.av_rig_fuse(*head, *tail)))
    out["av_rig_fuse_cls"] = run(lambda: nat.check(L.av_rig_fuse_cls(*head, nat.ptr(t_cls), *tail, nat.ptr(fcls))))
    out["av_rig_track"] = run(lambda: trk.update(fused, n_obs, ps, views=views, stream=s))
    out["av_rig_track_cls"] = run(lambda: trk_cls.update(fused, n_obs, ps, views=views, stream=s, cls=fcls))
    for _ in range(5):
        big.update(fused, n_obs, ps, views=views, stream=s, cls=fcls)
    out["av_rig_interact, tcap %d" % tcap] = run(lambda: tag.detect(trk_cls, ps, stream=s))
    out["av_rig_interact, tcap 512"] = run(lambda: tag_big.detect(big, ps, stream=s))
    sm = tag.summary.cpu().numpy().reshape(V, -1).view(np.dtype(nat.INTERACTION_SUMMARY_FIELDS)).reshape(V)
    out["agents / interactions per vehicle"] = (round(float(sm["agent_count"].mean()), 1), round(float(sm["n_interactions"].mean()), 1))
    # the cameras' lists: V * K tables of 64 tracker rows, boxes over the lower half of a 1280 x 720 frame
    S, T = V * K, 64
    rows = np.zeros((S, T), np.dtype(nat.TRACK_ROW_FIELDS))
    x1, y1 = rng.integers(0, 1100, (S, T)), rng.integers(380, 600, (S, T))
    rows["x1"], rows["y1"], rows["x2"], rows["y2"] = x1, y1, x1 + rng.integers(10, 150, (S, T)), y1 + rng.integers(10, 100, (S, T))
    rows["cls"], rows["flags"], rows["hist_len"] = rng.integers(0, 6, (S, T)), 1, 3
    rows["vx"], rows["vy"] = rng.integers(-10, 11, (S, T)) / 2.0, rng.integers(-10, 11, (S, T)) / 2.0
    cal = CameraCalibration.from_pose(1000.0, 1000.0, 640.0, 360.0, 1.5, 0.05, max_range=60.0)
    table = up(np.frombuffer(bytes(cal.cfg()) * S, np.uint8).reshape(S, 160).copy())
    d_rows, d_n = up(rows.view(np.uint8).reshape(S, T, 64)), up(np.full(S, T, np.int32))
    zero = torch.zeros(S, 4, dtype=torch.float64, device=dev)
    lists, l_n, l_off = torch.zeros(S, T, 5, dtype=torch.float64, device=dev), torch.zeros(S, dtype=i32, device=dev), torch.zeros(S, dtype=i32, device=dev)
    l_cls = torch.zeros(S, T, dtype=i32, device=dev)
    ocfg = nat.ObstacleCfg(radius=(C.c_double * 16)(1.5, 2.0, 0.5, 0.75, 1.0, 2.5))
    g_tail = (1, 1, 30.0, S, T, nat.ptr(d_rows), nat.ptr(d_n), None, nat.ptr(zero), T, nat.ptr(lists), nat.ptr(l_n), nat.ptr(l_off))
    g_head = (ctx.handle, s, C.byref(ocfg), nat.ptr(table))
    out["av_track_obstacles_ground"] = run(lambda: nat.check(L.av_track_obstacles_ground(*g_head, *g_tail)))
    out["av_track_obstacles_ground_cls"] = run(lambda: nat.check(L.av_track_obstacles_ground_cls(*g_head, None, *g_tail, nat.ptr(l_cls))))
    out["obstacles per table"] = round(float(l_n.cpu().numpy().mean()), 1)
    return out


def figures(V, rigs, tcap, reps, warm, what):
    L, out = nat.lib(), {}
    if "stages" in what:
        ctx = nat.Context(0)
        out.update(stage_legs(L, ctx, V, tcap, reps, warm))
        ctx.close()
    if "loop" in what:
        z = np.stack([np.asarray(generate_ego_motion(1, seed=k)) for k in range(rigs)])
        for tags in (None, "motion"):
            loop = RigLoop(rigs, rig4(), track=True, tags=tags)
            loop.load_measurements(z)
            out["rig (%d x 4), track%s" % (rigs, ", tags" if tags else "")] = timed(L, loop.cams.cam._s, loop.ego._s, loop.step, reps, warm,
                                                                                   loop.synchronize)
            if tags:
                out["rig, tags: frames logged per vehicle"] = int(loop.tag_log.lengths().min())
            del loop
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=64, help="rigs of the stage legs")
    ap.add_argument("--rigs", type=int, default=16, help="rigs of the loop leg")
    ap.add_argument("--tcap", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", default="stages,loop")
    a = ap.parse_args()
    for r in range(a.rounds):
        print("us per step:", figures(a.vehicles, a.rigs, a.tcap, a.reps, a.warm, a.what.split(",")), flush=True)
