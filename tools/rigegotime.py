#!/usr/bin/env python3
"""Timing of the rig odometry.  Not part of the bench contract.

16 vehicles x 4 cameras of 720 x 1280 (front, left, rear, right), the default patch (256 x 256 px of 0.1 m, tiles of 16 px, search
12 px): device time of av_rig_egoflow_solve and of the whole av_rig_egoflow_update between two HIP events, beside av_egoflow_solve
and av_egoflow_update over the same 64 cameras.  tools/egotime.py's protocol: every figure is the median of runs that each time
>= 0.2 s of work after a warm-up; the runs are printed, and the candidates are timed in turns (--rounds) so that the session's
drift shows as their spread.  The frames are renderings of tests/egoflow_cases.py's road from the poses the mounts imply, two
consecutive ones per camera, so the tiles have something to match."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.perception import (CameraCalibration, CameraRig, GroundOdometry,  # noqa: E402
                                                                                  RigOdometry)
from tests import egoflow_cases as cases  # noqa: E402
from tests import rigflow_cases as rig_cases  # noqa: E402
from tools.egotime import timed  # noqa: E402

H, W = 720, 1280
MOUNTS = [(2.0, 0.0, 0.0), (0.5, 0.9, np.pi / 2), (-1.0, 0.0, np.pi), (0.5, -0.9, -np.pi / 2)]       # (x, y, yaw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    V, K = a.vehicles, len(MOUNTS)
    cal = CameraCalibration.from_pose(1000.0, 1000.0, 640.0, 360.0, 1.5, np.deg2rad(4.0))
    rig = CameraRig([cal] * K, MOUNTS)
    mounts = rig.mounts_table(1)[0].numpy()
    pair, pose = [], (3.0, -2.0, 0.1)
    for i in range(2):                                          # one vehicle rendered; the others repeat it
        fr = np.stack([cases.render_frame(cal, H, W, rig_cases.camera_pose(pose, mounts[k])) for k in range(K)])
        pair.append(torch.as_tensor(np.tile(fr, (V, 1, 1, 1))).cuda())
        pose = cases.compose(pose, (0.5, 0.0, 0.01))
    odo, cams = RigOdometry(rig, V, H, W), GroundOdometry(cal, V * K, H, W)
    for i in range(2):
        r, rc = odo.update(pair[i]), cams.update(pair[i])
    print("%d vehicles x %d cameras, %d tiles each: accepted %.0f, inliers %.0f per vehicle, views %s, hypothesis %s; motion of vehicle 0: "
          "%s (a camera alone: %s)" % (V, K, odo.n_tiles, r["n_tiles"].mean(), r["n_inliers"].mean(), bin(int(r["views"][0])),
                                      int(r["hypothesis"][0]), r["motion"][0], rc["motion"][0]))
    L, ctx, st, cfg = odo.L, odo.ctx.handle, nat.stream_handle(), C.byref(odo.cfg)
    flip = [0, 0]

    def rig_update():
        flip[0] ^= 1
        odo.enqueue(pair[flip[0]], st)

    def cam_update():
        flip[1] ^= 1
        cams.enqueue(pair[flip[1]], st)
    cands = {
        "av_rig_egoflow_solve": lambda: nat.check(L.av_rig_egoflow_solve(ctx, st, cfg, V, K, nat.ptr(odo.mounts), nat.ptr(odo.tile_rows),
                                                                         nat.ptr(odo.motion), nat.ptr(odo.info))),
        "av_egoflow_solve": lambda: nat.check(L.av_egoflow_solve(ctx, st, cfg, V * K, nat.ptr(cams.tile_rows), nat.ptr(cams.motion))),
        "av_rig_egoflow_update": rig_update,
        "av_egoflow_update": cam_update,
    }
    runs = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():
            runs[k] += timed(L, st, fn)
    for k, v in runs.items():
        print("%-24s median %8.1f us   min %8.1f  max %8.1f   (%d runs: %s)" % (k, statistics.median(v), min(v), max(v), len(v),
                                                                              " ".join("%.1f" % x for x in v)), flush=True)
    if a.json:
        json.dump(dict(vehicles=V, cams=K, h=H, w=W, gh=odo.cfg.gh, gw=odo.cfg.gw, tile=odo.cfg.tile, search=odo.cfg.search, us=runs),
                  open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
