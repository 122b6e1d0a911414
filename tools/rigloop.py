#!/usr/bin/env python3
"""RigLoop: what fusing a rig's obstacle lists costs, and what a rig step costs beside the camera loop's.

  fuse8         av_rig_fuse alone: --vehicles rigs of 4 cameras, ocap_in 64, 8 obstacles per camera (the typical load)
  fuse64        the same with 64 obstacles per camera (full lists)
  rig           RigLoop(--vehicles / 4, a four-camera rig).step(): the same number of cameras as the next line
  camera        CameraLoop(--vehicles).step()

HIP events on the stream the work runs on (the loops' steps: from the camera half's stream to the planning half's), median of
--reps steps after --warm warm-up steps, every step waited for, the whole measurement --rounds times (the spread between rounds is
the figure's own noise).
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
from multimodal_autonomous_driving_perception_and_planning_amd.perception import CameraRig  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import CameraLoop, RigLoop  # noqa: E402

from cameraloop import timed  # noqa: E402

POSE = dict(fx=1000.0, fy=1000.0, cx=640.0, cy=360.0, height=1.5, pitch=math.radians(4.0))
MOUNTS = [dict(yaw=0.0, x=1.8, y=0.0), dict(yaw=math.pi / 2, x=0.5, y=0.9), dict(yaw=-math.pi / 2, x=0.5, y=-0.9),
          dict(yaw=math.pi, x=-1.0, y=0.0)]


def rig4():
    return CameraRig.from_poses([dict(POSE, **m) for m in MOUNTS])


def fuse_leg(L, ctx, V, per_cam, reps, warm, ocap_in=64, ncol=5):
    """av_rig_fuse on V four-camera rigs whose cameras each see per_cam discs in a 120-degree wedge, 3 .. 45 m out: neighbouring
    wedges overlap, so some discs are seen twice.  -> (median us, fused obstacles per vehicle, of them merged)."""
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
    ps = up(np.stack([np.asarray(generate_ego_motion(1, seed=k))[0] for k in range(V)]))
    mounts = rig.mounts_table(V, dev)
    out = torch.zeros(V, K * ocap_in, ncol, dtype=torch.float64, device=dev)
    n_obs, views = torch.zeros(V, dtype=torch.int32, device=dev), torch.zeros(V, K * ocap_in, dtype=torch.int32, device=dev)
    n_skip = torch.zeros(V, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    s = C.c_void_p(st.cuda_stream)
    cfg = nat.RigCfg(1.0, 1.0)
    torch.cuda.synchronize()

    def fn():
        nat.check(L.av_rig_fuse(ctx.handle, s, C.byref(cfg), V, K, nat.ptr(mounts), ncol, ocap_in, nat.ptr(t_obs), nat.ptr(t_n), nat.ptr(ps),
                                K * ocap_in, nat.ptr(out), nat.ptr(n_obs), nat.ptr(views), nat.ptr(n_skip)))

    us = timed(L, s, s, fn, reps, warm, st.synchronize)
    n = n_obs.cpu().numpy()
    return us, round(float(n.mean()), 1), round(float(K * per_cam - n.mean()), 1)


def figures(V, reps, warm, what):
    L, out = nat.lib(), {}
    if "fuse8" in what or "fuse64" in what:
        ctx = nat.Context(0)
        for per_cam in (8, 64):
            if "fuse%d" % per_cam in what:
                out["av_rig_fuse, %d per camera (us, fused, merged)" % per_cam] = fuse_leg(L, ctx, V, per_cam, reps, warm)
        ctx.close()
    if "rig" in what:
        n = max(1, V // 4)
        z = np.stack([np.asarray(generate_ego_motion(1, seed=k)) for k in range(n)])
        loop = RigLoop(n, rig4())
        loop.load_measurements(z)
        out["rig (%d x 4)" % n] = timed(L, loop.cams.cam._s, loop.ego._s, loop.step, reps, warm, loop.synchronize)
        r = loop.results()
        out["rig: camera rows / fused / seen twice"] = (int(r["cam_n_obs"].sum()), int(r["n_obs"].sum()),
                                                        int(sum(bin(int(m)).count("1") > 1 for v in range(n)
                                                                for m in r["views"][v, :r["n_obs"][v, 0]])))
        del loop
    if "camera" in what:
        z = np.stack([np.asarray(generate_ego_motion(1, seed=k)) for k in range(V)])
        loop = CameraLoop(V)
        loop.load_measurements(z)
        out["camera (%d)" % V] = timed(L, loop.cam._s, loop.hot._s, loop.step, reps, warm, loop.synchronize)
        del loop
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=64, help="rigs of the fuse legs; cameras of the loop legs")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", default="fuse8,fuse64,rig,camera")
    a = ap.parse_args()
    for r in range(a.rounds):
        print("us per step:", figures(a.vehicles, a.reps, a.warm, a.what.split(",")), flush=True)
