#!/usr/bin/env python3
"""The rig's surround view: what stitching costs beside the per-camera bird's-eye warp.

  surround      av_rig_surround, feather: --vehicles rigs of 4 cameras, 720 x 1280 frames -> one 800 x 800 panel per vehicle
  nearest       the same with blend = nearest
  warp          av_ground_warp of the same --vehicles x 4 frames to one 800 x 800 panel per CAMERA: the existing kernel that reads
                the same kind of taps and writes four times the bytes
  overlay       av_rig_view_build + av_raster_draw over the stitched panels (64 obstacles, a 50-point path, the planner's 51 waypoints)

Device events on the stream the work runs on, --reps calls per window after --warm warm-up calls, the legs alternating inside one
process and the whole measurement --rounds times (the spread between rounds is the figure's own noise).
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
from multimodal_autonomous_driving_perception_and_planning_amd.perception import CameraRig  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.visualization import SurroundView  # noqa: E402

H, W, GH, GW, X_FAR, M_PER_PX = 720, 1280, 800, 800, 40.0, 0.1
# front, left, right, rear: the side cameras' views overlap the front one's
POSES = [dict(fx=531.0, fy=428.0, cx=628.0, cy=195.0, height=1.5, pitch=math.radians(12.0), max_range=45.0, x=1.5, y=0.0, yaw=0.0),
         dict(fx=435.0, fy=350.0, cx=640.0, cy=234.0, height=1.4, pitch=math.radians(20.0), max_range=30.0, x=0.5, y=-0.8,
              yaw=math.radians(-50.0)),
         dict(fx=435.0, fy=350.0, cx=640.0, cy=234.0, height=1.4, pitch=math.radians(20.0), max_range=30.0, x=0.5, y=0.8,
              yaw=math.radians(50.0)),
         dict(fx=483.0, fy=389.0, cx=628.0, cy=214.0, height=1.2, pitch=math.radians(15.0), max_range=35.0, x=-1.0, y=0.0, yaw=math.pi)]


def window(st, fn, reps, warm):
    """Median-free and simple: `reps` calls between two events on the stream, after `warm` calls; -> us per call."""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    b.synchronize()
    return round(a.elapsed_time(b) * 1000.0 / reps, 1)


def figures(V, reps, warm, what):
    L, ctx, dev = nat.lib(), nat.Context(0), torch.device("cuda", 0)
    rig, K = CameraRig.from_poses(POSES), 4
    st = torch.cuda.Stream(device=dev)
    s = C.c_void_p(st.cuda_stream)
    frames = torch.randint(0, 256, (V * K, H, W, 3), dtype=torch.uint8, device=dev)
    views = {b: SurroundView(rig, V, H, W, gh=GH, gw=GW, x_far=X_FAR, m_per_px=M_PER_PX, blend=b, ctx=ctx) for b in ("feather", "nearest")}
    sv = views["feather"]
    warp_out = torch.zeros(V * K, GH, GW, 3, dtype=torch.uint8, device=dev)
    fill = (C.c_uint8 * 3)(0, 0, 0)
    rng = np.random.default_rng(0)
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    ocap, rcap, n_cand, n_pts = 64, 50, 35, 51
    obs = np.concatenate([rng.uniform(-35, 35, (V, ocap, 2)), rng.uniform(0.5, 2.5, (V, ocap, 1)), rng.uniform(-8, 8, (V, ocap, 2))], axis=2)
    ref = np.stack([np.linspace(1, 38, rcap), np.zeros(rcap)], axis=1)[None].repeat(V, 0)
    wp = np.zeros((V, n_cand, n_pts, 6))
    wp[..., 0], wp[..., 1] = np.linspace(0, 30, n_pts), np.linspace(-3, 3, n_cand)[:, None] * np.linspace(0, 1, n_pts)
    lists = dict(plan_state=up(np.zeros((V, 4))), obstacles=up(obs), n_obs=up(np.full(V, ocap, np.int32)),
                 ids=up(rng.integers(1, 99, (V, ocap)).astype(np.int32)), ref_path=up(ref), n_ref=up(np.full(V, rcap, np.int32)),
                 waypoints=up(wp), order=up(np.tile(np.arange(n_cand, dtype=np.int32), (V, 1))))
    torch.cuda.synchronize()

    def warp():
        nat.check(L.av_ground_warp(ctx.handle, s, nat.ptr(sv.ground), V * K, H, W, nat.ptr(frames), GH, GW, X_FAR, M_PER_PX, fill,
                                   nat.ptr(warp_out)))

    legs = dict(surround=lambda: views["feather"].render(frames, stream=s), nearest=lambda: views["nearest"].render(frames, stream=s), warp=warp,
                overlay=lambda: sv.draw(stream=s, **lists))
    out = {}
    for i, name in enumerate(what):      # alternating: the legs in the order given, a leg named twice measured twice
        out["%d %s" % (i, name)] = window(st, legs[name], reps, warm)
    cover = views["feather"].cover
    out["seen by 0 / 1 / 2+ cameras (%)"] = tuple(round(float(x) * 100.0, 1) for x in (
        (cover == 0).float().mean(), ((cover & (cover - 1)) == 0).float().mean() - (cover == 0).float().mean(),
        ((cover & (cover - 1)) != 0).float().mean()))
    ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=16)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", default="surround,warp,nearest,warp,overlay")
    a = ap.parse_args()
    for r in range(a.rounds):
        print("us per call:", figures(a.vehicles, a.reps, a.warm, a.what.split(",")), flush=True)
