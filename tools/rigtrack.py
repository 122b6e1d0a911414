#!/usr/bin/env python3
"""Vehicle-frame tracks: what following the fused lists costs.

  track8        av_rig_track alone on av_rig_fuse's output for --vehicles rigs of 4 cameras with 8 obstacles per camera (about 32
                fused rows per vehicle), --tcap slots, in steady state (the same scene every frame: every row finds its track),
                beside av_rig_fuse on the same load in the same run
  track64       the same with 64 obstacles per camera (about 241 fused rows: more than --tcap 128 holds, so the rest is dropped
                every frame; --tcap 256 holds them all)
  loop          RigLoop(--rigs, a four-camera rig).step() without and with track=True, in one process

HIP events on the stream the work runs on, median of --reps steps after --warm warm-up steps, every step waited for, the whole
measurement --rounds times (the spread between rounds is the figure's own noise), as tools/rigloop.py measures.
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
from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import RigLoop  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.tracking import RigTracker  # noqa: E402

from cameraloop import timed  # noqa: E402
from rigloop import rig4  # noqa: E402


def track_leg(L, ctx, V, per_cam, tcap, reps, warm, ocap_in=64, ncol=5):
    """tools/rigloop.py's fuse load (V four-camera rigs, per_cam discs per camera in overlapping wedges), fused, and the fused
    lists tracked.  -> (av_rig_fuse us, av_rig_track us, fused rows per vehicle, live tracks per vehicle, rows matched per vehicle,
    rows dropped per vehicle)."""
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
    fused = torch.zeros(V, K * ocap_in, ncol, dtype=torch.float64, device=dev)
    n_obs, views = torch.zeros(V, dtype=torch.int32, device=dev), torch.zeros(V, K * ocap_in, dtype=torch.int32, device=dev)
    n_skip = torch.zeros(V, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    s = C.c_void_p(st.cuda_stream)
    cfg = nat.RigCfg(1.0, 1.0)
    trk = RigTracker(V, tcap=tcap, ncol=ncol, ctx=ctx)
    torch.cuda.synchronize()

    def fuse():
        nat.check(L.av_rig_fuse(ctx.handle, s, C.byref(cfg), V, K, nat.ptr(mounts), ncol, ocap_in, nat.ptr(t_obs), nat.ptr(t_n), nat.ptr(ps),
                                K * ocap_in, nat.ptr(fused), nat.ptr(n_obs), nat.ptr(views), nat.ptr(n_skip)))

    def track():
        trk.update(fused, n_obs, ps, views=views, stream=s)

    us_fuse = timed(L, s, s, fuse, reps, warm, st.synchronize)
    us_track = timed(L, s, s, track, reps, warm, st.synchronize)
    n, m = n_obs.cpu().numpy(), trk.match.cpu().numpy()
    rows = np.arange(m.shape[1])[None, :] < n[:, None]
    live = (trk.tracks()["id"] >= 0).sum(axis=1)
    # (the last frame is a steady-state one: the table has no free slot left or every row has its track, so no row is born, and
    # a row with an id is a matched row)
    return (us_fuse, us_track, round(float(n.mean()), 1), round(float(live.mean()), 1),
            round(float(((m > 0) & rows).sum(axis=1).mean()), 1), round(float(trk.n_drop.cpu().numpy().mean()), 1))


def figures(V, rigs, tcap, reps, warm, what):
    L, out = nat.lib(), {}
    if "track8" in what or "track64" in what:
        ctx = nat.Context(0)
        for per_cam in (8, 64):
            if "track%d" % per_cam in what:
                out["%d per camera, tcap %d (fuse us, track us, rows, live, matched, dropped)" % (per_cam, tcap)] = \
                    track_leg(L, ctx, V, per_cam, tcap, reps, warm)
        ctx.close()
    if "loop" in what:
        z = np.stack([np.asarray(generate_ego_motion(1, seed=k)) for k in range(rigs)])
        for track in (False, True):
            loop = RigLoop(rigs, rig4(), track=track)
            loop.load_measurements(z)
            out["rig (%d x 4)%s" % (rigs, ", track" if track else "")] = timed(L, loop.cams.cam._s, loop.ego._s, loop.step, reps, warm,
                                                                              loop.synchronize)
            if track:
                r = loop.results()
                out["rig, track: fused rows / tracks / confirmed"] = (int(r["fused_n_obs"].sum()), int((r["rig_tracks"]["id"] >= 0).sum()),
                                                                      int(r["n_obs"].sum()))
            del loop
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=64, help="rigs of the track legs")
    ap.add_argument("--rigs", type=int, default=16, help="rigs of the loop leg")
    ap.add_argument("--tcap", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", default="track8,track64,loop")
    a = ap.parse_args()
    for r in range(a.rounds):
        print("us per step:", figures(a.vehicles, a.rigs, a.tcap, a.reps, a.warm, a.what.split(",")), flush=True)
