#!/usr/bin/env python3
"""Planner with per-state inputs: what the lookup costs, what motion costs (section 7e) and what the
per-track Kalman filter costs (section 7l).

  planner   av_planner_plan without extras | av_planner_plan_each with null lists | av_planner_plan with 16 shared obstacles |
            av_planner_plan_each with the same 16 per state | av_planner_plan_moving with the same 16 and a velocity each,
            at 64 and 16 384 start states, default planner
  step      HotLoop(64 streams, fused_step=False) plain, with obstacles="tracks" and with "moving_tracks", window 1 and 256
  filter    av_track_filter_update beside av_tracker_update on the same inputs (64 streams, tcap 64, window 1 and 256), and the
            "filtered_tracks" step beside the "moving_tracks" step; not part of the default --what
  ground    av_track_obstacles_ground (mode 1) beside av_track_obstacles_moving on the same full tables (64 and 16 384 states),
            av_ground_warp for 64 cameras 720 x 1280 -> 500 x 640 with the bytes it writes and touches, and CameraLoop(16)'s
            step with and without a calibration (section 7m); not part of the default --what
  lens      av_remap for 64 cameras 720 x 1280 -> 720 x 1280 through one shared table and through 64 tables, with its bytes;
            av_remap through av_lens_map_ground's table beside av_ground_warp on the 500 x 640 panel; av_track_obstacles_ground_lens
            (mode 1) beside av_track_obstacles_ground on the same full tables; the two table builders, first and second launch;
            CameraLoop(16)'s step with and without lenses (section 7n); not part of the default --what

HIP events on the stream the work runs on, median of --reps launches after warm-up, the whole measurement --rounds times
(the spread between rounds is the figure's own noise).  Runs on a tree without av_planner_plan_each or av_planner_plan_moving
too (those columns are left out): the same script gives the figures of an older commit.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.harness import generate_ego_motion  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop  # noqa: E402


def timed(L, stream, fn, reps, warm=10):
    """Median us of fn() (an enqueue on `stream`) between two events."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    nat.check(L.av_event_create(C.byref(e0)))
    nat.check(L.av_event_create(C.byref(e1)))
    ms, out = C.c_float(), []
    for k in range(warm + reps):
        nat.check(L.av_event_record(e0, stream))
        fn()
        nat.check(L.av_event_record(e1, stream))
        nat.check(L.av_event_elapsed_ms(e0, e1, C.byref(ms)))
        if k >= warm:
            out.append(ms.value * 1e3)
    L.av_event_destroy(e0), L.av_event_destroy(e1)
    return float(np.median(out))


def planner_figures(reps):
    L, ctx = nat.lib(), nat.Context(0)
    cfg = nat.PlannerCfg(5.0, 0.1, 7, 0, 1.0, 0.5, 0.3, 0.4)
    nat.check(L.av_planner_configure(ctx.handle, C.byref(cfg)))
    dev, st = torch.device("cuda", 0), torch.cuda.Stream()
    s = C.c_void_p(st.cuda_stream)
    rng = np.random.default_rng(1)
    has_each, has_moving = hasattr(L, "av_planner_plan_each"), hasattr(L, "av_planner_plan_moving")
    vrng = np.random.default_rng(2)          # (a generator of its own: the other inputs are those of a tree without the moving case)
    out = {}
    for S in (64, 16384):
        state = torch.as_tensor(np.stack([rng.uniform(-50, 50, S), rng.uniform(-50, 50, S), rng.uniform(-3, 3, S),
                                          rng.uniform(5, 15, S)], axis=1), device=dev)
        # 16 obstacles ahead of every state, in its own frame (so every list costs the same work)
        ahead = np.stack([rng.uniform(5, 40, 16), rng.uniform(-4, 4, 16), rng.uniform(0.5, 1.5, 16)], axis=1)
        sn = state.cpu().numpy()
        each = np.zeros((S, 16, 3))
        each[:, :, 0] = sn[:, None, 0] + ahead[None, :, 0] * np.cos(sn[:, None, 2]) - ahead[None, :, 1] * np.sin(sn[:, None, 2])
        each[:, :, 1] = sn[:, None, 1] + ahead[None, :, 0] * np.sin(sn[:, None, 2]) + ahead[None, :, 1] * np.cos(sn[:, None, 2])
        each[:, :, 2] = ahead[None, :, 2]
        obs_each, n_each = torch.as_tensor(each, device=dev), torch.full((S,), 16, dtype=torch.int32, device=dev)
        obs_shared = obs_each[0].contiguous()
        wp = torch.empty(S * 21 * 51 * 6, dtype=torch.float64, device=dev)
        cost = torch.empty(S, 21, dtype=torch.float64, device=dev)
        order = torch.empty(S, 21, dtype=torch.int32, device=dev)
        P = nat.ptr
        runs = {"plan": lambda: nat.check(L.av_planner_plan(ctx.handle, s, S, P(state), None, 0, None, 0, P(wp), P(cost), P(order))),
                "plan+16": lambda: nat.check(L.av_planner_plan(ctx.handle, s, S, P(state), None, 0, P(obs_shared), 16, P(wp), P(cost),
                                                               P(order)))}
        if has_each:
            runs["each(null)"] = lambda: nat.check(L.av_planner_plan_each(ctx.handle, s, S, P(state), None, None, 0, 1, None, None, 0,
                                                                          P(wp), P(cost), P(order)))
            runs["each+16"] = lambda: nat.check(L.av_planner_plan_each(ctx.handle, s, S, P(state), None, None, 0, 1, P(obs_each),
                                                                       P(n_each), 16, P(wp), P(cost), P(order)))
        if has_moving:
            # the same 16, each with the ego's speed along the state's heading and up to 2 m/s of its own
            rel = vrng.uniform(-2.0, 2.0, (16, 2))
            mov = np.zeros((S, 16, 5))
            mov[:, :, :3] = each
            mov[:, :, 3] = sn[:, None, 3] * np.cos(sn[:, None, 2]) + rel[None, :, 0]
            mov[:, :, 4] = sn[:, None, 3] * np.sin(sn[:, None, 2]) + rel[None, :, 1]
            obs_mov = torch.as_tensor(mov, device=dev)
            runs["moving+16"] = lambda: nat.check(L.av_planner_plan_moving(ctx.handle, s, S, P(state), None, None, 0, 1, P(obs_mov),
                                                                           P(n_each), 16, P(wp), P(cost), P(order)))
        for name, fn in runs.items():
            out["%s S=%d" % (name, S)] = round(timed(L, s, fn, reps), 2)
        torch.cuda.synchronize()
    ctx.close()
    return out


def step_figures(reps):
    L, out = nat.lib(), {}
    modes = [("plain", {})]
    if hasattr(L, "av_track_obstacles"):
        modes.append(("tracks", dict(obstacles="tracks")))
    if hasattr(L, "av_track_obstacles_moving"):
        modes.append(("moving_tracks", dict(obstacles="moving_tracks")))
    for W in (1, 256):
        z = np.stack([np.asarray(generate_ego_motion(W, seed=k)) for k in range(64)])
        for name, kw in modes:
            loop = HotLoop(n_streams=64, window=W, fused_step=False, **kw)
            loop.load_measurements(z)
            for graph in (False, True):
                us = timed(L, loop._s, lambda: loop.step(graph=graph), reps if W == 1 else max(5, reps // 4), warm=5)
                out["%s W=%d%s" % (name, W, " graph" if graph else "")] = round(us, 1)
            loop.synchronize()
            del loop
    return out


def filter_figures(reps):
    """Section 7l: the filter's launch beside the tracker's on the same detections and tables, and the two steps, eager."""
    L, out = nat.lib(), {}
    for W in (1, 256):
        z = np.stack([np.asarray(generate_ego_motion(W, seed=k)) for k in range(64)])
        loop = HotLoop(n_streams=64, window=W, fused_step=False, obstacles="filtered_tracks")
        loop.load_measurements(z)
        loop.step(sync=True)                                      # detections and tables of a window
        out["tracker W=%d" % W] = round(timed(L, loop._s, lambda: loop.enqueue_track(), reps), 2)
        out["filter W=%d" % W] = round(timed(L, loop._s, lambda: loop.enqueue_track_filter(), reps), 2)
        out["filter/tracker W=%d" % W] = round(out["filter W=%d" % W] / out["tracker W=%d" % W], 3)
        loop.synchronize()
        del loop
        for name in ("moving_tracks", "filtered_tracks"):
            loop = HotLoop(n_streams=64, window=W, fused_step=False, obstacles=name)
            loop.load_measurements(z)
            out["%s step W=%d" % (name, W)] = round(timed(L, loop._s, lambda: loop.step(), reps), 1)
            loop.synchronize()
            del loop
    return out


def ground_figures(reps):
    """Section 7m: av_track_obstacles_ground (mode 1) beside av_track_obstacles_moving on the same full tables at 64 and 16 384
    states, av_ground_warp for 64 cameras 720 x 1280 -> 500 x 640 with its bytes, and the CameraLoop step with and without a
    calibration.  On a tree without the ground entry points only the av_track_obstacles_moving figures come out."""
    L, ctx, out = nat.lib(), nat.Context(0), {}
    has_ground = hasattr(L, "av_track_obstacles_ground")
    dev, st = torch.device("cuda", 0), torch.cuda.Stream()
    s, P = C.c_void_p(st.cuda_stream), nat.ptr
    rng = np.random.default_rng(3)
    row_dtype = np.dtype(nat.TRACK_ROW_FIELDS)
    ocfg = nat.ObstacleCfg(x_center=640.0, x_scale=0.015, y_far=50.0, y_scale=50.0 / 720, radius=(C.c_double * 16)(*([1.5] * 6 + [0.0] * 10)))
    if has_ground:
        from multimodal_autonomous_driving_perception_and_planning_amd.perception import CameraCalibration
        cal = CameraCalibration.from_pose(1000.0, 1000.0, 640.0, 360.0, 1.5, np.deg2rad(4.0))
        table = torch.frombuffer(bytearray(bytes(cal.cfg()) * 64), dtype=torch.uint8).reshape(64, 160).to(dev)
    for S in (64, 16384):
        # full tables of confirmed cars whose feet stand on the road under either map: every lane of every wave works
        rows = np.zeros((S, 64), row_dtype)
        x1, y1 = rng.integers(0, 1100, (S, 64)), rng.integers(320, 560, (S, 64))
        rows["x1"], rows["y1"], rows["x2"], rows["y2"] = x1, y1, x1 + rng.integers(20, 180, (S, 64)), y1 + rng.integers(20, 140, (S, 64))
        rows["flags"], rows["hist_len"], rows["vx"], rows["vy"] = 1, 5, rng.integers(-9, 10, (S, 64)) / 2.0, rng.integers(-9, 10, (S, 64)) / 2.0
        snap = torch.as_tensor(rows.view(np.uint8).reshape(S, 64, 64), device=dev)
        snap_n = torch.full((S,), 64, dtype=torch.int32, device=dev)
        state = torch.as_tensor(np.stack([rng.uniform(-50, 50, S), rng.uniform(-50, 50, S), rng.uniform(-3, 3, S),
                                          rng.uniform(5, 15, S)], axis=1), device=dev)
        obs = torch.zeros(S, 64, 5, dtype=torch.float64, device=dev)
        n_obs, n_off = torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        runs = {"moving": lambda: nat.check(L.av_track_obstacles_moving(ctx.handle, s, C.byref(ocfg), 30.0, S, 64, P(snap), P(snap_n),
                                                                        P(state), 64, P(obs), P(n_obs)))}
        if has_ground:
            runs["ground"] = lambda: nat.check(L.av_track_obstacles_ground(ctx.handle, s, C.byref(ocfg), P(table), (S + 63) // 64, 1, 30.0,
                                                                           S, 64, P(snap), P(snap_n), None, P(state), 64, P(obs),
                                                                           P(n_obs), P(n_off)))
        for name, fn in runs.items():
            out["%s S=%d" % (name, S)] = round(timed(L, s, fn, reps), 2)
            st.synchronize()
            out["%s S=%d kept" % (name, S)] = int(n_obs.sum().item())
        if has_ground:
            out["ground/moving S=%d" % S] = round(out["ground S=%d" % S] / out["moving S=%d" % S], 3)
    if not has_ground:
        ctx.close()
        return out
    # the warp: 64 cameras, every frame its own noise (nothing is shared between cameras in the caches)
    n, h, w, gh, gw, f_far, m = 64, 720, 1280, 500, 640, 50.0, 0.1
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
    view = torch.zeros(n, gh, gw, 3, dtype=torch.uint8, device=dev)
    fill = (C.c_uint8 * 3)(0, 0, 0)
    torch.cuda.synchronize()
    us = timed(L, s, lambda: nat.check(L.av_ground_warp(ctx.handle, s, P(table), n, h, w, P(frames), gh, gw, f_far, m, fill, P(view))), reps)
    st.synchronize()
    # source bytes touched: the distinct source pixels among the four taps of every panel pixel that reads the frame
    q = np.array(cal.cfg().ginv)
    f = (f_far - (np.arange(gh) + 0.5) * m)[:, None]
    l = (((np.arange(gw) + 0.5) - gw / 2.0) * m)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        D = np.broadcast_to(q[6] * f + q[7] * l + q[8], (gh, gw))
        tu, tv = np.floor((q[0] * f + q[1] * l + q[2]) / D * 65536.0 + 0.5), np.floor((q[3] * f + q[4] * l + q[5]) / D * 65536.0 + 0.5)
        ok = (D > 0) & (tu >= 0) & (tu <= (w - 1) * 65536.0) & (tv >= 0) & (tv <= (h - 1) * 65536.0)
    x0, y0 = tu[ok].astype(np.int64) >> 16, tv[ok].astype(np.int64) >> 16
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    touched = len(np.unique(np.concatenate([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1])))
    written, read = n * gh * gw * 3, n * touched * 3
    out["warp us"] = round(us, 1)
    out["warp panel pixels reading the frame"] = round(float(ok.mean()), 3)
    out["warp MB written"], out["warp MB of source touched"] = round(written / 1e6, 1), round(read / 1e6, 1)
    out["warp GB/s (written + touched)"] = round((written + read) / us / 1e3, 1)
    ctx.close()
    # the camera loop's step, whole (camera half and hot half), host clock around a synchronised run of steps
    import time
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import CameraLoop
    for name, kw in (("linear", {}), ("calibrated", dict(calibration=cal))):
        loop = CameraLoop(16, **kw)
        z = np.stack([np.asarray(generate_ego_motion(1, seed=k)) for k in range(16)])
        loop.load_measurements(z)
        for _ in range(5):
            loop.step()
        loop.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            loop.step()
        loop.synchronize()
        out["camera step %s us" % name] = round((time.perf_counter() - t0) / reps * 1e6, 1)
        out["camera hot half %s us" % name] = round(timed(L, loop.hot._s, lambda: loop.hot.step(), reps), 1)
        loop.synchronize()
        del loop
    return out


def lens_figures(reps):
    """Section 7n (see the module text).  Every camera has the same lens; "64 tables" are 64 copies in memory of their own."""
    import time
    from multimodal_autonomous_driving_perception_and_planning_amd.perception import CameraCalibration
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import CameraLoop
    L, ctx, out = nat.lib(), nat.Context(0), {}
    dev, st = torch.device("cuda", 0), torch.cuda.Stream()
    s, P = C.c_void_p(st.cuda_stream), nat.ptr
    pose = dict(fx=1000.0, fy=1000.0, cx=640.0, cy=360.0, height=1.5, pitch=np.deg2rad(4.0))
    plain = CameraCalibration.from_pose(**pose)
    cal = CameraCalibration.from_pose(dist=(-0.30, 0.10, 1e-3, -5e-4, -0.02), size=(1280, 720), **pose)
    n, h, w, gh, gw, f_far, m = 64, 720, 1280, 500, 640, 50.0, 0.1
    ground = torch.frombuffer(bytearray(bytes(cal.cfg()) * n), dtype=torch.uint8).reshape(n, 160).to(dev)
    lens = torch.frombuffer(bytearray(bytes(cal.lens.cfg()) * n), dtype=torch.uint8).reshape(n, 112).to(dev)
    fill = (C.c_uint8 * 3)(0, 0, 0)

    def once(fn):
        """us of the first and of the second launch (a table is built once per lens)."""
        return [round(timed(L, s, fn, 1, warm=0), 1) for _ in range(2)]

    def taps(tu, tv, ok, sw, sh):
        x0, y0 = tu[ok].astype(np.int64) >> 16, tv[ok].astype(np.int64) >> 16
        x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
        return len(np.unique(np.concatenate([y0 * sw + x0, y0 * sw + x1, y1 * sw + x0, y1 * sw + x1])))

    # rectifying: 64 cameras, every frame its own noise
    frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
    rect = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=dev)
    maps = torch.empty(n, h, w, 2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    out["map_rectify 64 x 720 x 1280 us (first, second launch)"] = once(
        lambda: nat.check(L.av_lens_map_rectify(ctx.handle, s, P(lens), n, h, w, P(maps))))
    st.synchronize()
    host = maps[0].cpu().numpy()
    ok = host[..., 0] >= 0
    touched = taps(host[..., 0], host[..., 1], ok, w, h)
    for name, stride, n_maps in (("one shared table", n, 1), ("64 tables", 1, n)):
        us = timed(L, s, lambda: nat.check(L.av_remap(ctx.handle, s, P(maps), n, stride, h, w, P(frames), h, w, fill, P(rect))), reps)
        st.synchronize()
        moved = n * h * w * 3 + n_maps * h * w * 8 + n * touched * 3
        out["remap 720 x 1280, %s: us" % name] = round(us, 1)
        out["remap 720 x 1280, %s: MB (out + table + source touched)" % name] = [round(v / 1e6, 1) for v in (n * h * w * 3, n_maps * h * w * 8, n * touched * 3)]
        out["remap 720 x 1280, %s: GB/s" % name] = round(moved / us / 1e3, 1)
    del maps, rect
    # the bird's-eye panel: the table form from raw frames beside av_ground_warp from (what it takes as) rectified ones
    view = torch.zeros(n, gh, gw, 3, dtype=torch.uint8, device=dev)
    gmap = torch.empty(n, gh, gw, 2, dtype=torch.int32, device=dev)
    out["map_ground 64 x 500 x 640 us (first, second launch)"] = once(
        lambda: nat.check(L.av_lens_map_ground(ctx.handle, s, P(lens), P(ground), n, gh, gw, f_far, m, P(gmap))))
    out["ground_warp 500 x 640 us"] = round(timed(L, s, lambda: nat.check(L.av_ground_warp(ctx.handle, s, P(ground), n, h, w, P(frames), gh, gw,
                                                                                            f_far, m, fill, P(view))), reps), 1)
    out["remap 500 x 640 (64 tables) us"] = round(timed(L, s, lambda: nat.check(L.av_remap(ctx.handle, s, P(gmap), n, 1, h, w, P(frames), gh, gw,
                                                                                          fill, P(view))), reps), 1)
    st.synchronize()
    out["remap 500 x 640 panel pixels reading the frame"] = round(float((gmap[0, ..., 0] >= 0).float().mean().item()), 3)
    del frames, view, gmap
    # the obstacle kernel: full tables of confirmed cars, as ground_figures
    rng = np.random.default_rng(3)
    row_dtype = np.dtype(nat.TRACK_ROW_FIELDS)
    ocfg = nat.ObstacleCfg(radius=(C.c_double * 16)(*([1.5] * 6 + [0.0] * 10)))
    for S in (64, 16384):
        rows = np.zeros((S, 64), row_dtype)
        x1, y1 = rng.integers(0, 1100, (S, 64)), rng.integers(320, 560, (S, 64))
        rows["x1"], rows["y1"], rows["x2"], rows["y2"] = x1, y1, x1 + rng.integers(20, 180, (S, 64)), y1 + rng.integers(20, 140, (S, 64))
        rows["flags"], rows["hist_len"], rows["vx"], rows["vy"] = 1, 5, rng.integers(-9, 10, (S, 64)) / 2.0, rng.integers(-9, 10, (S, 64)) / 2.0
        snap = torch.as_tensor(rows.view(np.uint8).reshape(S, 64, 64), device=dev)
        snap_n = torch.full((S,), 64, dtype=torch.int32, device=dev)
        state = torch.as_tensor(np.stack([rng.uniform(-50, 50, S), rng.uniform(-50, 50, S), rng.uniform(-3, 3, S),
                                          rng.uniform(5, 15, S)], axis=1), device=dev)
        obs = torch.zeros(S, 64, 5, dtype=torch.float64, device=dev)
        n_obs, n_off = torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        tail = ((S + 63) // 64, 1, 30.0, S, 64, P(snap), P(snap_n), None, P(state), 64, P(obs), P(n_obs), P(n_off))
        runs = {"ground": lambda: nat.check(L.av_track_obstacles_ground(ctx.handle, s, C.byref(ocfg), P(ground), *tail)),
                "ground_lens": lambda: nat.check(L.av_track_obstacles_ground_lens(ctx.handle, s, C.byref(ocfg), P(ground), P(lens), *tail))}
        for name, fn in runs.items():
            out["%s S=%d" % (name, S)] = round(timed(L, s, fn, reps), 2)
            st.synchronize()
            out["%s S=%d kept" % (name, S)] = int(n_obs.sum().item())
        out["ground_lens/ground S=%d" % S] = round(out["ground_lens S=%d" % S] / out["ground S=%d" % S], 3)
    ctx.close()
    for name, c in (("calibrated", plain), ("with lenses", cal)):
        loop = CameraLoop(16, calibration=c)
        z = np.stack([np.asarray(generate_ego_motion(1, seed=k)) for k in range(16)])
        loop.load_measurements(z)
        for _ in range(5):
            loop.step()
        loop.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            loop.step()
        loop.synchronize()
        out["camera step %s us" % name] = round((time.perf_counter() - t0) / reps * 1e6, 1)
        out["camera hot half %s us" % name] = round(timed(L, loop.hot._s, lambda: loop.hot.step(), reps), 1)
        if loop.cam.lens is not None:
            out["camera rectify (16 frames, one table) us"] = round(timed(L, loop.cam._s, lambda: loop.cam.enqueue_rectify(), reps), 1)
        loop.synchronize()
        del loop
    return out


def warp_profile(launches=5):
    """ground_figures' warp launch a few times and nothing else, for a counter pass:
    rocprofv3 --kernel-trace --pmc <counters> -- python tools/peach.py --profile, then tools/rocpd_pmc.py on the database."""
    from multimodal_autonomous_driving_perception_and_planning_amd.perception import CameraCalibration
    L, ctx, dev = nat.lib(), nat.Context(0), torch.device("cuda", 0)
    cal = CameraCalibration.from_pose(1000.0, 1000.0, 640.0, 360.0, 1.5, np.deg2rad(4.0))
    table = torch.frombuffer(bytearray(bytes(cal.cfg()) * 64), dtype=torch.uint8).reshape(64, 160).to(dev)
    frames = torch.randint(0, 256, (64, 720, 1280, 3), dtype=torch.uint8, device=dev)
    view = torch.zeros(64, 500, 640, 3, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for _ in range(launches):
        nat.check(L.av_ground_warp(ctx.handle, None, nat.ptr(table), 64, 720, 1280, nat.ptr(frames), 500, 640, 50.0, 0.1,
                                   (C.c_uint8 * 3)(0, 0, 0), nat.ptr(view)))
    torch.cuda.synchronize()
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", default="planner,step")
    ap.add_argument("--profile", action="store_true", help="just launch section 7m's av_ground_warp five times (for rocprofv3)")
    a = ap.parse_args()
    if a.profile:
        warp_profile()
        sys.exit(0)
    for r in range(a.rounds):
        if "planner" in a.what:
            print("planner us:", planner_figures(a.reps), flush=True)
        if "step" in a.what:
            print("step us:", step_figures(a.reps), flush=True)
        if "filter" in a.what:
            print("filter us:", filter_figures(a.reps), flush=True)
        if "ground" in a.what:
            print("ground us:", ground_figures(a.reps), flush=True)
        if "lens" in a.what:
            print("lens us:", lens_figures(a.reps), flush=True)
