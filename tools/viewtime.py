#!/usr/bin/env python3
"""Timing of the device-composed demo view.  Not part of the bench contract.

  default      CameraLoop(64, 720 x 1280, view="demo"): device time of enqueue_view per step, between two HIP events on the hot
               stream, median of runs that each time >= 0.2 s of work after a warm-up; per launch with --split.  Two detectors:
               random:0 (a handful of boxes per frame) and the spread-weights seed 14 (300 boxes per frame: the long list).
  --profile    the same steps with no events, for a run under `rocprofv3 --kernel-trace --stats -- python tools/viewtime.py --profile`
  --classes N  the only route to the same pictures without the device builder: the tables downloaded, turned into Detection /
               LaneLine / Track objects, and the six class calls per camera (wall clock, N cameras; the route is linear in cameras)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.harness import generate_ego_motion  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import CameraLoop  # noqa: E402

HBM = 6.3e12          # bytes / s the card reaches
H, W = 720, 1280


def make_loop(S, model, view):
    loop = CameraLoop(S, h=H, w=W, model=model, dcap=8, tracker_kw=dict(min_hits=1), view=view)
    z = np.stack([np.asarray(generate_ego_motion(8, seed=s % 8), np.float64) for s in range(S)])
    view_mode, loop.view_mode = loop.view_mode, None       # the steps that fill the tables are not what is timed
    for k in range(4):
        loop.load_measurements(z[:, k:k + 1])
        loop.step(sync=True)
    loop.view_mode = view_mode
    return loop


def timed(loop, fn, min_s=0.2, runs=5):
    """-> [ms per call] x runs: each run = as many calls as fill min_s of device time, between two events on the hot stream"""
    L, st = loop.hot.L, loop.hot._s
    a, b, ms = C.c_void_p(), C.c_void_p(), C.c_float()
    nat.check(L.av_event_create(C.byref(a)))
    nat.check(L.av_event_create(C.byref(b)))
    for _ in range(5):
        fn()
    loop.synchronize()
    n, out = 8, []
    while len(out) < runs:
        nat.check(L.av_event_record(a, st))
        for _ in range(n):
            fn()
        nat.check(L.av_event_record(b, st))
        loop.synchronize()
        nat.check(L.av_event_elapsed_ms(a, b, C.byref(ms)))
        if ms.value < min_s * 1e3:
            n = int(n * max(2.0, 1.2 * min_s * 1e3 / max(ms.value, 1e-3)))
            continue
        out.append(ms.value / n)
    return out, n


def device_view(S, model, name, split):
    loop = make_loop(S, model, "demo")
    ms, n = timed(loop, lambda: loop.enqueue_view(fps=30.0))
    nd = loop.cam.det_n.cpu().numpy()
    prims = loop._view_n.cpu().numpy()
    th, tw = loop.view.shape[1:3]
    bev = 600 * 600 * 3
    moved = S * (H * W * 3 + 5 * bev + th * tw * 3)     # frame in; panel: base copy in / out, painting in / out, compose in; view out
    floor = S * (H * W * 3 + bev + th * tw * 3)
    res = dict(detector=name, cameras=S, ms=ms, calls_per_run=n, det_per_frame=float(nd.mean()), prims_per_camera=float(prims.mean()),
               bytes_moved=moved, bytes_min=floor)
    print("enqueue_view S=%d %s: median %.3f ms (runs of %d calls: %s); %.0f detections and %.0f primitives per camera; moves %.0f MB "
          "(minimum %.0f MB = %.0f us at 6.3 TB/s)" % (S, name, statistics.median(ms), n, " ".join("%.3f" % x for x in ms), nd.mean(),
                                                       prims.mean(), moved / 1e6, floor / 1e6, floor / HBM * 1e6), flush=True)
    if split:
        hot, cam, L = loop.hot, loop.cam, loop.hot.L
        h, st, a = hot.ctx.handle, hot._s, loop._view_args
        P = nat.ptr
        parts = {
            "av_camview_build": lambda: nat.check(L.av_camview_build(h, st, C.byref(a), P(loop._view_prims), loop._view_cap, P(loop._view_n),
                                                                       P(loop._view_verts), loop._view_vcap)),
            "av_raster_draw_to (camera view)": lambda: nat.check(L.av_raster_draw_to(
                h, st, S, H, W, P(cam.frames), W, P(loop.view), tw, 0, P(loop._view_prims), loop._view_cap, P(loop._view_n),
                P(loop._view_verts), loop._view_vcap)),
            "enqueue_bev": hot.enqueue_bev,
            "av_view_compose": lambda: nat.check(L.av_view_compose(h, st, S, None, H, W, P(hot.bev), 600, 600, P(loop.view), b"Camera View",
                                                                   b"Bird's Eye View")),
        }
        res["split_ms"] = {}
        for k, fn in parts.items():
            pm, _ = timed(loop, fn, min_s=0.05, runs=3)
            res["split_ms"][k] = pm
            print("    %-34s %.3f ms" % (k, statistics.median(pm)), flush=True)
        tiles = S * ((H + 31) // 32) * ((W + 31) // 32)
        rm = statistics.median(res["split_ms"]["av_raster_draw_to (camera view)"])
        print("    rasteriser: %.1f ns per 32 x 32 tile over %d tiles; its pixels alone (%.0f MB in and out) need %.0f us at 6.3 TB/s" % (
            rm * 1e6 / tiles, tiles, S * H * W * 6 / 1e6, S * H * W * 6 / HBM * 1e6), flush=True)
    return res


def class_route(n_cams, model, name):
    """What the parent commit offers: download, rebuild the objects, six class calls per camera."""
    from multimodal_autonomous_driving_perception_and_planning_amd.perception.detector import Detection, ObjectDetector
    from multimodal_autonomous_driving_perception_and_planning_amd.perception.lane_detector import LaneDetector, LaneLine
    from multimodal_autonomous_driving_perception_and_planning_amd.tracking.multi_object_tracker import MultiObjectTracker
    from multimodal_autonomous_driving_perception_and_planning_amd.visualization.overlays import OverlayRenderer
    loop = make_loop(n_cams, model, None)
    loop.hot.enqueue_bev()
    loop.synchronize()
    det, lane, trk, ov = ObjectDetector(mode="simulated"), LaneDetector(), MultiObjectTracker(), OverlayRenderer()
    names, tnames = loop.cam.yolo.names, ObjectDetector.CLASSES

    def once():
        c, hot = loop.cam, loop.hot
        frames, bev = c.frames.cpu().numpy(), hot.bev.cpu().numpy()
        dn, db, dc, dk = c.det_n.cpu().numpy(), c.det_box.cpu().numpy(), c.det_conf.cpu().numpy(), c.det_cls.cpu().numpy()
        pts, info, vs = c.pts.cpu().numpy(), c.info.cpu().numpy(), hot.vstate.cpu().numpy()
        rows, n = hot.snapshots()
        hdr, _, hist = hot.tracker_tables()
        L = hot.tcfg.trajectory_length
        out = []
        for s in range(n_cams):
            bi = db[s, :dn[s]].astype(np.int64)
            dets = [Detection(bbox=tuple(bi[i].tolist()), class_id=int(dk[s, i]), class_name=names.get(int(dk[s, i]), "unknown"),
                              confidence=float(dc[s, i])) for i in range(int(dn[s]))]
            ll = [LaneLine(points=pts[s, k], side=sd, confidence=1.0) if info[s, k] else None for k, sd in ((0, "left"), (1, "right"))]
            tracks = []
            for row in rows[s, 0, :n[s, 0]]:
                if row["flags"] & 1:
                    hl, slot, cid = int(row["hist_len"]), int(row["slot"]), int(row["cls"])
                    tracks.append(SimpleNamespace(track_id=int(row["id"]), bbox=(int(row["x1"]), int(row["y1"]), int(row["x2"]), int(row["y2"])),
                                                  class_name=tnames.get(cid, str(cid)), velocity=None,
                                                  trajectory=[tuple(hist[s, slot, e % L, :2]) for e in range(max(0, hl - L), hl)]))
            v = vs[s, 0]
            st = SimpleNamespace(x=v[0], y=v[1], heading=v[4], speed=v[5], acceleration=v[6])
            pic = det.draw_detections(frames[s], dets)
            pic = lane.draw_lanes(pic, ll[0], ll[1])
            pic = trk.draw_tracks(pic, tracks)
            pic = ov.draw_info_panel(pic, st, fps=30.0, frame_num=int(hdr[s, 2]) - 1)
            pic = ov.draw_detection_summary(pic, dets)
            out.append(ov.create_side_by_side(pic, bev[s], CameraLoop.VIEW_LABELS))
        return out
    once()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        once()
        ts.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ts)
    print("class route, %s, %d cameras: median %.1f ms per step (runs %s) = %.1f ms per camera -> %.0f ms for 64 cameras" % (
        name, n_cams, med, " ".join("%.1f" % t for t in ts), med / n_cams, med / n_cams * 64), flush=True)
    return dict(detector=name, cameras=n_cams, ms=ts, ms_64_cameras=med / n_cams * 64)


def models(tmp):
    from tests._util import spread_params
    path = os.path.join(tmp, "spread14.npy")
    np.save(path, spread_params(14))
    return (("random:0", "random:0"), (path, "spread weights, seed 14"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--split", action="store_true", help="also time every launch of enqueue_view on its own")
    ap.add_argument("--profile", action="store_true", help="just run 20 steps' views of the long-list detector (for rocprofv3)")
    ap.add_argument("--classes", type=int, default=0, metavar="N", help="time the class route for N cameras instead")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/viewtime.py measures on the GPU; none is visible")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        ms = models(tmp)
        if a.profile:
            loop = make_loop(a.cameras, ms[1][0], "demo")
            for _ in range(20):
                loop.enqueue_view(fps=30.0)
            loop.synchronize()
            return
        if a.classes:
            res = [class_route(a.classes, m, name) for m, name in ms]
        else:
            res = [device_view(a.cameras, m, name, a.split) for m, name in ms]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
