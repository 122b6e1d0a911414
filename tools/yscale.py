#!/usr/bin/env python3
"""YOLO detector timing per model: the 64-frame forward at 720 x 1280 and the single-frame call, half precision and float32, with the
plan's kernel family per layer.

Device time between events over windows of >= 0.2 s after a warm-up (median of --windows windows, their spread beside it); the
single-frame call is a host clock around ObjectDetector-style detect(), which ends in a wait for the device.  One JSON line per
(model, precision) on stdout, and in --out if given.  FLOPs: pipeline._yolo_flops of the model at the letterboxed size; the bar of
DESIGN section 6 is  time(model) <= time(n) * flops(model) / flops(n)  within one run of this tool.

--root DIR imports the package from another checkout (an older commit, for an A/B of the default model: `--models n`)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="n,s,m", help="comma list of scale[:nc]")
ap.add_argument("--precisions", default="fp16,fp32")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.2)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--layers", action="store_true", help="add the plan's launches (family, variant, ops covered) to each line")
a = ap.parse_args()
sys.path.insert(0, a.root)
import numpy as np
import torch
from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
from multimodal_autonomous_driving_perception_and_planning_amd import pipeline as P
from multimodal_autonomous_driving_perception_and_planning_amd.perception import yolo as Y
from multimodal_autonomous_driving_perception_and_planning_amd.harness import synthetic_frame

if not torch.cuda.is_available():
    sys.exit("yscale.py measures on the GPU; no device is visible")
FAMILIES = ("mfma", "gemm128", "lds", "ws3", "ws1", "gemm_f32", "f32_no_lds", "fixed")
L = nat.lib()
H, W = 720, 1280
frames = np.stack([synthetic_frame(H, W, s % 4, s // 4) for s in range(a.batch)])


def make(scale, nc, batch, precision):
    if hasattr(Y, "YoloV8"):
        return Y.YoloV8("random:0:%s:%d" % (scale, nc), batch=batch, precision=precision)
    assert (scale, nc) == ("n", 80), "this checkout builds the default model only"
    return Y.YoloV8n("random:0", batch=batch, precision=precision)


def flops(scale, nc):
    try:
        return P._yolo_flops(384, 640, scale, nc)
    except TypeError:
        return P._yolo_flops(384, 640)


def forward_ms(m, fr):
    """Median and spread of the per-forward device time over windows of >= min-seconds each."""
    st = m._dev.stream
    ea, eb = C.c_void_p(), C.c_void_p()
    L.av_event_create(C.byref(ea)), L.av_event_create(C.byref(eb))
    ms = C.c_float()
    for _ in range(3):
        m.forward_device(fr)
    torch.cuda.synchronize()
    L.av_event_record(ea, st), m.forward_device(fr), L.av_event_record(eb, st)
    torch.cuda.synchronize()
    L.av_event_elapsed_ms(ea, eb, C.byref(ms))
    reps = max(3, int(a.min_seconds * 1e3 / max(ms.value, 1e-3)) + 1)
    out = []
    for _ in range(a.windows):
        L.av_event_record(ea, st)
        for _ in range(reps):
            m.forward_device(fr)
        L.av_event_record(eb, st)
        torch.cuda.synchronize()
        L.av_event_elapsed_ms(ea, eb, C.byref(ms))
        out.append(ms.value / reps)
    return float(np.median(out)), float(min(out)), float(max(out)), reps


def single_ms(scale, nc, precision):
    m = make(scale, nc, 1, precision)
    for _ in range(5):
        m.detect(frames[0])
    t, n = [], 0
    t_end = time.perf_counter() + a.min_seconds * a.windows
    while time.perf_counter() < t_end or n < 20:
        t0 = time.perf_counter()
        m.detect(frames[n % len(frames)])
        t.append((time.perf_counter() - t0) * 1e3)
        n += 1
    m.close()
    return float(np.median(t)), n


lines = []
for spec in a.models.split(","):
    scale, nc = (spec.split(":") + ["80"])[:2]
    nc = int(nc)
    for precision in a.precisions.split(","):
        m = make(scale, nc, a.batch, precision)
        m._prepare(H, W)
        fr = torch.as_tensor(frames).to(m._dev.device)
        med, lo, hi, reps = forward_ms(m, fr)
        rec = dict(model="%s:%d" % (scale, nc), precision=precision, batch=a.batch, forward_ms=round(med, 4), forward_ms_min=round(lo, 4),
                   forward_ms_max=round(hi, 4), forwards_per_window=reps, gflop_per_frame=round(flops(scale, nc) / 1e9, 3))
        rec["tflops"] = round(rec["gflop_per_frame"] * a.batch / med, 2)
        if hasattr(m, "plan"):
            fam = {}
            for s in m.plan():
                if s.when != nat.YOLO_WHEN_BGR_UNALIGNED:
                    fam[FAMILIES[s.family]] = fam.get(FAMILIES[s.family], 0) + 1
            rec["launches_per_family"] = fam
            if a.layers:
                rec["plan"] = [dict(family=FAMILIES[s.family], variant=list(s.variant), first_op=s.first_op, n_ops=s.n_ops, grid=list(s.grid),
                                    block=s.block[0], lds=s.lds_bytes, lane=s.lane) for s in m.plan() if s.when != nat.YOLO_WHEN_BGR_UNALIGNED]
        m.close()
        del fr
        rec["single_frame_ms"], rec["single_frame_calls"] = single_ms(scale, nc, precision)
        rec["single_frame_ms"] = round(rec["single_frame_ms"], 4)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
