#!/usr/bin/env python3
"""Timing of the Motion-JPEG output.  Not part of the bench contract.

64 synthetic road frames of 1280 x 720 in HBM, quality 85, 4:2:0, one restart interval per MCU row:
  * the whole MJPEGWriter.write_device call (nine kernels, the download of the lengths and of the used bytes, the AVI chunks written),
    host clock around a synchronise, median of 9;
  * the nine kernels alone, between two HIP events, in runs of at least 0.2 s;
  * beside it the path that existed before, Y4MWriter.write_device on the same frames, to a file in the same directory;
  * the read of the written file by VideoDataLoader.read_frames_device (the decode side).
  --profile      20 encodes and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/mjpegenctime.py --profile`
  --stats CSV    no device needed: add the per-kernel times of such a run (its kernel_stats.csv) to the report --json names, with each
                 kernel's algorithmic bytes per second
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

HBM = 6.3e12          # bytes / s the card reaches (MI355X_MICROARCH: achievable HBM3E bandwidth)
H, W, N = 720, 1280, 64
BLOCKS_PER_PX = 6 / 256.0                      # 4:2:0: six blocks per 16 x 16 pixels
COEF = 128 * BLOCKS_PER_PX                     # bytes of int16 coefficients per pixel (3.0)
BITS = 4 * BLOCKS_PER_PX                       # bytes of bit counts / offsets per pixel


def kernel_bytes(px, stream_bytes, out_bytes):
    """Algorithmic HBM bytes of one call per kernel: px pixels, stream_bytes of unstuffed entropy data, out_bytes of frames"""
    return {"jpege_front_kernel": px * (3 + COEF), "jpege_size_kernel": px * (COEF + BITS), "jpege_scan_kernel": px * 2 * BITS,
            "jpege_zero_kernel": stream_bytes, "jpege_pack_kernel": px * (COEF + BITS) + stream_bytes, "jpege_count_kernel": stream_bytes,
            "jpege_gather_kernel": stream_bytes + out_bytes, "jpege_prefix_kernel": 0}


def event_ms(torch, fn, stream, min_ms=200.0, runs=5):
    for _ in range(3):
        fn()
    stream.synchronize()
    n, out = 4, []
    while len(out) < runs:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(n):
            fn()
        b.record(stream)
        stream.synchronize()
        ms = a.elapsed_time(b)
        if ms < min_ms:
            n = int(n * max(2.0, 1.2 * min_ms / max(ms, 1e-3)))
            continue
        out.append(ms / n)
    return out, n


def wall_ms(fn, sync, runs=9, before=None):
    for _ in range(2):
        fn()
    sync()
    out = []
    for _ in range(runs):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_stats(path):
    """rocprofv3's kernel_stats.csv -> {kernel name (without arguments): (calls, average ns)}"""
    out = {}
    names = list(kernel_bytes(0, 0, 0))
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for short in names:
                if short in name:
                    calls, total = int(row["Calls"]), float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
                    c0, t0 = out.get(short, (0, 0.0))
                    out[short] = (c0 + calls, t0 + total)
    return {k: (c, t / max(c, 1)) for k, (c, t) in out.items()}


def merge_stats(path_json, path_csv):
    with open(path_json) as f:
        res = json.load(f)
    px, ks = res["frames"] * res["height"] * res["width"], kernel_stats(path_csv)
    kb = kernel_bytes(px, res["compressed_bytes"], res["compressed_bytes"])       # the unstuffed stream is the frames less headers and stuffing
    res["kernel_ns"] = {}
    total = 0.0
    for k, (c, t) in sorted(ks.items(), key=lambda e: -e[1][1] * e[1][0]):
        per_call = t * (2 if k == "jpege_prefix_kernel" else 1)                    # two launches of it per call
        total += per_call
        e = dict(calls=c, average_ns=t, bytes=kb[k])
        if kb[k]:
            e["bytes_per_s"] = kb[k] / (t * 1e-9)
        res["kernel_ns"][k] = e
        print("    %-22s %6d calls, average %9.1f us, %6.1f MB -> %5.2f TB/s, %4.1f %% of %.1f TB/s" % (
            k, c, t / 1e3, kb[k] / 1e6, e.get("bytes_per_s", 0) / 1e12, 100 * e.get("bytes_per_s", 0) / HBM, HBM / 1e12))
    res["kernel_ns_sum_per_call"] = total
    with open(path_json, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a --profile run: merged into --json, no device needed")
    ap.add_argument("--commit", default="", help="the commit the measured tree is (or, with --dirty, is based on)")
    ap.add_argument("--dirty", action="store_true", help="the measured tree has changes that commit does not hold")
    ap.add_argument("--dir", default=None, help="where the video files are written (default: a temporary directory)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.stats:
        merge_stats(a.json, a.stats)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/mjpegenctime.py measures on the GPU; none is visible")
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    from multimodal_autonomous_driving_perception_and_planning_amd._dev import Dev
    from multimodal_autonomous_driving_perception_and_planning_amd.harness import synthetic_frame
    from multimodal_autonomous_driving_perception_and_planning_amd.loaders import MJPEGWriter, VideoDataLoader, Y4MWriter
    dev = Dev(0)
    L, stream = dev.lib, torch.cuda.current_stream()
    frames = dev.upload(np.stack([synthetic_frame(H, W, s, 3 * s) for s in range(N)]), np.uint8)
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        avi, y4m = os.path.join(tmp, "t.avi"), os.path.join(tmp, "t.y4m")
        wr = MJPEGWriter(avi, 30, (W, H))
        wr.write_device(frames)
        n, cap, _ = wr.last_call
        out = torch.empty((N, cap), dtype=torch.uint8, device=dev.device)
        info = torch.empty((2, N), dtype=torch.int32, device=dev.device)
        c = wr._const.data_ptr()

        def kernels():
            nat.check(L.av_jpeg_encode(dev.ctx.handle, nat.stream_handle(stream), N, H, W, nat.ptr(frames), c, wr._sub, wr.restart_mcus, c + 128,
                                       wr._header_len, nat.ptr(wr._ws), nat.ptr(out), cap, nat.ptr(info[0]), nat.ptr(info[1])))
        if a.profile:
            for _ in range(20):
                kernels()
            stream.synchronize()
            wr.release()
            return
        kernels()
        stream.synchronize()
        lens = info[0].cpu().numpy()
        assert not info[1].any().item()
        compressed = int(lens.sum())
        whole = wall_ms(lambda: wr.write_device(frames), stream.synchronize)
        dev_ms, calls = event_ms(torch, kernels, stream)
        wr.release()
        yw = Y4MWriter(y4m, 30, (W, H))
        at = yw._f.tell()
        ywhole = wall_ms(lambda: yw.write_device(frames), stream.synchronize, before=lambda: yw._f.seek(at))      # every run over the same 88 MB
        yw.release()
        # the decode side: the first 64 frames of the written file through the loader
        ld = VideoDataLoader(avi)
        read = wall_ms(lambda: ld.read_frames_device(0, N), stream.synchronize)
        assert not ld.last_status.any()
        ld.release()
    px = N * H * W
    res = dict(commit=a.commit, uncommitted_changes=bool(a.dirty), frames=N, height=H, width=W, quality=85, subsampling="4:2:0",
               restart_interval="one MCU row (80 MCUs), 45 per frame", hbm_bytes_per_s=HBM, compressed_bytes=compressed,
               bytes_per_pixel_to_host=compressed / px, workspace_bytes=int(wr._ws.numel()), slot_bytes=cap,
               write_device_ms=whole, kernels_ms=dev_ms, kernels_calls_per_run=calls,
               y4m=dict(bytes=px * 3 // 2, write_device_ms=ywhole), read_back_ms=read)
    print("MJPEGWriter.write_device, %d frames %dx%d: %.2f MB compressed (%.3f bytes per pixel); whole call median %.3f ms (host clock), "
          "nine kernels %.3f ms (events, runs of %d)" % (N, W, H, compressed / 1e6, compressed / px, statistics.median(whole),
                                                         statistics.median(dev_ms), calls), flush=True)
    print("Y4MWriter.write_device, the same frames: %.1f MB, whole call median %.3f ms (host clock)" % (px * 1.5 / 1e6, statistics.median(ywhole)),
          flush=True)
    print("VideoDataLoader.read_frames_device of the written file: median %.3f ms (host clock)" % statistics.median(read), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
