#!/usr/bin/env python3
"""Timing of the Motion-JPEG ingest.  Not part of the bench contract.

64 frames of 1280 x 720, 4:2:0, Pillow quality 85 (the project's synthetic road scenes), once with one restart interval per MCU row and
once with none, decoded in one av_jpeg_decode call:
  * the whole read (copy into the pinned buffer, av_jpeg_parse, one upload, the four kernels), host clock around a synchronise;
  * the four kernels alone, between two HIP events, replayed on the buffers already uploaded;
  * beside it the path that exists without a decoder, for I420 planes of the same size (random bytes): upload + av_i420_to_bgr.
  --encode PATH  only encode the frames (needs Pillow) and keep them in PATH (.npz); --frames PATH reads them back where Pillow is missing
  --profile      20 decodes of each variant and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/mjpegtime.py --profile`
  --stats CSV    add the per-kernel times of such a run (its kernel_stats.csv) to the report, with the pixel kernels' bytes per second
"""
import argparse
import csv
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

HBM = 6.3e12          # bytes / s the card reaches (MI355X_MICROARCH: achievable HBM3E bandwidth)
H, W, N = 720, 1280, 64
VARIANTS = (("restart interval per MCU row", dict(restart_marker_rows=1)), ("no restart markers", {}))
# HBM bytes per pixel each kernel has to move for 4:2:0: coefficients are 1.5 int16 per pixel, samples 1.5 bytes, the output 3
KERNEL_BYTES_PER_PX = {"jpeg_clear_kernel": 3.0, "jpeg_idct_kernel": 3.0 + 1.5, "jpeg_convert_kernel": 1.5 + 3.0}


def encode_frames():
    from PIL import Image
    from multimodal_autonomous_driving_perception_and_planning_amd.harness import synthetic_frame
    out = {}
    imgs = [Image.fromarray(np.ascontiguousarray(synthetic_frame(H, W, s, 3 * s)[:, :, ::-1])) for s in range(N)]
    for k, (_, kw) in enumerate(VARIANTS):
        for s, im in enumerate(imgs):
            b = io.BytesIO()
            im.save(b, "JPEG", quality=85, subsampling=2, **kw)
            out["v%d_%02d" % (k, s)] = np.frombuffer(b.getvalue(), np.uint8)
    return out


def load_frames(path):
    if path and os.path.exists(path):
        z = np.load(path)
        enc = {k: z[k] for k in z.files}
    else:
        enc = encode_frames()
    return [[enc["v%d_%02d" % (k, s)].tobytes() for s in range(N)] for k in range(len(VARIANTS))]


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


def wall_ms(fn, sync, runs=9):
    for _ in range(2):
        fn()
    sync()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_stats(path):
    """rocprofv3's kernel_stats.csv -> {kernel name (without arguments): (calls, average ns)}"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for short in list(KERNEL_BYTES_PER_PX) + ["jpeg_entropy_kernel", "i420_to_bgr_kernel"]:
                if short in name:
                    calls, total = int(row["Calls"]), float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
                    c0, t0 = out.get(short, (0, 0.0))
                    out[short] = (c0 + calls, t0 + total)
    return {k: (c, t / max(c, 1)) for k, (c, t) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode", default=None)
    ap.add_argument("--frames", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--variant", type=int, default=-1, help="with --profile: only this variant (0: restart rows, 1: none)")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a --profile run per variant, comma separated")
    ap.add_argument("--commit", default="", help="the commit the measured tree is (or, with --dirty, is based on)")
    ap.add_argument("--dirty", action="store_true", help="the measured tree has changes that commit does not hold")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.encode:
        np.savez(a.encode, **encode_frames())
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/mjpegtime.py measures on the GPU; none is visible")
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    from multimodal_autonomous_driving_perception_and_planning_amd._dev import Dev
    from multimodal_autonomous_driving_perception_and_planning_amd.loaders import JpegBatchDecoder
    dev = Dev(0)
    L, stream = dev.lib, torch.cuda.current_stream()
    variants = load_frames(a.frames)
    dst = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev.device)
    res = dict(commit=a.commit, uncommitted_changes=bool(a.dirty), frames=N, height=H, width=W, quality=85, subsampling="4:2:0", hbm_bytes_per_s=HBM, variants=[])
    px = N * H * W
    for k, ((name, _), jpegs) in enumerate(zip(VARIANTS, variants)):
        if a.profile and a.variant not in (-1, k):
            continue
        dec = JpegBatchDecoder(dev, H, W)
        dec.decode(jpegs, dst)
        assert not dec.last_status().any(), "the frames do not decode cleanly"
        n, b, seg_off, total, max_segs, desc_bytes, data_bytes = dec.last_call

        def kernels():
            nat.check(L.av_jpeg_decode(dev.ctx.handle, nat.stream_handle(stream), n, H, W, b, b + seg_off, total, max_segs, b + desc_bytes,
                                       data_bytes, nat.ptr(dec._ws), nat.ptr(dst), nat.ptr(dec.status)))
        if a.profile:
            for _ in range(20):
                kernels()
            stream.synchronize()
            continue
        whole = wall_ms(lambda: dec.decode(jpegs, dst), stream.synchronize)
        dev_ms, calls = event_ms(torch, kernels, stream)
        v = dict(name=name, compressed_bytes=sum(map(len, jpegs)), segments_per_frame=max_segs, whole_read_ms=whole, kernels_ms=dev_ms,
                 kernels_calls_per_run=calls)
        res["variants"].append(v)
        print("%-30s %5.1f MB compressed, %d segments per frame: whole read median %.3f ms (host clock), four kernels %.3f ms (events, runs of "
              "%d)" % (name, v["compressed_bytes"] / 1e6, max_segs, statistics.median(whole), statistics.median(dev_ms), calls), flush=True)
    if a.profile:
        return
    # the path without a decoder: 64 frames' worth of I420 planes (random bytes: the conversion's time does not depend on them)
    yuv = np.random.RandomState(0).randint(0, 256, (N, H * W * 3 // 2)).astype(np.uint8)
    dyuv = dev.upload(yuv, np.uint8)

    def convert():
        nat.check(L.av_i420_to_bgr(dev.ctx.handle, nat.stream_handle(stream), N, H, W, nat.ptr(dyuv), nat.ptr(dst)))

    def upload_convert():
        t = dev.upload(yuv, np.uint8)
        nat.check(L.av_i420_to_bgr(dev.ctx.handle, nat.stream_handle(stream), N, H, W, nat.ptr(t), nat.ptr(dst)))
    whole = wall_ms(upload_convert, stream.synchronize)
    conv, calls = event_ms(torch, convert, stream)
    res["i420"] = dict(bytes=int(yuv.nbytes), whole_read_ms=whole, kernel_ms=conv)
    print("%-30s %5.1f MB of planes: upload + av_i420_to_bgr median %.3f ms (host clock), the kernel %.3f ms = %.2f TB/s over its 4.5 bytes "
          "per pixel" % ("I420 planes (no decoder)", yuv.nbytes / 1e6, statistics.median(whole), statistics.median(conv),
                         px * 4.5 / (statistics.median(conv) * 1e-3) / 1e12), flush=True)
    for v, path in zip(res["variants"], a.stats.split(",") if a.stats else []):
        ks = kernel_stats(path)
        v["kernel_ns"] = {k: dict(calls=c, average_ns=t) for k, (c, t) in ks.items()}
        print("kernel trace, %s:" % v["name"])
        for k, (c, t) in sorted(ks.items()):
            bpp = KERNEL_BYTES_PER_PX.get(k)
            extra = ""
            if bpp:
                rate = px * bpp / (t * 1e-9)
                extra = ": %.1f bytes per pixel -> %.2f TB/s, %.0f %% of %.1f TB/s" % (bpp, rate / 1e12, 100 * rate / HBM, HBM / 1e12)
                v["kernel_ns"][k].update(bytes_per_pixel=bpp, bytes_per_s=rate)
            print("    %-22s %6d calls, average %9.1f us%s" % (k, c, t / 1e3, extra), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
