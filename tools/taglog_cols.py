#!/usr/bin/env python3
"""Timings of the tag log's records.  Not part of the bench contract.

  av_taglog_search (the mask query as it was) beside av_taglog_search_where with only mask bounds and with every bound set, on a
      log of S streams x n frames with records: HIP events on the stream, the median of REPS calls after WARM calls, three rounds,
      beside the time the bytes each query has to read need at 6.3 TB/s
  TagLog.records_where returning about 1 % of the frames: host clock around the whole call (search, gather, download, decoding)
  TagDatabase.save_tag_log of a 64 x 4096 log into a file, full_data on and off: host clock
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.database import TagDatabase  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.tagging import tag_log as T  # noqa: E402

HBM = 6.3e12          # bytes / s the card reaches (MI355X_MICROARCH: achievable HBM bandwidth)
WARM, REPS, ROUNDS = 5, 20, 3


def event_rounds(L, stream, fn):
    a, b, ms, out = C.c_void_p(), C.c_void_p(), C.c_float(), []
    nat.check(L.av_event_create(C.byref(a)))
    nat.check(L.av_event_create(C.byref(b)))
    for _ in range(ROUNDS):
        ts = []
        for k in range(WARM + REPS):
            nat.check(L.av_event_record(a, stream))
            fn()
            nat.check(L.av_event_record(b, stream))
            nat.check(L.av_event_elapsed_ms(a, b, C.byref(ms)))
            if k >= WARM:
                ts.append(ms.value)
        out.append(statistics.median(ts))
    return out


def fill(log, seed):
    """Frames as the loops log them, made on the device: one road type, day or night, the three maneuver enums, the three presence
    flags; speeds 0..130; records with a quarter of the min_ttc NaN and counts 0..3."""
    g = torch.Generator(device=log.dev)
    g.manual_seed(seed)
    S, n = log.S, log.cap
    ri = lambda hi, sh: torch.randint(0, hi, sh, generator=g, device=log.dev, dtype=torch.int64)       # noqa: E731
    for s in range(S):                                                  # a stream at a time: the temporaries stay small
        m = torch.ones(n, dtype=torch.int64, device=log.dev) << ri(6, (n,))
        m |= torch.ones_like(m) << (13 + ri(2, (n,)))
        for base, k in ((T.LATERAL, 4), (T.LONGITUDINAL, 5), (T.TURNING, 6)):
            m |= torch.ones_like(m) << (base + ri(k, (n,)))
        log.mask[s] = m | (7 << 61) - (1 << 64)                         # the three flags, as a signed 64-bit pattern
        log.speed[s] = torch.rand(n, generator=g, device=log.dev, dtype=torch.float64) * 130.0
        f = torch.rand(n, 10, generator=g, device=log.dev, dtype=torch.float64)
        f[:, 4] = f[:, 4] * 12.0 - 8.0                                  # acceleration
        none = torch.rand(n, generator=g, device=log.dev, dtype=torch.float64) < 0.25
        f[:, 6] = torch.where(none, torch.nan, f[:, 6] * 10.0)          # min_ttc
        f[:, 7] *= 80.0                                                 # closest distance
        f.view(torch.int32)[:, 16:20] = torch.randint(0, 4, (n, 4), generator=g, device=log.dev, dtype=torch.int32)
        log.cols[s] = f.view(torch.uint8)
    log.log_n.fill_(n)
    torch.cuda.synchronize()


def queries(S, n, res):
    log = T.TagLog(S, n, stream=torch.cuda.Stream(), columns=True)
    fill(log, S)
    L, h, st, P = log.L, log.ctx.handle, log._s(), nat.ptr
    out = torch.empty(S, n, dtype=torch.int32, device=log.dev)
    day = T.tag_mask(["day"])
    masks_only, _ = T._where(tags=["day"])
    every = dict(tags=["day"], none=["fog"], speed=(10.0, 120.0), acceleration=(-7.0, 3.5), max_ttc=9.0, max_distance=70.0, min_agents=1,
                 min_pedestrians=1, min_cyclists=1, min_vehicles=1)
    bounded, _ = T._where(**every)

    def search():
        nat.check(L.av_taglog_search(h, st, S, n, P(log.mask), P(log.log_n), day, 0, 0, 0, n, P(log.ws), n, P(out), P(log._out_n)))

    def where(q):
        nat.check(L.av_taglog_search_where(h, st, S, n, P(log.mask), P(log.speed), P(log.cols), P(log.log_n), C.byref(q), 0, n, P(log.ws),
                                           n, P(out), P(log._out_n)))
    # bytes a frame costs: the mask; with every bound also the speed and the five words of the record, which lie in its 80 B
    for name, fn, bpf in (("av_taglog_search", search, 8), ("search_where, mask bounds only", lambda: where(masks_only), 8),
                          ("search_where, every bound set", lambda: where(bounded), 96)):
        ms = event_rounds(L, st, fn)
        log._sync()
        hits = int(log._out_n.sum())
        floor = S * n * bpf / HBM * 1e3
        res[name] = dict(S=S, n=n, ms=ms, floor_ms=floor, matches=hits)
        print("S=%d n=%d  %-32s %.1f us (rounds %s), %d matches; %d B/frame at 6.3 TB/s: %.1f us" % (
            S, n, name, statistics.median(ms) * 1e3, " ".join("%.1f" % (x * 1e3) for x in ms), hits, bpf, floor * 1e3), flush=True)
    # about 1 % of the frames as records: min_ttc below 0.1333 of 10 on three quarters of the frames
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        recs = log.records_where(max_ttc=0.1333)
        ts.append((time.perf_counter() - t0) * 1e3)
    got = sum(len(r) for r in recs)
    res["records_where"] = dict(S=S, n=n, ms=ts, records=got, share=got / (S * n))
    print("S=%d n=%d  records_where: %d records (%.2f %% of the frames), host clock %.1f ms (calls %s)" % (
        S, n, got, 100.0 * got / (S * n), statistics.median(ts[1:]), " ".join("%.1f" % t for t in ts)), flush=True)


def saving(S, n, res):
    log = T.TagLog(S, n, columns=True)
    fill(log, 7)
    for full in (True, False):
        with tempfile.TemporaryDirectory() as d:
            db = TagDatabase(os.path.join(d, "tags.db"))
            t0 = time.perf_counter()
            db.save_tag_log(log, full_data=full)
            dt = time.perf_counter() - t0
            frames = db.get_tag_statistics()["frame_count"]
            size = os.path.getsize(os.path.join(d, "tags.db"))
            db.close()
        res["save_tag_log full_data=%s" % full] = dict(S=S, n=n, seconds=dt, frames=frames, file_bytes=size)
        print("save_tag_log S=%d n=%d full_data=%s: %.2f s host clock, %d frames, file %.1f MB" % (S, n, full, dt, frames, size / 1e6),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1 << 20, help="frames per stream of the query log")
    ap.add_argument("--save-frames", type=int, default=4096, help="frames per stream of the log that is saved")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/taglog_cols.py measures on the GPU; none is visible")
    res = {}
    queries(a.streams, a.frames, res)
    saving(a.streams, a.save_frames, res)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
