#!/usr/bin/env python3
"""Tag log timings: HIP events on the stream the work runs on, the median of 30 calls after 10 warm-up calls, three
rounds.  Not part of the bench contract.

  pack + append of 64 x 256 frames (the taggers' rows of a HotLoop(64, window=256) step)
  av_taglog_search / _segments / _stats at S = 64 x 4096 frames and S = 1 x 2^20 frames, beside the time their bytes need at
      6.3 TB/s (8 B per frame for search and segments, 16 B for stats)
  the host AutoTagger.search_by_tag over the same frames decoded to Python objects (wall clock)
  the step of HotLoop(64, window=256) with the maneuver and interaction stages, without and with enqueue_tags, alternating
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.harness import generate_ego_motion  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.tagging.auto_tagger import AutoTagger, FrameTags  # noqa: E402
from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import TagLog, tag_mask, tags_of  # noqa: E402

HBM = 6.3e12          # bytes / s the card reaches (MI355X_MICROARCH: achievable HBM bandwidth)
WARM, REPS, ROUNDS = 10, 30, 3


class Events:
    def __init__(self):
        self.L = nat.lib()
        self.a, self.b = C.c_void_p(), C.c_void_p()
        nat.check(self.L.av_event_create(C.byref(self.a)))
        nat.check(self.L.av_event_create(C.byref(self.b)))

    def rounds(self, stream, fn, each_round=None):
        """-> [median ms of REPS event-timed calls after WARM calls] x ROUNDS; each_round() runs ahead of every round"""
        ms, out = C.c_float(), []
        for _ in range(ROUNDS):
            if each_round is not None:
                each_round()
            ts = []
            for k in range(WARM + REPS):
                nat.check(self.L.av_event_record(self.a, stream))
                fn()
                nat.check(self.L.av_event_record(self.b, stream))
                nat.check(self.L.av_event_elapsed_ms(self.a, self.b, C.byref(ms)))
                if k >= WARM:
                    ts.append(ms.value)
            out.append(statistics.median(ts))
        return out


def fmt(ms):
    return "%.2f us (rounds %s)" % (statistics.median(ms) * 1e3, " ".join("%.2f" % (x * 1e3) for x in ms))


def random_masks(rng, S, n):
    """Frames as the loops log them: one road type, day or night, the three maneuver enums, sometimes an interaction and a risk."""
    m = np.uint64(1) << rng.integers(0, 6, (S, n)).astype(np.uint64)
    m |= np.uint64(1) << rng.choice([13, 14], (S, n)).astype(np.uint64)
    for base, k in ((18, 4), (22, 5), (27, 6)):
        m |= np.uint64(1) << (np.uint64(base) + rng.integers(0, k, (S, n)).astype(np.uint64))
    inter = rng.random((S, n)) < 0.3
    m |= np.where(inter, np.uint64(1) << (np.uint64(33) + rng.integers(0, 13, (S, n)).astype(np.uint64)), np.uint64(0))
    m |= np.where(rng.random((S, n)) < 0.05, np.uint64(1) << (np.uint64(46) + rng.integers(0, 3, (S, n)).astype(np.uint64)), np.uint64(0))
    # cut-ins come in runs, so the segment query has something to find
    runs = np.repeat(rng.random((S, (n + 31) // 32)) < 0.2, 32, axis=1)[:, :n]
    m |= np.where(runs, np.uint64(1) << np.uint64(37), np.uint64(0))
    return m | np.uint64(7 << 61)


def queries(ev, S, n, host_search):
    rng = np.random.default_rng(S)
    log = TagLog(S, n, stream=torch.cuda.Stream())
    masks = random_masks(rng, S, n)
    for f0 in range(0, n, 1 << 16):
        log.append(masks[:, f0:f0 + (1 << 16)], rng.uniform(0, 130, masks[:, f0:f0 + (1 << 16)].shape))
    assert log.lengths().tolist() == [n] * S
    L, h, st = log.L, log.ctx.handle, log._s()
    tag = tag_mask(["vehicle_cut_in"])
    out = torch.empty(S, n, 2, dtype=torch.int32, device=log.dev)
    stats = torch.empty(S, nat.TAGLOG_STATS_BYTES, dtype=torch.uint8, device=log.dev)
    P = nat.ptr

    def search():
        nat.check(L.av_taglog_search(h, st, S, n, P(log.mask), P(log.log_n), tag, 0, 0, 0, n, P(log.ws), n, P(out), P(log._out_n)))

    def segments():
        nat.check(L.av_taglog_segments(h, st, S, n, P(log.mask), P(log.log_n), tag, 0, 0, 0, n, 5, P(log.ws), n, P(out), P(log._out_n)))

    def stat():
        nat.check(L.av_taglog_stats(h, st, S, n, P(log.mask), P(log.speed), P(log.log_n), P(log.ws), P(stats)))
    res = {}
    for name, fn, bpf in (("search", search, 8), ("segments", segments, 8), ("stats", stat, 16)):
        ms = ev.rounds(st, fn)
        floor = S * n * bpf / HBM * 1e3
        res[name] = dict(ms=ms, floor_ms=floor)
        print("S=%d n=%d  %-8s %s   floor %.2f us (%d B/frame at 6.3 TB/s): x%.1f" % (
            S, n, name, fmt(ms), floor * 1e3, bpf, statistics.median(ms) / floor), flush=True)
    found = [len(x) for x in log.search_by_tag("vehicle_cut_in")]
    segs = [len(x) for x in log.get_event_segments("vehicle_cut_in", 5)]
    print("S=%d n=%d  matches %d, segments %d" % (S, n, sum(found), sum(segs)), flush=True)
    if host_search:
        # the host route: every frame decoded to the reference's Python objects, AutoTagger.search_by_tag per stream
        t0 = time.perf_counter()
        taggers = []
        for s in range(S):
            at = AutoTagger.__new__(AutoTagger)
            at.frame_tags = [FrameTags(frame_idx=i, timestamp=i / 30.0, all_tags=tags_of(m)) for i, m in enumerate(masks[s].tolist())]
            taggers.append(at)
        decode = time.perf_counter() - t0
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            hits = [len(at.search_by_tag("vehicle_cut_in")) for at in taggers]
            ts.append(time.perf_counter() - t0)
        assert hits == found
        res["host_search_ms"] = [t * 1e3 for t in ts]
        print("S=%d n=%d  host AutoTagger.search_by_tag %.1f ms (runs %s); decoding the masks to Python objects %.1f s" % (
            S, n, statistics.median(ts) * 1e3, " ".join("%.1f" % (t * 1e3) for t in ts), decode), flush=True)
    return res


def loop_stages(ev, S, W, steps):
    loop = HotLoop(n_streams=S, window=W, keep_waypoints=False)
    loop.reset(frame_offsets=[s * 17 for s in range(S)])
    loop.load_measurements(np.stack([np.asarray(generate_ego_motion(W, seed=s % 8), np.float64) for s in range(S)]))
    log = loop.enable_tag_log(W * (WARM + REPS + 2))
    L, h, s = loop.L, loop.ctx.handle, loop._s

    def step(tags):
        # bench.py --taggers' step, plus the tag stage
        nat.check(L.av_fork(h, s))
        loop.enqueue_detect(loop.ctx.side_stream)
        loop.enqueue_track(loop.ctx.side_stream)
        loop.enqueue_kf()
        loop.enqueue_plan()
        loop.enqueue_maneuver()
        nat.check(L.av_join(h, s))
        loop.enqueue_interactions()
        if tags:
            loop.enqueue_tags()
    with torch.cuda.stream(loop.stream):
        step(True)
    loop.synchronize()
    out = ev.rounds(s, loop.enqueue_tags, each_round=log.reset)       # pack + append alone; the log is emptied before it would fill up
    print("pack + append  S=%d W=%d  %s   (%d frames, %.2f ns/frame)" % (S, W, fmt(out), S * W, statistics.median(out) * 1e6 / (S * W)),
          flush=True)
    res = dict(pack_append_ms=out)
    # the step without / with the tag stage: `steps` steps per run between two host clocks, alternating
    runs = {False: [], True: []}
    for r in range(2 * 5):
        tags = bool(r % 2)
        log.reset()
        loop.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(tags)
        nat.check(L.av_join(h, s))
        loop.synchronize()
        runs[tags].append((time.perf_counter() - t0) / steps * 1e3)
    for tags in (False, True):
        v = runs[tags]
        print("step S=%d W=%d taggers%s: median %.4f ms, range %.4f .. %.4f (runs of %d steps: %s)" % (
            S, W, " + tags" if tags else "       ", statistics.median(v), min(v), max(v), steps, " ".join("%.4f" % x for x in v)), flush=True)
    res["step_ms"] = {"taggers": runs[False], "taggers_tags": runs[True]}
    assert log.dropped.cpu().tolist() == [0] * S
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", type=int, default=1 << 20, help="frames of the S = 1 log")
    ap.add_argument("--steps", type=int, default=30, help="steps per run of the loop comparison")
    ap.add_argument("--no-host", action="store_true", help="skip the host AutoTagger search")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/taglog.py measures on the GPU; none is visible")
    ev = Events()
    res = {"loop": loop_stages(ev, 64, 256, a.steps)}
    res["S64_n4096"] = queries(ev, 64, 4096, not a.no_host)
    res["S1_n%d" % a.long] = queries(ev, 1, a.long, not a.no_host)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
