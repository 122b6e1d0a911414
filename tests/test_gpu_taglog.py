"""The tag log on the device (csrc/taglog.hip, tagging/tag_log.py) against the NumPy restatement tests/taglog_ref.py.

(1) the 53 frames the real reference AutoTagger recorded (tests/golden/scene.npz), logged on three streams behind 0 / 5 / 11 frames
    of padding, as one window and as windows of 1, 7 and 45: searches, segments and statistics equal the recorded ones;
(2) av_tags_pack on the real reference's maneuver and interaction rows (tests/golden/maneuver.npz, interaction.npz) and on
    hand-made rows for what those do not hold; (3) boundaries of the wave rounds (64) and chunks (AV_TAGLOG_CHUNK), capacities,
    sub-ranges, appending past the capacity; (4) HotLoop.enqueue_tags; (5) CameraLoop(tags=...); (6) argument checks.
Everything is exact (integers, bit masks, min / max) except speed_sum: any summation order of n <= 4096 non-negative doubles stays
within (n - 1) * 2^-53 < 4.6e-13 of the exact sum relatively, so two orders agree to 1e-12.
"""
import json
import os

import numpy as np
import pytest

from tests import taglog_ref as R

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLAGS = (1 << R.HAS_SCENE) | (1 << R.HAS_MANEUVER) | (1 << R.HAS_INTERACTION)
EINVAL = -1


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    return torch, nat, nat.lib(), nat.default_context(0)


def _bytes(env, a):
    """A NumPy array (structured ones included) as a device tensor of its bytes."""
    torch = env[0]
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")


class RawLog:
    """The four arrays and the workspace of a log, driven through the C ABI on torch's current stream."""

    def __init__(self, env, S, cap):
        torch, nat, L, ctx = env
        self.env, self.S, self.cap = env, S, cap
        d = torch.device("cuda", 0)
        self.mask = torch.zeros(S, cap, dtype=torch.int64, device=d)
        self.speed = torch.zeros(S, cap, dtype=torch.float64, device=d)
        self.log_n = torch.zeros(S, dtype=torch.int32, device=d)
        self.dropped = torch.zeros(S, dtype=torch.int32, device=d)
        self.ws = torch.zeros(int(L.av_taglog_workspace_bytes(S, cap)), dtype=torch.uint8, device=d)
        self.out_n = torch.zeros(S, dtype=torch.int32, device=d)
        torch.cuda.synchronize()

    def load(self, masks, speeds=None):
        """Streams of different lengths: written straight into the arrays."""
        torch = self.env[0]
        m, v, n = np.zeros((self.S, self.cap), np.uint64), np.zeros((self.S, self.cap)), np.zeros(self.S, np.int32)
        for s, row in enumerate(masks):
            n[s] = len(row)
            m[s, :len(row)] = np.asarray(row, np.uint64)
            if speeds is not None:
                v[s, :len(row)] = speeds[s]
        self.mask.copy_(torch.from_numpy(m.view(np.int64)))
        self.speed.copy_(torch.from_numpy(v))
        self.log_n.copy_(torch.from_numpy(n))

    def append(self, masks, speeds):
        torch, nat, L, ctx = self.env
        m = torch.from_numpy(np.ascontiguousarray(masks, np.uint64).view(np.int64)).to("cuda:0")
        v = torch.from_numpy(np.ascontiguousarray(speeds, np.float64)).to("cuda:0")
        return L.av_taglog_append(ctx.handle, nat.stream_handle(), self.S, masks.shape[1], nat.ptr(m), nat.ptr(v), self.cap,
                                  nat.ptr(self.mask), nat.ptr(self.speed), nat.ptr(self.log_n), nat.ptr(self.dropped))

    def _run(self, fn, width, out_cap, args):
        torch, nat, L, ctx = self.env
        out = torch.full((self.S, max(out_cap, 1), width), -7, dtype=torch.int32, device="cuda:0")
        nat.check(fn(ctx.handle, nat.stream_handle(), self.S, self.cap, nat.ptr(self.mask), nat.ptr(self.log_n), *args,
                     nat.ptr(self.ws), out_cap, nat.ptr(out), nat.ptr(self.out_n)))
        torch.cuda.synchronize()
        return out.cpu().numpy(), self.out_n.cpu().numpy()

    def search(self, p, first, last, out_cap):
        out, n = self._run(self.env[2].av_taglog_search, 1, out_cap, (p[0], p[1], p[2], first, last))
        return out[:, :, 0], n

    def segments(self, p, first, last, min_duration, seg_cap):
        return self._run(self.env[2].av_taglog_segments, 2, seg_cap, (p[0], p[1], p[2], first, last, min_duration))

    def stats(self):
        torch, nat, L, ctx = self.env
        out = torch.zeros(self.S, nat.TAGLOG_STATS_BYTES, dtype=torch.uint8, device="cuda:0")
        nat.check(L.av_taglog_stats(ctx.handle, nat.stream_handle(), self.S, self.cap, nat.ptr(self.mask), nat.ptr(self.speed),
                                    nat.ptr(self.log_n), nat.ptr(self.ws), nat.ptr(out)))
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.dtype(nat.TAGLOG_STATS_FIELDS)).reshape(self.S)


def _check_queries(log, masks, p, first, last, min_duration, cap_small=None):
    """Search and segments of every stream against the restatement: with room for everything, and with cap_small rows."""
    ref_s = [R.search(m, *p, first=first, last=last) for m in masks]
    ref_g = [R.segments(m, *p, min_duration=min_duration, first=first, last=last) for m in masks]
    for cap in ([log.cap] if cap_small is None else [log.cap, cap_small]):
        idx, n = log.search(p, first, last, cap)
        seg, ns = log.segments(p, first, last, min_duration, cap)
        for s in range(log.S):
            where = "stream %d (%d frames) range [%d, %d) min_duration %d cap %d" % (s, len(masks[s]), first, last, min_duration, cap)
            k = min(len(ref_s[s]), cap)
            assert n[s] == len(ref_s[s]) and idx[s, :k].tolist() == ref_s[s][:k], where
            assert (idx[s, k:] == -7).all(), where                        # rows at or past min(out_n, out_cap): untouched
            k = min(len(ref_g[s]), cap)
            assert ns[s] == len(ref_g[s]) and [tuple(x) for x in seg[s, :k].tolist()] == ref_g[s][:k], where
            assert (seg[s, k:] == -7).all(), where
    return sum(map(len, ref_s)), sum(map(len, ref_g))


def _check_stats(log, masks, speeds):
    got = log.stats()
    for s in range(log.S):
        want = R.stats(masks[s], speeds[s])
        assert got[s]["tag_count"].tolist() == want["tag_count"], s
        assert (got[s]["n_frames"], got[s]["n_maneuver"]) == (want["n_frames"], want["n_maneuver"]), s
        assert got[s]["risk_count"].tolist() == want["risk_count"], s
        assert (got[s]["speed_min"], got[s]["speed_max"]) == (want["speed_min"], want["speed_max"]), s
        np.testing.assert_allclose(got[s]["speed_sum"], want["speed_sum"], rtol=1e-12, atol=0)


# ---- (1) the golden log ---------------------------------------------------------------------------------------------------

def _golden():
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import TAGS
    want = json.loads(str(np.load(os.path.join(GOLDEN, "scene.npz"))["auto_json"]))
    masks = np.array([R.mask_of(f["all_tags"], list(TAGS)) | FLAGS for f in want["frames"]], np.uint64)
    speeds = np.array([float(r["speed_kmh"]) for r in want["csv"]])
    return masks, speeds, want


@gpu
@pytest.mark.parametrize("windows", [(53,), (1, 7, 45)])
def test_golden_log(env, windows):
    torch = env[0]
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import TagLog
    masks, speeds, want = _golden()
    pads = [0, 5, 11]
    log = TagLog(3, 70, ctx=env[3])
    log.log_n.copy_(torch.tensor(pads, dtype=torch.int32))              # the padding: frames without a tag or a flag
    f0 = 0
    for W in windows:
        log.append(np.tile(masks[f0:f0 + W], (3, 1)), np.tile(speeds[f0:f0 + W], (3, 1)))
        f0 += W
    assert log.lengths().tolist() == [53, 58, 64] and len(log) == 64 and log.dropped.cpu().tolist() == [0, 0, 0]
    s, ws = want["searches"], want["statistics"]
    for k, pad in enumerate(pads):
        assert log.masks(k)[pad:].tolist() == masks.tolist() and not log.masks(k)[:pad].any()
        for tag, idx in s["by_tag"].items():
            assert (log.search_by_tag(tag, stream=k) - pad).tolist() == idx, (k, tag)
        assert (log.search_by_tags(["day", "residential"], stream=k) - pad).tolist() == s["all_"]
        assert (log.search_by_tags(["night", "congested"], match_all=False, stream=k) - pad).tolist() == s["any_"]
        assert log.get_high_risk_frames(stream=k).tolist() == s["high_risk"] == []
        for tag, d in dict(day=5, highway=3, night=5, residential=8).items():
            got = log.get_event_segments(tag, d, stream=k)
            assert got.shape == (len(s["segments"][tag]), 2) and (got - pad).tolist() == s["segments"][tag], (k, tag)
        st = log.get_tag_statistics(k)
        assert st["total_frames"] == 53 + pad and st["unique_tags"] == ws["unique_tags"]
        assert st["tag_counts"] == ws["tag_counts"] and st["risk_distribution"] == ws["risk_distribution"]
        assert st["speed_stats"]["min"] == ws["speed_stats"]["min"] and st["speed_stats"]["max"] == ws["speed_stats"]["max"]
        assert st["speed_stats"]["avg"] == pytest.approx(ws["speed_stats"]["avg"], rel=1e-12)
        assert st["tag_frequency"] == {t: c / (53 + pad) for t, c in ws["tag_counts"].items()}
    # all streams at once, the empty lists, a tag outside the vocabulary
    every = log.search_by_tags([])
    assert [e.tolist() for e in every] == [list(range(53 + p)) for p in pads]
    assert all(len(e) == 0 for e in log.search_by_tags([], match_all=False)) and len(log.search_by_tag("no such tag", stream=1)) == 0
    assert log.get_event_segments("no such tag", 1, stream=0).shape == (0, 2)
    assert [len(x) for x in log.search_by_tag("fog")] == [12, 12, 12]
    log.reset()
    assert len(log) == 0 and log.get_tag_statistics(0) == {}


@gpu
def test_query_buffers_grow(env):
    """More answers than the output buffers' first 256 rows: the query is repeated with room, nothing is cut."""
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import TagLog, tag_mask
    n = 700
    fog = np.uint64(tag_mask(["fog"]))
    masks = np.zeros((2, n), np.uint64)
    masks[0, ::2] = fog                                               # 350 runs of one frame
    masks[1, 5:] = fog
    log = TagLog(2, 1024, ctx=env[3])
    log.append(masks, np.zeros((2, n)))
    got = log.search_by_tag("fog")
    assert got[0].tolist() == list(range(0, n, 2)) and got[1].tolist() == list(range(5, n))
    segs = log.get_event_segments("fog", 1)
    assert segs[0].tolist() == [[i, i] for i in range(0, n, 2)] and segs[1].tolist() == [[5, n - 1]]
    assert log.get_event_segments("fog", 2, stream=0).shape == (0, 2) and len(log.search_by_tag("fog", stream=0)) == 350
    assert log.search_masks(none=int(fog), stream=1).tolist() == [0, 1, 2, 3, 4]


# ---- (2) pack ------------------------------------------------------------------------------------------------------------

def _pack(env, S, W, maneuver=None, irows=None, isum=None, snap_n=None, tcap=64, scene=None, det_n=None, det_cls=None, elem=None):
    torch, nat, L, ctx = env
    dev = {k: (None if v is None else _bytes(env, v)) for k, v in dict(m=maneuver, r=irows, q=isum, n=snap_n, s=scene, dn=det_n,
                                                                       dc=det_cls, e=elem).items()}
    om = torch.full((S, W), -1, dtype=torch.int64, device="cuda:0")
    ov = torch.zeros(S, W, dtype=torch.float64, device="cuda:0")
    rc = L.av_tags_pack(ctx.handle, nat.stream_handle(), S, W, nat.ptr(dev["m"]), nat.ptr(dev["r"]), nat.ptr(dev["q"]),
                        nat.ptr(dev["n"]), tcap, nat.ptr(dev["s"]), nat.ptr(dev["dn"]), nat.ptr(dev["dc"]),
                        0 if det_cls is None else det_cls.shape[-1], nat.ptr(dev["e"]), 0 if elem is None else len(elem),
                        nat.ptr(om), nat.ptr(ov))
    torch.cuda.synchronize()
    return rc, om.cpu().numpy().view(np.uint64), ov.cpu().numpy()


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)


@gpu
def test_pack_reference_rows(env):
    nat = env[1]
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging import interaction_detector as I, maneuver_detector as M
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import tag_mask
    gm, gi = np.load(os.path.join(GOLDEN, "maneuver.npz")), np.load(os.path.join(GOLDEN, "interaction.npz"))
    S, W = 2, 64
    man = np.zeros((S, W), np.dtype(nat.MANEUVER_ROW_FIELDS))
    idx, val = gm["idx"][:128].reshape(S, W, 3), gm["val"][:128].reshape(S, W, 7)
    man["lateral"], man["longitudinal"], man["turning"] = idx[..., 0], idx[..., 1], idx[..., 2]
    for k, name in enumerate(("lateral_confidence", "longitudinal_confidence", "turning_confidence", "speed_kmh", "acceleration",
                              "yaw_rate_deg", "timestamp")):
        man[name] = val[..., k]
    rows = np.zeros((S, W, 64), np.dtype(nat.INTERACTION_ROW_FIELDS))
    rows["type"], rows["confidence"] = gi["type"][:128].reshape(S, W, 64), gi["conf"][:128].reshape(S, W, 64)
    summ = np.zeros((S, W), np.dtype(nat.INTERACTION_SUMMARY_FIELDS))
    summ["overall_risk"] = gi["overall"][:128].reshape(S, W)
    snap_n = gi["n_tracks"][:128].reshape(S, W).astype(np.int32)
    rc, got_m, got_v = _pack(env, S, W, man, rows, summ, snap_n)
    assert rc == 0
    assert _same((got_m, got_v), R.pack(S, W, man, rows, summ, snap_n))
    # the port's dataclasses built from the same rows
    tagged = 0
    for s in range(S):
        for w in range(W):
            mt = M.ManeuverTags(lateral=M._LAT[idx[s, w, 0]], longitudinal=M._LON[idx[s, w, 1]], turning=M._TRN[idx[s, w, 2]])
            it = I.InteractionTags(interactions=[I.Interaction(I._TYPES[r["type"]], float(r["confidence"]), I.RiskLevel.LOW)
                                                 for r in rows[s, w, :snap_n[s, w]] if r["type"] >= 0],
                                   overall_risk=I._RISKS[summ[s, w]["overall_risk"]])
            tagged += len(it.get_tags_list())
            want = tag_mask(mt.get_tags_list() + it.get_tags_list()) | (1 << R.HAS_MANEUVER) | (1 << R.HAS_INTERACTION)
            assert int(got_m[s, w]) == want and got_v[s, w] == val[s, w, 3], (s, w)
    assert tagged > 0


def _hand_rows(nat):
    """Twelve frames of what the goldens do not hold (their confidences are 0.6 .. 0.9, their overall risk low or critical)."""
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import tags_of
    W, MD = 12, 70
    man = np.zeros((1, W), np.dtype(nat.MANEUVER_ROW_FIELDS))
    rows = np.zeros((1, W, 64), np.dtype(nat.INTERACTION_ROW_FIELDS))
    summ = np.zeros((1, W), np.dtype(nat.INTERACTION_SUMMARY_FIELDS))
    scene = np.zeros((1, W), np.dtype(nat.SCENE_ROW_FIELDS))
    snap_n, det_n = np.zeros((1, W), np.int32), np.zeros((1, W), np.int32)
    det_cls = np.zeros((1, W, MD), np.int32)
    elem = np.array([0, 1, 2, 0, 5, 6, 3], np.uint8)                 # class 5: an entry past the five elements
    rows["type"] = -1
    man["speed_kmh"] = np.arange(W) + 0.25
    want = {}
    # 0: confidence exactly 0.5 and just below it: no tag
    rows[0, 0, 0]["type"], rows[0, 0, 0]["confidence"] = 4, 0.5
    rows[0, 0, 1]["type"], rows[0, 0, 1]["confidence"] = 5, 0.4999
    snap_n[0, 0] = 2
    want[0] = ["unknown", "lane_keeping", "cruising", "straight"]
    # 1: type -1 is no interaction whatever its confidence; type 0 is the tag no_interaction; just above 0.5
    rows[0, 1, 0]["type"], rows[0, 1, 0]["confidence"] = -1, 0.9
    rows[0, 1, 1]["type"], rows[0, 1, 1]["confidence"] = 0, np.nextafter(0.5, 1.0)
    snap_n[0, 1] = 2
    want[1] = want[0] + ["no_interaction"]
    # 2: a row at index snap_n is ignored; row 63 of a full table is not
    rows[0, 2, 2]["type"], rows[0, 2, 2]["confidence"] = 6, 0.9
    rows[0, 2, 0]["type"], rows[0, 2, 0]["confidence"] = 1, 0.51
    snap_n[0, 2] = 2
    want[2] = want[0] + ["following_vehicle"]
    rows[0, 3, 63]["type"], rows[0, 3, 63]["confidence"] = 12, 0.7
    snap_n[0, 3] = 99                                                # clamped to the table
    want[3] = want[0] + ["being_passed"]
    # 4 .. 6: overall risk 1, 2 and out of range
    summ[0, 4]["overall_risk"], summ[0, 5]["overall_risk"], summ[0, 6]["overall_risk"] = 1, 2, 99
    want[4], want[5], want[6] = want[0] + ["risk_medium"], want[0] + ["risk_high"], want[0]
    # 7: every enum index -1; 8: every enum index 99 (13 for the interaction type: one past the last)
    for f, bad in ((7, -1), (8, 99)):
        man[0, f]["lateral"] = man[0, f]["longitudinal"] = man[0, f]["turning"] = bad
        scene[0, f]["road_type"], scene[0, f]["n_conditions"] = bad, 2
        scene[0, f]["conditions"] = [bad, 3, 0]
        rows[0, f, 0]["type"], rows[0, f, 0]["confidence"] = (13 if bad > 0 else bad), 0.9
        rows[0, f, 1]["type"], rows[0, f, 1]["confidence"] = bad, 0.9
        summ[0, f]["overall_risk"] = -1 if bad < 0 else 4
        snap_n[0, f] = 2
        want[f] = ["day"]
    # 9: n_conditions above the three slots and below zero; has_pedestrian any non-zero
    scene[0, 9]["road_type"], scene[0, 9]["n_conditions"], scene[0, 9]["conditions"], scene[0, 9]["has_pedestrian"] = 5, 7, [5, 4, 2], 2
    want[9] = ["parking", "night", "rain", "fog", "pedestrian_area", "lane_keeping", "cruising", "straight"]
    scene[0, 10]["n_conditions"], scene[0, 10]["conditions"] = -2, [1, 1, 1]
    # 10: det_n above max_det (the second round of 64 is visited up to max_det, not beyond); class ids outside the table,
    # an empty entry, an entry past the elements
    det_n[0, 10] = 100
    det_cls[0, 10, :8] = [-1, 1000, 0, 3, 5, 7, -2 ** 31, 2 ** 31 - 1]
    det_cls[0, 10, 66] = 6                                           # crosswalk, in the second round
    det_cls[0, 10, 69] = 4                                           # speed_limit, the last visited entry
    want[10] = ["unknown", "crosswalk", "speed_limit", "lane_keeping", "cruising", "straight"]
    # 11: detections behind det_n are not visited
    det_n[0, 11] = 1
    det_cls[0, 11, :3] = [2, 1, 1]
    want[11] = ["unknown", "stop_sign", "lane_keeping", "cruising", "straight"]
    return dict(maneuver=man, irows=rows, isum=summ, snap_n=snap_n, scene=scene, det_n=det_n, det_cls=det_cls, elem=elem), want, tags_of


@gpu
def test_pack_hand_made_rows_and_null_groups(env):
    nat = env[1]
    a, want, tags_of = _hand_rows(nat)
    W = a["maneuver"].shape[1]
    ref = lambda **kw: R.pack(1, W, kw.get("maneuver"), kw.get("irows"), kw.get("isum"), kw.get("snap_n"), 64, kw.get("scene"),  # noqa: E731
                              kw.get("det_n"), kw.get("det_cls"), kw.get("elem"))
    rc, m, v = _pack(env, 1, W, **a)
    assert rc == 0 and _same((m, v), ref(**a))
    for f, tags in want.items():
        assert sorted(tags_of(m[0, f])) == sorted(tags), (f, tags_of(m[0, f]))
    assert (m[0] >> np.uint64(61) == 7).all() and not (m[0] & np.uint64(0x1FFE000000000000)).any()      # bits 49..60 stay zero
    assert v[0].tolist() == a["maneuver"]["speed_kmh"][0].tolist()
    # each input group absent in turn
    groups = dict(maneuver=("maneuver",), interaction=("irows", "isum", "snap_n"), scene=("scene", "det_n", "det_cls", "elem"),
                  detections=("det_n", "det_cls", "elem"))
    flag = dict(maneuver=R.HAS_MANEUVER, interaction=R.HAS_INTERACTION, scene=R.HAS_SCENE)
    for name, keys in groups.items():
        b = {k: x for k, x in a.items() if k not in keys}
        rc, m2, v2 = _pack(env, 1, W, **b)
        assert rc == 0 and _same((m2, v2), ref(**b)), name
        if name in flag:
            assert not ((m2[0] >> np.uint64(flag[name])) & np.uint64(1)).any(), name
            assert ((m2[0] >> np.uint64(61)) == (7 & ~(1 << (flag[name] - 61)))).all(), name
        assert np.isnan(v2).all() if name == "maneuver" else np.array_equal(v2, v), name
    only_scene = {k: a[k] for k in groups["scene"]}
    rc, m3, v3 = _pack(env, 1, W, **only_scene)
    assert rc == 0 and _same((m3, v3), ref(**only_scene)) and (m3[0] >> np.uint64(61) == 1).all()
    assert not (m3[0] & np.uint64(((1 << 49) - 1) & ~((1 << 18) - 1))).any()


# ---- (3) boundaries ------------------------------------------------------------------------------------------------------

ALL, ANY, NONE = 1 << 0, (1 << 1) | (1 << 2), 1 << 3
PRED = (ALL, ANY, NONE)


def _random_masks(rng, n):
    """Junk in every bit, the predicate's four bits biased so that matches come in runs."""
    m = rng.integers(0, 2 ** 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    m &= ~np.uint64(15)
    m |= (rng.random(n) < 0.93).astype(np.uint64) | ((rng.random(n) < 0.6).astype(np.uint64) << np.uint64(1))
    m |= ((rng.random(n) < 0.6).astype(np.uint64) << np.uint64(2)) | ((rng.random(n) < 0.06).astype(np.uint64) << np.uint64(3))
    return m


@gpu
def test_boundary_lengths(env):
    nat = env[1]
    CH = nat.TAGLOG_CHUNK
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 3 * CH - 1, 3 * CH, 3 * CH + 1]
    rng = np.random.default_rng(7)
    found = [0, 0]
    for k in range(0, len(lengths), 3):
        # capacities: just past the longest stream; the longest case also with the log exactly full and a chunk of slack behind it
        for cap in ([max(lengths[k:k + 3]) + 5] if k < 9 else [3 * CH + 1, 4 * CH + 7]):
            log = RawLog(env, 3, cap)
            masks = [_random_masks(rng, n) for n in lengths[k:k + 3]]
            speeds = [rng.uniform(0.0, 130.0, len(m)) for m in masks]
            log.load(masks, speeds)
            for first, last, md, small in ((0, cap, 5, 3), (0, cap, 1, None), (0, cap, 0, None), (10, 900, 2, 2), (-4, 2 ** 31 - 1, 3, None),
                                           (CH - 1, 2 * CH + 1, 2, None), (70, 70, 1, None), (80, 60, 1, None)):
                a, b = _check_queries(log, masks, PRED, first, last, md, small)
                found[0] += a
                found[1] += b
            _check_queries(log, masks, (0, 0, 0), 0, cap, 5, 0)              # every frame matches: one run; out_cap 0
            _check_stats(log, masks, speeds)
    print("boundary lengths: %d matches and %d segments compared" % tuple(found))
    assert found[0] > 5000 and found[1] > 500


def _runs(n, runs, on_bit=7):
    rng = np.random.default_rng(n + len(runs))
    m = rng.integers(0, 2 ** 62, n, dtype=np.uint64) & ~np.uint64(1 << on_bit)
    for a, b in runs:
        m[a:b + 1] |= np.uint64(1 << on_bit)
    return m


@gpu
def test_boundary_patterns(env):
    nat = env[1]
    CH, MD = nat.TAGLOG_CHUNK, 9
    n = 3 * CH + 130
    every, none_, alt = _runs(n, [(0, n - 1)]), _runs(n, []), _runs(n, [(i, i) for i in range(0, n, 2)])
    edges = _runs(n, [(0, 4), (60, 63), (65, 127), (128, 191), (250, 260), (CH - 4, CH - 1), (CH + 64, CH + 64 + MD - 1),
                      (2 * CH - 8, 2 * CH - 1), (2 * CH + 100, 2 * CH + 100 + MD - 2), (2 * CH + 191, 2 * CH + 192),
                      (3 * CH, 3 * CH + 7), (n - 10, n - 1)])
    starts = _runs(n, [(64, 70), (CH, CH + 6), (2 * CH, 2 * CH + MD - 1), (3 * CH - 1, 3 * CH), (n - 1, n - 1)])
    span = _runs(n, [(5, 9), (CH - 24, 3 * CH + 24)])                      # one run over chunks 0 .. 3
    masks = [every, none_, alt, edges, starts, span]
    log = RawLog(env, len(masks), n)                                        # the log is full: the last run ends on the last slot
    log.load(masks)
    p = (1 << 7, 0, 0)
    for md in (0, 1, 2, MD - 1, MD, MD + 1, n, n + 1):
        _check_queries(log, masks, p, 0, n, md, 4)
    for first, last in ((62, n - 5), (64, CH), (CH, 2 * CH), (CH - 2, 3 * CH + 3), (129, 190), (n - 1, n), (3 * CH + 24, n)):
        _check_queries(log, masks, p, first, last, 2, None)
    _check_queries(log, masks, (0, 0, 1 << 7), 0, n, MD, None)              # the complement: runs of frames WITHOUT the bit
    # the restatement itself on the cases by hand
    assert R.segments(edges, *p, min_duration=MD)[:3] == [(65, 191), (250, 260), (CH + 64, CH + 64 + MD - 1)]
    assert R.segments(span, *p, min_duration=6) == [(CH - 24, 3 * CH + 24)] and R.segments(every, *p, min_duration=n) == [(0, n - 1)]
    assert R.segments(edges, *p, min_duration=MD)[-1] == (n - 10, n - 1) and R.segments(every, *p, min_duration=n + 1) == []


@gpu
def test_append_past_capacity(env):
    torch = env[0]
    rng = np.random.default_rng(3)
    S, cap, W = 3, 100, 60
    log = RawLog(env, S, cap)
    refs = [R.Log(cap) for _ in range(S)]
    start = [0, 50, 95]
    first = rng.integers(1, 2 ** 63, (S, cap), dtype=np.uint64)
    for s in range(S):
        refs[s].append(first[s, :start[s]], np.arange(start[s]) * 1.5)
    log.load([first[s, :start[s]] for s in range(S)], [np.arange(start[s]) * 1.5 for s in range(S)])
    for _ in range(3):
        m, v = rng.integers(1, 2 ** 63, (S, W), dtype=np.uint64), rng.uniform(0, 100, (S, W))
        assert log.append(m, v) == 0
        for s in range(S):
            refs[s].append(m[s], v[s])
    torch.cuda.synchronize()
    assert log.log_n.cpu().tolist() == [cap] * 3 and log.dropped.cpu().tolist() == [r.dropped for r in refs] == [80, 130, 175]
    got_m, got_v = log.mask.cpu().numpy().view(np.uint64), log.speed.cpu().numpy()
    for s in range(S):
        assert got_m[s].tolist() == refs[s].masks and got_v[s].tolist() == refs[s].speeds, s


# ---- (4) HotLoop ----------------------------------------------------------------------------------------------------------

def _rows(nat, t, fields, shape):
    return t.cpu().numpy().view(np.dtype(fields)).reshape(shape)


@gpu
def test_hot_loop_tags(env):
    torch, nat = env[0], env[1]
    from multimodal_autonomous_driving_perception_and_planning_amd.harness import generate_ego_motion
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import tag_mask, tags_of
    S, W, STEPS = 2, 8, 5
    loop = HotLoop(S, window=W, fused_step=False)
    loop.reset(frame_offsets=[0, 17])
    with pytest.raises(RuntimeError):
        loop.enqueue_tags()
    log = loop.enable_tag_log(64)
    assert log is loop.tag_log
    z = np.stack([np.asarray(generate_ego_motion(STEPS * W, seed=s)) for s in range(S)])
    want_m, want_v = [], []
    for k in range(STEPS):
        loop.load_measurements(z[:, k * W:(k + 1) * W])
        loop.step()
        with torch.cuda.stream(loop.stream):
            loop.enqueue_maneuver()
            loop.enqueue_interactions()
            loop.enqueue_tags()
        loop.synchronize()
        m, v = R.pack(S, W, _rows(nat, loop.maneuver, nat.MANEUVER_ROW_FIELDS, (S, W)),
                      _rows(nat, loop.inter_rows, nat.INTERACTION_ROW_FIELDS, (S, W, 64)),
                      _rows(nat, loop.inter_summary, nat.INTERACTION_SUMMARY_FIELDS, (S, W)), loop.snap_n.cpu().numpy())
        want_m.append(m)
        want_v.append(v)
    want_m, want_v = np.concatenate(want_m, axis=1), np.concatenate(want_v, axis=1)
    assert log.lengths().tolist() == [40, 40] and log.dropped.cpu().tolist() == [0, 0]
    # the query tag: the longitudinal maneuver of the very first frame, so at least one frame carries it
    cruising, on = tag_mask([t for t in tags_of(want_m[0, 0]) if t in ("cruising", "accelerating", "braking", "hard_braking", "stopped")]), 0
    name = tags_of(cruising)[0]
    for s in range(S):
        assert log.masks(s).tolist() == want_m[s].tolist() and log.speeds(s).tolist() == want_v[s].tolist(), s
        assert ((want_m[s] >> np.uint64(61)) == 6).all()                    # maneuver and interaction rows, no scene
        assert log.search_by_tag(name, stream=s).tolist() == R.search(want_m[s], all_=cruising)
        assert [tuple(x) for x in log.get_event_segments(name, 3, stream=s).tolist()] == R.segments(want_m[s], all_=cruising, min_duration=3)
        assert log.search_masks(none=cruising, stream=s, first=3, last=30).tolist() == R.search(want_m[s], none=cruising, first=3, last=30)
        on += len(R.search(want_m[s], all_=cruising))
        st, ref = log.get_tag_statistics(s), R.stats(want_m[s], want_v[s])
        assert st["total_frames"] == 40 and st["speed_stats"]["min"] == ref["speed_min"] and st["speed_stats"]["max"] == ref["speed_max"]
    print("hot loop: %d of 80 frames carry %r; stream 0 statistics %r" % (on, name, log.get_tag_statistics(0)["tag_counts"]))
    assert 0 < on


# ---- (5) CameraLoop -------------------------------------------------------------------------------------------------------

def _spread_weights(seed):
    """Seeded random YOLOv8n parameters whose class confidences spread over (0, 1): the three 80 -> 80 1x1 class convolutions
    of the Detect head get weights x 30 and biases - 8 (plain random weights put every anchor within 1e-3 of the next)."""
    from oracle import yolo_ref as Y
    p = Y.random_params(seed).copy()
    pos = 0
    for cin, cout, k, _, bn in Y.conv_specs():
        nw = cout * cin * k * k
        if not bn and cout == Y.NC:
            p[pos:pos + nw] *= 30.0
            p[pos + nw:pos + nw + cout] -= 8.0
        pos += nw + (4 * cout if bn else cout)
    assert pos == p.size
    return p


@gpu
def test_camera_loop_tags(env, tmp_path):
    nat = env[1]
    from multimodal_autonomous_driving_perception_and_planning_amd.harness import generate_ego_motion
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import CameraLoop
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import element_table
    path = str(tmp_path / "spread.npy")
    np.save(path, _spread_weights(14))
    S, STEPS = 2, 3
    z = np.stack([np.asarray(generate_ego_motion(STEPS, seed=s)) for s in range(S)])
    logs = {}
    for tags in ("all", "motion"):
        loop = CameraLoop(S, h=720, w=1280, model=path, dcap=8, tracker_kw=dict(min_hits=1), tags=tags, tag_capacity=8)
        assert loop.tag_log is loop.hot.tag_log
        elem = element_table(loop.cam.yolo.names)
        for k in range(STEPS):
            loop.load_measurements(z[:, k:k + 1])
            loop.step(sync=True)
            hot, cam = loop.hot, loop.cam
            kw = dict(maneuver=_rows(nat, hot.maneuver, nat.MANEUVER_ROW_FIELDS, (S, 1)),
                      inter_rows=_rows(nat, hot.inter_rows, nat.INTERACTION_ROW_FIELDS, (S, 1, 64)),
                      inter_summary=_rows(nat, hot.inter_summary, nat.INTERACTION_SUMMARY_FIELDS, (S, 1)),
                      snap_n=hot.snap_n.cpu().numpy())
            if tags == "all":
                kw.update(scene=cam.scene_results().reshape(S, 1), det_n=cam.det_n.cpu().numpy().reshape(S, 1),
                          det_cls=cam.det_cls.cpu().numpy().reshape(S, 1, -1), elem_table=elem)
                # the scene stage saw the Kalman filter's speed of this step, read on the device
                assert np.array_equal(cam.scene_speed.cpu().numpy(), hot.vstate.cpu().numpy()[:, 0, 5])
            m, v = R.pack(S, 1, **kw)
            for s in range(S):
                assert int(loop.tag_log.masks(s)[k]) == int(m[s, 0]) and loop.tag_log.speeds(s)[k] == v[s, 0], (tags, k, s)
        assert loop.tag_log.lengths().tolist() == [STEPS] * S
        from multimodal_autonomous_driving_perception_and_planning_amd.tagging.tag_log import tags_of
        print("camera loop tags=%s, camera 0: %s" % (tags, [tags_of(x) for x in loop.tag_log.masks(0)]))
        logs[tags] = np.stack([loop.tag_log.masks(s) for s in range(S)])
    assert ((logs["all"] >> np.uint64(61)) == 7).all()
    assert ((logs["motion"] >> np.uint64(61)) == 6).all() and not (logs["motion"] & np.uint64((1 << 18) - 1)).any()
    assert (logs["all"] & np.uint64((1 << 6) - 1)).all()                    # a road type in every frame
    # the motion tags do not depend on the scene stage
    keep = np.uint64(((1 << 49) - 1) & ~((1 << 18) - 1))
    assert np.array_equal(logs["all"] & keep, logs["motion"] & keep)
    with pytest.raises(ValueError):
        CameraLoop(S, h=720, w=1280, model=path, tags="scene")


# ---- (6) argument checks ---------------------------------------------------------------------------------------------------

@gpu
def test_argument_checks(env):
    torch, nat, L, ctx = env
    S, W, cap = 2, 4, 16
    d = "cuda:0"
    i64 = lambda *sh: torch.full(sh, -3, dtype=torch.int64, device=d)          # noqa: E731
    i32 = lambda *sh: torch.full(sh, -3, dtype=torch.int32, device=d)          # noqa: E731
    f64 = lambda *sh: torch.full(sh, -3.0, dtype=torch.float64, device=d)      # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=d)                 # noqa: E731
    P = nat.ptr
    sh = nat.stream_handle()
    om, ov = i64(S, W), f64(S, W)
    man, rows, summ, scn = u8(S * W * 72), u8(S * W * 64 * 48), u8(S * W * 56), u8(S * W * 240)
    sn, dn, dc, el = i32(S, W), i32(S, W), i32(S, W, 8), u8(4)

    def pack(ctx_=ctx.handle, S_=S, W_=W, man_=man, rows_=rows, summ_=summ, sn_=sn, tcap=64, scn_=scn, dn_=dn, dc_=dc, md=8, el_=el,
             ne=4, om_=om, ov_=ov):
        return L.av_tags_pack(ctx_, sh, S_, W_, P(man_), P(rows_), P(summ_), P(sn_), tcap, P(scn_), P(dn_), P(dc_), md, P(el_), ne,
                              P(om_), P(ov_))
    bad = [pack(ctx_=None), pack(om_=None), pack(ov_=None), pack(S_=0), pack(W_=0), pack(S_=-1), pack(tcap=32), pack(tcap=128),
           pack(rows_=None), pack(summ_=None), pack(sn_=None), pack(dn_=None), pack(dc_=None), pack(el_=None), pack(scn_=None),
           pack(md=0), pack(ne=-1)]
    assert bad == [EINVAL] * len(bad) and b"av_tags_pack" in L.av_last_error_string()
    mask, speed, n, dr = i64(S, cap), f64(S, cap), i32(S), i32(S)
    ws = u8(int(L.av_taglog_workspace_bytes(S, cap)))
    assert L.av_taglog_workspace_bytes(0, cap) == 0 and L.av_taglog_workspace_bytes(S, 0) == 0

    def append(ctx_=ctx.handle, S_=S, W_=W, m=om, v=ov, cap_=cap, lm=mask, lv=speed, n_=n, dr_=dr):
        return L.av_taglog_append(ctx_, sh, S_, W_, P(m), P(v), cap_, P(lm), P(lv), P(n_), P(dr_))
    bad = [append(ctx_=None), append(m=None), append(v=None), append(lm=None), append(lv=None), append(n_=None), append(dr_=None),
           append(S_=0), append(W_=0), append(cap_=0), append(cap_=-5)]
    assert bad == [EINVAL] * len(bad) and b"av_taglog_append" in L.av_last_error_string()
    out, seg, on = i32(S, 4), i32(S, 4, 2), i32(S)

    def search(ctx_=ctx.handle, S_=S, cap_=cap, lm=mask, n_=n, ws_=ws, oc=4, out_=out, on_=on):
        return L.av_taglog_search(ctx_, sh, S_, cap_, P(lm), P(n_), 1, 0, 0, 0, cap, P(ws_), oc, P(out_), P(on_))

    def segments(ctx_=ctx.handle, S_=S, cap_=cap, lm=mask, n_=n, ws_=ws, oc=4, out_=seg, on_=on):
        return L.av_taglog_segments(ctx_, sh, S_, cap_, P(lm), P(n_), 1, 0, 0, 0, cap, 5, P(ws_), oc, P(out_), P(on_))
    for fn in (search, segments):
        bad = [fn(ctx_=None), fn(lm=None), fn(n_=None), fn(ws_=None), fn(out_=None), fn(on_=None), fn(S_=0), fn(cap_=0), fn(cap_=-1),
               fn(oc=-1)]
        assert bad == [EINVAL] * len(bad), fn.__name__
    st = u8(S * nat.TAGLOG_STATS_BYTES)

    def stats(ctx_=ctx.handle, S_=S, cap_=cap, lm=mask, lv=speed, n_=n, ws_=ws, st_=st):
        return L.av_taglog_stats(ctx_, sh, S_, cap_, P(lm), P(lv), P(n_), P(ws_), P(st_))
    bad = [stats(ctx_=None), stats(lm=None), stats(lv=None), stats(n_=None), stats(ws_=None), stats(st_=None), stats(S_=0), stats(cap_=0)]
    assert bad == [EINVAL] * len(bad) and b"av_taglog_stats" in L.av_last_error_string()
    torch.cuda.synchronize()
    # nothing was launched: every output still holds what it was filled with
    for t in (om, mask, n, dr, out, seg, on):
        assert (t == -3).all()
    assert (ov == -3.0).all() and (speed == -3.0).all() and not st.any()
