"""av_road_marks (include/avhot.h) restated in NumPy on the same state bytes: one vehicle, one frame per call.

Positions are float64 array operations, each rounded on its own (no FMA), in the header's order; everything behind the pixel
positions is integer work, so the device must agree bit for bit.  The runs are found the plain way, sample by sample, not the way
the device finds them on its 64-bit words.

Like tests/roadlanes_ref.py it reports the MARGINS of the decisions: step() returns {name: smallest distance}.
  half      a pre-floor tu or tv (u * 65536 + 0.5) from the nearest integer, over every tap of every camera with D > 0: where floor()
            could land on the neighbouring 1/65536 pixel, or a tap pass or fail the frame test (both tests are on floor()'s result)
  ends      an end tap's f from 0 and from max_range, and its D from 0
  nearest   the centre tap's d2 in the nearest seeing camera from the second nearest's
  extent    a sample's X from the boundary's x_min and x_max
  contrast  peak - bg from contrast - 1/2: the comparison is between integers, so its threshold lies between two of them and the
            distance is at least 1/2 -- no rounding of a double can flip it
  counts    n_seen, n_paint, longest_gap from their thresholds and 10 * sum_b from yellow_tenths * min(sum_g, sum_r), each from
            threshold - 1/2 in the same way
A case stands for an exact comparison when every margin is non-zero (smallest_margin)."""
import numpy as np

from tests import roadlanes_ref as lanes_ref

DEFAULT_CFG = dict(x_near=4.0, ds=0.1, dl=0.05, gap_solid=0.5, gap_dash=1.5, min_seen=8.0, min_paint=2.0, n_samples=210, core=5,
                   shoulder0=9, shoulder1=13, contrast=40, yellow_tenths=7, hold=3, forget=30)
CFG_DOUBLES = ("x_near", "ds", "dl", "gap_solid", "gap_dash", "min_seen", "min_paint")
CFG_INTS = ("n_samples", "core", "shoulder0", "shoulder1", "contrast", "yellow_tenths", "hold", "forget")
UNKNOWN, SOLID, DASHED = 0, 1, 2
WHITE, YELLOW = 1, 2
AMBIGUOUS = 1
MAXB, MAX_SAMPLES, PROFILE_WORDS = 8, 512, 16
RUN_CAP = 1 << 30

BOUND_DTYPE, LANES_DTYPE = lanes_ref.BOUND_DTYPE, lanes_ref.ROW_DTYPE
MARK_DTYPE = np.dtype([(k, "<i4") for k in ("type", "colour", "flags", "n_seen", "n_paint", "n_runs", "longest_gap", "n_gaps", "n_dashes",
                                            "contrast", "views", "reserved")] + [("dash_m", "<f8"), ("gap_m", "<f8")])
SIDE_DTYPE = np.dtype([(k, "<i4") for k in ("type", "colour", "observed", "observed_colour", "run", "bound")])
ROW_DTYPE = np.dtype([("left", SIDE_DTYPE), ("right", SIDE_DTYPE), ("may_change_left", "<i4"), ("may_change_right", "<i4"),
                      ("reserved", "<i4", (2,))])
SIDE_STATE_DTYPE = np.dtype([(k, "<i4") for k in ("type", "colour", "cand_type", "cand_colour", "run", "since")])
STATE_DTYPE = np.dtype([("left", SIDE_STATE_DTYPE), ("right", SIDE_STATE_DTYPE), ("frames", "<i4"), ("reserved", "<i4", (3,))])
assert (MARK_DTYPE.itemsize, ROW_DTYPE.itemsize, STATE_DTYPE.itemsize, SIDE_DTYPE.itemsize) == (64, 64, 64, 24)
MARK_INTS = MARK_DTYPE.names[:12]


def cfg_of(**kw):
    c = dict(DEFAULT_CFG)
    for k in kw:
        if k not in c:
            raise KeyError(k)
    c.update(kw)
    return c


def counts_of(cfg):
    """The header's count() of the four lengths -> dict(gap_solid_n, gap_dash_n, min_seen_n, min_paint_n)."""
    return {k + "_n": int(np.floor(cfg[k] / cfg["ds"] + 0.5)) for k in ("gap_solid", "gap_dash", "min_seen", "min_paint")}


def zero_state():
    return np.zeros((), STATE_DTYPE)


def warp_position(q, h, w, f, l):
    """ground_dev.h's warp_position on arrays -> (passes, tu, tv as int64 (0 where it fails), D, pre-floor tu, pre-floor tv)."""
    with np.errstate(all="ignore"):
        U, V, D = (q[0] * f + q[1] * l) + q[2], (q[3] * f + q[4] * l) + q[5], (q[6] * f + q[7] * l) + q[8]
        pos = D > 0.0
        Ds = np.where(pos, D, 1.0)
        u, v = U / Ds, V / Ds
        pu, pv = u * 65536.0 + 0.5, v * 65536.0 + 0.5
        tu, tv = np.floor(pu), np.floor(pv)
        ok = pos & (tu >= 0.0) & (tu <= float(w - 1) * 65536.0) & (tv >= 0.0) & (tv <= float(h - 1) * 65536.0)
    return ok, np.where(ok, tu, 0.0).astype(np.int64), np.where(ok, tv, 0.0).astype(np.int64), D, np.where(pos, pu, np.nan), np.where(pos, pv, np.nan)


def bilinear(img, tu, tv):
    """resample_dev.h's bilinear sample of img uint8 [h, w, 3] at int64 positions in 1/65536 pixel -> int64 [..., 3] (b, g, r)."""
    h, w = img.shape[:2]
    x0, wx, y0, wy = tu >> 16, tu & 65535, tv >> 16, tv & 65535
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    im = img.astype(np.int64)
    wx, wy = wx[..., None], wy[..., None]
    top = im[y0, x0] * (65536 - wx) + im[y0, x1] * wx
    bot = im[y1, x0] * (65536 - wx) + im[y1, x1] * wx
    return (top * (65536 - wy) + bot * wy + (1 << 31)) >> 32


def _dist(a, b=0.0):
    a = np.abs(np.asarray(a, np.float64) - b)
    a = a[np.isfinite(a)]
    return float(a.min()) if a.size else float("inf")


def boundary(cfg, grounds, mounts, frames, bd, margins):
    """One live boundary -> (av_road_mark scalar, seen bool [n], paint bool [n], runs [(first, one past last)])."""
    n, core, s0, s1 = cfg["n_samples"], cfg["core"], cfg["shoulder0"], cfg["shoulder1"]
    K, (h, w) = len(grounds), frames.shape[1:3]
    cn = counts_of(cfg)
    a0, a1, a2 = float(bd["a0"]), float(bd["a1"]), float(bd["a2"])
    with np.errstate(all="ignore"):
        X = cfg["x_near"] + (np.arange(n).astype(np.float64) + 0.5) * cfg["ds"]
        Yc = (a0 + a1 * X) + a2 * (X * X)
        J = np.arange(-s1, s1 + 1)
        Y = Yc[:, None] + J.astype(np.float64)[None, :] * cfg["dl"]
        best_k, best = np.full(n, -1), np.zeros(n)
        second = np.full(n, np.inf)
        taps = []
        for k in range(K):
            cs, sn, mx, my = (float(t) for t in mounts[k])
            q, max_range = np.asarray(grounds[k][0], np.float64), float(grounds[k][1])
            dx, dy = (X - mx)[:, None], Y - my
            f, l = cs * dx + sn * dy, cs * dy - sn * dx
            ok, tu, tv, D, pu, pv = warp_position(q, h, w, f, l)
            inr = (f >= 0.0) & (f <= max_range)
            sees = ok[:, 0] & ok[:, -1] & inr[:, 0] & inr[:, -1]
            # the header's claim: the frame is convex, so between two taps that pass every tap passes
            assert ok[sees].all(), "a tap between two passing end taps does not pass (camera %d)" % k
            margins["half"] = min(margins["half"], _dist(pu - np.rint(pu)), _dist(pv - np.rint(pv)))
            ends = np.stack([f[:, 0], f[:, -1]])
            margins["ends"] = min(margins["ends"], _dist(ends), _dist(ends, max_range), _dist(np.stack([D[:, 0], D[:, -1]])))
            d2 = f[:, s1] * f[:, s1] + l[:, s1] * l[:, s1]
            take = sees & ((best_k < 0) | (d2 < best))
            second = np.where(take, np.where(best_k >= 0, best, second), np.where(sees, np.minimum(second, d2), second))
            best, best_k = np.where(take, d2, best), np.where(take, k, best_k)
            taps.append((ok, tu, tv))
        seen = (best_k >= 0) & (X >= float(bd["x_min"])) & (X <= float(bd["x_max"]))
    margins["nearest"] = min(margins["nearest"], _dist((second - best)[best_k >= 0]))
    margins["extent"] = min(margins["extent"], _dist(X, float(bd["x_min"])), _dist(X, float(bd["x_max"])))
    # the taps of each sample in its own camera
    px = np.zeros((n, len(J), 3), np.int64)
    for k in range(K):
        ok, tu, tv = taps[k]
        mine = seen & (best_k == k)
        if mine.any():
            px[mine] = np.where(ok[mine][..., None], bilinear(frames[k], tu[mine], tv[mine]), 0)
    gray = (1868 * px[..., 0] + 9617 * px[..., 1] + 4899 * px[..., 2] + 8192) >> 14
    cj = np.abs(J) <= core
    sj = (np.abs(J) >= s0) & (np.abs(J) <= s1)
    pj = np.argmax(gray[:, cj], axis=1)                                      # the first of equals: the smallest j
    peak = gray[:, cj][np.arange(n), pj]
    ppx = px[:, cj][np.arange(n), pj]
    n_sh = int(sj.sum())
    assert n_sh == 2 * (s1 - s0 + 1)
    bg = (2 * gray[:, sj].sum(axis=1) + n_sh) // (2 * n_sh)
    paint = seen & (peak - bg >= cfg["contrast"])
    margins["contrast"] = min(margins["contrast"], _dist((peak - bg)[seen], cfg["contrast"] - 0.5))
    sum_b, sum_g, sum_r = (int(ppx[paint, c].sum()) for c in range(3))
    sum_c = int((peak - bg)[paint].sum())
    views = 0
    for k in np.unique(best_k[seen]):
        views |= 1 << int(k)
    # ---- the runs, sample by sample ----
    runs, i = [], 0
    while i < n:
        if paint[i]:
            e = i
            while e < n and paint[e]:
                e += 1
            runs.append((i, e))
            i = e
        else:
            i += 1
    gaps = [b[0] - a[1] for a, b in zip(runs, runs[1:]) if seen[a[1]:b[0]].all()]
    dashes = [e - s for s, e in runs if s > 0 and seen[s - 1] and e < n and seen[e]]
    n_seen, n_paint, longest = int(seen.sum()), int(paint.sum()), max(gaps, default=0)
    m = np.zeros((), MARK_DTYPE)
    if n_seen >= cn["min_seen_n"] and n_paint >= cn["min_paint_n"]:
        if longest < cn["gap_solid_n"]:
            m["type"] = SOLID
        elif len(runs) >= 2 and longest >= cn["gap_dash_n"]:
            m["type"] = DASHED
        else:
            m["flags"] = AMBIGUOUS
    lim = cfg["yellow_tenths"] * min(sum_g, sum_r)
    if m["type"] != UNKNOWN:
        m["colour"] = YELLOW if 10 * sum_b < lim else WHITE
    margins["counts"] = min(margins["counts"], abs(n_seen - (cn["min_seen_n"] - 0.5)), abs(n_paint - (cn["min_paint_n"] - 0.5)),
                            abs(longest - (cn["gap_solid_n"] - 0.5)), abs(longest - (cn["gap_dash_n"] - 0.5)), abs(10 * sum_b - (lim - 0.5)))
    m["n_seen"], m["n_paint"], m["n_runs"], m["longest_gap"], m["n_gaps"], m["n_dashes"] = n_seen, n_paint, len(runs), longest, len(gaps), len(dashes)
    m["contrast"] = (2 * sum_c + n_paint) // (2 * n_paint) if n_paint else 0
    m["views"] = views
    m["dash_m"] = (float(sum(dashes)) / float(len(dashes))) * cfg["ds"] if dashes else 0.0
    m["gap_m"] = (float(sum(gaps)) / float(len(gaps))) * cfg["ds"] if gaps else 0.0
    return m, seen, paint, runs


def pack_bits(bits):
    """bool [n] -> uint32 [16]: sample i in bit i & 31 of word i >> 5."""
    full = np.zeros(MAX_SAMPLES, np.uint64)
    full[:len(bits)] = bits
    return (full.reshape(PROFILE_WORDS, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def side_step(s, typ, colour, hold, forget):
    if typ != UNKNOWN:
        s["since"] = 0
        if typ == s["cand_type"] and colour == s["cand_colour"]:
            s["run"] = min(int(s["run"]) + 1, RUN_CAP)
        else:
            s["cand_type"], s["cand_colour"], s["run"] = typ, colour, 1
        if s["run"] >= hold:
            s["type"], s["colour"] = s["cand_type"], s["cand_colour"]
    else:
        s["since"] = min(int(s["since"]) + 1, RUN_CAP)
        if s["since"] >= forget:
            s[()] = np.zeros((), SIDE_STATE_DTYPE)


def may_change(typ):
    return 1 if typ == DASHED else 0 if typ == SOLID else -1


def step(cfg, grounds, mounts, frames, bounds, lanes, state):
    """One frame of one vehicle.  grounds: [(ginv [9], max_range)] per camera; mounts [K, 4] (cos, sin, x, y); frames uint8
    [K, h, w, 3]; bounds BOUND_DTYPE [8]; lanes a LANES_DTYPE scalar; state a STATE_DTYPE scalar (not changed).
    -> dict(marks MARK_DTYPE [8], sides ROW_DTYPE scalar, state, profile uint32 [8, 2, 16], runs [per live boundary], margins)."""
    margins = dict(half=np.inf, ends=np.inf, nearest=np.inf, extent=np.inf, contrast=np.inf, counts=np.inf)
    nb = min(max(int(lanes["n_bounds"]), 0), MAXB)
    marks, profile, runs = np.zeros(MAXB, MARK_DTYPE), np.zeros((MAXB, 2, PROFILE_WORDS), np.uint32), []
    for b in range(nb):
        marks[b], seen, paint, r = boundary(cfg, grounds, mounts, frames, bounds[b], margins)
        profile[b, 0], profile[b, 1] = pack_bits(seen), pack_bits(paint)
        runs.append(r)
    st = np.array(state, STATE_DTYPE).copy()
    status = int(lanes["status"])
    if status & lanes_ref.CHANGE_LEFT:
        st["right"], st["left"] = st["left"].copy(), np.zeros((), SIDE_STATE_DTYPE)
    elif status & lanes_ref.CHANGE_RIGHT:
        st["left"], st["right"] = st["right"].copy(), np.zeros((), SIDE_STATE_DTYPE)
    row = np.zeros((), ROW_DTYPE)
    for side, flag in (("left", lanes_ref.BOUND_LEFT), ("right", lanes_ref.BOUND_RIGHT)):
        bi = next((b for b in range(nb) if int(bounds[b]["flags"]) & flag), -1)
        o = row[side]
        o["bound"] = bi
        if bi >= 0:
            o["observed"], o["observed_colour"] = marks[bi]["type"], marks[bi]["colour"]
        side_step(st[side], int(o["observed"]), int(o["observed_colour"]), cfg["hold"], cfg["forget"])
        o["type"], o["colour"], o["run"] = st[side]["type"], st[side]["colour"], st[side]["run"]
    st["frames"] += 1
    row["may_change_left"], row["may_change_right"] = may_change(int(st["left"]["type"])), may_change(int(st["right"]["type"]))
    return dict(marks=marks, sides=row, state=st, profile=profile, runs=runs, margins=margins)


def smallest_margin(margins):
    """-> (the smallest distance, its name)."""
    name = min(margins, key=lambda k: margins[k])
    return float(margins[name]), name
