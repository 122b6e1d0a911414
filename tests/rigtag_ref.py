"""Restatement of the rig's class lanes (av_track_obstacles_ground_cls, av_rig_fuse_cls, av_rig_track_cls) and of the rig tagger
(av_rig_interact) in plain NumPy / Python loops on the library's byte layouts (include/avhot.h): float64, every operation rounded on
its own, in the header's order.  The fuse's class lane restates the association itself; tests/rig_ref.py and tests/rigtrack_ref.py
are imported only to cross-check positions and to say which row went to which track."""
import math

import numpy as np

from tests import rigtrack_ref as tr

f8 = np.float64
HALF_PI = 1.5707963267948966
RING = 30
HDR_BYTES, SLOT_BYTES = 16, 248
SLOT = np.dtype([("id", "<i4"), ("cnt", "<i4"), ("lat", "<f8", (RING,))])
assert SLOT.itemsize == SLOT_BYTES
ROW = np.dtype([("type", "<i4"), ("risk", "<i4"), ("agent_id", "<i4"), ("cls", "<i4"), ("confidence", "<f8"), ("distance", "<f8"),
                ("relative_speed", "<f8"), ("ttc", "<f8")])
SUMMARY = np.dtype([("agent_count", "<i4"), ("pedestrian_count", "<i4"), ("cyclist_count", "<i4"), ("vehicle_count", "<i4"),
                    ("n_interactions", "<i4"), ("primary_type", "<i4"), ("overall_risk", "<i4"), ("primary_row", "<i4"),
                    ("closest_distance", "<f8"), ("min_ttc", "<f8"), ("timestamp", "<f8")])
assert ROW.itemsize == 48 and SUMMARY.itemsize == 56
# InteractionType / RiskLevel indices (the reference's Enum definition order)
FOLLOWING, BEING_FOLLOWED, CUT_IN, CUT_OUT, PED_CROSSING, PED_WAITING, CYCLIST, NEAR_MISS, PASSING, BEING_PASSED = 1, 2, 4, 5, 6, 7, 8, 9, 11, 12
LOW, MEDIUM, HIGH, CRITICAL = 0, 1, 2, 3
DEFAULTS = dict(dt=1.0 / 30.0, corridor_half=1.75, adjacent_half=5.25, alongside=10.0, pass_speed=1.0, min_hits=3)
KINDS = (0, 1, 2, 3, 4) + (0,) * 11              # class id -> kind when the tracks carry the category itself


def cfg(**over):
    c = dict(DEFAULTS, class_kind=KINDS)
    assert not set(over) - set(c), over
    c.update(over)
    return c


# ---- class lanes ----------------------------------------------------------------------------------------------------------------

def ground_cls(rows, n_rows, kept):
    """The class lane of one state's obstacle list: kept = the indices of the tracker rows that became obstacles, in order."""
    assert all(0 <= i < n_rows for i in kept) and list(kept) == sorted(kept)
    return np.array([rows["cls"][i] for i in kept], np.int32)


def fuse_cls(cam_obs, cam_n, cam_cls, mounts, merge_scale=1.0, merge_min=1.0):
    """One vehicle: cam_obs [K][ocap_in][ncol], cam_n [K], cam_cls [K][ocap_in], mounts [K][4] -> dict(cls [M], XY [M][2] (the
    clusters in the vehicle frame), w_margin (the smallest relative distance between a candidate's weight and the best weight of the
    cluster that absorbs it, exact ties excluded), n_ties (absorptions at exactly the best weight))."""
    cam_obs = np.asarray(cam_obs, f8)
    K, ocap_in, ncol = cam_obs.shape
    ms, mm = f8(merge_scale), f8(merge_min)
    cl = []
    w_margin, n_ties = math.inf, 0
    with np.errstate(all="ignore"):
        for k in range(K):
            c, s, mx, my = (f8(t) for t in mounts[k])
            cand = []
            for j in range(min(max(int(cam_n[k]), 0), ocap_in)):
                row = cam_obs[k, j]
                if not (np.isfinite(row).all() and row[2] > 0.0):
                    continue
                x, y = row[0], row[1]
                m = max(x * x + y * y, f8(1.0))
                cand.append(dict(w=f8(1.0) / (m * m), X=(mx + c * x) - s * y, Y=(my + s * x) + c * y, r=row[2], cls=int(cam_cls[k][j])))
            m0 = len(cl)
            pairs = []
            for i in range(m0):
                for j, q in enumerate(cand):
                    dx, dy = cl[i]["X"] - q["X"], cl[i]["Y"] - q["Y"]
                    d2 = dx * dx + dy * dy
                    gate = max(mm, ms * max(cl[i]["r"], q["r"]))
                    if np.isfinite(d2) and d2 <= gate * gate:
                        pairs.append((d2, i, j))
            pairs.sort()
            ti, tj, match = set(), set(), {}
            for d2, i, j in pairs:                      # the smallest d2 first, then the smallest i, then the smallest j
                if i not in ti and j not in tj:
                    ti.add(i), tj.add(j)
                    match[j] = i
            for j, q in enumerate(cand):
                if j in match:
                    t = cl[match[j]]
                    if q["w"] == t["best_w"]:
                        n_ties += 1
                    else:
                        w_margin = min(w_margin, abs(float(q["w"] - t["best_w"])) / float(max(q["w"], t["best_w"])))
                    if q["w"] > t["best_w"]:
                        t["best_w"], t["cls"] = q["w"], q["cls"]
                    t["sw"] = t["sw"] + q["w"]
                    t["sx"], t["sy"] = t["sx"] + q["w"] * q["X"], t["sy"] + q["w"] * q["Y"]
                    t["r"] = max(t["r"], q["r"])
                    t["X"], t["Y"] = t["sx"] / t["sw"], t["sy"] / t["sw"]
            for j, q in enumerate(cand):
                if j not in match:
                    cl.append(dict(X=q["X"], Y=q["Y"], r=q["r"], sw=q["w"], sx=q["w"] * q["X"], sy=q["w"] * q["Y"], best_w=q["w"],
                                   cls=q["cls"]))
    return dict(cls=np.array([t["cls"] for t in cl], np.int32), XY=np.array([[t["X"], t["Y"]] for t in cl], f8).reshape(len(cl), 2),
                w_margin=w_margin, n_ties=n_ties)


def track_cls(before, step, cls_in):
    """The class words of one vehicle after a frame.  before: the state bytes before it, step: rigtrack_ref.step's result for it,
    cls_in [ocap_in] or None -> (cls1 [tcap] (the slots' first reserved word), cls_out [M])."""
    old, new = tr.views_of(np.array(before, np.uint8, copy=True))[1], tr.views_of(step["state"])[1]
    tcap = len(new)
    cls1 = np.array(old["reserved"][:, 0], np.int64)
    row_of = {int(i): j for j, i in enumerate(step["match"]) if i > 0}             # id -> the row that went to it
    for t in range(tcap):
        was, now = int(old["id"][t]), int(new["id"][t])
        if was >= 0 and now != was:
            cls1[t] = 0                                                  # freed in this frame: a newborn inherits nothing
        if now < 0 or cls_in is None:
            continue                                                     # (without a class lane the word is carried)
        c = int(cls_in[row_of[now]]) if now in row_of else -1
        if now != was:
            cls1[t] = c + 1 if c >= 0 else 0                             # a birth
        elif c >= 0:
            cls1[t] = c + 1                                              # the latest classified observation wins
    return cls1.astype(np.int32), np.array([cls1[t] - 1 for t in step["obs_slot"]], np.int32)


# ---- the tagger -----------------------------------------------------------------------------------------------------------------

def state_bytes(tcap):
    return HDR_BYTES + SLOT_BYTES * tcap


def views_of(st):
    """(frames int64 [2], slots structured [tcap]) as views of one vehicle's state bytes."""
    return st[:HDR_BYTES].view(np.int64), st[HDR_BYTES:].view(SLOT)


def reset_state(tcap):
    st = np.zeros(state_bytes(tcap), np.uint8)
    views_of(st)[1]["id"] = -1
    return st


def quantities(slot, plan_state):
    """The header's per-agent quantities for one tracker slot: dict(X, Y, RVX, d, closing, ttc (None: none))."""
    x0, y0, h, v0 = (f8(t) for t in plan_state)
    cs, sn, c2, s2 = np.cos(h), np.sin(h), np.cos(h + f8(HALF_PI)), np.sin(h + f8(HALF_PI))
    x, y, vx, vy = (f8(t) for t in slot["x"])
    ex, ey = x - x0, y - y0
    X, Y = ex * cs + ey * sn, ex * c2 + ey * s2
    rvx, rvy = vx - v0 * cs, vy - v0 * sn
    RVX = rvx * cs + rvy * sn
    d = np.sqrt(ex * ex + ey * ey)
    closing = -((ex * rvx + ey * rvy) / d) if d > 0.0 else f8(0.0)
    return dict(X=X, Y=Y, RVX=RVX, d=d, closing=closing, ttc=d / closing if closing > 0.1 else None)


def interact(track_state, plan_state, state, c):
    """One frame of one vehicle.  track_state: the tracker's bytes (read), state: the tagger's bytes (left as they are) ->
    dict(state (the new bytes), rows ROW [tcap], summary SUMMARY [1], facts (per agent slot: the quantities, hl, Y0, kind))."""
    slots = tr.views_of(np.array(track_state, np.uint8, copy=True))[1]
    st = np.array(state, np.uint8, copy=True)
    hdr, ring = views_of(st)
    tcap = len(slots)
    assert len(ring) == tcap
    rows = np.zeros(tcap, ROW)
    rows["type"], rows["agent_id"], rows["cls"], rows["ttc"] = -1, -1, -1, np.nan
    ch, ah, al, ps = f8(c["corridor_half"]), f8(c["adjacent_half"]), f8(c["alongside"]), f8(c["pass_speed"])
    facts = {}
    sm = np.zeros(1, SUMMARY)
    s = sm[0]
    dists, ttcs = [], []
    with np.errstate(all="ignore"):
        for t in range(tcap):
            sl = slots[t]
            if not (sl["id"] >= 0 and sl["hits"] >= c["min_hits"]):
                continue
            q = quantities(sl, plan_state)
            X, Y, RVX, d, closing, ttc = q["X"], q["Y"], q["RVX"], q["d"], q["closing"], q["ttc"]
            cnt = int(ring["cnt"][t]) if ring["id"][t] == sl["id"] else 0
            ring["lat"][t][cnt % RING] = Y
            cnt += 1
            ring["id"][t], ring["cnt"][t] = sl["id"], cnt
            hl = min(cnt, RING)
            Y0 = ring["lat"][t][0] if cnt <= RING else ring["lat"][t][cnt % RING]
            cls1 = int(sl["reserved"][0])
            kind = c["class_kind"][cls1 - 1] if 1 <= cls1 <= 16 else 0
            ahead, in_path = X > 0.0, abs(Y) < ch
            beside = (not in_path) and abs(Y) < ah
            typ, conf, risk, rel, o_ttc = -1, 0.0, LOW, closing, ttc
            soon = ttc is not None and ttc < 3.0
            if d < 3.0:
                typ, conf, risk = NEAR_MISS, 0.9, CRITICAL
            elif kind == 1 and d < 10.0:
                if ahead and in_path:
                    typ, conf, risk = PED_CROSSING, 0.8, HIGH if d < 8.0 else MEDIUM
                else:
                    typ, conf, risk, rel, o_ttc = PED_WAITING, 0.6, LOW, 0.0, None
            elif kind == 2 and d < 15.0:
                typ, conf, risk, o_ttc = CYCLIST, 0.7, MEDIUM if d < 8.0 else LOW, None
            elif kind == 3:
                turn = hl >= 10 and d < 15.0 and ahead
                follow = in_path and 5.0 < d < 30.0
                along = beside and abs(X) < al
                if turn and in_path and abs(Y0) >= ch:
                    typ, conf, risk = CUT_IN, 0.7, MEDIUM
                elif turn and not in_path and abs(Y0) < ch:
                    typ, conf, risk = CUT_OUT, 0.7, LOW
                elif follow and ahead:
                    typ, conf, risk = FOLLOWING, 0.75, HIGH if soon else (MEDIUM if d < 10.0 else LOW)
                elif follow:
                    typ, conf, risk = BEING_FOLLOWED, 0.75, HIGH if soon else LOW
                elif along and RVX < -ps:
                    typ, conf, risk = PASSING, 0.7, LOW
                elif along and RVX > ps:
                    typ, conf, risk = BEING_PASSED, 0.7, LOW
            r = rows[t]
            r["type"], r["risk"], r["agent_id"], r["cls"], r["confidence"], r["distance"] = typ, risk, sl["id"], cls1 - 1, conf, d
            r["relative_speed"] = rel if typ >= 0 else 0.0
            r["ttc"] = o_ttc if (typ >= 0 and o_ttc is not None) else np.nan
            facts[t] = dict(q, hl=hl, Y0=Y0, kind=kind, type=typ)
            s["agent_count"] += 1
            s["pedestrian_count"] += kind == 1
            s["cyclist_count"] += kind == 2
            s["vehicle_count"] += kind in (3, 4)
            dists.append(d)
            if ttc is not None:
                ttcs.append(ttc)
    hit = [t for t in range(tcap) if rows["type"][t] >= 0]
    s["n_interactions"] = len(hit)
    s["closest_distance"] = min(dists) if dists else np.inf
    s["min_ttc"] = min(ttcs) if ttcs else np.nan
    s["primary_type"] = s["primary_row"] = -1
    if hit:
        p = min(hit, key=lambda t: (-int(rows["risk"][t]), -float(rows["confidence"][t]), t))
        s["primary_row"], s["primary_type"] = p, rows["type"][p]
        s["overall_risk"] = CRITICAL if (ttcs and min(ttcs) < 1.5) else max(int(rows["risk"][t]) for t in hit)
    s["timestamp"] = f8(int(hdr[0])) * f8(c["dt"])
    hdr[0] += 1
    return dict(state=st, rows=rows, summary=sm, facts=facts)


THRESHOLDS = dict(d=(3.0, 5.0, 8.0, 10.0, 15.0, 30.0), closing=(0.1,), ttc=(1.5, 3.0))


def margin(facts, c):
    """The smallest relative distance of an agent's quantity from a threshold it is compared with, exact hits excluded; and the
    number of exact hits: (margin, n_exact)."""
    best, exact = math.inf, 0

    def see(v, th):
        nonlocal best, exact
        v, th = float(v), float(th)
        if v == th:
            exact += 1
        else:
            best = min(best, abs(v - th) / max(abs(v), abs(th)))
    for q in facts.values():
        for th in THRESHOLDS["d"]:
            see(q["d"], th)
        for v in (abs(q["Y"]), abs(q["Y0"])):
            see(v, c["corridor_half"]), see(v, c["adjacent_half"])
        see(abs(q["X"]), c["alongside"])
        see(q["RVX"], c["pass_speed"]), see(q["RVX"], -c["pass_speed"])
        see(q["closing"], 0.1)
        if q["ttc"] is not None:
            see(q["ttc"], 1.5), see(q["ttc"], 3.0)
    return best, exact
