"""av_rig_fuse (include/avhot.h) restated in NumPy: a loop over cameras, match iterations and candidates, as the header writes it.

Every arithmetic step is one float64 operation (NumPy scalars and element-wise arrays: no fused multiply-add), in the header's
order.  Besides the result, fuse() reports how close the discrete decisions of its input came to their thresholds:

  gate_margin   the smallest |d2 - gate^2| / max(d2, gate^2) over every cluster x candidate pair it compared
  tie_margin    the smallest (runner-up d2 - winning d2) / runner-up d2 over the match iterations that had a runner-up

A test on random inputs first asserts both >= MARGIN: a few ulp of difference between two correct implementations then cannot
change a decision.  Hand-made exact ties (integer coordinates, mounts written as (1, 0, ., .) and (0, 1, ., .)) are exempt: their
arithmetic is exact.
"""
import math

import numpy as np

MARGIN = 1e-6
HALF_PI = 1.5707963267948966
f8 = np.float64


def mount(yaw, x=0.0, y=0.0):
    """(cos, sin, x, y) of a mount, as perception.CameraRig.mounts_table writes it."""
    return (math.cos(yaw), math.sin(yaw), float(x), float(y))


IDENTITY = (1.0, 0.0, 0.0, 0.0)


def fuse(cam_obs, cam_n, mounts, plan_state, merge_scale=1.0, merge_min=1.0):
    """One vehicle.  cam_obs [K][ocap_in][ncol], cam_n [K], mounts [K][4] (c, s, x, y), plan_state [4] ->
    dict(obstacles [M][ncol], views [M], n_skip, XY [M][2] (vehicle frame), members [M], gate_margin, tie_margin)."""
    cam_obs = np.asarray(cam_obs, f8)
    K, ocap_in, ncol = cam_obs.shape
    moving = ncol == 5
    ms, mm = f8(merge_scale), f8(merge_min)
    cl = []                      # clusters: dict(X, Y, VX, VY, r, sw, sx, sy, svx, svy, views, members)
    n_skip = 0
    gate_margin = tie_margin = math.inf
    with np.errstate(all="ignore"):
        for k in range(K):
            c, s, mx, my = (f8(t) for t in mounts[k])
            n = min(max(int(cam_n[k]), 0), ocap_in)
            cand = []
            for row in cam_obs[k, :n]:
                x, y, r = row[0], row[1], row[2]
                ok = np.isfinite(x) and np.isfinite(y) and np.isfinite(r) and r > 0.0
                vx = vy = f8(0.0)
                if moving:
                    vx, vy = row[3], row[4]
                    ok = ok and np.isfinite(vx) and np.isfinite(vy)
                if not ok:
                    n_skip += 1
                    continue
                m = max(x * x + y * y, f8(1.0))
                w = f8(1.0) / (m * m)
                cand.append(dict(w=w, X=(mx + c * x) - s * y, Y=(my + s * x) + c * y, VX=c * vx - s * vy, VY=s * vx + c * vy, r=r))
            m0, nc = len(cl), len(cand)
            match = [-1] * nc
            if m0 and nc:
                cX, cY, cr = (np.array([q[t] for q in cl], f8)[:, None] for t in ("X", "Y", "r"))
                aX, aY, ar = (np.array([q[t] for q in cand], f8)[None, :] for t in ("X", "Y", "r"))
                dx, dy = cX - aX, cY - aY
                d2 = dx * dx + dy * dy
                gate = np.maximum(mm, ms * np.maximum(cr, ar))
                g2 = gate * gate
                den = np.maximum(d2, g2)
                rel = np.where(den > 0.0, np.abs(d2 - g2) / np.where(den > 0.0, den, 1.0), 0.0)
                gate_margin = min(gate_margin, float(rel.min()))
                free = (d2 <= g2) & np.isfinite(d2)              # admissible, and not yet taken
                while free.any():
                    vals = np.sort(d2[free])
                    best = vals[0]
                    if len(vals) > 1:
                        tie_margin = min(tie_margin, float((vals[1] - best) / vals[1]) if vals[1] > 0.0 else 0.0)
                    i, j = np.argwhere(free & (d2 == best))[0]   # row-major: the smallest i, then the smallest j
                    match[j] = int(i)
                    free[i, :] = False
                    free[:, j] = False
            for j, q in enumerate(cand):
                w = q["w"]
                if match[j] >= 0:
                    t = cl[match[j]]
                    t["sw"] = t["sw"] + w
                    t["sx"], t["sy"] = t["sx"] + w * q["X"], t["sy"] + w * q["Y"]
                    t["svx"], t["svy"] = t["svx"] + w * q["VX"], t["svy"] + w * q["VY"]
                    t["r"] = max(t["r"], q["r"])
                    t["views"] |= 1 << k
                    t["members"] += 1
                    t["X"], t["Y"] = t["sx"] / t["sw"], t["sy"] / t["sw"]
                    t["VX"], t["VY"] = t["svx"] / t["sw"], t["svy"] / t["sw"]
            for j, q in enumerate(cand):
                if match[j] < 0:
                    w = q["w"]
                    cl.append(dict(X=q["X"], Y=q["Y"], VX=q["VX"], VY=q["VY"], r=q["r"], sw=w, sx=w * q["X"], sy=w * q["Y"],
                                   svx=w * q["VX"], svy=w * q["VY"], views=1 << k, members=1))
        x0, y0, h, v0 = (f8(t) for t in plan_state)
        cs, sn, c2, s2 = np.cos(h), np.sin(h), np.cos(h + f8(HALF_PI)), np.sin(h + f8(HALF_PI))
        out = np.zeros((len(cl), ncol), f8)
        for i, t in enumerate(cl):
            out[i, 0] = (x0 + t["X"] * cs) + t["Y"] * c2
            out[i, 1] = (y0 + t["X"] * sn) + t["Y"] * s2
            out[i, 2] = t["r"]
            if moving:
                vf = t["VX"] + v0
                out[i, 3] = vf * cs + t["VY"] * c2
                out[i, 4] = vf * sn + t["VY"] * s2
    return dict(obstacles=out, views=np.array([t["views"] for t in cl], np.int32), n_skip=n_skip,
                XY=np.array([[t["X"], t["Y"]] for t in cl], f8).reshape(len(cl), 2),
                members=np.array([t["members"] for t in cl], np.int32), gate_margin=gate_margin, tie_margin=tie_margin)


def fuse_all(cam_obs, cam_n, mounts, plan_state, merge_scale=1.0, merge_min=1.0):
    """V vehicles: cam_obs [V*K][ocap_in][ncol], cam_n [V*K], mounts [V][K][4], plan_state [V][4] -> a list of fuse()'s results."""
    mounts = np.asarray(mounts, f8)
    V, K = mounts.shape[:2]
    cam_obs, cam_n = np.asarray(cam_obs, f8), np.asarray(cam_n)
    return [fuse(cam_obs[v * K:(v + 1) * K], cam_n[v * K:(v + 1) * K], mounts[v], plan_state[v], merge_scale, merge_min)
            for v in range(V)]


def margins(results):
    return min(r["gate_margin"] for r in results), min(r["tie_margin"] for r in results)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------

RADII = (0.5, 0.75, 1.0, 1.5, 2.0, 2.5)
FOUR_MOUNTS = [mount(0.0, 1.8, 0.0), mount(math.pi / 2, 0.5, 0.9), mount(-math.pi / 2, 0.5, -0.9), mount(math.pi, -1.0, 0.0)]


def pack(lists, ocap_in, ncol):
    """Per-camera row lists -> (cam_obs [len][ocap_in][ncol] with NaN behind each list, cam_n)."""
    obs = np.full((len(lists), ocap_in, ncol), np.nan, f8)
    n = np.zeros(len(lists), np.int32)
    for k, rows in enumerate(lists):
        rows = np.asarray(rows, f8).reshape(-1, ncol)
        obs[k, :len(rows)] = rows
        n[k] = len(rows)
    return obs, n


def scene(seed, mounts, n_objects, ncol, ocap_in=64, half_fov=math.radians(65.0), max_range=45.0, spacing=7.0, extent=40.0,
          noise=4.0e-4):
    """n_objects discs scattered around a vehicle at least `spacing` metres apart, each seen by every camera that has it within
    half_fov of its axis and within max_range, at a position off by noise * range^2 metres (a pixel's footprint), rows shuffled
    per camera.  -> (per-camera row lists, the objects [n][ncol])."""
    rng = np.random.default_rng(seed)
    objs = []
    while len(objs) < n_objects:
        p = rng.uniform(-extent, extent, 2)
        if np.hypot(*p) > 3.0 and all(np.hypot(*(p - q[:2])) >= spacing for q in objs):
            objs.append(np.concatenate([p, [RADII[rng.integers(len(RADII))]], rng.uniform(-8.0, 8.0, 2)]))
    objs = np.array(objs)
    lists = []
    for c, s, mx, my in mounts:
        rows = []
        for o in objs:
            dx, dy = o[0] - mx, o[1] - my
            x, y = c * dx + s * dy, -s * dx + c * dy             # the vehicle frame -> the camera's road frame
            rng_ = math.hypot(x, y)
            if x <= 0.5 or abs(math.atan2(y, x)) > half_fov or rng_ > max_range or len(rows) >= ocap_in:
                continue
            e = rng.normal(0.0, noise * rng_ * rng_, 2)
            vx, vy = c * o[3] + s * o[4], -s * o[3] + c * o[4]
            rows.append([x + e[0], y + e[1], o[2], vx + rng.normal(0.0, 0.05), vy + rng.normal(0.0, 0.05)][:ncol])
        rows = [rows[i] for i in rng.permutation(len(rows))]
        lists.append(rows)
    return lists, objs[:, :ncol]


def crowd(seed, n_cams, ocap_in, ncol, radius=3.0, spread=0.4):
    """The matching loop's worst case: every row of every camera within one gate of every other (n_cams x ocap_in points inside a
    disc of `spread` metres, gate = `radius`), identity mounts."""
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(n_cams):
        p = np.array([12.0, -1.0]) + rng.uniform(-spread, spread, (ocap_in, 2)) / math.sqrt(2.0)
        rows = np.concatenate([p, np.full((ocap_in, 1), radius), rng.uniform(-3.0, 3.0, (ocap_in, 2))], axis=1)
        lists.append(rows[:, :ncol])
    return lists
