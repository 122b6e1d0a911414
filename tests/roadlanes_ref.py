"""av_road_lanes (include/avhot.h) restated as a NumPy / plain-float loop on the same state bytes: one vehicle, one frame per call.

Every operation is a Python float operation (IEEE double, rounded on its own, no FMA) in the header's order, and the sums follow
the device's order -- per lane (row index & 63) in ascending row order, the wave's tree of adjacent pairs, then the cameras in the
order k = 0 .. K - 1 -- so the doubles agree with the device to the last bits of sqrt, atan, sin and cos.

Like tests/rig_ref.py it reports the MARGINS of every decision a last-bit difference could flip: step() returns them as
{name: [distance, ...]} in the units of the quantity compared (metres, slopes, bins of votes).  A case is fit for an exact integer
comparison when every margin it does not exempt by name is >= 1e-6."""
import math

import numpy as np

DEFAULT_CFG = dict(min_len=0.5, slope_max=0.5, vote_len=0.25, x_vote=15.0, slope_tol=0.15, y_max=8.0, min_sep=2.0, gate=0.4,
                   span_quad=10.0, w_min=2.5, w_max=5.0, default_width=3.5, alpha=0.7, jump=1.0, path_near=2.0, path_far=40.0,
                   min_votes=16, max_coast=10, one_sided=1, n_points=50)
CFG_DOUBLES = ("min_len", "slope_max", "vote_len", "x_vote", "slope_tol", "y_max", "min_sep", "gate", "span_quad", "w_min", "w_max",
               "default_width", "alpha", "jump", "path_near", "path_far")
CFG_INTS = ("min_votes", "max_coast", "one_sided", "n_points")

BOUND_DTYPE = np.dtype([("a0", "<f8"), ("a1", "<f8"), ("a2", "<f8"), ("x_min", "<f8"), ("x_max", "<f8"), ("length", "<f8"),
                        ("n_members", "<i4"), ("views", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
ROW_DTYPE = np.dtype([("left", "<f8", (3,)), ("right", "<f8", (3,)), ("centre", "<f8", (3,)), ("width", "<f8"), ("lane_offset", "<f8"),
                      ("heading", "<f8"), ("curvature", "<f8"), ("n_bounds", "<i4"), ("lane_count", "<i4"), ("lane_index", "<i4"),
                      ("views", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
INFO_DTYPE = np.dtype([("cam_rows", "<i4", (8,)), ("n_over", "<i4"), ("n_off", "<i4"), ("n_short", "<i4"), ("n_steep", "<i4"),
                       ("n_voters", "<i4"), ("dir_bin", "<i4"), ("n_cand", "<i4"), ("n_peaks", "<i4"), ("m_star", "<f8")])
STATE_DTYPE = np.dtype([("left", "<f8", (3,)), ("right", "<f8", (3,)), ("width", "<f8"), ("xmax_left", "<f8"), ("xmax_right", "<f8"),
                        ("has_left", "<i4"), ("has_right", "<i4"), ("miss_left", "<i4"), ("miss_right", "<i4"), ("has_width", "<i4"),
                        ("frames", "<i4")])
assert (BOUND_DTYPE.itemsize, ROW_DTYPE.itemsize, INFO_DTYPE.itemsize, STATE_DTYPE.itemsize) == (64, 128, 72, 96)

BOUND_QUAD, BOUND_KEPT, BOUND_LEFT, BOUND_RIGHT = 1, 2, 4, 8
LANE, ONE_SIDED, COAST_LEFT, COAST_RIGHT, CHANGE_LEFT, CHANGE_RIGHT, NO_VOTER = 1, 2, 4, 8, 16, 32, 64
MAXB = 8


def cfg_of(**kw):
    c = dict(DEFAULT_CFG)
    for k in kw:
        if k not in c:
            raise KeyError(k)
    c.update(kw)
    return c


def project(g, max_range, u, v):
    """av_ground_cfg's projection -> (f, l, on_road)."""
    F = (g[0] * u + g[1] * v) + g[2]
    L = (g[3] * u + g[4] * v) + g[5]
    D = (g[6] * u + g[7] * v) + g[8]
    if D == 0.0:
        return float("nan"), float("nan"), False
    f, l = F / D, L / D
    return f, l, bool(D > 0.0 and f >= 0.0 and f <= max_range)


def tree(x):
    """The wave's fixed tree over 64 lanes: adjacent pairs, six levels."""
    x = list(x)
    assert len(x) == 64
    while len(x) > 1:
        x = [x[i] + x[i + 1] for i in range(0, len(x), 2)]
    return x[0]


def rig_sum(terms, K):
    """terms: [(k, i, value)] with i the row's index in camera k's list -> the header's sum (0.0 for a camera without a term)."""
    parts = []
    for k in range(K):
        lanes = [0.0] * 64
        for kk, i, val in sorted((t for t in terms if t[0] == k), key=lambda t: t[1]):
            lanes[i & 63] = lanes[i & 63] + val
        parts.append(tree(lanes))
    s = parts[0]
    for k in range(1, K):
        s = s + parts[k]
    return s


def model_at(a, X):
    return (a[0] + a[1] * X) + a[2] * (X * X)


def fit_bound(S, quad):
    S0, S1, S2, S3, S4, T0, T1, T2 = S
    c11 = S2 - (S1 * S1) / S0
    d1 = T1 - (S1 * T0) / S0
    if not c11 > 1e-9 * S2:
        return None
    if quad:
        c12 = S3 - (S1 * S2) / S0
        c22 = S4 - (S2 * S2) / S0
        d2 = T2 - (S2 * T0) / S0
        e22 = c22 - (c12 * c12) / c11
        if not e22 > 1e-9 * S4:
            return None
        a2 = (d2 - (c12 * d1) / c11) / e22
        a1 = (d1 - c12 * a2) / c11
        a0 = ((T0 - a1 * S1) - a2 * S2) / S0
        return [a0, a1, a2]
    a1 = d1 / c11
    return [(T0 - a1 * S1) / S0, a1, 0.0]


def smooth_hist(h):
    return [(h[i - 1] if i > 0 else 0) + 2 * h[i] + (h[i + 1] if i < 63 else 0) for i in range(64)]


def zero_state():
    return np.zeros((), STATE_DTYPE)


def step(cfg, grounds, mounts, segments, nseg, scap, state, motion=None, plan_state=(0.0, 0.0, 0.0, 0.0)):
    """One frame of one vehicle.  grounds: K pairs (g [9], max_range); mounts [K][4] (c, s, mx, my); segments int [K][max_segments][4];
    nseg [K]; state: a STATE_DTYPE scalar (not modified); motion: None or (t_f, t_l, omega, valid).
    -> dict(state, bounds [8], info, row, ref_path [n_ref][2], n_ref, lane_offset, margins, rows)."""
    c = cfg
    K = len(grounds)
    segments = np.asarray(segments)
    max_segments = segments.shape[1]
    mg = {}

    def margin(name, dist):
        mg.setdefault(name, []).append(abs(float(dist)))

    # ---- 1. rows ----
    rows = []
    info = np.zeros((), INFO_DTYPE)
    for k in range(K):
        g, max_range = [float(x) for x in grounds[k][0]], float(grounds[k][1])
        mc, ms_, mx, my = [float(x) for x in mounts[k]]
        n = min(max(int(nseg[k]), 0), max_segments)
        info["n_over"] += max(n - scap, 0)
        n = min(n, scap)
        for i in range(n):
            x1, y1, x2, y2 = [float(int(t)) for t in segments[k][i]]
            f1, l1, on1 = project(g, max_range, x1, y1)
            f2, l2, on2 = project(g, max_range, x2, y2)
            if not (on1 and on2):
                info["n_off"] += 1
                continue
            xa, ya = (mx + mc * f1) - ms_ * l1, (my + ms_ * f1) + mc * l1
            xb, yb = (mx + mc * f2) - ms_ * l2, (my + ms_ * f2) + mc * l2
            if xb < xa:
                xa, ya, xb, yb = xb, yb, xa, ya
            dX, dY = xb - xa, yb - ya
            ln = math.sqrt(dX * dX + dY * dY)
            margin("min_len", ln - c["min_len"])
            if not ln >= c["min_len"]:
                info["n_short"] += 1
                continue
            margin("slope_max", abs(dY) - c["slope_max"] * dX)
            if not (dX > 0.0 and abs(dY) <= c["slope_max"] * dX):
                info["n_steep"] += 1
                continue
            q = ln / c["vote_len"]
            if 1.0 <= q < 256.0:
                margin("vote_weight", min(q - math.floor(q), math.floor(q) + 1.0 - q) * c["vote_len"])
            w = int(min(max(math.floor(q), 1.0), 255.0))
            rows.append(dict(k=k, i=i, X1=xa, Y1=ya, X2=xb, Y2=yb, len=ln, m=dY / dX, w=w, Xm=(xa + xb) * 0.5, Ym=(ya + yb) * 0.5))
            info["cam_rows"][k] += 1

    bounds = []          # dict(a, n, xmin, xmax, S0, views, flags)
    no_voter = True
    # ---- 2. direction vote ----
    for r in rows:
        margin("x_vote", r["Xm"] - c["x_vote"])
    voters = [r for r in rows if r["Xm"] <= c["x_vote"]]
    info["n_voters"] = len(voters)
    info["dir_bin"] = -1
    if voters:
        no_voter = False
        scale = 32.0 / c["slope_max"]
        h = [0] * 64
        for r in voters:
            t = (r["m"] + c["slope_max"]) * scale
            ft = math.floor(t)
            if 0.0 < t < 64.0:
                margin("m_bin_edge", min(t - ft, ft + 1.0 - t) / scale)
            r["bin_m"] = 0 if ft < 0.0 else (63 if ft > 63.0 else int(ft))
            h[r["bin_m"]] += r["w"]
        hp = smooth_hist(h)
        pm = max(range(64), key=lambda i: (hp[i], -i))
        info["dir_bin"] = pm
        near = [r for r in voters if abs(r["bin_m"] - pm) <= 1]
        m_star = rig_sum([(r["k"], r["i"], float(r["w"]) * r["m"]) for r in near], K) / float(sum(r["w"] for r in near))
        info["m_star"] = m_star
        # ---- 3. offset vote ----
        scale = 32.0 / c["y_max"]
        h = [0] * 64
        ov = []
        for r in voters:
            margin("slope_tol", abs(r["m"] - m_star) - c["slope_tol"])
            if not abs(r["m"] - m_star) <= c["slope_tol"]:
                continue
            r["b"] = r["Ym"] - m_star * r["Xm"]
            t = (r["b"] + c["y_max"]) * scale
            margin("b_bin_edge", min(t - math.floor(t), math.floor(t) + 1.0 - t) / scale)
            if t >= 0.0 and t < 64.0:
                r["bin_b"] = int(math.floor(t))
                h[r["bin_b"]] += r["w"]
                ov.append(r)
        hp = smooth_hist(h)
        cand = [i for i in range(64) if hp[i] >= c["min_votes"] and hp[i] > (hp[i - 1] if i > 0 else 0)
                and hp[i] >= (hp[i + 1] if i < 63 else 0)]
        info["n_cand"] = len(cand)
        bw = c["y_max"] / 32.0
        acc = []
        left = list(cand)
        while left and len(acc) < MAXB:
            ia = max(left, key=lambda i: (hp[i], -i))
            acc.append(ia)
            for j in left:
                if j != ia:
                    margin("min_sep", float(abs(j - ia)) * bw - c["min_sep"])
            left = [j for j in left if not float(abs(j - ia)) * bw < c["min_sep"]]
        acc.sort()
        info["n_peaks"] = len(acc)
        for pk in acc:
            near = [r for r in ov if abs(r["bin_b"] - pk) <= 1]
            a0 = rig_sum([(r["k"], r["i"], float(r["w"]) * r["b"]) for r in near], K) / float(sum(r["w"] for r in near))
            bounds.append(dict(a=[a0, m_star, 0.0], n=0, xmin=0.0, xmax=0.0, S0=0.0, views=0, flags=0, peak=pk))
        # ---- 4. grow and refit ----
        for rnd in range(3):
            rng_ = c["x_vote"] if rnd == 0 else 2.0 * c["x_vote"]
            members = [[] for _ in bounds]
            for r in rows:
                if rnd < 2:
                    margin("range", r["Xm"] - rng_)
                if not (rnd == 2 or r["Xm"] <= rng_):
                    continue
                best, bp, costs = float("inf"), -1, []
                for p, b in enumerate(bounds):
                    r1 = abs(r["Y1"] - model_at(b["a"], r["X1"]))
                    r2 = abs(r["Y2"] - model_at(b["a"], r["X2"]))
                    margin("gate", r1 - c["gate"])
                    margin("gate", r2 - c["gate"])
                    if r1 <= c["gate"] and r2 <= c["gate"]:
                        cost = max(r1, r2)
                        costs.append(cost)
                        if cost < best:
                            best, bp = cost, p
                if len(costs) > 1:
                    costs.sort()
                    margin("boundary_tie", costs[1] - costs[0])
                if bp >= 0:
                    members[bp].append(r)
            for p, b in enumerate(bounds):
                mem = members[p]
                keep_quad = b["flags"] & BOUND_QUAD
                b["flags"] &= BOUND_KEPT
                b["n"] = len(mem)
                if not mem:
                    b["flags"] |= BOUND_KEPT | keep_quad
                    b["xmin"] = b["xmax"] = b["S0"] = 0.0
                    b["views"] = 0
                    continue
                terms = [[] for _ in range(8)]
                for r in mem:
                    ln = r["len"]
                    # a lane adds a member's two end points one after the other: two terms under one row index, in this order
                    for X, Y in ((r["X1"], r["Y1"]), (r["X2"], r["Y2"])):
                        XX = X * X
                        vals = (ln, ln * X, ln * XX, ln * (XX * X), ln * (XX * XX), ln * Y, ln * (X * Y), ln * (XX * Y))
                        for q in range(8):
                            terms[q].append((r["k"], r["i"], vals[q]))
                S = [rig_sum(t, K) for t in terms]
                b["xmin"], b["xmax"] = min(r["X1"] for r in mem), max(r["X2"] for r in mem)
                b["views"] = 0
                for r in mem:
                    b["views"] |= 1 << r["k"]
                b["S0"] = S[0]
                if len(mem) >= 3:
                    margin("span_quad", (b["xmax"] - b["xmin"]) - c["span_quad"])
                quad = len(mem) >= 3 and b["xmax"] - b["xmin"] >= c["span_quad"]
                a = fit_bound(S, quad)
                if a is None:
                    b["flags"] |= BOUND_KEPT | keep_quad
                else:
                    b["a"] = a
                    if quad:
                        b["flags"] |= BOUND_QUAD
        bounds = [b for b in bounds if b["n"] > 0]

    # ---- 5. the ego lane ----
    nb = len(bounds)
    iL = iR = -1
    for p, b in enumerate(bounds):
        a0 = b["a"][0]
        margin("ego_sign", a0)
        if a0 < 0.0:
            if iL < 0 or a0 > bounds[iL]["a"][0]:
                iL = p
        elif a0 >= 0.0:
            if iR < 0 or a0 < bounds[iR]["a"][0]:
                iR = p
    if iL >= 0 and iR >= 0:
        wd = bounds[iR]["a"][0] - bounds[iL]["a"][0]
        margin("width_range", wd - c["w_min"])
        margin("width_range", wd - c["w_max"])
        if not (wd >= c["w_min"] and wd <= c["w_max"]):
            margin("nearer_side", -bounds[iL]["a"][0] - bounds[iR]["a"][0])
            if -bounds[iL]["a"][0] <= bounds[iR]["a"][0]:
                iR = -1
            else:
                iL = -1
    if iL >= 0:
        bounds[iL]["flags"] |= BOUND_LEFT
    if iR >= 0:
        bounds[iR]["flags"] |= BOUND_RIGHT

    # ---- 6. following ----
    st = np.array(state, STATE_DTYPE).copy()
    mv = motion is not None and int(motion[3]) != 0
    tf, tl, om = (float(motion[0]), float(motion[1]), float(motion[2])) if mv else (0.0, 0.0, 0.0)
    one_m_alpha = 1.0 - c["alpha"]
    status = NO_VOTER if no_voter else 0
    jumped, jump_d = [False, False], [0.0, 0.0]
    for side, (name, ib) in enumerate((("left", iL), ("right", iR))):
        a = [float(x) for x in st[name]]
        xmax = float(st["xmax_" + name])
        pr, pxmax = list(a), xmax
        if mv:
            pr[0] = ((a[0] + a[1] * tf) + a[2] * (tf * tf)) - tl
            pr[1] = (a[1] + (2.0 * a[2]) * tf) - om
            pxmax = xmax - tf
        if ib >= 0:
            nw = bounds[ib]["a"]
            smooth = False
            if st["has_" + name]:
                d = nw[0] - pr[0]
                margin("jump", abs(d) - c["jump"])
                if abs(d) <= c["jump"]:
                    smooth = True
                else:
                    jumped[side], jump_d[side] = True, d
            st[name] = [c["alpha"] * pr[i] + one_m_alpha * nw[i] if smooth else nw[i] for i in range(3)]
            st["xmax_" + name], st["has_" + name], st["miss_" + name] = bounds[ib]["xmax"], 1, 0
        elif st["has_" + name]:
            st["miss_" + name] += 1
            if st["miss_" + name] > c["max_coast"]:
                st[name], st["xmax_" + name], st["has_" + name], st["miss_" + name] = [0.0, 0.0, 0.0], 0.0, 0, 0
            else:
                st[name], st["xmax_" + name] = pr, pxmax
                status |= COAST_RIGHT if side else COAST_LEFT
    if iL >= 0 and iR >= 0:
        st["width"], st["has_width"] = float(st["right"][0]) - float(st["left"][0]), 1
    if jumped[0] and jumped[1]:
        d0, d1 = abs(jump_d[0]), abs(jump_d[1])
        for d in (d0, d1):
            margin("change_range", d - c["w_min"])
            margin("change_range", d - c["w_max"])
        if c["w_min"] <= d0 <= c["w_max"] and c["w_min"] <= d1 <= c["w_max"]:
            if jump_d[0] < 0.0 and jump_d[1] < 0.0:
                status |= CHANGE_LEFT
            if jump_d[0] > 0.0 and jump_d[1] > 0.0:
                status |= CHANGE_RIGHT
    st["frames"] += 1
    oL, oR = [float(x) for x in st["left"]], [float(x) for x in st["right"]]
    xL, xR = float(st["xmax_left"]), float(st["xmax_right"])
    outL, outR = bool(st["has_left"]), bool(st["has_right"])
    if c["one_sided"] and ((iL >= 0) != (iR >= 0)) and not (outL and outR):
        W = float(st["width"]) if st["has_width"] else c["default_width"]
        if iL >= 0:
            oR, xR, outR = [oL[0] + W, oL[1], oL[2]], xL, True
        else:
            oL, xL, outL = [oR[0] - W, oR[1], oR[2]], xR, True
        status |= ONE_SIDED
    lane = outL and outR
    if lane:
        status |= LANE

    # ---- 7. outputs ----
    row = np.zeros((), ROW_DTYPE)
    if outL:
        row["left"] = oL
    if outR:
        row["right"] = oR
    centre = [(oL[i] + oR[i]) * 0.5 for i in range(3)] if lane else [0.0, 0.0, 0.0]
    row["centre"] = centre
    row["width"] = oR[0] - oL[0] if lane else 0.0
    row["lane_offset"] = -centre[0] if lane else float("nan")
    row["heading"] = -math.atan(centre[1]) if lane else 0.0
    q = 1.0 + centre[1] * centre[1]
    row["curvature"] = (2.0 * centre[2]) / (q * math.sqrt(q)) if lane else 0.0
    nl = nr = 0
    if lane:
        if iL >= 0:
            for j in range(iL - 1, -1, -1):
                sp = bounds[j + 1]["a"][0] - bounds[j]["a"][0]
                margin("width_range", sp - c["w_min"])
                margin("width_range", sp - c["w_max"])
                if not (sp >= c["w_min"] and sp <= c["w_max"]):
                    break
                nl += 1
        if iR >= 0:
            for j in range(iR + 1, nb):
                sp = bounds[j]["a"][0] - bounds[j - 1]["a"][0]
                margin("width_range", sp - c["w_min"])
                margin("width_range", sp - c["w_max"])
                if not (sp >= c["w_min"] and sp <= c["w_max"]):
                    break
                nr += 1
    row["n_bounds"], row["lane_count"], row["lane_index"] = nb, (1 + nl + nr) if lane else 0, nl
    row["views"] = (bounds[iL]["views"] if iL >= 0 else 0) | (bounds[iR]["views"] if iR >= 0 else 0)
    row["status"] = status
    out_b = np.zeros(MAXB, BOUND_DTYPE)
    for p, b in enumerate(bounds):
        out_b[p] = (b["a"][0], b["a"][1], b["a"][2], b["xmin"], b["xmax"], b["S0"] * 0.5, b["n"], b["views"], b["flags"], 0)
    x_end = min(c["path_far"], min(xL, xR))
    if lane:
        margin("path", (x_end - c["path_near"]) - 1.0)
    n_ref = c["n_points"] if lane and x_end - c["path_near"] >= 1.0 else 0
    path = np.zeros((n_ref, 2))
    if n_ref:
        x0, y0, hd = float(plan_state[0]), float(plan_state[1]), float(plan_state[2])
        cs, sn = math.cos(hd), math.sin(hd)
        c2, s2 = math.cos(hd + 1.5707963267948966), math.sin(hd + 1.5707963267948966)
        stp = (x_end - c["path_near"]) / float(c["n_points"] - 1)
        for i in range(n_ref):
            X = c["path_near"] + float(i) * stp
            Y = model_at(centre, X)
            path[i] = ((x0 + X * cs) + Y * c2, (y0 + X * sn) + Y * s2)
    return dict(state=st, bounds=out_b, info=info, row=row, ref_path=path, n_ref=n_ref, lane_offset=float(row["lane_offset"]),
                margins=mg, rows=rows)


def smallest_margin(margins, exempt=()):
    """-> (distance, name) of the smallest margin outside `exempt`; (inf, None) without one."""
    best = (float("inf"), None)
    for name, vals in margins.items():
        if name in exempt or not vals:
            continue
        best = min(best, (min(vals), name))
    return best
