"""av_lane_plan (include/avhot.h) restated in NumPy / math on the same row bytes: one vehicle per call, steps 1 - 5 in the device's
order, every loop sequential in the waypoint index i and the line index j, every operation a float64 operation rounded on its own.

Like tests/roadmarks_ref.py it reports the MARGINS of the decisions, the smallest over the valid waypoints of every (candidate, line):
  side    |e|: where `side` could flip
  on      |half_width - |e||: where a waypoint could start or stop counting as on the line
  extent  |X - min(xe, x_far)|: where a waypoint could become valid or invalid (the first waypoint of a planner's candidate is the
          start state itself, X = 0 exactly at any pose)
  rank    the smallest gap between consecutive ranked totals
A case at the pose (0, 0, 0) has exact vehicle-frame coordinates (sin 0 = 0, cos 0 = 1 on both sides) and is compared bit for bit;
a case at another pose must have every margin >= 1e-6 (MIN_MARGIN)."""
import math

import numpy as np

from tests import roadlanes_ref as lanes_ref
from tests import roadmarks_ref as marks_ref

DEFAULT_CFG = dict(half_width=0.9, x_far=40.0, w_cross=(300.0, 1000.0, 0.0), w_on=(2.0, 5.0, 0.0), w_end=500.0, follow=1)
UNKNOWN, SOLID, DASHED = marks_ref.UNKNOWN, marks_ref.SOLID, marks_ref.DASHED
MAXB, MAXL, MAX_CAND, MAX_POINTS = 8, 10, 192, 256
SRC_LEFT, SRC_RIGHT = 8, 9
KEEP, LEFT, RIGHT = 0, 1, 2
FOLLOW, CHANGED, FORCED, NO_LINES = 1, 2, 4, 8
MIN_MARGIN = 1e-6

BOUND_DTYPE, LANES_DTYPE, MARK_DTYPE, SIDES_DTYPE = marks_ref.BOUND_DTYPE, marks_ref.LANES_DTYPE, marks_ref.MARK_DTYPE, marks_ref.ROW_DTYPE
LINE_DTYPE = np.dtype([("a0", "<f8"), ("a1", "<f8"), ("a2", "<f8"), ("xe", "<f8"), ("type", "<i4"), ("source", "<i4"),
                       ("reserved", "<i4", (2,))])
ROW_DTYPE = np.dtype([("best", "<i4"), ("base_best", "<i4"), ("maneuver", "<i4"), ("delta", "<i4"), ("crossed", "<u4"),
                      ("crossed_solid", "<u4"), ("crossed_unknown", "<u4"), ("n_lines", "<i4"), ("flags", "<i4"), ("reserved", "<i4"),
                      ("base_cost", "<f8"), ("lane_cost", "<f8"), ("total", "<f8")])
assert (LINE_DTYPE.itemsize, ROW_DTYPE.itemsize) == (48, 64)


def cfg_of(**kw):
    c = dict(DEFAULT_CFG)
    for k in kw:
        if k not in c:
            raise KeyError(k)
    c.update(kw)
    return c


def _type(t):
    t = int(t)
    return t if 0 <= t <= 2 else UNKNOWN


def lines_of(cfg, bounds, lanes, marks, sides):
    """Step 1 -> (LINE_DTYPE [10], n_lines)."""
    out = np.zeros(MAXL, LINE_DTYPE)
    out["source"] = -1
    nb = min(max(int(lanes["n_bounds"]), 0), MAXB)
    left_type = _type(sides["left"]["type"]) if sides is not None else UNKNOWN
    right_type = _type(sides["right"]["type"]) if sides is not None else UNKNOWN
    has_left = has_right = False
    for b in range(nb):
        bd, l = bounds[b], out[b]
        l["a0"], l["a1"], l["a2"], l["xe"], l["source"] = bd["a0"], bd["a1"], bd["a2"], bd["x_max"], b
        if bd["flags"] & lanes_ref.BOUND_LEFT:
            l["type"], has_left = left_type, True
        elif bd["flags"] & lanes_ref.BOUND_RIGHT:
            l["type"] = right_type
        else:
            l["type"] = _type(marks[b]["type"]) if marks is not None else UNKNOWN
        has_right |= bool(bd["flags"] & lanes_ref.BOUND_RIGHT)
    n = nb
    if int(lanes["status"]) & lanes_ref.LANE:
        for missing, poly, typ, src in ((not has_left, lanes["left"], left_type, SRC_LEFT), (not has_right, lanes["right"], right_type, SRC_RIGHT)):
            if missing:
                l = out[n]
                l["a0"], l["a1"], l["a2"], l["xe"], l["type"], l["source"] = poly[0], poly[1], poly[2], cfg["x_far"], typ, src
                n += 1
    return out, n


def stable_order(values):
    """rank_and_store's rule: candidate c's rank is the count of o with v[o] < v[c] or (v[o] == v[c] and o < c)."""
    C = len(values)
    order = np.zeros(C, np.int32)
    for c in range(C):
        rank = sum(1 for o in range(C) if values[o] < values[c] or (values[o] == values[c] and o < c))
        order[rank] = c
    return order


def step(cfg, plan_state, wp, cost, bounds, lanes, marks=None, sides=None):
    """One vehicle.  plan_state [4]; wp [C, n, >= 2]; cost [C]; bounds BOUND_DTYPE [8]; lanes LANES_DTYPE scalar; marks MARK_DTYPE [8]
    and sides marks_ref.ROW_DTYPE scalar, or both None.  -> dict(lines, n_lines, lane_cost, total, order, cross, delta, row,
    margins)."""
    f = np.float64
    hw, x_far, w_end = f(cfg["half_width"]), f(cfg["x_far"]), f(cfg["w_end"])
    w_cross, w_on = [f(x) for x in cfg["w_cross"]], [f(x) for x in cfg["w_on"]]
    lines, n_lines = lines_of(cfg, bounds, lanes, marks, sides)
    follow = bool(cfg["follow"]) and bool(int(lanes["status"]) & lanes_ref.LANE)
    c1, c2 = (f(lanes["centre"][1]), f(lanes["centre"][2])) if follow else (f(0.0), f(0.0))
    x0, y0, h = f(plan_state[0]), f(plan_state[1]), f(plan_state[2])
    cs, sn = f(math.cos(h)), f(math.sin(h))
    C, n = wp.shape[0], wp.shape[1]
    lane_cost, total = np.zeros(C), np.zeros(C)
    cross, delta = np.zeros(C, np.uint32), np.zeros(C, np.int32)
    margins = dict(side=np.inf, on=np.inf, extent=np.inf, rank=np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            XY = []
            for i in range(n):
                dx, dy = f(wp[c, i, 0]) - x0, f(wp[c, i, 1]) - y0
                XY.append((dx * cs + dy * sn, dy * cs - dx * sn))
            s = f(0.0)
            for j in range(n_lines):
                l = lines[j]
                t = int(l["type"])
                a0, b1, b2, xe = f(l["a0"]), f(l["a1"]) - c1, f(l["a2"]) - c2, f(l["xe"])
                any_, crossed, on_any, first, last, last_d, on = False, False, False, False, False, f(0.0), f(0.0)
                lim = min(xe, x_far)
                for X, Y in XY:
                    if lim == lim and X == X:
                        margins["extent"] = min(margins["extent"], abs(X - lim))
                    if not (X >= 0.0 and X <= xe and X <= x_far):
                        continue
                    e = Y - ((a0 + b1 * X) + b2 * (X * X))
                    side = bool(e > 0.0)
                    d = hw - abs(e)
                    margins["side"], margins["on"] = min(margins["side"], abs(e)), min(margins["on"], abs(d))
                    if any_:
                        crossed |= side != last
                    else:
                        first = side
                    if d > 0.0:
                        on, on_any = on + w_on[t] * (d * d), True
                    any_, last, last_d = True, side, d
                end = w_end * (last_d * last_d) if any_ and last_d > 0.0 else f(0.0)
                s = s + (((w_cross[t] if crossed else f(0.0)) + on) + end)
                cross[c] |= (int(crossed) << j) | (int(on_any) << (16 + j))
                delta[c] += (int(last) - int(first)) if any_ else 0
            lane_cost[c], total[c] = s, f(cost[c]) + s
    order = stable_order(total)
    ranked = total[order]
    if C > 1 and np.isfinite(ranked).all():
        margins["rank"] = float(np.min(np.diff(ranked)))
    base = stable_order(np.asarray(cost, np.float64))
    row = np.zeros((), ROW_DTYPE)
    best = int(order[0])
    row["best"], row["base_best"], row["delta"], row["n_lines"] = best, int(base[0]), delta[best], n_lines
    row["maneuver"] = LEFT if delta[best] < 0 else RIGHT if delta[best] > 0 else KEEP
    row["crossed"] = int(cross[best]) & 0xFFFF
    for j in range(n_lines):
        if (int(row["crossed"]) >> j) & 1:
            if lines[j]["type"] == SOLID:
                row["crossed_solid"] |= np.uint32(1 << j)
            if lines[j]["type"] == UNKNOWN:
                row["crossed_unknown"] |= np.uint32(1 << j)
    row["flags"] = ((FOLLOW if follow else 0) | (CHANGED if best != int(base[0]) else 0)
                    | (FORCED if int(row["crossed_solid"]) | int(row["crossed_unknown"]) else 0) | (NO_LINES if n_lines == 0 else 0))
    row["base_cost"], row["lane_cost"], row["total"] = cost[best], lane_cost[best], total[best]
    return dict(lines=lines, n_lines=n_lines, lane_cost=lane_cost, total=total, order=order, cross=cross, delta=delta, row=row,
                margins=margins)


def smallest_margin(margins, rank=True):
    return min(v for k, v in margins.items() if rank or k != "rank")
