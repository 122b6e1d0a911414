"""av_rig_track (include/avhot.h) restated in NumPy: one frame of one vehicle as a loop over slots, rows and match iterations, on
the same 96-byte slots the device keeps.

Every arithmetic step is one float64 operation (NumPy scalars and element-wise arrays: no fused multiply-add), in the header's
order.  Besides the result, step() reports how close the discrete decisions of its input came to their thresholds, as
tests/rig_ref.py does:

  gate_margin   the smallest |d2 - gate^2| / max(d2, gate^2) over every live slot x kept row pair
  tie_margin    the smallest (runner-up d2 - winning d2) / runner-up d2 over the match iterations that had a runner-up

Planted ties (integer-valued coordinates and velocities, dt a power of two) are exempt from the margin: their arithmetic is exact.
"""
import math

import numpy as np

MARGIN = 1e-6
f8 = np.float64
HDR_BYTES, SLOT_BYTES = 64, 96
SLOT = np.dtype([("id", "<i4"), ("hits", "<i4"), ("misses", "<i4"), ("age", "<i4"), ("views", "<i4"), ("views_ever", "<i4"),
                 ("reserved", "<i4", (2,)), ("x", "<f8", (4,)), ("p", "<f8", (3,)), ("r", "<f8")])
assert SLOT.itemsize == SLOT_BYTES
DEFAULTS = dict(dt=1.0 / 30.0, q_accel=4.0, r_meas=0.25, r_range=1e-6, p0_pos=1.0, p0_vel=25.0, gate_scale=2.0, gate_min=2.0,
                max_age=30, min_hits=3)


def cfg(**over):
    c = dict(DEFAULTS)
    unknown = set(over) - set(c)
    assert not unknown, unknown
    c.update(over)
    return c


def state_bytes(tcap):
    return HDR_BYTES + SLOT_BYTES * tcap


def reset_state(tcap):
    """One vehicle's state after av_rig_track_reset: uint8 [state_bytes(tcap)]."""
    st = np.zeros(state_bytes(tcap), np.uint8)
    hdr, slots = views_of(st)
    hdr[1] = 1
    slots["id"] = -1
    return st


def views_of(st):
    """(hdr int32 [16], slots structured [tcap]) as views of one vehicle's state bytes."""
    return st[:HDR_BYTES].view(np.int32), st[HDR_BYTES:].view(SLOT)


def step(state, obs, n_in, views, plan_state, c):
    """One frame of one vehicle.  state: uint8 [state_bytes(tcap)], left as it is; obs [ocap_in][ncol]; views [ocap_in] or None
    -> dict(state (the new bytes), obstacles [M][ncol], obs_slot [M], match [clamp(n_in)], n_skip, n_drop, gate_margin, tie_margin)."""
    st = np.array(state, np.uint8, copy=True)
    hdr, sl = views_of(st)
    tcap = len(sl)
    obs = np.asarray(obs, f8)
    ocap_in, ncol = obs.shape
    moving = ncol == 5
    dt, q, rm, rr = f8(c["dt"]), f8(c["q_accel"]), f8(c["r_meas"]), f8(c["r_range"])
    gs, gm = f8(c["gate_scale"]), f8(c["gate_min"])
    x0, y0 = f8(plan_state[0]), f8(plan_state[1])
    gate_margin = tie_margin = math.inf
    with np.errstate(all="ignore"):
        # 1 predict
        dt2 = dt * dt
        q11, q12, q22 = q * ((dt2 * dt2) / f8(4.0)), q * ((dt2 * dt) / f8(2.0)), q * dt2
        for s in sl:
            if s["id"] < 0:
                continue
            x, y, vx, vy = s["x"]
            a, b, cc = s["p"]
            s["x"][0], s["x"][1] = x + vx * dt, y + vy * dt
            bc = b + dt * cc
            s["p"][0] = ((a + dt * b) + dt * bc) + q11
            s["p"][1] = bc + q12
            s["p"][2] = cc + q22
            s["age"] += 1
        # 2 candidates
        n = min(max(int(n_in), 0), ocap_in)
        match = np.full(n, -1, np.int32)
        kept, n_skip = [], 0
        for j in range(n):
            ok = np.isfinite(obs[j, 0]) and np.isfinite(obs[j, 1]) and np.isfinite(obs[j, 2]) and obs[j, 2] > 0.0
            if moving:
                ok = ok and np.isfinite(obs[j, 3]) and np.isfinite(obs[j, 4])
            if ok:
                kept.append(j)
            else:
                n_skip += 1
        vw = lambda j: 0 if views is None else int(views[j])                 # noqa: E731
        # 3 association
        live = [i for i in range(tcap) if sl["id"][i] >= 0]
        row_of = {}
        if live and kept:
            sx, sy, sr = (np.array([t for t in v], f8)[:, None] for v in (sl["x"][live, 0], sl["x"][live, 1], sl["r"][live]))
            cx, cy, cr = (obs[kept, k][None, :] for k in range(3))
            dx, dy = sx - cx, sy - cy
            d2 = dx * dx + dy * dy
            gate = np.maximum(gm, gs * np.maximum(sr, cr))
            g2 = gate * gate
            den = np.maximum(d2, g2)
            rel = np.where(den > 0.0, np.abs(d2 - g2) / np.where(den > 0.0, den, 1.0), 0.0)
            gate_margin = min(gate_margin, float(rel.min()))
            free = (d2 <= g2) & np.isfinite(d2)
            while free.any():
                vals = d2[free]
                vals = np.sort(vals) if len(vals) <= 2 else np.partition(vals, 1)[:2]      # the winner and the runner-up
                best = vals[0]
                if len(vals) > 1:
                    tie_margin = min(tie_margin, float((vals[1] - best) / vals[1]) if vals[1] > 0.0 else 0.0)
                i, j = np.argwhere(free & (d2 == best))[0]                   # row-major: the smallest slot, then the smallest row
                row_of[live[i]] = kept[j]
                free[i, :] = False
                free[:, j] = False
        # 4 update, 5 misses and deaths
        for i in live:
            s = sl[i]
            if i in row_of:
                j = row_of[i]
                zx, zy = obs[j, 0], obs[j, 1]
                ex, ey = zx - x0, zy - y0
                m = max(ex * ex + ey * ey, f8(1.0))
                R = rm + rr * (m * m)
                a, b, cc = s["p"]
                S = a + R
                k0, k1 = a / S, b / S
                yx, yy = zx - s["x"][0], zy - s["x"][1]
                s["x"][0], s["x"][2] = s["x"][0] + k0 * yx, s["x"][2] + k1 * yx
                s["x"][1], s["x"][3] = s["x"][1] + k0 * yy, s["x"][3] + k1 * yy
                s["p"][0], s["p"][1], s["p"][2] = a - k0 * a, b - k0 * b, cc - k1 * b
                s["r"] = obs[j, 2]
                s["hits"] += 1
                s["misses"] = 0
                s["views"] = vw(j)
                s["views_ever"] |= vw(j)
                match[j] = s["id"]
            else:
                s["misses"] += 1
                s["views"] = 0
                if s["misses"] > c["max_age"]:
                    sl[i] = np.zeros((), SLOT)
                    sl[i]["id"] = -1
        # 6 births
        taken = set(row_of.values())
        free_slots = [i for i in range(tcap) if sl["id"][i] < 0]
        n_drop = 0
        for j in kept:
            if j in taken:
                continue
            if not free_slots:
                match[j] = -2
                n_drop += 1
                continue
            s = sl[free_slots.pop(0)]
            s["id"] = hdr[1]
            hdr[1] += 1
            s["x"] = (obs[j, 0], obs[j, 1], obs[j, 3] if moving else 0.0, obs[j, 4] if moving else 0.0)
            s["p"] = (c["p0_pos"], 0.0, c["p0_vel"])
            s["r"] = obs[j, 2]
            s["hits"], s["misses"], s["age"] = 1, 0, 0
            s["views"] = s["views_ever"] = vw(j)
            match[j] = s["id"]
        if n_drop:
            hdr[0] |= 1
        # 7 output
        out_slots = [i for i in range(tcap) if sl["id"][i] >= 0 and sl["hits"][i] >= c["min_hits"]]
        out = np.zeros((len(out_slots), ncol), f8)
        for row, i in enumerate(out_slots):
            out[row, :2], out[row, 2] = sl["x"][i, :2], sl["r"][i]
            if moving:
                out[row, 3:] = sl["x"][i, 2:]
        hdr[2] += 1
        hdr[3] = int((sl["id"] >= 0).sum())
    return dict(state=st, obstacles=out, obs_slot=np.array(out_slots, np.int32), match=match, n_skip=n_skip, n_drop=n_drop,
                gate_margin=gate_margin, tie_margin=tie_margin)


def run(frames, tcap, c, state=None):
    """A whole sequence of one vehicle, free-running: frames = [(obs [ocap_in][ncol], n_in, views or None, plan_state [4])] ->
    the list of step()'s results."""
    st = reset_state(tcap) if state is None else state
    out = []
    for obs, n_in, views, ps in frames:
        r = step(st, obs, n_in, views, ps, c)
        st = r["state"]
        out.append(r)
    return out


def margins(results):
    return min(r["gate_margin"] for r in results), min(r["tie_margin"] for r in results)


def tracks(state):
    """The slots of one vehicle's state bytes (a copy)."""
    return views_of(np.array(state, np.uint8, copy=True))[1]
