"""The road memory's arithmetic in NumPy (include/avhot.h: av_roadmem_*): stages 1 - 3 in the header's operation order, float64 with
every operation rounded on its own, integers as int64.  The device is held against this byte for byte; tests/test_roadmem_host.py
holds it against the world the panels were rendered from, and against a restatement without a torus."""
import numpy as np

f8, i8 = np.float64, np.int64
POSE_LIMIT = 2.0 ** 30


def cfg(n=256, max_age=90, m_per_px=0.1, gh=160, gw=160, x_far=8.0, panel_m_per_px=0.1, fill=(0, 0, 0)):
    return dict(n=int(n), max_age=int(max_age), m_per_px=f8(m_per_px), gh=int(gh), gw=int(gw), x_far=f8(x_far),
                panel_m_per_px=f8(panel_m_per_px), fill=tuple(int(c) for c in fill))


def pose_from(x, y, psi, mode=None):
    """Stage 1 -> (x, y, cs, sn, reset)."""
    return (f8(x), f8(y), f8(np.cos(f8(psi))), f8(np.sin(f8(psi))), int(mode is not None and int(mode) == 2))


def blend(p00, p01, p10, p11, wx, wy):
    """av_ground_warp's bilinear rule on one channel: int64 arrays (the sum stays below 2^41)."""
    top = p00 * (65536 - wx) + p01 * wx
    bot = p10 * (65536 - wx) + p11 * wx
    return (top * (65536 - wy) + bot * wy + (1 << 31)) >> 32


def window(x, y, c):
    """-> (i0, j0, bad) of the pose."""
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = f8(x) / c["m_per_px"], f8(y) / c["m_per_px"]
        bad = not (abs(qx) <= POSE_LIMIT and abs(qy) <= POSE_LIMIT)
    if bad:
        return 0, 0, True
    return int(np.floor(qx)) - c["n"] // 2, int(np.floor(qy)) - c["n"] // 2, False


def panel_points(c):
    """-> (X [gh, 1], Y [1, gw]): the vehicle-frame road point of every panel pixel, av_rig_surround's."""
    X = c["x_far"] - (np.arange(c["gh"], dtype=f8) + 0.5) * c["panel_m_per_px"]
    Y = ((np.arange(c["gw"], dtype=f8) + 0.5) - f8(c["gw"]) / 2.0) * c["panel_m_per_px"]
    return X[:, None], Y[None, :]


def cell_taps(c, pose, i, j):
    """Steps 2 - 4's positions for world cells (i, j) (int64 arrays of one shape) -> dict(inside, r0, r1, c0, c1, wr, wc, args), args
    the two arguments of floor() (for margin())."""
    x, y, cs, sn = pose[:4]
    m, pm, gh, gw = c["m_per_px"], c["panel_m_per_px"], c["gh"], c["gw"]
    with np.errstate(invalid="ignore", over="ignore"):
        xc, yc = (i.astype(f8) + 0.5) * m, (j.astype(f8) + 0.5) * m
        dx, dy = xc - x, yc - y
        X, Y = cs * dx + sn * dy, cs * dy - sn * dx
        pr, pc = (c["x_far"] - X) / pm - 0.5, Y / pm + f8(gw) / 2.0 - 0.5
        ar, ac = pr * 65536.0 + 0.5, pc * 65536.0 + 0.5
        tr, tc = np.floor(ar), np.floor(ac)
        inside = (tr >= 0.0) & (tr <= f8(gh - 1) * 65536.0) & (tc >= 0.0) & (tc <= f8(gw - 1) * 65536.0)
    itr, itc = np.where(inside, tr, 0.0).astype(i8), np.where(inside, tc, 0.0).astype(i8)
    r0, c0 = itr >> 16, itc >> 16
    return dict(inside=inside, r0=r0, c0=c0, r1=np.minimum(r0 + 1, gh - 1), c1=np.minimum(c0 + 1, gw - 1), wr=itr & 65535, wc=itc & 65535,
                args=(ar, ac))


def pixel_taps(c, pose, i0, j0):
    """Steps 1 - 3 of the fill for every panel pixel, and the window test of step 4 -> dict(inwin, ia, ja, wi, wj, args)."""
    x, y, cs, sn = pose[:4]
    m, n = c["m_per_px"], c["n"]
    X, Y = panel_points(c)
    with np.errstate(invalid="ignore", over="ignore"):
        xw, yw = (x + cs * X) - sn * Y, (y + sn * X) + cs * Y
        ai, aj = (xw / m - 0.5) * 65536.0 + 0.5, (yw / m - 0.5) * 65536.0 + 0.5
        ti, tj = np.floor(ai), np.floor(aj)
        inwin = ((ti >= f8(i0) * 65536.0) & (ti < (f8(i0) + f8(n - 1)) * 65536.0) & (tj >= f8(j0) * 65536.0)
                 & (tj < (f8(j0) + f8(n - 1)) * 65536.0))
    iti, itj = np.where(inwin, ti, 0.0).astype(i8), np.where(inwin, tj, 0.0).astype(i8)
    return dict(inwin=inwin, ia=iti >> 16, ja=itj >> 16, wi=iti & 65535, wj=itj & 65535, args=(ai, aj))


class RoadMemory:
    """One vehicle's canvas, stamps and state."""

    def __init__(self, c):
        self.c = c
        n = c["n"]
        self.canvas = np.zeros((n, n, 4), np.uint8)
        self.stamp = np.zeros((n, n), np.uint32)
        self.state = dict(i0=0, j0=0, frames=0, status=0)

    def reset(self):
        self.state = dict(i0=0, j0=0, frames=0, status=0)

    def state_row(self):
        s = self.state
        return (s["i0"], s["j0"], s["frames"], s["status"])

    def window_cells(self, i0, j0):
        """The cells of the window at (i0, j0) -> (i [N, 1], j [1, N]) int64."""
        n = self.c["n"]
        return (i0 + np.arange(n, dtype=i8))[:, None], (j0 + np.arange(n, dtype=i8))[None, :]

    def update(self, pose, panel, cover):
        """Stage 2.  pose: (x, y, cs, sn, reset); panel uint8 [gh, gw, 3] (before any fill), cover uint8 [gh, gw].  -> the mask
        [N, N] of the new window's cells that were seen (in window order)."""
        c, s, n = self.c, self.state, self.c["n"]
        i0n, j0n, bad = window(pose[0], pose[1], c)
        if bad:
            self.state = dict(i0=0, j0=0, frames=0, status=1)
            return np.zeros((n, n), bool)
        fresh = bool(pose[4]) or s["frames"] == 0
        F = 1 if fresh else s["frames"] + 1
        i, j = self.window_cells(i0n, j0n)
        i, j = np.broadcast_arrays(i, j)
        entered = fresh | (i < s["i0"]) | (i >= s["i0"] + n) | (j < s["j0"]) | (j >= s["j0"] + n)
        a, b = np.mod(i, n), np.mod(j, n)
        self.stamp[a[entered], b[entered]] = 0
        t = cell_taps(c, pose, i, j)
        r0, r1, c0, c1 = t["r0"], t["r1"], t["c0"], t["c1"]
        seen = t["inside"] & (cover[r0, c0] != 0) & (cover[r0, c1] != 0) & (cover[r1, c0] != 0) & (cover[r1, c1] != 0)
        p = panel.astype(i8)
        for ch in range(3):
            v = blend(p[r0, c0, ch], p[r0, c1, ch], p[r1, c0, ch], p[r1, c1, ch], t["wc"], t["wr"])
            self.canvas[a[seen], b[seen], ch] = v[seen].astype(np.uint8)
        self.canvas[a[seen], b[seen], 3] = 0
        self.stamp[a[seen], b[seen]] = F
        self.state = dict(i0=i0n, j0=j0n, frames=F, status=0)
        return seen

    def fill(self, pose, panel, cover):
        """Stage 3 -> (panel [gh, gw, 3], age [gh, gw]), the panel a copy."""
        c, s, n = self.c, self.state, self.c["n"]
        F = s["frames"]
        t = pixel_taps(c, pose, s["i0"], s["j0"])
        a0, b0 = np.mod(t["ia"], n), np.mod(t["ja"], n)
        a1, b1 = np.mod(t["ia"] + 1, n), np.mod(t["ja"] + 1, n)
        st = self.stamp.astype(i8)
        s00, s01, s10, s11 = st[a0, b0], st[a0, b1], st[a1, b0], st[a1, b1]
        old = F - np.minimum(np.minimum(s00, s01), np.minimum(s10, s11))
        rem = (F != 0) & t["inwin"] & (s00 != 0) & (s01 != 0) & (s10 != 0) & (s11 != 0) & (old <= c["max_age"])
        unseen = cover == 0
        out, age = panel.copy(), np.zeros(cover.shape, np.uint8)
        cv = self.canvas.astype(i8)
        for ch in range(3):
            v = blend(cv[a0, b0, ch], cv[a0, b1, ch], cv[a1, b0, ch], cv[a1, b1, ch], t["wj"], t["wi"])
            out[..., ch] = np.where(unseen, np.where(rem, v, c["fill"][ch]), panel[..., ch]).astype(np.uint8)
        age[unseen] = np.where(rem, np.minimum(old, 254), 255)[unseen].astype(np.uint8)
        return out, age

    def step(self, pose, panel, cover):
        self.update(pose, panel, cover)
        return self.fill(pose, panel, cover)

    def world_cell(self, i, j):
        """(b, g, r, stamp) of world cell (i, j) of the current window."""
        n = self.c["n"]
        a, b = i % n, j % n
        return tuple(int(v) for v in self.canvas[a, b, :3]) + (int(self.stamp[a, b]),)
