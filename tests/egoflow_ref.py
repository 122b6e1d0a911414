"""CPU restatement of the ground odometry (include/avhot.h: av_egoflow_patch / _match / _solve / _measure / _update), test
infrastructure.

NumPy integers and float64 scalars in the operation order the header states.  A configuration is a dict with av_egoflow_cfg's
fields (cfg()); a tile table is a structured array with av_egoflow_tile's fields; a motion is a dict with av_egoflow_motion's.
The fit's sums are taken sequentially in tile order; the device sums per lane and then over a tree, so its sums may differ in the
last bits.
"""
import numpy as np

from tests import ground_ref

f8 = np.float64

ACCEPTED, LIVE, GATED, INLIER = 1, 2, 4, 8
TILE_FIELDS = [("flags", "<i4"), ("dy", "<i4"), ("dx", "<i4"), ("sad", "<i4"), ("texture", "<i4"), ("reserved", "<i4"),
               ("sub_dy", "<f8"), ("sub_dx", "<f8"), ("f", "<f8"), ("l", "<f8")]


def cfg(gh=256, gw=256, f_far=None, m_per_px=0.1, tile=16, search=12, frame_rate=30.0, min_texture=None, gate_px=3, inlier_px=1.0,
        min_inliers=8):
    """av_egoflow_cfg with GroundOdometry's defaults (near edge 4 m ahead, min_texture 2 T T)."""
    return dict(gh=int(gh), gw=int(gw), tile=int(tile), search=int(search),
                f_far=4.0 + gh * float(m_per_px) if f_far is None else float(f_far), m_per_px=float(m_per_px),
                frame_rate=float(frame_rate), min_texture=2 * tile * tile if min_texture is None else int(min_texture),
                gate_px=int(gate_px), inlier_px=float(inlier_px), min_inliers=int(min_inliers))


def tile_grid(c):
    """-> (tiles_y, tiles_x)."""
    return (c["gh"] - 2 * c["search"]) // c["tile"], (c["gw"] - 2 * c["search"]) // c["tile"]


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
def patch(cam, bgr, c):
    """bgr uint8 [h, w, 3] through camera `cam` (ground_ref's dict) -> (gray uint8 [gh, gw], valid bool [gh, gw])."""
    bgr = np.asarray(bgr)
    h, w = bgr.shape[:2]
    gh, gw = c["gh"], c["gw"]
    D, su, sv = ground_ref.warp_positions(cam, h, w, gh, gw, c["f_far"], c["m_per_px"])
    with np.errstate(invalid="ignore"):
        tu, tv = np.floor(su), np.floor(sv)
        ok = (D > 0.0) & (tu >= 0.0) & (tu <= f8(w - 1) * 65536.0) & (tv >= 0.0) & (tv <= f8(h - 1) * 65536.0)
    p = ground_ref.ground_warp(cam, bgr, gh, gw, c["f_far"], c["m_per_px"]).astype(np.int64)
    gray = (1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14
    return np.where(ok, gray, 0).astype(np.uint8), ok


def pack_valid(valid):
    """bool [gh, gw] -> uint32 [gh, (gw + 31) // 32]: bit c & 31 of word c >> 5."""
    gh, gw = valid.shape
    vw = (gw + 31) // 32
    bits = np.zeros((gh, vw * 32), np.uint64)
    bits[:, :gw] = valid
    return (bits.reshape(gh, vw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
def tile_sads(cur, prev, y0, x0, T, R):
    """-> int64 [2R+1, 2R+1]: SAD(dy, dx) of the tile at (y0, x0)."""
    win = prev[y0 - R:y0 + T + R, x0 - R:x0 + T + R].astype(np.int64)
    blk = cur[y0:y0 + T, x0:x0 + T].astype(np.int64)
    sw = np.lib.stride_tricks.sliding_window_view(win, (T, T))
    return np.abs(sw - blk).sum(axis=(2, 3))


def subpixel(sm, s0, sp):
    den = f8(int(sm) - 2 * int(s0) + int(sp)) * 2.0
    return f8(int(sm) - int(sp)) / den if den > 0.0 else f8(0.0)


def match(cur, prev, valid, c, sads_out=None):
    """cur, prev uint8 [gh, gw], valid bool [gh, gw] -> tile table [n_tiles].  sads_out: a dict that receives tile -> SAD array."""
    T, R, m = c["tile"], c["search"], f8(c["m_per_px"])
    ty, tx = tile_grid(c)
    out = np.zeros(ty * tx, np.dtype(TILE_FIELDS))
    for k in range(ty * tx):
        y0, x0 = R + (k // tx) * T, R + (k % tx) * T
        o = out[k]
        o["f"] = f8(c["f_far"]) - (f8(y0) + f8(T) / 2.0) * m
        o["l"] = ((f8(x0) + f8(T) / 2.0) - f8(c["gw"]) / 2.0) * m
        if not valid[y0 - R:y0 + T + R, x0 - R:x0 + T + R].all():
            continue
        sad = tile_sads(cur, prev, y0, x0, T, R)
        if sads_out is not None:
            sads_out[k] = sad
        best = int(np.argmin(sad))                          # the first of equal minima in row-major order
        by, bx = best // (2 * R + 1), best % (2 * R + 1)
        s0 = int(sad[by, bx])
        blk = cur[y0:y0 + T, x0:x0 + T].astype(np.int64)
        tex = int(np.abs(blk[:, :-1] - blk[:, 1:]).sum() + np.abs(blk[:-1, :] - blk[1:, :]).sum())
        dy, dx = by - R, bx - R
        iy, ix = abs(dy) < R, abs(dx) < R
        o["dy"], o["dx"], o["sad"], o["texture"] = dy, dx, s0, tex
        o["flags"] = LIVE | (ACCEPTED if (tex >= c["min_texture"] and iy and ix) else 0)
        if iy:
            o["sub_dy"] = subpixel(sad[by - 1, bx], s0, sad[by + 1, bx])
        if ix:
            o["sub_dx"] = subpixel(sad[by, bx - 1], s0, sad[by, bx + 1])
    return out


# ---- stage 3 ---------------------------------------------------------------------------------------------------------------------
def displacement(t, m):
    return -(f8(int(t["dy"])) + f8(t["sub_dy"])) * m, (f8(int(t["dx"])) + f8(t["sub_dx"])) * m


def fit(rows, m):
    """The header's fit over tile rows -> (ok, t_f, t_l, omega)."""
    n = len(rows)
    Sf = Sl = Q = B1 = B2 = B3 = f8(0.0)
    for t in rows:
        f, l = f8(t["f"]), f8(t["l"])
        df, dl = displacement(t, m)
        Sf, Sl, Q = Sf + f, Sl + l, Q + (f * f + l * l)
        B1, B2, B3 = B1 + df, B2 + dl, B3 + (f * dl - l * df)
    if n < 1:
        return False, f8(0.0), f8(0.0), f8(0.0)
    nd = f8(n)
    den = (Q - (Sl * Sl) / nd) - (Sf * Sf) / nd
    if not den > 1e-9 * Q:
        return False, f8(0.0), f8(0.0), f8(0.0)
    om = ((B3 + (Sl * B1) / nd) - (Sf * B2) / nd) / den
    return True, (B1 + om * Sl) / nd, (B2 - om * Sf) / nd, om


def residual2(t, m, tf, tl, om):
    df, dl = displacement(t, m)
    rf, rl = df - (tf - om * f8(t["l"])), dl - (tl + om * f8(t["f"]))
    return rf * rf + rl * rl


def solve(tiles, c):
    """tile table [n_tiles] (the match's fields) -> (motion dict, flags int32 [n_tiles] with the gate and inlier bits, info dict:
    hist (the vote's histogram), res_px (first-fit residuals of the gated tiles in pixels, NaN elsewhere))."""
    R, m, gate = c["search"], f8(c["m_per_px"]), c["gate_px"]
    C1 = 2 * R + 1
    acc = np.array([bool(t["flags"] & ACCEPTED) and abs(int(t["dy"])) <= R and abs(int(t["dx"])) <= R for t in tiles], bool)
    hist = np.zeros(C1 * C1, np.int64)
    for t in tiles[acc]:
        hist[(int(t["dy"]) + R) * C1 + int(t["dx"]) + R] += 1
    flags = tiles["flags"].astype(np.int32) & (ACCEPTED | LIVE)
    mo = dict(t_f=f8(0.0), t_l=f8(0.0), omega=f8(0.0), rms=f8(0.0), n_accepted=int(acc.sum()), n_gated=0, n_inliers=0, valid=0,
              vote_dy=0, vote_dx=0)
    res_px = np.full(len(tiles), np.nan)
    info = dict(hist=hist, res_px=res_px)
    if not acc.any():
        return mo, flags, info
    b = int(np.argmax(hist))                                # the first of equal maxima in row-major order
    my, mx = b // C1 - R, b % C1 - R
    mo["vote_dy"], mo["vote_dx"] = my, mx
    gated = acc & (np.abs(tiles["dy"] - my) <= gate) & (np.abs(tiles["dx"] - mx) <= gate)
    flags[gated] |= GATED
    mo["n_gated"] = int(gated.sum())
    ok1, tf, tl, om = fit(tiles[gated], m)
    if not ok1:
        return mo, flags, info
    thr = f8(c["inlier_px"]) * m
    inl = gated.copy()
    for k in np.nonzero(gated)[0]:
        r2 = residual2(tiles[k], m, tf, tl, om)
        res_px[k] = np.sqrt(r2) / m
        inl[k] = not r2 > thr * thr
    flags[inl] |= INLIER
    mo["n_inliers"] = int(inl.sum())
    ok2, tf, tl, om = fit(tiles[inl], m)
    if not ok2:
        return mo, flags, info
    ss = f8(0.0)
    for t in tiles[inl]:
        ss = ss + residual2(t, m, tf, tl, om)
    mo.update(t_f=tf, t_l=tl, omega=om, rms=np.sqrt(ss / f8(mo["n_inliers"])), valid=int(mo["n_inliers"] >= c["min_inliers"]))
    return mo, flags, info


# ---- stage 4 ---------------------------------------------------------------------------------------------------------------------
def measure(state, mo, c):
    """state: dict(x, y, psi, frames), advanced in place -> (z [4], mode)."""
    use = bool(mo["valid"]) and state["frames"] >= 1
    vx = vy = f8(0.0)
    if use:
        cs, sn = np.cos(f8(state["psi"])), np.sin(f8(state["psi"]))
        Dx, Dy = mo["t_f"] * cs - mo["t_l"] * sn, mo["t_f"] * sn + mo["t_l"] * cs
        state["x"], state["y"], state["psi"] = state["x"] + Dx, state["y"] + Dy, state["psi"] + mo["omega"]
        vx, vy = Dx * f8(c["frame_rate"]), Dy * f8(c["frame_rate"])
    state["frames"] += 1
    return np.array([state["x"], state["y"], vx, vy], f8), 1 if use else 2


class Odometer:
    """One camera of av_egoflow_update on gray patches (update_patch) or frames (update_frame)."""

    def __init__(self, c, cam=None, pose=(0.0, 0.0, 0.0)):
        self.c, self.cam = c, cam
        self.state = dict(x=f8(pose[0]), y=f8(pose[1]), psi=f8(pose[2]), frames=0)
        self.prev = np.zeros((c["gh"], c["gw"]), np.uint8)          # (the device's ping-pong pair starts zero-filled)
        self.tiles = self.motion = self.flags = None

    def update_patch(self, gray, valid):
        self.tiles = match(gray, self.prev, valid, self.c)
        self.motion, self.flags, _ = solve(self.tiles, self.c)
        self.prev = gray
        return measure(self.state, self.motion, self.c)

    def update_frame(self, bgr):
        return self.update_patch(*patch(self.cam, bgr, self.c))

    @property
    def pose(self):
        return np.array([self.state["x"], self.state["y"], self.state["psi"]], f8)
