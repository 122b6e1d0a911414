"""The cases of the ground-odometry tests, shared by tests/test_egoflow_host.py (the NumPy reference against known motion) and
tests/test_gpu_egoflow.py (the device against the reference): a rendered road, hand-made patches and hand-made tile tables."""
import numpy as np

from tests import egoflow_ref as ref

f8 = np.float64

# ---- a road with a fixed smooth texture, seen from above -----------------------------------------------------------------------------
# (d_f, d_l, d_psi): the camera's motion between two frames, metres and radians
KNOWN_MOTIONS = [(0.333, 0.0, 0.0), (0.47, 0.03, 0.01), (0.12, -0.05, -0.02), (0.0, 0.0, 0.0), (0.6, 0.0, 0.015)]
KNOWN_CFG = ref.cfg(gh=128, gw=128, f_far=14.8, m_per_px=0.1, tile=16, search=8)
# the moving block: 32 x 32 patch pixels on the tile grid (tiles (2, 3), (2, 4), (3, 3), (3, 4) of 7 x 7), whose content was
# BLOCK_FLOW = (dy, dx) pixels away in the previous patch -- no rigid motion of the road
BLOCK_AT, BLOCK_FLOW = (40, 56), (5, -4)
BLOCK_TILES = [2 * 7 + 3, 2 * 7 + 4, 3 * 7 + 3, 3 * 7 + 4]

_rng = np.random.default_rng(20240607)
_WAVES = [(_rng.uniform(0.8, 3.0), _rng.uniform(0.0, np.pi), _rng.uniform(0.0, 2 * np.pi), _rng.uniform(10.0, 24.0)) for _ in range(14)]


def world(x, y, seed_shift=0.0):
    """The road's gray level at world point (x, y) metres: a sum of plane waves of 0.8 .. 3 m wavelength -> float64 in about 30 .. 225."""
    v = np.zeros(np.broadcast(x, y).shape)
    for lam, ang, ph, amp in _WAVES:
        v = v + amp * np.sin((2 * np.pi / lam) * (x * np.cos(ang) + y * np.sin(ang)) + ph + seed_shift)
    return 128.0 + v * (95.0 / sum(a for _, _, _, a in _WAVES)) * 2.2


def compose(pose, motion):
    """pose (x, y, psi) of the camera's ground point, moved by (d_f, d_l, d_psi) in its own road frame."""
    x, y, psi = pose
    df, dl, dpsi = motion
    return (x + df * np.cos(psi) - dl * np.sin(psi), y + df * np.sin(psi) + dl * np.cos(psi), psi + dpsi)


def patch_points(c):
    """-> (f [gh, 1], l [1, gw]): the road point of every patch pixel."""
    f = (c["f_far"] - (np.arange(c["gh"]) + 0.5) * c["m_per_px"])[:, None]
    l = (((np.arange(c["gw"]) + 0.5) - c["gw"] / 2.0) * c["m_per_px"])[None, :]
    return f, l


def render_patch(pose, c, seed_shift=0.0):
    """The gray bird's-eye patch a camera at `pose` sees of world(): uint8 [gh, gw]."""
    f, l = patch_points(c)
    x, y, psi = pose
    wx = x + f * np.cos(psi) - l * np.sin(psi)
    wy = y + f * np.sin(psi) + l * np.cos(psi)
    return np.clip(np.rint(world(wx, wy, seed_shift)), 0, 255).astype(np.uint8)


def patch_pair(motion, c=KNOWN_CFG, pose=(3.0, -2.0, 0.3), block=False):
    """-> (prev, cur): the patches before and after `motion`; block: a 32 x 32 block of another texture that moves by BLOCK_FLOW."""
    prev, cur = render_patch(pose, c), render_patch(compose(pose, motion), c)
    if block:
        other = render_patch((40.0, 17.0, 1.1), c, seed_shift=1.7)          # another piece of road
        (by, bx), (fy, fx) = BLOCK_AT, BLOCK_FLOW
        cur, prev = cur.copy(), prev.copy()
        cur[by:by + 32, bx:bx + 32] = other[by:by + 32, bx:bx + 32]
        prev[by + fy:by + fy + 32, bx + fx:bx + fx + 32] = other[by:by + 32, bx:bx + 32]
    return prev, cur


# ---- hand-made patches for the match stage --------------------------------------------------------------------------------------------
MATCH_GEOMS = [dict(gh=48, gw=64, tile=8, search=4), dict(gh=48, gw=50, tile=8, search=4)]      # 5 x 7 = 35 and 5 x 5 = 25 tiles
MATCH_SHIFTS = [(-2.3, 1.4), (2.75, -2.5), (0.0, 0.0)]          # camera k: cur(y, x) = texture(y + sy, x + sx), prev = texture(y, x)
# tile indices (ty * tiles_x + tx) of the hand-made kinds, valid in both geometries' grids by (ty, tx)
MATCH_KINDS = dict(flat=(1, 1), border=(2, 3), tie=(3, 1), invalid=(0, 4))


def _texture(rng):
    """A smooth random float texture: tex(y, x) at any (fractional) patch position."""
    waves = [(rng.uniform(5.0, 14.0), rng.uniform(0.0, np.pi), rng.uniform(0.0, 2 * np.pi), rng.uniform(12.0, 30.0)) for _ in range(10)]

    def tex(y, x):
        v = np.zeros(np.broadcast(y, x).shape)
        for lam, ang, ph, amp in waves:
            v = v + amp * np.sin((2 * np.pi / lam) * (y * np.cos(ang) + x * np.sin(ang)) + ph)
        return 128.0 + v * 0.55
    return tex


def match_case(geom, n_cams=3, seed=0):
    """-> (cfg, cur uint8 [n, gh, gw], prev, valid bool [n, gh, gw], kinds: name -> tile index).  Camera k's road moves by
    MATCH_SHIFTS[k]; on top, in every camera: a flat tile, a tile whose best match is on the search border, a tile with two equal
    minima, and invalid pixels beside one tile's neighbourhood and inside another's."""
    c = ref.cfg(f_far=10.0, m_per_px=0.1, **geom)
    gh, gw, T, R = c["gh"], c["gw"], c["tile"], c["search"]
    ty, tx = ref.tile_grid(c)
    rng = np.random.default_rng(77 + seed)
    yy, xx = np.mgrid[0:gh, 0:gw].astype(f8)
    cur = np.zeros((n_cams, gh, gw), np.uint8)
    prev = np.zeros_like(cur)
    valid = np.ones((n_cams, gh, gw), bool)
    kinds = {k: v[0] * tx + v[1] for k, v in MATCH_KINDS.items()}
    origin = lambda k: (R + (k // tx) * T, R + (k % tx) * T)                # noqa: E731
    for k in range(n_cams):
        tex = _texture(rng)
        sy, sx = MATCH_SHIFTS[k % len(MATCH_SHIFTS)]
        prev[k] = np.clip(np.rint(tex(yy, xx)), 0, 255)
        cur[k] = np.clip(np.rint(tex(yy + sy, xx + sx)), 0, 255)
        # flat: the tile and its whole neighbourhood in prev are one gray level (texture 0; every candidate's SAD equal)
        y0, x0 = origin(kinds["flat"])
        cur[k, y0:y0 + T, x0:x0 + T] = 90
        prev[k, y0 - R:y0 + T + R, x0 - R:x0 + T + R] = 90
        # border: the tile shows what prev has R rows further down, exactly
        y0, x0 = origin(kinds["border"])
        noise = rng.integers(0, 256, (T + 2 * R, T + 2 * R)).astype(np.uint8)
        prev[k, y0 - R:y0 + T + R, x0 - R:x0 + T + R] = noise
        cur[k, y0:y0 + T, x0:x0 + T] = noise[2 * R:2 * R + T, R:R + T]                  # (dy, dx) = (R, 0)
        # tie: a pattern of period 4 along x (random along y) lies in prev one row down over 14 columns, in noise: SAD 0 at
        # (dy, dx) = (1, -3) and (1, 1), and the first wins
        y0, x0 = origin(kinds["tie"])
        noise = rng.integers(0, 256, (T + 2 * R, T + 2 * R)).astype(np.uint8)
        pat = rng.integers(0, 256, (T, 4)).astype(np.uint8)
        strip = np.tile(pat, (1, 4))[:, :T + 2 * R - 2]                                 # [T, 14]: columns 1 .. 14 of the window
        noise[R + 1:R + 1 + T, 1:1 + strip.shape[1]] = strip
        prev[k, y0 - R:y0 + T + R, x0 - R:x0 + T + R] = noise
        cur[k, y0:y0 + T, x0:x0 + T] = strip[:, :T]
        # invalid: one pixel just right of tile (0, 4)'s neighbourhood (the tile stays live) in camera 0; its last column in the
        # others (the tile, and its right neighbour if there is one, are not live)
        y0, x0 = origin(kinds["invalid"])
        valid[k, y0 + 3, x0 + T + R - (0 if k == 0 else 1)] = False                     # (x0 + T + R < gw in both geometries)
    return c, cur, prev, valid, kinds


# ---- hand-made tile tables for the solve stage ------------------------------------------------------------------------------------------
SOLVE_CFG = ref.cfg(gh=128, gw=136, f_far=16.0, m_per_px=0.1, tile=8, search=4, min_inliers=8)     # 15 x 16 = 240 tiles


def _grid_table(c):
    ty, tx = ref.tile_grid(c)
    t = np.zeros(ty * tx, np.dtype(ref.TILE_FIELDS))
    T, R, m = c["tile"], c["search"], c["m_per_px"]
    k = np.arange(ty * tx)
    t["f"] = c["f_far"] - ((R + (k // tx) * T) + T / 2.0) * m
    t["l"] = (((R + (k % tx) * T) + T / 2.0) - c["gw"] / 2.0) * m
    return t


def _flow_table(c, motion, rng, outliers=0, drop=0.0, noise=0.02):
    """A tile table as the match would leave it for a road moving under `motion` = (t_f, t_l, omega): every tile's displacement
    d = t + omega J p plus `noise` px of scatter, split into the integer best and the sub-pixel offset."""
    t = _grid_table(c)
    m = c["m_per_px"]
    tf, tl, om = motion
    dy = -(tf - om * t["l"]) / m + rng.normal(0.0, noise, len(t))
    dx = (tl + om * t["f"]) / m + rng.normal(0.0, noise, len(t))
    t["dy"], t["dx"] = np.rint(dy), np.rint(dx)
    t["sub_dy"], t["sub_dx"] = dy - t["dy"], dx - t["dx"]
    t["flags"] = ref.LIVE | ref.ACCEPTED
    t["sad"], t["texture"] = 100, 1000
    t["flags"][rng.random(len(t)) < drop] = ref.LIVE                # textureless tiles
    for i, k in enumerate(rng.choice(len(t), outliers, replace=False)):     # other vehicles, flows of their own: inside the vote's
        if i % 2:                                                           # gate (the fit has to reject them) and outside it
            t["dy"][k], t["dx"][k] = t["dy"][k] + rng.integers(1, 3), t["dx"][k] - rng.integers(1, 3)
        else:
            t["dy"][k] = 3 if t["dy"][k] < 0 else -4
    return t


def solve_cases():
    """-> list of (name, tile table [240]) for SOLVE_CFG."""
    c, rng = SOLVE_CFG, np.random.default_rng(5)
    out = [("straight", _flow_table(c, (0.21, 0.0, 0.0), rng, outliers=9, drop=0.2)),
           ("turn", _flow_table(c, (0.17, 0.02, 0.012), rng, outliers=14, drop=0.3)),
           ("reverse_turn", _flow_table(c, (-0.11, -0.03, -0.02), rng, outliers=5))]
    t = _grid_table(c)                                              # tied vote, integer flows only: 60 tiles each at (1, 2) and
    t["flags"] = ref.LIVE                                           # (-1, 2); the first in row-major order, (-1, 2), is the mode
    t["flags"][0:60], t["dy"][0:60], t["dx"][0:60] = ref.LIVE | ref.ACCEPTED, 1, 2
    t["flags"][100:160], t["dy"][100:160], t["dx"][100:160] = ref.LIVE | ref.ACCEPTED, -1, 2
    out.append(("tied_vote", t))
    t = _grid_table(c)                                              # nothing accepted
    t["flags"] = ref.LIVE
    out.append(("none_accepted", t))
    t = _flow_table(c, (0.2, 0.0, 0.0), rng)                        # five tiles: fewer than min_inliers
    t["flags"][5:] = ref.LIVE
    out.append(("too_few", t))
    t = _flow_table(c, (0.2, 0.0, 0.0), rng)                        # one tile: the fit is singular
    t["flags"][:17] = ref.LIVE
    t["flags"][18:] = ref.LIVE
    out.append(("singular", t))
    return out


# ---- rendered camera frames -------------------------------------------------------------------------------------------------------
def render_frame(cal, h, w, pose, rng=None):
    """The frame a camera with calibration `cal` at `pose` takes of world(): uint8 [h, w, 3] (b, g, r all the road's gray, the sky
    -- pixels at or above the horizon -- noise or 200)."""
    g = np.asarray(cal.g, f8).reshape(3, 3)
    v, u = np.mgrid[0:h, 0:w].astype(f8)
    F, L, D = (g[i, 0] * u + g[i, 1] * v + g[i, 2] for i in range(3))
    road = D > 0.0
    Ds = np.where(road, D, 1.0)
    f, l = F / Ds, L / Ds
    x, y, psi = pose
    gray = world(x + f * np.cos(psi) - l * np.sin(psi), y + f * np.sin(psi) + l * np.cos(psi))
    sky = rng.integers(0, 256, (h, w)) if rng is not None else np.full((h, w), 200)
    img = np.where(road, np.clip(np.rint(gray), 0, 255), sky).astype(np.uint8)
    return np.repeat(img[..., None], 3, axis=2)
