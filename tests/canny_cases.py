"""Hand-made u8 gray images for the lane detector's pixel stages (pure NumPy, no GPU, no files): inputs of the given-gray entry
of av_lane_detect (stage bit 64: image in workspace view 0, thresholds in view 4) and, with b = g = r, of the BGR front ends.
tests/test_canny_cases_host.py proves with the oracle alone that every case is what its claim says; tests/test_gpu_canny_cases.py
compares the device with the oracle on them, exactly.

What the geometry rests on (oracle/c/lane_ref.c, cv::Canny with L2gradient = False):
  * a straight step of contrast c has |gx| + |gy| = 4 c on the two pixels next to it, and of two equal neighbours along the
    gradient non-maximum suppression keeps the first (upper / left) one: the step between rows y - 1 (one level) and y (another)
    leaves its candidates on row y - 1, a step between columns x - 1 and x on column x - 1, whichever side is brighter;
  * a step whose row drops by one at some column leaves a chain that continues through ONE diagonal pair of pixels;
  * contrast 20 (magnitude 80) is weak and contrast 150 (600) is strong for the thresholds 50 / 150 used here.
A `Case` is (name, image, lo, hi, claim); claim["kind"] says which statement the host test proves:
  "lit"      the edge map has >= min_pixels pixels in >= min_tiles distinct 16 x 256 tiles (and >= min_far inside claim["far"])
  "dark"     the edge map is empty although the image has >= min_candidates candidates
  "cut"      nothing survives inside claim["far"] although there are candidates there; the seed's side is lit
  "same_as"  the edge map equals the oracle's for claim["image"] (a contour that must vanish leaves no trace)
  "verdict"  inside claim["probe"] the edge map is all set (keep = True) or all clear
  "wedge"    the edge map is non-empty, its pixels inside the ramp have the claimed direction class, and a suppression with the
             class boundary moved past the ramp's direction (or with the other diagonal's neighbours) keeps other pixels
  "classes"  the edge map's pixels cover every direction class, and moved class boundaries change it
  "ties"     plateaus of equal magnitudes along every outline: the edge map is non-empty
  "borders"  the edge map has pixels on row 0, row h - 1, column 0 and column w - 1
"""
import collections
import functools

import numpy as np

SHAPES = ((64, 32), (100, 528), (90, 300), (75, 333), (40, 16), (9, 8))
TILE_R, TILE_C = 16, 256                    # hysteresis tile of csrc/lane.hip
LO, HI = 50, 150
BG, WEAK, SEED = 100, 120, 250              # gray levels: contrast 20 is weak, 150 strong
# the same structures through the BGR front ends (b = g = r, so gray = the level): the background is the larger part of every
# frame, so the median is 100 and lo, hi = 70, 130; after the 5 x 5 blur a straight step of contrast c has magnitude 2.5 c, a
# corner up to sqrt(2) times that (|gx| + |gy|): contrast 32 gives 80 .. 116, weak everywhere
BGR_BG, BGR_WEAK, BGR_SEED = 100, 132, 250

Case = collections.namedtuple("Case", "name image lo hi claim")


def tiles_of(mask):
    """The distinct 16 x 256 tiles that hold a set pixel of `mask`."""
    ys, xs = np.nonzero(mask)
    return set(zip((ys // TILE_R).tolist(), (xs // TILE_C).tolist()))


def roi_rows_full(shape):
    h, w = shape
    return np.tile(np.array([0, w - 1], np.int32), (h, 1))


def roi_rows_handmade(shape):
    """Per-row inclusive [xl, xr]: a band that wanders over the frame, every 5th row empty (xl > xr), every 7th a single column,
    every 11th the whole row."""
    h, w = shape
    rows = np.zeros((h, 2), np.int32)
    for y in range(h):
        xl = (y * 7) % max(w // 2, 1)
        xr = min(w - 1, xl + w // 3 + (y * 13) % max(w // 4, 1))
        if y % 5 == 2:
            xl, xr = (xr, xl) if xr > xl else (1, 0)        # empty: xl > xr, both inside the frame
        elif y % 7 == 3:
            xr = xl
        elif y % 11 == 0:
            xl, xr = 0, w - 1
        rows[y] = xl, xr
    return rows


def mask_rows(edges, rows):
    """`edges` with everything outside the inclusive per-row ranges cleared: the oracle's statement of a caller-defined ROI."""
    x = np.arange(edges.shape[1])[None, :]
    return np.where((x >= rows[:, :1]) & (x <= rows[:, 1:]), edges, 0).astype(np.uint8)


def seed_block(level):
    """-> seed(img, region, y, x, vertical): a 4 x 4 block of `level` with its top-left corner at (y, x)."""
    def seed(img, region, y, x, vertical=False):
        assert y >= 0 and x >= 0 and y + 4 <= img.shape[0] and x + 4 <= img.shape[1]
        img[y:y + 4, x:x + 4] = level
    return seed


def seed_tapered(level, taper, floor):
    """-> seed(img, region, y, x, vertical): the same 4 x 4 block, continued along the chain it sits on (along the row, or down the
    column with `vertical`) in both directions by a level that falls by `taper` per pixel down to `floor`; only pixels of `region`
    are touched and none is lowered.  After a blur an abrupt end of the seed would turn the gradient there and non-maximum
    suppression would open a gap between the seed and the chain."""
    def seed(img, region, y, x, vertical=False):
        n = -(-(level - floor) // taper)
        for i in range(-n, 4 + n):
            lv = level - taper * (-i if i < 0 else max(0, i - 3))
            for j in range(4):
                yy, xx = (y + i, x + j) if vertical else (y + j, x + i)
                if 0 <= yy < img.shape[0] and 0 <= xx < img.shape[1] and region[yy, xx]:
                    img[yy, xx] = max(int(img[yy, xx]), lv)
    return seed


# ---- long chains -----------------------------------------------------------------------------------------------------------------
def _serp_geometry(shape, thick=None):
    """(margin, thickness, pitch, runs) of the serpentine band, or None when the frame cannot hold two runs."""
    h, w = shape
    m, t, p = (4, 8, 24) if w >= 32 and h >= 60 else (3, 4, 12)
    if w < 2 * m + 2 * t + 2:
        return None
    n = (h - 2 * m - t) // p + 1
    return (m, thick or t, p, n) if n >= 2 else None


def serpentine(shape, where, bg=BG, weak=WEAK, seed=seed_block(SEED), thick=None):
    """A band `t` thick that runs right, down, left, down ... over the whole frame; `where`: the seed at the "first" or "last"
    corner or in the "middle" (inside the band, flush with its outline), or None.  -> (image, band mask) or None."""
    geo = _serp_geometry(shape, thick)
    if geo is None:
        return None
    h, w = shape
    m, t, p, n = geo
    band = np.zeros(shape, bool)
    for k in range(n):
        r = m + k * p
        band[r:r + t, m:w - m] = True
        if k + 1 < n:
            c = w - m - t if k % 2 == 0 else m
            band[r:r + p + t, c:c + t] = True
    img = np.where(band, weak, bg).astype(np.uint8)
    if where == "first":
        seed(img, band, m, m)
    elif where == "last":
        seed(img, band, m + (n - 1) * p + t - 4, (w - m - 4) if (n - 1) % 2 == 0 else m)
    elif where == "middle":
        seed(img, band, m + (n // 2) * p, w // 2 - 2)
    else:
        assert where is None
    return img, band


def _thick_path(shape, pts, t):
    """Mask of the rectilinear path through `pts` ((y, x) of the top-left corner of a t x t pen)."""
    mask = np.zeros(shape, bool)
    for (y0, x0), (y1, x1) in zip(pts[:-1], pts[1:]):
        mask[min(y0, y1):max(y0, y1) + t, min(x0, x1):max(x0, x1) + t] = True
    return mask


def interleaved(shape, seed_a=True, with_b=True, with_a=True, seed_b=False):
    """Two serpentines 4 px thick that run 3 px apart for their whole length: A, and B on A's one side all the way (inside A's
    right turns, around the outside of its left turns).  -> image or None."""
    h, w = shape
    t, g = 4, 3
    d, P = t + g, 3 * (t + g) + 1
    ya, xa, xb = 3, d + 3, w - 3 - t
    n = (h - ya - t - d - 3) // P + 1                 # A's runs; B's last run may lie d below A's
    if n < 2 or xb - d - xa < 2 * t:
        return None
    a_pts, b_pts = [], []
    for k in range(n):
        y = ya + k * P
        a_pts += [(y, xa), (y, xb)] if k % 2 == 0 else [(y, xb), (y, xa)]
        yb = y + d if k % 2 == 0 else y - d
        b_pts += [(yb, xa if k == 0 else xa - d), (yb, xb - d)] if k % 2 == 0 else [(yb, xb - d), (yb, xa - d)]
    a, b = _thick_path(shape, a_pts, t), _thick_path(shape, b_pts, t)
    assert not (a & b).any()
    img = np.full(shape, BG, np.uint8)
    if with_a:
        img[a] = WEAK
        if seed_a:
            seed_block(SEED)(img, a, ya, xa)
    if with_b:
        img[b] = WEAK
        if seed_b:
            seed_block(SEED)(img, b, ya + d, xa)
    return img


# ---- seams -----------------------------------------------------------------------------------------------------------------------
def seam_row(shape):
    """The tile seam row 16 k the seam cases use: the first one at or below 0.6 h (inside the default ROI's rows)."""
    h = shape[0]
    y = -(-int(h * 0.6) // TILE_R) * TILE_R
    return y if y + 8 <= h else None


def _placements(shape):
    """name -> (y, x) of the lower pixel of the step: on a horizontal seam, on the vertical seam 255 / 256, on the tile corner."""
    h, w = shape
    ys = seam_row(shape)
    out = {}
    if ys is None or w < 16:
        return out
    out["hseam"] = (ys, w // 2 + w // 10)
    if w >= TILE_C + 24:
        out["vseam"] = (ys + 5, TILE_C)
        out["corner"] = (ys, TILE_C)
    return out


def jog(shape, y, x, mirror, cut, bg=BG, weak=WEAK, seed=seed_block(SEED), slot=2):
    """A half plane (weak level below) whose upper outline steps down by one row: its candidates are row y - 1 left of the step
    and row y right of it, joined by the single diagonal pair (y - 1, x - 1) -> (y, x); mirrored: row y left of the step, row
    y - 1 right of it, (y, x - 1) -> (y - 1, x).  The seed sits at the left end.  `cut`: the plane lacks the columns x ..
    x + slot - 1, the step's own: the left part's outline turns down along column x - 1 and the right part starts beyond the slot.
    -> (image, far mask: from the slot's last column on, gap mask: the slot)."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    plane = yy >= (np.where(xx < x - 1, y + 1, y) if mirror else np.where(xx < x + 1, y, y + 1))
    gap = (xx >= x) & (xx < x + slot)
    if cut:
        plane &= ~gap
    img = np.where(plane, weak, bg).astype(np.uint8)
    seed(img, plane, y + 1 if mirror else y, 0)
    return img, xx >= x + slot, gap


def jog_down(shape, y, x, mirror, cut, **kw):
    """jog() transposed: a chain that runs down the frame, on column x - 1 above the step and on column x below it (mirrored: x
    and x - 1), through the same diagonal pair; the seed at the top, the cut a slot of the rows y .. y + slot - 1."""
    img, far, gap = jog(shape[::-1], x, y, mirror, cut, **kw)
    return np.ascontiguousarray(img.T), far.T, gap.T


def straight(shape, y, x, vertical, cut, bg=BG, weak=WEAK, seed=seed_block(SEED), slot=2):
    """A chain that crosses a seam by a 4-connected step.  vertical: the outline of the half plane right of column x (candidates
    on column x - 1, every row) crossing the seam above row y, seed at the top, cut by a slot of the rows y .. y + slot - 1; else the
    outline of the half plane below row y (candidates on row y - 1) crossing the seam left of column x, seed at the left end, cut
    by a slot of the columns x .. x + slot - 1.  -> (image, far mask, gap mask: the slot)."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    plane = (xx >= x) if vertical else (yy >= y)
    gap = ((yy >= y) & (yy < y + slot)) if vertical else ((xx >= x) & (xx < x + slot))
    if cut:
        plane &= ~gap
    img = np.where(plane, weak, bg).astype(np.uint8)
    if vertical:
        seed(img, plane, 0, x, vertical=True)
    else:
        seed(img, plane, y, 0)
    return img, (yy >= y + slot) if vertical else (xx >= x + slot), gap


L_ARM = 160        # columns of the L's horizontal arm


def corner_l(shape, y, x, cut, bg=BG, weak=WEAK, seed=seed_block(SEED), slot=2):
    """The outline of the rectangle rows 0 .. y, columns x - L_ARM .. x: an L with a 4-connected corner pixel at (y, x), candidates
    on column x for rows <= y and on row y for columns <= x.  With (y, x) = (16 k, 256) the L passes three tiles around the tile
    corner: (16 k - 1, 256) above the horizontal seam, (16 k, 256), and (16 k, 255) left of the vertical seam -- which is also the
    diagonal neighbour of the first.  Seed at the top of the column.  `cut`: a tab of the same level, columns x - slot .. x, hangs
    from the rectangle to the frame's last row: column x's outline runs straight on and the arm starts left of the tab.
    -> (image, far mask: the arm (and the tab's outline) left of the tab, gap mask: the tab's columns left of column x)."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    rect = (yy <= y) & (xx <= x) & (xx >= x - L_ARM)
    if cut:
        rect |= (xx >= x - slot) & (xx <= x) & (yy > y)
    img = np.where(rect, weak, bg).astype(np.uint8)
    seed(img, rect, 0, x - 3, vertical=True)
    return img, (xx < x - slot) & (yy >= y), (xx >= x - slot) & (xx < x) & (yy >= y)


# ---- dense -----------------------------------------------------------------------------------------------------------------------
def dense(shape, seed, everywhere):
    """Slanted one-pixel stripes (level 140 on 100) of period 4 whose phase moves by one column every third row: every second
    pixel of a row is a candidate of magnitude 160 and the rows where the phase moves tie all of them into one component by
    diagonal steps.  The largest magnitude is 240 (first and last column), so with hi = DENSE_HI nothing is strong.  everywhere: the
    whole frame, else rows 16 .. 31 (one tile row) -- the stripes above and below are at level 110, magnitude 40, no candidates.
    Seed: ONE pixel of a stripe raised by 50, which lifts the candidates left and right of it to 260."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    peak = np.full(shape, 140)
    if not everywhere and h >= 48:
        peak[:TILE_R] = 110
        peak[2 * TILE_R:] = 110
    img = np.where((xx + yy // 3) % 4 == 2, peak, BG).astype(np.uint8)
    if seed:
        y0 = (TILE_R + 8 if h >= 48 else h // 6 * 3) + 1            # the middle row of three of one phase
        col = [x for x in range(w // 2, w // 2 + 4) if img[y0, x] == 140][0]
        assert img[y0 - 1, col] == 140 and img[y0 + 1, col] == 140
        img[y0, col] += 50
    return img


DENSE_HI = 240


# ---- threshold equalities ----------------------------------------------------------------------------------------------------------
def step(shape, contrast=20, seed=False):
    """A vertical step of `contrast` at the middle column (magnitude 4 * contrast on column x - 1, after the tie rule), optionally
    with a 3 x 3 strong seed at its top.  -> (image, probe mask: the step's column away from the seed and the frame's ends)."""
    h, w = shape
    x = w // 2
    img = np.full(shape, BG, np.uint8)
    img[:, x:] = BG + contrast
    if seed:
        img[0:3, x:x + 3] = SEED
    probe = np.zeros(shape, bool)
    probe[5:h - 1, x - 1] = True
    return img, probe


STEP_CASES = (          # name, lo, hi, seed, the step is kept        (magnitude m = 80)
    ("m_eq_lo", 80, 300, True, False),              # a candidate needs m > lo
    ("m_eq_lo_plus_1", 79, 300, True, True),
    ("m_eq_hi", 50, 80, False, False),              # strong needs m > hi
    ("m_eq_hi_plus_1", 50, 79, False, True),
    ("lo_eq_hi_below_m", 79, 79, False, True),
    ("lo_eq_hi_eq_m", 80, 80, False, False),
    ("lo_zero", 0, 79, False, True),
    ("lo_zero_weak", 0, 80, False, False),
    ("swapped_keep", 79, 50, False, True) ,         # lo > hi: both sides swap them
    ("swapped_weak_seeded", 300, 79, True, True),
    ("swapped_drop", 300, 80, True, False),
)


# ---- direction classes and ties ------------------------------------------------------------------------------------------------------
WEDGES = ((5, 2), (12, 5), (5, 12), (2, 5))     # (a, b): |gy| / |gx| = b / a sits just below / above tan 22.5, below / above tan 67.5


def wedge(shape, a, b, sy):
    """The ramp a x + sy b y clipped to 10 .. 250: inside the ramp gx = 8 a, gy = 8 sy b exactly and the magnitude is the plateau
    8 (a + b), which falls off at the two clip lines.  Non-maximum suppression drops the plateau's inside (equal neighbours) and
    keeps its first line along the gradient: those pixels are compared with neighbours chosen by the direction class, so with
    hi = 8 (a + b) - 1 they are the strong pixels of the edge map, and lo = 4 (a + b) lets the fall-off's candidates join them.
    -> (image, lo, hi)."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(130 + a * (xx - w // 2) + sy * b * (yy - h // 2), 10, 250).astype(np.uint8), 4 * (a + b), 8 * (a + b) - 1


# a tan 22.5 constant (x 2^15; the oracle's and the kernels' is 13573) that moves the wedge's direction into the neighbouring class
WEDGE_MOVED_TG22 = {(5, 2): 13000, (12, 5): 13700, (5, 12): 13000, (2, 5): 16500}
CONE_LO, CONE_HI = 20, 40


def nms(img, lo, tg22=13573, swap_diagonals=False):
    """The candidates cv::Canny's non-maximum suppression keeps (magnitude above lo, a maximum along its direction class), restated
    in NumPy with the tan 22.5 constant and the choice of the diagonal as parameters: what a kernel with a moved class boundary,
    or one that takes the other diagonal's neighbours, would keep."""
    _, gx, gy = sobel_classes(img, 0)
    m = np.pad(np.abs(gx) + np.abs(gy), 1)
    c = m[1:-1, 1:-1]
    ax, ay = np.abs(gx), np.abs(gy) << 15
    t22 = ax * tg22
    t67 = t22 + (ax << 16)
    horiz = (c > m[1:-1, :-2]) & (c >= m[1:-1, 2:])
    vert = (c > m[:-2, 1:-1]) & (c >= m[2:, 1:-1])
    same = (c > m[:-2, :-2]) & (c > m[2:, 2:])                 # gx, gy of equal signs: neighbours (y - 1, x - 1), (y + 1, x + 1)
    opp = (c > m[:-2, 2:]) & (c > m[2:, :-2])
    neg = ((gx ^ gy) < 0) != swap_diagonals
    return (c > lo) & np.where(ay < t22, horiz, np.where(ay > t67, vert, np.where(neg, opp, same)))


def cone(shape):
    """A cone, 5 gray levels per pixel of radius: every gradient direction."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.sqrt((yy - h / 2.0 + 0.25) ** 2 + (xx - min(w, 2 * h) / 2.0 + 0.25) ** 2)
    return np.clip(220 - np.floor(5 * r), 40, 220).astype(np.uint8)


def terraces(shape):
    """Plateaus: steps of 37 every 7 rows and of 53 every 5 columns -- equal neighbouring magnitudes along every outline."""
    h, w = shape
    return ((np.arange(h)[:, None] // 7 * 37 + np.arange(w)[None, :] // 5 * 53) % 256).astype(np.uint8)


def sobel_classes(img, lo):
    """Direction class (0 horizontal, 1 vertical, 2 diagonal of equal signs, 3 diagonal of opposite signs; -1 where the magnitude is
    not above lo) with the oracle's integer rule; also gx and gy."""
    p = np.pad(img.astype(np.int64), 1, mode="edge")
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    ax, ay = np.abs(gx), np.abs(gy) << 15
    tg22 = ax * 13573
    tg67 = tg22 + (ax << 16)
    cls = np.where(ay < tg22, 0, np.where(ay > tg67, 1, np.where((gx ^ gy) < 0, 3, 2)))
    return np.where(ax + np.abs(gy) > lo, cls, -1), gx, gy


# ---- borders -------------------------------------------------------------------------------------------------------------------------
def frame_rings(shape):
    """Outermost ring 140, the next 100, the inside 120: the magnitude on the outermost ring (4 * 40) beats the one inside it
    (4 * 20), so the edge pixels lie on row 0, row h - 1, column 0 and column w - 1."""
    img = np.full(shape, 120, np.uint8)
    img[[0, -1], :] = 140
    img[:, [0, -1]] = 140
    img[1, 1:-1] = img[-2, 1:-1] = 100
    img[1:-1, 1] = img[1:-1, -2] = 100
    return img


# ---- the case list -------------------------------------------------------------------------------------------------------------------
def _chain_cases(shape, bg, weak, seed, slot, thick=None):
    """Serpentines and seams at the given levels, seed and slot width: (name, image, claim); the thresholds are the caller's."""
    h, w = shape
    kw = dict(bg=bg, weak=weak, seed=seed)
    out = []
    geo = _serp_geometry(shape, thick)
    if geo is not None:
        m, t, p, n = geo
        band = serpentine(shape, None, thick=thick, **kw)[1]
        # both outlines of every run, less the turns: a lower bound that needs the whole contour lit
        lit = dict(kind="lit", min_pixels=2 * n * (w - 2 * m - 2 * t), min_tiles=len(tiles_of(band)), far=None, min_far=0)
        for s in ("first", "last", "middle"):
            out.append(("serpentine_seed_" + s, serpentine(shape, s, thick=thick, **kw)[0], lit))
        out.append(("serpentine_no_seed", serpentine(shape, None, thick=thick, **kw)[0], dict(kind="dark", min_candidates=lit["min_pixels"])))

    def pair(tag, build, min_pixels, min_tiles, min_far, seam, **extra):
        """The chain and its cut twin."""
        img, far, gap = build(False)
        out.append((tag, img, dict(kind="lit", min_pixels=min_pixels, min_tiles=min_tiles, far=far, min_far=min_far, **extra)))
        img, far, gap = build(True)
        out.append((tag + "_cut", img, dict(kind="cut", far=far, min_far=min_far, gap=gap, seam=seam)))

    pls = _placements(shape)
    for pl, (y, x) in pls.items():
        for mirror in (False, True):
            tag = "seam_diag_%s%s" % (pl, "_mirror" if mirror else "")
            if pl == "hseam":           # down the frame, across the row seam; the cut's gap is rows y .. y + slot - 1
                pair(tag, lambda cut: jog_down(shape, y, x, mirror, cut, slot=slot, **kw), h - 8, 2, h - y - slot - 3, ("row", y),
                     step=(y, x, mirror))
            else:                       # along the frame, across the column seam; the gap is columns 256 .. 256 + slot - 1
                pair(tag, lambda cut: jog(shape, y, x, mirror, cut, slot=slot, **kw), w - 8, 2, w - x - slot - 8, ("col", x),
                     step=(y, x, mirror))
    if "hseam" in pls:
        y, x = pls["hseam"]
        pair("seam_4conn_hseam", lambda cut: straight(shape, y, x, True, cut, slot=slot, **kw), h - 8, 2, h - y - slot - 3, ("row", y))
    if "vseam" in pls:
        y, x = pls["vseam"]
        pair("seam_4conn_vseam", lambda cut: straight(shape, y, x, False, cut, slot=slot, **kw), w - 8, 2, w - x - slot - 3, ("col", x))
        y, x = pls["corner"]
        pair("seam_4conn_corner", lambda cut: corner_l(shape, y, x, cut, slot=slot, **kw), y + L_ARM - 8, 3, L_ARM - slot - 6,
             ("col", x - 1))
    return out


@functools.lru_cache(maxsize=None)
def cases(shape):
    """Every given-gray case that fits a frame of `shape`, as a tuple of Case."""
    h, w = shape
    out = [Case(n, i, LO, HI, c) for n, i, c in _chain_cases(shape, BG, WEAK, seed_block(SEED), 2)]
    both = interleaved(shape)
    if both is not None:
        out.append(Case("interleaved_one_seeded", both, LO, HI,
                        dict(kind="same_as", image=interleaved(shape, with_b=False), other=interleaved(shape, with_a=False, seed_b=True))))
        out.append(Case("interleaved_no_seed", interleaved(shape, seed_a=False), LO, HI, dict(kind="dark", min_candidates=4 * w)))
    if h >= 16 and w >= 16:
        n_tile = min(h, TILE_R) * min(w, TILE_C) if h < 48 else TILE_R * min(w, TILE_C)
        out.append(Case("dense_one_tile", dense(shape, True, False), LO, DENSE_HI,
                        dict(kind="lit", min_pixels=int(0.45 * n_tile), min_tiles=1, far=None, min_far=0)))
        full = np.ones(shape, bool)
        out.append(Case("dense_every_tile", dense(shape, True, True), LO, DENSE_HI,
                        dict(kind="lit", min_pixels=int(0.45 * h * w), min_tiles=len(tiles_of(full)), far=None, min_far=0)))
        out.append(Case("dense_no_seed", dense(shape, False, True), LO, DENSE_HI, dict(kind="dark", min_candidates=int(0.45 * h * w))))
    for name, lo, hi, seed, keep in STEP_CASES:
        img, probe = step(shape, 20, seed)
        out.append(Case("step_" + name, img, lo, hi, dict(kind="verdict", probe=probe, keep=keep)))
    for a, b in WEDGES:
        for sy in (1, -1):
            img, lo, hi = wedge(shape, a, b, sy)
            cl = {(5, 2): 0, (12, 5): 2, (5, 12): 2, (2, 5): 1}[a, b]
            out.append(Case("wedge_%d_%d_%s" % (a, b, "pos" if sy > 0 else "neg"), img, lo, hi,
                            dict(kind="wedge", ab=(a, b), sy=sy, cls=3 if cl == 2 and sy < 0 else cl)))
    out.append(Case("cone", cone(shape), CONE_LO, CONE_HI, dict(kind="classes", want=(0, 1, 2, 3))))
    out.append(Case("terraces", terraces(shape), LO, HI, dict(kind="ties")))
    out.append(Case("frame_rings", frame_rings(shape), LO, HI, dict(kind="borders")))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert c.image.shape == shape and c.image.dtype == np.uint8
        c.image.setflags(write=False)
    return tuple(out)


def names(shape):
    return [c.name for c in cases(shape)]


def case(shape, name):
    return next(c for c in cases(shape) if c.name == name)


def all_ids():
    """[(shape, name)] over SHAPES, and the matching pytest ids."""
    pairs = [(s, n) for s in SHAPES for n in names(s)]
    return pairs, ["%dx%d-%s" % (s[0], s[1], n) for s, n in pairs]


# ---- the same chains through the BGR front ends -------------------------------------------------------------------------------------
BGR_SHAPES = ((64, 32), (100, 528), (90, 300), (75, 333))


@functools.lru_cache(maxsize=None)
def bgr_cases(shape):
    """(name, frame u8 [h][w][3], claim): the serpentine and seam cases with b = g = r at the BGR levels; the thresholds come from
    the frame's median (the host test states them)."""
    out = []
    for n, img, c in _chain_cases(shape, BGR_BG, BGR_WEAK, seed_tapered(BGR_SEED, 12, BGR_BG), 6, thick=4):
        frame = np.repeat(img[:, :, None], 3, axis=2)
        frame.setflags(write=False)
        out.append((n, frame, c))
    return tuple(out)


def bgr_ids():
    pairs = [(s, n) for s in BGR_SHAPES for n, _, _ in bgr_cases(s)]
    return pairs, ["%dx%d-%s" % (s[0], s[1], n) for s, n in pairs]


def bgr_case(shape, name):
    return next(c for c in bgr_cases(shape) if c[0] == name)
