"""Hand-made inputs of the lane back end (pure NumPy, no GPU): edge maps and their row-major point lists for the three
progressive-probabilistic-Hough kernels, segment lists for the slope split / quadratic fit, and a NumPy restatement of the two
capacity formulas that decide which kernel takes a frame.  tests/test_lane_cases_host.py proves with the oracle alone that
the inputs have the properties the GPU tests rely on."""
import numpy as np

# (threshold, min_line_length, max_line_gap) -> the kernel a small, sparse frame must end in (workspace view 8)
A_CONFIGS = [((50, 50, 150), 1), ((20, 20, 3), 1), ((20, 20, 4), 1), ((10, 10, 1), 1), ((30, 10, 62), 1), ((30, 10, 63), 1),
             ((15, 30, 0), 3)]
A_SHAPE, A_S, A_MS = (96, 160), 8, 64
B_SHAPE, B_MS = (160, 512), 2048
B_COUNTS, B_KERNELS = (4096, 4097, 12288, 12289), (1, 2, 2, 3)
B_CONFIGS = [(50, 50, 150), (40, 30, 5)]
C_CONFIGS = [(50, 50, 150), (20, 20, 4)]
E_CONFIG, E_LINES = (30, 30, 2), 22
E_FAST_CONFIG, E_FAST_MS = (40, 30, 5), 8

# capacities of csrc/lane.hip
HS_NZ, HS_BMW, HS_ACCW, HQ, HTL = 4096, 9216, 6144, 16, 12          # theta-sharded kernel
NZCAP, BMWORDS = 12288, 16384                                       # single-workgroup kernel
NUMANGLE = 180


def point_list(edge_map):
    """Row-major list x | y << 16 of the non-zero pixels: what the compaction pass leaves in workspace view 9."""
    ys, xs = np.nonzero(edge_map)
    return xs.astype(np.uint32) | (ys.astype(np.uint32) << 16)


def _blank(shape):
    return np.zeros(shape, np.uint8)


def _segment(img, x0, y0, x1, y1, on=1, off=0, thick=1):
    """Pixels of the straight walk (x0, y0) -> (x1, y1), one per step of the longer axis, `on` drawn then `off` skipped;
    `thick` pixels across the shorter axis.  Pixels outside the frame are dropped."""
    h, w = img.shape
    n = max(abs(x1 - x0), abs(y1 - y0))
    steep = abs(y1 - y0) > abs(x1 - x0)
    for t in range(n + 1):
        if (t % (on + off)) >= on:
            continue
        x = x0 + int(round((x1 - x0) * t / n)) if n else x0
        y = y0 + int(round((y1 - y0) * t / n)) if n else y0
        for d in range(thick):
            xx, yy = (x + d, y) if steep else (x, y + d)
            if 0 <= xx < w and 0 <= yy < h:
                img[yy, xx] = 255
    return img


def _normal_line(img, deg, thick):
    """The line through the frame's centre whose normal stands at `deg` degrees: pixels with 0 <= x cos + y sin - rho0 < thick."""
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w]
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    d = (xx - w // 2) * c + (yy - h // 2) * s
    img[(d >= 0) & (d < thick)] = 255
    return img


def mixed_picture(shape=A_SHAPE):
    """A diagonal dashed 6 on / 4 off (a gap of 3 breaks it into dashes, a gap of 4 joins it), a vertical, a crossing
    anti-diagonal and a horizontal with one hole of exactly 63 pixels (a gap of 62 ends the walk there, 63 crosses it)."""
    h, w = shape
    img = _blank(shape)
    _segment(img, 10, 2, 10 + h - 6, h - 4, on=6, off=4)
    _segment(img, w - 30, 0, w - 30, h - 1)
    _segment(img, w - 60, 5, w - 60 - (h - 16), h - 11)
    y = h - 2
    img[y, 8:w - 101] = 255                     # w - 109 pixels, then the hole: columns w - 101 .. w - 39
    img[y, w - 38:w - 2] = 255                  # 36 pixels
    return img


def threshold_picture(shape, threshold, gap):
    """One horizontal line of exactly threshold - 1 points and one of exactly threshold points (every second pixel when the
    gap rule allows holes, so that the longer one passes the length rule too)."""
    h, w = shape
    img = _blank(shape)
    step = 2 if gap >= 1 and 2 * threshold + 4 < w else 1
    img[h // 4, 3:3 + step * (threshold - 1):step] = 255
    img[3 * h // 4, 3:3 + step * threshold:step] = 255
    assert int((img[h // 4] != 0).sum()) == threshold - 1 and int((img[3 * h // 4] != 0).sum()) == threshold
    return img


def border_picture(shape):
    """The four border rows / columns and the corner-to-corner diagonal: walks that leave the image at once."""
    h, w = shape
    img = _blank(shape)
    img[0, :] = img[h - 1, :] = 255
    img[:, 0] = img[:, w - 1] = 255
    return _segment(img, 0, 0, w - 1, h - 1)


def seam_picture(shape):
    """2-pixel-thick lines through the centre with normals at the seams between sub-shards theta = 16 tl + q (15 | 16 | 17,
    31 | 32), at 90 degrees and on the last row of the accumulator, 179."""
    img = _blank(shape)
    for deg in (15, 16, 17, 31, 32, 90, 179):
        _normal_line(img, deg, 2)
    return img


def noise_picture(shape, seed=11):
    """Two crossing 3-pixel lines over 2 % salt noise: erasing a line decrements cells of pixels that have not voted yet."""
    h, w = shape
    img = _blank(shape)
    img[np.random.RandomState(seed).rand(h, w) < 0.02] = 255
    _segment(img, 12, 6, w - 20, h - 12, thick=3)
    _segment(img, 15, h - 9, w - 14, 4, thick=3)
    return img


def length_picture(shape, L):
    """Horizontal and vertical dashes whose extent |end - start| is L - 1, L and L + 1: the length rule is `>=`."""
    h, w = shape
    img = _blank(shape)
    for k, ext in enumerate((L - 1, L, L + 1)):
        img[6 + 8 * k, 4:4 + ext + 1] = 255
        img[30:30 + ext + 1, w - 12 - 14 * k] = 255
    return img


def pictures_a(cfg, shape=A_SHAPE):
    """The eight pictures of batch A for one configuration (pictures 4 and 8 follow its threshold and minimum length)."""
    threshold, length, gap = cfg
    single = _blank(shape)
    single[shape[0] // 2 + 1, shape[1] // 3] = 255
    return [mixed_picture(shape), _blank(shape), single, threshold_picture(shape, threshold, gap), border_picture(shape),
            seam_picture(shape), noise_picture(shape), length_picture(shape, length)]


def hatch(shape, spacing=12):
    """Dense double hatch: one-pixel diagonals of both directions every `spacing` columns."""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return ((((xx + yy) % spacing) == 0) | (((xx - yy) % spacing) == 0)).astype(np.uint8) * 255


def truncated(edge_map, n):
    """`edge_map` with only its first n points in row-major order."""
    ys, xs = np.nonzero(edge_map)
    assert len(ys) >= n
    out = np.zeros_like(edge_map)
    out[ys[:n], xs[:n]] = 255
    return out


def pictures_b():
    full = hatch(B_SHAPE)
    return [truncated(full, n) for n in B_COUNTS]


def sparse_lines(shape, box=None):
    """A few hundred points on long lines, every fourth pixel (a gap of 3), spanning exactly `box` = (y0, y1, x0, x1)
    inclusive (default: the whole frame): the diagonals, the middle row, the middle column and the four corners."""
    h, w = shape
    y0, y1, x0, x1 = box if box else (0, h - 1, 0, w - 1)
    img = _blank(shape)
    _segment(img, x0, y0, x1, y1, on=1, off=3)
    _segment(img, x0, y1, x1, y0, on=1, off=3)
    _segment(img, x0, (y0 + y1) // 2, x1, (y0 + y1) // 2, on=1, off=3)
    _segment(img, (x0 + x1) // 2, y0, (x0 + x1) // 2, y1, on=1, off=3)
    for yy in (y0, y1):
        for xx in (x0, x1):
            img[yy, xx] = 255
    return img


# frame shape, box of the points, kernel that must take the frame, why
C_CASES = [((320, 1024), None, 2, "10 240 bitmap words: over the sharded kernel's 9 216, within the single-workgroup kernel's 16 384"),
           ((160, 1616), None, 2, "8 160 bitmap words fit, the largest sub-shard's accumulator rows do not"),
           ((720, 1280), None, 3, "28 800 bitmap words: over both caps; the generic kernel rebuilds its mask from the list"),
           ((720, 1280), (432, 719, 128, 1151), 1, "exactly 9 216 bitmap words: the cap, from the inside")]


def cap_picture(shape=A_SHAPE):
    """22 horizontal lines of different lengths, four rows apart."""
    img = _blank(shape)
    for k in range(E_LINES):
        img[4 + 4 * k, 5 + k:90 + 3 * k] = 255
    return img


def trig_table():
    """cv::HoughLinesProbabilistic's table as the kernels hold it: theta a float, angles in double, rounded to float."""
    theta = np.float32(np.pi / 180.0)
    ang = np.arange(NUMANGLE, dtype=np.float64) * np.float64(theta)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _rint(v):
    return int(np.rint(np.float32(v)))


def geometry(points, shape):
    """The capacity figures the kernels derive from a sorted point list: (sharded bitmap words, largest sub-shard's accumulator
    cells, single-workgroup bitmap words).  Restates houghp_shard's bounding box / row_lo_hi in float32."""
    h, w = shape
    if len(points) == 0:
        return 1, 0, (w + 31) >> 5
    xs, ys = (points & 0xffff).astype(np.int64), (points >> 16).astype(np.int64)
    ymin, ymax, xmn, xmx = int(ys[0]), int(ys[-1]), int(xs.min()), int(xs.max())
    wpr = (xmx >> 5) - (xmn >> 5) + 1
    half = ((w + h) * 2 + 1 - 1) // 2
    ct, sn = trig_table()
    f = np.float32
    size = np.zeros(HQ * HTL, np.int64)
    for t in range(NUMANGLE):
        r = [f(f(f(x) * ct[t]) + f(f(y) * sn[t])) for x in (xmn, xmx) for y in (ymin, ymax)]
        lo, hi = max(_rint(min(r)) - 2, -half), min(_rint(max(r)) + 2, half)
        size[t] = hi - lo + 1
    cells = max(int(size[q::HQ].sum()) for q in range(HQ))
    return (ymax - ymin + 1) * wpr, cells, (ymax - ymin + 1) * ((w + 31) >> 5)


def expected_kernel(points, shape, gap):
    """Which kernel a Hough-stage call (stage bits 16) must end in for this list: 1 sharded, 2 single-workgroup, 3 generic."""
    n = len(points)
    bmw, cells, bmw_fast = geometry(points, shape)
    if gap < 1:
        return 3
    if n <= HS_NZ and bmw <= HS_BMW and cells <= 2 * HS_ACCW:
        return 1
    if n <= NZCAP and bmw_fast <= BMWORDS:
        return 2
    return 3


# ---- segment lists for the fit (x1, y1, x2, y2) -------------------------------------------------------------------------------

def filter_list(w=640):
    """Slope filter and side rule, one list at w = 640 -> (segments, kept left, kept right)."""
    cx = w // 2
    segs = [
        (100, 400, 110, 397),        # left,  dy/dx = -0.3 exactly: kept
        (110, 397, 100, 400),        # the same segment, endpoints swapped: kept
        (500, 400, 510, 403),        # right, +0.3 exactly: kept
        (120, 400, 140, 395),        # -0.25: dropped
        (520, 400, 540, 405),        # +0.25: dropped
        (200, 300, 200, 400),        # x2 == x1: dropped
        (cx - 20, 420, cx + 20, 380),    # negative slope, mid == w / 2 exactly: dropped from both sides
        (cx - 20, 380, cx + 20, 420),    # positive slope, mid == w / 2 exactly: dropped from both sides
        (cx - 21, 420, cx + 20, 380),    # mid half a pixel left of the centre: kept left
        (cx - 20, 380, cx + 21, 420),    # mid half a pixel right of the centre: kept right
        (400, 420, 440, 380),        # negative slope in the right half: dropped
        (100, 380, 140, 420),        # positive slope in the left half: dropped
        (150, 470, 250, 300),        # plain left
        (390, 300, 600, 475),        # plain right
        (610, 478, 380, 290),        # plain right, endpoints right to left
    ]
    return np.array(segs, np.int32), 4, 4


def side_segments(n, h, w, side, seed):
    """n segments of one lane side, |slope| between 0.5 and 2, on a gently curved lane in the lower 40 % of the frame."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        ya = rng.randint(int(0.6 * h), h - 30)
        yb = ya + rng.randint(20, min(80, h - ya))
        ta, tb = (ya - 0.6 * h) / (0.4 * h), (yb - 0.6 * h) / (0.4 * h)
        sign, x0 = (-1, 0.42 * w) if side == 0 else (1, 0.58 * w)
        xa, xb = x0 + sign * (0.30 * w * ta + 0.04 * w * ta ** 2), x0 + sign * (0.30 * w * tb + 0.04 * w * tb ** 2)
        xa, xb = int(round(xa + rng.uniform(-2, 2))), int(round(xb + rng.uniform(-2, 2)))
        if xa == xb or abs((yb - ya) / (xb - xa)) < 0.5 or abs((yb - ya) / (xb - xa)) > 2:
            continue
        out.append((xa, ya, xb, yb))
    return out


def lane_list(nl, nr, h, w, seed=0, shuffle=True):
    """A list that keeps exactly nl left and nr right segments (plus nothing else), interleaved."""
    segs = side_segments(nl, h, w, 0, seed) + side_segments(nr, h, w, 1, seed + 1000)
    if shuffle:
        np.random.RandomState(seed + 7).shuffle(segs)
    return np.array(segs, np.int32).reshape(-1, 4)


def count_lists(MS=64, h=720, w=1280):
    """(segments, nl, nr): 1, 9, 10, 11 kept per side, and a full list of MS segments with MS kept on one side."""
    out = [(lane_list(n, n, h, w, seed=n), n, n) for n in (1, 9, 10, 11)]
    out.append((lane_list(MS, 0, h, w, seed=64), MS, 0))
    out.append((lane_list(0, MS, h, w, seed=65), 0, MS))
    return out


def rank_lists():
    """One segment (two points: rank 2), all endpoints on two rows (rank 2), all endpoints on three rows (rank 3, exact fit)."""
    one = np.array([[300, 600, 420, 480]], np.int32)
    two = np.array([[300, 600, 420, 480], [310, 600, 428, 480], [295, 600, 415, 480]], np.int32)
    three = np.array([[300, 600, 380, 540], [380, 540, 430, 480], [296, 600, 434, 480], [302, 600, 377, 540]], np.int32)
    return [("one_segment", one), ("two_rows", two), ("three_rows", three)]


def outside_list(h=720, w=1280):
    """Steep curves whose abscissae leave the frame over rows 0.6 h .. h: the left lane goes negative, the right one past w."""
    left = [(int(0.12 * w - 0.25 * w * t - 0.1 * w * t * t), int(0.6 * h + 0.4 * h * t)) for t in (0.0, 0.12, 0.25, 0.4)]
    right = [(int(0.88 * w + 0.25 * w * t + 0.1 * w * t * t), int(0.6 * h + 0.4 * h * t)) for t in (0.0, 0.12, 0.25, 0.4)]
    segs = [(a[0], a[1], b[0], b[1]) for pts in (left, right) for a, b in zip(pts[:-1], pts[1:])]
    return np.array(segs, np.int32)


# heights at which a sample row of np.linspace(0.6 h, h, 50) is mathematically an integer that a fused multiply-add misses
SAMPLE_HEIGHTS = [(343, 9, 231), (441, 9, 297), (511, 14, 365)]

EMA_PATTERNS = [(), (2,), (2, 3), (0, 1, 2, 3, 4, 5)]                # frames in which the stream's list is empty
EMA_SMOOTHINGS = (0.7, 0.0, 0.95)


def ema_lists(h=480, w=640, calls=6):
    """[call][stream] -> segment list: four streams with different lanes that change from call to call; EMA_PATTERNS[s]
    names the calls in which stream s sees nothing.  Stream 1 loses only its left side in call 2 (the right one stays)."""
    out = []
    for c in range(calls):
        row = []
        for s, drop in enumerate(EMA_PATTERNS):
            segs = lane_list(3 + s + c % 3, 2 + (s + c) % 4, h, w, seed=100 * s + c)
            if c in drop:
                segs = segs[[k for k in range(len(segs)) if s == 1 and (segs[k, 3] - segs[k, 1]) / (segs[k, 2] - segs[k, 0]) > 0]]
            row.append(segs.reshape(-1, 4))
        out.append(row)
    return out


def fit_cases():
    """Every fit case as (name, h, w, MS, smoothing, calls); calls[c][s] is stream s's segment list in call c."""
    cases = [("filter", 480, 640, 64, 0.7, [[filter_list(640)[0]]]),
             ("counts", 720, 1280, 64, 0.7, [[segs for segs, _, _ in count_lists(64, 720, 1280)]]),
             ("rank", 720, 1280, 64, 0.7, [[segs for _, segs in rank_lists()]]),
             ("outside", 720, 1280, 64, 0.7, [[outside_list(720, 1280)]])]
    for h in [r[0] for r in SAMPLE_HEIGHTS] + [720]:
        cases.append(("rows%d" % h, h, 640, 64, 0.7, [[lane_list(5, 4, h, 640, seed=h), lane_list(3, 6, h, 640, seed=h + 1)]]))
    for sm in EMA_SMOOTHINGS:
        cases.append(("ema%g" % sm, 480, 640, 64, sm, ema_lists(480, 640)))
    return cases


def fit_reference(case):
    """The oracle carried from call to call: ref[c][s] = dict(n, kept=(nl, nr), sides=[None | (points, confidence, coefficients,
    float64 abscissae)] * 2, state=[None | coefficients] * 2 after the call)."""
    from oracle.lane_ref import fit, separate
    _, h, w, _, smoothing, calls = case
    prev = [[None, None] for _ in calls[0]]
    out = []
    for row in calls:
        res = []
        for s, segs in enumerate(row):
            kept = separate(segs, w)
            sides = []
            for side in (0, 1):
                f = fit(kept[side], h, prev[s][side], smoothing)
                if f is not None:
                    prev[s][side] = f[2]
                    f = f + (np.polyval(f[2], np.linspace(h * 0.6, h, 50)),)
                sides.append(f)
            res.append(dict(n=len(segs), kept=(len(kept[0]), len(kept[1])), sides=sides, state=[None if p is None else p.copy() for p in prev[s]]))
        out.append(res)
    return out
