"""YOLO tail: hand-made candidate lists for threshold + sort + NMS + scale_boxes (nms_sort_kernel, nms_greedy_kernel in csrc/yolo.hip).

Pure NumPy and deterministic.  A case is a candidate list of one image -- box float32 [A, 4] in network pixels, conf float32 [A], cls
int32 [A] -- with the parameters of the call (conf_thres, iou_thres, max_det).  What the device must give is always
oracle.yolo_ref.nms on that list followed by scale_boxes (`expected`); the one list that holds confidences outside (conf_thres, 1]
has them masked out first, which is the candidate rule of include/avhot.h.

`nms_variant` is this file's own restatement of that NMS with switches for deliberately WRONG conventions (WRONG): with none set it
must equal the oracle on every case, and each family must give a different result under the wrong convention it is there to catch
(tests/test_yolo_tail_cases_host.py shows both, and that every list sits at the counts, chunk edges, pass counts and masks it
claims).  tests/test_gpu_yolo_tail.py then holds the device to `expected`, bit for bit.
"""
import functools

import numpy as np

from oracle import yolo_ref as R

# frame (h, w) -> anchors of its network input: 420 .. 7 140 take nms_sort_kernel<8> (1 .. 7 rounds of 1 024), 7 560 and 7 980 <7>
FRAMES = {420: (64, 1280), 1260: (192, 1280), 2520: (90, 333), 7140: (1088, 1280), 7560: (1152, 1280), 7980: (1216, 1280)}
FAMILIES = ("counts", "ties", "passes", "threshold", "exact_iou", "chains", "max_det", "mapping")
WRONG = ("ties_descending_anchor", "conf_ge", "iou_ge", "dead_suppress", "no_class_offset", "cut_after", "admit_above_one")
# the wrong convention(s) each family must tell from the right one (counts: where more than its max_det = 2 500 anchors exist; the
# mapping family is about scale_boxes, which no selection convention touches)
CATCHES = {"counts": ("cut_after",), "ties": ("ties_descending_anchor",), "passes": ("ties_descending_anchor",),
           "threshold": ("conf_ge", "admit_above_one"), "exact_iou": ("iou_ge", "no_class_offset"), "chains": ("dead_suppress",),
           "max_det": ("cut_after",), "mapping": ()}
ONE = 0x3F800000                     # bits of 1.0f: the sort key is ONE - bits(conf)
F = np.float32


def catches(fam, A):
    return () if fam == "counts" and A <= 2500 else CATCHES[fam]


def n_anchors(h, w):
    _, _, _, _, _, H, W = R.letterbox_shape(h, w)
    return sum((H // s) * (W // s) for s in R.STRIDES)


def digit_bits(A):
    """Digit width of the sort kernel that serves A anchors: 8 bits up to 7 rounds of 1 024, 7 bits beyond."""
    return 8 if (A + 1023) // 1024 <= 7 else 7


def passing(case):
    c, t = case["conf"], F(case["conf_thres"])
    return (c > t) & (c <= F(1.0))


def radix_passes(case):
    """Passes the radix sort makes on this list: digits until the largest key is exhausted ((vmax >> shift) != 0)."""
    ok = passing(case)
    vmax = int((ONE - case["conf"][ok].view(np.uint32).astype(np.int64)).max()) if ok.any() else 0
    return -(-vmax.bit_length() // digit_bits(len(case["conf"])))


def sorted_anchors(case):
    """Anchors of the passing candidates in the tail's order: confidence descending, equal confidences in anchor order."""
    a = np.nonzero(passing(case))[0]
    return a[np.argsort(-case["conf"][a], kind="stable")]


def grid_boxes(n, first=0, y0=0.0):
    """n pairwise disjoint 4.5 x 4.5 boxes on a 6-pixel grid of 106 columns, from cell `first` on."""
    k = np.arange(first, first + n)
    x1, y1 = 6.0 * (k % 106) + 0.75, 6.0 * (k // 106) + 0.75 + y0
    return np.stack([x1, y1, x1 + 4.5, y1 + 4.5], 1).astype(F)


def _case(family, name, A, box, conf, cls, conf_thres=0.25, iou_thres=0.7, max_det=300, **kw):
    box, conf, cls = np.ascontiguousarray(box, F), np.ascontiguousarray(conf, F), np.ascontiguousarray(cls, np.int32)
    assert box.shape == (A, 4) and conf.shape == (A,) and cls.shape == (A,) and 0 <= cls.min() and cls.max() < R.NC
    for a in (box, conf, cls):
        a.setflags(write=False)
    return dict(kw, family=family, name=name, A=A, box=box, conf=conf, cls=cls, conf_thres=float(F(conf_thres)), iou_thres=float(F(iou_thres)),
                max_det=max_det)


def _below(rs, A, thres=0.25):
    """Confidences of anchors that are no candidates: spread below the threshold, the threshold's lower neighbour among them."""
    c = (rs.uniform(0.02, 0.98, A) * thres).astype(F)
    c[rs.randint(A)] = np.nextafter(F(thres), F(0))
    return np.minimum(c, np.nextafter(F(thres), F(0)))


def _distinct(rs, n, lo, hi):
    """n distinct float32 values in (lo, hi), in random order."""
    bits = np.arange(n, dtype=np.int64) * ((int(F(hi).view(np.uint32)) - int(F(lo).view(np.uint32)) - 2) // max(n, 1)) + int(F(lo).view(np.uint32)) + 1
    return rs.permutation(bits.astype(np.uint32).view(F))


def _ranked(rs, A, boxes, classes, conf_hi=0.96, conf_lo=0.30, **kw):
    """A list whose candidates are `boxes` in THIS sorted order (distinct descending confidences), at scattered anchors."""
    n = len(boxes)
    assert n <= A
    anchors = rs.permutation(A)[:n]
    conf, box, cls = _below(rs, A), grid_boxes(A, y0=4000.0), np.zeros(A, np.int32)
    conf[anchors] = np.sort(_distinct(rs, n, conf_lo, conf_hi))[::-1]
    box[anchors], cls[anchors] = boxes, classes
    return box, conf, cls


# ---- the families -------------------------------------------------------------------------------------------------------------------
def counts_cases(A):
    """n passing candidates at scattered anchors, the rest below the threshold; disjoint boxes: everything up to max_det is kept."""
    out = []
    for n in sorted({0, 1, 63, 64, 65, 128, 129, 1023, 1024, 1025, A - 1, A}):
        if not 0 <= n <= A:
            continue
        rs = np.random.RandomState(100 + n)
        conf = _below(rs, A)
        conf[rs.permutation(A)[:n]] = _distinct(rs, n, 0.26, 0.97)
        out.append(_case("counts", "counts_%d" % n, A, grid_boxes(A), conf, rs.randint(0, R.NC, A), max_det=2500, n=n))
    return out


def ties_cases(A):
    """Every anchor a candidate.  three: confidences from 3 values, so that equal keys meet in every round, wave and digit group;
    deep1 / deep2: the same with the candidates of the top one / two values all on one box of one class, so that one of them
    is kept and the detections show the order of the NEXT value's candidates -- ranks far beyond max_det; equal: one value;
    ones: all exactly 1.0f (key 0: no pass at all)."""
    rs = np.random.RandomState(7)
    vals = np.array([0.9, 0.6, 0.3], F)
    pick = rs.randint(0, 3, A)
    cls = rs.randint(0, R.NC, A)
    out = [_case("ties", "ties_three", A, grid_boxes(A), vals[pick], cls, max_det=2500)]
    for deep in (1, 2):
        box, k = grid_boxes(A), cls.copy()
        for v in range(deep):
            box[pick == v], k[pick == v] = grid_boxes(1, first=A + v)[0], 11 + v
        out.append(_case("ties", "ties_deep%d" % deep, A, box, vals[pick], k, max_det=2500))
    out.append(_case("ties", "ties_equal", A, grid_boxes(A), np.full(A, 0.5, F), cls, max_det=2500))
    out.append(_case("ties", "ties_ones", A, grid_boxes(A), np.ones(A, F), cls, max_det=2500))
    return out


def passes_cases(A):
    """Every anchor a candidate; the largest key decides how many digits the sort walks.  ulpN: confidences within N ulp below 1.0,
    N itself among them (127 and 255: one pass with 8-bit digits, one and two with 7-bit digits; 65 535: two and three); spread:
    down to the threshold's upper neighbour at 0.25 (keys below 2^24) and 0.001 (below 2^27).  Few distinct keys per list make
    ties of every one."""
    out = []
    for name, ulp in (("ulp127", 127), ("ulp255", 255), ("ulp65535", 65535)):
        rs = np.random.RandomState(ulp)
        v = rs.randint(0, ulp + 1, A).astype(np.int64)
        v[rs.randint(A)] = ulp
        out.append(_case("passes", "passes_" + name, A, grid_boxes(A), (ONE - v).astype(np.uint32).view(F), rs.randint(0, R.NC, A), max_det=2500))
    for name, thres in (("spread_0.25", 0.25), ("spread_0.001", 0.001)):
        rs = np.random.RandomState(int(thres * 4000))
        conf = np.maximum((F(thres) ** rs.uniform(0, 1, A)).astype(F), np.nextafter(F(thres), F(1)))
        conf[rs.randint(A)] = np.nextafter(F(thres), F(1))
        conf[rs.randint(0, A, A // 3)] = conf[rs.randint(0, A, A // 3)]              # and ties among them
        out.append(_case("passes", "passes_" + name, A, grid_boxes(A), conf, rs.randint(0, R.NC, A), conf_thres=thres, max_det=2500))
    return out


def threshold_cases(A):
    """Confidences equal to conf_thres and its float32 neighbours on either side (strict: only the upper neighbour passes), among
    clear candidates; `specials` also holds NaN (both signs), +-inf, 1.5, the upper neighbour of 1.0, -1 and -0.0, none of which is a
    candidate, and 1.0 itself, which is."""
    out = []
    for thres in (0.25, 0.5):
        t = F(thres)
        rs = np.random.RandomState(int(thres * 100))
        vals = np.array([t, np.nextafter(t, F(0)), np.nextafter(t, F(1)), 0.9, 0.1], F)
        conf = vals[rs.randint(0, 5, A)]
        out.append(_case("threshold", "threshold_%g" % thres, A, grid_boxes(A), conf, rs.randint(0, R.NC, A), conf_thres=thres, max_det=2500))
    rs = np.random.RandomState(99)
    t = F(0.25)
    neg_nan = np.array([0xFFC00000], np.uint32).view(F)[0]
    vals = np.array([t, np.nextafter(t, F(0)), np.nextafter(t, F(1)), 0.9, np.nan, neg_nan, np.inf, -np.inf, 1.5, np.nextafter(F(1), F(2)),
                     -1.0, -0.0, 1.0, 0.7], F)
    conf = vals[rs.randint(0, len(vals), A)]
    conf[:len(vals)] = vals
    out.append(_case("threshold", "threshold_specials", A, grid_boxes(A), conf, rs.randint(0, R.NC, A), max_det=2500, masked=True))
    return out


def exact_iou_cases(A):
    """Box (0, 0, 4, 4) against (0, 0, 4, 2): IoU 8 / 16 = 0.5 exactly, in classes 0 and 5 (offset 38 400: still exact).  At
    iou_thres 0.5 both are kept (strict), at its lower neighbour the second dies.  Identical boxes of different class are both kept;
    identical zero-area boxes (a point, a vertical line) have IoU 0 / 0 = NaN: both kept.  Each pair stands 1, about 70 and about 200
    places apart in the sorted list: decided inside a chunk, against the previous chunk's survivors, against earlier ones."""
    rs = np.random.RandomState(3)
    slots, pairs, n = {}, [], 210

    def pair(kind, r0, r1, b0, b1, k0, k1):
        assert r0 not in slots and r1 not in slots and r0 < r1 < n
        slots[r0], slots[r1] = (b0, k0), (b1, k1)
        pairs.append((kind, r0, r1))
    x = 0.0
    for r0, r1, k in ((0, 1, 0), (2, 70, 0), (3, 200, 0), (10, 11, 5), (12, 75, 5), (13, 208, 5)):
        pair("half", r0, r1, (x, 0, x + 4, 4), (x, 0, x + 4, 2), k, k)
        x += 20
    for r0, r1 in ((4, 5), (6, 100), (7, 202)):
        pair("classes", r0, r1, (x, 10, x + 10, 20), (x, 10, x + 10, 20), 1, 2)                 # identical, classes differ
        pair("point", r0 + 20, r1 + 20 if r1 == 5 else r1 + 2, (x, 30, x, 30), (x, 30, x, 30), 3, 3)        # identical points
        pair("line", r0 + 30, r1 + 30 if r1 == 5 else r1 + 4, (x, 40, x, 48), (x, 40, x, 48), 4, 4)        # identical vertical lines
        x += 20
    boxes, classes = grid_boxes(n, y0=100.0), np.full(n, 7, np.int32)
    for r, (b, k) in slots.items():
        boxes[r], classes[r] = b, k
    assert len(slots) == 30
    box, conf, cls = _ranked(rs, A, boxes, classes)
    half = F(0.5)
    return [_case("exact_iou", "exact_iou_at_half", A, box, conf, cls, iou_thres=half, pairs=tuple(pairs)),
            _case("exact_iou", "exact_iou_below_half", A, box, conf, cls, iou_thres=np.nextafter(half, F(0)), pairs=tuple(pairs))]


def chain_layout(A):
    """(gap, clusters, members) of the three segments of the chain list, sized to A."""
    return ((1, 2, 8), (64, 64, 4), (240, 240, 4)) if A >= 1260 else ((1, 2, 8), (64, 64, 2), (128, 20, 3))


def chains_cases(A):
    """20 x 20 boxes in clusters 40 px apart, member j of a cluster shifted 4 j px: IoU 2/3 with its neighbour, 3/7 two apart, at
    iou_thres 0.5: member 0 is kept, 1 dies, 2 is kept BECAUSE 1 is dead, 3 dies ...  Three segments follow one another in the sorted
    list; inside a segment a member's rank is j gap + cluster with gap 1 (a chain inside a chunk), 64 (killer in the previous chunk)
    and 240 (killer in an earlier chunk); ranks of a segment that no member takes hold disjoint boxes.  420 anchors have no room for
    three members 240 apart: there the third gap is 128, two chunks."""
    rs = np.random.RandomState(11)
    boxes, classes, cluster0 = [], [], 0
    for gap, clusters, members in chain_layout(A):
        n = (members - 1) * gap + clusters if gap > 1 else clusters * members
        seg_b, seg_k = grid_boxes(n, first=len(boxes), y0=2000.0), np.full(n, 9, np.int32)
        for c in range(clusters):
            for j in range(members):
                r = j * gap + c if gap > 1 else c * members + j
                g = cluster0 + c
                x, y = 40.0 * (g % 16) + 4.0 * j, 40.0 * (g // 16)
                seg_b[r], seg_k[r] = (x, y, x + 20, y + 20), g % R.NC
        cluster0 += clusters
        boxes += list(seg_b)
        classes += list(seg_k)
    box, conf, cls = _ranked(rs, A, np.array(boxes, F), np.array(classes, np.int32))
    return [_case("chains", "chains", A, box, conf, cls, iou_thres=0.5, max_det=2500),
            _case("chains", "chains_300", A, box, conf, cls, iou_thres=0.5, max_det=300)]


def max_det_cases(A):
    """One list, every anchor a candidate with a confidence of its own, disjoint boxes: the first min(A, max_det) are kept.  The cut
    falls at a chunk's first member (1, 65), its last (63 -- and 64, exactly the chunk's end) and inside (300, 2 500)."""
    rs = np.random.RandomState(5)
    conf, cls = _distinct(rs, A, 0.26, 0.99), rs.randint(0, R.NC, A)
    return [_case("max_det", "max_det_%d" % m, A, grid_boxes(A), conf, cls, max_det=m) for m in (1, 63, 64, 65, 300, 2500)]


def mapping_cases(A):
    """Boxes with fractional corners inside the picture's part of the network input, straddling each of its edges, and wholly outside it
    (inside the letterbox's padding rows where the frame has them, as (90, 333) has: 9 above, 10 below): scale_boxes subtracts the
    padding, divides by the gain and clips to the frame."""
    h, w = FRAMES[A]
    _, nh, nw, top, left, H, W = R.letterbox_shape(h, w)
    rs = np.random.RandomState(13)
    x0, y0, x1, y1 = float(left), float(top), float(left + nw), float(top + nh)
    boxes = []
    for _ in range(12):                                                               # inside
        cx, cy, bw, bh = rs.uniform(x0 + 8, x1 - 8), rs.uniform(y0 + 4, y1 - 4), rs.uniform(2, 8), rs.uniform(1, 4)
        boxes.append((cx - bw, cy - bh, cx + bw, cy + bh))
    for _ in range(3):                                                                # across the left, right, top and bottom edge
        cy, cx = rs.uniform(y0 + 4, y1 - 4), rs.uniform(x0 + 30, x1 - 30)
        boxes += [(x0 - rs.uniform(1, 9), cy - 3, x0 + rs.uniform(1, 9), cy + 3), (x1 - rs.uniform(1, 9), cy - 2, x1 + rs.uniform(1, 9), cy + 2),
                  (cx - 20, y0 - rs.uniform(0.5, 6), cx - 10, y0 + rs.uniform(0.5, 6)), (cx + 10, y1 - rs.uniform(0.5, 6), cx + 20, y1 + rs.uniform(0.5, 6))]
    for _ in range(3):                                                                # wholly outside: above, below, left, right
        cx, cy = rs.uniform(x0 + 30, x1 - 30), rs.uniform(y0 + 4, y1 - 4)
        boxes += [(cx - 5, y0 - 8.5, cx + 5, y0 - 1.25), (cx - 5, y1 + 1.25, cx + 5, y1 + 8.5), (x0 - 30, cy - 2, x0 - 2.5, cy + 2),
                  (x1 + 2.5, cy - 2, x1 + 30, cy + 2)]
    boxes = np.array(boxes, F)
    kinds = np.array([0] * 12 + [1] * 12 + [2] * 12)
    order = rs.permutation(len(boxes))
    box, conf, cls = _ranked(rs, A, boxes[order], rs.randint(0, R.NC, len(boxes)))
    return [_case("mapping", "mapping", A, box, conf, cls, iou_thres=0.7, kinds=kinds[order], rect=(x0, y0, x1, y1))]


_BUILDERS = dict(counts=counts_cases, ties=ties_cases, passes=passes_cases, threshold=threshold_cases, exact_iou=exact_iou_cases,
                 chains=chains_cases, max_det=max_det_cases, mapping=mapping_cases)


@functools.lru_cache(maxsize=None)
def family(A, name):
    """The cases of one family at A anchors (built once; the arrays are read-only)."""
    return tuple(_BUILDERS[name](A))


def all_cases(A):
    return [c for f in FAMILIES for c in family(A, f)]


def partner(A, like):
    """A second, short list for the same call as case `like` (its parameters): 129 candidates at scattered anchors."""
    c = family(A, "counts")[[k["n"] for k in family(A, "counts")].index(129)]
    return dict(c, name="partner", conf_thres=like["conf_thres"], iou_thres=like["iou_thres"], max_det=like["max_det"], n=None)


def empty(A, like):
    """A list without a candidate, with the parameters of case `like`."""
    rs = np.random.RandomState(1)
    c = _case("counts", "empty_below_%g" % like["conf_thres"], A, grid_boxes(A), _below(rs, A, like["conf_thres"]), rs.randint(0, R.NC, A))
    return dict(c, conf_thres=like["conf_thres"], iou_thres=like["iou_thres"], max_det=like["max_det"])


# ---- what the device must give ------------------------------------------------------------------------------------------------------
def candidate_conf(case):
    """The confidences the oracle is given: those outside (conf_thres, 1] -- NaN included -- are no candidates (include/avhot.h), which
    the oracle's `conf > conf_thres` alone does not say for values above 1; only a list marked `masked` holds any."""
    if not case.get("masked"):
        assert np.array_equal(passing(case), case["conf"] > F(case["conf_thres"])), case["name"]
        return case["conf"]
    return np.where(passing(case), case["conf"], F(0))


_EXPECTED = {}


def expected(case):
    """-> (kept anchors, boxes in frame pixels float32 [n, 4], conf [n], cls [n]) from oracle/yolo_ref.py; computed once per list
    and parameter set."""
    key = (case["A"], case["name"], case["conf_thres"], case["iou_thres"], case["max_det"])
    if key not in _EXPECTED:
        h, w = FRAMES[case["A"]]
        keep = R.nms(case["box"], candidate_conf(case), case["cls"], F(case["conf_thres"]), F(case["iou_thres"]), case["max_det"])
        _EXPECTED[key] = (keep, R.scale_boxes(case["box"][keep].reshape(-1, 4), h, w), case["conf"][keep], case["cls"][keep])
    return _EXPECTED[key]


def nms_variant(case, wrong=None, trace=False):
    """This file's restatement of the tail's selection, with one convention deliberately wrong (one of WRONG) or none.
    -> kept anchors; with trace, also (sorted anchors, dead flags, kept flags, killers): killers[i] = sorted positions of the KEPT
    boxes that overlap sorted candidate i beyond the threshold."""
    assert wrong is None or wrong in WRONG
    conf, t, thr = case["conf"], F(case["conf_thres"]), F(case["iou_thres"])
    ok = (conf >= t) if wrong == "conf_ge" else (conf > t)
    if wrong != "admit_above_one":
        ok &= conf <= F(1.0)
    a = np.nonzero(ok)[0]
    if wrong == "ties_descending_anchor":
        a = a[::-1]
    order = a[np.argsort(-conf[a], kind="stable")]
    off = np.zeros(len(order), F) if wrong == "no_class_offset" else case["cls"][order].astype(F) * F(7680.0)
    b = (case["box"][order] + off[:, None]).astype(F)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    n, limit = len(order), case["max_det"] + (wrong == "cut_after")
    dead, kept, killers = np.zeros(n, bool), np.zeros(n, bool), [[] for _ in range(n)]
    n_kept = 0
    for i in range(n):
        if dead[i] and wrong != "dead_suppress":
            continue
        if not dead[i]:
            kept[i] = True
            n_kept += 1
            if n_kept >= limit:
                break
        with np.errstate(invalid="ignore", divide="ignore"):
            inter = (np.maximum(np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]), F(0))
                     * np.maximum(np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]), F(0)))
            iou = inter / (area[i] + area[i + 1:] - inter)
        hit = (iou >= thr) if wrong == "iou_ge" else (iou > thr)
        if trace and kept[i]:
            for j in np.nonzero(hit)[0]:
                killers[i + 1 + j].append(i)
        dead[i + 1:] |= hit
    keep = order[kept]
    return (keep, (order, dead, kept, killers)) if trace else keep


def mask_counts(case):
    """Which of nms_greedy_kernel's decisions the list reaches, in chunks of 64 sorted candidates: candidates whose only killers
    stand in their own chunk (wave 0's ballot loop), candidates with a killer in the previous chunk (the `late` mask), with a killer
    in an earlier chunk (the `early` mask), and KEPT candidates that overlap, beyond the threshold, a dead one of an earlier chunk
    (what a kernel in which dead boxes suppress would lose)."""
    keep, (order, dead, kept, killers) = nms_variant(case, trace=True)
    same = prev = early = 0
    for i, ks in enumerate(killers):
        if not ks:
            continue
        d = i // 64 - np.array(ks) // 64
        same, prev, early = same + bool((d == 0).all()), prev + bool((d == 1).any()), early + bool((d >= 2).any())
    off = case["cls"][order].astype(F) * F(7680.0)
    b = (case["box"][order] + off[:, None]).astype(F)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    later_chunk = np.arange(len(order)) // 64
    hit_by_dead = np.zeros(len(order), bool)
    for j in np.nonzero(dead)[0]:
        inter = (np.maximum(np.minimum(b[j, 2], b[:, 2]) - np.maximum(b[j, 0], b[:, 0]), F(0))
                 * np.maximum(np.minimum(b[j, 3], b[:, 3]) - np.maximum(b[j, 1], b[:, 1]), F(0)))
        hit_by_dead |= (inter / (area[j] + area - inter) > F(case["iou_thres"])) & (later_chunk > j // 64)
    spared = int((kept & hit_by_dead).sum())
    return dict(same=same, prev=prev, early=early, spared=spared, kept=int(kept.sum()), dead=int(dead.sum()))
