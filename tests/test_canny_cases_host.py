"""Conditions on the hand-made gray images (tests/canny_cases.py), proved with the oracle alone: the GPU comparison only tells a
wrong hysteresis or suppression kernel from a right one if a chain really is long, weak, lit by one seed, cut where it says."""
import numpy as np
import pytest

from tests import canny_cases as K

_PAIRS, _IDS = K.all_ids()
_BPAIRS, _BIDS = K.bgr_ids()


@pytest.fixture(scope="module")
def ref():
    from oracle import lane_ref
    return lane_ref


def _check(ref, image, lo, hi, claim, shape, exact=True):
    edges = ref.canny(image, lo, hi) != 0
    lo_, hi_ = min(lo, hi), max(lo, hi)
    cands = ref.canny(image, lo_, lo_) != 0                    # lo == hi: every candidate is strong, the edge map is the candidate set
    assert not (edges & ~cands).any()
    kind = claim["kind"]
    if kind == "lit":
        assert edges.sum() >= claim["min_pixels"], (int(edges.sum()), claim["min_pixels"])
        assert len(K.tiles_of(edges)) >= claim["min_tiles"], (sorted(K.tiles_of(edges)), claim["min_tiles"])
        # one seed lights it: without the strong level nothing is left
        levels = np.unique(image)
        assert not ref.canny(np.minimum(image, levels[-2]), lo, hi).any()
        if claim["far"] is not None:
            assert (edges & claim["far"]).sum() >= claim["min_far"], (int((edges & claim["far"]).sum()), claim["min_far"])
            assert (cands & claim["far"]).sum() == (edges & claim["far"]).sum()
    elif kind == "dark":
        assert not edges.any()
        assert cands.sum() >= claim["min_candidates"], (int(cands.sum()), claim["min_candidates"])
    elif kind == "cut":
        far = claim["far"]
        assert not (edges & far).any()
        assert (cands & far).sum() >= claim["min_far"], (int((cands & far).sum()), claim["min_far"])
        assert (edges & ~far).sum() >= 8                        # the seed's side is lit
        # the two sides do not touch: no candidate of the far side has a lit 8-neighbour
        grown = np.zeros_like(edges)
        p = np.pad(edges, 1)
        for dy in range(3):
            for dx in range(3):
                grown |= p[dy:dy + shape[0], dx:dx + shape[1]]
        assert not (grown & cands & far).any()
        if "gap" in claim and exact:
            # the gap lies on the seam itself: no candidate inside it, lit pixels on its one side, dark candidates on the other
            gap = claim["gap"]
            axis, k = claim["seam"]
            assert (gap[k] if axis == "row" else gap[:, k]).any() and k % (K.TILE_R if axis == "row" else K.TILE_C) in (0, K.TILE_C - 1)
            assert not (cands & gap).any()
            around = np.zeros_like(gap)
            p = np.pad(gap, 1)
            for dy in range(3):
                for dx in range(3):
                    around |= p[dy:dy + shape[0], dx:dx + shape[1]]
            assert (around & edges).any() and (around & cands & far).any()
    elif kind == "same_as":
        assert np.array_equal(edges, ref.canny(claim["image"], lo, hi) != 0)
        other = ref.canny(claim["other"], lo, hi) != 0           # the contour that vanishes is a chain of its own when seeded
        assert other.sum() >= 0.8 * edges.sum() and len(K.tiles_of(other)) >= len(K.tiles_of(edges)) - 2
        assert edges.sum() >= 4 * shape[1]
    elif kind == "verdict":
        probe = claim["probe"]
        assert probe.sum() >= 2
        assert (edges[probe].all() if claim["keep"] else not edges[probe].any()), int(edges[probe].sum())
    elif kind == "wedge":
        (a, b), sy = claim["ab"], claim["sy"]
        cls, gx, gy = K.sobel_classes(image, lo_)
        inside = (gx == 8 * a) & (gy == 8 * sy * b)
        assert (edges & inside).sum() >= 2, int((edges & inside).sum())
        assert set(cls[inside].tolist()) == {claim["cls"]}
        # strong pixels are exactly the kept pixels of the plateau, and they depend on the class: with the boundary moved past
        # b / a, or the other diagonal's neighbours, suppression keeps another set
        strong = ref.canny(image, hi_, hi_) != 0
        assert strong.any() and not (strong & ~inside).any() and np.array_equal(strong, K.nms(image, hi_))
        moved = K.nms(image, hi_, tg22=K.WEDGE_MOVED_TG22[a, b])
        assert not np.array_equal(moved, strong), (a, b, sy)
        if claim["cls"] in (2, 3):
            assert not np.array_equal(K.nms(image, hi_, swap_diagonals=True), strong), (a, b, sy)
    elif kind == "classes":
        cls, _, _ = K.sobel_classes(image, lo_)
        assert set(np.unique(cls[edges]).tolist()) == set(claim["want"])
        assert min(int((cls[edges] == k).sum()) for k in claim["want"]) >= 2
        assert np.array_equal(cands, K.nms(image, lo_))
        if min(shape) >= 16:                  # tan 22.5 moved to 0.336 and to 0.504 (tan 67.5 moves with it), the diagonals swapped
            for tg in (11000, 16500):
                assert not np.array_equal(K.nms(image, lo_, tg22=tg), cands), tg
            assert not np.array_equal(K.nms(image, lo_, swap_diagonals=True), cands)
    elif kind == "ties":
        assert edges.any() and np.array_equal(cands, K.nms(image, lo_))
    elif kind == "borders":
        assert edges[0].any() and edges[-1].any() and edges[:, 0].any() and edges[:, -1].any()
    else:
        raise AssertionError(kind)
    return edges, cands


@pytest.mark.parametrize("shape,name", _PAIRS, ids=_IDS)
def test_case_is_what_it_claims(ref, shape, name):
    c = K.case(shape, name)
    _check(ref, c.image, c.lo, c.hi, c.claim, shape)


@pytest.mark.parametrize("shape,name", [(s, n) for s, n in _PAIRS if n.startswith("seam_diag") and not n.endswith("_cut")],
                         ids=[i for (s, n), i in zip(_PAIRS, _IDS) if n.startswith("seam_diag") and not n.endswith("_cut")])
def test_diagonal_steps_sit_where_they_say(ref, shape, name):
    """The chain crosses through exactly the stated diagonal pair: the other two pixels of that 2 x 2 block are no candidates, and
    the rows above and below (for a chain that runs down the frame: the columns left and right) are empty around it."""
    c = K.case(shape, name)
    y, x, mirror = c.claim["step"]
    cands = ref.canny(c.image, c.lo, c.lo) != 0
    block = cands[y - 1:y + 1, x - 1:x + 1].astype(int).tolist()
    assert block == ([[0, 1], [1, 0]] if mirror else [[1, 0], [0, 1]]), block
    if "hseam" in name:             # the chain runs down the frame: one pixel wide
        assert not cands[y - 4:y + 4, x - 2].any() and not cands[y - 4:y + 4, x + 1].any()
    else:
        assert not cands[y - 2, x - 4:x + 4].any() and not cands[y + 1, x - 4:x + 4].any()
    if "vseam" in name:
        assert x == K.TILE_C and y % K.TILE_R not in (0, K.TILE_R - 1)
    elif "corner" in name:
        assert x == K.TILE_C and y % K.TILE_R == 0
    else:
        assert y % K.TILE_R == 0 and x % K.TILE_C not in (0, K.TILE_C - 1)


def test_corner_l_passes_three_tiles_around_the_tile_corner(ref):
    for shape in K.SHAPES:
        if "seam_4conn_corner" not in K.names(shape):
            continue
        c = K.case(shape, "seam_4conn_corner")
        cands = ref.canny(c.image, c.lo, c.lo) != 0
        y, x = K.seam_row(shape), K.TILE_C
        assert cands[y - 1:y + 1, x - 1:x + 1].astype(int).tolist() == [[0, 1], [1, 1]]


def test_every_shape_has_its_families():
    fam = {s: {n.split("_")[0] for n in K.names(s)} for s in K.SHAPES}
    for s in K.SHAPES:
        assert {"step", "wedge", "cone", "terraces", "frame"} <= fam[s], s
    for s in ((64, 32), (100, 528), (90, 300), (75, 333), (40, 16)):
        assert {"serpentine", "seam", "dense"} <= fam[s], s
    for s in ((64, 32), (100, 528), (90, 300), (75, 333)):
        assert "interleaved" in fam[s], s
    for s in ((100, 528), (90, 300), (75, 333)):
        assert {"seam_diag_vseam", "seam_diag_vseam_mirror", "seam_diag_corner", "seam_diag_corner_mirror", "seam_4conn_vseam",
                "seam_4conn_corner"} <= set(K.names(s)), s


def test_threshold_cases_hit_the_equalities(ref):
    img, probe = K.step((64, 32))
    cls, gx, gy = K.sobel_classes(img, 0)
    assert (np.abs(gx) + np.abs(gy))[probe].tolist() == [80] * int(probe.sum())
    los = {(lo, hi) for _, lo, hi, _, _ in K.STEP_CASES}
    assert {(80, 300), (79, 300), (50, 80), (50, 79), (79, 79), (80, 80), (0, 79)} <= los and any(lo > hi for lo, hi in los)


def test_wedges_sit_on_both_sides_of_both_class_boundaries():
    want = {(5, 2): 0, (12, 5): 2, (5, 12): 2, (2, 5): 1}
    for (a, b), cl in want.items():
        for sy in (1, -1):
            img = K.wedge((64, 32), a, b, sy)[0]
            cls, gx, gy = K.sobel_classes(img, K.LO)
            inside = (gx == 8 * a) & (gy == 8 * sy * b)
            assert inside.sum() >= 8, (a, b, sy)
            assert set(cls[inside].tolist()) == {cl if cl != 2 or sy > 0 else 3}, (a, b, sy)


def test_default_roi_sees_the_chains(ref):
    """Serpentines and seams reach below 0.6 h inside the trapezoid: the production shape's bit-map resolve has work."""
    for shape in K.SHAPES:
        for c in K.cases(shape):
            if c.claim["kind"] == "lit" and (c.name.startswith("serpentine") or c.name.startswith("seam")):
                assert ref.apply_roi(ref.canny(c.image, c.lo, c.hi)).any(), (shape, c.name)


def test_handmade_roi_rows_have_every_kind_of_row():
    for shape in K.SHAPES:
        rows = K.roi_rows_handmade(shape)
        h, w = shape
        assert ((rows[:, 1] < w) & (rows[:, 0] >= 0)).all()
        assert (rows[:, 0] > rows[:, 1]).any() and (rows[:, 0] == rows[:, 1]).any() and ((rows[:, 0] == 0) & (rows[:, 1] == w - 1)).any()
        full = K.roi_rows_full(shape)
        assert np.array_equal(K.mask_rows(np.full(shape, 255, np.uint8), full), np.full(shape, 255, np.uint8))


@pytest.mark.parametrize("shape,name", _BPAIRS, ids=_BIDS)
def test_bgr_case_is_what_it_claims(ref, shape, name):
    _, frame, claim = K.bgr_case(shape, name)
    st = ref.LaneRef().stages(frame)
    assert np.array_equal(st["gray"], frame[:, :, 0])
    # the background is the larger part of every frame, so the thresholds are known: a blurred straight step of contrast 32
    # (magnitude 80) is a candidate and a blurred corner (up to 116) is not strong
    assert (st["median"], st["lo"], st["hi"]) == (100.0, 70, 130)
    c = dict(claim)
    if c["kind"] == "lit":                       # the blur rounds the turns and thickens nothing: a looser count, the same tiles
        c["min_pixels"] = int(0.8 * c["min_pixels"])
        c["min_far"] = int(0.8 * c["min_far"])
    edges = st["edges"] != 0
    cands = ref.canny(st["blur"], st["lo"], st["lo"]) != 0
    if c["kind"] == "lit":
        assert edges.sum() >= c["min_pixels"] and len(K.tiles_of(edges)) >= c["min_tiles"]
        if c["far"] is not None:
            assert (edges & c["far"]).sum() >= c["min_far"]
        flat = np.minimum(frame, K.BGR_WEAK)
        assert not ref.LaneRef().stages(flat)["edges"].any()
    elif c["kind"] == "dark":
        assert not edges.any() and cands.sum() >= 0.8 * c["min_candidates"]
    else:
        assert c["kind"] == "cut"
        assert not (edges & c["far"]).any() and (cands & c["far"]).sum() >= 0.8 * c["min_far"] and (edges & ~c["far"]).sum() >= 8
