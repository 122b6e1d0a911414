"""Lane pixel stages on hand-made gray images (tests/canny_cases.py; proved on the CPU by tests/test_canny_cases_host.py): the
given-gray entry of av_lane_detect (stage bit 64: Sobel, non-maximum suppression, hysteresis, ROI, compaction) against the oracle's
cv::Canny restatement, pixel by pixel, in the debug shape, the production shape, with caller-defined ROIs and in batches that reuse
a workspace; and the same chains through the BGR front ends.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from tests import canny_cases as K
from tests._util import LaneBatch

pytestmark = pytest.mark.gpu

GIVEN, PIXELS, KEEP = 64, 2, 1          # AV_LANE_GIVEN_GRAY, AV_LANE_PIXELS_ONLY, AV_LANE_KEEP_EDGES
MS = 16
_PAIRS, _IDS = K.all_ids()
_BPAIRS, _BIDS = K.bgr_ids()


@pytest.fixture(scope="module", autouse=True)
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


@functools.lru_cache(maxsize=None)
def _want(shape, name):
    """The oracle's (edge map, default-ROI edge map) of a case, computed once."""
    from oracle.lane_ref import apply_roi, canny
    c = K.case(shape, name)
    e = canny(c.image, c.lo, c.hi)
    m = apply_roi(e)
    e.setflags(write=False)
    m.setflags(write=False)
    return e, m


@functools.lru_cache(maxsize=None)
def _want_bgr(shape, name):
    from oracle.lane_ref import LaneRef
    return LaneRef().stages(np.ascontiguousarray(K.bgr_case(shape, name)[1]))


def _list(edge_map):
    ys, xs = np.nonzero(edge_map)
    return xs.astype(np.uint32) | (ys.astype(np.uint32) << 16)


def _diff(got, want):
    """Where two maps differ, for the assertion message."""
    ys, xs = np.nonzero(got != want)
    return "%d pixels differ, first (y, x) %s" % (len(ys), list(zip(ys[:6].tolist(), xs[:6].tolist())))


def _batch(shape, names):
    h, w = shape
    lb = LaneBatch(len(names), h, w, MS)
    for s, n in enumerate(names):
        c = K.case(shape, n)
        lb.load_gray(s, c.image, c.lo, c.hi)
    return lb


@pytest.mark.parametrize("shape,name", _PAIRS, ids=_IDS)
def test_debug_shape_is_the_oracles_canny(shape, name):
    """View 2 is canny(image, lo, hi) byte for byte, view 3 the default trapezoid's part of it."""
    h, w = shape
    edges, masked = _want(shape, name)
    lb = _batch(shape, [name])
    lb.run(GIVEN | PIXELS | KEEP)
    got = lb.view(2, np.uint8, (h, w))
    assert np.array_equal(got, edges), _diff(got, edges)
    got = lb.view(3, np.uint8, (h, w))
    assert np.array_equal(got, masked), _diff(got, masked)
    assert np.array_equal(lb.points(0), _list(masked))


@pytest.mark.parametrize("shape,name", _PAIRS, ids=_IDS)
def test_production_shape_point_list(shape, name):
    """No debug edge map (tiled widths: ROI candidate bits, bit-map resolve, box compaction): views 9 / 10 hold exactly the oracle's
    ROI-masked non-zero pixels in row-major order."""
    _, masked = _want(shape, name)
    lb = _batch(shape, [name])
    lb.run(GIVEN | PIXELS)
    got, want = lb.points(0), _list(masked)
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape,name", _PAIRS, ids=_IDS)
def test_caller_defined_roi(shape, name):
    """roi_rows = the full frame (what the scene stage passes), then hand-made rows (empty rows, single columns, whole rows): the
    point list and the masked map are the oracle's edge map inside exactly those inclusive ranges."""
    h, w = shape
    edges, _ = _want(shape, name)
    lb = _batch(shape, [name])
    for rows, stages in ((K.roi_rows_full(shape), GIVEN | PIXELS), (K.roi_rows_handmade(shape), GIVEN | PIXELS),
                         (K.roi_rows_handmade(shape), GIVEN | PIXELS | KEEP)):
        want = K.mask_rows(edges, rows)
        lb.run(stages, roi_rows=rows)
        got = lb.view(3, np.uint8, (h, w))
        assert np.array_equal(got, want), _diff(got, want)
        assert np.array_equal(lb.points(0), _list(want))
        if stages & KEEP:
            assert np.array_equal(lb.view(2, np.uint8, (h, w)), edges)


def _batch_order(shape):
    """Five cases such that the reversed order puts a seeded chain into the slot its unseeded twin just used, and the other way
    round: [A seeded, B unseeded, X, B seeded, A unseeded]."""
    have = set(K.names(shape))
    if "serpentine_seed_first" in have:
        return ["serpentine_seed_first", "dense_no_seed", "step_swapped_weak_seeded", "dense_every_tile", "serpentine_no_seed"]
    return ["step_m_eq_lo_plus_1", "step_m_eq_hi", "cone", "step_m_eq_hi_plus_1", "step_m_eq_lo"]      # twins by threshold


@pytest.mark.parametrize("shape", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
def test_batches_reuse_the_workspace(shape):
    """S = 5 different cases in one call, each with its own thresholds, then the reverse order on the same workspace, production and
    debug shape: nothing of the call before may survive -- labels, tile edge words, bit maps, row counters."""
    h, w = shape
    order = _batch_order(shape)
    lb = LaneBatch(len(order), h, w, MS)
    for stages in (GIVEN | PIXELS, GIVEN | PIXELS | KEEP):
        for names in (order, order[::-1], order):
            for s, n in enumerate(names):
                c = K.case(shape, n)
                lb.load_gray(s, c.image, c.lo, c.hi)
            lb.run(stages)
            for s, n in enumerate(names):
                edges, masked = _want(shape, n)
                assert np.array_equal(lb.points(s), _list(masked)), (stages, s, n)
                if stages & KEEP:
                    got = lb.view(2, np.uint8, (len(order), h, w))[s]
                    assert np.array_equal(got, edges), (s, n, _diff(got, edges))
    for lit, dark in ((order[0], order[4]), (order[3], order[1])):          # the twins really differ: the slots changed content
        assert _want(shape, lit)[0].sum() > _want(shape, dark)[0].sum()


@pytest.mark.parametrize("shape,name", _BPAIRS, ids=_BIDS)
def test_chains_through_the_bgr_front_ends(shape, name):
    """b = g = r frames: the fused front end applies the thresholds inside the hysteresis pass (64 x 32, 100 x 528), the streaming
    (90 x 300) and generic (75 x 333) front ends before it.  Thresholds, edge map and point list against LaneRef().stages."""
    h, w = shape
    frame = K.bgr_case(shape, name)[1]
    want = _want_bgr(shape, name)
    lb = LaneBatch(1, h, w, MS, [frame])
    lb.run(PIXELS | KEEP)
    thr = lb.view(4, np.float64, (4,))
    assert (thr[0], thr[1], thr[2]) == (want["lo"], want["hi"], want["median"])
    got = lb.view(2, np.uint8, (h, w))
    assert np.array_equal(got, want["edges"]), _diff(got, want["edges"])
    assert np.array_equal(lb.view(3, np.uint8, (h, w)), want["masked"])
    lb.run(PIXELS)
    thr = lb.view(4, np.float64, (4,))
    assert (thr[0], thr[1], thr[2]) == (want["lo"], want["hi"], want["median"])
    assert np.array_equal(lb.points(0), _list(want["masked"]))


@pytest.mark.parametrize("shape", K.BGR_SHAPES, ids=["%dx%d" % s for s in K.BGR_SHAPES])
def test_bgr_batches_reuse_the_workspace(shape):
    """The seeded serpentine, its unseeded twin, a seam chain and its cut twin in one call, then in reverse order on the same
    workspace (production shape): each slot then holds the twin of what it held."""
    import torch
    h, w = shape
    order = ["serpentine_seed_last", "seam_diag_hseam_cut", "seam_4conn_hseam", "seam_diag_hseam", "serpentine_no_seed"]
    lb = LaneBatch(len(order), h, w, MS)
    for names in (order, order[::-1], order):
        bgr = torch.as_tensor(np.stack([K.bgr_case(shape, n)[1] for n in names])).to("cuda")
        lb.run(PIXELS, bgr=bgr)
        thr = lb.view(4, np.float64, (len(order), 4))
        for s, n in enumerate(names):
            want = _want_bgr(shape, n)
            assert (thr[s, 0], thr[s, 1], thr[s, 2]) == (want["lo"], want["hi"], want["median"]), (s, n)
            assert np.array_equal(lb.points(s), _list(want["masked"])), (s, n)
