"""Slope split, quadratic fit, EMA and resampling on hand-made segment lists (tests/lane_cases.py), through the fit-only hook of
av_lane_detect (stage bits 16 | 32), against oracle.lane_ref.separate + fit carried from call to call.

Tolerances: coefficients rtol = atol = 1e-6 (tests/test_gpu_lane.py); a float64 host emulation of the device algorithm (scaled
Gram matrix, eigen-decomposition) uses less than a thousandth of that on these lists and stays below 1e-8 pixel on the curve.  The
sample rows must equal the oracle's exactly; the abscissae must equal the oracle's wherever its float64 abscissa lies farther
than 1e-4 from an integer (at least 49 of 50 points in every case: tests/test_lane_cases_host.py) and within 1 elsewhere."""
import numpy as np
import pytest

from tests import lane_cases as K
from tests._util import LaneBatch

pytestmark = pytest.mark.gpu

FIT = 16 | 32
CASES = {c[0]: c for c in K.fit_cases()}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


def reference(name):
    if name not in _REF:
        _REF[name] = K.fit_reference(CASES[name])
    return _REF[name]


def check_call(lb, row, want, tag):
    """One fit-only call on `row` (a segment list per stream) against the oracle's results `want`."""
    for s, segs in enumerate(row):
        lb.load_segments(s, segs)
    before = lb.state.cpu().numpy().copy()
    lb.run(FIT)
    info, poly, pts, conf, state = (t.cpu().numpy() for t in (lb.info, lb.poly, lb.pts, lb.conf, lb.state))
    for s, exp in enumerate(want):
        assert info[s, 4] == exp["n"], (tag, s)
        assert tuple(info[s, 2:4]) == exp["kept"], (tag, s, info[s].tolist(), exp["kept"])
        for side, f in enumerate(exp["sides"]):
            at = (tag, s, side)
            st = state[s, 4 * side:4 * side + 4]
            assert bool(info[s, side]) == (f is not None), at
            if exp["state"][side] is None:
                assert st[3] == 0.0, at
            else:
                assert st[3] == 1.0, at
                np.testing.assert_allclose(st[:3], exp["state"][side], rtol=1e-6, atol=1e-6, err_msg=str(at))
            if f is None:
                # a side that vanishes reports nothing and keeps its state to the bit
                assert conf[s, side] == 0.0, at
                assert np.array_equal(st, before[s, 4 * side:4 * side + 4]), at
                continue
            p, c, co, xf = f
            assert conf[s, side] == c == min(1.0, exp["kept"][side] / 10), at
            np.testing.assert_allclose(poly[s, side], co, rtol=1e-6, atol=1e-6, err_msg=str(at))
            assert np.array_equal(state[s, 4 * side:4 * side + 3], poly[s, side]), at
            assert np.array_equal(pts[s, side, :, 1], p[:, 1]), (at, pts[s, side, :, 1].tolist(), p[:, 1].tolist())
            far = np.abs(xf - np.rint(xf)) > 1e-4
            assert np.array_equal(pts[s, side, far, 0], p[far, 0]), (at, pts[s, side, :, 0].tolist(), p[:, 0].tolist())
            assert np.abs(pts[s, side, :, 0].astype(np.int64) - p[:, 0]).max() <= 1, at
    return info, poly, pts


def run_case(name):
    _, h, w, MS, smoothing, calls = CASES[name]
    lb = LaneBatch(len(calls[0]), h, w, MS, None, smoothing=smoothing)
    want = reference(name)
    out = None
    for c, row in enumerate(calls):
        out = check_call(lb, row, want[c], (name, c))
    return lb, out


def test_slope_filter_and_side_rule():
    """|slope| == 0.3 exactly is kept, 0.25 and vertical are dropped, a midpoint exactly on w / 2 belongs to neither side, a
    slope of the wrong sign for its half is dropped, endpoint order does not matter: every decision through info[2:4]."""
    segs, nl, nr = K.filter_list(640)
    lb = LaneBatch(1, 480, 640, 64, None)
    want = reference("filter")[0]
    assert want[0]["kept"] == (nl, nr)
    check_call(lb, [segs], want, "filter")
    # one segment at a time: the verdict of every entry on its own
    from oracle.lane_ref import separate
    for k in range(len(segs)):
        left, right = separate(segs[k:k + 1], 640)
        lb.load_segments(0, segs[k:k + 1])
        lb.run(FIT)
        assert tuple(lb.info.cpu().numpy()[0, 2:4]) == (len(left), len(right)), (k, segs[k].tolist())


def test_counts_and_confidence_over_streams():
    """Six streams with different lists in one call: 1, 9, 10, 11 kept segments per side (the confidence ramp min(1, n / 10) on
    both sides of its knee) and a full list of max_segments = 64 entries, all kept, on either side."""
    lb, (info, _, _) = run_case("counts")
    assert info[:, 2:4].tolist() == [[1, 1], [9, 9], [10, 10], [11, 11], [64, 0], [0, 64]]
    assert lb.conf.cpu().numpy().tolist() == [[0.1, 0.1], [0.9, 0.9], [1.0, 1.0], [1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]
    assert info[:, 4].tolist() == [2, 18, 20, 22, 64, 64]


def test_rank_deficient_lists():
    """One segment, endpoints on two rows (rank 2: the minimum-norm solution of the scaled problem) and on three rows (rank
    3): coefficients as everywhere, and the curves agree below 1e-5 pixel over the fitted rows."""
    lb, (_, poly, _) = run_case("rank")
    for s, (_, segs) in enumerate(K.rank_lists()):
        co = reference("rank")[0][s]["sides"][0][2]
        yy = np.linspace(segs[:, [1, 3]].min(), segs[:, [1, 3]].max(), 7)
        err = float(np.abs(np.polyval(poly[s, 0], yy) - np.polyval(co, yy)).max())
        print("rank case %d: max |x_device - x_polyfit| over the fitted rows %.2e px" % (s, err))
        assert err < 1e-5, (s, err)


def test_abscissae_outside_the_frame():
    """Curves that run below 0 and past w over rows 0.6 h .. h: no clamp, truncation toward zero on both signs."""
    _, (_, _, pts) = run_case("outside")
    assert pts[0, 0, :, 0].min() < 0 and pts[0, 1, :, 0].max() > 1280


@pytest.mark.parametrize("h,k,row", K.SAMPLE_HEIGHTS + [(720, 0, 432)], ids=["343", "441", "511", "720"])
def test_sample_rows(h, k, row):
    """Heights at which a sample row of np.linspace(0.6 h, h, 50) is an integer that lane * step + ya only reaches when the
    multiply and the add round separately (a fused multiply-add lands one ulp below and truncates to the row above)."""
    _, (_, _, pts) = run_case("rows%d" % h)
    assert pts[0, 0, k, 1] == row and pts[1, 1, k, 1] == row and pts[0, 0, 49, 1] == h


@pytest.mark.parametrize("smoothing", K.EMA_SMOOTHINGS)
def test_ema_across_dropouts(smoothing):
    """Four streams over six calls -- never empty, the left side gone in call 2, both sides gone in calls 2-3, always empty --
    with smoothing 0.7, 0.0 (no memory) and 0.95; then zeroing `state` starts afresh."""
    name = "ema%g" % smoothing
    lb, _ = run_case(name)
    want = reference(name)
    assert [r["kept"] for r in want[2]][1][0] == 0 and [r["kept"] for r in want[2]][1][1] > 0
    assert want[3][2]["kept"] == (0, 0) and all(r[3]["kept"] == (0, 0) for r in want)
    assert (lb.state.cpu().numpy()[3] == 0).all()
    lb.state.zero_()
    _, h, w, MS, _, calls = CASES[name]
    fresh = K.fit_reference((name, h, w, MS, smoothing, calls[5:6]))
    check_call(lb, calls[5], fresh[0], (name, "afresh"))
