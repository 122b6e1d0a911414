"""Conditions on the hand-made lane inputs (tests/lane_cases.py), proved with the oracle alone: the GPU tests of the Hough
and fit stages only tell a wrong kernel from a right one if the inputs really sit where they claim to."""
import numpy as np
import pytest

from tests import lane_cases as K


@pytest.fixture(scope="module")
def houghp():
    from oracle.lane_ref import houghp
    return houghp


def _all_pictures():
    for cfg, _ in K.A_CONFIGS:
        for shape in (K.A_SHAPE, (96, 150)):
            for p in K.pictures_a(cfg, shape):
                yield p
    for p in K.pictures_b():
        yield p
    for shape, box, _, _ in K.C_CASES:
        yield K.sparse_lines(shape, box)
    yield K.cap_picture()


def test_point_lists_are_strictly_increasing_and_inside_the_frame():
    for p in _all_pictures():
        pl = K.point_list(p)
        key = ((pl >> 16).astype(np.int64) << 16) | (pl & 0xffff)
        assert (np.diff(key) > 0).all()
        assert ((pl & 0xffff) < p.shape[1]).all() and ((pl >> 16) < p.shape[0]).all()
        assert p.shape[0] < 32768 and p.shape[1] < 32768


def test_batch_a_sizes_and_kernels():
    for cfg, kernel in K.A_CONFIGS:
        pics = K.pictures_a(cfg)
        assert len(pics) == K.A_S and 4 * K.A_S % 32 == 0                  # 32 workgroups: the permuted frame map
        lists = [K.point_list(p) for p in pics]
        assert len(lists[1]) == 0 and len(lists[2]) == 1
        assert [K.expected_kernel(pl, K.A_SHAPE, cfg[2]) for pl in lists] == [kernel] * K.A_S
        assert [K.expected_kernel(K.point_list(p), (96, 150), cfg[2]) for p in K.pictures_a(cfg, (96, 150))] == [kernel] * K.A_S


def test_point_count_boundaries_have_the_four_counts():
    lists = [K.point_list(p) for p in K.pictures_b()]
    assert [len(pl) for pl in lists] == [4096, 4097, 12288, 12289] == [K.HS_NZ, K.HS_NZ + 1, K.NZCAP, K.NZCAP + 1]
    for cfg in K.B_CONFIGS:
        assert [K.expected_kernel(pl, K.B_SHAPE, cfg[2]) for pl in lists] == list(K.B_KERNELS)
    # the count alone decides here: bitmap and accumulator are far inside their caps
    for pl in lists:
        bmw, cells, bmw_fast = K.geometry(pl, K.B_SHAPE)
        assert bmw <= K.HS_BMW // 2 and cells <= K.HS_ACCW and bmw_fast <= K.BMWORDS // 2


def test_geometry_cases_give_the_stated_verdicts():
    figures = []
    for shape, box, kernel, _ in K.C_CASES:
        pl = K.point_list(K.sparse_lines(shape, box))
        assert 200 <= len(pl) <= K.HS_NZ
        figures.append(K.geometry(pl, shape))
        for cfg in K.C_CONFIGS:
            assert K.expected_kernel(pl, shape, cfg[2]) == kernel
    (b0, c0, f0), (b1, c1, f1), (b2, c2, f2), (b3, c3, f3) = figures
    assert b0 == 10240 > K.HS_BMW and f0 == 10240 <= K.BMWORDS                          # 320 x 1024: the sharded bitmap cap
    assert b1 == 8160 <= K.HS_BMW and c1 == 14014 > 2 * K.HS_ACCW and f1 <= K.BMWORDS   # 160 x 1616: the accumulator cap
    assert b2 == 28800 > K.HS_BMW and f2 == 28800 > K.BMWORDS                           # 720p: both bitmap caps
    assert b3 == 9216 == K.HS_BMW and c3 <= 2 * K.HS_ACCW                               # the 720p default box: exactly the cap


def test_gap_decides_segments_in_batch_a(houghp):
    for a, b in (((20, 20, 3), (20, 20, 4)), ((30, 10, 62), (30, 10, 63))):
        differ = [not np.array_equal(houghp(p, *a, max_lines=K.A_MS), houghp(q, *b, max_lines=K.A_MS))
                  for p, q in zip(K.pictures_a(a), K.pictures_a(b))]
        assert any(differ), (a, b)
    # the hole of exactly 63 pixels in the mixed picture's bottom row
    row = K.mixed_picture()[K.A_SHAPE[0] - 2] != 0
    on = np.flatnonzero(row)
    assert np.diff(on).max() == 64
    # the dashed diagonal exists with a gap of 4 and not with 3
    d3 = houghp(K.mixed_picture(), 20, 20, 3, max_lines=K.A_MS).tolist()
    d4 = houghp(K.mixed_picture(), 20, 20, 4, max_lines=K.A_MS).tolist()
    assert [10, 2, 100, 92] in d4 and [10, 2, 100, 92] not in d3


def test_threshold_and_length_pictures_pin_their_rules(houghp):
    for cfg, _ in K.A_CONFIGS:
        t, L, gap = cfg
        segs = houghp(K.threshold_picture(K.A_SHAPE, t, gap), *cfg, max_lines=K.A_MS)
        rows = set(segs[:, 1].tolist()) | set(segs[:, 3].tolist())
        assert K.A_SHAPE[0] // 4 not in rows                                # threshold - 1 points never make a line
        if gap >= 1:
            assert rows == {3 * K.A_SHAPE[0] // 4}                          # threshold points do
        if t <= L:
            segs = houghp(K.length_picture(K.A_SHAPE, L), *cfg, max_lines=K.A_MS)
            ext = sorted(np.maximum(np.abs(segs[:, 2] - segs[:, 0]), np.abs(segs[:, 3] - segs[:, 1])).tolist())
            assert len(ext) == 4 and ext[0] == L and ext[-1] == L + 1, (cfg, ext)       # two dashes of six fall to the rule


def test_no_small_picture_reaches_the_cap(houghp):
    for cfg, _ in K.A_CONFIGS:
        assert max(len(houghp(p, *cfg, max_lines=4096)) for p in K.pictures_a(cfg)) < K.A_MS


def test_cap_pictures_exceed_their_caps(houghp):
    assert len(houghp(K.cap_picture(), *K.E_CONFIG, max_lines=4096)) == K.E_LINES > 4
    pl = K.point_list(K.cap_picture())
    assert K.expected_kernel(pl, K.A_SHAPE, K.E_CONFIG[2]) == 1
    for p, kernel in zip(K.pictures_b()[:2], (1, 2)):
        assert len(houghp(p, *K.E_FAST_CONFIG, max_lines=4096)) > K.E_FAST_MS
        assert K.expected_kernel(K.point_list(p), K.B_SHAPE, K.E_FAST_CONFIG[2]) == kernel


def test_fit_cases_keep_the_counts_they_claim():
    from oracle.lane_ref import separate
    segs, nl, nr = K.filter_list(640)
    left, right = separate(segs, 640)
    assert (len(left), len(right)) == (nl, nr)
    kept = [tuple(map(len, separate(segs[k:k + 1], 640))) for k in range(len(segs))]
    assert kept == [(1, 0), (1, 0), (0, 1), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (1, 0), (0, 1), (0, 0), (0, 0), (1, 0), (0, 1), (0, 1)]
    for segs, nl, nr in K.count_lists(64, 720, 1280):
        left, right = separate(segs, 1280)
        assert (len(left), len(right)) == (nl, nr) and len(segs) == nl + nr <= 64
    for _, segs in K.rank_lists():
        assert len(separate(segs, 1280)[0]) == len(segs)
    assert [len(np.unique(segs[:, [1, 3]])) for _, segs in K.rank_lists()] == [2, 2, 3]
    assert tuple(map(len, separate(K.outside_list(720, 1280), 1280))) == (3, 3)


def test_fit_cases_are_mostly_compared_exactly():
    for case in K.fit_cases():
        fitted = 0
        for c, row in enumerate(K.fit_reference(case)):
            for s, res in enumerate(row):
                for f in res["sides"]:
                    if f is None:
                        continue
                    fitted += 1
                    xf = f[3]
                    assert int((np.abs(xf - np.rint(xf)) > 1e-4).sum()) >= 45, (case[0], c, s)
        assert fitted > 0, case[0]
    out = K.fit_reference([c for c in K.fit_cases() if c[0] == "outside"][0])[0][0]["sides"]
    assert out[0][0][:, 0].min() < 0 and out[1][0][:, 0].max() > 1280


def test_sample_heights_hit_integer_rows():
    for h, k, row in K.SAMPLE_HEIGHTS:
        yp = np.linspace(h * 0.6, h, 50)
        assert yp[k] == row                                                  # exactly: astype(int32) keeps the row
        step = (h - h * 0.6) / 49.0
        assert k * step + h * 0.6 == row
        # what one rounding instead of two gives (exact rational arithmetic, rounded once): one ulp below
        from fractions import Fraction
        fused = float(Fraction(k) * Fraction(step) + Fraction(h * 0.6))
        assert fused < row and int(fused) == row - 1


def test_ema_dropout_patterns():
    ref = K.fit_reference([c for c in K.fit_cases() if c[0] == "ema0.7"][0])
    kept = [[r["kept"] for r in row] for row in ref]
    assert len(kept) == 6 and all(len(row) == 4 for row in kept)
    assert all(min(row[0]) > 0 for row in kept)                                        # stream 0: never empty
    assert kept[2][1][0] == 0 and kept[2][1][1] > 0 and min(kept[1][1]) > 0 and min(kept[3][1]) > 0
    assert kept[2][2] == kept[3][2] == (0, 0) and min(kept[1][2]) > 0 and min(kept[4][2]) > 0
    assert all(row[3] == (0, 0) for row in kept)                                       # stream 3: always empty
