"""The YOLO tail's hand-made candidate lists (tests/yolo_tail_cases.py) sit where they claim, shown with the oracle alone: counts at the
chunk and round edges, the radix pass counts, the chain list's masks, and per family a deliberately wrong NMS that the family tells
from the right one.  No device: tests/test_gpu_yolo_tail.py runs the lists through the library."""
import numpy as np
import pytest

from tests import yolo_tail_cases as K
from oracle import yolo_ref as R

pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered")        # (0 / 0 IoU of zero-area boxes is a case)

ANCHORS = sorted(K.FRAMES)
# the anchor counts at which the variant comparisons run (each is a NumPy NMS per case and variant): the smallest, and the largest
VARIANT_ANCHORS = (420, 7980)


def test_frames_give_the_anchor_counts_and_both_sort_kernels():
    for A, (h, w) in K.FRAMES.items():
        assert K.n_anchors(h, w) == A
    assert [K.digit_bits(A) for A in ANCHORS] == [8, 8, 8, 8, 7, 7] and (7140 + 1023) // 1024 == 7 and (7560 + 1023) // 1024 == 8
    _, nh, nw, top, left, H, W = R.letterbox_shape(*K.FRAMES[2520])
    assert (H, W, top, H - top - nh, left) == (192, 640, 9, 10, 0) and abs(min(H / 90, W / 333) - 1.92) < 0.01


@pytest.mark.parametrize("A", ANCHORS)
def test_counts_sit_on_the_chunk_and_round_edges(A):
    cases = K.family(A, "counts")
    want = [n for n in (0, 1, 63, 64, 65, 128, 129, 1023, 1024, 1025, A - 1, A) if n <= A]
    assert sorted(c["n"] for c in cases) == sorted(set(want))
    for c in cases:
        ok = K.passing(c)
        assert ok.sum() == c["n"]
        a = np.nonzero(ok)[0]
        if 1 < c["n"] < A:                                          # scattered: over the whole anchor range, not one run
            assert a.min() < A // 4 and a.max() > 3 * A // 4 and (np.diff(a) > 1).any()
        assert len(np.unique(c["conf"][ok])) == c["n"]
    ns = {c["n"] for c in cases}
    assert {0, 1, 63, 64, 65, 128, 129, A - 1, A} <= ns and (A < 1025 or {1023, 1024, 1025} <= ns)
    # disjoint boxes: all kept up to max_det
    for c in cases:
        if c["n"] <= 129:
            assert len(K.expected(c)[0]) == min(c["n"], c["max_det"])


@pytest.mark.parametrize("A", ANCHORS)
def test_ties_and_pass_counts(A):
    db = K.digit_bits(A)
    ties = {c["name"]: c for c in K.family(A, "ties")}
    three = ties["ties_three"]
    assert K.passing(three).all() and len(np.unique(three["conf"])) == 3
    rounds = np.arange(A) // 1024
    for v in np.unique(three["conf"]):                              # every value in every round of 1 024 and in every wave of 64
        assert len(np.unique(rounds[three["conf"] == v])) == rounds.max() + 1
        assert len(np.unique((np.arange(A) // 64)[three["conf"] == v])) == (A + 63) // 64
    assert len(np.unique(ties["ties_equal"]["conf"])) == 1 and (ties["ties_ones"]["conf"].view(np.uint32) == K.ONE).all()
    assert K.radix_passes(ties["ties_ones"]) == 0
    # the deep lists show ranks beyond max_det: the kept boxes after the first come from the second / third value
    for deep in (1, 2):
        c = ties["ties_deep%d" % deep]
        keep = K.expected(c)[0]
        vals = np.sort(np.unique(c["conf"]))[::-1]
        assert [c["conf"][k] for k in keep[:deep]] == list(vals[:deep]) and (c["conf"][keep[deep:]] <= vals[deep]).all()
        assert c["conf"][keep[deep]] == vals[deep]
        first_rank = int((c["conf"] > vals[deep]).sum())
        assert len(keep) > deep and first_rank > A // (4 - deep) - A // 10
    passes = {c["name"]: K.radix_passes(c) for c in K.family(A, "passes")}
    assert all(K.passing(c).all() for c in K.family(A, "passes"))
    want = {8: dict(passes_ulp127=1, passes_ulp255=1, passes_ulp65535=2, **{"passes_spread_0.25": 3, "passes_spread_0.001": 4}),
            7: dict(passes_ulp127=1, passes_ulp255=2, passes_ulp65535=3, **{"passes_spread_0.25": 4, "passes_spread_0.001": 4})}[db]
    assert passes == want
    # with the ties lists: every pass count from 0 to 4, so the ping-pong buffer ends in either half
    assert {0, K.radix_passes(three)} | set(passes.values()) == {0, 1, 2, 3, 4}
    for c in K.family(A, "passes"):
        v = K.ONE - c["conf"].view(np.uint32).astype(np.int64)
        assert v.min() >= 0 and len(np.unique(v)) < A               # ties in every list


@pytest.mark.parametrize("A", ANCHORS)
def test_threshold_lists_hold_the_threshold_and_its_neighbours(A):
    for c in K.family(A, "threshold"):
        t = np.float32(c["conf_thres"])
        conf = c["conf"]
        for v in (t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))):
            assert (conf == v).sum() > 0
        assert not K.passing(c)[conf == t].any() and K.passing(c)[conf == np.nextafter(t, np.float32(1))].all()
        if c.get("masked"):
            assert np.isnan(conf).sum() >= 2 and np.isinf(conf).sum() >= 2 and (conf == np.float32(1.5)).any() and (conf == -1).any()
            assert (conf == np.nextafter(np.float32(1), np.float32(2))).any() and K.passing(c)[conf == 1].all() and (conf == 1).any()
            assert not K.passing(c)[~((conf > t) & (conf <= 1))].any()


@pytest.mark.parametrize("A", ANCHORS)
def test_exact_iou_pairs(A):
    at, below = K.family(A, "exact_iou")
    assert np.float32(at["iou_thres"]) == np.float32(0.5) and np.float32(below["iou_thres"]) == np.nextafter(np.float32(0.5), np.float32(0))
    order = K.sorted_anchors(at)
    pairs = at["pairs"]
    # the 0.5 pairs: IoU exactly 0.5 in float32 with the class offset applied; the others: identical boxes
    b = (at["box"][order] + (at["cls"][order].astype(np.float32) * np.float32(7680))[:, None]).astype(np.float32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    for kind, i, j in pairs:
        if kind == "half":
            inter = (min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0])) * (min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            assert inter / (area[i] + area[j] - inter) == np.float32(0.5) and at["cls"][order[i]] == at["cls"][order[j]]
        else:
            assert np.array_equal(at["box"][order[i]], at["box"][order[j]]) and (area[i] == 0) == (kind in ("point", "line"))
            assert (at["cls"][order[i]] != at["cls"][order[j]]) == (kind == "classes")
    assert sorted(k for k, _, _ in pairs) == ["classes"] * 3 + ["half"] * 6 + ["line"] * 3 + ["point"] * 3
    for kind in ("half", "classes", "point", "line"):               # decided in the chunk, against the previous chunk, against an earlier one
        d = sorted(j // 64 - i // 64 for k, i, j in pairs if k == kind)
        assert d[0] == 0 and 1 in d and d[-1] >= 2, (kind, d)
    slots = [r for _, i, j in pairs for r in (i, j)]
    keep_at, keep_below = set(K.expected(at)[0].tolist()), set(K.expected(below)[0].tolist())
    assert all(order[r] in keep_at for r in slots)                   # strict comparison; classes apart; NaN is "not suppressed"
    dropped = sorted(int(np.nonzero(order == a)[0][0]) for a in keep_at - keep_below)
    assert len(dropped) == 6 and keep_below < keep_at
    assert dropped == sorted(j for k, _, j in pairs if k == "half")


@pytest.mark.parametrize("A", ANCHORS)
def test_chain_list_reaches_every_mask(A):
    for c in K.family(A, "chains"):
        m = K.mask_counts(c)
        print(A, c["name"], m)
        assert m["same"] > 0 and m["prev"] > 0 and m["early"] > 0 and (m["spared"] > 0 or c["max_det"] == 300), m
        assert (m["kept"] == 300) == (c["max_det"] == 300)          # the second list is cut inside the third segment
        order = K.sorted_anchors(c)
        pos = 0
        for gap, clusters, members in K.chain_layout(A):            # a member's rank inside its segment is j gap + cluster
            n = (members - 1) * gap + clusters if gap > 1 else clusters * members
            seg = c["box"][order[pos:pos + n]]
            for cl in (0, clusters - 1):
                for j in range(1, members):
                    r0, r1 = ((j - 1) * gap + cl, j * gap + cl) if gap > 1 else (cl * members + j - 1, cl * members + j)
                    assert np.array_equal(seg[r1] - seg[r0], np.array([4, 0, 4, 0], np.float32)) and seg[r0][2] - seg[r0][0] == 20
            pos += n
        assert pos == K.passing(c).sum() <= A
    full = K.family(A, "chains")[0]
    assert K.mask_counts(full)["kept"] < full["max_det"]            # the whole list is walked


@pytest.mark.parametrize("A", ANCHORS)
def test_max_det_cuts_inside_a_chunk_and_at_its_end(A):
    cases = K.family(A, "max_det")
    assert [c["max_det"] for c in cases] == [1, 63, 64, 65, 300, 2500]
    assert all(K.passing(c).all() and len(np.unique(c["conf"])) == A for c in cases)
    assert [len(K.expected(c)[0]) for c in cases] == [min(A, m) for m in (1, 63, 64, 65, 300, 2500)]
    assert [c["max_det"] % 64 for c in cases] == [1, 63, 0, 1, 44, 4]


@pytest.mark.parametrize("A", ANCHORS)
def test_mapping_boxes_lie_inside_across_and_outside_the_picture(A):
    (c,) = K.family(A, "mapping")
    h, w = K.FRAMES[A]
    x0, y0, x1, y1 = c["rect"]
    order = K.sorted_anchors(c)
    b, kinds = c["box"][order], c["kinds"]
    inside = (b[:, 0] >= x0) & (b[:, 1] >= y0) & (b[:, 2] <= x1) & (b[:, 3] <= y1)
    outside = (b[:, 2] <= x0) | (b[:, 0] >= x1) | (b[:, 3] <= y0) | (b[:, 1] >= y1)
    assert np.array_equal(inside, kinds == 0) and np.array_equal(outside, kinds == 2) and [int((kinds == k).sum()) for k in range(3)] == [12, 12, 12]
    keep, box, _, _ = K.expected(c)
    assert len(keep) == 36
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    rank = {a: r for r, a in enumerate(order)}
    k = kinds[[rank[a] for a in keep]]
    assert (area[k == 2] == 0).all() and (area[k != 2] > 0).all()   # clipped away / clipped at an edge / untouched
    full = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[[rank[a] for a in keep]] / np.float32(min(R.letterbox_shape(h, w)[5] / h, R.letterbox_shape(h, w)[6] / w)) ** 2
    assert (area[k == 1] < 0.999 * full[k == 1]).all() and np.allclose(area[k == 0], full[k == 0], rtol=1e-3)
    if A == 2520:                                                   # the frame with padding rows: boxes wholly inside them
        H = R.letterbox_shape(h, w)[5]
        in_pad = (kinds == 2) & (b[:, 1] >= 0) & (b[:, 3] <= H) & (b[:, 0] >= 0) & (b[:, 2] <= 640)
        assert in_pad.sum() == 6


@pytest.mark.parametrize("A", VARIANT_ANCHORS)
@pytest.mark.parametrize("fam", K.FAMILIES)
def test_restatement_equals_the_oracle_and_each_family_catches_its_wrong_conventions(A, fam):
    cases = K.family(A, fam)
    for c in cases:
        assert np.array_equal(K.nms_variant(c), K.expected(c)[0]), c["name"]
    for wrong in K.catches(fam, A):
        caught = [c["name"] for c in cases if not np.array_equal(K.nms_variant(c, wrong), K.expected(c)[0])]
        print(A, fam, wrong, "caught by", caught)
        assert caught, (fam, wrong)


def test_every_wrong_convention_is_caught_by_some_family():
    assert set(w for ws in K.CATCHES.values() for w in ws) == set(K.WRONG)
