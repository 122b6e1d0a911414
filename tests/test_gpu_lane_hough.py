"""The three progressive-probabilistic-Hough kernels on hand-made point lists (tests/lane_cases.py), through the Hough-only
hook of av_lane_detect (stage bits 16; 16 | 8 runs the generic kernel alone): configurations other than the detector's
(50, 50, 150), the segment cap, the capacity verdicts that hand a frame from the theta-sharded kernel to the
single-workgroup one and on to the generic one, and the generic kernel's two mask sources.  Every frame's segment list must
be the oracle's cv::HoughLinesProbabilistic restatement's, element for element and in order, made by the expected kernel."""
import numpy as np
import pytest

from tests import lane_cases as K
from tests._util import LaneBatch

pytestmark = pytest.mark.gpu

HOUGH, GENERIC = 16, 16 | 8
_WANT = {}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


def want_segments(key, pic, cfg, MS):
    """The oracle's segments for one picture, computed once per (picture, configuration, cap)."""
    k = (key, pic.shape, tuple(cfg), MS)
    if k not in _WANT:
        from oracle.lane_ref import houghp
        _WANT[k] = houghp(pic, *cfg, max_lines=MS)
    return _WANT[k]


def run_hough(lb, pics, stages, dirty_mask=False):
    """Reload every frame's list, run the Hough stage, return (nseg, segments, kernel per frame, info, point counts).
    dirty_mask: the masked byte map (view 3) is set to all-ones after the lists are loaded."""
    counts = [lb.load_points(s, p) for s, p in enumerate(pics)]
    if dirty_mask:
        lb._put(3, 0, np.full(lb.S * lb.h * lb.w, 255, np.uint8))
    lb.run(stages)
    return (lb.view(6, np.int32, (lb.S,)).copy(), lb.view(5, np.int32, (lb.S, lb.MS, 4)).copy(), lb.view(8, np.int32, (lb.S,)).copy(),
            lb.info.cpu().numpy(), counts)


def check_batch(lb, keys, pics, cfg, stages, kernels, dirty_mask=False):
    """One Hough-only call on `pics` (one per frame) against the oracle.  Returns the oracle's segment counts."""
    nseg, segs, path, info, counts = run_hough(lb, pics, stages, dirty_mask)
    wants = [want_segments(k, p, cfg, lb.MS) for k, p in zip(keys, pics)]
    for s, want in enumerate(wants):
        tag = (cfg, stages, keys[s])
        assert nseg[s] == len(want), (tag, int(nseg[s]), len(want), int(path[s]))
        assert np.array_equal(segs[s, :nseg[s]], want), (tag, segs[s, :nseg[s]].tolist(), want.tolist())
        assert path[s] == kernels[s], (tag, int(path[s]), kernels[s])
        assert info[s, 4] == nseg[s] and info[s, 5] == counts[s], (tag, info[s].tolist(), counts[s])
    return [len(x) for x in wants]


def batch(S, shape, MS, cfg):
    return LaneBatch(S, shape[0], shape[1], MS, None, *cfg)


A_KEYS = ["mixed", "empty", "single", "threshold", "border", "seams", "noise", "length"]


@pytest.mark.parametrize("cfg,kernel", K.A_CONFIGS, ids=["%d-%d-%d" % c for c, _ in K.A_CONFIGS])
def test_small_pictures_under_every_configuration(cfg, kernel):
    """Eight 96 x 160 pictures as the frames of one batch (32 workgroups: the permuted frame-to-workgroup map) under seven
    configurations: the general gap loop (gaps 3, 4, 1), the two sides of its word-at-a-time shortcut (62, 63), the `>=` of
    the vote threshold and of the length rule, walks that start on the border, the seams between theta sub-shards, counts
    that go negative, and gap 0, which the sharded and the single-workgroup kernel both hand on to the generic one."""
    pics = K.pictures_a(cfg)
    lb = batch(K.A_S, K.A_SHAPE, K.A_MS, cfg)
    n = check_batch(lb, A_KEYS, pics, cfg, HOUGH, [kernel] * K.A_S)
    assert max(n) < K.A_MS and n[1] == 0 and n[2] == 0


def test_point_count_boundaries():
    """A dense hatch cut to exactly 4 096, 4 097, 12 288 and 12 289 points: the last list each kernel still takes and the
    first one it hands on."""
    pics = K.pictures_b()
    keys = ["hatch%d" % n for n in K.B_COUNTS]
    for cfg in K.B_CONFIGS:
        lb = batch(len(pics), K.B_SHAPE, K.B_MS, cfg)
        n = check_batch(lb, keys, pics, cfg, HOUGH, list(K.B_KERNELS))
        assert lb.info.cpu().numpy()[:, 5].tolist() == list(K.B_COUNTS) and max(n) < K.B_MS


@pytest.mark.parametrize("shape", [(320, 1024), (160, 1616), (720, 1280)], ids=["320x1024", "160x1616", "720x1280"])
def test_geometry_verdicts(shape):
    """Sparse lists whose bounding box, not their length, decides the kernel: the bitmap caps of the sharded (9 216 words, reached
    exactly by the 720p default box) and the single-workgroup kernel (16 384), and the sharded kernel's accumulator cap."""
    cases = [c for c in K.C_CASES if c[0] == shape]
    pics = [K.sparse_lines(shape, box) for _, box, _, _ in cases]
    keys = ["sparse%s" % (box,) for _, box, _, _ in cases]
    for cfg in K.C_CONFIGS:
        lb = batch(len(pics), shape, 256, cfg)
        n = check_batch(lb, keys, pics, cfg, HOUGH, [k for _, _, k, _ in cases])
        assert 0 < min(n) and max(n) < 256


@pytest.mark.parametrize("cfg,stages,kernel", [((15, 30, 0), HOUGH, 3), ((20, 20, 4), GENERIC, 3), ((10, 10, 1), GENERIC, 3),
                                               ((20, 20, 4), HOUGH, 1)], ids=["chain-gap0", "alone-gap4", "alone-gap1", "sharded-gap4"])
def test_generic_kernel_reads_the_byte_map_at_odd_widths(cfg, stages, kernel):
    """96 x 150: no bit-map path at this width, so the generic kernel walks the masked byte map (view 3) as it was written,
    reached through the hand-over chain (gap 0) and alone (stage bit 8); the sharded kernel at the same width for contrast."""
    shape = (96, 150)
    pics = K.pictures_a(cfg, shape)
    lb = batch(K.A_S, shape, K.A_MS, cfg)
    check_batch(lb, A_KEYS, pics, cfg, stages, [kernel] * K.A_S)


def test_generic_kernel_rebuilds_its_mask_between_runs():
    """96 x 160, generic kernel alone, two different sets of pictures on one workspace: the mask the kernel rebuilds from the
    second list must hold nothing the first run's walks left (pixels no line erased stay set in the byte map), nor anything
    else that lies in the byte map: it is set to all-ones before the second run."""
    cfg = (20, 20, 4)
    pics = K.pictures_a(cfg)
    lb = batch(K.A_S, K.A_SHAPE, K.A_MS, cfg)
    check_batch(lb, A_KEYS, pics, cfg, GENERIC, [3] * K.A_S)
    left = lb.view(3, np.uint8, (K.A_S,) + K.A_SHAPE)
    assert left.any()                                                   # the first run did leave pixels behind
    rolled = pics[3:] + pics[:3]
    check_batch(lb, A_KEYS[3:] + A_KEYS[:3], rolled, cfg, GENERIC, [3] * K.A_S, dirty_mask=True)


@pytest.mark.parametrize("stages,kernel", [(HOUGH, 1), (GENERIC, 3)], ids=["sharded", "generic"])
@pytest.mark.parametrize("MS", [4, 22, 64])
def test_segment_cap(MS, stages, kernel):
    """22 horizontal lines under (30, 30, 2) with max_segments 4 (capped), 22 (the cap reached by the last line) and 64: the
    device list is the oracle's first MS segments and the fit reads exactly that many.  Frame 1 holds another picture, so a
    capped frame 0 must also leave frame 1's rows of the segment array alone."""
    pics = [K.cap_picture(), K.mixed_picture()]
    lb = batch(2, K.A_SHAPE, MS, K.E_CONFIG)
    n = check_batch(lb, ["cap", "mixed"], pics, K.E_CONFIG, stages, [kernel] * 2)
    assert n[0] == min(MS, K.E_LINES)
    assert lb.info.cpu().numpy()[0, 4] == min(MS, K.E_LINES)


def test_segment_cap_single_workgroup_kernel():
    """The 4 097-point hatch (single-workgroup kernel) beside the 4 096-point one (sharded) with max_segments 8."""
    pics = K.pictures_b()[1::-1]
    lb = batch(2, K.B_SHAPE, K.E_FAST_MS, K.E_FAST_CONFIG)
    n = check_batch(lb, ["hatch4097", "hatch4096"], pics, K.E_FAST_CONFIG, HOUGH, [2, 1])
    assert n == [K.E_FAST_MS] * 2 and lb.info.cpu().numpy()[:, 4].tolist() == n


def test_sharded_hough_repeats_itself_under_a_small_gap():
    """Batch A under (20, 20, 3), three runs from reloaded lists: identical segments each time."""
    cfg = (20, 20, 3)
    pics = K.pictures_a(cfg)
    lb = batch(K.A_S, K.A_SHAPE, K.A_MS, cfg)
    runs = [run_hough(lb, pics, HOUGH)[:3] for _ in range(3)]
    for nseg, segs, path in runs:
        assert path.tolist() == [1] * K.A_S
        assert np.array_equal(nseg, runs[0][0])
        for s in range(K.A_S):
            assert np.array_equal(segs[s, :nseg[s]], runs[0][1][s, :nseg[s]]), s
            assert np.array_equal(segs[s, :nseg[s]], want_segments(A_KEYS[s], pics[s], cfg, K.A_MS)), s
