"""YOLO tail on hand-made candidate lists: av_yolo_tail (the forward's own threshold + sort and NMS launches, on given candidates)
against oracle/yolo_ref.py's nms + scale_boxes, bit for bit, on the lists of tests/yolo_tail_cases.py -- at 420, 1 260, 2 520 and
7 140 anchors (nms_sort_kernel<8> with 1, 2, 3 and 7 rounds) and at 7 560 and 7 980 (nms_sort_kernel<7>, which no network-driven
test reaches).  tests/test_yolo_tail_cases_host.py shows without a device that the lists sit on the edges they claim.

Every call carries three different lists (the case, a short partner list, an empty one), writes into outputs that lie between guard
words and are prefilled, and is repeated with the images reversed."""
import ctypes as C

import numpy as np
import pytest

from tests import yolo_tail_cases as K

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered")]    # (0 / 0 IoU of zero-area boxes is a case)

GUARD = 64                                           # words on either side of every output
FILL = {"n": -7, "box": -3.5, "conf": -2.5, "cls": -9}


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    from multimodal_autonomous_driving_perception_and_planning_amd.perception import yolo as Y
    from oracle import yolo_ref as R
    return torch, nat, Y, R


@pytest.fixture(scope="module", params=sorted(K.FRAMES), ids=lambda A: "A%d" % A)
def handle(env, request):
    """One scale-n handle per anchor count, batch 3, fp16 (the tail does not read the weights)."""
    torch, nat, Y, R = env
    A = request.param
    m = Y.YoloV8n("random:0", batch=3)
    m._prepare(*K.FRAMES[A])
    assert m.dims()[2] == A
    yield A, m
    m.close()


class Outputs:
    """det_n / det_box / det_conf / det_cls for one call, each between GUARD words, everything prefilled."""

    def __init__(self, torch, m, max_det):
        B = m.batch
        self.shapes = {"n": (B,), "box": (B, max_det, 4), "conf": (B, max_det), "cls": (B, max_det)}
        self.raw = {k: torch.full((2 * GUARD + int(np.prod(s)),), FILL[k], dtype=torch.int32 if k in ("n", "cls") else torch.float32,
                                  device=m._dev.device) for k, s in self.shapes.items()}
        self.views = tuple(self.raw[k][GUARD:GUARD + int(np.prod(s))].view(s) for k, s in self.shapes.items())

    def untouched(self):
        """Nothing at all was written."""
        return all(bool((r == FILL[k]).all()) for k, r in self.raw.items())

    def check(self, want):
        """The guards and the rows at and beyond det_n hold the prefill; det_n and the first det_n rows are the oracle's, bit for bit.
        want: per image (kept anchors, boxes, conf, cls)."""
        host = {k: r.cpu().numpy() for k, r in self.raw.items()}
        for k, a in host.items():
            assert (a[:GUARD] == FILL[k]).all() and (a[-GUARD:] == FILL[k]).all(), "guard words of det_%s were written" % k
        n, box, conf, cls = (host[k][GUARD:-GUARD].reshape(s) for k, s in self.shapes.items())
        for i, (keep, wb, wc, wk) in enumerate(want):
            assert n[i] == len(keep), "image %d: %d detections, the oracle keeps %d" % (i, n[i], len(keep))
            k = len(keep)
            assert np.array_equal(box[i, :k].view(np.uint32), wb.view(np.uint32)), "image %d: boxes" % i
            assert np.array_equal(conf[i, :k].view(np.uint32), wc.view(np.uint32)), "image %d: confidences" % i
            assert np.array_equal(cls[i, :k], wk), "image %d: classes" % i
            assert (box[i, k:] == FILL["box"]).all() and (conf[i, k:] == FILL["conf"]).all() and (cls[i, k:] == FILL["cls"]).all(), \
                "image %d: rows at and beyond det_n were written" % i


def run_lists(env, m, lists):
    """One av_yolo_tail call on `lists` (one per image, same parameters), checked; then the same with the images reversed."""
    torch = env[0]
    p = lists[0]
    assert all((c["conf_thres"], c["iou_thres"], c["max_det"]) == (p["conf_thres"], p["iou_thres"], p["max_det"]) for c in lists)
    want = [K.expected(c) for c in lists]
    for order in (lists, lists[::-1]):
        out = Outputs(torch, m, p["max_det"])
        m.tail(np.stack([c["box"] for c in order]), np.stack([c["conf"] for c in order]), np.stack([c["cls"] for c in order]),
               p["conf_thres"], p["iou_thres"], p["max_det"], out=out.views)
        out.check(want if order is lists else want[::-1])
    return want


@pytest.mark.parametrize("fam", K.FAMILIES)
def test_family_against_the_oracle(env, handle, fam):
    A, m = handle
    for c in K.family(A, fam):
        want = run_lists(env, m, [c, K.partner(A, c), K.empty(A, c)])
        assert len(want[2][0]) == 0
        print("A %d %-22s passes %d, candidates %d, kept %d" % (A, c["name"], K.radix_passes(c), int(K.passing(c).sum()), len(want[0][0])))


def test_a_short_list_after_a_long_one(env, handle):
    """The scratch (sorted boxes, sorted anchors, counts) of a long list does not reach into a short list's result."""
    A, m = handle
    long = K.family(A, "ties")[0]
    short = [c for c in K.family(A, "counts") if c["n"] == 1][0]
    assert long["max_det"] == short["max_det"] and K.passing(long).all()
    run_lists(env, m, [long, long, long])
    run_lists(env, m, [short, K.empty(A, short), K.partner(A, short)])


def test_refusals_leave_the_outputs_alone(env):
    torch, nat, Y, R = env
    A = 420
    m = Y.YoloV8n("random:0", batch=3)
    m._prepare(*K.FRAMES[A])
    d, lib = m._dev, m._dev.lib
    c = K.family(A, "counts")[-1]
    cand = [d.upload(np.stack([c[k]] * 3), dt) for k, dt in (("box", np.float32), ("conf", np.float32), ("cls", np.int32))]

    def call(out, cand=cand, conf_thres=0.25, max_det=300, outs=None):
        rc = lib.av_yolo_tail(m._h, d.stream, *[nat.ptr(t) for t in cand], conf_thres, 0.7, max_det,
                              *([nat.ptr(t) for t in out.views] if outs is None else outs))
        d.sync()
        return rc

    EINVAL, ESTATE = -1, -4
    for kw in (dict(max_det=0), dict(max_det=2501), dict(conf_thres=0.0), dict(conf_thres=-0.5)):
        out = Outputs(torch, m, 300)
        assert call(out, **kw) == EINVAL and out.untouched(), kw
    for null in range(7):
        out = Outputs(torch, m, 300)
        cd, outs = list(cand), [nat.ptr(t) for t in out.views]
        if null < 3:
            cd[null] = None
        else:
            outs[null - 3] = None
        assert call(out, cand=cd, outs=outs) == EINVAL and out.untouched(), null
    out = Outputs(torch, m, 300)
    assert lib.av_yolo_tail(None, d.stream, *[nat.ptr(t) for t in cand], 0.25, 0.7, 300, *[nat.ptr(t) for t in out.views]) == EINVAL and out.untouched()
    # a deferred tail of a forward is pending: the scratch is in use
    m._frames.zero_()
    nat.check(lib.av_yolo_defer_tail(m._h, 1))
    m.forward_device(m._frames)
    out = Outputs(torch, m, 300)
    assert call(out) == ESTATE and out.untouched()
    assert b"pending" in lib.av_last_error_string()
    nat.check(lib.av_yolo_join_tail(m._h, d.stream))
    nat.check(lib.av_yolo_defer_tail(m._h, 0))
    d.sync()
    assert call(out) == 0
    out.check([K.expected(dict(c, max_det=300))] * 3)
    m.close()


def blocks_frame(h, w, seed=2):
    """Flat colour blocks of 64 x 64 pixels: with the spread parameters about a quarter of the anchors pass 0.25."""
    rs = np.random.RandomState(seed)
    return np.kron(rs.randint(0, 256, (h // 64, w // 64, 3)).astype(np.uint8), np.ones((64, 64, 1), np.uint8))


@pytest.mark.parametrize("A", [7560, 7980])
def test_forward_end_to_end_at_the_seven_bit_sort(env, tmp_path, A):
    """The real network at the two frame shapes whose anchor count takes nms_sort_kernel<7>: detect() equals the oracle's tail applied
    to the device's own candidates (the statement of test_tail_on_the_devices_candidates)."""
    torch, nat, Y, R = env
    from tests._util import spread_params
    path = str(tmp_path / "spread.npy")
    np.save(path, spread_params(0))
    h, w = K.FRAMES[A]
    m = Y.YoloV8n(path, batch=1)
    box, conf, cls = m.detect(blocks_frame(h, w))
    assert m.dims() == (h // 2, w // 2, A)
    cb, cc, ck = m.tensor(110)[0], m.tensor(111)[0, :, 0], m.tensor(112)[0, :, 0]
    passed = int((cc > 0.25).sum())
    print("%d anchors: %d pass 0.25, %d kept" % (A, passed, len(box)))
    assert 0.10 * A <= passed <= 0.90 * A, passed
    keep = R.nms(cb, cc, ck)
    want = R.scale_boxes(cb[keep], h, w)
    assert len(keep) == len(box)
    assert np.array_equal(want, box) and np.array_equal(np.trunc(want), np.trunc(box))
    assert np.array_equal(cc[keep], conf) and np.array_equal(ck[keep], cls)
    m.close()
