"""CPU-only checks of the camera -> hot loop bridge: the ABI of av_dets_to_tracker / av_lane_paths, and their NumPy restatements
(tests/bridge_ref.py) on the real reference's detector output (tests/golden/tracker_sim720.npz) and on hand-made lane fits."""
import os

import numpy as np
import pytest

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
from oracle.tracker_ref import TrackerRef
from tests import bridge_ref as B


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nat.lib()


def test_exports_and_bindings(lib):
    for name in ("av_dets_to_tracker", "av_lane_paths"):
        assert name in nat.declared_symbols() and hasattr(lib, name)
        assert name in {s[0] for s in nat._SIGS}
    assert lib.av_version() == 103


def test_argument_validation_without_gpu(lib):
    assert lib.av_dets_to_tracker(None, None, 1, 300, None, None, None, None, None, 0, 8, None, None, None, None, None) == -1
    assert lib.av_lane_paths(None, None, None, 1, 720, 1280, 50, None, None, None, None, 1, 50, None, None, None) == -1


def test_reference_class_map_by_name():
    from multimodal_autonomous_driving_perception_and_planning_amd.perception.yolo import COCO_NAMES
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import _REFERENCE_IDS, reference_class_map
    m = reference_class_map(dict(enumerate(COCO_NAMES)))
    assert m.dtype == np.int32 and np.array_equal(m, B.coco_class_map())
    assert [int(np.nonzero(m == k)[0][0]) for k in range(8)] == B.COCO_OF_REFERENCE and (m >= 0).sum() == 8
    assert list(reference_class_map(["Pedestrian", "cyclist", "traffic light", "stop_sign", "tram"])) == [2, 3, 6, 7, -1]
    assert B.REFERENCE_IDS == _REFERENCE_IDS


def test_truncation_saturation_and_nan():
    vals = [-0.5, -1.7, 1279.99, 3e9, -3e9, float("nan"), 0.75, 2147483520.0, -2147483648.0]
    assert [B.trunc_sat(v) for v in vals] == [0, -1, 1279, 2147483647, -2147483648, 0, 0, 2147483520, -2147483648]


def test_restatement_returns_the_golden_tracker_input(golden):
    """The reference's detector output, made float32 detector output with fractions, COCO ids and unmapped classes in between,
    comes back through the restatement as exactly the tracker input it was; TrackerRef on it reproduces the golden tables."""
    g = golden("tracker_sim720")
    src_n, src_box, src_conf, src_cls = B.floatified_golden(g)
    assert (src_box != np.trunc(src_box)).any() and set(np.unique(src_cls)) >= set(B.UNMAPPED) | set(B.COCO_OF_REFERENCE)
    det_n, det_box, det_cls, det_conf, dropped = B.dets_to_tracker(src_n, src_box, src_conf, src_cls, B.coco_class_map(), 8,
                                                                   sentinel=(0, 0, 0.0))
    assert np.array_equal(det_n, g["in_n"]) and np.array_equal(det_box, g["in_box"]) and np.array_equal(det_cls, g["in_cls"])
    assert np.array_equal(det_conf, g["in_conf"].astype(np.float32).astype(np.float64))
    assert not dropped.any()
    trk = TrackerRef()
    for f in range(len(det_n)):
        r = trk.update(det_n[f], det_box[f], det_cls[f], det_conf[f])
        t = trk.table(64)
        assert t["n"] == g["n_live"][f], f
        assert np.array_equal(t["ids"], g["ids"][f]) and np.array_equal(t["box"], g["box"][f]), f
        assert np.array_equal(t["cls"], g["cls"][f]) and np.array_equal(t["ahm"], g["ahm"][f]), f
        assert np.array_equal(r["det2trk"], g["det2trk"][f][:det_n[f]]), f
    assert len(det_n) == 300 and trk.next_id > 100


def test_restatement_cap_map_and_clamp():
    rng = np.random.default_rng(1)
    F, md = 4, 12
    box = rng.uniform(0, 100, (F, md, 4)).astype(np.float32)
    conf = np.sort(rng.uniform(0.3, 1, (F, md)).astype(np.float32), axis=1)[:, ::-1]
    cls = np.tile(np.array([2, 4, 0, 80, -1, 7, 2, 2, 5, 9, 11, 3], np.int32), (F, 1))     # mapped: 2 0 7 2 2 5 9 11 3 -> 9 kept
    n = np.array([12, -3, 400, 5], np.int32)
    det_n, det_box, det_cls, det_conf, dropped = B.dets_to_tracker(n, box, conf, cls, B.coco_class_map(), 4)
    assert list(det_n) == [4, 0, 4, 2] and list(dropped) == [5, 0, 5, 0]
    assert list(det_cls[0]) == [0, 2, 1, 0] and list(det_cls[3]) == [0, 2, -9, -9] and (det_cls[1] == -9).all()
    assert np.array_equal(det_box[0, 1], np.trunc(box[0, 2]).astype(np.int32)) and det_conf[0, 3] == np.float64(conf[0, 6])
    # no map: raw ids, negative and out-of-range ones included, in order
    det_n, _, det_cls, _, dropped = B.dets_to_tracker(n, box, conf, cls, None, 4)
    assert list(det_n) == [4, 0, 4, 4] and list(dropped) == [8, 0, 8, 1] and list(det_cls[0]) == [2, 4, 0, 80]


def _lanes():
    poly = np.array([[[1e-4, -0.9, 900.0], [-2e-4, 1.1, 200.0]]] * 4)
    pts = np.zeros((4, 2, 50, 2), np.int32)
    pts[:, 0, 49, 0], pts[:, 1, 49, 0] = 401, 900
    info = np.zeros((4, 8), np.int32)
    info[0, :2], info[1, :2], info[2, :2] = (1, 1), (1, 0), (0, 1)
    return poly, pts, info


def test_lane_restatement_validity_and_end_points():
    poly, pts, info = _lanes()
    ps = np.array([[3.0, -2.0, 0.0, 10.0]] * 4)
    paths, n_ref, off = B.lane_paths(poly, pts, info, ps, 1, 720, 1280, 2)
    assert list(n_ref) == [2, 0, 0, 0] and [len(p) for p in paths] == [2, 0, 0, 0]
    assert np.isnan(off[1:]).all() and off[0] == (640.0 - 1301 / 2.0) * 0.03
    assert list(B.lane_rows(720, 2)) == [720.0, 0.6 * 720] and B.lane_rows(720, 50)[0] == 720.0
    assert abs(B.lane_rows(720, 50)[-1] - 432.0) < 1e-10 and (np.diff(B.lane_rows(720, 50)) < 0).all()
    # heading 0: x = forward = 50 - y * 0.1, y = lateral = (xc - 320) * 0.03, both shifted by the start position
    for k, y in enumerate((720.0, 432.0)):
        xl = 1e-4 * y * y - 0.9 * y + 900.0
        xr = -2e-4 * y * y + 1.1 * y + 200.0
        np.testing.assert_allclose(paths[0][k], [3.0 + (50.0 - y * 0.1), -2.0 + ((xl + xr) / 2 - 320.0) * 0.03], rtol=0, atol=1e-12)
    # the stream's start state is the first of its window; heading pi/2 turns forward into +y and lateral into -x
    ps3 = np.zeros((12, 4))
    ps3[0] = [0.0, 0.0, np.pi / 2, 5.0]
    ps3[1:3] = 77.0
    info[:, :2] = 1
    p3, n3, _ = B.lane_paths(poly, pts, info, ps3, 3, 720, 1280, 50, dict(x_center=640.0, x_scale=0.015, y_far=50.0, y_scale=50 / 720))
    assert list(n3) == [50] * 4 and p3[0].shape == (50, 2)
    y = 720.0
    xc = ((1e-4 * y * y - 0.9 * y + 900.0) + (-2e-4 * y * y + 1.1 * y + 200.0)) / 2
    np.testing.assert_allclose(p3[0][0], [-(xc - 640.0) * 0.015, 50.0 - y * (50 / 720)], rtol=0, atol=1e-12)
    assert np.array_equal(p3[1], p3[2])                       # states 3 and 6: both zero
