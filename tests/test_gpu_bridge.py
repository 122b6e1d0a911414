"""The camera -> hot loop bridge on the device: av_dets_to_tracker, av_lane_paths, HotLoop.set_detections / set_lane_inputs and
CameraLoop.

(1) av_dets_to_tracker against tests/bridge_ref.py, every output byte for byte (integer outputs, and a float32 -> float64
    conversion that is exact);
(2) av_lane_paths against the restatement: counts, untouched rows and the NaN pattern exact, lane_offset bit-equal (one
    subtraction, one division and one product of exactly representable operands' results, the same three roundings on both
    sides), positions at the project's waypoint tolerance (rtol 1e-12, atol 1e-11, tests/test_gpu_plan_each.py: sin / cos of the
    device against libm);
(3) argument checks; (4) HotLoop.set_detections on the real reference's detector output (tests/golden/tracker_sim720.npz);
(5) HotLoop.set_lane_inputs; (6) CameraLoop, stage by stage against the restatements fed the device's own detections and fits.
"""
import ctypes as C

import numpy as np
import pytest

from tests import bridge_ref as B
from tests._util import order_mismatch
from tests.obstacles_ref import track_obstacles

gpu = pytest.mark.gpu
CAM_CFG = dict(x_center=640.0, x_scale=0.03 * 640.0 / 1280, y_far=50.0, y_scale=50.0 / 720)       # CameraLoop's defaults at 1280 x 720


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    return torch, nat, nat.lib(), nat.Context(0)


def _dev(env, a, dtype):
    torch = env[0]
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=torch.device("cuda", 0))


# ---- (1) av_dets_to_tracker ---------------------------------------------------------------------------------------------------------

MAX_DET = 300
KEPT = [0, 1, 63, 64, 65, 300]                                   # entries of a mapped class per frame (with the class map)
SRC_N = [-3, 200, 130, 130, 299, 400]                            # clamped to 0 and 300; frame 0's mapped entries are never visited
_BAD = [4, 80, 1000, -1, -5, 6, 79, 2 ** 31 - 1, -2 ** 31]       # in range without a reference class, out of range, negative


def _detector_output():
    rng = np.random.default_rng(42)
    F = len(KEPT)
    box = rng.uniform(-50, 1400, (F, MAX_DET, 4)).astype(np.float32)
    conf = np.sort(rng.uniform(0.25, 1, (F, MAX_DET)).astype(np.float32), axis=1)[:, ::-1].copy()
    cls = np.asarray(_BAD, np.int64)[rng.integers(0, len(_BAD), (F, MAX_DET))].astype(np.int32)
    for f in range(1, F):
        n = min(max(SRC_N[f], 0), MAX_DET)
        where = np.sort(rng.choice(n, KEPT[f], replace=False))     # spread over the 64-entry rounds
        cls[f, where] = np.asarray(B.COCO_OF_REFERENCE)[rng.integers(0, 8, KEPT[f])]
        cls[f, n:] = 2                                             # a mapped class behind the count: must not be visited
    cls[0, :] = 2
    special = np.array([-0.5, -1.7, 1279.99, 3e9, np.nan, -3e9, 0.999, 2147483520.0], np.float32)
    cmap = B.coco_class_map()
    for f in (2, 3, 4):                                            # in the first kept entries (inside dcap 8) and in the first raw ones
        mapped = [i for i in range(MAX_DET) if 0 <= cls[f, i] < 80 and cmap[cls[f, i]] >= 0][:2]
        box[f, 0], box[f, 1] = special[4:], special[:4]
        box[f, mapped[0]], box[f, mapped[1]] = special[:4], special[4:]
    return np.asarray(SRC_N, np.int32), box, conf, cls


@gpu
@pytest.mark.parametrize("dcap", [8, 64])
@pytest.mark.parametrize("mapped", [True, False], ids=["map", "nomap"])
def test_dets_to_tracker_matches_restatement(env, dcap, mapped):
    torch, nat, L, ctx = env
    src_n, box, conf, cls = _detector_output()
    F = len(src_n)
    cmap = B.coco_class_map() if mapped else None
    want = B.dets_to_tracker(src_n, box, conf, cls, cmap, dcap, sentinel=(-9, -9, -9.0))
    if mapped:
        assert list(want[0] + want[4]) == KEPT
    else:
        assert list(want[0] + want[4]) == [0, 200, 130, 130, 299, 300]
    assert want[4].max() > 0 and (want[0] == dcap).any() and (want[0] < dcap).any()
    G = 2                                                          # guard frames behind the outputs
    det_n = torch.full((F + G,), -7, dtype=torch.int32, device="cuda")
    dropped = torch.full((F + G,), -7, dtype=torch.int32, device="cuda")
    det_box = torch.full((F + G, dcap, 4), -9, dtype=torch.int32, device="cuda")
    det_cls = torch.full((F + G, dcap), -9, dtype=torch.int32, device="cuda")
    det_conf = torch.full((F + G, dcap), -9.0, dtype=torch.float64, device="cuda")
    t_n, t_box, t_conf, t_cls = (_dev(env, a, dt) for a, dt in ((src_n, torch.int32), (box, torch.float32), (conf, torch.float32),
                                                                (cls, torch.int32)))
    t_map = None if cmap is None else _dev(env, cmap, torch.int32)
    nat.check(L.av_dets_to_tracker(ctx.handle, None, F, MAX_DET, nat.ptr(t_n), nat.ptr(t_box), nat.ptr(t_conf), nat.ptr(t_cls),
                                   nat.ptr(t_map), 0 if cmap is None else len(cmap), dcap, nat.ptr(det_n), nat.ptr(det_box),
                                   nat.ptr(det_cls), nat.ptr(det_conf), nat.ptr(dropped)))
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (det_n, det_box, det_cls, det_conf, dropped)]
    for name, g, w, fill in zip(("det_n", "det_box", "det_cls", "det_conf", "dropped"), got, want, (-7, -9, -9, -9.0, -7)):
        assert np.array_equal(g[:F].view(np.uint8), w.view(np.uint8)), name
        assert (g[F:] == fill).all(), "%s: written past the last frame" % name
    # without the dropped counts: the same tables
    det_box.fill_(-9), det_cls.fill_(-9), det_conf.fill_(-9.0), det_n.fill_(-7)
    nat.check(L.av_dets_to_tracker(ctx.handle, None, F, MAX_DET, nat.ptr(t_n), nat.ptr(t_box), nat.ptr(t_conf), nat.ptr(t_cls),
                                   nat.ptr(t_map), 0 if cmap is None else len(cmap), dcap, nat.ptr(det_n), nat.ptr(det_box),
                                   nat.ptr(det_cls), nat.ptr(det_conf), None))
    torch.cuda.synchronize()
    for g, t in zip(got[:4], (det_n, det_box, det_cls, det_conf)):
        assert np.array_equal(t.cpu().numpy().view(np.uint8), g.view(np.uint8))


# ---- (2) av_lane_paths ----------------------------------------------------------------------------------------------------------------

def _lane_inputs():
    poly = np.array([[[1.1e-4, -0.93, 905.0], [-2.3e-4, 1.07, 231.0]],
                     [[2.0e-4, -0.80, 800.0], [-1.0e-4, 0.90, 300.0]],
                     [[0.0, -0.50, 700.0], [0.0, 0.50, 500.0]],
                     [[3.0e-4, -1.00, 950.0], [-3.0e-4, 1.00, 250.0]]])
    pts = np.random.default_rng(3).integers(0, 1280, (4, 2, 50, 2)).astype(np.int32)
    pts[0, 0, 49, 0], pts[0, 1, 49, 0] = 401, 900              # an odd sum: a half-pixel centre
    info = np.zeros((4, 8), np.int32)
    info[:, 2:] = 5
    info[0, :2], info[1, :2], info[2, :2] = (1, 7), (1, 0), (0, 1)     # both sides (any non-zero value), left only, right only, neither
    return poly, pts, info


@gpu
@pytest.mark.parametrize("n_points", [2, 50, 64])
def test_lane_paths_matches_restatement(env, n_points):
    torch, nat, L, ctx = env
    S, rcap = 4, n_points + 3
    poly, pts, info = _lane_inputs()
    cfg = nat.ObstacleCfg(CAM_CFG["x_center"], CAM_CFG["x_scale"], CAM_CFG["y_far"], CAM_CFG["y_scale"], (C.c_double * 16)(*([0.0] * 16)))
    t_poly, t_pts, t_info = _dev(env, poly, torch.float64), _dev(env, pts, torch.int32), _dev(env, info, torch.int32)
    for heading in (0.0, 2.3):
        for stride in (1, 3):
            for flip in (False, True):                         # flipped: stream 3 has the lane pair, stream 0 none
                inf = info[::-1].copy() if flip else info
                t_info.copy_(torch.as_tensor(inf))
                rng = np.random.default_rng(int(heading * 10) + stride)
                ps = np.stack([rng.uniform(-200, 200, S * stride), rng.uniform(-200, 200, S * stride),
                               rng.uniform(-3, 3, S * stride), rng.uniform(0, 20, S * stride)], axis=1)
                ps[::stride, 2] = heading
                t_ps = _dev(env, ps, torch.float64)
                out = torch.full((S * rcap * 2 + 8,), float("nan"), dtype=torch.float64, device="cuda")
                n_ref = torch.full((S + 4,), -7, dtype=torch.int32, device="cuda")
                off = torch.full((S + 4,), -7.0, dtype=torch.float64, device="cuda")
                nat.check(L.av_lane_paths(ctx.handle, None, C.byref(cfg), S, 720, 1280, n_points, nat.ptr(t_poly), nat.ptr(t_pts),
                                          nat.ptr(t_info), nat.ptr(t_ps), stride, rcap, nat.ptr(out), nat.ptr(n_ref), nat.ptr(off)))
                torch.cuda.synchronize()
                want, want_n, want_off = B.lane_paths(poly, pts, inf, ps, stride, 720, 1280, n_points, CAM_CFG)
                where = "heading %g stride %d flip %d" % (heading, stride, flip)
                got, got_n, got_off = out.cpu().numpy(), n_ref.cpu().numpy(), off.cpu().numpy()
                assert np.array_equal(got_n[:S], want_n) and (got_n[S:] == -7).all(), where
                assert np.array_equal(got_off[:S].view(np.int64), want_off.view(np.int64)) and (got_off[S:] == -7.0).all(), where
                assert np.isnan(got[S * rcap * 2:]).all(), where
                got = got[:S * rcap * 2].reshape(S, rcap, 2)
                valid = 3 if flip else 0
                assert list(want_n) == [n_points if s == valid else 0 for s in range(S)]
                for s in range(S):
                    m = int(want_n[s])
                    assert np.isnan(got[s, m:]).all(), "%s stream %d: a row past the count was written" % (where, s)
                    np.testing.assert_allclose(got[s, :m], want[s], rtol=1e-12, atol=1e-11, err_msg=where)
                # without the offsets: the same paths
                out2 = torch.full_like(out, float("nan"))
                nat.check(L.av_lane_paths(ctx.handle, None, C.byref(cfg), S, 720, 1280, n_points, nat.ptr(t_poly), nat.ptr(t_pts),
                                          nat.ptr(t_info), nat.ptr(t_ps), stride, rcap, nat.ptr(out2), nat.ptr(n_ref), None))
                torch.cuda.synchronize()
                assert np.array_equal(out2.cpu().numpy().view(np.int64), out.cpu().numpy().view(np.int64)), where


# ---- (3) argument checks --------------------------------------------------------------------------------------------------------------

@gpu
def test_argument_checks(env):
    torch, nat, L, ctx = env
    P = nat.ptr
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    n, box, conf, cls = i32(2), torch.zeros(2, 4, 4, device="cuda"), torch.zeros(2, 4, device="cuda"), i32(2, 4)
    dn, db, dc, df = i32(2), i32(2, 64, 4), i32(2, 64), torch.zeros(2, 64, dtype=torch.float64, device="cuda")
    call = lambda F, md, dcap, a=n, b=db: L.av_dets_to_tracker(ctx.handle, None, F, md, P(a), P(box), P(conf), P(cls), None, 0, dcap,
                                                                 P(dn), P(b), P(dc), P(df), None)
    assert call(2, 4, 8) == 0 and call(2, 4, 1) == 0 and call(2, 4, 64) == 0
    assert call(2, 4, 0) == -1 and call(2, 4, 65) == -1 and call(2, 0, 8) == -1 and call(0, 4, 8) == -1
    assert call(2, 4, 8, a=None) == -1 and call(2, 4, 8, b=None) == -1
    assert L.av_dets_to_tracker(None, None, 2, 4, P(n), P(box), P(conf), P(cls), None, 0, 8, P(dn), P(db), P(dc), P(df), None) == -1
    cfg = nat.ObstacleCfg(320.0, 0.03, 50.0, 0.1, (C.c_double * 16)(*([0.0] * 16)))
    poly, pts, info = torch.zeros(2, 2, 3, dtype=torch.float64, device="cuda"), i32(2, 2, 50, 2), i32(2, 8)
    ps, ref, nr = (torch.zeros(2, 4, dtype=torch.float64, device="cuda"), torch.zeros(2, 64, 2, dtype=torch.float64, device="cuda"), i32(2))
    lane = lambda npt, rcap, c=C.byref(cfg), p=poly, r=ref: L.av_lane_paths(ctx.handle, None, c, 2, 720, 1280, npt, P(p), P(pts), P(info),
                                                                            P(ps), 1, rcap, P(r), P(nr), None)
    assert lane(2, 2) == 0 and lane(64, 64) == 0 and lane(50, 64) == 0
    assert lane(1, 64) == -1 and lane(65, 65) == -1 and lane(50, 49) == -1
    assert lane(50, 64, c=None) == -1 and lane(50, 64, p=None) == -1 and lane(50, 64, r=None) == -1
    assert L.av_lane_paths(ctx.handle, None, C.byref(cfg), 2, 720, 1280, 50, P(poly), P(pts), P(info), P(ps), 0, 64, P(ref), P(nr),
                           None) == -1
    torch.cuda.synchronize()


# ---- (4) HotLoop.set_detections -------------------------------------------------------------------------------------------------------

FRAMES = 60


@gpu
@pytest.mark.parametrize("W", [1, 4])
def test_loop_tracks_the_golden_detections(env, golden, W):
    torch, nat, L, ctx = env
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.detector_ref import detection_table
    from oracle.harness_ref import ego_motion
    g = golden("tracker_sim720")
    src = B.floatified_golden(g, frames=FRAMES)
    md = src[1].shape[1]
    loop = HotLoop(1, window=W, dcap=8, fused_step=False, obstacles="tracks")
    t_n = torch.zeros(1, W, dtype=torch.int32, device="cuda")
    t_box = torch.zeros(1, W, md, 4, dtype=torch.float32, device="cuda")
    t_conf = torch.zeros(1, W, md, dtype=torch.float32, device="cuda")
    t_cls = torch.zeros(1, W, md, dtype=torch.int32, device="cuda")
    loop.set_detections(t_n, t_box, t_conf, t_cls, class_map=B.coco_class_map())
    z = ego_motion(FRAMES, seed=0)[None]
    total = 0
    for k in range(FRAMES // W):
        sl = slice(k * W, (k + 1) * W)
        for t, a in zip((t_n, t_box, t_conf, t_cls), src):
            t.copy_(torch.as_tensor(a[sl])[None])
        torch.cuda.synchronize()
        loop.load_measurements(z[:, sl])
        loop.step(sync=True)
        r = loop.results()
        rows, n = loop.snapshots()
        ps = loop.plan_state.cpu().numpy()
        assert not r["det_dropped"].any() and r["det_dropped"].shape == (1, W)
        for f in range(W):
            fr = k * W + f
            nd = int(g["in_n"][fr])
            assert r["det_n"][0, f] == nd and np.array_equal(r["det_box"][0, f, :nd], g["in_box"][fr][:nd]), fr
            assert np.array_equal(r["det_cls"][0, f, :nd], g["in_cls"][fr][:nd]), fr
            assert np.array_equal(r["det_conf"][0, f, :nd], g["in_conf"][fr][:nd].astype(np.float32).astype(np.float64)), fr
            m, row = int(n[0, f]), rows[0, f]
            assert m == g["n_live"][fr], fr
            assert np.array_equal(row["id"][:m], g["ids"][fr][:m]) and np.array_equal(row["cls"][:m], g["cls"][fr][:m]), fr
            assert np.array_equal(np.stack([row["x1"], row["y1"], row["x2"], row["y2"]], axis=1)[:m], g["box"][fr][:m]), fr
            assert np.array_equal(np.stack([row["age"], row["hits"], row["misses"]], axis=1)[:m], g["ahm"][fr][:m]), fr
            assert np.array_equal(row["conf"][:m], g["conf"][fr][:m].astype(np.float32).astype(np.float64)), fr
            assert np.array_equal(r["det2trk"][0, f, :nd], g["det2trk"][fr][:nd]), fr
            assert np.array_equal(row["id"][:m][row["flags"][:m] & 1 == 1], g["conf_ids"][fr][:g["n_conf"][fr]]), fr
            want = track_obstacles(row, m, ps[0, f])
            assert r["n_obs"][0, f] == len(want), fr
            assert np.array_equal(r["obstacles"][0, f, :len(want), 2], want[:, 2]), fr
            np.testing.assert_allclose(r["obstacles"][0, f, :len(want), :2], want[:, :2], rtol=1e-12, atol=1e-11, err_msg=str(fr))
            total += len(want)
    assert total > 0 and loop.frame_count.cpu().tolist() == [FRAMES]
    # back to the simulated detector: the frames a loop that never left it would see next
    loop.set_detections(None)
    loop.load_measurements(z[:, :W])
    loop.step(sync=True)
    r = loop.results()
    dn, dbox, dcls, dconf = detection_table(FRAMES + 1, W, 720, 1280)
    assert "det_dropped" not in r and loop.frame_count.cpu().tolist() == [FRAMES + W]
    assert np.array_equal(r["det_n"][0], dn) and np.array_equal(r["det_box"][0], dbox) and np.array_equal(r["det_cls"][0], dcls)
    assert np.array_equal(r["det_conf"][0], dconf)


@gpu
def test_set_detections_refusals(env):
    torch = env[0]
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    mk = lambda S: (torch.zeros(S, 1, dtype=torch.int32, device="cuda"), torch.zeros(S, 1, 16, 4, device="cuda"),
                    torch.zeros(S, 1, 16, device="cuda"), torch.zeros(S, 1, 16, dtype=torch.int32, device="cuda"))
    fused = HotLoop()
    assert fused.fused_step is True
    with pytest.raises(RuntimeError):
        fused.set_detections(*mk(1))
    with pytest.raises(RuntimeError):
        HotLoop(n_streams=2, overlap=2).set_detections(*mk(2))
    plain = HotLoop(n_streams=2, window=1, fused_step=False)
    n, box, conf, cls = mk(2)
    for bad in ((n.long(), box, conf, cls), (n, box.double(), conf, cls), (n, box[:, :, :, :3], conf, cls), (n, box, conf[:1], cls),
                (n, box, conf, cls.float()), (n.cpu(), box, conf, cls), (n, box, conf, cls[:, :, ::2]), (n, box, None, cls)):
        with pytest.raises(ValueError):
            plain.set_detections(*bad)
    plain.set_detections(n, box, conf, cls)
    plain.step(sync=True)
    assert plain.results()["det_n"].tolist() == [[0], [0]] and plain.frame_count.cpu().tolist() == [1, 1]


# ---- (5) HotLoop.set_lane_inputs --------------------------------------------------------------------------------------------------------

@gpu
def test_loop_follows_its_lane_paths(env):
    torch, nat, L, ctx = env
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.harness_ref import ego_motion
    S, W = 3, 2
    poly, pts, info = (a[:S].copy() for a in _lane_inputs())
    info[:, :2] = [(1, 1), (0, 1), (1, 1)]
    loop = HotLoop(S, window=W, fused_step=False, obstacle_kw=CAM_CFG)
    t_poly, t_pts, t_info = _dev(env, poly, torch.float64), _dev(env, pts, torch.int32), _dev(env, info, torch.int32)
    loop.set_lane_inputs(t_poly, t_pts, t_info)
    assert loop._per_state() and tuple(loop.ref_paths.shape) == (S, 50, 2)
    with pytest.raises(RuntimeError):
        loop.set_reference_paths(torch.zeros(S, 4, 2, dtype=torch.float64, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda"))
    z = np.stack([ego_motion(2 * W, seed=s) for s in range(S)])
    for k in range(2):
        loop.load_measurements(z[:, k * W:(k + 1) * W])
        loop.step(sync=True)
    r = loop.results()
    ps = loop.plan_state.cpu().numpy()
    want, want_n, want_off = B.lane_paths(poly, pts, info, ps.reshape(S * W, 4), W, 720, 1280, 50, CAM_CFG)
    assert np.array_equal(r["n_ref"], want_n) and list(want_n) == [50, 0, 50]
    assert np.array_equal(r["lane_offset"].view(np.int64), want_off.view(np.int64))
    for s in (0, 2):
        np.testing.assert_allclose(r["ref_paths"][s], want[s], rtol=1e-12, atol=1e-11)
    # the plans: av_planner_plan_each on the step's own start states with the device's own paths, bit for bit
    n_cand, n_pts = loop.n_cand, loop.n_points
    cost = torch.full((S * W, n_cand), float("nan"), dtype=torch.float64, device="cuda")
    order = torch.full((S * W, n_cand), -1, dtype=torch.int32, device="cuda")
    w = torch.full((S * W, n_cand, n_pts, 6), float("nan"), dtype=torch.float64, device="cuda")
    nat.check(L.av_planner_plan_each(loop.ctx.handle, None, S * W, nat.ptr(loop.plan_state), nat.ptr(loop.ref_paths), nat.ptr(loop.n_ref),
                                     50, W, None, None, 0, nat.ptr(w), nat.ptr(cost), nat.ptr(order)))
    torch.cuda.synchronize()
    assert np.array_equal(cost.cpu().numpy().view(np.int64), r["cost"].reshape(S * W, n_cand).view(np.int64))
    assert np.array_equal(order.cpu().numpy(), r["order"].reshape(S * W, n_cand))
    assert np.array_equal(w.cpu().numpy().view(np.int64), r["wp"].reshape(S * W, n_cand, n_pts, 6).view(np.int64))
    # no path at all: the stream without a lane pair plans as before, the others do not
    nat.check(L.av_planner_plan(loop.ctx.handle, None, S * W, nat.ptr(loop.plan_state), None, 0, None, 0, None, nat.ptr(cost), nat.ptr(order)))
    torch.cuda.synchronize()
    free = cost.cpu().numpy().reshape(S, W, n_cand)
    assert np.array_equal(free[1].view(np.int64), r["cost"][1].view(np.int64))
    assert np.array_equal(order.cpu().numpy().reshape(S, W, n_cand)[1], r["order"][1])
    assert (free[0] != r["cost"][0]).any() and (free[2] != r["cost"][2]).any()
    # window 1: the offsets are what the maneuver stage takes
    one = HotLoop(S, window=1, fused_step=False, obstacle_kw=CAM_CFG)
    one.set_lane_inputs(t_poly, t_pts, t_info, n_points=7)
    one.load_measurements(z[:, :1])
    one.step()
    one.enqueue_maneuver(lane_offset=one.lane_offset)
    one.synchronize()
    assert tuple(one.ref_paths.shape) == (S, 7, 2) and one.n_ref.cpu().tolist() == [7, 0, 7]
    # refusals
    with pytest.raises(RuntimeError):
        HotLoop().set_lane_inputs(t_poly[:1], t_pts[:1], t_info[:1])
    given = HotLoop(S, window=W, fused_step=False)
    given.set_reference_paths(torch.zeros(S, 4, 2, dtype=torch.float64, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        given.set_lane_inputs(t_poly, t_pts, t_info)
    for bad in ((t_poly.float(), t_pts, t_info), (t_poly, t_pts[:, :, :49], t_info), (t_poly, t_pts, t_info[:2]), (t_poly, t_pts, None)):
        with pytest.raises(ValueError):
            loop.set_lane_inputs(*bad)
    with pytest.raises(ValueError):
        loop.set_lane_inputs(t_poly, t_pts, t_info, n_points=65)
    loop.set_lane_inputs(None)
    assert loop.ref_paths is None and not loop._per_state() and "ref_paths" not in loop.results()


# ---- (6) CameraLoop --------------------------------------------------------------------------------------------------------------------

# The weights' seed decides how many detections carry one of the eight reference classes (2 cameras, 4 steps, counted on the
# detector's own output): seeds 0 .. 8, 10, 11, 13 and 15 .. 17 give at most one per frame, so no cap drops anything; seed 9 gives
# 31 .. 34 of 77 .. 80, seed 12 gives 10 .. 12 of 17 .. 19, seed 14 gives 300 of 300.  Seed 14 with dcap 8 keeps 8 and drops 292.
CAM_SEED, CAM_STEPS, CAM_DCAP = 14, 4, 8


def _run_camera(path, z):
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import CameraLoop
    loop = CameraLoop(2, h=720, w=1280, model=path, dcap=CAM_DCAP, tracker_kw=dict(min_hits=1))
    steps = []
    for k in range(CAM_STEPS):
        loop.load_measurements(z[:, k:k + 1])
        loop.step(sync=True)
        c = loop.cam
        cam = dict(det_n=c.det_n.cpu().numpy(), det_box=c.det_box.cpu().numpy(), det_conf=c.det_conf.cpu().numpy(),
                   det_cls=c.det_cls.cpu().numpy(), poly=c.poly.cpu().numpy(), pts=c.pts.cpu().numpy(), info=c.info.cpu().numpy())
        rows, n = loop.hot.snapshots()
        steps.append((loop.results(), cam, rows.copy(), n.copy(), loop.hot.plan_state.cpu().numpy()))
    return loop, steps


@gpu
def test_camera_loop_stage_by_stage(env, tmp_path):
    from oracle.harness_ref import ego_motion
    from oracle.tracker_ref import TrackerRef
    from tests._util import spread_params
    from tests.moving_ref import MovingPlannerRef, track_obstacles_moving
    path = str(tmp_path / "spread.npy")
    np.save(path, spread_params(CAM_SEED))
    z = np.stack([ego_motion(CAM_STEPS, seed=s) for s in range(2)])
    loop, steps = _run_camera(path, z)
    assert np.array_equal(loop.class_map, B.coco_class_map()) and loop.hot.frame_rate == 30.0
    assert (loop.hot.ocfg.x_center, loop.hot.ocfg.x_scale, loop.hot.ocfg.y_far, loop.hot.ocfg.y_scale) == (
        CAM_CFG["x_center"], CAM_CFG["x_scale"], CAM_CFG["y_far"], CAM_CFG["y_scale"])
    trackers = [TrackerRef(min_hits=1) for _ in range(2)]
    seen = dict(det=0, dropped=0, ref=0, obs=0)
    for k, (r, cam, rows, n, ps) in enumerate(steps):
        want = B.dets_to_tracker(cam["det_n"], cam["det_box"], cam["det_conf"], cam["det_cls"], B.coco_class_map(), CAM_DCAP)
        paths, want_nref, want_off = B.lane_paths(cam["poly"], cam["pts"], cam["info"], ps.reshape(2, 4), 1, 720, 1280, 50, CAM_CFG)
        assert np.array_equal(r["det_n"][:, 0], want[0]) and np.array_equal(r["det_dropped"][:, 0], want[4]), k
        assert np.array_equal(r["n_ref"], want_nref) and np.array_equal(r["lane_offset"].view(np.int64), want_off.view(np.int64)), k
        for s in range(2):
            where = "step %d stream %d" % (k, s)
            nd = int(want[0][s])
            assert np.array_equal(r["det_box"][s, 0, :nd], want[1][s, :nd]) and np.array_equal(r["det_cls"][s, 0, :nd], want[2][s, :nd]), where
            assert np.array_equal(r["det_conf"][s, 0, :nd], want[3][s, :nd]), where
            tr = trackers[s].update(nd, want[1][s], want[2][s], want[3][s])
            t = trackers[s].table(64)
            m, row = int(n[s, 0]), rows[s, 0]
            assert m == t["n"], where
            assert np.array_equal(row["id"][:m], t["ids"][:m]) and np.array_equal(row["cls"][:m], t["cls"][:m]), where
            assert np.array_equal(np.stack([row["x1"], row["y1"], row["x2"], row["y2"]], axis=1)[:m], t["box"][:m]), where
            assert np.array_equal(np.stack([row["age"], row["hits"], row["misses"]], axis=1)[:m], t["ahm"][:m]), where
            assert np.array_equal(row["conf"][:m], t["conf"][:m]) and np.array_equal(r["det2trk"][s, 0, :nd], tr["det2trk"]), where
            obs = track_obstacles_moving(row, m, ps[s, 0], CAM_CFG, 30.0)
            assert r["n_obs"][s, 0] == len(obs), where
            got_obs = r["obstacles"][s, 0, :len(obs)]
            assert np.array_equal(got_obs[:, 2], obs[:, 2]), where
            np.testing.assert_allclose(got_obs[:, [0, 1, 3, 4]], obs[:, [0, 1, 3, 4]], rtol=1e-12, atol=1e-11, err_msg=where)
            np.testing.assert_allclose(r["ref_paths"][s, :want_nref[s]], paths[s], rtol=1e-12, atol=1e-11, err_msg=where)
            seen["det"] += nd
            seen["dropped"] += int(want[4][s] > 0)
            seen["ref"] += int(want_nref[s] > 0)
            seen["obs"] += len(obs)
        # the plan of stream 0 against the oracle, fed the device's own obstacles and path
        p = MovingPlannerRef()
        p.set_reference_path(r["ref_paths"][0, :r["n_ref"][0]])
        plan = p.plan(ps[0, 0], r["obstacles"][0, 0, :r["n_obs"][0, 0]])
        cost, order, wp = r["cost"][0, 0], r["order"][0, 0], r["wp"][0, 0]
        best = int(order[0])
        print("step %d: %d detections kept, %d dropped, n_ref %r, %d obstacles; best candidate %d (oracle %d), cost off by %.3g, "
              "waypoints by %.3g" % (k, int(want[0].sum()), int(want[4].sum()), want_nref.tolist(), int(r["n_obs"].sum()), best,
                                      int(plan["order"][0]), abs(cost[best] - plan["cost"][best]), np.abs(wp[best] - plan["wp"][best]).max()))
        assert np.array_equal(order, np.argsort(cost, kind="stable")), k
        why = order_mismatch(plan["cost"], plan["order"], cost, order)
        assert why is None, "step %d: %s" % (k, why)
        np.testing.assert_allclose(cost[best], plan["cost"][best], rtol=1e-12, atol=1e-12, err_msg="step %d" % k)
        np.testing.assert_allclose(wp[best], plan["wp"][best], rtol=1e-12, atol=1e-11, err_msg="step %d" % k)
    print("camera loop: %r" % seen)
    assert seen["det"] > 0 and seen["dropped"] > 0 and seen["ref"] > 0
    # a second loop stepped the same way: byte-identical results
    _, again = _run_camera(path, z)
    for (r, _, _, _, _), (r2, _, _, _, _) in zip(steps, again):
        assert set(r) == set(r2)
        for key in r:
            assert np.array_equal(r[key].view(np.uint8), r2[key].view(np.uint8)), key
    # the deferred modes leave det_* / poly one frame behind: refused
    loop.cam.defer_detector_tail(True)
    with pytest.raises(RuntimeError):
        loop.step()
    loop.cam.defer_detector_tail(False)
