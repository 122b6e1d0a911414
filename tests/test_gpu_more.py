"""Fallback paths, edge cases and full-size properties (GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return torch


def test_kf_dense_fallback_for_non_separable_covariance(torch_gpu):
    """A user-assigned P with cross-axis terms must take the dense 6x6 kernel and still match the oracle."""
    from src.state_estimation import VehicleStateEstimator
    from oracle.harness_ref import ego_motion
    from oracle.kf_ref import KalmanRef
    rng = np.random.RandomState(11)
    A = rng.standard_normal((6, 6))
    P0 = A @ A.T + 6 * np.eye(6)
    est, ref = VehicleStateEstimator(), KalmanRef()
    est.kf.P = P0
    ref.P = P0.copy()
    z = ego_motion(40, seed=4)
    for f in range(40):
        got, want = est.step(z[f]), ref.step(z[f])
        np.testing.assert_allclose([got.x, got.y, got.vx, got.vy, got.heading, got.speed, got.acceleration, got.yaw_rate,
                                    got.pos_uncertainty, got.vel_uncertainty], want[[0, 1, 2, 3, 4, 5, 6, 7, 9, 10]],
                                   rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(est.kf.P, ref.P, rtol=1e-8, atol=1e-10)
    assert float(est._state[0, 45].item()) == 1.0            # flagged for the dense kernel
    est.reset()
    assert float(est._state[0, 45].item()) == 0.0


def test_generic_hough_kernel_matches_fast_path(torch_gpu):
    """stages bit 3 forces the generic (global-memory) PPHT kernel; both must give the oracle's segments."""
    from src.perception import LaneDetector
    from oracle.lane_ref import LaneRef, synthetic_frame
    frame = synthetic_frame(480, 640, 2, 5)
    want = LaneRef().stages(frame)["segments"]
    for stages in (0, 8):
        det = LaneDetector()
        det._run(frame, stages=stages)
        n = int(det._view(6, np.int32, (1,))[0])
        assert np.array_equal(det._view(5, np.int32, (det.MAX_SEGMENTS, 4))[:n], want), stages
    # repeated frames reuse the accumulator: it must come back clean every time
    det = LaneDetector()
    for _ in range(3):
        det._run(frame)
        n = int(det._view(6, np.int32, (1,))[0])
        assert np.array_equal(det._view(5, np.int32, (det.MAX_SEGMENTS, 4))[:n], want)


def test_custom_roi_polygon(torch_gpu):
    from src.perception import LaneDetector
    from oracle.lane_ref import LaneRef, synthetic_frame
    frame = synthetic_frame(480, 640, 0, 3)
    h, w = 480, 640
    verts = np.array([[(int(w * 0.1), h), (int(w * 0.4), int(h * 0.6)), (int(w * 0.6), int(h * 0.6)), (int(w * 0.9), h)]])
    a, b = LaneDetector(), LaneDetector(roi_vertices=verts)
    a._run(frame, stages=3)
    b._run(frame, stages=3)
    ma, mb = a._view(3, np.uint8, (h, w)), b._view(3, np.uint8, (h, w))
    assert (ma != mb).mean() < 0.002               # same trapezoid up to boundary rounding
    assert mb[: int(h * 0.6)].sum() == 0
    # the exact statement: the caller's ROI is one inclusive column range per row, and the masked map is the oracle's edge map
    # inside exactly those ranges (tests/test_gpu_canny_cases.py states the same for hand-made ranges)
    from multimodal_autonomous_driving_perception_and_planning_amd.perception.lane_detector import _roi_rows
    from tests.canny_cases import mask_rows
    rows = _roi_rows(verts, h, w)
    assert (rows[: int(h * 0.6), 0] > rows[: int(h * 0.6), 1]).all() and (rows[int(h * 0.6):, 0] <= rows[int(h * 0.6):, 1]).all()
    edges = LaneRef().stages(frame)["edges"]
    assert np.array_equal(b._view(2, np.uint8, (h, w)), edges)
    assert np.array_equal(mb, mask_rows(edges, rows))
    n = int(b._view(10, np.int32, (1,))[0])
    ys, xs = np.nonzero(mask_rows(edges, rows))
    assert n == len(ys) > 0
    assert np.array_equal(b._view(9, np.uint32, (h * w,))[:n], xs.astype(np.uint32) | (ys.astype(np.uint32) << 16))


def test_tracker_wide_detection_lists_and_multiwave(torch_gpu):
    """dcap > 8 takes the 16-wide / generic association paths, tcap 256 the multi-wave kernel."""
    import torch
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.tracker_ref import TrackerRef
    rng = np.random.RandomState(2)
    W = 40
    for dcap, tcap, nmax in ((16, 64, 14), (32, 256, 30)):
        loop = HotLoop(n_streams=1, window=W, tcap=tcap, dcap=dcap, keep_waypoints=False,
                       tracker_kw=dict(min_hits=2, max_age=3))
        ref = TrackerRef(min_hits=2, max_age=3)
        n = rng.randint(0, nmax + 1, size=W).astype(np.int32)
        cx = rng.randint(50, 1200, size=(W, dcap))
        cy = rng.randint(50, 650, size=(W, dcap))
        box = np.stack([cx - 30, cy - 20, cx + 30, cy + 20], axis=2).astype(np.int32)
        box[1:] = np.where(rng.rand(W - 1, dcap, 1) < 0.6, box[:-1] + rng.randint(-4, 5, size=(W - 1, dcap, 1)), box[1:])
        cls = rng.randint(0, 8, size=(W, dcap)).astype(np.int32)
        conf = rng.uniform(0.3, 1, size=(W, dcap))
        loop.det_n.copy_(torch.as_tensor(n).view(1, W))
        loop.det_box.copy_(torch.as_tensor(box).view(1, W, dcap, 4))
        loop.det_cls.copy_(torch.as_tensor(cls).view(1, W, dcap))
        loop.det_conf.copy_(torch.as_tensor(conf).view(1, W, dcap))
        torch.cuda.synchronize()
        loop.enqueue_track()
        rows, cnt = loop.snapshots()
        d2t = loop.det2trk.cpu().numpy()
        for f in range(W):
            r = ref.update(n[f], box[f], cls[f], conf[f])
            t = ref.table(tcap)
            assert cnt[0, f] == t["n"], (dcap, f)
            assert np.array_equal(rows[0, f]["id"][:t["n"]], t["ids"][:t["n"]]), (dcap, f)
            assert np.array_equal(d2t[0, f, :n[f]], r["det2trk"]), (dcap, f)


@pytest.mark.parametrize("thr,rep", [(0.3, None), (0.5, None), (0.3, "1"), (0.5, "1"), (0.0, None)])
def test_tracker_association_paths_dense_scenes(torch_gpu, thr, rep, monkeypatch):
    """dcap 8 / tcap 64 takes the divide-free front end: isolated edges, contested columns resolved by a
    per-column arg-max, rows with two candidates (generic greedy loop), exact duplicates (row-major ties) and
    quotients exactly on the threshold (guard band -> exact divide).  thr 0 keeps the all-pairs path.
    rep None: 8 replica waves per stream (one per detection column); rep "1": the single-wave kernel."""
    import torch
    if rep is not None:
        monkeypatch.setenv("AVHOT_TRACKER_REP", rep)
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.tracker_ref import TrackerRef
    W, S, dcap, tcap = 120, 6, 8, 64
    kw = dict(iou_threshold=thr, min_hits=2, max_age=3)
    loop = HotLoop(n_streams=S, window=W, tcap=tcap, dcap=dcap, keep_waypoints=False, tracker_kw=kw)
    n = np.zeros((S, W), np.int32)
    box = np.zeros((S, W, dcap, 4), np.int32)
    for s in range(S):
        rng = np.random.RandomState(100 + s)
        n[s] = rng.randint(0, dcap + 1, size=W)
        if s < 2:      # crowded: few anchor positions, heavy overlap between different objects
            ax = rng.randint(100, 400, size=4)
            ay = rng.randint(100, 300, size=4)
            k = rng.randint(0, 4, size=(W, dcap))
            x = ax[k] + rng.randint(-25, 26, size=(W, dcap))
            y = ay[k] + rng.randint(-15, 16, size=(W, dcap))
            w_ = rng.randint(60, 100, size=(W, dcap))
            h_ = rng.randint(40, 70, size=(W, dcap))
        elif s < 4:    # boxes on a coarse grid: exact duplicates and quotients of small integers (1/3, 1/2, ...)
            x = rng.randint(0, 6, size=(W, dcap)) * 20
            y = rng.randint(0, 3, size=(W, dcap)) * 20
            w_ = rng.choice([20, 40, 60], size=(W, dcap))
            h_ = rng.choice([20, 40], size=(W, dcap))
        else:          # sparse, temporally coherent
            x = (np.arange(dcap) * 150)[None, :] + rng.randint(-12, 13, size=(W, dcap))
            y = 300 + rng.randint(-8, 9, size=(W, dcap))
            w_ = np.full((W, dcap), 90)
            h_ = np.full((W, dcap), 60)
        box[s] = np.stack([x, y, x + w_, y + h_], axis=2)
    cls = np.random.RandomState(7).randint(0, 8, size=(S, W, dcap)).astype(np.int32)
    conf = np.random.RandomState(8).uniform(0.3, 1, size=(S, W, dcap))
    loop.det_n.copy_(torch.as_tensor(n))
    loop.det_box.copy_(torch.as_tensor(box))
    loop.det_cls.copy_(torch.as_tensor(cls))
    loop.det_conf.copy_(torch.as_tensor(conf))
    torch.cuda.synchronize()
    loop.enqueue_track()
    rows, cnt = loop.snapshots()
    d2t = loop.det2trk.cpu().numpy()
    hdr, _, _ = loop.tracker_tables()
    for s in range(S):
        ref = TrackerRef(**kw)
        overflow = False
        for f in range(W):
            r = ref.update(n[s, f], box[s, f], cls[s, f], conf[s, f])
            t = ref.table(tcap) if len(ref.rows) <= tcap else None
            if t is None:
                overflow = True
                break
            assert cnt[s, f] == t["n"], (s, f)
            m = t["n"]
            assert np.array_equal(rows[s, f]["id"][:m], t["ids"][:m]), (s, f)
            got_box = np.stack([rows[s, f][k][:m] for k in ("x1", "y1", "x2", "y2")], axis=1)
            assert np.array_equal(got_box, t["box"][:m]), (s, f)
            assert np.array_equal(np.stack([rows[s, f][k][:m] for k in ("age", "hits", "misses")], axis=1), t["ahm"][:m]), (s, f)
            assert np.array_equal(rows[s, f]["conf"][:m], t["conf"][:m]), (s, f)
            assert np.array_equal(d2t[s, f, :n[s, f]], r["det2trk"]), (s, f)
        assert overflow == bool(hdr[s, 3] & 1), s


def test_full_size_properties(torch_gpu):
    """Size-independent checks at the bench's scale (64 streams x 256 frames)."""
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.harness_ref import ego_motion
    S, W = 64, 256
    loop = HotLoop(n_streams=S, window=W)
    loop.reset(frame_offsets=[s * 17 for s in range(S)])
    loop.load_measurements(np.stack([ego_motion(W, seed=s) for s in range(S)]))
    loop.step(sync=True)
    r = loop.results()
    rows, n = loop.snapshots()
    cost, order = r["cost"], r["order"]
    srt = np.take_along_axis(cost, order.astype(np.int64), axis=2)
    assert np.all(np.diff(srt, axis=2) >= 0)                                     # sortedness
    assert np.array_equal(np.sort(order, axis=2), np.broadcast_to(np.arange(21), order.shape))   # permutation
    assert np.all(np.isfinite(r["wp"])) and np.all(r["wp"][..., 4] >= 0)
    # every track id is unique within a frame and ids grow monotonically with the row index
    for s in (0, 17, 63):
        for f in (0, 100, 255):
            ids = rows[s, f]["id"][:n[s, f]]
            assert np.all(np.diff(ids) > 0)
    assert int(loop.det_status.cpu().abs().sum()) == 0 and n.max() <= 64
    # streams with identical detector phase and identical measurements give identical results (determinism)
    loop2 = HotLoop(n_streams=2, window=W)
    loop2.reset(frame_offsets=[17, 17])
    loop2.load_measurements(np.stack([ego_motion(W, seed=1)] * 2))
    loop2.step(sync=True)
    r2 = loop2.results()
    assert np.array_equal(r2["cost"][0], r2["cost"][1]) and np.array_equal(r2["wp"][0], r2["wp"][1])
    # the small launch takes the workgroup-cooperative planner kernel, the big one the wave kernel: their cost
    # reductions use different (fixed) trees, so agreement is to the last bits, not bitwise
    np.testing.assert_allclose(r2["cost"][0], cost[1], rtol=1e-13)
    assert np.array_equal(r2["vstate"][0], r["vstate"][1])                        # KF path is the same kernel: bitwise


def test_track_table_exchange_single_rank_nccl(torch_gpu):
    """Exercises the RCCL path (one rank), both gather modes: step k's gather overlaps step k+1 and returns the right
    tables; the device pack kernel (av_pack_tracks) equals its torch statement bit for bit."""
    import torch.distributed as dist
    from multimodal_autonomous_driving_perception_and_planning_amd import distributed as D
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.harness_ref import ego_motion
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch_gpu.device("cuda", 0))
    try:
        S, W = 4, 32
        for per_frame in (False, True):
            loop = HotLoop(n_streams=S, window=W, keep_waypoints=False)
            loop.load_measurements(np.stack([ego_motion(W, seed=s) for s in range(S)]))
            x = D.TrackTableExchange(loop, 1, 0, per_frame=per_frame)
            for _ in range(3):
                loop.step()
                x.exchange()
            hdr, rows = x.latest()
            want_rows, want_n = loop.snapshots()
            frames = range(W) if per_frame else [W - 1]
            assert hdr.shape == (S, len(frames))
            for s in range(S):
                for j, f in enumerate(frames):
                    n = want_n[s, f]
                    assert hdr["n_rows"][s, j] == n and hdr["stream"][s, j] == s and hdr["frame"][s, j] == 2 * W + f + 1
                    w = want_rows[s, f][:n]
                    g = rows[s, j]
                    for k in ("id", "x1", "y1", "x2", "y2", "age", "hits", "misses", "cls", "flags"):
                        assert np.array_equal(g[k][:n], w[k]), k
                    assert np.array_equal(g["conf"][:n], w["conf"].astype(np.float32))
                    assert np.array_equal(g["vx2"][:n], (2 * w["vx"]).astype(np.int16))
                    assert np.array_equal(g["vy2"][:n], (2 * w["vy"]).astype(np.int16))
                    assert not g[n:].view(np.uint8).any()
            # kernel == torch statement on the same device tables (whole messages, bytewise)
            # (header.frame = the detector's frame count at that frame: 1-based, three windows in)
            ref = D.pack_wire(loop.snap, loop.snap_n, x.frame_lo, x.n_sel, 0, 0, loop.frame_count)
            assert torch_gpu.equal(ref, x.send[(x.k - 1) & 1])
    finally:
        dist.destroy_process_group()


def test_track_table_exchange_native_allgather(torch_gpu):
    """The gather as a library call (av_allgather_tracks on a communicator made by av_comm_unique_id / av_comm_create, RCCL
    opened with dlopen): one rank, no torch.distributed at all -- the received buffer equals the packed tables, step after step,
    and equals what the torch.distributed path of the same class receives."""
    from multimodal_autonomous_driving_perception_and_planning_amd import distributed as D
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.harness_ref import ego_motion
    S, W = 4, 16
    loop = HotLoop(n_streams=S, window=W, keep_waypoints=False)
    loop.load_measurements(np.stack([ego_motion(W, seed=s) for s in range(S)]))
    x = D.TrackTableExchange(loop, 1, 0, per_frame=True, native=True)
    assert x.native and x.nccl is not None
    try:
        for k in range(3):
            loop.step()
            got = x.exchange()
            x.synchronize()
            want = D.pack_wire(loop.snap, loop.snap_n, 0, W, 0, 0, loop.frame_count)
            assert torch_gpu.equal(got, want), k
        hdr, rows = x.latest()
        want_rows, want_n = loop.snapshots()
        assert np.array_equal(hdr["n_rows"], want_n) and np.array_equal(hdr["frame"][0], 2 * W + 1 + np.arange(W))
    finally:
        x.close()
    assert x.nccl is None


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tracker_randomised_configurations(torch_gpu, seed):
    """Random tracker parameters and scene styles (crowded / grid / coherent / mixed), 4 streams x 90 frames per case, both
    kernels (8 replica waves and AVHOT_TRACKER_REP=1 via dcap 9): every field of every row incl. the last velocity."""
    import torch
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.tracker_ref import TrackerRef
    rng = np.random.RandomState(1000 + seed)
    for case in range(4):
        kw = dict(iou_threshold=float(rng.choice([0.1, 0.3, 0.5, 0.7])), max_age=int(rng.randint(0, 6)),
                  min_hits=int(rng.randint(1, 4)), trajectory_length=int(rng.choice([1, 3, 50])))
        dcap = int(rng.choice([5, 8, 9]))                      # 9: wider than the replica kernel takes -> single-wave 16-column path
        S, W, tcap = 4, 90, 64
        loop = HotLoop(n_streams=S, window=W, tcap=tcap, dcap=dcap, keep_waypoints=False, tracker_kw=kw)
        n = rng.randint(0, dcap + 1, size=(S, W)).astype(np.int32)
        box = np.zeros((S, W, dcap, 4), np.int32)
        for s in range(S):
            style = (s + case) % 4
            if style == 0:
                a = rng.randint(50, 500, size=(3, 2))
                k = rng.randint(0, 3, size=(W, dcap))
                x, y = a[k, 0] + rng.randint(-20, 21, size=(W, dcap)), a[k, 1] + rng.randint(-12, 13, size=(W, dcap))
                w_, h_ = rng.randint(50, 90, size=(W, dcap)), rng.randint(30, 60, size=(W, dcap))
            elif style == 1:
                x, y = rng.randint(0, 5, size=(W, dcap)) * 20, rng.randint(0, 3, size=(W, dcap)) * 20
                w_, h_ = rng.choice([20, 40], size=(W, dcap)), rng.choice([20, 40], size=(W, dcap))
            elif style == 2:
                x = (np.arange(dcap) * 140)[None, :] + rng.randint(-10, 11, size=(W, dcap))
                y = 250 + rng.randint(-6, 7, size=(W, dcap))
                w_, h_ = np.full((W, dcap), 80), np.full((W, dcap), 50)
            else:
                x, y = rng.randint(0, 900, size=(W, dcap)), rng.randint(0, 500, size=(W, dcap))
                w_, h_ = rng.randint(1, 200, size=(W, dcap)), rng.randint(1, 150, size=(W, dcap))
            box[s] = np.stack([x, y, x + w_, y + h_], axis=2)
        cls = rng.randint(0, 8, size=(S, W, dcap)).astype(np.int32)
        conf = rng.uniform(0.3, 1, size=(S, W, dcap))
        loop.det_n.copy_(torch.as_tensor(n))
        loop.det_box.copy_(torch.as_tensor(box))
        loop.det_cls.copy_(torch.as_tensor(cls))
        loop.det_conf.copy_(torch.as_tensor(conf))
        torch.cuda.synchronize()
        loop.enqueue_track()
        rows, cnt = loop.snapshots()
        d2t = loop.det2trk.cpu().numpy()
        hdr, _, _ = loop.tracker_tables()
        for s in range(S):
            ref = TrackerRef(**kw)
            over = False
            for f in range(W):
                r = ref.update(n[s, f], box[s, f], cls[s, f], conf[s, f])
                if len(ref.rows) > tcap:
                    over = True
                    break
                m = len(ref.rows)
                g = rows[s, f]
                tag = (seed, case, s, f, kw, dcap)
                assert cnt[s, f] == m, tag
                assert np.array_equal(g["id"][:m], [q["id"] for q in ref.rows]), tag
                assert np.array_equal(np.stack([g[k][:m] for k in ("x1", "y1", "x2", "y2")], 1).reshape(m, 4), np.array([q["bbox"] for q in ref.rows]).reshape(m, 4)), tag
                assert np.array_equal(np.stack([g[k][:m] for k in ("age", "hits", "misses")], 1).reshape(m, 3), np.array([(q["age"], q["hits"], q["misses"]) for q in ref.rows]).reshape(m, 3)), tag
                assert np.array_equal(g["conf"][:m], [q["conf"] for q in ref.rows]) and np.array_equal(g["cls"][:m], [q["cls"] for q in ref.rows]), tag
                assert np.array_equal(g["flags"][:m] & 1, [int(q["hits"] >= kw["min_hits"]) for q in ref.rows]), tag
                for i, q in enumerate(ref.rows):
                    if q["vel"]:
                        assert (g["vx"][i], g["vy"][i]) == q["vel"][-1], tag
                        assert g["hist_len"][i] >= 2, tag
                assert np.array_equal(d2t[s, f, :n[s, f]], r["det2trk"]), tag
            assert over == bool(hdr[s, 3] & 1), (seed, case, s)


def test_tracker_long_window_many_detection_chunks(torch_gpu):
    """bench config2 runs one stream over a 131072-frame window: the kernel stages detections 56 frames at a time
    (the replica kernel fetches the next chunk into registers while it works on the current one).  4133 frames --
    73 full chunks and a ragged one -- then a second window on the carried state, against the oracle tracker fed
    the same simulated detections: ids, boxes, counters and detection->track ids of every frame."""
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    from oracle.tracker_ref import TrackerRef
    S, W = 2, 4133
    loop = HotLoop(n_streams=S, window=W, keep_waypoints=False)
    loop.reset(frame_offsets=[0, 1234])
    refs = [TrackerRef() for _ in range(S)]
    for window in range(2):
        loop.enqueue_detect()
        loop.enqueue_track()
        loop.synchronize()
        n = loop.det_n.cpu().numpy()
        box, cls, conf = loop.det_box.cpu().numpy(), loop.det_cls.cpu().numpy(), loop.det_conf.cpu().numpy()
        rows, cnt = loop.snapshots()
        d2t = loop.det2trk.cpu().numpy()
        for s in range(S):
            for f in range(W):
                r = refs[s].update(n[s, f], box[s, f], cls[s, f], conf[s, f])
                t = refs[s].table(64)
                k = t["n"]
                assert cnt[s, f] == k, (window, s, f)
                got = rows[s, f]
                assert np.array_equal(got["id"][:k], t["ids"][:k]), (window, s, f)
                assert np.array_equal(d2t[s, f, :n[s, f]], r["det2trk"]), (window, s, f)
                if f % 97 == 0 or f == W - 1:
                    for name, key in (("x1", 0), ("y1", 1), ("x2", 2), ("y2", 3)):
                        assert np.array_equal(got[name][:k], t["box"][:k, key]), (window, s, f, name)
                    for name, key in (("age", 0), ("hits", 1), ("misses", 2)):
                        assert np.array_equal(got[name][:k], t["ahm"][:k, key]), (window, s, f, name)
                    assert np.array_equal(got["cls"][:k], t["cls"][:k]) and np.array_equal(got["conf"][:k], t["conf"][:k])
    assert int(loop.det_status.cpu().abs().sum()) == 0


@pytest.mark.parametrize("W", [16, 55, 56, 57, 113])
def test_tracker_trailing_wave_equals_in_place_update(torch_gpu, W, monkeypatch):
    """Windows of >= 16 frames keep the complete rows on a ninth wave that trails the column waves by one frame
    (AVHOT_TRACKER_PIPE=0: the in-place kernel).  Window lengths around the 56-frame detection chunk, crowded random scenes
    with births and deaths in most frames, two windows on the carried state: every output of the call and the persisted
    state (header, rows, history rings) must be the same bytes."""
    import torch
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    rng = np.random.RandomState(77 + W)
    S, dcap = 6, 8
    kw = dict(iou_threshold=0.3, max_age=2, min_hits=2, trajectory_length=5)
    n = rng.randint(0, dcap + 1, size=(2, S, W)).astype(np.int32)
    a = rng.randint(50, 700, size=(12, 2))
    k = rng.randint(0, 12, size=(2, S, W, dcap))
    x, y = a[k, 0] + rng.randint(-25, 26, size=k.shape), a[k, 1] + rng.randint(-15, 16, size=k.shape)
    w_, h_ = rng.randint(50, 90, size=k.shape), rng.randint(30, 60, size=k.shape)
    box = np.stack([x, y, x + w_, y + h_], axis=-1).astype(np.int32)
    cls = rng.randint(0, 8, size=k.shape).astype(np.int32)
    conf = rng.uniform(0.3, 1, size=k.shape)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("AVHOT_TRACKER_PIPE", mode)
        loop = HotLoop(n_streams=S, window=W, tcap=64, dcap=dcap, keep_waypoints=False, tracker_kw=kw)
        got = []
        for win in range(2):
            loop.det_n.copy_(torch.as_tensor(n[win]))
            loop.det_box.copy_(torch.as_tensor(box[win]))
            loop.det_cls.copy_(torch.as_tensor(cls[win]))
            loop.det_conf.copy_(torch.as_tensor(conf[win]))
            torch.cuda.synchronize()
            loop.enqueue_track()
            rows, cnt = loop.snapshots()
            live = np.arange(64)[None, None, :] < cnt[:, :, None]
            got.append((np.where(live, rows.view(np.uint8).reshape(S, W, 64, -1).sum(-1), 0), cnt.copy(), loop.det2trk.cpu().numpy().copy()))
            got.append(tuple(np.array(t, copy=True) for t in loop.tracker_tables()))
            # live rows, byte for byte
            got.append(tuple(rows[s, f][: cnt[s, f]].tobytes() for s in range(S) for f in range(W)))
        out[mode] = got
    assert int(out["1"][1][0][:, 0].max()) > 8                      # the scenes do fill the tables
    for p, q in zip(out["0"], out["1"]):
        for u, v in zip(p, q):
            if isinstance(u, bytes):
                assert u == v
            else:
                assert np.array_equal(u, v)
