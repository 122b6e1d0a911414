"""The two per-stream chains of the one-launch time-step from the outside, bit for bit against code the step
does not share its entry paths with -- the stage launches (simdet_kernel, tracker_kernel, kf_axis_kernel / kf_kernel, planner_kernel)
-- and, for the overlapped loop, against the serial one:
  tracker role   the detections' output arrays, which thread 0's wave stores in front of the role's wait; a full tracker table through
                 tracker_body's LDS-read path (INIT_LDS)
  Kalman role    the three branches of the chain part's heading; the separability verdict on a record the host edited between two
                 steps (1e-300, -0.0, NaN in a cross-axis entry of P; the dense flag preset); dense and separable streams in one launch

Streams: S = 1 and 3, depth 1 (serial launches, sixteen waves) and depth 4 (twelve waves, the shape it has at 64 streams)."""
import numpy as np
import pytest

from tests import kf_cases as K

pytestmark = pytest.mark.gpu

CFG = "B"
D = 4


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return t


def _kw():
    return dict(zip(("dt", "process_noise", "measurement_noise"), K.SETTINGS[CFG]))


def _loop(monkeypatch, S, depth=1, fused=True, **kw):
    """A HotLoop of S streams from the reset state: depth 1 = serial launches (fused or the four stage launches), depth 4 = overlapped
    steps in the twelve-wave shape (AVHOT_STEP_PW is read at every launch: the caller's monkeypatch keeps it for the test)."""
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    if depth > 1:
        monkeypatch.setenv("AVHOT_STEP_PW", "12")
        lp = HotLoop(n_streams=S, window=1, kf_kw=_kw(), overlap=depth, **kw)
        assert lp.fused_step and lp.overlap == depth and lp.step_waves == 12
    else:
        monkeypatch.delenv("AVHOT_STEP_PW", raising=False)
        lp = HotLoop(n_streams=S, window=1, kf_kw=_kw(), fused_step=fused, **kw)
        assert bool(lp.fused_step) == fused and lp.overlap == 1
    lp.reset()
    return lp


def _set_outputs(lp, k=None):
    """The per-step outputs in buffer set k (None: the set of the step enqueued last), snapshot rows past the live count zeroed."""
    lp.synchronize()
    b = lp._sets[k] if k is not None else {n: getattr(lp, n) for n in lp._sets[0]}
    out = {n: b[n].cpu().numpy() for n in ("det_n", "det_box", "det_cls", "det_conf", "det2trk", "vstate", "plan_state", "wp", "cost", "order",
                                           "snap_n")}
    snap = b["snap"].cpu().numpy().copy()
    for s in range(lp.S):
        snap[s, 0, out["snap_n"][s, 0]:] = 0
    out["snap"] = snap
    return out


def _state(lp):
    lp.synchronize()
    return dict(kf=lp.kf_state.cpu().numpy(), trk=lp.trk_state.cpu().numpy(), fc=lp.frame_count.cpu().numpy())


def _same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (where, k, int((x.view(np.uint8) != y.view(np.uint8)).sum()))


def _run(torch, lp, z, t0, t1, keep=()):
    """Steps t0 .. t1 - 1 with the measurements z[:, t]: one unsynchronised library call at depth 2.., step by step otherwise.
    -> {t: outputs} for the steps in `keep` that a serial loop can still show (it is synchronised there)."""
    got = {}
    if lp.overlap > 1:
        zs = torch.as_tensor(np.ascontiguousarray(z[:, t0:t1].transpose(1, 0, 2))).to(lp.dev)
        torch.cuda.synchronize()
        lp.enqueue_steps(t1 - t0, z_steps=zs)
        lp.synchronize()
        fl = lp.seq_flags.cpu().numpy()
        assert fl[0:64 * lp.S:32].tolist() == [t1] * (2 * lp.S) and fl[64 * lp.S] == 0, "every role published every step; fault word 0"
        return got
    for t in range(t0, t1):
        lp.load_measurements(z[:, t:t + 1])
        lp.enqueue_step()
        if t in keep:
            got[t] = dict(_set_outputs(lp), **_state(lp))
    return got


def _last_sets(lp, steps):
    """{t: outputs} of the last D steps of an overlapped loop: step t wrote buffer set t % D."""
    return {t: _set_outputs(lp, t % lp.overlap) for t in range(steps - lp.overlap, steps)}


# ---- test 1: the three branches of the chain part's heading ------------------------------------------------------------------------
HEADING_SEEDS = (0, 1, 2)
HEADING_STEPS = K.LOOP_STEPS                       # 150


def _heading_branches(c):
    """Per frame of a mode-1 sequence the oracle extracts after the predict (p) and after the update (q).  The chain part hands on
    atan2 of the post-update velocity when speed_q > 0.1, else atan2 of the predict-time velocity when speed_p > 0.1, else the record's
    heading.  -> how often each is taken, and how often the frame's heading difference wraps at +-pi."""
    m = c["margins"]
    W = len(c["mode"])
    assert len(m["frame"]) == 2 * W and np.array_equal(m["frame"][0::2], np.arange(W))
    hp, hq = m["held"][0::2], m["held"][1::2]
    return dict(post=int((~hq).sum()), pred=int((hq & ~hp).sum()), held=int((hq & hp).sum()),
                wraps=int(m["wrapped"][0::2].sum() + m["wrapped"][1::2].sum()))


@pytest.fixture(scope="module")
def heading_cases():
    cases = [K.case("loop", CFG, s) for s in HEADING_SEEDS]
    for c in cases:                                 # from the oracle alone, before any launch
        v = _heading_branches(c)
        assert v["post"] >= 5 and v["pred"] >= 5 and v["held"] >= 5 and v["wraps"] >= 1, v
        assert K.min_margin(c["margins"]) >= K.MARGIN
        assert c["P0"] is None and len(c["mode"]) == HEADING_STEPS
    return cases


@pytest.fixture(scope="module")
def heading_stage(torch, heading_cases):
    """{S: every step's outputs and state from the four stage launches (kf_axis_kernel's kf_axis_body)}; computed once, left alone."""
    mp = pytest.MonkeyPatch()
    want = {}
    for S in (1, 3):
        z = np.stack([c["z"] for c in heading_cases[:S]])
        want[S] = _run(torch, _loop(mp, S, fused=False), z, 0, HEADING_STEPS, keep=range(HEADING_STEPS))
    mp.undo()
    return want


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("S", [1, 3])
def test_heading_branches(torch, monkeypatch, heading_cases, heading_stage, S, depth):
    cases, want = heading_cases[:S], heading_stage[S]
    z = np.stack([c["z"] for c in cases])
    lp = _loop(monkeypatch, S, depth)
    if depth == 1:
        got = _run(torch, lp, z, 0, HEADING_STEPS, keep=range(HEADING_STEPS))
        for t in range(HEADING_STEPS):
            _same(want[t], got[t], "S = %d, serial fused step %d against the stage launches" % (S, t))
            for s in range(S):
                np.testing.assert_allclose(got[t]["vstate"][s, 0], cases[s]["want"][t], rtol=1e-9, atol=1e-9, err_msg="s=%d t=%d" % (s, t))
    else:
        _run(torch, lp, z, 0, HEADING_STEPS)
        last = _last_sets(lp, HEADING_STEPS)
        for t, o in last.items():
            _same({k: want[t][k] for k in o}, o, "S = %d, depth %d, step %d against the stage launches" % (S, depth, t))
            for s in range(S):
                np.testing.assert_allclose(o["vstate"][s, 0], cases[s]["want"][t], rtol=1e-9, atol=1e-9, err_msg="s=%d t=%d" % (s, t))
        st = _state(lp)
        _same({k: want[HEADING_STEPS - 1][k] for k in st}, st, "S = %d, depth %d, records after the last step" % (S, depth))
        for s in range(S):                          # the record's heading, speed and time are the oracle's
            np.testing.assert_allclose(st["kf"][s, :45], cases[s]["rec"], rtol=1e-9, atol=1e-9)


# ---- test 2: the separability verdict on a record the host edited ---------------------------------------------------------------
VERDICT_K, VERDICT_STEPS, VERDICT_S, VERDICT_STREAM = 7, 30, 3, 1


def _verdict_run(torch, monkeypatch, depth, fused, edit):
    """VERDICT_K steps, the host edits stream VERDICT_STREAM's record, one step, then the rest.  -> (flags after step K + 1, final)."""
    cases = [K.case("loop", CFG, s) for s in HEADING_SEEDS]
    z = np.stack([c["z"] for c in cases])
    lp = _loop(monkeypatch, VERDICT_S, depth, fused)
    _run(torch, lp, z, 0, VERDICT_K)
    lp.synchronize()
    rec = lp.kf_state.cpu().numpy().copy()
    assert (rec[:, 45] == 0).all()
    edit(rec[VERDICT_STREAM])
    lp.kf_state.copy_(torch.as_tensor(rec))
    torch.cuda.synchronize()
    _run(torch, lp, z, VERDICT_K, VERDICT_K + 1)
    flags = _state(lp)["kf"][:, 45].copy()
    _run(torch, lp, z, VERDICT_K + 1, VERDICT_STEPS)
    return flags, dict(_set_outputs(lp), **_state(lp))


def _edits():
    out = []
    for r, c in ((0, 1), (5, 0)):                    # a cross-axis entry in the first and in the last row of P
        assert (r ^ c) & 1
        for name, v, dense in (("tiny", 1e-300, True), ("negzero", -0.0, False), ("nan", float("nan"), True)):
            out.append(pytest.param(6 + 6 * r + c, v, dense, id="P%d%d-%s" % (r, c, name)))
    out.append(pytest.param(45, 1.0, True, id="flag-preset"))          # kf_state[45] preset with a clean P
    return out


@pytest.mark.parametrize("word,value,dense", _edits())
def test_separability_verdict_after_a_host_edit(torch, monkeypatch, word, value, dense):
    def edit(rec):
        rec[word] = value
    want_flags, want = _verdict_run(torch, monkeypatch, 1, False, edit)              # the stage launches (kf_axis_body's own check)
    expect = [1.0 if (dense and s == VERDICT_STREAM) else 0.0 for s in range(VERDICT_S)]
    assert want_flags.tolist() == expect
    for depth in (1, 4):
        flags, got = _verdict_run(torch, monkeypatch, depth, True, edit)
        assert flags.tolist() == expect, ("depth", depth)
        _same(want, got, "depth %d" % depth)
    if not dense:
        assert np.signbit(want["kf"][VERDICT_STREAM, word]) and want["kf"][VERDICT_STREAM, word] == 0.0      # -0.0 stays in the record


# ---- test 3: dense and separable streams in one launch ------------------------------------------------------------------------------
def test_dense_and_separable_streams_in_one_launch(torch, monkeypatch):
    seeds, dense, steps = (2, 3, 4), 1, 150
    assert seeds[dense] == K.LOOP_DENSE_STREAM
    cases = [K.case("loop", CFG, s) for s in seeds]
    z = np.stack([c["z"] for c in cases])

    def make(depth):
        lp = _loop(monkeypatch, 3, depth)
        rec = lp.kf_state.cpu().numpy()
        rec[dense, 6:42] = cases[dense]["P0"].reshape(36)
        lp.kf_state.copy_(torch.as_tensor(rec))
        torch.cuda.synchronize()
        return lp
    want = _run(torch, make(1), z, 0, steps, keep=range(steps - D, steps))
    over = make(D)
    _run(torch, over, z, 0, steps)                  # one library call, no host synchronisation
    for t, o in _last_sets(over, steps).items():
        _same({k: want[t][k] for k in o}, o, "step %d (buffer set %d)" % (t, t % D))
    st = _state(over)
    _same({k: want[steps - 1][k] for k in st}, st, "state after %d steps" % steps)
    assert st["kf"][:, 45].tolist() == [0.0, 1.0, 0.0]


# ---- test 4: the detections' output arrays, stored in front of the wait ------------------------------------------------------------
DET_STEPS = 100
_det_refs = {}


def _det_reference(torch, dcap):
    """Per dcap, once: simdet_kernel's output for the last D of DET_STEPS frames, and the serial fused loop's snapshot rows."""
    if dcap not in _det_refs:
        mp = pytest.MonkeyPatch()
        z = np.stack([K.case("loop", CFG, s)["z"] for s in HEADING_SEEDS])
        det = _loop(mp, 3, fused=False, dcap=dcap)
        dets = {}
        for t in range(DET_STEPS):
            det.enqueue_detect()
            if t >= DET_STEPS - D:
                det.synchronize()
                dets[t] = {k: getattr(det, k).cpu().numpy() for k in ("det_n", "det_box", "det_cls", "det_conf")}
        status = det.det_status.cpu().numpy()
        serial = _run(torch, _loop(mp, 3, dcap=dcap), z, 0, DET_STEPS, keep=range(DET_STEPS - D, DET_STEPS))
        mp.undo()
        _det_refs[dcap] = (z, dets, status, serial)
    return _det_refs[dcap]


@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("status", [True, False])
@pytest.mark.parametrize("dcap", [7, 8])
def test_detection_outputs_stored_before_the_wait(torch, monkeypatch, dcap, status, wire):
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    z, dets, want_status, serial = _det_reference(torch, dcap)
    lp = _loop(monkeypatch, 3, D, dcap=dcap)
    if not status:
        lp._cloop.det_status = None
    zs = torch.as_tensor(np.ascontiguousarray(z[:, :DET_STEPS].transpose(1, 0, 2))).to(lp.dev)
    wires = None
    if wire:
        wires = torch.zeros(DET_STEPS, 3, int(nat.lib().av_wire_table_bytes(64)), dtype=torch.uint8, device=lp.dev)
        lp.set_wire(None, stream0=40, frame0=1000)
    torch.cuda.synchronize()
    lp.enqueue_steps(DET_STEPS, z_steps=zs, wire_steps=wires)
    lp.synchronize()
    fl = lp.seq_flags.cpu().numpy()
    assert fl[0:64 * 3:32].tolist() == [DET_STEPS] * 6 and fl[64 * 3] == 0
    for t, o in _last_sets(lp, DET_STEPS).items():
        _same(dets[t], {k: o[k] for k in dets[t]}, "dcap %d, step %d against simdet_kernel" % (dcap, t))
        _same({k: serial[t][k] for k in ("snap", "snap_n", "det2trk")}, {k: o[k] for k in ("snap", "snap_n", "det2trk")},
              "dcap %d, step %d against the serial loop" % (dcap, t))
    assert np.array_equal(lp.det_status.cpu().numpy(), want_status if status else np.zeros_like(want_status))
    if wire:
        assert wires[DET_STEPS - D:].cpu().numpy().any(axis=2).all()          # every stream's table of the last D steps was written


# ---- test 5: a full tracker table through the LDS-read path ------------------------------------------------------------------------
def test_full_table_read_from_lds(torch, monkeypatch):
    """Rows 55..63 live (the construction of tests/test_gpu_step_full_table.py): the fused step, launched serially and at depth 4,
    against tracker_kernel's stage launches."""
    from tests import test_gpu_step_full_table as F
    kw, steps = dict(iou_threshold=0.95, max_age=30), 30
    z = F._measurements(steps)
    want, want_wires = F._stage_launches(torch, kw, steps, z)
    serial, wires, live = F._serial_reference(torch, kw, steps, z)
    assert live.max() == 64 and (want["hdr"][:, 0] == 64).any()          # rows 55..63 are live
    F._same(want, serial, "serial fused loop")
    assert np.array_equal(want_wires, wires)
    got, wires = F._overlapped(torch, monkeypatch, kw, steps, z, 4)
    F._same(want, got, "depth 4")
    assert np.array_equal(want_wires, wires)
