"""The Kalman stage (csrc/kf.hip, csrc/kf_dev.h, csrc/kf_dense.inc) through av_kf_step against oracle/kf_ref.py on the paths the other
tests never feed: mode arrays in a window, standstill (the heading hold and its carries across 64-frame batches), the +-pi wrap,
non-default settings, dt = 0, the steady loop left and re-entered, the register-form dense kernel over windows -- and the bit
identities the kernel claims: every partition of a sequence into launches gives the same bytes, and the dense filter's register
and LDS forms give the same bytes.  The inputs come from tests/kf_cases.py; tests/test_kf_cases_host.py proves on the CPU that
they visit these paths and keep every decision of the extract 1e-6 away from its threshold.

Tolerances are those of the existing tests (test_gpu_kernels.py::test_kf_matches_oracle for the axis path,
test_gpu_more.py::test_kf_dense_fallback_for_non_separable_covariance for the dense one).  Every test prints its largest error."""
import ctypes as C

import numpy as np
import pytest

from tests import kf_cases as K

pytestmark = pytest.mark.gpu

AXIS = dict(state=(1e-9, 1e-9), x=(1e-10, 1e-10), P=(1e-10, 1e-12))          # (rtol, atol)
DENSE = dict(state=(1e-8, 1e-8), x=(1e-8, 1e-8), P=(1e-8, 1e-10))


class Kf:
    """av_kf_step / av_kf_reset on torch tensors."""

    def __init__(self, torch):
        from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
        self.torch, self.nat, self.L = torch, nat, nat.lib()
        self.ctx = nat.default_context(0)
        self.dev = torch.device("cuda", 0)

    def reset(self, S, P0=None, x0=None):
        """[S, 48] device records in the reset state; P0 / x0: {stream: array} assigned on top of it."""
        st = self.torch.full((S, self.nat.KF_STATE_DOUBLES), float("nan"), dtype=self.torch.float64, device=self.dev)
        self.nat.check(self.L.av_kf_reset(self.ctx.handle, self.nat.stream_handle(), S, self.nat.ptr(st)))
        if P0 or x0:
            h = st.cpu().numpy()
            for s, P in (P0 or {}).items():
                h[s, 6:42] = np.asarray(P, np.float64).reshape(36)
            for s, x in (x0 or {}).items():
                h[s, :6] = x
            st.copy_(self.torch.as_tensor(h))
        return st

    def call(self, cfg, S, W, z, mode, st, out, plan):
        c = self.nat.KfCfg(*cfg)
        return self.L.av_kf_step(self.ctx.handle, self.nat.stream_handle(), C.byref(c), S, W, self.nat.ptr(z), self.nat.ptr(mode),
                                 self.nat.ptr(st), self.nat.ptr(out), self.nat.ptr(plan))

    def run(self, cfg, z, mode, st, chunks=None, null_z=False):
        """Advances the records `st` over z [S, W, 4] / mode [S, W] (NumPy), one launch per chunk of frames (default: one
        window).  Returns (out_state [S, W, 12], plan_state [S, W, 4], kf_state [S, 48]) as NumPy arrays; outputs the
        kernels did not write stay NaN."""
        t = self.torch
        S, W = mode.shape
        zt = None if null_z else t.as_tensor(np.array(z, np.float64)).to(self.dev)
        mt = t.as_tensor(np.array(mode, np.uint8)).to(self.dev)
        outs, plans, f0 = [], [], 0
        for n in (chunks or [W]):
            zc = None if zt is None else zt[:, f0:f0 + n].contiguous()
            mc = mt[:, f0:f0 + n].contiguous()
            out = t.full((S, n, 12), float("nan"), dtype=t.float64, device=self.dev)
            plan = t.full((S, n, 4), float("nan"), dtype=t.float64, device=self.dev)
            self.nat.check(self.call(cfg, S, n, zc, mc, st, out, plan))
            outs.append(out), plans.append(plan)
            f0 += n
        assert f0 == W
        t.cuda.synchronize()
        return t.cat(outs, 1).cpu().numpy(), t.cat(plans, 1).cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def kf():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return Kf(torch)


def _chunks(W, n):
    return [n] * (W // n) + ([W % n] if W % n else [])


def _split(W):
    head = [63, 65, 64, 1, 2, 129]
    assert W > sum(head)
    return head + [W - sum(head)]


class Worst:
    """Largest absolute and relative error seen by the comparisons of one test, and the largest fraction of the allowed error."""

    def __init__(self):
        self.abs = self.rel = self.bound = 0.0

    def close(self, got, want, tol, what):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, what
        assert np.isfinite(got).all(), what
        d = np.abs(got - want)
        self.abs = max(self.abs, float(d.max()))
        nz = tol[0] * np.abs(want) >= tol[1]            # (relative error where the relative term of the bound is the larger one)
        if nz.any():
            self.rel = max(self.rel, float((d[nz] / np.abs(want[nz])).max()))
        self.bound = max(self.bound, float((d / (tol[1] + tol[0] * np.abs(want))).max()))
        np.testing.assert_allclose(got, want, rtol=tol[0], atol=tol[1], err_msg=str(what))

    def report(self, name):
        print("%s: largest error abs %.3e, rel %.3e (where rtol |want| >= atol), %.3e of the bound atol + rtol |want|"
              % (name, self.abs, self.rel, self.bound))


def _against_oracle(worst, out, plan, st, s, c, tol, where):
    """Every frame and field of stream s against the oracle run c: out_state, plan_state (x, y, heading, speed), the final
    record (x, P, prev_heading, prev_speed, time)."""
    worst.close(out[s], c["want"], tol["state"], (where, s, "out_state"))
    worst.close(plan[s], c["want"][:, [0, 1, 4, 5]], tol["state"], (where, s, "plan_state"))
    worst.close(st[s, :6], c["rec"][:6], tol["x"], (where, s, "x"))
    worst.close(st[s, 6:42], c["rec"][6:42], tol["P"], (where, s, "P"))
    worst.close(st[s, 42:45], c["rec"][42:45], tol["state"], (where, s, "prev_heading, prev_speed, time"))
    assert np.array_equal(plan[s], out[s][:, [0, 1, 4, 5]]), (where, s)
    assert not st[s, 46:48].any(), (where, s)


def _stack(cases):
    return np.stack([c["z"] for c in cases]), np.stack([c["mode"] for c in cases])


def _same_bytes(a, b, where):
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        diff = x.view(np.uint64) != y.view(np.uint64)
        assert not diff.any(), (where, ("out_state", "plan_state", "kf_state")[k], int(diff.sum()), np.argwhere(diff)[:4].tolist())


# ---- (a) mixed modes, standstill and wrap in one window ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["A", "B", "C"])
def test_mixed_modes_standstill_and_wrap_in_one_window(kf, cfg):
    cases = [K.case("mixed", cfg, s) for s in K.MIXED_SEEDS]
    z, mode = _stack(cases)
    out, plan, st = kf.run(K.SETTINGS[cfg], z, mode, kf.reset(len(cases)))
    worst = Worst()
    for s, c in enumerate(cases):
        _against_oracle(worst, out, plan, st, s, c, AXIS, "mixed " + cfg)
    assert (st[:, 45] == 0.0).all()
    worst.report("mixed modes, setting " + cfg)


def test_every_pair_of_modes_across_a_batch_edge(kf):
    c = K.case("edges", "B", 100)
    out, plan, st = kf.run(K.B, c["z"][None], c["mode"][None], kf.reset(1))
    worst = Worst()
    _against_oracle(worst, out, plan, st, 0, c, AXIS, "edges")
    assert st[0, 45] == 0.0
    worst.report("mode pairs at batch edges")


# ---- (b) z == NULL ----------------------------------------------------------------------------------------------------------------
def test_window_without_measurements_does_not_read_z(kf):
    cases = [K.case("null_z", "B", s) for s in K.NULL_Z_SEEDS]
    z, mode = _stack(cases)
    S, H = len(cases), K.NULL_Z_HEAD
    runs = []
    for variant in ("null", "nan"):
        st = kf.reset(S)
        head = kf.run(K.B, z[:, :H], mode[:, :H], st)
        if variant == "null":
            tail = kf.run(K.B, None, mode[:, H:], st, null_z=True)
        else:
            tail = kf.run(K.B, np.full_like(z[:, H:], np.nan), mode[:, H:], st)
        runs.append((np.concatenate([head[0], tail[0]], 1), np.concatenate([head[1], tail[1]], 1), tail[2]))
    worst = Worst()
    for s, c in enumerate(cases):
        _against_oracle(worst, *runs[0], s, c, AXIS, "z == NULL")
    _same_bytes(runs[0], runs[1], "z == NULL against a z full of NaN")
    worst.report("z == NULL")
    # neither measurements nor modes: refused
    t = kf.torch
    st = kf.reset(1)
    before = st.cpu().numpy()
    out = t.zeros(1, 1, 12, dtype=t.float64, device=kf.dev)
    assert kf.call(K.B, 1, 1, None, None, st, out, None) == -1                    # AV_EINVAL
    t.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), before)


# ---- (c) dt = 0 -------------------------------------------------------------------------------------------------------------------
def test_zero_dt_gives_exact_zero_rates(kf):
    cases = [K.case("zero_dt", "Z", s) for s in K.ZERO_DT_SEEDS]
    z, mode = _stack(cases)
    out, plan, st = kf.run(K.Z, z, mode, kf.reset(len(cases)))
    assert (out[:, :, 6] == 0.0).all() and (out[:, :, 7] == 0.0).all()          # acceleration, yaw rate
    assert (out[:, :, 8] == 0.0).all() and (st[:, 44] == 0.0).all()              # the clock does not move
    worst = Worst()
    for s, c in enumerate(cases):
        _against_oracle(worst, out, plan, st, s, c, AXIS, "dt = 0")
    worst.report("dt = 0")


# ---- (d) the steady loop entered, left and re-entered -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["B", "D"])
def test_steady_loop_is_left_and_reentered_on_disturbances(kf, cfg):
    cases = [K.case("steady", cfg, s) for s in K.STEADY_SEEDS]
    z, mode = _stack(cases)
    out, plan, st = kf.run(K.SETTINGS[cfg], z, mode, kf.reset(len(cases)))
    worst = Worst()
    for s, c in enumerate(cases):
        _against_oracle(worst, out, plan, st, s, c, AXIS, "steady " + cfg)
    # the device's own covariance repeats bit for bit before each disturbance (the steady loop's condition) and moves on it
    for s in range(len(cases)):
        for f in K.STEADY_DISTURBANCES:
            unc = out[s, :, 9:11]
            assert (unc[f - 20:f] == unc[f - 1]).all(), (s, f)
            assert (unc[f] != unc[f - 1]).all(), (s, f)
    worst.report("steady loop, setting " + cfg)


# ---- (e) partition invariance, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cfg,seeds", [("mixed", "A", K.MIXED_SEEDS[:3]), ("mixed", "B", K.MIXED_SEEDS[:3]),
                                            ("mixed", "C", K.MIXED_SEEDS[:3]), ("steady", "B", K.STEADY_SEEDS),
                                            ("steady", "D", K.STEADY_SEEDS), ("edges", "B", (100,))])
def test_every_partition_into_launches_gives_the_same_bytes(kf, kind, cfg, seeds):
    """One window against launches of 1, 2 and 3 frames and an uneven split around the 64-frame batch size: the steady loop
    against the general loop, the lane = frame extract against the extract carried through kf_state[42..43], and
    kf_axis_kernel<true> (one and two frames) against <false>."""
    cases = [K.case(kind, cfg, s) for s in seeds]
    z, mode = _stack(cases)
    S, W = mode.shape
    one = kf.run(K.SETTINGS[cfg], z, mode, kf.reset(S))
    assert np.isfinite(one[0]).all() and (one[2][:, 45] == 0.0).all()
    for name, chunks in (("1-frame launches", _chunks(W, 1)), ("2-frame launches", _chunks(W, 2)),
                         ("3-frame launches", _chunks(W, 3)), ("63+65+64+1+2+129+rest", _split(W))):
        _same_bytes(one, kf.run(K.SETTINGS[cfg], z, mode, kf.reset(S), chunks), (kind, cfg, name))


# ---- (f) the register-form dense kernel over windows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_dense_kernel_over_windows(kf, cfg):
    """67 streams, four of them with a non-separable covariance: kf_kernel (the register form of kf_dense.inc) runs them over a
    200-frame window in two blocks; the LDS form (one- and two-frame launches, inside kf_axis_kernel<true>) gives the same bytes."""
    S, W, flagged = K.DENSE_S, K.DENSE_W, sorted(K.DENSE_STREAMS)
    setting = K.SETTINGS[cfg]
    zm = [K.kf_scenario(W, K.DENSE_SEED0 + s, setting[0]) for s in range(S)]
    z, mode = np.stack([a for a, _ in zm]), np.stack([b for _, b in zm])
    P0 = {s: K.dense_P0(kind) for s, kind in K.DENSE_STREAMS.items()}
    window = kf.run(setting, z, mode, kf.reset(S, P0))
    out, plan, st = window
    worst = Worst()
    for s in flagged:
        c = K.case("dense", cfg, s)
        assert np.array_equal(c["z"], z[s]) and np.array_equal(c["mode"], mode[s])
        _against_oracle(worst, out, plan, st, s, c, DENSE, "dense " + cfg)
    assert np.flatnonzero(st[:, 45]).tolist() == flagged and (st[flagged, 45] == 1.0).all()
    # the other 63 streams are not touched by it: the same bytes as a run in which no stream is flagged
    plain = kf.run(setting, z, mode, kf.reset(S))
    assert (plain[2][:, 45] == 0.0).all()
    rest = [s for s in range(S) if s not in flagged]
    _same_bytes([a[rest] for a in window], [a[rest] for a in plain], "unflagged streams")
    assert not np.array_equal(window[0][flagged], plain[0][flagged])
    # register form == LDS form (kf_dense.inc)
    zf, mf = z[flagged], mode[flagged]
    Pf = {i: P0[s] for i, s in enumerate(flagged)}
    for name, n in (("1-frame launches", 1), ("2-frame launches", 2)):
        lds = kf.run(setting, zf, mf, kf.reset(len(flagged), Pf), _chunks(W, n))
        assert (lds[2][:, 45] == 1.0).all()
        _same_bytes([a[flagged] for a in window], lds, ("dense", cfg, name))
    worst.report("dense kernel over windows, setting " + cfg)


# ---- (g) user-assigned separable covariance ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def estimator(kf):
    from src.state_estimation import VehicleStateEstimator
    return VehicleStateEstimator


def _drive(est, z, mode):
    """The estimator's own calls for a (z, mode) sequence; returns the 12-field states."""
    from oracle.kf_ref import STATE_FIELDS
    got = np.zeros((len(mode), 12))
    for f in range(len(mode)):
        m = int(mode[f])
        st = est.predict() if m == 0 else est.step(z[f]) if m == 1 else est.step() if m == 2 else est.update(z[f])
        got[f] = [getattr(st, n) for n in STATE_FIELDS]
    return got


def test_user_assigned_separable_covariance_stays_on_the_axis_path(estimator):
    c = K.case("separable", "A", K.SEPARABLE_SEED)
    est = estimator()
    est.kf.P = c["P0"]
    est.kf.x = c["x0"]
    assert np.array_equal(est.kf.P, c["P0"]) and np.array_equal(est.kf.x, c["x0"])
    got = _drive(est, c["z"], c["mode"])
    worst = Worst()
    worst.close(got, c["want"], AXIS["state"], "separable: states")
    worst.close(est.kf.x, c["rec"][:6], AXIS["x"], "separable: x")
    worst.close(est.kf.P.reshape(36), c["rec"][6:42], AXIS["P"], "separable: P")
    worst.close([est.prev_heading, est.prev_speed, est.time], c["rec"][42:45], AXIS["state"], "separable: carries")
    assert float(est._state[0, 45].item()) == 0.0
    worst.report("user-assigned separable covariance")


# ---- (h) non-default settings through the fused step and the class -----------------------------------------------------------------------
def _outputs(loop):
    loop.synchronize()
    r = loop.results()
    rows, n = loop.snapshots()
    hdr, trows, hist = loop.tracker_tables()
    out = dict(r)
    out.update(snap=rows.view(np.uint8), snap_n=n, hdr=hdr, trows=trows.view(np.uint8), hist=hist,
               kf=loop.kf_state.cpu().numpy(), plan_state=loop.plan_state.cpu().numpy(), fc=loop.frame_count.cpu().numpy())
    return out


def _same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (where, k, int((x != y).sum()))


def test_fused_step_with_non_default_settings(kf):
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import HotLoop
    torch = kf.torch
    cases = [K.case("loop", "B", s) for s in K.LOOP_SEEDS]
    S, steps, dense = len(cases), K.LOOP_STEPS, K.LOOP_DENSE_STREAM
    z = np.stack([c["z"] for c in cases])
    kw = dict(zip(("dt", "process_noise", "measurement_noise"), K.B))
    fused = HotLoop(n_streams=S, window=1, kf_kw=kw, fused_step=True)
    stage = HotLoop(n_streams=S, window=1, kf_kw=kw, fused_step=False)
    assert fused.fused_step and not stage.fused_step
    for lp in (fused, stage):
        lp.reset()
        rec = lp.kf_state.cpu().numpy()
        rec[dense, 6:42] = cases[dense]["P0"].reshape(36)
        lp.kf_state.copy_(torch.as_tensor(rec))
    got = {id(fused): np.zeros((S, steps, 12)), id(stage): np.zeros((S, steps, 12))}
    plans = np.zeros((S, steps, 4))
    for t in range(steps):
        for lp in (fused, stage):
            lp.load_measurements(z[:, t:t + 1])
            lp.step(graph=False)
            lp.synchronize()
            got[id(lp)][:, t] = lp.vstate.cpu().numpy()[:, 0]
        plans[:, t] = fused.plan_state.cpu().numpy()[:, 0]
        if t % 10 == 0 or t > steps - 3:
            _same(_outputs(fused), _outputs(stage), "step %d" % t)
    assert np.array_equal(got[id(fused)].view(np.uint64), got[id(stage)].view(np.uint64))
    st = fused.kf_state.cpu().numpy()
    assert st[:, 45].tolist() == [1.0 if s == dense else 0.0 for s in range(S)]
    worst = Worst()
    for s, c in enumerate(cases):
        _against_oracle(worst, got[id(fused)], plans, st, s, c, DENSE if s == dense else AXIS, "fused step, setting B")
    worst.report("fused step, setting B")


def test_vehicle_state_estimator_with_non_default_settings(estimator):
    from oracle.kf_ref import KalmanRef
    c = K.case("class", "B", K.CLASS_SEED)
    dt, q, r = K.B
    est = estimator(dt=dt, process_noise=q, measurement_noise=r)
    got = _drive(est, c["z"], c["mode"])
    worst = Worst()
    worst.close(got, c["want"], AXIS["state"], "class: states")
    worst.close(est.kf.x, c["rec"][:6], AXIS["x"], "class: x")
    worst.close(est.kf.P.reshape(36), c["rec"][6:42], AXIS["P"], "class: P")
    worst.close([est.prev_heading, est.prev_speed, est.time], c["rec"][42:45], AXIS["state"], "class: carries")
    assert len(est.state_history) == K.CLASS_W                 # predict() alone does not append
    assert np.array_equal(est.kf.Q, KalmanRef(*K.B).Q) and np.array_equal(est.kf.R, KalmanRef(*K.B).R)
    assert np.array_equal(est.kf.F, KalmanRef(*K.B).F)
    # a step whose heading wraps from just under +pi to just over -pi
    est.reset()
    ref = KalmanRef(*K.B)
    est.set_initial_state(*K.WRAP_INIT)
    ref.set_initial_state(*K.WRAP_INIT)
    assert est.prev_heading == ref.prev_heading and est.prev_speed == ref.prev_speed
    want = ref.step(K.WRAP_Z)
    st = est.step(K.WRAP_Z)
    assert st.heading < -3.0 and abs(st.yaw_rate) < 1.0
    from oracle.kf_ref import STATE_FIELDS
    worst.close([getattr(st, n) for n in STATE_FIELDS], want, AXIS["state"], "class: wrap step")
    worst.report("VehicleStateEstimator, setting B")
