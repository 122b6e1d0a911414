"""CPU-only checks of the per-track Kalman filter: the ABI of av_track_filter_* / av_track_obstacles_filtered, the NumPy
restatement (tests/track_filter_ref.py) against a track computed by hand and against an independent per-axis scalar form, what
the filter buys over the last centre difference, and the conditions on the inputs of tests/test_gpu_track_filter.py, proved with
the oracles and the restatement alone (the precedent: tests/test_moving_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
from tests import moving_cases as M
from tests.moving_ref import MovingPlannerRef, margin_and_allowance
from tests.track_filter_ref import (DEFAULT_FILTER, TrackFilterRef, filtered_scenario, hand_table, oracle_tables,
                                    track_obstacles_filtered)

NEW = ("av_track_filter_state_bytes", "av_track_filter_reset", "av_track_filter_update", "av_track_obstacles_filtered")
ROW = np.dtype(nat.TRACK_ROW_FIELDS)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nat.lib()


# ---- (1) exports and null arguments ----------------------------------------------------------------------------------------------

def test_exports_and_cfg_layout(lib):
    assert C.sizeof(nat.TrackFilterCfg) == 32
    for name in NEW:
        assert name in nat.declared_symbols() and hasattr(lib, name)
        assert name in {s[0] for s in nat._SIGS}
    assert lib.av_version() == 103
    assert lib.av_track_filter_state_bytes(0) == 0 and lib.av_track_filter_state_bytes(-64) == 0
    sizes = [lib.av_track_filter_state_bytes(t) for t in (64, 128, 1024)]
    assert sizes[0] > 0 and sizes[0] < sizes[1] < sizes[2]
    assert sizes[0] == nat.TRACK_FILTER_HDR_BYTES + 64 * np.dtype(nat.TRACK_FILTER_SLOT_FIELDS).itemsize
    assert np.dtype(nat.TRACK_FILTER_SLOT_FIELDS).itemsize == 64


def test_argument_validation_without_gpu(lib):
    cfg = nat.TrackFilterCfg(**DEFAULT_FILTER)
    assert lib.av_track_filter_reset(None, None, 1, 64, None) == -1
    assert lib.av_track_filter_update(None, None, None, 1, 1, 64, None, None, None, None) == -1
    assert lib.av_track_filter_update(None, None, C.byref(cfg), 1, 1, 64, None, None, None, None) == -1
    assert lib.av_track_obstacles_filtered(None, None, None, 30.0, 1, 64, None, None, None, None, 64, None, None) == -1
    assert b"null argument" in lib.av_last_error_string()


def test_python_cfg_ranges():
    from multimodal_autonomous_driving_perception_and_planning_amd.tracking.track_filter import filter_cfg
    c = filter_cfg()
    assert (c.q_accel, c.r_meas, c.p0_pos, c.p0_vel) == (1.0, 4.0, 4.0, 100.0)
    assert filter_cfg(q_accel=0.0, p0_pos=0.0, p0_vel=0.0).q_accel == 0.0
    for bad in (dict(q_accel=-1.0), dict(r_meas=0.0), dict(r_meas=-4.0), dict(p0_pos=-1.0), dict(p0_vel=float("inf")),
                dict(q_accel=float("nan")), dict(gain=1.0)):
        with pytest.raises(ValueError):
            filter_cfg(**bad)


# ---- (2) the restatement on its own ------------------------------------------------------------------------------------------------

def _table(frames, tcap=64):
    return hand_table(frames, tcap, ROW)


def test_restatement_against_a_hand_computed_track():
    """Birth at (100, 50), a match at (103, 48), a miss; q = 1, r = 4, p0 = (4, 100), all by hand per axis.
    Birth: x = (100, 50, 0, 0), P = diag(4, 4, 100, 100); the newborn row has misses == 0, so the update follows with innovation
    0: per axis S = 8, K = (1/2, 0), P = [[2, 0], [0, 100]] -> sigma (sqrt 4, sqrt 200).
    Predict: per axis P = [[2 + 100 + 1/4, 100 + 1/2], [100 + 1/2, 101]] = [[102.25, 100.5], [100.5, 101]], x = (100, 50, 0, 0).
    Update: S = 106.25, K = (102.25, 100.5) / 106.25; innovation (3, -2)."""
    rows, n = _table([[(7, 5, 200, 100, 0)], [(7, 5, 206, 96, 0)], [(7, 5, 206, 96, 1)]])
    got = TrackFilterRef(64).update(rows, n)
    assert np.isnan(got[:, 1:]).all()
    np.testing.assert_allclose(got[0, 0], [100, 50, 0, 0, 2.0, np.sqrt(200.0)], rtol=1e-15)
    k0, k1 = 102.25 / 106.25, 100.5 / 106.25
    ppp, ppv, pvv = 102.25 - k0 * 102.25, 100.5 - k0 * 100.5, 101.0 - k1 * 100.5
    want1 = [100 + 3 * k0, 50 - 2 * k0, 3 * k1, -2 * k1, np.sqrt(2 * ppp), np.sqrt(2 * pvv)]
    np.testing.assert_allclose(got[1, 0], want1, rtol=1e-12)
    # the miss: prediction only
    want2 = [want1[0] + want1[2], want1[1] + want1[3], want1[2], want1[3], np.sqrt(2 * (ppp + 2 * ppv + pvv + 0.25)), np.sqrt(2 * (pvv + 1.0))]
    np.testing.assert_allclose(got[2, 0], want2, rtol=1e-12)


def _scalar_axis(zs, hits, q, r, p0, pv):
    """One axis on its own with scalars and the plain (not Joseph) covariance update: -> [(c, v, ppp, pvv)] per frame."""
    out, c, v, a, b, d = [], None, 0.0, 0.0, 0.0, 0.0
    for z, hit in zip(zs, hits):
        if c is None:
            c, v, a, b, d = z, 0.0, p0, 0.0, pv
        else:
            c, a, b, d = c + v, a + 2 * b + d + q / 4, b + d + q / 2, d + q
        if hit:
            s = a + r
            k0, k1 = a / s, b / s
            y = z - c
            c, v = c + k0 * y, v + k1 * y
            a, b, d = a - k0 * a, b - k0 * b, d - k1 * b
        out.append((c, v, a, d))
    return out


@pytest.mark.parametrize("cfg", [DEFAULT_FILTER, dict(q_accel=0.25, r_meas=9.0, p0_pos=1.0, p0_vel=25.0),
                                 dict(q_accel=0.0, r_meas=1.0, p0_pos=0.0, p0_vel=0.0)], ids=["default", "other", "zeros"])
def test_general_matrices_against_a_per_axis_scalar_form(cfg):
    rng = np.random.default_rng(3)
    W = 40
    hits = rng.random(W) < 0.7
    hits[0] = True
    cx2 = (2 * (300 + 4.5 * np.arange(W)) + rng.integers(-6, 7, W)).astype(int)
    cy2 = (2 * (200 - 2.0 * np.arange(W)) + rng.integers(-6, 7, W)).astype(int)
    misses = np.where(hits, 0, 1)
    bank = TrackFilterRef(64, **cfg)
    got = np.stack([bank.frame(*[a[0] for a in _table([[(3, 9, int(cx2[f]), int(cy2[f]), int(misses[f]))]])])[0] for f in range(W)])
    ax = _scalar_axis(cx2 / 2.0, hits, cfg["q_accel"], cfg["r_meas"], cfg["p0_pos"], cfg["p0_vel"])
    ay = _scalar_axis(cy2 / 2.0, hits, cfg["q_accel"], cfg["r_meas"], cfg["p0_pos"], cfg["p0_vel"])
    want = np.array([(x[0], y[0], x[1], y[1], np.sqrt(x[2] + y[2]), np.sqrt(x[3] + y[3])) for x, y in zip(ax, ay)])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    P = bank.P[9]
    assert np.array_equal(P, P.T) or np.abs(P - P.T).max() <= 1e-13 * np.abs(P).max()
    assert P[0, 1] == 0 and P[0, 3] == 0 and P[1, 2] == 0 and P[2, 3] == 0          # x and y never mix


def test_covariance_converges_without_misses_and_grows_with_them():
    W = 60
    rows, n = _table([[(1, 0, 400 + 6 * f, 300, 0)] for f in range(W)])
    got = TrackFilterRef(64).update(rows, n)
    assert abs(got[-1, 0, 4] - got[-2, 0, 4]) < 1e-9 and abs(got[-1, 0, 5] - got[-2, 0, 5]) < 1e-9
    # the steady state: a posterior position variance below the measurement's (sigma < sqrt(2 r)), a velocity far better known than at birth
    assert got[-1, 0, 4] < np.sqrt(2 * 4.0) and got[-1, 0, 5] < 0.2 * got[0, 0, 5]
    rows, n = _table([[(1, 0, 400 + 6 * f, 300, 0 if f < 20 else f - 19)] for f in range(30)])
    got = TrackFilterRef(64).update(rows, n)
    assert (np.diff(got[19:, 0, 4]) > 0).all() and (np.diff(got[19:, 0, 5]) > 0).all()
    np.testing.assert_allclose(got[29, 0, 2:4], got[19, 0, 2:4], rtol=0, atol=0)      # the velocity is carried, the centre moves with it
    np.testing.assert_allclose(got[29, 0, 0], got[19, 0, 0] + 10 * got[19, 0, 2], rtol=1e-13)


# ---- (3) it matters ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gap", [1, 3, 6])
def test_velocity_after_a_gap_is_closer_to_the_truth_than_the_last_difference(gap):
    """A track moving at (4.3, -2.6) px/frame with integer-rounded centres, matched for 12 frames, missed for `gap`, matched again:
    Track.velocity at the re-match is the displacement over gap + 1 frames."""
    v = np.array([4.3, -2.6])
    frames, prev, last_diff = [], None, None
    for f in range(12 + gap + 1):
        c = np.round(np.array([300.0, 400.0]) + v * f).astype(int)
        hit = f < 12 or f == 12 + gap
        if hit:
            last_diff, prev = (None if prev is None else c - prev), c
        frames.append([(1, 2, int(2 * prev[0]), int(2 * prev[1]), 0 if hit else f - 11)])
    rows, n = _table(frames)
    got = TrackFilterRef(64).update(rows, n)[-1, 0, 2:4]
    err_f, err_d = np.linalg.norm(got - v), np.linalg.norm(last_diff - v)
    print("gap %d: filtered velocity off by %.3f px/frame, last difference by %.3f" % (gap, err_f, err_d))
    assert err_f < err_d and err_f < 1.0 and err_d > gap * 4.0


@pytest.fixture(scope="module")
def long_tables():
    return [oracle_tables(ROW, off, 120) for off in M.OFFSETS]


def test_filtered_velocity_is_steadier_than_the_last_difference_on_the_loop_scenario(long_tables):
    """Per track with at least 10 matched frames, over its matched frames from the second on: the standard deviation of the
    filtered velocity is below that of row.vx, row.vy, per axis.  The figures are DESIGN 7l's."""
    tracks = 0
    for s, (rows, n, _) in enumerate(long_tables):
        filt = TrackFilterRef(64).update(rows, n)
        per = {}
        for f in range(len(n)):
            for i in range(n[f]):
                r = rows[f, i]
                if r["misses"] == 0 and r["hist_len"] >= 2:
                    per.setdefault(int(r["id"]), []).append((r["vx"], r["vy"], filt[f, i, 2], filt[f, i, 3]))
        for tid, v in sorted(per.items()):
            if len(v) + 1 < 10:
                continue
            sd = np.std(np.asarray(v, np.float64), axis=0)
            print("stream %d track %d, %d matches: last difference sd (%.2f, %.2f), filtered (%.2f, %.2f) px/frame" % ((s, tid, len(v) + 1) + tuple(sd)))
            assert sd[2] < sd[0] and sd[3] < sd[1], (s, tid, sd)
            tracks += 1
    assert tracks >= 3


# ---- (4) the GPU tests' inputs are legitimate --------------------------------------------------------------------------------------

@pytest.mark.parametrize("tracker_kw,deaths", [(None, False), (dict(max_age=3), True)], ids=["default", "max_age3"])
def test_filtered_scenario_stays_1e6_from_the_branch_boundaries(tracker_kw, deaths):
    scenario, died = filtered_scenario(ROW, M.OFFSETS, M.FRAMES, M.LOOP_CFG, M.FRAME_RATE, tracker_kw)
    p = MovingPlannerRef()
    worst, hard, soft, total, coasting = np.inf, 0, 0, 0, 0
    for s, per in enumerate(scenario):
        assert len(per) == M.FRAMES
        for f, (ps, obs5, rows, n, filt) in enumerate(per):
            assert np.isfinite(filt[:n]).all() and np.isnan(filt[n:]).all()
            want = p.plan(ps, obs5)
            margin, _, h, so = margin_and_allowance(want["wp"], obs5)
            assert margin >= M.MARGIN, "stream %d frame %d: %g m from a branch boundary" % (s, f, margin)
            worst, hard, soft, total = min(worst, margin), hard + h, soft + so, total + len(obs5)
            live = rows[:n]
            coasting += int((((live["flags"] & 1) == 1) & (live["misses"] > 0)).sum())
    print("margin %.3g m, %d obstacle rows (%d of coasting tracks), %d track deaths, %d hard and %d soft pairs" % (worst, total, coasting,
                                                                                                                 died, hard, soft))
    assert hard >= 1 and soft >= 1 and total > 0 and coasting > 0
    assert (died > 0) == deaths


def test_filtered_obstacles_follow_the_filter():
    """A coasting track's disc sits where the filter predicts it: the restatement with the rows' own centre and velocity is
    track_obstacles_moving, and with a shifted filter row the disc moves by the shift in the road plane."""
    from tests.moving_ref import track_obstacles_moving
    rows, n = _table([[(1, 0, 840, 400, 4), (2, 1, 500, 300, 0)]])
    rows["vx"], rows["vy"] = [[1.5, -2.0] + [0.0] * 62], [[-0.5, 3.0] + [0.0] * 62]
    ps = (1.0, 2.0, 0.3, 9.0)
    own = np.zeros((64, 6))
    own[:2, 0], own[:2, 1], own[:2, 2], own[:2, 3] = [420.0, 250.0], [200.0, 150.0], [1.5, -2.0], [-0.5, 3.0]
    a = track_obstacles_filtered(rows[0], 2, own, ps, None, 30.0)
    assert np.array_equal(a, track_obstacles_moving(rows[0], 2, ps, None, 30.0))
    own[0, 1] -= 40.0                                    # 40 px up the image: 4 m further ahead
    b = track_obstacles_filtered(rows[0], 2, own, ps, None, 30.0)
    np.testing.assert_allclose(b[0, :2] - a[0, :2], [4.0 * np.cos(0.3), 4.0 * np.sin(0.3)], atol=1e-12)
    assert np.array_equal(b[1], a[1]) and np.array_equal(b[:, 2:], a[:, 2:])
