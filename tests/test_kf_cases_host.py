"""Conditions on the inputs of tests/test_gpu_kf.py, proved on the CPU with the oracle alone (tests/kf_cases.py).

A GPU comparison at 1e-9 means something only if the device cannot legitimately take another branch than the oracle: every
decision of _extract_state (speed > 0.1, |dh| > pi, the side of atan2's branch cut) must sit further than 1e-6 from its
threshold in every sequence compared, and the sequences must really visit the paths the GPU tests are there for."""
import numpy as np
import pytest

from tests import kf_cases as K

ALL_PAIRS = {(a, b) for a in range(4) for b in range(4)}


@pytest.mark.parametrize("kind,cfg,seed", K.all_gpu_cases())
def test_no_decision_of_the_extract_is_within_1e6_of_its_threshold(kind, cfg, seed):
    m = K.case(kind, cfg, seed)["margins"]
    assert len(m["frame"]) >= len(K.case(kind, cfg, seed)["mode"])          # at least one extract per frame
    assert m["speed"].min() > K.MARGIN and m["dh"].min() > K.MARGIN and m["vy"].min() > K.MARGIN, \
        (m["speed"].min(), m["dh"].min(), m["vy"].min())


def test_run_oracle_is_the_step_sequence_of_the_reference_class():
    """run_oracle's four modes against KalmanRef's own step / predict / update, state for state."""
    from oracle.kf_ref import KalmanRef
    z, mode = K.kf_scenario(90, 3, K.B[0])
    got, m = K.run_oracle(z, mode, KalmanRef(*K.B))
    ref = KalmanRef(*K.B)
    n_extracts = 0
    for f in range(90):
        if mode[f] == 0:
            want = ref.predict()
        elif mode[f] == 1:
            want = ref.step(z[f])
        elif mode[f] == 2:
            want = ref.step(None)
        else:
            want = ref.update(z[f])
        n_extracts += 1 if mode[f] in (0, 3) else 2
        assert np.array_equal(got[f], want), f
    assert len(m["frame"]) == n_extracts
    assert set(mode.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("cfg", ["A", "B", "C"])
def test_mixed_sequences_visit_modes_standstill_and_wrap(cfg):
    cases = [K.case("mixed", cfg, s) for s in K.MIXED_SEEDS]
    wraps = []
    for c in cases:
        assert set(c["mode"].tolist()) == {0, 1, 2, 3}
        assert int(c["margins"]["held"].sum()) >= 50
        wraps.append(int(c["margins"]["wrapped"].sum()))
    # (seed 0 draws 0 m/s for the whole sequence at the slow settings, so not every single sequence wraps: the set does, and so
    # do the first three sequences, which the partition test takes)
    assert sum(w >= 5 for w in wraps) >= 2 and max(wraps[:3]) >= 5, wraps
    assert any(not K.held_frames(c).all() and K.held_frames(c).any() for c in cases[:3])


def test_mixed_sequences_visit_the_batch_carries():
    """Across the three settings of the mixed test, and already within the first three seeds (the partition test): a 64-frame
    batch without any giver (carry_h is handed through it) and a giver in the last lane of a batch before a held first lane.
    (Setting B follows the measurements closely, r = 0.04: the noise lifts the estimated speed over 0.1 every few frames, so its
    held runs stay short and it is the one that has giver | held edges; A and C smooth, and have the long held runs.)"""
    first3 = {cfg: [K.case("mixed", cfg, s) for s in K.MIXED_SEEDS[:3]] for cfg in "ABC"}
    assert any(K.whole_batch_held(c) and not K.held_frames(c).all() for c in first3["A"])
    assert any(K.whole_batch_held(c) and not K.held_frames(c).all() for c in first3["C"])
    assert any(K.giver_then_held_across_edge(c) for c in first3["B"])
    held_runs = []
    for c in first3["A"]:
        h, best, cur = K.held_frames(c), 0, 0
        for v in h:
            cur = cur + 1 if v else 0
            best = max(best, cur)
        held_runs.append(best)
    assert max(r for r in held_runs if r < K.MIXED_W) > K.KF_BATCH


def test_every_ordered_pair_of_modes_meets_at_a_batch_edge():
    pairs = set()
    for cfg in "ABC":
        for s in K.MIXED_SEEDS:
            pairs |= K.edge_mode_pairs(K.case("mixed", cfg, s))
    assert len(pairs) >= 12                                   # the i.i.d. modes of six sequences leave a few rare pairs out ...
    edges = K.case("edges", "B", 100)
    assert K.edge_mode_pairs(edges) == ALL_PAIRS              # ... the constructed sequence has all sixteen
    m = edges["margins"]
    assert int(m["wrapped"].sum()) >= 5 and int(m["held"].sum()) >= 50
    assert (0, 3) in K.edge_mode_pairs(K.case("steady", "B", 0))


@pytest.mark.parametrize("cfg", ["B", "D"])
def test_steady_scenario_repeats_its_covariance_before_every_disturbance(cfg):
    """The oracle's own covariance is bitwise constant over the 20 frames before each disturbance and moves on it (what the GPU
    test then shows of the device's), at least one disturbance lies inside a batch and one on a batch edge."""
    for s in K.STEADY_SEEDS:
        c = K.case("steady", cfg, s)
        unc = c["want"][:, 9:11]
        assert set(c["mode"].tolist()) == {0, 1, 2, 3}
        for f, ms in K.STEADY_DISTURBANCES.items():
            assert f >= 120 and (c["mode"][f - 120:f] == 1).sum() >= 117
            assert (c["mode"][f - 20:f] == 1).all()
            assert (unc[f - 20:f] == unc[f - 1]).all() and (unc[f] != unc[f - 1]).all(), (s, f)
    d = sorted(K.STEADY_DISTURBANCES)
    assert any(0 < f % K.KF_BATCH < K.KF_BATCH - 1 and 0 < (f + len(K.STEADY_DISTURBANCES[f]) - 1) % K.KF_BATCH < K.KF_BATCH - 1
               for f in d)
    assert any(f % K.KF_BATCH == K.KF_BATCH - 1 for f in d)
    assert any(f % K.KF_BATCH == K.KF_BATCH - 1 and len(K.STEADY_DISTURBANCES[f]) == 2 for f in d)   # a pair across the edge


def test_the_other_cases_visit_what_they_are_for():
    for s in K.ZERO_DT_SEEDS:
        c = K.case("zero_dt", "Z", s)
        assert set(c["mode"].tolist()) == {0, 1, 2, 3}
        assert c["margins"]["wrapped"].sum() >= 5 and c["margins"]["held"].sum() >= 50
        assert (c["want"][:, 6:8] == 0.0).all()
    for s in K.NULL_Z_SEEDS:
        c = K.case("null_z", "B", s)
        assert set(c["mode"][K.NULL_Z_HEAD:].tolist()) == {0, 2} and set(c["mode"][:K.NULL_Z_HEAD].tolist()) == {0, 1, 2, 3}
    for cfg in "AB":
        wraps = held = 0
        for s in K.DENSE_STREAMS:
            c = K.case("dense", cfg, s)
            assert set(c["mode"].tolist()) == {0, 1, 2, 3}
            assert not np.array_equal(c["P0"], np.eye(6) * 10)
            wraps += int(c["margins"]["wrapped"].sum())
            held += int(c["margins"]["held"].sum())
        assert wraps >= 5 and held >= 50
    assert sorted(K.DENSE_STREAMS) == [0, 63, 64, 66] and K.DENSE_S == 67      # both blocks of kf_kernel, and its bounds guard
    c = K.case("separable", "A", K.SEPARABLE_SEED)
    P0 = c["P0"]
    assert all(P0[r, c2] == 0 for r in range(6) for c2 in range(6) if (r ^ c2) & 1) and not np.array_equal(P0, P0.T)
    assert c["margins"]["wrapped"].sum() >= 1
    loop = [K.case("loop", "B", s) for s in K.LOOP_SEEDS]
    assert all(cc["margins"]["wrapped"].sum() >= 1 and cc["margins"]["held"].sum() >= 50 for cc in loop)
    assert loop[K.LOOP_DENSE_STREAM]["P0"][0, 1] == 0.25
    cl = K.case("class", "B", K.CLASS_SEED)
    assert set(cl["mode"].tolist()) == {0, 1, 2, 3} and cl["margins"]["wrapped"].sum() >= 1 and cl["margins"]["held"].sum() >= 5


def test_the_wrap_step_wraps():
    from oracle.kf_ref import KalmanRef
    ref = KalmanRef(*K.B)
    ref.set_initial_state(*K.WRAP_INIT)
    assert np.pi - 1e-3 < ref.prev_heading < np.pi
    want, m = K.run_oracle(K.WRAP_Z[None], np.array([1], np.uint8), ref)
    assert m["wrapped"].any() and K.min_margin(m) > K.MARGIN
    assert want[0, 4] < -3.0 and abs(want[0, 7]) < 1.0                  # heading just above -pi; the yaw rate is the small wrapped one
