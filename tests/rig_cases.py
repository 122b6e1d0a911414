"""The inputs of tests/test_gpu_rig.py, built once and shared with tests/test_rig_host.py, which pins their margins on the CPU.

case(name, ncol) -> dict(V, K, ocap_in, ncol, mounts [V][K][4], cam_obs [V*K][ocap_in][ncol], cam_n [V*K], plan_state [V][4],
cfg (merge_scale, merge_min), exact (hand-made in exact arithmetic: exempt from the margins), want (rig_ref.fuse_all's results))."""
import functools
import math

import numpy as np

from tests import rig_ref as rr

ID = rr.IDENTITY
QUARTER = (0.0, 1.0, 0.0, 0.0)          # yaw +90 degrees, written by hand: math.cos(pi / 2) is not 0
PLAN = [[3.0, -2.0, 0.4, 7.5], [-11.0, 4.0, -2.1, 0.0], [0.5, 0.25, 3.0, 12.0]]


def _rows(rows, ncol, seed=0):
    """(x, y, r) rows -> ncol columns, with velocities that differ per row."""
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    if ncol == 3:
        return rows
    v = np.random.default_rng(100 + seed).uniform(-6.0, 6.0, (len(rows), 2))
    return np.concatenate([rows, v], axis=1)


def _case(V, K, ocap_in, ncol, mounts, lists, cfg=(1.0, 1.0), exact=False, cam_n=None):
    obs, n = rr.pack(lists, ocap_in, ncol)
    if cam_n is not None:
        n = np.asarray(cam_n, np.int32)
    mounts = np.asarray(mounts, np.float64).reshape(V, K, 4)
    ps = np.asarray(PLAN[:V], np.float64)
    want = rr.fuse_all(obs, n, mounts, ps, *cfg)
    return dict(V=V, K=K, ocap_in=ocap_in, ncol=ncol, mounts=mounts, cam_obs=obs, cam_n=n, plan_state=ps, cfg=cfg, exact=exact, want=want)


def _passthrough(ncol):
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.uniform(2.0, 40.0, (9, 1)), rng.uniform(-15.0, 15.0, (9, 1)), rng.choice(rr.RADII, (9, 1))], axis=1)
    return _case(1, 1, 16, ncol, [[ID]], [_rows(rows, ncol)])


def _growth(ncol):
    # vehicle 0: the seed at 10 m takes camera 1's row at 10.9 and moves to about 10.4, so camera 2's row at 11.3 -- 1.3 m from the
    # seed, outside its 1 m gate -- joins.  vehicle 1, mirrored: the seed takes a row at 9.1 and moves AWAY from camera 2's row at
    # 10.9, which the seed would have taken (0.9 m) and the fused cluster does not (about 1.4 m)
    lists = [[[10.0, 0.0, 1.0]], [[10.9, 0.0, 0.75]], [[11.3, 0.0, 0.5]],
             [[10.0, 0.0, 1.0]], [[9.1, 0.0, 0.75]], [[10.9, 0.0, 0.5]]]
    return _case(2, 3, 4, ncol, [[ID] * 3] * 2, [_rows(l, ncol, i) for i, l in enumerate(lists)])


def _contest(ncol):
    # two rows of camera 1 inside the 1.5 m gate of camera 0's disc: the nearer (the second row) wins, the other founds a cluster
    lists = [[[10.0, 0.0, 1.5], [25.0, 6.0, 1.0]], [[10.5, 0.2, 1.0], [10.3, -0.1, 1.0], [25.2, 6.1, 0.5]]]
    return _case(1, 2, 8, ncol, [[ID, rr.mount(0.0, 0.0, 0.0)]], [_rows(l, ncol, i) for i, l in enumerate(lists)])


def _ties(ncol):
    # camera 0 (identity): clusters 0 .. 11.  camera 1 (a quarter turn: vehicle (X, Y) = (-y, x)) in integer coordinates:
    #   row 0 at (12, 0): 2 m from clusters 0 (10, 0) and 1 (14, 0), on the gate itself (r = 2) -> cluster 0 (the smallest i)
    #   rows 1, 2 at (31, 0), (29, 0): 1 m from cluster 2 (30, 0) -> row 1 (the smallest j), row 2 founds a cluster
    #   row 3 at (42, 0): 2 m from clusters 3 (40, 0) and 11 (44, 0), which share a slice of the kernel -> cluster 3
    c0 = [[10, 0, 2], [14, 0, 2], [30, 0, 2], [40, 0, 2]] + [[100 + 10 * t, 50, 1] for t in range(7)] + [[44, 0, 2]]
    c1 = [[0, -12, 1], [0, -31, 1], [0, -29, 1], [0, -42, 1]]
    return _case(1, 2, 16, ncol, [[ID, QUARTER]], [_rows(c0, ncol, 0), _rows(c1, ncol, 1)], exact=True)


def _empty(ncol):
    lists = [[], [[8.0, 1.0, 1.0], [20.0, -3.0, 2.0], [8.5, 1.2, 0.5]], [], [], [], []]
    return _case(2, 3, 4, ncol, [[ID, rr.mount(0.3, 1.0, 0.5), ID]] * 2, [_rows(l, ncol, i) for i, l in enumerate(lists)])


def _clamp(ncol):
    rng = np.random.default_rng(8)
    full = [np.concatenate([rng.uniform(3.0, 60.0, (8, 1)), rng.uniform(-20.0, 20.0, (8, 1)), rng.choice(rr.RADII, (8, 1))], axis=1)
            for _ in range(2)]
    return _case(1, 2, 8, ncol, [[ID, rr.mount(-0.2, 0.4, -0.3)]], [_rows(l, ncol, i) for i, l in enumerate(full)], cam_n=[-3, 13])


def _skipped(ncol):
    nan, inf = math.nan, math.inf
    c0 = _rows([[10, 1, 1], [nan, 2, 1], [12, inf, 1], [14, 3, 0], [16, 4, -1], [18, 5, nan], [20, 6, 2], [22, -inf, 1], [24, 7, inf]], ncol, 0)
    c1 = _rows([[10.2, 1.1, 1], [30, 1, 1], [20.3, 6.2, 1], [40, 0, 1]], ncol, 1)
    if ncol == 5:
        c1[1, 3], c1[3, 4] = nan, -inf
    return _case(1, 2, 16, ncol, [[ID, ID]], [c0, c1])


def _mounts8():
    return [rr.mount(2.0 * math.pi * k / 8.0 + 0.05, 1.2 * math.cos(2.0 * math.pi * k / 8.0), 0.8 * math.sin(2.0 * math.pi * k / 8.0))
            for k in range(8)]


FULL_SEEDS = {3: (41, 7), 5: (41, 7)}    # (scene, crowd): seeds at which both margins hold (asserted in tests/test_rig_host.py)


def _full(ncol):
    m8 = _mounts8()
    s_seed, c_seed = FULL_SEEDS[ncol]
    lists, _ = rr.scene(s_seed, m8, 60, ncol, noise=1.5e-4)
    lists = lists + rr.crowd(c_seed, 8, 64, ncol) + [[] for _ in range(8)]
    return _case(3, 8, 64, ncol, [m8, [ID] * 8, m8], lists)


def _coincident(ncol):
    # merge_scale = merge_min = 0: only coincident points merge.  Camera 1 is a quarter turn, integer coordinates: (3, -5) lands on
    # (5, 3) exactly, (4, -6) lands on (6, 4), one metre beside camera 0's (6, 3)
    return _case(1, 2, 4, ncol, [[ID, QUARTER]], [_rows([[5, 3, 1], [6, 3, 2]], ncol, 0), _rows([[3, -5, 2], [4, -6, 1]], ncol, 1)],
                 cfg=(0.0, 0.0), exact=True)


def _min_gate(ncol):
    # the gate is merge_min = 4 m whatever the radii (0.5 m): 3 m apart merges, 5 m apart does not
    lists = [[[10.0, 0.0, 0.5], [30.0, 0.0, 0.5]], [[13.0, 0.0, 0.5], [35.0, 0.0, 0.5]]]
    return _case(1, 2, 4, ncol, [[ID, ID]], [_rows(l, ncol, i) for i, l in enumerate(lists)], cfg=(1.0, 4.0))


BUILDERS = dict(passthrough=_passthrough, growth=_growth, contest=_contest, ties=_ties, empty=_empty, clamp=_clamp, skipped=_skipped,
                full=_full, coincident=_coincident, min_gate=_min_gate)
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name, ncol):
    return BUILDERS[name](ncol)


def permutation_scene(seed=11, ncol=5):
    """The 30-object, four-camera scene of the permutation property: (mounts, per-camera row lists)."""
    lists, _ = rr.scene(seed, rr.FOUR_MOUNTS, 30, ncol, noise=1.5e-4)
    return rr.FOUR_MOUNTS, lists
