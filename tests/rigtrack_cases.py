"""The sequences of tests/test_gpu_rigtrack.py, built once and shared with tests/test_rigtrack_host.py, which pins their margins
and what each of them shows on the CPU.

case(name, ncol) -> dict(V, tcap, ocap_in, ncol, cfg (rigtrack_ref.cfg), frames [(obs [V][ocap_in][ncol], n_in [V], views
[V][ocap_in] or None, plan_state [V][4])], exact (hand-made in exact arithmetic: exempt from the margins), want [V][frame]
(rigtrack_ref.run's free-running results))."""
import functools

import numpy as np

from tests import rigtrack_ref as tr

PLAN = np.array([[3.0, -2.0, 0.4, 7.5], [-11.0, 4.0, -2.1, 0.0], [0.5, 0.25, 3.0, 12.0]])
NAMES = ["handover", "contest", "ties", "life", "full", "skipped", "worst", "empty", "steady"]


def _plan(V, f):
    """The ego states of frame f: every vehicle moves a little each frame (only x0, y0 enter the tracker)."""
    ps = PLAN[:V].copy()
    ps[:, 0] += 0.25 * f
    ps[:, 1] -= 0.125 * f
    return ps


def _frame(V, ocap_in, ncol, f, lists, views=None, n_in=None):
    """Per-vehicle row lists (five columns, cut to ncol) -> one frame; NaN behind each list, -9 behind each views list."""
    obs = np.full((V, ocap_in, ncol), np.nan)
    n = np.zeros(V, np.int32)
    vw = None if views is None else np.full((V, ocap_in), -9, np.int32)
    for v, rows in enumerate(lists):
        rows = np.asarray(rows, np.float64).reshape(-1, 5)[:, :ncol]
        obs[v, :len(rows)] = rows
        n[v] = len(rows)
        if views is not None:
            vw[v, :len(rows)] = views[v]
    if n_in is not None:
        n = np.asarray(n_in, np.int32)
    return obs, n, vw, _plan(V, f)


def _case(V, tcap, ocap_in, ncol, frames, exact=False, **cfg):
    c = tr.cfg(**cfg)
    want = [tr.run([(o[v], n[v], None if w is None else w[v], p[v]) for o, n, w, p in frames], tcap, c) for v in range(V)]
    return dict(V=V, tcap=tcap, ocap_in=ocap_in, ncol=ncol, cfg=c, frames=frames, exact=exact, want=want)


HANDOVER_FRAMES, HANDOVER_GAP = 20, range(10, 15)


def _handover(ncol):
    # an object crossing in front of the vehicle from right to left at 6 m/s, 20 m ahead: camera 0 (views 0b01) sees it for ten
    # frames, nobody for five (between the two fields of view), camera 1 (views 0b10) from then on; a second object stands still,
    # seen by camera 0 throughout
    rng = np.random.default_rng(11)
    frames = []
    for f in range(HANDOVER_FRAMES):
        t = f / 30.0
        e = rng.normal(0.0, 0.02, 4)
        still = [40.0 + e[0], 8.0 + e[1], 1.5, 0.0, 0.0]
        if f in HANDOVER_GAP:
            frames.append(_frame(1, 2, ncol, f, [[still]], views=[[1]]))
            continue
        mover = [20.0 + e[2], -3.0 + 6.0 * t + e[3], 1.0, rng.normal(0.0, 0.05), 6.0 + rng.normal(0.0, 0.05)]
        frames.append(_frame(1, 2, ncol, f, [[still, mover]], views=[[1, 1 if f < 10 else 2]]))
    return _case(1, 2, 2, ncol, frames)


def _contest(ncol):
    # frame 0: tracks 1 .. 4 at (10, 0), (25, 6), (40, -5), (41.5, -5).  frame 1: rows 0 and 1 both inside track 1's gate, the
    # nearer (row 1) wins and row 0 founds track 5; row 3 lies between tracks 3 and 4, nearer to 4, so 3 coasts
    f0 = [[10.0, 0.0, 1.5, 0.5, 0.0], [25.0, 6.0, 1.0, 0.0, 1.0], [40.0, -5.0, 0.5, 0.0, 0.0], [41.5, -5.0, 0.5, 0.0, 0.0]]
    f1 = [[10.6, 0.3, 1.0, 0.5, 0.0], [10.3, -0.1, 1.0, 0.5, 0.0], [25.1, 6.05, 1.0, 0.0, 1.0], [40.9, -5.1, 0.5, 0.0, 0.0]]
    f2 = [[10.35, -0.1, 1.0, 0.5, 0.0], [40.05, -5.0, 0.5, 0.0, 0.0], [41.0, -5.1, 0.5, 0.0, 0.0], [10.7, 0.3, 1.0, 0.5, 0.0]]
    return _case(1, 64, 64, ncol, [_frame(1, 64, ncol, f, [rows]) for f, rows in enumerate((f0, f1, f2))], min_hits=1)


TIE_SLOTS = 140


def _ties(ncol):
    # dt = 1/32 and integer-valued coordinates (velocities multiples of 32): every position, distance and gate is exact.  frame 0
    # founds slot k = row k at (20 k, 0), r = 1, so every gate is 2 m and a distance of 2 m lies on it.  frame 1, relative to the
    # predicted places p_k (p_k = 20 k without velocities):
    #   row 0   at p_10 + (0, 2)                  one row, one slot, on the gate: taken
    #   slots 20 and 21 are founded 4 m apart (frame 0 rows 20, 21 at (400, 0) and (404, 0)): row 2 at (402, 0) is 2 m from both
    #           -> slot 20 (the smallest slot); row 3 at (398, 0) is 2 m from slot 20 only and loses it to row 2 (the smallest
    #           row would be 2 either way; the slot order decides first) -> born
    #   rows 4 and 5 at p_30 -+ (1, 0)            two rows of one wave 1 m from slot 30 -> row 4, row 5 born
    #   rows 6 and 100 at p_40 -+ (0, 1)          two rows of different waves 1 m from slot 40 -> row 6, row 100 born
    #   row 130 at p_50 + (1, 0), row 7 at p_50 - (1, 0)   the same with the smaller row in the later position -> row 7
    #   slots 60, 61 founded 4 m apart like 20, 21; row 131 halfway (2 m from both), row 8 2 m beyond slot 60 on the other side:
    #           (60, 8), (60, 131), (61, 131) all at d2 = 4 -> (60, 8) first (slot 60, the smaller row), then (61, 131)
    #   every other row k re-observes slot k exactly (d2 = 0: 120 and more equal distances, in every wave)
    vel = lambda k: (32.0 * (k % 3 - 1), 0.0) if ncol == 5 else (0.0, 0.0)          # noqa: E731
    base = np.array([[20.0 * k, 0.0] for k in range(TIE_SLOTS)])
    base[21] = base[20] + (4.0, 0.0)
    base[61] = base[60] + (4.0, 0.0)
    v = np.array([vel(k) for k in range(TIE_SLOTS)])
    v[21], v[61] = v[20], v[60]
    f0 = [[base[k, 0], base[k, 1], 1.0, v[k, 0], v[k, 1]] for k in range(TIE_SLOTS)]
    p = base + v / 32.0
    special = {0: p[10] + (0, 2), 2: p[20] + (2, 0), 3: p[20] - (2, 0), 4: p[30] - (1, 0), 5: p[30] + (1, 0), 6: p[40] - (0, 1),
               100: p[40] + (0, 1), 130: p[50] + (1, 0), 7: p[50] - (1, 0), 131: p[60] + (2, 0), 8: p[60] - (2, 0)}
    used = {10, 20, 21, 30, 40, 50, 60, 61}
    f1 = []
    for k in range(TIE_SLOTS):
        if k in special:
            f1.append([special[k][0], special[k][1], 1.0, 0.0, 0.0])
        elif k in used:
            f1.append([p[k, 0], p[k, 1] + 1000.0, 1.0, 0.0, 0.0])              # far from everything: born
        else:
            f1.append([p[k, 0], p[k, 1], 1.0, v[k, 0], v[k, 1]])
    frames = [_frame(1, 512, ncol, 0, [f0]), _frame(1, 512, ncol, 1, [f1]), _frame(1, 512, ncol, 2, [[]])]
    return _case(1, 512, 512, ncol, frames, exact=True, dt=1.0 / 32.0, min_hits=1)


LIFE = dict(max_age=2, min_hits=3)


def _life(ncol):
    # one slot, one row.  frames 0 .. 2: hits 1, 2, 3 -> confirmed in frame 2, not before.  frames 3 .. 5: no row -> misses 1, 2, 3;
    # 3 = max_age + 1 frees the slot in frame 5, where a row far away is born into it at once (frame 4's far row was dropped)
    a = lambda f: [12.0 + 0.1 * f, 1.0, 1.0, 3.0, 0.0]                            # noqa: E731
    far = [60.0, -20.0, 2.0, 0.0, 0.0]
    lists = [[a(0)], [a(1)], [a(2)], [], [far], [far], [far], [far]]
    return _case(1, 1, 1, ncol, [_frame(1, 1, ncol, f, [rows]) for f, rows in enumerate(lists)], **LIFE)


def _full(ncol):
    # two slots, five rows far apart: rows 2 .. 4 are dropped in frame 0; frame 1 re-observes rows 3, 0 (matched) and a new one
    # (dropped); frame 2 is empty.  vehicle 1 has room for its single row; vehicle 2 sees nothing
    rows = [[10.0 * k + 5.0, 2.0 * k, 1.0, 1.0, -1.0] for k in range(5)]
    near = lambda row, dx, dy: [row[0] + dx, row[1] + dy] + row[2:]               # noqa: E731
    f1 = [rows[3], near(rows[0], 0.25, 0.0), [90.0, 0.0, 1.0, 0.0, 0.0], near(rows[1], 0.0, -0.5)]
    one = [[7.0, 7.0, 0.5, 0.0, 0.0]]
    frames = [_frame(3, 65, ncol, 0, [rows, one, []]), _frame(3, 65, ncol, 1, [f1, one, []]), _frame(3, 65, ncol, 2, [[], [], []])]
    return _case(3, 2, 65, ncol, frames, min_hits=1)


def _skipped(ncol):
    # vehicle 0: rows that are not obstacles between rows that are; vehicle 1: a count beyond the list (clamped to 65 rows, all of
    # them good); vehicle 2: a negative count in front of good rows
    nan, inf = np.nan, np.inf
    good = lambda k: [8.0 * k + 3.0, -2.0 * k, 0.75, 0.5, 0.25]                   # noqa: E731
    bad = [[nan, 1.0, 1.0, 0.0, 0.0], [1.0, inf, 1.0, 0.0, 0.0], [1.0, 1.0, nan, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0, 0.0],
           [2.0, 2.0, -1.0, 0.0, 0.0], [3.0, 3.0, inf, 0.0, 0.0], [-inf, 3.0, 1.0, 0.0, 0.0],
           [100.0, 50.0, 1.0, nan, 0.0], [110.0, 50.0, 1.0, 0.0, -inf]]           # (the last two: kept with three columns)
    v0 = [good(0), bad[0], bad[1], good(1), bad[2], bad[3], bad[4], good(2), bad[5], bad[6], bad[7], good(3), bad[8]]
    v1 = [[6.0 * (k % 13), 6.0 * (k // 13), 0.5, 0.0, 0.0] for k in range(65)]
    v2 = [good(k) for k in range(4)]
    # (frame 1 sees every object a little further on, each by its own amount: no two distances are equal)
    moved = lambda rows: [[r[0] + 0.01 * (k + 1), r[1] - 0.005 * (k + 1)] + r[2:] for k, r in enumerate(rows)]      # noqa: E731
    frames = [_frame(3, 65, ncol, 0, [v0, v1, v2], n_in=[len(v0), 1000, -3]),
              _frame(3, 65, ncol, 1, [moved(v0), moved(v1), moved(v2)], n_in=[len(v0), 1000, -3])]
    return _case(3, 64, 65, ncol, frames, min_hits=1)


def _worst(ncol):
    # the matching loop's worst case: 512 tracks and 512 rows, every row inside every track's gate (r = 3: a 6 m gate around
    # points spread over 0.4 m)
    rng = np.random.default_rng(21)
    p = np.array([12.0, -1.0]) + rng.uniform(-0.2, 0.2, (512, 2))
    f0 = np.concatenate([p, np.full((512, 1), 3.0), rng.uniform(-1.0, 1.0, (512, 2))], axis=1)
    q = p[rng.permutation(512)] + rng.uniform(-0.05, 0.05, (512, 2))
    f1 = np.concatenate([q, np.full((512, 1), 3.0), rng.uniform(-1.0, 1.0, (512, 2))], axis=1)
    return _case(1, 512, 512, ncol, [_frame(1, 512, ncol, 0, [f0]), _frame(1, 512, ncol, 1, [f1])], min_hits=2)


def _empty(ncol):
    # vehicle 0 sees its objects in every frame; vehicle 1 for two frames and then nothing (predict, misses, death at max_age + 1);
    # vehicle 2 never sees anything
    rng = np.random.default_rng(31)
    objs = np.concatenate([rng.uniform(-30.0, 30.0, (20, 2)) + np.arange(20)[:, None] * (70.0, 0.0), np.full((20, 1), 1.0),
                           rng.uniform(-5.0, 5.0, (20, 2))], axis=1)
    frames = []
    for f in range(7):
        rows = objs.copy()
        rows[:, :2] += objs[:, 3:] * (f / 30.0) + rng.normal(0.0, 0.01, (20, 2))
        frames.append(_frame(3, 64, ncol, f, [rows, rows[:9] if f < 2 else [], []]))
    return _case(3, 65, 64, ncol, frames, max_age=3, min_hits=2)


def _steady(ncol):
    # three vehicles, objects on constant-velocity paths at least 9 m apart at all times (a grid with small velocities), seen with
    # noise in shuffled row order, each missing from a frame with probability 0.15; vehicle 0's list is full (64 rows)
    rng = np.random.default_rng(41)
    frames, V, counts = [], 3, (64, 40, 17)
    objs = []
    for nobj in counts:
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8)), axis=-1).reshape(-1, 2)[:nobj] * 12.0 - 40.0
        objs.append(np.concatenate([g, rng.choice([0.5, 1.0, 1.5, 2.5], (nobj, 1)), rng.uniform(-3.0, 3.0, (nobj, 2))], axis=1))
    for f in range(8):
        lists, views = [], []
        for v in range(V):
            o = objs[v].copy()
            o[:, :2] += o[:, 3:] * (f / 30.0) + rng.normal(0.0, 0.03, (len(o), 2))
            o[:, 3:] += rng.normal(0.0, 0.1, (len(o), 2))
            seen = rng.uniform(size=len(o)) >= (0.15 if v else 0.0)
            idx = rng.permutation(np.flatnonzero(seen))
            lists.append(o[idx])
            views.append(rng.integers(1, 16, len(idx)).astype(np.int32))
        frames.append(_frame(V, 64, ncol, f, lists, views=views))
    return _case(V, 64, 64, ncol, frames)


_BUILD = dict(handover=_handover, contest=_contest, ties=_ties, life=_life, full=_full, skipped=_skipped, worst=_worst, empty=_empty,
              steady=_steady)


@functools.lru_cache(maxsize=None)
def case(name, ncol):
    return _BUILD[name](ncol)


def straight_line(n_frames, ncol, speed=(4.0, -2.0), noise=0.02, seed=3):
    """One object on a straight line in the world frame, measured with noise: frames of one vehicle for rigtrack_ref.run."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n_frames):
        t = f / 30.0
        row = [15.0 + speed[0] * t + rng.normal(0.0, noise), 2.0 + speed[1] * t + rng.normal(0.0, noise), 1.0, 0.0, 0.0][:ncol]
        out.append((np.array([row]), 1, None, _plan(1, f)[0]))
    return out
