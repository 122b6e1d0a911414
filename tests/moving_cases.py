"""The inputs of tests/test_gpu_moving.py, shared with tests/test_moving_host.py, which proves on the CPU that they are
legitimate (no oracle distance within 1e-6 m of a branch boundary, both branches taken, motion changes the plan)."""
import numpy as np

from tests.moving_ref import MovingPlannerRef
from tests.test_gpu_plan_each import FRAMES, FULL, LOOP_CFG, LOOP_RADIUS, OFFSETS
from tests.test_gpu_planner import N_OF, OBS, POOL, U

MARGIN = 1e-6
FRAME_RATE = 30.0

# (n, num_samples, n_states): one shape per kernel of the dispatch, and the n = 1 edge
SHAPES = [(51, 7, 5), (151, 7, 3), (256, 64, 2), (51, 7, 513), (65, 2, 1025), (65, 1, 4097), (51, 7, 1025), (16, 64, 1024), (1, 7, 3)]
CONFIGS = sorted({(n, ns) for n, ns, _ in SHAPES})

# FULL (64 discs around the origin) with velocities of up to 12 m/s per axis
MFULL = np.concatenate([FULL, np.random.default_rng(12).uniform(-12.0, 12.0, (64, 2))], axis=1)
_zero = lambda l: np.concatenate([l, np.zeros((len(l), 2))], axis=1)
FAR_MOVER = np.array([[5000.0, -5000.0, 1.0, 3.0, -4.0]])
# list of state f: MLISTS[f % 5]
MLISTS = [np.zeros((0, 5)), _zero(OBS[:1]), _zero(OBS), MFULL, FAR_MOVER]

_PLANNERS, _PLANS = {}, {}


def planner(n, ns, path=None):
    """MovingPlannerRef of a configuration (with reference path `path`, keyed by its bytes), built once."""
    key = (n, ns, None if path is None or len(path) < 2 else path.tobytes())
    if key not in _PLANNERS:
        H, dt = N_OF[n]
        p = MovingPlannerRef(planning_horizon=H, dt=dt, num_samples=ns)
        assert p.n == n
        if key[2] is not None:
            p.set_reference_path(path)
        _PLANNERS[key] = p
    return _PLANNERS[key]


def oracle_wp(n, ns, state):
    """The oracle's waypoints [C, n, 6] of every candidate from `state` (they do not depend on lists or paths)."""
    key = (n, ns, tuple(state))
    if key not in _PLANS:
        p = planner(n, ns)
        _PLANS[key] = np.stack([p.generate(state, df, vt) for df in p.lat for vt in (8.0, 10.0, 12.0)])
    return _PLANS[key]
