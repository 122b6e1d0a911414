"""Cases for the lane planner (tests/laneplan_ref.py, csrc/laneplan.hip): plans of oracle.planner_ref.PlannerRef (wp, cost) -- 21
candidates of 51 waypoints, a straight reference path along the heading -- with hand-made boundary, lane, mark and side rows.

Every road case exists at two poses: (0, 0, 0, 9), where the vehicle-frame coordinates are exact and the comparison is bit for bit,
and NAME_p at POSE_P, where the device's sin / cos may differ in the last bits and every margin must be >= 1e-6.  The lines avoid
+-1.75 m and the speed avoids 10 m/s: the +-3.5 m candidates pass 1.75 m exactly at waypoint 25, and 10 m/s puts X on x_far."""
import functools

import numpy as np

from oracle.planner_ref import PlannerRef
from tests import laneplan_ref as ref
from tests import roadlanes_ref as lanes_ref
from tests.roadmarks_cases import bounds_of

U, S, D = ref.UNKNOWN, ref.SOLID, ref.DASHED
POSE_0, POSE_P = (0.0, 0.0, 0.0, 9.0), (12.0, -7.0, 0.3, 9.0)
OBSTACLE = (20.0, 0.0, 1.5)                 # in the vehicle frame
A_LINES, A_TYPES = (-5.1, -1.6, 1.9, 5.4), (S, S, D, S)


def to_world(pose, X, Y):
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return pose[0] + X * c - Y * s, pose[1] + X * s + Y * c


@functools.lru_cache(maxsize=None)
def plan(pose, obstacle, num_samples=7):
    """PlannerRef's plan from `pose` with a straight reference path along the heading and one obstacle (vehicle frame) or None."""
    p = PlannerRef(num_samples=num_samples)
    X = np.linspace(0.0, 60.0, 61)
    p.set_reference_path(np.stack(to_world(pose, X, np.zeros_like(X)), axis=1))
    obs = None
    if obstacle is not None:
        ox, oy = to_world(pose, obstacle[0], obstacle[1])
        obs = [(ox, oy, obstacle[2])]
    return p.plan(pose, obs)


def road(offsets, types, left=None, right=None, a1=0.0, a2=0.0, x_max=60.0, status=lanes_ref.LANE, own=None, side_types=None):
    """Boundaries Y = off + a1 X + a2 X^2 with their mark types; left / right: the indices of the ego lane's measured sides (flags
    LEFT / RIGHT) or None; own: (left a0, right a0) of the lane row when it is not the flagged boundaries'; side_types: the published
    (left, right) types when they are not the flagged boundaries'.  -> dict(bounds, lanes, marks, sides)."""
    flags = [(lanes_ref.BOUND_LEFT if i == left else 0) | (lanes_ref.BOUND_RIGHT if i == right else 0) for i in range(len(offsets))]
    bounds, lanes = bounds_of([(o, a1, a2) for o in offsets], flags=flags, x_max=x_max)
    marks, sides = np.zeros(ref.MAXB, ref.MARK_DTYPE), np.zeros((), ref.SIDES_DTYPE)
    marks["type"][:len(types)] = types
    lo = own[0] if own is not None else (offsets[left] if left is not None else None)
    ro = own[1] if own is not None else (offsets[right] if right is not None else None)
    lanes["status"] = status
    if status & lanes_ref.LANE:
        lanes["left"], lanes["right"] = (lo, a1, a2), (ro, a1, a2)
        lanes["centre"] = ((lo + ro) * 0.5, a1, a2)
        lanes["width"] = ro - lo
    st = side_types or (types[left] if left is not None else U, types[right] if right is not None else U)
    sides["left"]["type"], sides["right"]["type"] = st
    sides["left"]["bound"], sides["right"]["bound"] = (-1 if left is None else left), (-1 if right is None else right)
    return dict(bounds=bounds, lanes=lanes, marks=marks, sides=sides)


def case(name, pose, obstacle, rd, cfg=None, null_marks=False, **claims):
    p = plan(pose, obstacle)
    c = dict(name=name, pose=pose, cfg=ref.cfg_of(**(cfg or {})), plan_state=np.asarray(pose, np.float64), wp=p["wp"], cost=p["cost"],
             claims=claims, **rd)
    if null_marks:
        c["marks"] = c["sides"] = None
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    mirror = tuple(-o for o in reversed(A_LINES))
    solid_sides = road((-1.6, 1.9), (S, S), 0, 1)
    roads = dict(
        A=(OBSTACLE, road(A_LINES, A_TYPES, 1, 2), None, dict(best=18, maneuver=ref.RIGHT, delta=1, forced=False)),
        A_mirror=(OBSTACLE, road(mirror, tuple(reversed(A_TYPES)), 1, 2), None, dict(best=0, maneuver=ref.LEFT, delta=-1, forced=False)),
        B=(None, road(A_LINES, A_TYPES, 1, 2), None, dict(kept=True, free=(9, 10, 11), maneuver=ref.KEEP)),
        E=(None, road(A_LINES, A_TYPES, 1, 2, a1=0.01, a2=1.0 / 300.0), None, dict(kept=True, free=(9, 10, 11), follow=True)),
    )
    for pose, tag in ((POSE_0, ""), (POSE_P, "_p")):
        for name, (obs, rd, cfg, claims) in roads.items():
            out.append(case(name + tag, pose, obs, rd, cfg, **claims))
    out += [
        case("E_raw", POSE_0, None, road(A_LINES, A_TYPES, 1, 2, a1=0.01, a2=1.0 / 300.0), dict(follow=0), charged=(9,), follow=False),
        case("C", POSE_0, OBSTACLE, solid_sides, forced=True, solid=True),
        case("F", POSE_0, OBSTACLE, road((-1.6, 1.9), (U, U), 0, 1), forced=True, unknown=True),
        case("F_null", POSE_0, OBSTACLE, road((-1.6, 1.9), (S, D), 0, 1), null_marks=True, forced=True, unknown=True, same_as="F"),
        case("G", POSE_0, OBSTACLE, road(A_LINES, A_TYPES, 1, 2, x_max=12.0), all_free=True, n_lines=4),
        # the right side is the left one shifted by the width: no boundary carries RIGHT, the lane row's right side is line 1
        case("derived", POSE_0, OBSTACLE, road((-1.6,), (S,), 0, None, status=lanes_ref.LANE | lanes_ref.ONE_SIDED, own=(-1.6, 1.9),
                                               side_types=(S, U)), n_lines=2, sources=(0, ref.SRC_RIGHT)),
        # the left side coasts: its boundary was not measured, its type is still held
        case("coasting", POSE_0, OBSTACLE, road((1.9, 5.4), (D, S), None, 0, status=lanes_ref.LANE | lanes_ref.COAST_LEFT, own=(-1.6, 1.9),
                                                side_types=(S, D)), n_lines=3, sources=(0, 1, ref.SRC_LEFT), best=18),
        case("no_lane", POSE_0, OBSTACLE, road((-1.6, 1.9), (S, D), None, None, a1=0.01, status=lanes_ref.NO_VOTER), n_lines=2, follow=False),
        case("no_bounds", POSE_0, OBSTACLE, road((), (), None, None, status=0), n_lines=0, identity=True),
        case("eight", POSE_0, OBSTACLE, road((-8.6, -5.1, -1.6, 1.9, 5.4, 8.9, 12.4, 15.9), (S, S, S, D, S, S, U, D), 2, 3), n_lines=8, best=18),
    ]
    return out


def by_name(name):
    for c in cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def run(name):
    """The restatement on a case -> tests/laneplan_ref.step's result."""
    c = by_name(name)
    return ref.step(c["cfg"], c["plan_state"], c["wp"], c["cost"], c["bounds"], c["lanes"], c["marks"], c["sides"])


def exact(c):
    """Whether the case is compared bit for bit: the pose (0, 0, 0)."""
    return tuple(c["pose"][:3]) == (0.0, 0.0, 0.0)


def small(n_points):
    """C = 3 candidates of n_points (2 or 1) waypoints on road A: candidates 0, 9 and 18 of the plan, their start and their
    waypoint 30 (n = 2: the +-3.5 m candidates cross a line between the two) or waypoint 30 alone (n = 1: no pair, nothing crossed)."""
    c = dict(by_name("A"))
    pick = [0, 30] if n_points == 2 else [30]
    c["wp"], c["cost"] = np.ascontiguousarray(c["wp"][[0, 9, 18]][:, pick]), np.ascontiguousarray(c["cost"][[0, 9, 18]])
    c["name"] = "small%d" % n_points
    return c


def large(seed=5):
    """C = 192 straight-line candidates of n = 256 waypoints from a posed start, over road A's lines: the candidate tiling."""
    rng = np.random.default_rng(seed)
    c = dict(by_name("A_p"))
    C, n = ref.MAX_CAND, ref.MAX_POINTS
    X = np.linspace(0.0, 45.0, n)[None, :] * rng.uniform(0.6, 1.0, (C, 1))
    Y = rng.uniform(-4.0, 4.0, (C, 1)) + rng.uniform(-0.1, 0.1, (C, 1)) * X
    wp = np.zeros((C, n, 6))
    wp[..., 0], wp[..., 1] = to_world(c["pose"], X, Y)
    c["wp"], c["cost"], c["name"] = wp, rng.uniform(0.0, 2000.0, C), "large"
    return c
