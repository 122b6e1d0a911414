"""The cases of the rig-odometry tests, shared by tests/test_rigflow_host.py (the NumPy reference against known motion) and
tests/test_gpu_rigflow.py (the device against the reference): mount sets, rendered patches of a rig and hand-made tile tables.

A mount is (c, s, mx, my), av_rig_mount's fields; quarter turns are written exactly."""
import numpy as np

from tests import egoflow_cases as ego
from tests import egoflow_ref as ref

f8 = np.float64

C55, S55 = float(np.cos(np.deg2rad(55.0))), float(np.sin(np.deg2rad(55.0)))
IDENTITY = [(1.0, 0.0, 0.0, 0.0)]
# front, left, rear, right: yaw 0, 90, 180 and -90 degrees
MOUNTS_4 = [(1.0, 0.0, 2.0, 0.0), (0.0, 1.0, 0.5, 0.9), (-1.0, 0.0, -1.0, 0.0), (0.0, -1.0, 0.5, -0.9)]
MOUNTS_4_ARMS = [(1.0, 0.0, 2.0, 0.0), (0.0, 1.0, 0.0, 2.0), (-1.0, 0.0, -2.0, 0.0), (0.0, -1.0, 0.0, -2.0)]      # 2 m lever arms
MOUNTS_3 = [(1.0, 0.0, 1.8, 0.0), (C55, S55, 0.9, 0.6), (-1.0, 0.0, -1.0, 0.0)]                                 # one oblique mount
MOUNTS_8 = MOUNTS_4 + [(C55, S55, 1.5, 0.8), (C55, -S55, 1.5, -0.8), (-C55, S55, -0.8, 0.8), (-C55, -S55, -0.8, -0.8)]
RIG_MOTIONS = ego.KNOWN_MOTIONS + [(0.3, 0.0, 0.03)]
COVERED_ROAD = (-0.3, 0.2, 0.0)         # what the covered camera sees instead of the road moves by this under it (another
                                        # vehicle's deck): the patches of a camera that itself moves by the opposite
COVERED_FLOW = (0.3, 0.25, 0.0)         # the same for the hand-made tables: five pixels from the rear camera's own flow


def camera_pose(pose, mount):
    """The pose (x, y, psi) of a camera's ground point from the vehicle's pose and the camera's mount."""
    x, y, psi = pose
    c, s, mx, my = mount
    return (x + mx * np.cos(psi) - my * np.sin(psi), y + mx * np.sin(psi) + my * np.cos(psi), psi + np.arctan2(s, c))


def camera_motion(motion, mount):
    """The small-angle motion (t_f, t_l, omega) of a camera's ground point in its own road frame when the vehicle's origin moves
    by (T_f, T_l, Omega) in the vehicle frame: t = R^T (T + Omega J M), omega = Omega."""
    Tf, Tl, Om = motion
    c, s, mx, my = mount
    a, b = Tf - Om * my, Tl + Om * mx
    return (c * a + s * b, c * b - s * a, Om)


def rig_patch_pairs(motion, mounts, c=ego.KNOWN_CFG, pose=(3.0, -2.0, 0.3)):
    """-> [(prev, cur)] per camera: the patches before and after the VEHICLE at `pose` moves by `motion` in its own frame."""
    after = ego.compose(pose, motion)
    return [(ego.render_patch(camera_pose(pose, mt), c), ego.render_patch(camera_pose(after, mt), c)) for mt in mounts]


def rig_tables(motion, mounts, c=ego.KNOWN_CFG, covered=None):
    """-> the K tile tables the reference's match makes of rig_patch_pairs; camera `covered` sees a surface moving by COVERED_ROAD instead."""
    ones = np.ones((c["gh"], c["gw"]), bool)
    pairs = rig_patch_pairs(motion, mounts, c)
    if covered is not None:
        pairs[covered] = ego.patch_pair(tuple(-v for v in COVERED_ROAD), c, pose=(40.0, 17.0, 1.1))
    return [ref.match(cur, prev, ones, c) for prev, cur in pairs]


def keep_accepted(table, keep):
    """The table with the accepted bit on `keep` of its accepted tiles only (spread over the grid), the others merely live."""
    t = table.copy()
    acc = np.nonzero(t["flags"] & ref.ACCEPTED)[0]
    drop = np.setdiff1d(acc, acc[np.linspace(0, len(acc) - 1, keep).round().astype(int)])
    t["flags"][drop] &= ~ref.ACCEPTED
    return t


# ---- hand-made tile tables for the rig solve (SOLVE_CFG: 240 tiles) -----------------------------------------------------------------
def _tables(motion, mounts, rng, **kw):
    return [ego._flow_table(ego.SOLVE_CFG, camera_motion(motion, mt), rng, **kw) for mt in mounts]


def _none(c=ego.SOLVE_CFG):
    t = ego._grid_table(c)
    t["flags"] = ref.LIVE
    return t


def solve_cases():
    """-> list of dict(name, mounts [K][4], tables [K][240], top): `top` is the set of hypotheses the case builds to share the
    largest count (every hypothesis that explains all the road rows does), None where no hypothesis is regular."""
    rng = np.random.default_rng(11)
    out = []

    def case(name, mounts, tables, top):
        out.append(dict(name=name, mounts=np.array(mounts, f8), tables=tables, top=top))

    case("straight", MOUNTS_4, _tables((0.21, 0.0, 0.0), MOUNTS_4, rng, outliers=9, drop=0.2), {0, 1, 2, 3, 4})
    case("turn_arms", MOUNTS_4_ARMS, _tables((0.17, 0.02, 0.012), MOUNTS_4_ARMS, rng, outliers=12, drop=0.3), {0, 1, 2, 3, 4})
    t = _tables((0.15, -0.02, -0.01), MOUNTS_4, rng, outliers=6)
    t[1] = _none()                                                  # a camera with nothing accepted: its hypothesis is dropped
    case("blind_camera", MOUNTS_4, t, {0, 1, 3, 4})
    t = [keep_accepted(x, 5) for x in _tables((0.2, 0.01, 0.008), MOUNTS_4, rng)]
    case("sparse", MOUNTS_4, t, {0, 1, 2, 3, 4})                    # five tiles per camera: each alone is below min_inliers
    t = _tables((0.2, 0.0, 0.01), MOUNTS_4, rng, outliers=4)
    t[2] = ego._flow_table(ego.SOLVE_CFG, COVERED_FLOW, rng)      # the rear camera's whole patch shows another vehicle
    case("covered", MOUNTS_4, t, {1, 2, 4})
    case("none_accepted", MOUNTS_4, [_none() for _ in range(4)], None)
    t = [_none() for _ in range(4)]
    t[3] = ego._flow_table(ego.SOLVE_CFG, (0.1, 0.0, 0.0), rng)     # one gated tile in all: every fit is singular
    t[3]["flags"][:17] = ref.LIVE
    t[3]["flags"][18:] = ref.LIVE
    case("singular", MOUNTS_4, t, None)
    case("oblique", MOUNTS_3, _tables((0.18, 0.03, 0.011), MOUNTS_3, rng, outliers=10, drop=0.25), {0, 1, 2, 3})
    case("oblique_reverse", MOUNTS_3, _tables((-0.12, -0.02, -0.015), MOUNTS_3, rng, outliers=5), {0, 1, 2, 3})
    case("eight", MOUNTS_8, _tables((0.16, 0.02, 0.009), MOUNTS_8, rng, outliers=8, drop=0.2), set(range(9)))
    case("eight_straight", MOUNTS_8, _tables((0.22, -0.01, 0.0), MOUNTS_8, rng, outliers=3), set(range(9)))
    return out


def identity_cases():
    """tests/egoflow_cases.py's solve cases as rigs of one camera under the identity mount: h_0 = h_1, a tie by construction."""
    return [dict(name=name, mounts=np.array(IDENTITY, f8), tables=[t], top=None if name in ("none_accepted", "singular") else {0, 1})
            for name, t in ego.solve_cases()]
