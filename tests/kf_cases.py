"""Inputs and the oracle driver of the Kalman tests (host only: NumPy and oracle/kf_ref.py).

tests/test_gpu_kf.py runs these sequences through av_kf_step; tests/test_kf_cases_host.py proves on the CPU, with the
oracle alone, that they visit what they are meant to visit (every mode, the heading hold, the +-pi wrap, the carries across
64-frame batches) and that no decision of the extract sits within 1e-6 of its threshold -- 1000 times the comparison
tolerance -- so that the device can never legitimately take another branch than the oracle.
"""
import functools

import numpy as np

from oracle.kf_ref import KalmanRef

# (dt, process_noise, measurement_noise)
A = (0.033, 0.1, 1.0)          # the default av_kf_cfg
B = (0.1, 0.5, 0.04)
C = (0.01, 0.02, 4.0)
D = (0.5, 2.0, 0.25)
Z = (0.0, 0.1, 1.0)            # dt = 0: acceleration and yaw rate are exactly 0
SETTINGS = {"A": A, "B": B, "C": C, "D": D, "Z": Z}

KF_BATCH = 64                  # frames per batch of the kernel's lane = frame extract (csrc/kf_dev.h)
MARGIN = 1e-6

_SPEEDS = (0.0, 0.0, 0.03, 3.0, 8.0)
_HEADINGS = (np.pi, -np.pi + 0.01, 3.0, -2.4, 0.7, np.pi - 0.005)


def kf_scenario(W, seed, dt):
    """(z [W, 4] float64, mode [W] uint8): a stop-and-go ego vehicle that mostly heads west.  Piecewise-constant profile in
    segments of 20..149 frames, speed from {0, 0, 0.03, 3, 8} m/s (three of five choices stay under the 0.1 m/s heading-hold
    threshold), heading from headings at and next to +-pi; positions integrated with dt; noise sigma 0.1 on positions and 0.05 on
    velocities (the 0.05 on vy is what flips atan2 between +pi and -pi while heading west); modes i.i.d. with
    P(0, 1, 2, 3) = (0.10, 0.60, 0.15, 0.15)."""
    rs = np.random.RandomState(seed)
    prof = []
    while len(prof) < W:
        n = rs.randint(20, 150)
        sp = rs.choice(_SPEEDS)
        hd = rs.choice(_HEADINGS)
        prof += [(sp, hd)] * n
    z = np.zeros((W, 4))
    x = y = 0.0
    for i in range(W):
        sp, hd = prof[i]
        vx, vy = sp * np.cos(hd), sp * np.sin(hd)
        x += vx * dt
        y += vy * dt
        z[i] = (x + rs.normal(0, 0.1), y + rs.normal(0, 0.1), vx + rs.normal(0, 0.05), vy + rs.normal(0, 0.05))
    mode = rs.choice([0, 1, 2, 3], size=W, p=[0.1, 0.6, 0.15, 0.15]).astype(np.uint8)
    return z, mode


# frames of kf_steady_scenario that are not mode 1: {first frame: modes}.  150 and 450..452 lie inside a batch, 319 | 320 are
# the last frame of one batch and the first of the next, 575 is the last frame of a batch; the gaps are >= 120 frames.
STEADY_DISTURBANCES = {150: (2,), 319: (0, 3), 450: (2, 2, 2), 575: (2,)}
STEADY_W = 700


def kf_steady_scenario(W, dt, seed=0):
    """(z, mode): 8 m/s on a constant heading, every frame predict + update (mode 1) except the isolated disturbances of
    STEADY_DISTURBANCES -- the covariance reaches its bitwise fixed point before each of them (settings B and D: after 57 and 14
    frames), so the kernel's steady loop is entered, left on the disturbance and entered again."""
    assert W >= max(STEADY_DISTURBANCES) + 100
    rs = np.random.RandomState(1000 + seed)
    hd, sp = 0.7, 8.0
    vx, vy = sp * np.cos(hd), sp * np.sin(hd)
    t = np.arange(1, W + 1) * dt
    z = np.stack([vx * t, vy * t, np.full(W, vx), np.full(W, vy)], axis=1)
    z += rs.normal(0, 1, (W, 4)) * np.array([0.1, 0.1, 0.05, 0.05])
    mode = np.ones(W, np.uint8)
    for f, ms in STEADY_DISTURBANCES.items():
        mode[f:f + len(ms)] = ms
    return z, mode


def edge_pairs_scenario(dt, seed=100):
    """(z, mode) of 17 batches: kf_scenario with the modes at the 16 batch edges (frames 64k+63 -> 64k+64) set to the 16
    ordered pairs of modes, so that every way of handing prev_heading / prev_speed across a batch edge occurs."""
    W = 17 * KF_BATCH
    z, mode = kf_scenario(W, seed, dt)
    for k in range(16):
        mode[KF_BATCH * k + KF_BATCH - 1], mode[KF_BATCH * k + KF_BATCH] = k // 4, k % 4
    return z, mode


def class_schedule(z):
    """The call pattern of tests/test_gpu_classes.py::test_vehicle_state_estimator as (z, mode) frames: step(None) when
    f % 7 == 3, predict() + update(z) when f % 11 == 5 (two frames with the same z), step(z) otherwise."""
    zz, mm = [], []
    for f in range(len(z)):
        if f % 7 == 3:
            zz.append(z[f]), mm.append(2)
        elif f % 11 == 5:
            zz.append(z[f]), mm.append(0)
            zz.append(z[f]), mm.append(3)
        else:
            zz.append(z[f]), mm.append(1)
    return np.array(zz), np.array(mm, np.uint8)


def run_oracle(z, mode, kf):
    """Drives a KalmanRef as include/avhot.h defines the modes -- 0: predict; 1: predict, update; 2: predict, _extract;
    3: update -- from the state `kf` is in.  Returns (states [W, 12], margins); margins holds one entry per _extract call:
      frame   the frame of the call
      speed   |speed - 0.1|                      (distance from the heading-hold threshold)
      dh      ||heading - prev_heading| - pi|    (distance from the wrap threshold)
      vy      |vy| where speed > 0.1 and vx < 0  (distance from atan2's branch cut), inf elsewhere
      wrapped |dh| > pi, held: speed <= 0.1."""
    z = None if z is None else np.asarray(z, np.float64)
    rec = []
    frame = [0]
    plain = kf._extract

    def probed():
        vx, vy = kf.x[2], kf.x[3]
        sp = np.sqrt(vx ** 2 + vy ** 2)
        hd = np.arctan2(vy, vx) if sp > 0.1 else kf.prev_heading
        dh = hd - kf.prev_heading
        rec.append((frame[0], abs(sp - 0.1), abs(abs(dh) - np.pi), abs(vy) if (sp > 0.1 and vx < 0) else np.inf,
                    abs(dh) > np.pi, sp <= 0.1))
        return plain()

    kf._extract = probed
    out = np.zeros((len(mode), 12))
    try:
        for f in range(len(mode)):
            frame[0] = f
            m = int(mode[f])
            if m == 0:
                st = kf.predict()
            elif m == 1:
                kf.predict()
                st = kf.update(z[f])
            elif m == 2:
                kf.predict()
                st = kf._extract()
            elif m == 3:
                st = kf.update(z[f])
            else:
                raise ValueError("mode %d" % m)
            out[f] = st
    finally:
        del kf._extract
    r = np.array(rec, np.float64).reshape(-1, 6)
    margins = dict(frame=r[:, 0].astype(np.int64), speed=r[:, 1], dh=r[:, 2], vy=r[:, 3], wrapped=r[:, 4] > 0, held=r[:, 5] > 0)
    return out, margins


def min_margin(m):
    return float(min(m["speed"].min(), m["dh"].min(), m["vy"].min()))


def final_record(kf):
    """The first 45 doubles of the device record a filter in kf's state has: x, P row-major, prev_heading, prev_speed, time."""
    return np.concatenate([kf.x, kf.P.reshape(36), [kf.prev_heading, kf.prev_speed, kf.time]])


# ---- covariances assigned by the user before the first call ------------------------------------------------------------------
def dense_P0(kind):
    """Non-separable covariances (cross-axis terms): the stream is flagged and takes the dense 6x6 filter."""
    P = np.eye(6) * 10.0
    if kind == "spd":                       # random SPD, as tests/test_gpu_more.py
        a = np.random.RandomState(11).standard_normal((6, 6))
        P = a @ a.T + 6 * np.eye(6)
    elif kind == "spd2":
        a = np.random.RandomState(12).standard_normal((6, 6))
        P = a @ a.T + 6 * np.eye(6)
    elif kind == "xy":                      # one symmetric cross-axis pair only
        P[0, 1] = P[1, 0] = 0.25
    elif kind == "nonsym":                  # a cross term on one side of the diagonal only
        P[2, 3], P[3, 2] = 0.5, 0.0
        P[0, 5] = -0.125
    else:
        raise ValueError(kind)
    return P


DENSE_STREAMS = {0: "spd", 63: "xy", 64: "nonsym", 66: "spd2"}     # of 67: both blocks of kf_kernel, first and last lanes
DENSE_S, DENSE_W, DENSE_SEED0 = 67, 200, 300          # stream s runs kf_scenario(seed = 300 + s)


def separable_P0():
    """Block-diagonal per axis (x: states 0, 2, 4; y: states 1, 3, 5), not symmetric within an axis: stays on the axis path."""
    rs = np.random.RandomState(21)
    P = np.zeros((6, 6))
    for ax in (0, 1):
        a = rs.standard_normal((3, 3))
        blk = a @ a.T + 4 * np.eye(3)
        blk[0, 1] += 0.375                  # P[r][c] != P[c][r]
        blk[2, 0] -= 0.25
        idx = np.array([ax, 2 + ax, 4 + ax])
        P[np.ix_(idx, idx)] = blk
    return P


SEPARABLE_X0 = np.array([1.5, -2.0, -0.75, 0.5, 0.25, -0.125])
SEPARABLE_W, SEPARABLE_SEED = 80, 7

# set_initial_state(0, 0, -5, 1e-3) leaves prev_heading just under +pi; this measurement pulls vy below zero, so the heading of
# the step is just above -pi and the difference wraps
WRAP_INIT = (0.0, 0.0, -5.0, 1e-3)
WRAP_Z = np.array([-0.5, 0.0, -5.0, -0.2])

MIXED_SEEDS, MIXED_W = tuple(range(6)), 700       # test (a); the partition test takes the first three
ZERO_DT_SEEDS, ZERO_DT_W = (18, 21, 26), 130      # (of seeds 0..39, three that both wrap and stand still in 130 frames)
STEADY_SEEDS = (0, 1, 2)
NULL_Z_SEEDS, NULL_Z_HEAD, NULL_Z_W = (1, 2), 40, 130
LOOP_SEEDS, LOOP_STEPS, LOOP_DENSE_STREAM = tuple(range(5)), 150, 3
CLASS_SEED, CLASS_W = 2, 60


def _fresh(cfg, P0=None, x0=None):
    kf = KalmanRef(*cfg)
    if P0 is not None:
        kf.P = np.array(P0, np.float64)
    if x0 is not None:
        kf.x = np.array(x0, np.float64)
    return kf


@functools.lru_cache(maxsize=None)
def case(kind, cfg_name, seed):
    """One sequence and its oracle run from the reset state (cached: the tests share them and must not modify them).
    Returns dict(z, mode, want [W, 12], margins, rec [45] final record)."""
    cfg = SETTINGS[cfg_name]
    P0 = x0 = None
    if kind == "mixed":
        z, mode = kf_scenario(MIXED_W, seed, cfg[0])
    elif kind == "zero_dt":
        z, mode = kf_scenario(ZERO_DT_W, seed, cfg[0])
    elif kind == "steady":
        z, mode = kf_steady_scenario(STEADY_W, cfg[0], seed)
    elif kind == "edges":
        z, mode = edge_pairs_scenario(cfg[0], seed)
    elif kind == "dense":                   # seed = stream index of the 67
        z, mode = kf_scenario(DENSE_W, DENSE_SEED0 + seed, cfg[0])
        P0 = dense_P0(DENSE_STREAMS[seed]) if seed in DENSE_STREAMS else None
    elif kind == "null_z":                  # NULL_Z_HEAD frames of every mode, then a window of modes 0 and 2 only (z is not read)
        z, mode = kf_scenario(NULL_Z_HEAD + NULL_Z_W, seed, cfg[0])
        mode[NULL_Z_HEAD:] = np.where(mode[NULL_Z_HEAD:] & 1, 2, 0)
    elif kind == "separable":
        z, mode = kf_scenario(SEPARABLE_W, seed, cfg[0])
        P0, x0 = separable_P0(), SEPARABLE_X0
    elif kind == "loop":                    # HotLoop: mode NULL = 1 everywhere
        z, _ = kf_scenario(LOOP_STEPS, seed, cfg[0])
        mode = np.ones(LOOP_STEPS, np.uint8)
        P0 = dense_P0("xy") if seed == LOOP_DENSE_STREAM else None
    elif kind == "class":
        z, mode = class_schedule(kf_scenario(CLASS_W, seed, cfg[0])[0])
    else:
        raise ValueError(kind)
    kf = _fresh(cfg, P0, x0)
    want, margins = run_oracle(z, mode, kf)
    for a in (z, mode, want):
        a.setflags(write=False)
    return dict(z=z, mode=mode, want=want, margins=margins, rec=final_record(kf), P0=P0, x0=x0)


def all_gpu_cases():
    """Every (kind, setting, seed) whose oracle run a GPU test compares with: the host test checks the margins of each."""
    out = [("mixed", c, s) for c in "ABC" for s in MIXED_SEEDS]
    out += [("zero_dt", "Z", s) for s in ZERO_DT_SEEDS]
    out += [("steady", c, s) for c in "BD" for s in STEADY_SEEDS]
    out += [("null_z", "B", s) for s in NULL_Z_SEEDS]
    out += [("edges", "B", 100)]
    out += [("dense", c, s) for c in "AB" for s in DENSE_STREAMS]
    out += [("separable", "A", SEPARABLE_SEED)]
    out += [("loop", "B", s) for s in LOOP_SEEDS]
    out += [("class", "B", CLASS_SEED)]
    return out


# ---- what a sequence visits (from the margins of its oracle run) ------------------------------------------------------------------
def held_frames(c):
    """bool [W]: no extract of the frame had speed > 0.1 (the frame gives no heading: the kernel's `gives` is false)."""
    m = c["margins"]
    gives = np.zeros(len(c["mode"]), bool)
    gives[m["frame"][~m["held"]]] = True
    return ~gives


def whole_batch_held(c):
    """A 64-frame batch (frames 64k .. 64k+63) without a giver: the next batch starts from carry_h handed through it."""
    h = held_frames(c)
    return any(h[f0:f0 + KF_BATCH].all() for f0 in range(0, len(h) - KF_BATCH + 1, KF_BATCH))


def giver_then_held_across_edge(c):
    """A giver in the last lane of a batch followed by a held first lane of the next."""
    h = held_frames(c)
    return any(not h[f - 1] and h[f] for f in range(KF_BATCH, len(h), KF_BATCH))


def edge_mode_pairs(c):
    mode = c["mode"]
    return {(int(mode[f - 1]), int(mode[f])) for f in range(KF_BATCH, len(mode), KF_BATCH)}
