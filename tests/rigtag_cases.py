"""The inputs of tests/test_gpu_rigtag.py, built once and shared with tests/test_rigtag_host.py, which pins their margins and what
each of them claims to show.

The tagger reads the tracker's state, so its cases plant that state directly: plant() writes the slots of one vehicle.  A planted
case uses integer-valued coordinates, heading 0 and dt = 1/32, so that a quantity can sit exactly on its threshold."""
import functools

import numpy as np

from tests import rig_cases as rc
from tests import rig_ref as rr
from tests import rigtag_ref as tg
from tests import rigtrack_ref as tr

TCAPS = (1, 64, 65, 512)
PLANTED = dict(dt=1.0 / 32.0, corridor_half=2.0, adjacent_half=5.0, alongside=10.0, pass_speed=1.0, min_hits=3)
EGO = (100.0, 50.0, 0.0, 8.0)           # the planted cases' start state: integers, heading 0


def plant(tcap, slots, ego=EGO):
    """One vehicle's tracker state: slots = {slot: dict(id, cls (class id, None: no class word), rel (ex, ey, rvx, rvy: position and
    velocity relative to the ego, along the world axes), hits=5, misses=0)}."""
    st = tr.reset_state(tcap)
    hdr, sl = tr.views_of(st)
    for t, q in slots.items():
        s = sl[t]
        ex, ey, rvx, rvy = q["rel"]
        s["id"], s["hits"], s["misses"], s["age"] = q["id"], q.get("hits", 5), q.get("misses", 0), 7
        s["reserved"][0] = 0 if q["cls"] is None else q["cls"] + 1
        s["x"] = (ego[0] + ex, ego[1] + ey, rvx + ego[3] * np.cos(ego[2]), rvy + ego[3] * np.sin(ego[2]))
        s["p"], s["r"] = (1.0, 0.0, 25.0), 1.0
    hdr[1], hdr[3] = 1000, len(slots)
    return st


# (label, (ex, ey, rvx, rvy), class id, expected type, expected risk, extra slot fields); class ids are the kinds themselves (tg.KINDS)
RULES = [
    ("near_miss", (2, 0, 0, 0), 3, tg.NEAR_MISS, 3, {}),
    ("d == 3 is no near miss", (3, 0, 0, 0), 0, -1, 0, {}),
    ("d == 0", (0, 0, 0, 0), 3, tg.NEAR_MISS, 3, {}),
    ("pedestrian crossing, d < 8", (6, 1, 0, 0), 1, tg.PED_CROSSING, 2, {}),
    ("pedestrian crossing, d >= 8", (9, 1, 0, 0), 1, tg.PED_CROSSING, 1, {}),
    ("pedestrian crossing, d == 8", (8, 0, 0, 0), 1, tg.PED_CROSSING, 1, {}),
    ("pedestrian at |Y| == corridor_half waits", (3, 2, 0, 0), 1, tg.PED_WAITING, 0, {}),
    ("pedestrian behind waits", (-6, 0, 3, 0), 1, tg.PED_WAITING, 0, {}),
    ("pedestrian at d == 10", (10, 0, 0, 0), 1, -1, 0, {}),
    ("cyclist, d < 8", (5, 5, 0, 0), 2, tg.CYCLIST, 1, {}),
    ("cyclist, d >= 8", (0, 12, 0, 0), 2, tg.CYCLIST, 0, {}),
    ("cyclist at d == 15", (15, 0, 0, 0), 2, -1, 0, {}),
    ("following", (20, 0, -1, 0), 3, tg.FOLLOWING, 0, {}),
    ("following, d < 10", (8, 1, 0, 0), 3, tg.FOLLOWING, 1, {}),
    ("following, ttc 2 s", (20, 0, -10, 0), 3, tg.FOLLOWING, 2, {}),
    ("following, ttc == 3 s", (15, 0, -5, 0), 3, tg.FOLLOWING, 0, {}),
    ("vehicle at d == 5", (5, 0, 0, 0), 3, -1, 0, {}),
    ("vehicle at d == 30", (30, 0, 0, 0), 3, -1, 0, {}),
    ("being followed", (-12, 0, 0, 0), 3, tg.BEING_FOLLOWED, 0, {}),
    ("being followed, ttc 2 s", (-12, 0, 6, 0), 3, tg.BEING_FOLLOWED, 2, {}),
    ("passing", (4, 4, -3, 0), 3, tg.PASSING, 0, {}),
    ("being passed", (-4, -4, 3, 0), 3, tg.BEING_PASSED, 0, {}),
    ("RVX == -pass_speed", (4, 4, -1, 0), 3, -1, 0, {}),
    ("RVX == pass_speed", (4, -4, 1, 0), 3, -1, 0, {}),
    ("|Y| == adjacent_half", (1, 5, -3, 0), 3, -1, 0, {}),
    ("|X| == alongside", (10, 4, -3, 0), 3, -1, 0, {}),
    ("motorcycle: a vehicle without rules", (20, 0, 0, 0), 4, -1, 0, {}),
    ("class 16", (20, 0, 0, 0), 16, -1, 0, {}),
    ("no class", (20, 0, 0, 0), None, -1, 0, {}),
    ("coasting", (22, 0, 0, 0), 3, tg.FOLLOWING, 0, dict(misses=2)),
    ("unconfirmed", (2, 0, 0, 0), 3, None, 0, dict(hits=2)),
]


def rule_slots(tcap):
    """Where the rules sit in a table of tcap slots: spread over every wave."""
    if tcap == 1:
        return {0: 12}                                           # the one slot follows
    step = 1 if tcap < 128 else 16
    return {k * step + (3 if step > 1 else 0): k for k in range(len(RULES))}


def _rule_state(tcap):
    slots = {}
    for t, k in rule_slots(tcap).items():
        label, rel, cls, typ, risk, extra = RULES[k]
        slots[t] = dict(id=10 + k, cls=cls, rel=rel, **extra)
    return plant(tcap, slots)


def _tie_state(tcap):
    """Two followers of equal risk and confidence in the first and the last slot (waves 0 and 7 of 512): the smaller slot is primary."""
    q = dict(cls=3, rel=(20, 0, 0, 0))
    return plant(tcap, {0: dict(id=1, **q), tcap - 1: dict(id=2, **q)} if tcap > 1 else {0: dict(id=1, **q)})


def _critical_state(tcap):
    """A follower one second from contact: its own risk is high, the frame's is critical."""
    return plant(tcap, {tcap - 1: dict(id=4, cls=3, rel=(12, 0, -12, 0))})


@functools.lru_cache(maxsize=None)
def planted(V, tcap):
    """One frame: vehicle 0 holds the rule table, vehicle 1 the primary tie, vehicle 2 nothing."""
    states = [_rule_state(tcap), _tie_state(tcap), tr.reset_state(tcap)][:V]
    ps = np.array([EGO] * V)
    return dict(V=V, tcap=tcap, cfg=tg.cfg(**PLANTED), frames=[(np.stack(states), ps)], exact=True)


@functools.lru_cache(maxsize=None)
def critical(tcap):
    return dict(V=1, tcap=tcap, cfg=tg.cfg(**PLANTED), frames=[(np.stack([_critical_state(tcap)]), np.array([EGO]))], exact=True)


RING_FRAMES = 35


@functools.lru_cache(maxsize=None)
def ring(tcap=65):
    """35 frames of one vehicle, lateral offsets by frame:
    slot 0   a vehicle 12 m ahead: outside the corridor in frames 0..2, inside from frame 3 -- followed while the ring is short
             (frames 3..8), a cut-in from the tenth entry (frame 9) while the oldest of the last 30 lies outside (up to frame 31: the
             ring wraps at frame 30), followed again from frame 32
    slot 64  the reverse: inside in frames 0..4, outside from 5 -- a cut-out from frame 9 to frame 33, nothing at frame 34
    slot 2   outside under id 7 up to frame 19, inside under id 8 from frame 20: the ring restarts, so no cut-in at any frame"""
    frames = []
    for f in range(RING_FRAMES):
        slots = {0: dict(id=5, cls=3, rel=(12, 4 if f < 3 else 1, 0, 0)),
                 2: dict(id=7 if f < 20 else 8, cls=3, rel=(12, -4 if f < 20 else -1, 0, 0))}
        if tcap > 64:
            slots[64] = dict(id=6, cls=3, rel=(12, 1 if f < 5 else 3, 0, 0))
        frames.append((np.stack([plant(tcap, slots)]), np.array([EGO])))
    return dict(V=1, tcap=tcap, cfg=tg.cfg(**PLANTED), frames=frames, exact=True)


@functools.lru_cache(maxsize=None)
def rotated(V=3, tcap=65, n_frames=3, seed=7):
    """Random slots around egos whose headings are no multiple of pi/2, with the default settings; classes from -1 to 17, hits
    around min_hits, free slots in between.  The tracks move a little from frame to frame."""
    rng = np.random.default_rng(seed)
    ps = np.array([[3.0, -2.0, 0.7, 7.5], [-11.0, 4.0, -2.1, 0.25], [0.5, 0.25, 3.0, 12.0]][:V])
    live = rng.random((V, tcap)) < 0.7
    rel = np.concatenate([rng.uniform(-32, 32, (V, tcap, 1)), rng.uniform(-7, 7, (V, tcap, 1)), rng.uniform(-9, 9, (V, tcap, 2))], axis=2)
    cls = rng.integers(-1, 18, (V, tcap))
    hits = rng.integers(1, 7, (V, tcap))
    frames = []
    for f in range(n_frames):
        states = []
        for v in range(V):
            slots = {}
            for t in range(tcap):
                if live[v, t]:
                    ex, ey, rvx, rvy = rel[v, t]
                    c, s = np.cos(ps[v, 2]), np.sin(ps[v, 2])           # rel is in the ego's axes here: forward, lateral
                    ex, ey = ex + rvx * f / 30.0, ey + rvy * f / 30.0
                    slots[t] = dict(id=int(100 * v + t + 1), cls=None if cls[v, t] < 0 else int(cls[v, t]), hits=int(hits[v, t]) + f,
                                    rel=(c * ex - s * ey, s * ex + c * ey, c * rvx - s * rvy, s * rvx + c * rvy))
            states.append(plant(tcap, slots, ego=ps[v]))
        frames.append((np.stack(states), ps))
    c = tg.cfg(class_kind=(3, 3, 1, 2, 4, 3, 0, 0) + (0,) * 8)          # the reference's eight classes
    return dict(V=V, tcap=tcap, cfg=c, frames=frames, exact=False)


def play(case):
    """The restatement, free-running over the case: [frame][vehicle] -> rigtag_ref.interact's result."""
    V, tcap = case["V"], case["tcap"]
    st = [tg.reset_state(tcap) for _ in range(V)]
    out = []
    for track, ps in case["frames"]:
        res = [tg.interact(track[v], ps[v], st[v], case["cfg"]) for v in range(V)]
        st = [r["state"] for r in res]
        out.append(res)
    return out


# ---- class lanes ----------------------------------------------------------------------------------------------------------------

def _classes(shape, seed):
    return np.random.default_rng(seed).integers(-3, 21, shape).astype(np.int32)


@functools.lru_cache(maxsize=None)
def fuse(name, ncol=5):
    """A case of tests/rig_cases.py with a class per row (negatives among them), or one of the two hand-made ones:
    nearest   three cameras in a row see one object at 10, 15 and 5 metres: the third holds the largest weight
    mirror    two cameras a metre to either side see it in mirror-image rows: exactly equal weights, the earlier camera's class"""
    if name == "nearest":
        mounts = [[rr.mount(0.0, 0.0, 0.0), rr.mount(0.0, -5.0, 0.0), rr.mount(0.0, 5.0, 0.0)]]
        lists = [[[10.0, 0.0, 1.0]], [[15.0, 0.0, 1.0]], [[5.0, 0.0, 1.0]]]
        c = rc._case(1, 3, 4, ncol, mounts, [rc._rows(l, ncol, i) for i, l in enumerate(lists)])
        c["cam_cls"] = np.array([[2, 0, 0, 0], [-4, 0, 0, 0], [5, 0, 0, 0]], np.int32)
        c["want_cls"] = [[5]]
    elif name == "mirror":
        mounts = [[rr.mount(0.0, 0.0, 1.0), rr.mount(0.0, 0.0, -1.0)]]
        lists = [[[8.0, -1.0, 1.0]], [[8.0, 1.0, 1.0]]]
        c = rc._case(1, 2, 4, ncol, mounts, [rc._rows(l, ncol, i) for i, l in enumerate(lists)])
        c["cam_cls"] = np.array([[-2, 0, 0, 0], [9, 0, 0, 0]], np.int32)
        c["want_cls"] = [[-2]]
    else:
        c = dict(rc.case(name, ncol))
        c["cam_cls"] = _classes(c["cam_obs"].shape[:2], 31)
        c["want_cls"] = None
    V, K = c["V"], c["K"]
    c["cls"] = [tg.fuse_cls(c["cam_obs"][v * K:(v + 1) * K], c["cam_n"][v * K:(v + 1) * K], c["cam_cls"][v * K:(v + 1) * K],
                            c["mounts"][v], *c["cfg"]) for v in range(V)]
    return c


FUSE_CASES = ("growth", "contest", "full", "coincident", "nearest", "mirror")


@functools.lru_cache(maxsize=None)
def track(tcap):
    """Four frames of one vehicle, max_age 0 and min_hits 1: two objects are born with class 2 and without one; then both are seen
    with classes 5 and 7 (the latest wins); then both without a class (they keep theirs); then the first is not seen and dies while
    a new object without a class appears: it is born into the slot just freed and inherits nothing.  (One slot: the second object
    never finds room.)"""
    c = tr.cfg(max_age=0, min_hits=1)
    rows = [([[0.0, 0.0, 1.0], [20.0, 0.0, 1.0]], [2, -1]), ([[0.1, 0.0, 1.0], [20.1, 0.0, 1.0]], [5, 7]),
            ([[0.2, 0.0, 1.0], [20.2, 0.0, 1.0]], [-1, -7]), ([[50.0, 50.0, 1.0], [20.3, 0.0, 1.0]], [-1, 11])]
    frames = []
    for r, k in rows:
        obs = np.full((1, 4, 3), np.nan)
        obs[0, :2] = r
        cls = np.full((1, 4), 99, np.int32)
        cls[0, :2] = k
        frames.append((obs, np.array([2], np.int32), None, np.array([[0.0, 0.0, 0.0, 0.0]]), cls))
    return dict(V=1, tcap=tcap, ocap_in=4, ncol=3, cfg=c, frames=frames)
