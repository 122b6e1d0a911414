"""CPU restatements of the moving-obstacle planner inputs (include/avhot.h: av_planner_plan_moving, av_planner_evaluate_moving,
av_track_obstacles_moving), test infrastructure.

A moving obstacle is (x, y, radius, vx, vy) in the planner's frame; the waypoint with timestamp t meets the disc at
px = x + vx * t, py = y + vy * t, and the rest of the cost is PlannerRef's.  A track becomes one with the velocity its last
centre difference predicts (Track.velocity, multi_object_tracker.py:35-47), scaled like its position and by the frame rate, plus
the ego's own speed along its heading (the image is ego-centric).  NumPy float64 in the operation order the header states.
"""
import numpy as np

from oracle.planner_ref import PlannerRef
from tests.obstacles_ref import DEFAULT_CFG, track_obstacles


def positions_at(wp, obstacles5):
    """wp [..., n, 6], obstacles5 [m, 5] -> (px, py) [..., n, m]: every obstacle where it is at every waypoint's timestamp."""
    o = np.asarray(obstacles5, np.float64).reshape(-1, 5)
    t = np.asarray(wp)[..., 4, None]
    return o[:, 0] + o[:, 3] * t, o[:, 1] + o[:, 4] * t


class MovingPlannerRef(PlannerRef):
    def cost(self, wp, obstacles=None):
        """PlannerRef.cost without obstacles, followed in the same strict left-to-right sum by one term vector per obstacle
        (x, y, radius, vx, vy), each evaluated at the waypoints' own timestamps wp[:, 4]."""
        base = PlannerRef.cost(self, wp, None)
        if obstacles is None or len(obstacles) == 0:
            return base
        t = wp[:, 4]
        terms = []
        for ox, oy, r, vx, vy in obstacles:
            px = ox + vx * t
            py = oy + vy * t
            dist = np.sqrt((wp[:, 0] - px) ** 2 + (wp[:, 1] - py) ** 2)
            hard = 1000 * (r * 2 - dist)
            with np.errstate(divide="ignore"):
                soft = 10 / (dist - r + 0.1)
            terms.append(np.where(dist < r * 2, hard, np.where(dist < r * 4, soft, 0.0)))
        return float(np.cumsum(np.concatenate([[base]] + terms))[-1])


def track_obstacles_moving(rows, n_rows, plan_state, cfg=None, frame_rate=30.0):
    """rows: structured av_track_row array of one frame, plan_state (x, y, heading, speed) -> float64 [m, 5]
    (x, y, radius, vx, vy); columns 0..2 are tests.obstacles_ref.track_obstacles' own."""
    c = dict(DEFAULT_CFG)
    c.update(cfg or {})
    static = track_obstacles(rows, n_rows, plan_state, c)
    radius = np.asarray(c["radius"], np.float64)
    x_scale, y_scale, rate = np.float64(c["x_scale"]), np.float64(c["y_scale"]), np.float64(frame_rate)
    h, v0 = np.float64(plan_state[2]), np.float64(plan_state[3])
    cs, sn = np.cos(h), np.sin(h)
    c2, s2 = np.cos(h + np.pi / 2), np.sin(h + np.pi / 2)
    vel = []
    for k in range(int(n_rows)):
        r = rows[k]
        cls = int(r["cls"])
        if not (int(r["flags"]) & 1) or cls < 0 or cls >= len(radius) or not radius[cls] > 0.0:
            continue
        has_vel = int(r["hist_len"]) >= 2
        rvx = np.float64(r["vx"]) if has_vel else np.float64(0.0)
        rvy = np.float64(r["vy"]) if has_vel else np.float64(0.0)
        vl = (rvx * x_scale) * rate
        vf = v0 - (rvy * y_scale) * rate
        vel.append((vf * cs + vl * c2, vf * sn + vl * s2))
    assert len(vel) == len(static)
    return np.concatenate([static, np.asarray(vel, np.float64).reshape(-1, 2)], axis=1)


def margin_and_allowance(wp, obstacles5):
    """tests/test_gpu_plan_each.py's _margin_and_allowance with every obstacle at its place for each waypoint's time:
    wp [C, n, 6] of the oracle, obstacles5 [m, 5] -> (smallest | dist - 2r |, | dist - 4r | over all pairs, allowance [C],
    pairs in the hard branch, pairs in the soft branch).  The obstacle's own position is reproduced exactly (the same two
    roundings on both sides), so the allowance is the static one: the term's Lipschitz constant times the waypoint's accepted
    position error eps_i = sqrt(2) (1e-12 max(|x_i|, |y_i|) + 1e-11), summed over the pairs in a branch."""
    obstacles5 = np.asarray(obstacles5, np.float64).reshape(-1, 5)
    if len(obstacles5) == 0:
        return np.inf, np.zeros(len(wp)), 0, 0
    x, y = wp[:, :, 0, None], wp[:, :, 1, None]
    px, py = positions_at(wp, obstacles5)
    r = obstacles5[:, 2]
    dist = np.sqrt((x - px) ** 2 + (y - py) ** 2)                                    # [C, n, m]
    eps = np.sqrt(2.0) * (1e-12 * np.maximum(np.abs(x), np.abs(y)) + 1e-11)          # [C, n, 1]
    hard, soft = dist < 2 * r, (dist >= 2 * r) & (dist < 4 * r)
    with np.errstate(divide="ignore", invalid="ignore"):
        allow = np.where(hard, 1000.0 * eps, 0.0) + np.where(soft, 10.0 * eps / (dist - r + 0.1) ** 2, 0.0)
    margin = min(np.abs(dist - 2 * r).min(), np.abs(dist - 4 * r).min())
    return float(margin), allow.sum(axis=(1, 2)), int(hard.sum()), int(soft.sum())


# ---- the loop scenario of tests/test_gpu_moving.py on the CPU: TrackerRef + KalmanRef + detection_table ---------------------------

def oracle_rows(trk, row_dtype):
    """TrackerRef's table as av_track_row records (the fields av_track_obstacles_moving reads and the counters beside them)."""
    rows = np.zeros(len(trk.rows), row_dtype)
    for k, r in enumerate(trk.rows):
        rows[k]["id"], rows[k]["cls"], rows[k]["conf"] = r["id"], r["cls"], r["conf"]
        rows[k]["x1"], rows[k]["y1"], rows[k]["x2"], rows[k]["y2"] = r["bbox"]
        rows[k]["age"], rows[k]["hits"], rows[k]["misses"] = r["age"], r["hits"], r["misses"]
        rows[k]["hist_len"] = r["hits"]                     # a centre at birth and one per match
        rows[k]["flags"] = 1 if r["hits"] >= trk.min_hits else 0
        if r["vel"]:
            rows[k]["vx"], rows[k]["vy"] = r["vel"][-1]
    return rows


def loop_scenario(row_dtype, offsets, frames, cfg, frame_rate, h=720, w=1280):
    """-> per stream a list of (plan_state [4], obstacles5 [m, 5]) for every frame, from the oracles alone."""
    from oracle.detector_ref import detection_table
    from oracle.harness_ref import ego_motion
    from oracle.kf_ref import KalmanRef
    from oracle.tracker_ref import TrackerRef
    out = []
    for s, off in enumerate(offsets):
        n, box, cls, conf = detection_table(off + 1, frames, h, w)
        z = ego_motion(frames, seed=s)
        trk, kf, per = TrackerRef(), KalmanRef(), []
        for f in range(frames):
            trk.update(n[f], box[f], cls[f], conf[f])
            st = kf.step(z[f])
            ps = np.array([st[0], st[1], st[4], st[5]])
            rows = oracle_rows(trk, row_dtype)
            per.append((ps, track_obstacles_moving(rows, len(rows), ps, cfg, frame_rate)))
        out.append(per)
    return out
