"""CPU restatement of av_track_obstacles (include/avhot.h), test infrastructure.

A stream's confirmed tracks become the planner's obstacles at the place the BEV panel draws them (bev_renderer.py:207-208:
lateral = (cx - 320) * 0.03 m, forward = 50 - cy * 0.1 m), carried into the planner's frame with the start state's position
and heading the way MotionPlanner places a candidate of lateral offset l at arc length f (motion_planner.py:175-180).  Plain
NumPy scalar arithmetic in the operation order the header states.
"""
import numpy as np

DEFAULT_CFG = dict(x_center=320.0, x_scale=0.03, y_far=50.0, y_scale=0.1, radius=[1.5] * 6 + [0.0] * 10)


def track_obstacles(rows, n_rows, plan_state, cfg=None):
    """rows: structured av_track_row array [>= n_rows] of one frame, plan_state (x, y, heading, speed)
    -> float64 [m, 3] (x, y, radius) of the confirmed rows with a positive radius, in table order."""
    c = dict(DEFAULT_CFG)
    c.update(cfg or {})
    radius = np.asarray(c["radius"], np.float64)
    x_center, x_scale = np.float64(c["x_center"]), np.float64(c["x_scale"])
    y_far, y_scale = np.float64(c["y_far"]), np.float64(c["y_scale"])
    x0, y0, h = (np.float64(v) for v in plan_state[:3])
    cs, sn = np.cos(h), np.sin(h)
    c2, s2 = np.cos(h + np.pi / 2), np.sin(h + np.pi / 2)
    out = []
    for k in range(int(n_rows)):
        r = rows[k]
        cls = int(r["cls"])
        if not (int(r["flags"]) & 1) or cls < 0 or cls >= len(radius) or not radius[cls] > 0.0:
            continue
        cx = np.float64(int(r["x1"]) + int(r["x2"])) / 2.0
        cy = np.float64(int(r["y1"]) + int(r["y2"])) / 2.0
        lat = (cx - x_center) * x_scale
        fwd = y_far - cy * y_scale
        ox = (x0 + fwd * cs) + lat * c2
        oy = (y0 + fwd * sn) + lat * s2
        out.append((ox, oy, radius[cls]))
    return np.asarray(out, np.float64).reshape(-1, 3)
