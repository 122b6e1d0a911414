"""CPU restatement of the per-track Kalman filter (include/avhot.h: av_track_filter_update, av_track_obstacles_filtered), test
infrastructure.

The filter is written here with general 4 x 4 NumPy matrices and the Joseph-form update P <- (I - KH) P (I - KH)^T + K R K^T,
with no use of the structure the kernel exploits (x and y never mix, so P is two equal 2 x 2 blocks).  State is keyed by the
row's slot, as on the device.  The scenario helpers run it on the oracles' tables (TrackerRef + KalmanRef + detection_table);
TrackerRef has no slots, so a track gets the lowest free one at birth and gives it back when it dies: any assignment that is
unique among live rows and stable for a track's life gives the same filter output.
"""
import numpy as np

from tests.moving_ref import oracle_rows
from tests.obstacles_ref import DEFAULT_CFG, track_obstacles

F = np.array([[1.0, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]])
G = np.array([[0.5, 0], [0, 0.5], [1, 0], [0, 1]])
H = np.array([[1.0, 0, 0, 0], [0, 1, 0, 0]])
DEFAULT_FILTER = dict(q_accel=1.0, r_meas=4.0, p0_pos=4.0, p0_vel=100.0)


class TrackFilterRef:
    """One stream's filter bank: ids [tcap] (-1: free), x [tcap, 4], P [tcap, 4, 4], status."""

    def __init__(self, tcap=64, **cfg):
        c = dict(DEFAULT_FILTER)
        c.update(cfg)
        self.tcap = tcap
        self.Q = np.float64(c["q_accel"]) * (G @ G.T)
        self.R = np.float64(c["r_meas"]) * np.eye(2)
        self.P0 = np.diag([c["p0_pos"], c["p0_pos"], c["p0_vel"], c["p0_vel"]]).astype(np.float64)
        self.reset()

    def reset(self):
        self.ids = np.full(self.tcap, -1, np.int64)
        self.x = np.zeros((self.tcap, 4))
        self.P = np.zeros((self.tcap, 4, 4))
        self.status = 0

    def frame(self, rows, n):
        """rows: structured av_track_row array [tcap] of one frame, n its live count -> filt [tcap, 6], NaN at and past the
        clamped count."""
        out = np.full((self.tcap, 6), np.nan)
        for i in range(min(max(int(n), 0), self.tcap)):
            r = rows[i]
            k = int(r["slot"])
            if k < 0 or k >= self.tcap:
                out[i], self.status = 0.0, self.status | 1
                continue
            z = np.array([(np.float64(r["x1"]) + np.float64(r["x2"])) / 2, (np.float64(r["y1"]) + np.float64(r["y2"])) / 2])
            if self.ids[k] != int(r["id"]):
                self.ids[k] = int(r["id"])
                x, P = np.array([z[0], z[1], 0.0, 0.0]), self.P0.copy()
            else:
                x, P = F @ self.x[k], F @ self.P[k] @ F.T + self.Q
            if int(r["misses"]) == 0:
                S = H @ P @ H.T + self.R
                K = P @ H.T @ np.linalg.inv(S)
                x = x + K @ (z - H @ x)
                A = np.eye(4) - K @ H
                P = A @ P @ A.T + K @ self.R @ K.T
            self.x[k], self.P[k] = x, P
            out[i, :4] = x
            out[i, 4], out[i, 5] = np.sqrt(P[0, 0] + P[1, 1]), np.sqrt(P[2, 2] + P[3, 3])
        return out

    def update(self, rows, n):
        """rows [W, tcap], n [W] -> filt [W, tcap, 6]."""
        return np.stack([self.frame(rows[f], n[f]) for f in range(len(n))])


def run_filter(rows, n, tcap, **cfg):
    """rows [S, W, tcap], n [S, W] -> (filt [S, W, tcap, 6], status [S]); every stream from a reset state."""
    banks = [TrackFilterRef(tcap, **cfg) for _ in range(rows.shape[0])]
    return np.stack([b.update(rows[s], n[s]) for s, b in enumerate(banks)]), np.array([b.status for b in banks])


def track_obstacles_filtered(rows, n_rows, filt, plan_state, cfg=None, frame_rate=30.0):
    """tests.moving_ref.track_obstacles_moving with centre and velocity of row i from filt[i] (cx, cy, vx, vy, ., .): -> float64
    [m, 5] (x, y, radius, vx, vy).  Selection, order and radius are tests.obstacles_ref.track_obstacles'."""
    c = dict(DEFAULT_CFG)
    c.update(cfg or {})
    static = track_obstacles(rows, n_rows, plan_state, c)
    radius = np.asarray(c["radius"], np.float64)
    x_center, x_scale = np.float64(c["x_center"]), np.float64(c["x_scale"])
    y_far, y_scale, rate = np.float64(c["y_far"]), np.float64(c["y_scale"]), np.float64(frame_rate)
    x0, y0, h, v0 = (np.float64(v) for v in plan_state)
    cs, sn = np.cos(h), np.sin(h)
    c2, s2 = np.cos(h + np.pi / 2), np.sin(h + np.pi / 2)
    out = []
    for k in range(int(n_rows)):
        r = rows[k]
        cls = int(r["cls"])
        if not (int(r["flags"]) & 1) or cls < 0 or cls >= len(radius) or not radius[cls] > 0.0:
            continue
        cx, cy, rvx, rvy = (np.float64(v) for v in filt[k][:4])
        l, fw = (cx - x_center) * x_scale, y_far - cy * y_scale
        vl = (rvx * x_scale) * rate
        vf = v0 - (rvy * y_scale) * rate
        out.append(((x0 + fw * cs) + l * c2, (y0 + fw * sn) + l * s2, radius[cls], vf * cs + vl * c2, vf * sn + vl * s2))
    out = np.asarray(out, np.float64).reshape(-1, 5)
    assert len(out) == len(static) and np.array_equal(out[:, 2], static[:, 2])
    return out


def hand_table(frames, tcap, row_dtype):
    """frames: per frame a list of (id, slot, cx2, cy2, misses) with cx2, cy2 = TWICE the centre (so that half-integer centres can
    be written) -> rows [W, tcap], n [W]: confirmed rows of class 0 with 20 x 10 px boxes around the centre (as far as integers
    allow) and hist_len 2."""
    rows, n = np.zeros((len(frames), tcap), row_dtype), np.zeros(len(frames), np.int32)
    for f, live in enumerate(frames):
        n[f] = len(live)
        for i, (tid, slot, cx2, cy2, misses) in enumerate(live):
            r = rows[f, i]
            r["id"], r["slot"], r["misses"], r["flags"], r["hist_len"] = tid, slot, misses, 1, 2
            r["x1"], r["x2"] = (cx2 - 20) // 2, cx2 - (cx2 - 20) // 2
            r["y1"], r["y2"] = (cy2 - 10) // 2, cy2 - (cy2 - 10) // 2
            assert r["x1"] + r["x2"] == cx2 and r["y1"] + r["y2"] == cy2
    return rows, n


# ---- the loop scenario (tests/moving_cases.py) on the CPU, with slots ------------------------------------------------------------

def oracle_tables(row_dtype, offset, frames, tcap=64, tracker_kw=None, h=720, w=1280):
    """TrackerRef on detection_table(offset + 1, ...) -> (rows [frames, tcap], n [frames], deaths): av_track_row records per frame
    with a slot per track (lowest free at birth, freed at death); deaths = tracks that left the table."""
    from oracle.detector_ref import detection_table
    from oracle.tracker_ref import TrackerRef
    dn, box, cls, conf = detection_table(offset + 1, frames, h, w)
    trk = TrackerRef(**(tracker_kw or {}))
    slot_of, deaths = {}, 0
    rows, n = np.zeros((frames, tcap), row_dtype), np.zeros(frames, np.int32)
    for f in range(frames):
        trk.update(dn[f], box[f], cls[f], conf[f])
        live = {r["id"] for r in trk.rows}
        for tid in [t for t in slot_of if t not in live]:
            del slot_of[tid]
            deaths += 1
        for r in trk.rows:
            if r["id"] not in slot_of:
                slot_of[r["id"]] = min(set(range(tcap)) - set(slot_of.values()))
        cur = oracle_rows(trk, row_dtype)
        cur["slot"] = [slot_of[r["id"]] for r in trk.rows]
        rows[f, :len(cur)], n[f] = cur, len(cur)
    return rows, n, deaths


def filtered_scenario(row_dtype, offsets, frames, cfg, frame_rate, tracker_kw=None, filter_kw=None, tcap=64):
    """-> (per stream a list of (plan_state [4], obstacles5 [m, 5], rows [tcap], n, filt [tcap, 6]) for every frame, deaths) from
    the oracles and the restatement alone."""
    from oracle.harness_ref import ego_motion
    from oracle.kf_ref import KalmanRef
    out, deaths = [], 0
    for s, off in enumerate(offsets):
        rows, n, d = oracle_tables(row_dtype, off, frames, tcap, tracker_kw)
        deaths += d
        filt = TrackFilterRef(tcap, **(filter_kw or {})).update(rows, n)
        z, kf, per = ego_motion(frames, seed=s), KalmanRef(), []
        for f in range(frames):
            st = kf.step(z[f])
            ps = np.array([st[0], st[1], st[4], st[5]])
            per.append((ps, track_obstacles_filtered(rows[f], n[f], filt[f], ps, cfg, frame_rate), rows[f], int(n[f]), filt[f]))
        out.append(per)
    return out, deaths
