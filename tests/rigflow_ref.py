"""CPU restatement of the rig odometry (include/avhot.h: av_rig_egoflow_solve / _update), test infrastructure.

Built on tests/egoflow_ref.py: the per-camera vote and gate are ref.solve's, the fit and the residual are ref.fit and ref.residual2
fed vehicle-frame rows (X, Y, DX, DY) in the places of (f, l, d_f, d_l).  All sums are sequential -- camera 0's rows in tile order,
then camera 1's, ... -- while the device sums per lane, over a tree and then over the cameras: the last bits may differ.
A mount is (c, s, mx, my), av_rig_mount's fields."""
import numpy as np

from tests import egoflow_ref as ref

f8 = np.float64
MAX_CAMS = 8
ONE = f8(1.0)


def vehicle_rows(tiles, mount, m):
    """Tile rows of one camera -> rows of the same dtype that ref.fit and ref.residual2 read (with m_per_px = 1) as the
    vehicle-frame rows: f = X, l = Y, and (dy, sub_dy, dx, sub_dx) = (0, -DX, 0, DY), so that ref.displacement gives
    (-(0 + -DX) * 1, (0 + DY) * 1) = (DX, DY) exactly."""
    c, s, mx, my = (f8(v) for v in mount)
    out = np.zeros(len(tiles), np.dtype(ref.TILE_FIELDS))
    for i, t in enumerate(tiles):
        f, l = f8(t["f"]), f8(t["l"])
        df, dl = ref.displacement(t, m)
        out[i]["f"] = (mx + c * f) - s * l
        out[i]["l"] = (my + s * f) + c * l
        out[i]["sub_dy"] = -(c * df - s * dl)
        out[i]["sub_dx"] = s * df + c * dl
    return out


def solve(tables, mounts, c):
    """tables: K tile tables [n_tiles] of one vehicle (the match's fields), mounts [K][4] -> (motion dict, flags int32 [K, n_tiles],
    info dict: av_rig_egoflow_info's fields, and hyp_res_px: per regular hypothesis the residuals, in pixels, of all gated rows in
    camera order, what the inlier counts rest on)."""
    K, m = len(tables), f8(c["m_per_px"])
    thr = f8(c["inlier_px"]) * m
    thr2 = thr * thr
    flags = np.zeros((K, len(tables[0])), np.int32)
    info = dict(hypothesis=-1, views=0, cam_accepted=np.zeros(MAX_CAMS, np.int32), cam_gated=np.zeros(MAX_CAMS, np.int32),
                cam_inliers=np.zeros(MAX_CAMS, np.int32), cam_vote_dy=np.zeros(MAX_CAMS, np.int32),
                cam_vote_dx=np.zeros(MAX_CAMS, np.int32), hyp_count=np.full(MAX_CAMS + 1, -1, np.int32), hyp_res_px={}, hists=[])
    rows, owner, index = [], [], []                           # the vehicle's gated rows, their camera and tile index
    for k in range(K):
        mo, fl, inf = ref.solve(tables[k], c)
        flags[k] = fl & (ref.ACCEPTED | ref.LIVE | ref.GATED)
        info["cam_accepted"][k], info["cam_gated"][k] = mo["n_accepted"], mo["n_gated"]
        info["cam_vote_dy"][k], info["cam_vote_dx"][k] = mo["vote_dy"], mo["vote_dx"]
        info["hists"].append(inf["hist"])
        g = np.nonzero(fl & ref.GATED)[0]
        rows.append(vehicle_rows(tables[k][g], mounts[k], m))
        owner.append(np.full(len(g), k)), index.append(g)
    cam_rows = rows
    rows, owner, index = np.concatenate(rows), np.concatenate(owner), np.concatenate(index)
    motion = dict(t_f=f8(0.0), t_l=f8(0.0), omega=f8(0.0), rms=f8(0.0), n_accepted=int(info["cam_accepted"].sum()),
                  n_gated=int(info["cam_gated"].sum()), n_inliers=0, valid=0, vote_dy=0, vote_dx=0)
    best, within = -1, None
    for i, rset in enumerate([rows] + cam_rows):
        ok, tf, tl, om = ref.fit(rset, ONE)
        if not ok:
            continue
        r2 = np.array([ref.residual2(r, ONE, tf, tl, om) for r in rows], f8)
        info["hyp_res_px"][i] = np.sqrt(r2) / m
        inl = ~(r2 > thr2)
        info["hyp_count"][i] = int(inl.sum())
        if best < 0 or info["hyp_count"][i] > info["hyp_count"][best]:
            best, within = i, inl
    info["hypothesis"] = best
    if best < 0:
        return motion, flags, info
    for k, i in zip(owner[within], index[within]):
        flags[k, i] |= ref.INLIER
        info["cam_inliers"][k] += 1
    info["views"] = int(sum(1 << k for k in range(K) if info["cam_inliers"][k] > 0))
    motion["n_inliers"] = int(within.sum())
    ok, tf, tl, om = ref.fit(rows[within], ONE)
    if not ok:
        return motion, flags, info
    ss = f8(0.0)
    for r in rows[within]:
        ss = ss + ref.residual2(r, ONE, tf, tl, om)
    motion.update(t_f=tf, t_l=tl, omega=om, rms=np.sqrt(ss / f8(motion["n_inliers"])),
                  valid=int(motion["n_inliers"] >= c["min_inliers"]))
    return motion, flags, info


class RigOdometer:
    """One vehicle of av_rig_egoflow_update on gray patches (update_patches) or frames (update_frames): K cameras, one state."""

    def __init__(self, c, mounts, cams=None, pose=(0.0, 0.0, 0.0)):
        self.c, self.mounts, self.cams, self.K = c, [tuple(f8(v) for v in mt) for mt in mounts], cams, len(mounts)
        self.state = dict(x=f8(pose[0]), y=f8(pose[1]), psi=f8(pose[2]), frames=0)
        self.prev = [np.zeros((c["gh"], c["gw"]), np.uint8) for _ in range(self.K)]     # (the ping-pong pairs start zero-filled)
        self.tiles = self.motion = self.flags = self.info = None

    def update_patches(self, grays, valids):
        self.tiles = [ref.match(grays[k], self.prev[k], valids[k], self.c) for k in range(self.K)]
        self.motion, self.flags, self.info = solve(self.tiles, self.mounts, self.c)
        self.prev = list(grays)
        return ref.measure(self.state, self.motion, self.c)

    def update_frames(self, bgrs):
        pv = [ref.patch(self.cams[k], bgrs[k], self.c) for k in range(self.K)]
        return self.update_patches([p for p, _ in pv], [v for _, v in pv])

    @property
    def pose(self):
        return np.array([self.state["x"], self.state["y"], self.state["psi"]], f8)
