"""The cases of the road-memory tests, shared by tests/test_roadmem_host.py (the NumPy reference against the world the panels were
rendered from) and tests/test_gpu_roadmem.py (the device against the reference): surround panels rendered straight from
egoflow_cases.world() at known poses, with a made-up cover."""
import numpy as np

from tests import egoflow_cases as ego
from tests import roadmem_ref as ref

f8 = np.float64
SHIFTS = (0.0, 0.9, 1.7)        # b, g, r: three different roads, so that a swapped channel shows


def world_bgr(x, y):
    """The panel's bytes at world point (x, y): uint8 [..., 3]."""
    return np.stack([np.clip(np.rint(ego.world(x, y, s)), 0, 255) for s in SHIFTS], axis=-1).astype(np.uint8)


def render_panel(pose, c):
    """The surround panel of a vehicle at pose (x, y, psi), every pixel seen: uint8 [gh, gw, 3]."""
    X, Y = ref.panel_points(c)
    x, y, psi = pose
    return world_bgr(x + X * np.cos(psi) - Y * np.sin(psi), y + X * np.sin(psi) + Y * np.cos(psi))


def cover_map(c, hole=(5.0, 2.4), wedge=(100.0, 125.0), band=6):
    """A made-up cover [gh, gw]: 0 in a rectangular hole of hole[0] x hole[1] metres round the origin, in the wedge between the two
    bearings (degrees from the forward axis, towards +Y) and in the `band` farthest rows; elsewhere 1 or 3 (any non-zero counts)."""
    X, Y = ref.panel_points(c)
    X, Y = np.broadcast_arrays(X, Y)
    cover = np.where(Y > 0.0, 3, 1).astype(np.uint8)
    in_hole = (np.abs(X) <= hole[0] / 2.0) & (np.abs(Y) <= hole[1] / 2.0)
    bearing = np.degrees(np.arctan2(Y, X))
    cover[in_hole | ((bearing >= wedge[0]) & (bearing <= wedge[1]))] = 0
    cover[:band] = 0
    return cover, in_hole


def arc(start, step, n_frames):
    """-> [n_frames] poses (x, y, psi): `step` = (d_f, d_l, d_psi) per frame from `start`."""
    poses = [tuple(f8(v) for v in start)]
    for _ in range(n_frames - 1):
        poses.append(ego.compose(poses[-1], step))
    return poses


def margin(c, frames):
    """The smallest distance of any `* 65536 + 0.5` argument from an integer over the cells and pixels whose outcome can depend on
    it: in the update the cells of the window within one pixel of the panel, in the fill the uncovered pixels.  frames: a list of
    (pose5, cover) in order, pose5 = (x, y, cs, sn, reset) of one vehicle.  (The device and NumPy round the same operations the
    same way; the margin says that no case rests on it.)"""
    best = np.inf
    for pose, cover in frames:
        i0, j0, bad = ref.window(pose[0], pose[1], c)
        if bad:
            continue
        n = c["n"]
        i, j = np.broadcast_arrays((i0 + np.arange(n))[:, None], (j0 + np.arange(n))[None, :])
        ar, ac = ref.cell_taps(c, pose, i, j)["args"]
        near = (ar > -65536.0) & (ar < (c["gh"] + 1) * 65536.0) & (ac > -65536.0) & (ac < (c["gw"] + 1) * 65536.0)
        ai, aj = ref.pixel_taps(c, pose, i0, j0)["args"]
        for a, sel in ((ar, near), (ac, near), (ai, cover == 0), (aj, cover == 0)):
            if sel.any():
                best = min(best, float(np.abs(a[sel] - np.round(a[sel])).min()))
    return best


# ---- the device case: three vehicles, a panel that is no multiple of the tile, a small canvas -----------------------------------------
DEV_CFG = ref.cfg(n=48, max_age=7, m_per_px=0.1, gh=40, gw=36, x_far=2.0, panel_m_per_px=0.1, fill=(7, 99, 201))
DEV_FRAMES = 12
DEV_STARTS = [(1.03, -2.07, 0.3), (-7.31, -4.12, 2.0), (-0.38, -0.61, -2.5)]    # one at negative coordinates, two rotated beyond pi/2
DEV_STEP = (0.13, 0.004, 0.011)
DEV_RESET = (1, 6)              # vehicle 1 is told to reset on frame 6
DEV_JUMP = (2, 7, 6.2)          # vehicle 2 is 6.2 m (more than 48 cells) further along x from frame 7 on


def device_case():
    """-> (cfg, poses [F][V] of (x, y, cs, sn, reset), panels uint8 [F, V, gh, gw, 3], covers uint8 [F, V, gh, gw]).  The hole is
    1.6 m x 1.0 m; the cover's wedge moves with the frame number, so that cells are seen on one frame and not on the next."""
    c = DEV_CFG
    tracks = [arc(s, DEV_STEP, DEV_FRAMES) for s in DEV_STARTS]
    poses, panels, covers = [], [], []
    for f in range(DEV_FRAMES):
        row, pr, cr = [], [], []
        for v, tr in enumerate(tracks):
            x, y, psi = tr[f]
            if v == DEV_JUMP[0] and f >= DEV_JUMP[1]:
                x = x + DEV_JUMP[2]
            row.append((f8(x), f8(y), f8(np.cos(psi)), f8(np.sin(psi)), int((v, f) == DEV_RESET)))
            pr.append(render_panel((x, y, psi), c))
            cr.append(cover_map(c, hole=(1.6, 1.0), wedge=(95.0 + 3.0 * f, 125.0 + 3.0 * f), band=3)[0])
        poses.append(row), panels.append(np.stack(pr)), covers.append(np.stack(cr))
    return c, poses, np.stack(panels), np.stack(covers)


def run_reference(c, poses, panels, covers):
    """The reference over a case -> per frame a dict(canvas [V, N, N, 4], stamp [V, N, N], state [V, 4], panel [V, gh, gw, 3],
    age [V, gh, gw])."""
    V = panels.shape[1]
    mems, out = [ref.RoadMemory(c) for _ in range(V)], []
    for f in range(panels.shape[0]):
        filled = [mems[v].step(poses[f][v], panels[f, v], covers[f, v]) for v in range(V)]
        out.append(dict(canvas=np.stack([m.canvas for m in mems]).copy(), stamp=np.stack([m.stamp for m in mems]).copy(),
                        state=np.array([m.state_row() for m in mems], np.int32), panel=np.stack([p for p, _ in filled]),
                        age=np.stack([a for _, a in filled])))
    return out


# ---- row tails: panels whose width is no multiple of the four pixels a thread makes, and a panel one pixel wide -----------------------
TAIL_WIDTHS = (37, 38, 39, 1)
TAIL_FRAMES = 6
TAIL_STARTS = [(1.07, -2.03, 0.28), (-7.31, -4.15, 2.1)]     # (chosen, like the device case's, for a margin() above 1e-6 at every width)
TAIL_STEP = (0.13, -0.03, 0.011)        # drifting towards -Y: what the rows' last pixels show was inside the panel before


def tail_case(gw):
    """-> device_case()'s tuple for two vehicles and a 40 x gw panel over TAIL_FRAMES frames.  gw = 37, 38, 39: two arcs
    like device_case()'s (the last thread of a row makes one, two or three pixels).  gw = 1: the panel is the one column on the forward axis,
    and a cell is inside it only when its centre lies on that axis to within 1/131072 pixel, so both vehicles drive along a line
    of cell centres, one along +x and one along -y (cosines exactly 0 and +-1), and the cells on that line are seen."""
    c = dict(DEV_CFG, gw=int(gw))
    if gw == 1:
        tracks = [[(0.03 + 0.13 * f, 0.05, 0.0) for f in range(TAIL_FRAMES)], [(-0.25, 0.71 - 0.13 * f, None) for f in range(TAIL_FRAMES)]]
    else:
        tracks = [arc(s, TAIL_STEP, TAIL_FRAMES) for s in TAIL_STARTS]
    poses, panels, covers = [], [], []
    for f in range(TAIL_FRAMES):
        row, pr, cr = [], [], []
        for tr in tracks:
            x, y, psi = tr[f]
            cs, sn = (f8(0.0), f8(-1.0)) if psi is None else (f8(np.cos(psi)), f8(np.sin(psi)))
            row.append((f8(x), f8(y), cs, sn, 0))
            pr.append(render_panel((x, y, -np.pi / 2 if psi is None else psi), c))
            cr.append(cover_map(c, hole=(1.6, 1.0), wedge=(95.0 + 3.0 * f, 125.0 + 3.0 * f), band=3)[0])
            cr[-1][20:27, -5:] = 0      # unseen at the rows' ends, behind road that was seen there: remembered pixels in the tails
        poses.append(row), panels.append(np.stack(pr)), covers.append(np.stack(cr))
    return c, poses, np.stack(panels), np.stack(covers)
