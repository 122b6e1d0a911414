"""Road marks on the device (csrc/roadmarks.hip: av_road_marks, perception.RoadMarks, RigLoop(marks=True)) against
tests/roadmarks_ref.py on the cases of tests/roadmarks_cases.py.

Before each frame the device state is downloaded and one restatement step is run from it; marks, sides, state and the profile words
must agree bit for bit, the two doubles of a mark row included (they are one division and one product of integers).  Every case's
margins are non-zero (asserted in tests/test_roadmarks_host.py and again here).  The free-running restatement must agree as well.
Guard bytes around the state and every output are read back unchanged."""
import ctypes as C

import numpy as np
import pytest

from tests import roadlanes_cases as lanes_cases
from tests import roadlanes_ref as lanes_ref
from tests import roadmarks_cases as cases
from tests import roadmarks_ref as ref

gpu = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    return torch, nat, nat.lib(), nat.Context(0)


def _dev(env, a):
    return env[0].as_tensor(np.ascontiguousarray(a), device=env[0].device("cuda", 0))


class Guarded:
    """nbytes of device memory between two guards of 0xAB; the payload starts as `fill` bytes."""

    def __init__(self, env, nbytes, fill=0xAB):
        self.torch, self.n = env[0], int(nbytes)
        self.t = self.torch.full((self.n + 2 * GUARD,), 0xAB, dtype=self.torch.uint8, device="cuda")
        self.payload = self.t[GUARD:GUARD + self.n]
        self.payload.fill_(fill)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + GUARD)

    def host(self, dtype=np.uint8):
        return self.payload.cpu().numpy().view(dtype)

    def guards_intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:GUARD] == 0xAB).all() and (h[GUARD + self.n:] == 0xAB).all())


def ground_rows(grounds):
    """[(ginv [9], max_range)] -> float64 [n, 20] of av_ground_cfg entries (g is not read by the stage)."""
    g = np.zeros((len(grounds), 20))
    for i, (q, max_range) in enumerate(grounds):
        g[i, 9:18], g[i, 18] = q, max_range
    return g


class Bench:
    """The buffers of one call shape, V vehicles of K cameras, and the raw entry point on them."""

    def __init__(self, env, V, K, h, w, grounds, mounts, cfg):
        torch, nat, L, ctx = env
        self.env, self.V, self.K, self.h, self.w = env, V, K, h, w
        self.cfg = nat.RoadMarksCfg(**cfg)
        self.ground, self.mounts = _dev(env, ground_rows(grounds)), _dev(env, np.asarray(mounts, np.float64).reshape(V, K, 4))
        self.frames = torch.zeros(V * K, h, w, 3, dtype=torch.uint8, device="cuda")
        self.bounds = torch.zeros(V, 8, nat.ROAD_LANE_BOUND_BYTES, dtype=torch.uint8, device="cuda")
        self.lanes = torch.zeros(V, nat.ROAD_LANES_ROW_BYTES, dtype=torch.uint8, device="cuda")
        self.state = Guarded(env, V * nat.ROAD_MARKS_STATE_BYTES, fill=0)
        self.marks = Guarded(env, V * 8 * nat.ROAD_MARK_BYTES)
        self.sides = Guarded(env, V * nat.ROAD_MARKS_ROW_BYTES)
        self.profile = Guarded(env, V * 8 * 2 * 16 * 4)
        self.outputs = (self.state, self.marks, self.sides, self.profile)

    def load(self, frames):
        """frames: one dict per vehicle (a case's frame)."""
        self.frames.copy_(_dev(self.env, np.concatenate([f["images"] for f in frames])))
        self.bounds.copy_(_dev(self.env, np.stack([f["bounds"] for f in frames]).view(np.uint8).reshape(self.V, 8, -1)))
        self.lanes.copy_(_dev(self.env, np.stack([f["lanes"] for f in frames]).view(np.uint8).reshape(self.V, -1)))

    def call(self, **over):
        torch, nat, L, ctx = self.env
        a = dict(ctx=ctx.handle, cfg=self.cfg, V=self.V, K=self.K, mounts=nat.ptr(self.mounts), ground=nat.ptr(self.ground), h=self.h, w=self.w,
                 bgr=nat.ptr(self.frames), bounds=nat.ptr(self.bounds), lanes=nat.ptr(self.lanes), state=self.state.ptr, marks=self.marks.ptr,
                 sides=self.sides.ptr, profile=self.profile.ptr)
        a.update(over)
        rc = L.av_road_marks(a["ctx"], nat.stream_handle(), C.byref(a["cfg"]) if a["cfg"] is not None else None, a["V"], a["K"], a["mounts"],
                             a["ground"], a["h"], a["w"], a["bgr"], a["bounds"], a["lanes"], a["state"], a["marks"], a["sides"], a["profile"])
        torch.cuda.synchronize()
        return rc

    def states(self):
        return self.state.host(ref.STATE_DTYPE).copy()

    def read(self):
        V = self.V
        return dict(state=self.states(), marks=self.marks.host(ref.MARK_DTYPE).reshape(V, 8).copy(), sides=self.sides.host(ref.ROW_DTYPE).copy(),
                    profile=self.profile.host(np.uint32).reshape(V, 8, 2, 16).copy())

    def snapshot(self):
        return [o.t.cpu().numpy().copy() for o in self.outputs]


def _compare(got, v, want, name, profile=True):
    """Vehicle v of a Bench.read() against one restatement step: bit for bit."""
    for b in range(8):
        for f in ref.MARK_DTYPE.names:
            assert got["marks"][v][b][f].tobytes() == want["marks"][b][f].tobytes(), (name, b, f, got["marks"][v][b], want["marks"][b])
    assert got["sides"][v].tobytes() == want["sides"].tobytes(), (name, got["sides"][v], want["sides"])
    assert got["state"][v].tobytes() == want["state"].tobytes(), (name, got["state"][v], want["state"])
    if profile:
        assert np.array_equal(got["profile"][v], want["profile"]), (name, np.argwhere(got["profile"][v] != want["profile"])[:4])


def _run(env, group, profile=True):
    """The cases of `group` (one shape, one cfg, the same number of frames) as the vehicles of one call, frame by frame."""
    first = group[0]
    V, K = len(group), first["K"]
    for c in group:
        assert (c["K"], c["h"], c["w"], c["cfg"], len(c["frames"])) == (K, first["h"], first["w"], first["cfg"], len(first["frames"]))
        d, which = cases.smallest_margin(c["name"])
        assert d > 0.0, (c["name"], which, d)
    b = Bench(env, V, K, first["h"], first["w"], [g for c in group for g in c["grounds"]], np.stack([c["mounts"] for c in group]), first["cfg"])
    free = [cases.run(c["name"]) for c in group]
    out = []
    for i in range(len(first["frames"])):
        frames = [c["frames"][i] for c in group]
        before = b.states()
        b.load(frames)
        assert b.call(**({} if profile else dict(profile=None))) == 0, env[2].av_last_error_string()
        got = b.read()
        for v, c in enumerate(group):
            fr = frames[v]
            want = ref.step(c["cfg"], c["grounds"], c["mounts"], fr["images"], fr["bounds"], fr["lanes"], before[v])
            _compare(got, v, want, (c["name"], i), profile)
            _compare(got, v, free[v][i], (c["name"], i, "free-running"), profile)
        assert all(o.guards_intact() for o in b.outputs), (first["name"], i)
        out.append(got)
    return b, out


@gpu
@pytest.mark.parametrize("name", [c["name"] for c in cases.cases()])
def test_one_vehicle(env, name):
    """Every case on its own: the rendered roads; 1, 63, 64, 65, 256, 257 and 512 samples; 1, 2 and 8 cameras; 0, 1 and 8
    boundaries; frames of 2 x 2, 5 x 1 and 1 x 5 pixels (the sample's unpacked form below two columns); a quarter-turned mount; a far
    half no camera sees; an extent that cuts the sample grid; a camera above the horizon; painted stripes; and the sequences, frame
    by frame."""
    _run(env, [cases.by_name(name)])


@gpu
def test_three_vehicles_in_one_call(env):
    """An indexing error in v shows: 0, 1 and 8 live boundaries side by side, each vehicle with its own noise."""
    b, out = _run(env, [cases.by_name(n) for n in ("bounds_0", "bounds_1", "bounds_8")])
    got = out[0]
    assert not got["marks"][0].view(np.uint8).any() and not got["profile"][0].any() and got["marks"][2]["n_seen"].all()
    assert got["sides"]["right"]["bound"].tolist() == [-1, 0, 0]


@gpu
def test_profile_null(env):
    """profile = NULL: the same rows, and the profile's memory is not touched."""
    b, out = _run(env, [cases.by_name("dashed_white")], profile=False)
    assert (b.profile.host() == 0xAB).all()


@gpu
def test_refusals_leave_everything_untouched(env):
    torch, nat, L, ctx = env
    c = cases.by_name("solid_yellow")
    b = Bench(env, 1, 2, c["h"], c["w"], c["grounds"], c["mounts"][None], c["cfg"])
    b.load(c["frames"])
    assert b.call() == 0
    before = b.snapshot()
    EINVAL = L.av_road_marks_check(None)
    bad = [nat.RoadMarksCfg(**dict(c["cfg"], **kw)) for kw in (dict(n_samples=513), dict(ds=0.0), dict(core=9), dict(gap_dash=0.1))]
    for over in [dict(ctx=None), dict(cfg=None)] + [dict(cfg=x) for x in bad] + [
            dict(V=0), dict(V=65536), dict(K=0), dict(K=9), dict(h=0), dict(w=0), dict(h=32769), dict(w=32769), dict(mounts=None),
            dict(ground=None), dict(bgr=None), dict(bounds=None), dict(lanes=None), dict(state=None), dict(marks=None), dict(sides=None)]:
        assert b.call(**over) == EINVAL, over
        assert all(np.array_equal(x, y) for x, y in zip(before, b.snapshot())), over
    assert b.states()["frames"][0] == 1


@gpu
def test_the_class_with_views_into_larger_tensors_and_reset(env):
    """perception.RoadMarks.update on a slice of a larger frame tensor and on boundary and lane rows that lie inside larger
    buffers, against the raw entry on tensors of their own, bit for bit; reset(vehicle) and reset()."""
    torch, nat, L, ctx = env
    from multimodal_autonomous_driving_perception_and_planning_amd.perception import RoadMarks
    a, c = cases.by_name("solid_white"), cases.by_name("dashed_yellow")
    rig, V, K = cases.rig_of(cases.POSES), 2, 2
    rm = RoadMarks(rig, V, cases.H, cases.W, ctx=ctx, hold=2)
    b = Bench(env, V, K, cases.H, cases.W, a["grounds"] * V, np.stack([a["mounts"]] * V), ref.cfg_of(hold=2))
    assert np.array_equal(rm.mounts.cpu().numpy()[0], a["mounts"])
    assert np.array_equal(rm.ground.cpu().numpy().view(np.float64)[:, 9:19], ground_rows(a["grounds"] * V)[:, 9:19])
    big = torch.full((V * K + 3, cases.H, cases.W, 3), 7, dtype=torch.uint8, device="cuda")
    rows = torch.full((5 * V * 8 * 64,), 0xCD, dtype=torch.uint8, device="cuda")
    frames, bounds = big[2:2 + V * K], rows[128:128 + V * 8 * 64].view(V, 8, 64)
    lanes = rows[2048:2048 + V * 128].view(V, 128)
    assert frames.data_ptr() != big.data_ptr() and bounds.data_ptr() != rows.data_ptr()

    def same():
        got = b.read()
        assert rm.marks().tobytes() == got["marks"].tobytes() and rm.sides().tobytes() == got["sides"].tobytes()
        assert rm.states().tobytes() == got["state"].tobytes() and rm.profile.cpu().numpy().view(np.uint32).tobytes() == got["profile"].tobytes()
        return got

    for i in range(3):
        b.load([a["frames"][0], c["frames"][0]])
        frames.copy_(b.frames), bounds.copy_(b.bounds), lanes.copy_(b.lanes)
        assert b.call() == 0
        rm.update(frames, bounds, lanes)
        got = same()
    assert got["sides"]["left"]["type"].tolist() == [ref.SOLID, ref.DASHED] and got["sides"]["left"]["colour"].tolist() == [ref.WHITE, ref.YELLOW]
    assert got["sides"]["may_change_left"].tolist() == [0, 1] and got["sides"]["may_change_right"].tolist() == [1, 0]
    prof = rm.profiles()
    assert prof.shape == (V, 8, 2, 210) and prof[0, 0, 1].sum() == got["marks"][0][0]["n_paint"] and prof[1, 1, 0].sum() == got["marks"][1][1]["n_seen"]
    assert (big[:2] == 7).all() and (big[2 + V * K:] == 7).all() and (rows[:128] == 0xCD).all()       # read in place, nothing written
    for vehicle in (1, None):
        rm.reset(vehicle)
        assert L.av_road_marks_reset(ctx.handle, nat.stream_handle(), V, -1 if vehicle is None else vehicle, b.state.ptr) == 0
        torch.cuda.synchronize()
        st = b.states()
        assert rm.states().tobytes() == st.tobytes() and b.state.guards_intact()
        assert st["frames"][1] == 0 and not st[1:].view(np.uint8).any() and (st["frames"][0] == 0) == (vehicle is None)
        b.call(), rm.update(frames, bounds, lanes)
        got = same()
        assert got["state"]["frames"][1] == 1 and got["sides"]["left"]["type"][1] == ref.UNKNOWN and got["sides"]["left"]["run"][1] == 1
    with pytest.raises(ValueError, match="frames"):
        rm.update(big[:V * K, :, :100], bounds, lanes)
    with pytest.raises(ValueError, match="bounds"):
        rm.update(frames, bounds[:1], lanes)
    with pytest.raises(ValueError, match="lanes"):
        rm.update(frames, bounds, rows[2049:2049 + V * 128])


# ---- RigLoop(lanes="road", marks=True) ---------------------------------------------------------------------------------------------
NEW_KEYS = ("lane_mark_left", "lane_mark_right", "lane_colour_left", "lane_colour_right", "may_change_left", "may_change_right", "bound_marks")


@gpu
def test_rig_loop_reads_a_solid_yellow_and_a_dashed_white_line(env):
    """A rendered 720 x 1280 road, solid yellow on the left and dashed white on the right, through the whole loop -- frames, the
    lane chain, av_road_lanes, av_road_marks -- for `hold` frames: the lane is found, and both sides publish what is painted."""
    torch, nat, L, ctx = env
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import RigLoop
    rig, hold = lanes_cases.render_rig(), ref.DEFAULT_CFG["hold"]
    frames = _dev(env, cases.e2e_frames(*cases.E2E_PATTERN))
    loop = RigLoop(1, rig, h=lanes_cases.RENDER_H, w=lanes_cases.RENDER_W, lanes="road", marks=True, tracker_kw=dict(min_hits=1))
    assert loop.road_marks.cfg.hold == hold and loop.road_marks.ctx is loop.ego.ctx
    for i in range(hold):
        loop.step(frames=frames, sync=True)
        r = loop.results()
        print("frame", i, "status", r["lane_status"], "left", r["lane_left"], "right", r["lane_right"], "sides",
              loop.road_marks.sides(), "marks", r["bound_marks"][0][:int(loop.road_lanes.lanes()[0]["n_bounds"])])
        assert r["lane_status"][0] & lanes_ref.LANE, r["lane_status"]
        assert r["lane_mark_left"][0] == (ref.SOLID if i == hold - 1 else ref.UNKNOWN)
    assert set(NEW_KEYS) <= set(r) and r["bound_marks"].shape == (1, 8) and r["bound_marks"].dtype == ref.MARK_DTYPE
    assert (r["lane_mark_left"][0], r["lane_colour_left"][0]) == (ref.SOLID, ref.YELLOW)
    assert (r["lane_mark_right"][0], r["lane_colour_right"][0]) == (ref.DASHED, ref.WHITE)
    assert r["may_change_left"][0] == 0 and r["may_change_right"][0] == 1
    # the loop's rows are the stand-alone call's on the loop's own tables, frames and boundaries
    rm, rl = loop.road_marks, loop.road_lanes
    state, marks, sides = Guarded(env, 64, fill=0), Guarded(env, 8 * 64), Guarded(env, 64)
    nat.check(L.av_road_marks(ctx.handle, None, C.byref(rm.cfg), 1, rig.K, nat.ptr(rm.mounts), nat.ptr(rm.ground), loop.h, loop.w,
                              nat.ptr(loop.cams.cam.frames), nat.ptr(rl.bound_rows), nat.ptr(rl.rows), state.ptr, marks.ptr, sides.ptr, None))
    torch.cuda.synchronize()
    assert marks.host().tobytes() == r["bound_marks"].tobytes() and all(o.guards_intact() for o in (state, marks, sides))


@gpu
def test_rig_loop_without_marks_is_the_parent(env):
    """marks=False: no new key in results(), no RoadMarks, and enqueue_road_marks refuses by name."""
    torch, nat, L, ctx = env
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import RigLoop
    from tests import test_gpu_rigflow as tf
    kw = dict(lanes="road", h=tf.LOOP_H, w=tf.LOOP_W, tracker_kw=dict(min_hits=1))
    off, default, on = RigLoop(1, tf._loop_rig(), marks=False, **kw), RigLoop(1, tf._loop_rig(), **kw), RigLoop(1, tf._loop_rig(), marks=True, **kw)
    for lp in (off, default, on):
        lp.step(sync=True)
    ro, rd, rn = off.results(), default.results(), on.results()
    assert off.road_marks is None and default.road_marks is None and on.road_marks is not None
    assert sorted(ro) == sorted(rd) == sorted(set(rn) - set(NEW_KEYS)) and set(NEW_KEYS) <= set(rn)
    for name in ("wp", "cost", "order", "ref_paths", "n_ref", "lane_offset", "lane_status"):
        assert np.array_equal(ro[name], rd[name], equal_nan=True) and np.array_equal(ro[name], rn[name], equal_nan=True), name
    with pytest.raises(RuntimeError, match="marks=True"):
        off.enqueue_road_marks()
