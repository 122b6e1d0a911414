"""Interaction tags of a camera rig (av_rig_interact): the rule table of InteractionDetector on the vehicle-frame tracks.

A tracking.RigTracker holds, per vehicle, what the one-camera tagger has to guess: positions in metres, filtered velocities on the
road, ids that survive camera hand-overs, objects beside and behind the vehicle.  RigInteractionDetector reads its state on the
device and leaves one av_interaction_row per slot and one av_interaction_summary per vehicle, the structs the tag log packs.  The
kernel is in libavhot.so; this class owns the state (the rings of lateral offsets) and the output buffers.
"""
import ctypes as C

import numpy as np

from .. import _native as nat
from .interaction_detector import _RISKS, _TYPES, Interaction, InteractionTags, class_kind

_DEFAULTS = dict(dt=1.0 / 30.0, corridor_half=1.75, adjacent_half=5.25, alongside=10.0, pass_speed=1.0, min_hits=3)


def rig_interact_cfg(class_names=None, **cfg):
    """av_rig_interact_cfg from keyword overrides of its defaults; class_names: the class names by id (None: the tracks carry the
    category itself, 1 pedestrian, 2 cyclist, 3 car / truck / bus, 4 motorcycle).  ValueError outside the library's ranges."""
    unknown = set(cfg) - set(_DEFAULTS)
    if unknown:
        raise ValueError("rig tagger: unknown setting(s) %s (known: %s)" % (sorted(unknown), sorted(_DEFAULTS)))
    c = dict(_DEFAULTS)
    c.update(cfg)
    if isinstance(c["min_hits"], bool) or not isinstance(c["min_hits"], (int, np.integer)) or not 1 <= c["min_hits"] <= 2**31 - 1:
        raise ValueError("rig tagger: min_hits is an integer >= 1")
    out = nat.RigInteractCfg()
    for k in ("dt", "corridor_half", "adjacent_half", "alongside", "pass_speed"):
        v = float(c[k])
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError("rig tagger: %s must be finite and > 0" % k)
        setattr(out, k, v)
    out.min_hits = int(c["min_hits"])
    if class_names is not None and isinstance(class_names, dict):
        class_names = [class_names.get(k, "") for k in range(16)]
    for k in range(16):
        out.class_kind[k] = (k if k < 5 else 0) if class_names is None else (class_kind(class_names[k]) if k < len(class_names) else 0)
    return out


class RigInteractionDetector:
    def __init__(self, n_vehicles, tcap, class_names=None, ctx=None, device=0, **cfg):
        """n_vehicles x tcap slots, the RigTracker's shape.  cfg: av_rig_interact_cfg's fields -- dt (1/30 s), corridor_half
        (1.75 m), adjacent_half (5.25 m), alongside (10 m), pass_speed (1 m/s), min_hits (3: the tracker's)."""
        import torch
        if int(n_vehicles) < 1:
            raise ValueError("RigInteractionDetector: n_vehicles must be >= 1")
        if not 1 <= int(tcap) <= nat.RIG_TRACK_MAX:
            raise ValueError("RigInteractionDetector: tcap is 1 .. %d" % nat.RIG_TRACK_MAX)
        self.cfg = rig_interact_cfg(class_names, **cfg)
        self.class_names = None if class_names is None else (dict(class_names) if isinstance(class_names, dict)
                                                             else dict(enumerate(class_names)))
        if not torch.cuda.is_available():
            raise RuntimeError("RigInteractionDetector needs a HIP device; this package has no CPU path")
        self.V, self.tcap = int(n_vehicles), int(tcap)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.dev = torch.device("cuda", self.ctx.device)
        d = self.dev
        self.state = torch.zeros(self.V, int(self.L.av_rig_interact_state_bytes(self.tcap)), dtype=torch.uint8, device=d)
        self.rows = torch.zeros(self.V, 1, self.tcap, nat.INTERACTION_ROW_BYTES, dtype=torch.uint8, device=d)
        self.summary = torch.zeros(self.V, 1, nat.INTERACTION_SUMMARY_BYTES, dtype=torch.uint8, device=d)
        self.reset()

    @staticmethod
    def _stream(stream):
        return stream if isinstance(stream, C.c_void_p) else nat.stream_handle(stream)

    def reset(self, stream=None):
        """Frame counter 0, every ring empty (stream-ordered)."""
        nat.check(self.L.av_rig_interact_reset(self.ctx.handle, self._stream(stream), self.V, self.tcap, nat.ptr(self.state)))

    def detect(self, tracker, plan_state, stream=None):
        """One frame: tracker (a tracking.RigTracker of this shape, or its state tensor) as its update() left it, plan_state float64
        [V, 4] (or [V, 1, 4]) -> self.rows (uint8 view of av_interaction_row [V, 1, tcap]) and self.summary ([V, 1]).  Enqueued on
        `stream`, behind the tracker's update on the same stream."""
        import torch
        state = getattr(tracker, "state", tracker)
        want = int(self.L.av_rig_track_state_bytes(self.tcap))
        if not (torch.is_tensor(state) and state.is_cuda and state.is_contiguous() and state.dtype == torch.uint8
                and state.numel() == self.V * want):
            raise ValueError("RigInteractionDetector.detect: the tracker's state is a contiguous uint8 device tensor [V, %d]" % want)
        if not (torch.is_tensor(plan_state) and plan_state.is_cuda and plan_state.is_contiguous() and plan_state.dtype == torch.float64
                and plan_state.numel() == self.V * 4 and plan_state.shape[0] == self.V and plan_state.shape[-1] == 4):
            raise ValueError("RigInteractionDetector.detect: plan_state is a contiguous float64 device tensor [V, 4]")
        nat.check(self.L.av_rig_interact(self.ctx.handle, self._stream(stream), C.byref(self.cfg), self.V, self.tcap, nat.ptr(state),
                                         nat.ptr(plan_state), nat.ptr(self.state), nat.ptr(self.rows), nat.ptr(self.summary)))
        return self.rows, self.summary

    def results(self):
        """The last detect() as one InteractionTags per vehicle: the interactions in slot order, the primary one first.
        Synchronises."""
        import torch
        torch.cuda.synchronize(self.dev)
        rows = self.rows.cpu().numpy().reshape(self.V, self.tcap, -1).view(np.dtype(nat.INTERACTION_ROW_FIELDS)).reshape(self.V, self.tcap)
        summ = self.summary.cpu().numpy().reshape(self.V, -1).view(np.dtype(nat.INTERACTION_SUMMARY_FIELDS)).reshape(self.V)
        return [decode(rows[v], summ[v], self.class_names) for v in range(self.V)]


def decode(rows, sm, class_names=None):
    """One vehicle's av_interaction_row [tcap] and av_interaction_summary (structured host arrays) -> InteractionTags."""
    tags = InteractionTags()
    inter = []
    for k in range(len(rows)):
        o = rows[k]
        if o["type"] < 0:
            continue
        ttc, cls = float(o["ttc"]), int(o["cls"])
        it = Interaction(type=_TYPES[int(o["type"])], confidence=float(o["confidence"]), risk_level=_RISKS[int(o["risk"])],
                         agent_id=int(o["agent_id"]), agent_class=None if class_names is None else class_names.get(cls),
                         distance=float(o["distance"]), relative_speed=float(o["relative_speed"]),
                         time_to_collision=None if ttc != ttc else ttc)
        if k == int(sm["primary_row"]):
            inter.insert(0, it)
        else:
            inter.append(it)
    tags.interactions = inter
    tags.agent_count, tags.pedestrian_count = int(sm["agent_count"]), int(sm["pedestrian_count"])
    tags.cyclist_count, tags.vehicle_count = int(sm["cyclist_count"]), int(sm["vehicle_count"])
    tags.closest_agent_distance = float(sm["closest_distance"])
    mt = float(sm["min_ttc"])
    tags.min_ttc = None if mt != mt else mt
    tags.timestamp = float(sm["timestamp"])
    if int(sm["primary_type"]) >= 0:
        tags.primary_interaction = _TYPES[int(sm["primary_type"])]
    tags.overall_risk = _RISKS[int(sm["overall_risk"])]
    return tags
