"""TagLog -- AutoTagger's bookkeeping (src/tagging/auto_tagger.py:112-310) for S streams, resident on the device.

A logged frame is one 64-bit mask over the fixed vocabulary TAGS (include/avhot.h: AV_TAG_*) plus the frame's speed.  The
log is appended by av_tags_pack + av_taglog_append from the three taggers' rows in HBM (HotLoop.enqueue_tags,
CameraLoop(tags=...)) and queried by kernels (av_taglog_search / _segments / _stats); only the answers come back to the host.
The query surface carries the reference's names with a stream axis added; searches return frame indices, not FrameTags.
"""
import ctypes as C

import numpy as np
import torch

from .. import _native as nat
from .interaction_detector import InteractionType, RiskLevel
from .maneuver_detector import LateralManeuver, LongitudinalManeuver, TurningManeuver
from .scene_classifier import _ELEMENT_OF, Condition, RoadType, TrafficElement

# base bit of every group (include/avhot.h: AV_TAG_*)
ROAD_TYPE, ELEMENT, CONDITION, PEDESTRIAN_AREA, LATERAL, LONGITUDINAL, TURNING, INTERACTION, RISK = 0, 6, 11, 17, 18, 22, 27, 33, 46
HAS_SCENE, HAS_MANEUVER, HAS_INTERACTION = 61, 62, 63

# the 49 tags in bit order: each Enum in the reference's definition order
TAGS = tuple([e.value for e in RoadType] + [e.value for e in TrafficElement] + [e.value for e in Condition] + ["pedestrian_area"] +
             [e.value for e in LateralManeuver] + [e.value for e in LongitudinalManeuver] + [e.value for e in TurningManeuver] +
             [e.value for e in InteractionType] + ["risk_%s" % e.value for e in list(RiskLevel)[1:]])
_BIT = {t: k for k, t in enumerate(TAGS)}
_RISKS = [e.value for e in RiskLevel]


def tag_mask(names):
    """The mask of a list of tag strings.  A string outside the vocabulary contributes no bit."""
    m = 0
    for t in names:
        k = _BIT.get(t)
        if k is not None:
            m |= 1 << k
    return m


def tags_of(mask):
    """The tag strings of a mask in vocabulary order (presence flags and reserved bits are not tags)."""
    mask = int(mask)
    return [t for k, t in enumerate(TAGS) if (mask >> k) & 1]


def element_table(class_names):
    """av_tags_pack's elem_table from a detector's class names (a list, or a dict id -> name): TrafficElement index + 1 where the
    reference turns a detection into a traffic element (its literal 'traffic_light' / 'stop_sign', as category_table), else 0."""
    elems = list(TrafficElement)
    if isinstance(class_names, dict):
        n = max(class_names) + 1 if class_names else 0
        class_names = [class_names.get(k) for k in range(n)]
    return np.array([elems.index(_ELEMENT_OF[c]) + 1 if c in _ELEMENT_OF else 0 for c in class_names], np.uint8)


def _predicate(tags, match_all):
    """(all, any, none) of search_by_tags, or None where no frame can match: an unknown tag under match_all, no known tag under
    match-any (`tag in ft.all_tags` is False for every frame)."""
    known = [t for t in tags if t in _BIT]
    if match_all:
        return None if len(known) != len(tags) else (tag_mask(known), 0, 0)
    return (0, tag_mask(known), 0) if known else None


class TagLog:
    """mask u64 [S][cap] (held as int64), speed f64 [S][cap], log_n int32 [S], dropped int32 [S] on the device."""

    def __init__(self, n_streams, capacity, device=0, ctx=None, stream=None):
        """stream: the torch stream appends and queries run on (None: torch's current stream at the time of the call)."""
        if not torch.cuda.is_available():
            raise RuntimeError("TagLog needs a HIP device; this package has no CPU path")
        if n_streams <= 0 or capacity <= 0:
            raise ValueError("n_streams and capacity must be > 0")
        self.S, self.cap = int(n_streams), int(capacity)
        self.dev = torch.device("cuda", device)
        self.ctx = ctx or nat.default_context(device)
        self.L = nat.lib()
        self.stream = stream
        d = self.dev
        self.mask = torch.zeros(self.S, self.cap, dtype=torch.int64, device=d)
        self.speed = torch.zeros(self.S, self.cap, dtype=torch.float64, device=d)
        self.log_n = torch.zeros(self.S, dtype=torch.int32, device=d)
        self.dropped = torch.zeros(self.S, dtype=torch.int32, device=d)
        self.ws = torch.zeros(int(self.L.av_taglog_workspace_bytes(self.S, self.cap)), dtype=torch.uint8, device=d)
        self._stats = torch.zeros(self.S, nat.TAGLOG_STATS_BYTES, dtype=torch.uint8, device=d)
        self._out_n = torch.zeros(self.S, dtype=torch.int32, device=d)
        self._out = {}                     # per query kind: the output buffer, grown on demand
        self._win = None                   # pack_and_append's [S][W] masks and speeds
        torch.cuda.current_stream(d).synchronize()      # the zero fills above, before a kernel on another stream meets them

    # ---- streams ---------------------------------------------------------------------------------------------------
    def _torch_stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    def _s(self, stream=None):
        return stream if stream is not None else C.c_void_p(self._torch_stream().cuda_stream)

    def _to_dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            if a.dtype != dtype or a.device != self.dev or not a.is_contiguous():
                raise ValueError("device input must be a contiguous %s tensor on %s" % (dtype, self.dev))
            return a
        a = np.ascontiguousarray(a, np.uint64 if dtype == torch.int64 else np.float64)
        with torch.cuda.stream(self._torch_stream()):
            return torch.from_numpy(a.view(np.int64) if dtype == torch.int64 else a).to(self.dev)

    # ---- writing ---------------------------------------------------------------------------------------------------
    def append(self, masks, speeds, stream=None):
        """masks u64 / speeds f64 [S, W] (NumPy, or device tensors: int64 bit patterns / float64) behind every stream's log_n.
        Frames that do not fit are counted in `dropped`, not written.  Stream-ordered, no synchronisation."""
        m, v = self._to_dev(masks, torch.int64), self._to_dev(speeds, torch.float64)
        if m.dim() != 2 or m.shape[0] != self.S or tuple(v.shape) != tuple(m.shape):
            raise ValueError("masks and speeds are [n_streams, W]")
        nat.check(self.L.av_taglog_append(self.ctx.handle, self._s(stream), self.S, int(m.shape[1]), nat.ptr(m), nat.ptr(v), self.cap,
                                          nat.ptr(self.mask), nat.ptr(self.speed), nat.ptr(self.log_n), nat.ptr(self.dropped)))

    def pack_and_append(self, window, maneuver=None, inter_rows=None, inter_summary=None, snap_n=None, scene_rows=None,
                        det_n=None, det_cls=None, elem_table=None, stream=None):
        """The taggers' rows of [S][window] frames (device tensors, uint8 views of the row structs as the stages leave them; each
        group may be None) -> masks and speeds (av_tags_pack) -> the log.  The window's masks stay in self.win_mask / win_speed."""
        W = int(window)
        if self._win is None or self._win[0].shape[1] != W:
            self._win = (torch.empty(self.S, W, dtype=torch.int64, device=self.dev),
                         torch.empty(self.S, W, dtype=torch.float64, device=self.dev))
        wm, wv = self._win
        max_det = int(det_cls.shape[-1]) if det_cls is not None else 0
        n_elem = int(elem_table.numel()) if elem_table is not None else 0
        tcap = int(inter_rows.shape[2]) if inter_rows is not None else 0
        st = self._s(stream)
        nat.check(self.L.av_tags_pack(self.ctx.handle, st, self.S, W, nat.ptr(maneuver), nat.ptr(inter_rows), nat.ptr(inter_summary),
                                      nat.ptr(snap_n), tcap, nat.ptr(scene_rows), nat.ptr(det_n), nat.ptr(det_cls), max_det,
                                      nat.ptr(elem_table), n_elem, nat.ptr(wm), nat.ptr(wv)))
        self.append(wm, wv, stream=st)

    @property
    def win_mask(self):
        return None if self._win is None else self._win[0]

    @property
    def win_speed(self):
        return None if self._win is None else self._win[1]

    def reset(self):
        with torch.cuda.stream(self._torch_stream()):
            self.log_n.zero_()
            self.dropped.zero_()

    # ---- reading ---------------------------------------------------------------------------------------------------
    def _sync(self):
        self._torch_stream().synchronize()

    def lengths(self):
        """Frames logged per stream (synchronises)."""
        self._sync()
        return self.log_n.cpu().numpy()

    def __len__(self):
        return int(self.lengths().max())

    def masks(self, stream):
        """The logged masks of one stream as uint64 (synchronises)."""
        n = int(self.lengths()[stream])
        return self.mask[stream, :n].cpu().numpy().view(np.uint64)

    def speeds(self, stream):
        n = int(self.lengths()[stream])
        return self.speed[stream, :n].cpu().numpy()

    def _query(self, kind, width, call, stream):
        """Runs `call(cap, out)` with an output of `cap` rows per stream, again with a larger one while out_n says rows were cut."""
        cap = self._out[kind].shape[1] if kind in self._out else 256
        while True:
            if kind not in self._out or self._out[kind].shape[1] != cap:
                self._out[kind] = torch.empty(self.S, cap, width, dtype=torch.int32, device=self.dev)
            out = self._out[kind]
            call(cap, out)
            self._sync()
            n = self._out_n.cpu().numpy()
            if int(n.max()) <= cap:
                break
            cap = int(n.max())
        host = out.cpu().numpy()
        res = [host[s, :n[s]].reshape(-1) if width == 1 else host[s, :n[s]].copy() for s in range(self.S)]
        return res if stream is None else res[stream]

    def _empty(self, width, stream):
        res = [np.zeros((0,) if width == 1 else (0, width), np.int32) for _ in range(self.S)]
        return res if stream is None else res[stream]

    def search_masks(self, all_=0, any_=0, none=0, stream=None, first=0, last=None):
        """Frame indices with (m & all_) == all_, (any_ == 0 or m & any_) and not m & none, inside [first, last): one int32
        array for a given stream, a list of S for None."""
        last = self.cap if last is None else int(last)

        def call(cap, out):
            nat.check(self.L.av_taglog_search(self.ctx.handle, self._s(), self.S, self.cap, nat.ptr(self.mask), nat.ptr(self.log_n),
                                              all_, any_, none, int(first), last, nat.ptr(self.ws), cap, nat.ptr(out),
                                              nat.ptr(self._out_n)))
        return self._query("search", 1, call, stream)

    def segment_masks(self, all_=0, any_=0, none=0, min_duration=5, stream=None, first=0, last=None):
        """Maximal runs of matching frames at least min_duration long: int32 [n, 2] (first, last) per stream."""
        last = self.cap if last is None else int(last)

        def call(cap, out):
            nat.check(self.L.av_taglog_segments(self.ctx.handle, self._s(), self.S, self.cap, nat.ptr(self.mask), nat.ptr(self.log_n),
                                                all_, any_, none, int(first), last, int(min_duration), nat.ptr(self.ws), cap,
                                                nat.ptr(out), nat.ptr(self._out_n)))
        return self._query("segments", 2, call, stream)

    def search_by_tag(self, tag, stream=None):
        return self.search_by_tags([tag], True, stream)

    def search_by_tags(self, tags, match_all=True, stream=None):
        """[] matches every frame under match_all and none otherwise, like all([]) / any([])."""
        p = _predicate(list(tags), match_all)
        return self._empty(1, stream) if p is None else self.search_masks(*p, stream=stream)

    def get_high_risk_frames(self, stream=None):
        return self.search_masks(any_=tag_mask(["risk_high", "risk_critical"]), stream=stream)

    def get_event_segments(self, event_tag, min_duration=5, stream=None):
        """(first, last) frame index pairs, int32 [n, 2] per stream."""
        p = _predicate([event_tag], True)
        return self._empty(2, stream) if p is None else self.segment_masks(*p, min_duration=min_duration, stream=stream)

    def stats_rows(self):
        """av_taglog_stats_row of every stream (structured NumPy array [S]; synchronises)."""
        nat.check(self.L.av_taglog_stats(self.ctx.handle, self._s(), self.S, self.cap, nat.ptr(self.mask), nat.ptr(self.speed),
                                         nat.ptr(self.log_n), nat.ptr(self.ws), nat.ptr(self._stats)))
        self._sync()
        return self._stats.cpu().numpy().view(np.dtype(nat.TAGLOG_STATS_FIELDS)).reshape(self.S)

    def get_tag_statistics(self, stream):
        """The reference's dict without session_info; {} for an empty log.  tag_frequency: the 20 most frequent tags,
        count-descending, ties in vocabulary order."""
        return statistics_dict(self.stats_rows()[stream])


def statistics_dict(row):
    """get_tag_statistics' dict (auto_tagger.py:210-250, without session_info) from one av_taglog_stats_row."""
    n = int(row["n_frames"])
    if n == 0:
        return {}
    counts = {t: int(row["tag_count"][k]) for k, t in enumerate(TAGS) if row["tag_count"][k] > 0}
    freq = sorted(counts.items(), key=lambda kv: -kv[1])                        # stable: ties stay in vocabulary order
    nm = int(row["n_maneuver"])
    return {'total_frames': n, 'unique_tags': len(counts), 'tag_frequency': {t: c / n for t, c in freq[:20]},
            'tag_counts': counts,
            'speed_stats': {'min': float(row["speed_min"]) if nm else 0, 'max': float(row["speed_max"]) if nm else 0,
                            'avg': float(row["speed_sum"]) / nm if nm else 0},
            'risk_distribution': {r: int(row["risk_count"][k]) for k, r in enumerate(_RISKS)}}
