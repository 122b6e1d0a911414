"""TagLog -- AutoTagger's bookkeeping (src/tagging/auto_tagger.py:112-310) for S streams, resident on the device.

A logged frame is one 64-bit mask over the fixed vocabulary TAGS (include/avhot.h: AV_TAG_*) plus the frame's speed.  The
log is appended by av_tags_pack + av_taglog_append_ex from the three taggers' rows in HBM (HotLoop.enqueue_tags,
CameraLoop(tags=...)) and queried by kernels (av_taglog_search_where / _segments_where / _stats); only the answers come back to the host.
The query surface carries the reference's names with a stream axis added; searches return frame indices, not FrameTags.

TagLog(columns=True) also keeps a record per frame (av_taglog_cols: the confidences, the acceleration, min_ttc, the closest
distance and the agent counts of the taggers' rows), which search_where / segments_where bound numerically, records /
records_where bring back, and frame_dict turns into the FrameTags.to_dict() shape that database.TagDatabase stores.
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
_GROUPS = {"road_type": (ROAD_TYPE, 6), "lateral": (LATERAL, 4), "longitudinal": (LONGITUDINAL, 5), "turning": (TURNING, 6)}
COLS_DTYPE = np.dtype(nat.TAGLOG_COLS_FIELDS)


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


def _range(r):
    """None, or (lo, hi) with None for an open end -> the two bounds as doubles, NaN = unset."""
    lo, hi = (None, None) if r is None else r
    return (float("nan") if lo is None else float(lo)), (float("nan") if hi is None else float(hi))


def _where(tags=(), match_all=True, none=(), speed=None, acceleration=None, max_ttc=None, max_distance=None, min_agents=0,
           min_pedestrians=0, min_cyclists=0, min_vehicles=0):
    """(av_taglog_where or None where no frame can match -- see _predicate --, whether a bound on a record's field is set)."""
    p = _predicate(list(tags), match_all)
    q = nat.TaglogWhere()
    if p is not None:
        q.all, q.any = p[0], p[1]
    q.none = tag_mask(none)
    q.speed_min, q.speed_max = _range(speed)
    q.accel_min, q.accel_max = _range(acceleration)
    q.ttc_max, q.distance_max = _range((None, max_ttc))[1], _range((None, max_distance))[1]
    q.agents_min, q.pedestrians_min, q.cyclists_min, q.vehicles_min = (int(min_agents), int(min_pedestrians), int(min_cyclists),
                                                                        int(min_vehicles))
    counts = max(q.agents_min, q.pedestrians_min, q.cyclists_min, q.vehicles_min) > 0
    on_cols = counts or any(v == v for v in (q.accel_min, q.accel_max, q.ttc_max, q.distance_max))
    return (None if p is None else q), on_cols


class TagLog:
    """mask u64 [S][cap] (held as int64), speed f64 [S][cap], log_n int32 [S], dropped int32 [S] on the device; with columns=True
    also cols, av_taglog_cols [S][cap] held as uint8 [S, cap, 80]."""

    def __init__(self, n_streams, capacity, device=0, ctx=None, stream=None, columns=False):
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
        self.columns = bool(columns)
        self.cols = torch.zeros(self.S, self.cap, nat.TAGLOG_COLS_BYTES, dtype=torch.uint8, device=d) if self.columns else None
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
    def _cols_to_dev(self, cols, W):
        if isinstance(cols, torch.Tensor):
            if cols.dtype != torch.uint8 or cols.device != self.dev or not cols.is_contiguous():
                raise ValueError("device records must be a contiguous uint8 tensor on %s" % self.dev)
            c = cols
        else:
            a = np.ascontiguousarray(cols)
            if a.dtype != COLS_DTYPE:
                raise ValueError("host records are a structured array of _native.TAGLOG_COLS_FIELDS")
            with torch.cuda.stream(self._torch_stream()):
                c = torch.from_numpy(a.view(np.uint8).reshape(a.shape + (nat.TAGLOG_COLS_BYTES,)).copy()).to(self.dev)
        if tuple(c.shape) != (self.S, W, nat.TAGLOG_COLS_BYTES):
            raise ValueError("records are [n_streams, W] (as uint8: [n_streams, W, %d])" % nat.TAGLOG_COLS_BYTES)
        return c

    def append(self, masks, speeds, cols=None, stream=None):
        """masks u64 / speeds f64 [S, W] (NumPy, or device tensors: int64 bit patterns / float64) behind every stream's log_n; for
        a log with columns also cols, the frames' records (uint8 [S, W, 80] on the device, or a structured host array [S, W]).
        Frames that do not fit are counted in `dropped`, not written.  Stream-ordered, no synchronisation."""
        m, v = self._to_dev(masks, torch.int64), self._to_dev(speeds, torch.float64)
        if m.dim() != 2 or m.shape[0] != self.S or tuple(v.shape) != tuple(m.shape):
            raise ValueError("masks and speeds are [n_streams, W]")
        if (cols is not None) != self.columns:
            raise ValueError("a log with columns takes the frames' records with every append, a log without takes none")
        c = self._cols_to_dev(cols, int(m.shape[1])) if self.columns else None
        nat.check(self.L.av_taglog_append_ex(self.ctx.handle, self._s(stream), self.S, int(m.shape[1]), nat.ptr(m), nat.ptr(v),
                                             nat.ptr(c), self.cap, nat.ptr(self.mask), nat.ptr(self.speed), nat.ptr(self.cols),
                                             nat.ptr(self.log_n), nat.ptr(self.dropped)))

    def pack_and_append(self, window, maneuver=None, inter_rows=None, inter_summary=None, snap_n=None, scene_rows=None,
                        det_n=None, det_cls=None, elem_table=None, stream=None):
        """The taggers' rows of [S][window] frames (device tensors, uint8 views of the row structs as the stages leave them; each
        group may be None) -> masks and speeds (av_tags_pack) and, for a log with columns, records (av_tags_cols) -> the log.  The
        window's masks, speeds and records stay in self.win_mask / win_speed / win_cols.  Interaction rows with snap_n=None are
        slot-indexed ([S][window][tcap] with any tcap in 1 .. 512, av_rig_interact's) and go through av_tags_pack_slots, which takes
        no scene group."""
        W = int(window)
        if self._win is None or self._win[0].shape[1] != W:
            self._win = (torch.empty(self.S, W, dtype=torch.int64, device=self.dev),
                         torch.empty(self.S, W, dtype=torch.float64, device=self.dev),
                         torch.empty(self.S, W, nat.TAGLOG_COLS_BYTES, dtype=torch.uint8, device=self.dev) if self.columns else None)
        wm, wv, wc = self._win
        max_det = int(det_cls.shape[-1]) if det_cls is not None else 0
        n_elem = int(elem_table.numel()) if elem_table is not None else 0
        tcap = int(inter_rows.shape[2]) if inter_rows is not None else 0
        st = self._s(stream)
        if inter_rows is not None and snap_n is None:
            if scene_rows is not None or det_n is not None or det_cls is not None or elem_table is not None:
                raise ValueError("slot-indexed interaction rows (snap_n=None) come without a scene group")
            nat.check(self.L.av_tags_pack_slots(self.ctx.handle, st, self.S, W, nat.ptr(maneuver), nat.ptr(inter_rows),
                                                nat.ptr(inter_summary), tcap, nat.ptr(wm), nat.ptr(wv)))
        else:
            nat.check(self.L.av_tags_pack(self.ctx.handle, st, self.S, W, nat.ptr(maneuver), nat.ptr(inter_rows), nat.ptr(inter_summary),
                                          nat.ptr(snap_n), tcap, nat.ptr(scene_rows), nat.ptr(det_n), nat.ptr(det_cls), max_det,
                                          nat.ptr(elem_table), n_elem, nat.ptr(wm), nat.ptr(wv)))
        if self.columns:
            nat.check(self.L.av_tags_cols(self.ctx.handle, st, self.S, W, nat.ptr(maneuver), nat.ptr(inter_summary),
                                          nat.ptr(scene_rows), nat.ptr(wc)))
        self.append(wm, wv, wc, stream=st)

    @property
    def win_mask(self):
        return None if self._win is None else self._win[0]

    @property
    def win_speed(self):
        return None if self._win is None else self._win[1]

    @property
    def win_cols(self):
        return None if self._win is None else self._win[2]

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

    def records_of(self, stream):
        """The logged records of one stream as a structured array of _native.TAGLOG_COLS_FIELDS (None without columns)."""
        if not self.columns:
            return None
        n = int(self.lengths()[stream])
        return self.cols[stream, :n].cpu().numpy().reshape(-1).view(COLS_DTYPE)

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

    def _run(self, q, stream, first, last, min_duration=None):
        """The search (min_duration None) or the segment query of the av_taglog_where `q`, through _query."""
        last = self.cap if last is None else int(last)
        head = lambda: (self.ctx.handle, self._s(), self.S, self.cap, nat.ptr(self.mask), nat.ptr(self.speed),  # noqa: E731
                        nat.ptr(self.cols), nat.ptr(self.log_n), C.byref(q), int(first), last)

        def search(cap, out):
            nat.check(self.L.av_taglog_search_where(*head(), nat.ptr(self.ws), cap, nat.ptr(out), nat.ptr(self._out_n)))

        def segments(cap, out):
            nat.check(self.L.av_taglog_segments_where(*head(), int(min_duration), nat.ptr(self.ws), cap, nat.ptr(out),
                                                      nat.ptr(self._out_n)))
        if min_duration is None:
            return self._query("search", 1, search, stream)
        return self._query("segments", 2, segments, stream)

    def search_masks(self, all_=0, any_=0, none=0, stream=None, first=0, last=None):
        """Frame indices with (m & all_) == all_, (any_ == 0 or m & any_) and not m & none, inside [first, last): one int32
        array for a given stream, a list of S for None."""
        q = _where()[0]                     # every bound unset
        q.all, q.any, q.none = all_, any_, none
        return self._run(q, stream, first, last)

    def segment_masks(self, all_=0, any_=0, none=0, min_duration=5, stream=None, first=0, last=None):
        """Maximal runs of matching frames at least min_duration long: int32 [n, 2] (first, last) per stream."""
        q = _where()[0]
        q.all, q.any, q.none = all_, any_, none
        return self._run(q, stream, first, last, int(min_duration))

    # ---- numeric queries and records -----------------------------------------------------------------------------------
    def _run_where(self, stream, first, last, min_duration, *where, **where_kw):
        """_run of _where(*where, **where_kw); None where no frame can match (see _predicate)."""
        q, on_cols = _where(*where, **where_kw)
        if on_cols and not self.columns:
            raise ValueError("a bound on acceleration, TTC, distance or an agent count needs TagLog(columns=True)")
        return None if q is None else self._run(q, stream, first, last, min_duration)

    def search_where(self, tags=(), match_all=True, none=(), speed=None, acceleration=None, max_ttc=None, max_distance=None,
                     min_agents=0, min_pedestrians=0, min_cyclists=0, min_vehicles=0, stream=None, first=0, last=None):
        """Frame indices carrying `tags` (all of them, or any under match_all=False; unknown tags as in search_by_tags) and none of
        `none`, with speed / acceleration inside (lo, hi) (None = open end), min_ttc <= max_ttc, closest distance <= max_distance
        and at least the given agent counts.  A frame without the bounded value (min_ttc None, no maneuver row) does not match."""
        res = self._run_where(stream, first, last, None, tags, match_all, none, speed, acceleration, max_ttc, max_distance, min_agents,
                              min_pedestrians, min_cyclists, min_vehicles)                # _where's order
        return self._empty(1, stream) if res is None else res

    def segments_where(self, tags=(), match_all=True, none=(), speed=None, acceleration=None, max_ttc=None, max_distance=None,
                       min_agents=0, min_pedestrians=0, min_cyclists=0, min_vehicles=0, stream=None, first=0, last=None,
                       min_duration=5):
        """Maximal runs of frames matching search_where's predicate, at least min_duration long: int32 [n, 2] per stream."""
        res = self._run_where(stream, first, last, int(min_duration), tags, match_all, none, speed, acceleration, max_ttc, max_distance,
                              min_agents, min_pedestrians, min_cyclists, min_vehicles)
        return self._empty(2, stream) if res is None else res

    def record_dtype(self):
        """(frame_idx, mask, speed, then the record's fields for a log with columns)."""
        return np.dtype([("frame_idx", "<i4"), ("mask", "<u8"), ("speed", "<f8")] + (nat.TAGLOG_COLS_FIELDS if self.columns else []))

    def _gather(self, idx, idx_n, counts):
        """av_taglog_gather of the device indices idx int32 [S, idx_cap(, 1)] / idx_n [S] -> one structured array per stream
        (counts: idx_n on the host, already clamped to idx_cap)."""
        icap = int(idx.shape[1])
        om = torch.empty(self.S, icap, dtype=torch.int64, device=self.dev)
        ov = torch.empty(self.S, icap, dtype=torch.float64, device=self.dev)
        oc = torch.empty(self.S, icap, nat.TAGLOG_COLS_BYTES, dtype=torch.uint8, device=self.dev) if self.columns else None
        with torch.cuda.stream(self._torch_stream()):
            nat.check(self.L.av_taglog_gather(self.ctx.handle, self._s(), self.S, self.cap, nat.ptr(self.mask), nat.ptr(self.speed),
                                              nat.ptr(self.cols), nat.ptr(self.log_n), nat.ptr(idx), nat.ptr(idx_n), icap, nat.ptr(om),
                                              nat.ptr(ov), nat.ptr(oc)))
        self._sync()
        hi, hm, hv = idx.cpu().numpy().reshape(self.S, icap), om.cpu().numpy().view(np.uint64), ov.cpu().numpy()
        hc = oc.cpu().numpy().reshape(self.S, icap * nat.TAGLOG_COLS_BYTES).view(COLS_DTYPE) if self.columns else None
        res = []
        for s in range(self.S):
            n = int(counts[s])
            r = np.zeros(n, self.record_dtype())
            r["frame_idx"], r["mask"], r["speed"] = hi[s, :n], hm[s, :n], hv[s, :n]
            for name in (COLS_DTYPE.names if self.columns else ()):
                r[name] = hc[s, :n][name]
            res.append(r)
        return res

    def records(self, indices, stream):
        """The logged frames `indices` of one stream as a structured array (record_dtype()).  An index outside the stream's log
        gives an all-zero record."""
        want = np.ascontiguousarray(indices, np.int32).reshape(-1)
        n = np.zeros(self.S, np.int32)
        n[stream] = len(want)
        host = np.zeros((self.S, max(len(want), 1)), np.int32)
        host[stream, :len(want)] = want
        with torch.cuda.stream(self._torch_stream()):
            idx, idx_n = torch.from_numpy(host).to(self.dev), torch.from_numpy(n).to(self.dev)
        return self._gather(idx, idx_n, n)[stream]

    def records_where(self, stream=None, first=0, last=None, **where):
        """The frames search_where(**where) finds, as records: the indices go from the search to the gather on the device."""
        found = self._run_where(None, first, last, None, **where)
        if found is None:
            res = [np.zeros(0, self.record_dtype()) for _ in range(self.S)]
        else:                               # _query left the indices in its output buffer and their counts in _out_n
            res = self._gather(self._out["search"], self._out_n, [len(f) for f in found])
        return res if stream is None else res[stream]

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


def _group(mask, name, enum):
    base, n = _GROUPS[name]
    k = (int(mask) >> base) & ((1 << n) - 1)
    return list(enum)[k.bit_length() - 1].value if k else None


def _none_if_nan(v):
    v = float(v)
    return None if v != v else v


def frame_dict(frame_idx, mask, speed, cols=None, fps=30.0):
    """FrameTags.to_dict()'s shape (auto_tagger.py:32-45) holding what the log knows of one frame: its mask, its speed and -- for
    a log with columns -- its record `cols` (one element of a _native.TAGLOG_COLS_FIELDS array; None: the keys it bears are left
    out).  A group whose presence flag is clear is {} as in the reference; timestamp = frame_idx / fps as AutoTagger.tag_frame
    sets it.  all_tags is in vocabulary order."""
    mask = int(mask)
    tags = tags_of(mask)
    scene, maneuver, interaction, conf = {}, {}, {}, {}
    if (mask >> HAS_SCENE) & 1:
        scene['road_type'] = _group(mask, "road_type", RoadType) or RoadType.UNKNOWN.value
        if cols is not None:
            scene['road_type_confidence'] = float(cols["road_type_confidence"])
            conf[scene['road_type']] = scene['road_type_confidence']
    if (mask >> HAS_MANEUVER) & 1:
        names = (_group(mask, "lateral", LateralManeuver), _group(mask, "longitudinal", LongitudinalManeuver),
                 _group(mask, "turning", TurningManeuver))
        for key, name in zip(("lateral", "longitudinal", "turning"), names):
            if name is not None:
                maneuver[key] = name
            if cols is not None:
                maneuver[key + "_confidence"] = float(cols[key + "_confidence"])
                if name is not None:
                    conf[name] = maneuver[key + "_confidence"]
        maneuver['speed_kmh'] = float(speed)
        if cols is not None:
            maneuver['acceleration'], maneuver['yaw_rate_deg'] = float(cols["acceleration"]), float(cols["yaw_rate_deg"])
    if (mask >> HAS_INTERACTION) & 1:
        risk = (mask >> RISK) & 7
        interaction['overall_risk'] = _RISKS[risk.bit_length()]
        if cols is not None:
            for key in ("agent_count", "pedestrian_count", "cyclist_count", "vehicle_count"):
                interaction[key] = int(cols[key])
            interaction['closest_agent_distance'] = _none_if_nan(cols["closest_distance"])
            interaction['min_ttc'] = _none_if_nan(cols["min_ttc"])
    return {'frame_idx': int(frame_idx), 'timestamp': int(frame_idx) / float(fps), 'scene': scene, 'maneuver': maneuver,
            'interaction': interaction, 'all_tags': tags, 'tag_confidences': conf}
