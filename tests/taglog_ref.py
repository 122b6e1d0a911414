"""NumPy restatement of the tag log (pack, append, search, segments, statistics), written from the rules of include/avhot.h
and from the reference's AutoTagger (auto_tagger.py: search_by_tag(s), get_high_risk_frames, get_event_segments,
get_tag_statistics) -- plain loops over frames, nothing of the kernels' chunking."""
import numpy as np

# bit layout: each Enum of the reference in definition order
ROAD_TYPE, ELEMENT, CONDITION, PEDESTRIAN_AREA, LATERAL, LONGITUDINAL, TURNING, INTERACTION, RISK = 0, 6, 11, 17, 18, 22, 27, 33, 46
N_ROAD, N_ELEMENT, N_CONDITION, N_LATERAL, N_LONGITUDINAL, N_TURNING, N_INTERACTION = 6, 5, 6, 4, 5, 6, 13
HAS_SCENE, HAS_MANEUVER, HAS_INTERACTION = 61, 62, 63
N_TAGS = 49


def _bit(value, n, base):
    value = int(value)
    return (1 << (base + value)) if 0 <= value < n else 0


def pack_frame(maneuver=None, inter_rows=None, inter_summary=None, snap_n=0, tcap=64, scene=None, det_n=0, det_cls=None,
               max_det=0, elem_table=None):
    """One frame's (mask, speed).  maneuver / inter_summary / scene: one structured row each (or None); inter_rows: the
    frame's tcap rows; det_cls: the frame's max_det class ids (or None)."""
    m, speed = 0, float("nan")
    if scene is not None:
        m |= 1 << HAS_SCENE
        m |= _bit(scene["road_type"], N_ROAD, ROAD_TYPE)
        for k in range(min(max(int(scene["n_conditions"]), 0), 3)):
            m |= _bit(scene["conditions"][k], N_CONDITION, CONDITION)
        if int(scene["has_pedestrian"]) != 0:
            m |= 1 << PEDESTRIAN_AREA
        if det_cls is not None:
            for i in range(min(max(int(det_n), 0), max_det)):
                c = int(det_cls[i])
                if 0 <= c < len(elem_table) and elem_table[c] != 0:
                    m |= _bit(int(elem_table[c]) - 1, N_ELEMENT, ELEMENT)
    if maneuver is not None:
        m |= 1 << HAS_MANEUVER
        m |= _bit(maneuver["lateral"], N_LATERAL, LATERAL) | _bit(maneuver["longitudinal"], N_LONGITUDINAL, LONGITUDINAL)
        m |= _bit(maneuver["turning"], N_TURNING, TURNING)
        speed = float(maneuver["speed_kmh"])
    if inter_summary is not None:
        m |= 1 << HAS_INTERACTION
        for i in range(min(max(int(snap_n), 0), tcap)):
            if int(inter_rows["type"][i]) >= 0 and float(inter_rows["confidence"][i]) > 0.5:
                m |= _bit(inter_rows["type"][i], N_INTERACTION, INTERACTION)
        risk = int(inter_summary["overall_risk"])
        if risk != 0:
            m |= _bit(risk - 1, 3, RISK)
    return m, speed


def pack(S, W, maneuver=None, inter_rows=None, inter_summary=None, snap_n=None, tcap=64, scene=None, det_n=None, det_cls=None,
         elem_table=None):
    """Arrays shaped [S][W]... -> masks uint64 [S][W], speeds float64 [S][W]."""
    masks, speeds = np.zeros((S, W), np.uint64), np.zeros((S, W), np.float64)
    for s in range(S):
        for w in range(W):
            masks[s, w], speeds[s, w] = pack_frame(
                None if maneuver is None else maneuver[s, w], None if inter_rows is None else inter_rows[s, w],
                None if inter_summary is None else inter_summary[s, w], 0 if snap_n is None else snap_n[s, w], tcap,
                None if scene is None else scene[s, w], 0 if det_n is None else det_n[s, w],
                None if det_cls is None else det_cls[s, w], 0 if det_cls is None else det_cls.shape[-1], elem_table)
    return masks, speeds


class Log:
    """One stream's log: Python lists, a capacity, a drop counter."""

    def __init__(self, cap):
        self.cap, self.masks, self.speeds, self.dropped = cap, [], [], 0

    def append(self, masks, speeds):
        for m, v in zip(masks, speeds):
            if len(self.masks) < self.cap:
                self.masks.append(int(m))
                self.speeds.append(float(v))
            else:
                self.dropped += 1


def matches(m, all_=0, any_=0, none=0):
    m = int(m)
    return (m & all_) == all_ and (any_ == 0 or (m & any_) != 0) and (m & none) == 0


def search(masks, all_=0, any_=0, none=0, first=0, last=None):
    n = len(masks)
    last = n if last is None else min(last, n)
    return [i for i in range(max(first, 0), last) if matches(masks[i], all_, any_, none)]


def segments(masks, all_=0, any_=0, none=0, min_duration=5, first=0, last=None):
    """get_event_segments' loop over the frames of [first, last)."""
    n = len(masks)
    last = n if last is None else min(last, n)
    first = max(first, 0)
    segs, start = [], None
    for i in range(first, last):
        on = matches(masks[i], all_, any_, none)
        if on and start is None:
            start = i
        elif not on and start is not None:
            if i - start >= min_duration:
                segs.append((start, i - 1))
            start = None
    if start is not None and last - start >= min_duration:
        segs.append((start, last - 1))
    return segs


def stats(masks, speeds):
    """-> dict(tag_count int[64], n_frames, n_maneuver, risk_count int[4], speed_min, speed_max, speed_sum)."""
    tag_count, risk = [0] * 64, [0] * 4
    sp = []
    for m, v in zip(masks, speeds):
        m = int(m)
        for b in range(64):
            tag_count[b] += (m >> b) & 1
        if (m >> HAS_MANEUVER) & 1:
            sp.append(float(v))
        for k in (1, 2, 3):
            risk[k] += (m >> (RISK + k - 1)) & 1
        if (m >> HAS_INTERACTION) & 1 and not (m >> RISK) & 7:
            risk[0] += 1
    return dict(tag_count=tag_count, n_frames=len(masks), n_maneuver=len(sp), risk_count=risk,
                speed_min=min(sp) if sp else float("inf"), speed_max=max(sp) if sp else float("-inf"),
                speed_sum=float(np.sum(np.array(sp, np.float64))) if sp else 0.0)


def mask_of(tags, vocabulary):
    """Mask of a frame's all_tags given the 49 names in bit order (every name must be in the vocabulary)."""
    m = 0
    for t in tags:
        m |= 1 << vocabulary.index(t)
    return m
