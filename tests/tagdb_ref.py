"""NumPy restatement of the tag log's records (av_tags_cols), the numeric predicate (av_taglog_where), the gather and
frame_dict, written from the rules of include/avhot.h and from FrameTags.to_dict() / TagDatabase.save_frame_tags of the
reference -- plain loops over frames, nothing of the kernels' chunking."""
import math

import numpy as np

from tests import taglog_ref as R

COLS_FIELDS = [("road_type_confidence", "<f8"), ("lateral_confidence", "<f8"), ("longitudinal_confidence", "<f8"),
               ("turning_confidence", "<f8"), ("acceleration", "<f8"), ("yaw_rate_deg", "<f8"), ("min_ttc", "<f8"),
               ("closest_distance", "<f8"), ("agent_count", "<i4"), ("pedestrian_count", "<i4"), ("cyclist_count", "<i4"),
               ("vehicle_count", "<i4")]
COLS = np.dtype(COLS_FIELDS)
NAN_BITS = 0x7ff8000000000000

ROADS = ["unknown", "intersection", "highway", "urban", "residential", "parking"]
LATERAL = ["lane_keeping", "lane_change_left", "lane_change_right", "swerving"]
LONGITUDINAL = ["cruising", "accelerating", "braking", "hard_braking", "stopped"]
TURNING = ["straight", "turning_left", "turning_right", "u_turn", "curving_left", "curving_right"]
RISKS = ["low", "medium", "high", "critical"]


def cols(S, W, maneuver=None, inter_summary=None, scene=None):
    """Row arrays shaped [S][W] (or None) -> records [S][W].  Copies only: the doubles go through their bit patterns."""
    out = np.zeros((S, W), COLS)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)            # noqa: E731
    put = lambda name, a: out[name].view(np.uint64).__setitem__(Ellipsis, bits(a))          # noqa: E731
    if scene is not None:
        put("road_type_confidence", scene["confidence"])
    if maneuver is not None:
        for name in ("lateral_confidence", "longitudinal_confidence", "turning_confidence", "acceleration", "yaw_rate_deg"):
            put(name, maneuver[name])
    if inter_summary is not None:
        put("min_ttc", inter_summary["min_ttc"])
        put("closest_distance", inter_summary["closest_distance"])
        for name in ("agent_count", "pedestrian_count", "cyclist_count", "vehicle_count"):
            out[name] = inter_summary[name]
    else:
        out["min_ttc"].view(np.uint64)[...] = NAN_BITS
        out["closest_distance"].view(np.uint64)[...] = NAN_BITS
    return out


def same_bits(a, b):
    """Two record (or any) arrays byte for byte."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _unset(bound):
    return bound is None or (isinstance(bound, float) and math.isnan(bound))


def frame_matches(mask, speed, rec, all_=0, any_=0, none=0, speed_min=None, speed_max=None, accel_min=None, accel_max=None,
                  ttc_max=None, distance_max=None, agents_min=0, pedestrians_min=0, cyclists_min=0, vehicles_min=0):
    """av_taglog_where on one frame: an unset bound (None or NaN) imposes nothing, a set one is an inclusive comparison, false
    against a stored NaN; a count bound <= 0 imposes nothing."""
    if not R.matches(mask, all_, any_, none):
        return False
    for value, lo, hi in ((speed, speed_min, speed_max), (None if rec is None else rec["acceleration"], accel_min, accel_max),
                          (None if rec is None else rec["min_ttc"], None, ttc_max),
                          (None if rec is None else rec["closest_distance"], None, distance_max)):
        if not _unset(lo) and not float(value) >= lo:
            return False
        if not _unset(hi) and not float(value) <= hi:
            return False
    for name, bound in (("agent_count", agents_min), ("pedestrian_count", pedestrians_min), ("cyclist_count", cyclists_min),
                        ("vehicle_count", vehicles_min)):
        if bound > 0 and not int(rec[name]) >= bound:
            return False
    return True


def search_where(masks, speeds, recs, first=0, last=None, **where):
    n = len(masks)
    last = n if last is None else min(last, n)
    return [i for i in range(max(first, 0), last) if frame_matches(masks[i], speeds[i], None if recs is None else recs[i], **where)]


def segments_where(masks, speeds, recs, min_duration=5, first=0, last=None, **where):
    """get_event_segments' loop over [first, last) with the numeric predicate: the matching frames as a one-bit mask."""
    on = np.zeros(len(masks), np.uint64)
    on[search_where(masks, speeds, recs, first, last, **where)] = 1
    return R.segments(on, all_=1, min_duration=min_duration, first=first, last=last)


def gather(masks, speeds, recs, idx):
    """The frames idx of one stream: (masks, speeds, records); an index outside [0, len(masks)) gives zeros."""
    om, ov = np.zeros(len(idx), np.uint64), np.zeros(len(idx))
    oc = None if recs is None else np.zeros(len(idx), COLS)
    for j, f in enumerate(idx):
        if 0 <= int(f) < len(masks):
            om[j], ov[j] = masks[f], speeds[f]
            if recs is not None:
                oc[j] = recs[f]
    return om, ov, oc


def _name(mask, base, names):
    field = (int(mask) >> base) & ((1 << len(names)) - 1)
    return names[field.bit_length() - 1] if field else None


def frame_dict(frame_idx, mask, speed, rec=None, fps=30.0, vocabulary=None):
    """FrameTags.to_dict()'s shape from a logged frame.  vocabulary: the 49 tag names in bit order (for all_tags)."""
    mask = int(mask)
    scene, maneuver, interaction, conf = {}, {}, {}, {}
    none_if_nan = lambda v: None if math.isnan(float(v)) else float(v)  # noqa: E731
    if (mask >> R.HAS_SCENE) & 1:
        scene["road_type"] = _name(mask, R.ROAD_TYPE, ROADS) or "unknown"
        if rec is not None:
            scene["road_type_confidence"] = conf[scene["road_type"]] = float(rec["road_type_confidence"])
    if (mask >> R.HAS_MANEUVER) & 1:
        for key, base, names in (("lateral", R.LATERAL, LATERAL), ("longitudinal", R.LONGITUDINAL, LONGITUDINAL),
                                 ("turning", R.TURNING, TURNING)):
            name = _name(mask, base, names)
            if name is not None:
                maneuver[key] = name
            if rec is not None:
                maneuver[key + "_confidence"] = float(rec[key + "_confidence"])
                if name is not None:
                    conf[name] = maneuver[key + "_confidence"]
        maneuver["speed_kmh"] = float(speed)
        if rec is not None:
            maneuver["acceleration"], maneuver["yaw_rate_deg"] = float(rec["acceleration"]), float(rec["yaw_rate_deg"])
    if (mask >> R.HAS_INTERACTION) & 1:
        interaction["overall_risk"] = RISKS[((mask >> R.RISK) & 7).bit_length()]
        if rec is not None:
            for key in ("agent_count", "pedestrian_count", "cyclist_count", "vehicle_count"):
                interaction[key] = int(rec[key])
            interaction["closest_agent_distance"] = none_if_nan(rec["closest_distance"])
            interaction["min_ttc"] = none_if_nan(rec["min_ttc"])
    tags = [] if vocabulary is None else [t for k, t in enumerate(vocabulary) if (mask >> k) & 1]
    return {"frame_idx": int(frame_idx), "timestamp": int(frame_idx) / float(fps), "scene": scene, "maneuver": maneuver,
            "interaction": interaction, "all_tags": tags, "tag_confidences": conf}
