"""Host side of the tag log's records: tagging.tag_log.frame_dict against the restatement tests/tagdb_ref.py and against
tag_mask / tags_of, what the database makes of absent groups, NaN -> None, and TagDatabase.save_tag_log against the per-frame
path it is defined by -- on a stand-in log whose arrays are host tensors (the GPU test repeats it on a real TagLog).
Everything is compared by equality."""
import json
import math
from datetime import datetime

import numpy as np
import pytest

from tests import tagdb_ref as D
from tests import taglog_ref as R
from tests.test_tagdb_host import dump_tables

FLAGS = {"scene": 1 << R.HAS_SCENE, "maneuver": 1 << R.HAS_MANEUVER, "interaction": 1 << R.HAS_INTERACTION}


def _tl():
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging import tag_log
    return tag_log


def random_log(rng, n, junk=False):
    """n frames as the taggers would leave them: one bit per enum group, flags for the groups present, about a quarter of the
    min_ttc NaN, some distances infinite.  junk: also masks no tagger produces (several bits in a group, bits without their flag)."""
    tl = _tl()
    masks = np.zeros(n, np.uint64)
    ri = lambda hi: int(rng.integers(hi))                           # noqa: E731
    for k in range(n):
        m = 0
        if rng.random() < 0.8:
            m |= FLAGS["scene"] | 1 << (tl.ROAD_TYPE + ri(6)) | 1 << (tl.CONDITION + ri(6))
            m |= (1 << tl.PEDESTRIAN_AREA) * ri(2) | (1 << (tl.ELEMENT + ri(5))) * ri(2)
        if rng.random() < 0.8:
            m |= FLAGS["maneuver"] | 1 << (tl.LATERAL + ri(4)) | 1 << (tl.LONGITUDINAL + ri(5))
            m |= 1 << (tl.TURNING + ri(6))
        if rng.random() < 0.8:
            m |= FLAGS["interaction"] | (1 << (tl.INTERACTION + ri(13))) * ri(2)
            risk = ri(4)
            m |= (1 << (tl.RISK + risk - 1)) if risk else 0
        if junk and rng.random() < 0.2:
            m = int(rng.integers(0, 2 ** 63)) << 1 | ri(2)
        masks[k] = m
    recs = np.zeros(n, D.COLS)
    for name in ("road_type_confidence", "lateral_confidence", "longitudinal_confidence", "turning_confidence"):
        recs[name] = rng.uniform(0.0, 1.0, n)
    recs["acceleration"], recs["yaw_rate_deg"] = rng.uniform(-8.0, 4.0, n), rng.uniform(-30.0, 30.0, n)
    recs["min_ttc"] = np.where(rng.random(n) < 0.25, np.nan, rng.uniform(0.1, 10.0, n))
    recs["closest_distance"] = np.where(rng.random(n) < 0.1, np.inf, rng.uniform(0.5, 80.0, n))
    for name in ("pedestrian_count", "cyclist_count", "vehicle_count"):
        recs[name] = rng.integers(0, 4, n)
    recs["agent_count"] = recs["pedestrian_count"] + recs["cyclist_count"] + recs["vehicle_count"]
    speeds = np.where((masks >> np.uint64(R.HAS_MANEUVER)) & np.uint64(1), rng.uniform(0.0, 130.0, n), np.nan)
    return masks, speeds, recs


def test_frame_dict_round_trips_and_equals_the_restatement():
    tl = _tl()
    rng = np.random.default_rng(5)
    masks, speeds, recs = random_log(rng, 300, junk=True)
    for k in range(len(masks)):
        for rec in (recs[k], None):
            got = tl.frame_dict(k, masks[k], speeds[k], rec, fps=25.0)
            want = D.frame_dict(k, masks[k], speeds[k], rec, fps=25.0, vocabulary=list(tl.TAGS))
            assert json.dumps(got) == json.dumps(want), (k, hex(int(masks[k])))      # NaN speeds included: compared as text
            m = int(masks[k])
            assert got["all_tags"] == tl.tags_of(m) and tl.tag_mask(got["all_tags"]) == m & ((1 << 49) - 1)
            assert got["timestamp"] == k / 25.0 and type(got["frame_idx"]) is int
            assert (got["scene"] == {}) == (not m & FLAGS["scene"]) and (got["maneuver"] == {}) == (not m & FLAGS["maneuver"])
            assert (got["interaction"] == {}) == (not m & FLAGS["interaction"])
            assert set(got["tag_confidences"]) <= set(got["all_tags"]) | {"unknown"}
            if rec is None:
                assert got["tag_confidences"] == {} and set(got["scene"]) <= {"road_type"}
                assert set(got["maneuver"]) <= {"lateral", "longitudinal", "turning", "speed_kmh"}
                assert set(got["interaction"]) <= {"overall_risk"}


def test_frame_dict_values_by_hand():
    tl = _tl()
    rec = np.zeros(1, D.COLS)[0]
    rec["road_type_confidence"], rec["lateral_confidence"], rec["longitudinal_confidence"], rec["turning_confidence"] = 0.6, 0.7, 0.8, 0.9
    rec["acceleration"], rec["yaw_rate_deg"], rec["min_ttc"], rec["closest_distance"] = -2.5, 3.25, np.nan, np.inf
    rec["agent_count"], rec["pedestrian_count"], rec["cyclist_count"], rec["vehicle_count"] = 5, 1, 2, 2
    tags = ["highway", "traffic_light", "night", "lane_change_left", "braking", "curving_right", "vehicle_cut_in", "risk_high"]
    m = tl.tag_mask(tags) | sum(FLAGS.values())
    d = tl.frame_dict(7, m, 88.5, rec, fps=10.0)
    assert d == {"frame_idx": 7, "timestamp": 0.7, "scene": {"road_type": "highway", "road_type_confidence": 0.6},
                 "maneuver": {"lateral": "lane_change_left", "lateral_confidence": 0.7, "longitudinal": "braking",
                              "longitudinal_confidence": 0.8, "turning": "curving_right", "turning_confidence": 0.9, "speed_kmh": 88.5,
                              "acceleration": -2.5, "yaw_rate_deg": 3.25},
                 "interaction": {"overall_risk": "high", "agent_count": 5, "pedestrian_count": 1, "cyclist_count": 2, "vehicle_count": 2,
                                 "closest_agent_distance": math.inf, "min_ttc": None},
                 "all_tags": tl.tags_of(m),
                 "tag_confidences": {"highway": 0.6, "lane_change_left": 0.7, "braking": 0.8, "curving_right": 0.9}}
    assert sorted(d["all_tags"]) == sorted(tags)
    rec["closest_distance"], rec["min_ttc"] = np.nan, 1.5                    # NaN = None, whichever of the two
    d = tl.frame_dict(0, m, 0.0, rec)
    assert d["interaction"]["closest_agent_distance"] is None and d["interaction"]["min_ttc"] == 1.5 and d["timestamp"] == 0.0
    # no risk bit with an interaction summary is 'low'
    assert tl.frame_dict(0, FLAGS["interaction"], math.nan)["interaction"] == {"overall_risk": "low"}


def test_absent_groups_take_the_database_defaults():
    """A frame without an interaction summary is 'low' in the database, one without a scene row 'unknown', one without a
    maneuver row lane_keeping / cruising / straight at speed 0 -- the reference's defaults for an empty group."""
    tl = _tl()
    from multimodal_autonomous_driving_perception_and_planning_amd.database import TagDatabase
    db = TagDatabase(":memory:")
    db.save_session({"session_id": "s", "video_path": "v", "start_time": "t"})
    rec = np.zeros(1, D.COLS)[0]
    rec["min_ttc"] = rec["closest_distance"] = np.nan
    db.save_frame_tags("s", tl.frame_dict(0, 0, math.nan, rec))
    db.save_frame_tags("s", tl.frame_dict(1, tl.tag_mask(["risk_critical", "fog"]) | FLAGS["interaction"] | FLAGS["scene"], math.nan, rec))
    rows = dump_tables(db.conn, None)["frames"]
    assert rows[0][4:17] == ["unknown", 0.0, "lane_keeping", "cruising", "straight", 0.0, 0.0, "low", 0, 0, 0, None, None]
    assert rows[1][4:17] == ["unknown", 0.0, "lane_keeping", "cruising", "straight", 0.0, 0.0, "critical", 0, 0, 0, None, None]
    assert db.get_tag_statistics()["risk_distribution"] == {"critical": 1, "low": 1}
    assert [r.frame_idx for r in db.search_high_risk()] == [1] and [r.frame_idx for r in db.search_by_tag("fog")] == [1]


def test_where_restatement_by_hand():
    rec = np.zeros(4, D.COLS)
    rec["min_ttc"] = [1.0, np.nan, 2.0, 3.0]
    rec["closest_distance"] = [5.0, 5.0, np.inf, 12.0]
    rec["acceleration"] = [-3.0, 0.0, 1.0, np.nan]
    rec["pedestrian_count"] = [0, 1, 2, 3]
    masks, speeds = np.array([1, 1, 3, 1], np.uint64), np.array([10.0, np.nan, 30.0, 40.0])
    q = lambda **kw: D.search_where(masks, speeds, rec, **kw)           # noqa: E731
    assert q() == [0, 1, 2, 3] and q(ttc_max=2.0) == [0, 2] and q(ttc_max=float("nan")) == [0, 1, 2, 3]
    assert q(distance_max=12.0) == [0, 1, 3] and q(speed_min=10.0) == [0, 2, 3] and q(speed_max=30.0) == [0, 2]
    assert q(accel_min=-3.0, accel_max=0.0) == [0, 1] and q(accel_max=5.0) == [0, 1, 2] and q(pedestrians_min=2) == [2, 3]
    assert q(pedestrians_min=0) == q(pedestrians_min=-4) == [0, 1, 2, 3] and q(all_=2, ttc_max=5.0) == [2]
    assert D.segments_where(masks, speeds, rec, min_duration=2, speed_min=20.0) == [(2, 3)]
    assert D.segments_where(masks, speeds, rec, min_duration=1, ttc_max=9.0) == [(0, 0), (2, 3)]


class HostLog:
    """What save_tag_log reads of a TagLog, as host tensors."""

    def __init__(self, masks, speeds, recs, cap, dropped):
        import torch
        self.S, self.cap, self.columns = len(masks), cap, recs is not None
        m, v, c = np.zeros((self.S, cap), np.uint64), np.zeros((self.S, cap)), np.zeros((self.S, cap), D.COLS)
        for s in range(self.S):
            m[s, :len(masks[s])], v[s, :len(masks[s])] = masks[s], speeds[s]
            if recs is not None:
                c[s, :len(masks[s])] = recs[s]
        self.mask, self.speed = torch.from_numpy(m.view(np.int64)), torch.from_numpy(v)
        self.cols = torch.from_numpy(c.view(np.uint8).reshape(self.S, cap, 80)) if recs is not None else None
        self.dropped = torch.tensor(dropped, dtype=torch.int32)
        self._n = np.array([len(x) for x in masks], np.int32)

    def lengths(self):
        return self._n


def save_per_frame(db, masks, speeds, recs, ids, paths, fps, start, dropped):
    """save_tag_log's definition: a session per stream, then every frame through frame_dict and save_frame_tags."""
    from multimodal_autonomous_driving_perception_and_planning_amd.database import tag_log_session
    tl = _tl()
    for s in range(len(masks)):
        db.save_session(tag_log_session(ids[s], paths[s], start, len(masks[s]), fps, s, dropped[s]))
        for k in range(len(masks[s])):
            db.save_frame_tags(ids[s], tl.frame_dict(k, masks[s][k], speeds[s][k], None if recs is None else recs[s][k], fps))


@pytest.mark.parametrize("columns", [True, False])
@pytest.mark.parametrize("full_data", [True, False])
def test_save_tag_log_equals_the_per_frame_path(columns, full_data):
    from multimodal_autonomous_driving_perception_and_planning_amd.database import TagDatabase
    rng = np.random.default_rng(11)
    logs = [random_log(rng, n, junk=True) for n in (0, 37, 150)]
    masks, speeds = [x[0] for x in logs], [x[1] for x in logs]
    recs = [x[2] for x in logs] if columns else None
    start, dropped = datetime(2024, 5, 6, 7, 8, 9), [0, 3, 0]
    bulk, slow = TagDatabase(":memory:"), TagDatabase(":memory:")
    ids = bulk.save_tag_log(HostLog(masks, speeds, recs, 160, dropped), fps=12.5, start_time=start, full_data=full_data)
    assert ids == ["20240506_070809_s000", "20240506_070809_s001", "20240506_070809_s002"]
    save_per_frame(slow, masks, speeds, recs, ids, ["stream_%03d" % s for s in range(3)], 12.5, start, dropped)
    if not full_data:
        slow.conn.execute("UPDATE frames SET full_data = NULL")
    got, want = dump_tables(bulk.conn, None), dump_tables(slow.conn, None)
    for table in want:
        assert got[table] == want[table], table
    assert len(want["frames"]) == 187 and len(want["frame_tags"]) > 1000
    assert json.loads(got["sessions"][1][-1])["dropped"] == 3 and got["sessions"][0][4] == 0
    assert bulk.get_tag_statistics() == slow.get_tag_statistics()
    for sid in ids:
        assert bulk.export_session(sid) == slow.export_session(sid)
    # saving the log again replaces every frame (new row ids) and orphans the old frame_tags rows, as the per-frame path does
    bulk.save_tag_log(HostLog(masks, speeds, recs, 160, dropped), fps=12.5, start_time=start, full_data=full_data)
    save_per_frame(slow, masks, speeds, recs, ids, ["stream_%03d" % s for s in range(3)], 12.5, start, dropped)
    if not full_data:
        slow.conn.execute("UPDATE frames SET full_data = NULL")
    assert dump_tables(bulk.conn, None) == dump_tables(slow.conn, None)
    with pytest.raises(ValueError):
        bulk.save_tag_log(HostLog(masks, speeds, recs, 160, dropped), session_ids=["only one"])
