#!/usr/bin/env python3
"""Generate tests/golden/tagdb.json by running the REAL reference TagDatabase (src/database/tag_database.py).

Runs only where the reference checkout is available (AV_REFERENCE, default: a `reference` directory beside this repository);
only the .json is committed.  The class is loaded from its file (it needs sqlite3 and json only).  The fixture holds
  sessions / saves   the inputs, in the order they are saved: two sessions, 40 frame dicts, one of them saved twice
  calls              every query method with several arguments each, and what the reference returned (a search's QueryResults
                     as rows of ROW_FIELDS plus the `tags` list they all carry)
  dump               the four tables, tag names in place of tag ids (INSERT OR IGNORE burns AUTOINCREMENT values), ordered;
                     frames.full_data is checked here to be json.dumps of the saved dict and recorded as that save's index
  after_delete       statistics, sessions and the tables' row counts once the second session is deleted
Data only: dicts, lists, strings and numbers (Python's JSON dialect: Infinity appears as such).

Usage:  python tests/golden/make_golden_tagdb.py
"""
import copy
import dataclasses
import importlib.util
import json
import os
import random

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AV_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference"))

ROADS = ["unknown", "intersection", "highway", "urban", "residential", "parking"]
LATERAL = ["lane_keeping", "lane_change_left", "lane_change_right", "swerving"]
LONGITUDINAL = ["cruising", "accelerating", "braking", "hard_braking", "stopped"]
TURNING = ["straight", "turning_left", "turning_right", "u_turn", "curving_left", "curving_right"]
RISKS = ["low", "medium", "high", "critical"]
SID_A, SID_B = "20240102_030405", "20240102_040506"


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_tag_database", os.path.join(REF, "src", "database", "tag_database.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ROW_FIELDS = ["session_id", "video_path", "frame_idx", "timestamp", "road_type", "maneuver", "risk_level", "speed_kmh"]


def dump_tables(conn, saves):
    """The four tables as lists of lists, tag names for tag ids, ordered; created_at (a wall-clock time) left out; full_data as
    the index of the save it is the JSON text of."""
    q = lambda sql: [list(r) for r in conn.execute(sql).fetchall()]      # noqa: E731
    texts = [json.dumps(ft) for _, ft in saves]
    out = _dump(q)
    for row in out["frames"]:
        hits = [i for i, text in enumerate(texts) if text == row[-1] and saves[i][0] == row[1]]
        assert hits, "full_data of frame row %d is not the JSON of a saved dict" % row[0]
        row[-1] = hits[-1]
    return out


def _dump(q):
    return {
        "sessions": q("SELECT session_id, video_path, start_time, end_time, total_frames, fps, metadata FROM sessions ORDER BY session_id"),
        "tags": q("SELECT tag_name, tag_category FROM tags ORDER BY tag_name"),
        "frames": q("SELECT id, session_id, frame_idx, timestamp, road_type, road_type_confidence, lateral_maneuver, "
                    "longitudinal_maneuver, turning_maneuver, speed_kmh, acceleration, risk_level, agent_count, pedestrian_count, "
                    "vehicle_count, min_ttc, closest_distance, full_data FROM frames ORDER BY id"),
        "frame_tags": q("SELECT ft.frame_id, t.tag_name, ft.confidence FROM frame_tags ft JOIN tags t ON ft.tag_id = t.tag_id "
                        "ORDER BY ft.frame_id, t.tag_name"),
    }


def make_frame(rng, k, fps):
    """A FrameTags.to_dict()-shaped dict; every third group or so is the empty dict of a tagger that gave nothing."""
    tags, conf = [], {}
    scene, maneuver, interaction = {}, {}, {}
    if k % 7 != 5:
        road = ROADS[(k * 5 + k // 4) % 6]
        scene = {"road_type": road, "road_type_confidence": round(rng.uniform(0.3, 1.0), 3), "conditions": [["day", 0.8]],
                 "has_pedestrian_area": k % 4 == 0}
        tags += [road, "day"] + (["pedestrian_area"] if k % 4 == 0 else [])
        conf[road] = scene["road_type_confidence"]
    if k % 5 != 3:
        lat, lon, trn = LATERAL[(k // 3) % 4], LONGITUDINAL[(k // 2) % 5], TURNING[(k // 6) % 6]
        maneuver = {"lateral": lat, "lateral_confidence": 0.9, "longitudinal": lon, "longitudinal_confidence": 0.75, "turning": trn,
                    "turning_confidence": 0.5, "speed_kmh": round(rng.uniform(0.0, 120.0), 2),
                    "acceleration": round(rng.uniform(-6.0, 3.0), 3), "yaw_rate_deg": round(rng.uniform(-20.0, 20.0), 3)}
        tags += [lat, lon, trn]
        conf.update({lat: 0.9, lon: 0.75, trn: 0.5})
    if k % 4 != 2:
        risk = RISKS[(k * 3 + k // 5) % 4]
        interaction = {"interactions": [], "primary_interaction": None, "overall_risk": risk, "agent_count": k % 6,
                       "pedestrian_count": k % 3, "cyclist_count": k % 2, "vehicle_count": (k % 6) // 2,
                       "closest_agent_distance": float("inf") if k % 6 == 0 else round(rng.uniform(1.0, 60.0), 2),
                       "min_ttc": None if k % 3 == 0 else round(rng.uniform(0.2, 9.0), 2)}
        if risk != "low":
            tags.append("risk_" + risk)
        if k % 6:
            tags.append("following_vehicle")
            conf["following_vehicle"] = 0.7
    if k % 9 == 4:
        tags.append("construction_zone")           # not in the tag log's vocabulary: the database takes any string
    return {"frame_idx": k, "timestamp": k / fps, "scene": scene, "maneuver": maneuver, "interaction": interaction,
            "all_tags": list(dict.fromkeys(tags)), "tag_confidences": conf}


def main():
    ref = load_reference()
    rng = random.Random(20240102)
    sessions = [
        {"session_id": SID_A, "video_path": "drive_a.mp4", "start_time": "2024-01-02T03:04:05", "end_time": None, "total_frames": 35,
         "fps": 30.0},
        {"session_id": SID_B, "video_path": "drive_b.mp4", "start_time": "2024-01-02T04:05:06", "end_time": "2024-01-02T04:05:07",
         "total_frames": 5, "fps": 10.0},
    ]
    saves = [[SID_A, make_frame(rng, k, 30.0)] for k in range(35)] + [[SID_B, make_frame(rng, k, 10.0)] for k in range(5)]
    again = copy.deepcopy(saves[3][1])             # frame 3 of the first session once more, with other tags
    again["all_tags"] = ["highway", "risk_critical", "construction_zone"]
    again["interaction"] = dict(again["interaction"] or {}, overall_risk="critical")
    saves.append([SID_A, again])

    db = ref.TagDatabase(":memory:")
    for s in sessions:
        db.save_session(copy.deepcopy(s))
    frame_ids = [db.save_frame_tags(sid, copy.deepcopy(ft)) for sid, ft in saves]

    two = ["highway", "day"]
    plan = [("search_by_tag", [t], kw) for t in ("highway", "construction_zone", "no_such_tag", "risk_critical")
            for kw in ({}, {"session_id": SID_A}, {"session_id": SID_B, "limit": 1}, {"limit": 2})]
    plan += [("search_by_multiple_tags", [tags], dict(kw, match_all=m))
             for tags in (two, ["day", "cruising", "lane_keeping"], ["highway", "no_such_tag"], ["day", "day"], [])
             for m in (True, False) for kw in ({}, {"session_id": SID_B}, {"limit": 2})]
    plan += [("search_high_risk", [], kw) for kw in ({}, {"session_id": SID_A}, {"session_id": SID_B}, {"limit": 2})]
    plan += [("get_tag_statistics", [], kw) for kw in ({}, {"session_id": SID_A}, {"session_id": SID_B}, {"session_id": "nobody"})]
    plan += [("get_sessions", [], {}), ("export_session", [SID_B], {}), ("export_session", [SID_B, "csv"], {}),
             ("export_session", [SID_B, "xml"], {})]
    calls = []
    for name, args, kw in plan:
        got = getattr(db, name)(*copy.deepcopy(args), **kw)
        if isinstance(got, list) and got and dataclasses.is_dataclass(got[0]):
            got = {"tags": got[0].tags, "rows": [[dataclasses.asdict(r)[k] for k in ROW_FIELDS] for r in got]}
            assert all(r.tags == got["tags"] for r in getattr(db, name)(*copy.deepcopy(args), **kw))
        calls.append({"method": name, "args": args, "kwargs": kw, "result": got})
    out = {"sessions": sessions, "saves": saves, "frame_ids": frame_ids, "calls": calls, "row_fields": ROW_FIELDS,
           "dump": dump_tables(db.conn, saves)}
    db.delete_session(SID_B)
    out["after_delete"] = {"deleted": SID_B, "statistics": db.get_tag_statistics(), "statistics_deleted": db.get_tag_statistics(SID_B),
                           "sessions": db.get_sessions(),
                           "row_counts": {k: len(v) for k, v in dump_tables(db.conn, saves).items()}}
    path = os.path.join(OUT, "tagdb.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote %s: %d saves, %d calls, %d bytes" % (path, len(saves), len(calls), os.path.getsize(path)))


if __name__ == "__main__":
    main()
