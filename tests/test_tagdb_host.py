"""database.TagDatabase against what the REAL reference TagDatabase recorded (tests/golden/tagdb.json, written by
tests/golden/make_golden_tagdb.py): the same saves in the same order, then every recorded query and the dump of the four tables.
Everything is compared by equality; tag_counts and risk_distribution as dicts (their order under ties is SQLite's choice).
"""
import copy
import dataclasses
import json
import os
import sqlite3

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tagdb.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def dump_tables(conn, saves):
    """The four tables, tag names for tag ids, ordered; frames.full_data as the index of the save whose JSON text it is."""
    q = lambda sql: [list(r) for r in conn.execute(sql).fetchall()]      # noqa: E731
    out = {
        "sessions": q("SELECT session_id, video_path, start_time, end_time, total_frames, fps, metadata FROM sessions ORDER BY session_id"),
        "tags": q("SELECT tag_name, tag_category FROM tags ORDER BY tag_name"),
        "frames": q("SELECT id, session_id, frame_idx, timestamp, road_type, road_type_confidence, lateral_maneuver, "
                    "longitudinal_maneuver, turning_maneuver, speed_kmh, acceleration, risk_level, agent_count, pedestrian_count, "
                    "vehicle_count, min_ttc, closest_distance, full_data FROM frames ORDER BY id"),
        "frame_tags": q("SELECT ft.frame_id, t.tag_name, ft.confidence FROM frame_tags ft JOIN tags t ON ft.tag_id = t.tag_id "
                        "ORDER BY ft.frame_id, t.tag_name"),
    }
    if saves is not None:
        texts = [json.dumps(ft) for _, ft in saves]
        for row in out["frames"]:
            hits = [i for i, text in enumerate(texts) if text == row[-1] and saves[i][0] == row[1]]
            assert hits, "full_data of frame row %d is not the JSON text of a saved dict" % row[0]
            row[-1] = hits[-1]
    return out


def _filled(golden, path):
    from multimodal_autonomous_driving_perception_and_planning_amd.database import TagDatabase
    db = TagDatabase(path)
    for s in golden["sessions"]:
        assert db.save_session(copy.deepcopy(s)) == s["session_id"]
    ids = [db.save_frame_tags(sid, copy.deepcopy(ft)) for sid, ft in golden["saves"]]
    assert ids == golden["frame_ids"]
    return db


def _plain(got, fields):
    """A query's answer in the fixture's form."""
    if isinstance(got, list) and got and dataclasses.is_dataclass(got[0]):
        assert all(r.tags == got[0].tags for r in got)
        return {"tags": got[0].tags, "rows": [[getattr(r, k) for k in fields] for r in got]}
    return got


@pytest.mark.parametrize("where", ["memory", "file"])
def test_every_recorded_call_and_the_tables(golden, where, tmp_path):
    db = _filled(golden, ":memory:" if where == "memory" else str(tmp_path / "tags.db"))
    assert len(golden["calls"]) >= 50 and len(golden["saves"]) == 41
    seen = set()
    for call in golden["calls"]:
        args, kw, want = copy.deepcopy(call["args"]), call["kwargs"], call["result"]
        got = _plain(getattr(db, call["method"])(*args, **kw), golden["row_fields"])
        what = (call["method"], call["args"], kw)
        assert args == call["args"], what                               # the caller's lists are left alone
        seen.add(call["method"])
        if call["method"] == "get_tag_statistics":
            assert got == want and isinstance(got["tag_counts"], dict), what         # dict equality: tie order is unspecified
        elif call["method"] == "get_sessions":
            assert got == want, what
        elif call["method"] == "search_by_multiple_tags" and not kw["match_all"] and want:
            # the reference appends its SQL parameters to the caller's list in this mode, which then shows in QueryResult.tags;
            # the port returns the list it was given (documented deviation)
            extra = ([kw["session_id"]] if kw.get("session_id") else []) + [kw.get("limit", 100)]
            assert want["tags"] == call["args"][0] + extra and got["tags"] == call["args"][0], what
            assert got["rows"] == want["rows"], what
        else:
            assert got == want, what
    assert seen == {"search_by_tag", "search_by_multiple_tags", "search_high_risk", "get_tag_statistics", "get_sessions", "export_session"}
    assert dump_tables(db.conn, golden["saves"]) == golden["dump"]
    # the frame saved twice: a new row id, the old frame_tags rows orphaned -- counted globally, not per session
    live = {r[0] for r in golden["dump"]["frames"]}
    orphans = [r for r in golden["dump"]["frame_tags"] if r[0] not in live]
    assert orphans and golden["frame_ids"][-1] == max(golden["frame_ids"]) and golden["frame_ids"][3] not in live
    stats = {c["kwargs"].get("session_id"): c["result"] for c in golden["calls"] if c["method"] == "get_tag_statistics"}
    per_session = sum(sum(stats[s["session_id"]]["tag_counts"].values()) for s in golden["sessions"])
    assert sum(stats[None]["tag_counts"].values()) == per_session + len(orphans)
    db.close()
    db.close()                                                          # closing twice is harmless
    if where == "file":                                                 # the file is a plain SQLite database with the four tables
        conn = sqlite3.connect(str(tmp_path / "tags.db"))
        names = {r[0] for r in conn.execute("SELECT name FROM sqlite_master")}
        assert {"sessions", "tags", "frames", "frame_tags", "idx_frames_session", "idx_frames_road_type", "idx_frames_risk",
                "idx_tags_name"} <= names
        conn.close()


def test_a_file_opens_again(golden, tmp_path):
    from multimodal_autonomous_driving_perception_and_planning_amd.database import TagDatabase
    path = str(tmp_path / "again.db")
    _filled(golden, path).close()
    db = TagDatabase(path)                                              # CREATE ... IF NOT EXISTS: the contents stay
    assert dump_tables(db.conn, golden["saves"]) == golden["dump"]


def test_delete_session_then_statistics(golden):
    db = _filled(golden, ":memory:")
    want = golden["after_delete"]
    db.delete_session(want["deleted"])
    assert db.get_tag_statistics() == want["statistics"]
    assert db.get_tag_statistics(want["deleted"]) == want["statistics_deleted"]
    assert db.get_sessions() == want["sessions"]
    assert {k: len(v) for k, v in dump_tables(db.conn, golden["saves"]).items()} == want["row_counts"]
    with pytest.raises(KeyError):
        db.export_session(want["deleted"])


def test_export_session_both_formats(golden):
    db = _filled(golden, ":memory:")
    sid = golden["sessions"][1]["session_id"]
    text = db.export_session(sid)
    parsed = json.loads(text)
    frames = [ft for s, ft in golden["saves"] if s == sid]
    assert parsed["frames"] == frames and parsed["session"]["session_id"] == sid and text.startswith('{\n  "session"')
    assert db.export_session(sid, format="csv") == frames
    assert db.export_session(sid, format="parquet") is None


def test_src_shim_imports():
    from src.database import QueryResult, TagDatabase
    from multimodal_autonomous_driving_perception_and_planning_amd import database
    assert TagDatabase is database.TagDatabase and QueryResult is database.QueryResult
    assert [f.name for f in dataclasses.fields(QueryResult)] == ["session_id", "video_path", "frame_idx", "timestamp", "tags", "road_type",
                                                                  "maneuver", "risk_level", "speed_kmh"]
    import inspect
    assert list(inspect.signature(TagDatabase.__init__).parameters) == ["self", "db_path"]
    assert inspect.signature(TagDatabase.__init__).parameters["db_path"].default == "tags.db"


def test_save_all_tags_on_a_stand_in_tagger(golden):
    """save_all_tags needs .session (to_dict(), session_id) and .frame_tags (to_dict() each): the package's own dataclasses."""
    from datetime import datetime
    from multimodal_autonomous_driving_perception_and_planning_amd.database import TagDatabase
    from multimodal_autonomous_driving_perception_and_planning_amd.tagging.auto_tagger import FrameTags, TaggingSession

    class Tagger:
        session = TaggingSession(session_id="s1", video_path="v.mp4", start_time=datetime(2024, 1, 2, 3, 4, 5), total_frames=3, fps=25.0)
        frame_tags = [FrameTags(frame_idx=k, timestamp=k / 25.0, all_tags=["day"] + (["fog"] if k else []), tag_confidences={"day": 0.5})
                      for k in range(3)]
    db = TagDatabase(":memory:")
    assert db.save_all_tags(Tagger) == 3
    assert db.get_sessions() == [{"session_id": "s1", "video_path": "v.mp4", "start_time": "2024-01-02T03:04:05", "total_frames": 3, "fps": 25.0}]
    assert [r.frame_idx for r in db.search_by_tag("fog")] == [1, 2] and db.search_by_tag("fog")[0].road_type == "unknown"
    assert db.search_by_tag("fog")[0].maneuver == "lane_keeping" and db.search_by_tag("fog")[0].risk_level == "low"
    st = db.get_tag_statistics("s1")
    assert st["tag_counts"] == {"day": 3, "fog": 2} and st["risk_distribution"] == {"low": 3} and st["frame_count"] == 3
    assert dump_tables(db.conn, None)["frame_tags"] == [[1, "day", 0.5], [2, "day", 0.5], [2, "fog", 1.0], [3, "day", 0.5], [3, "fog", 1.0]]
    assert json.loads(db.export_session("s1"))["frames"] == [ft.to_dict() for ft in Tagger.frame_tags]


def test_rows_saved_without_full_data_are_rebuilt(golden):
    """A frames row whose full_data is NULL (save_tag_log(full_data=False) writes such rows) exports as a dict rebuilt from the row
    and its tags."""
    db = _filled(golden, ":memory:")
    sid, ft = golden["saves"][1]
    db.conn.execute("UPDATE frames SET full_data = NULL WHERE session_id = ? AND frame_idx = ?", (sid, ft["frame_idx"]))
    got = db.export_session(sid, format="csv")[ft["frame_idx"]]
    assert got["frame_idx"] == ft["frame_idx"] and got["timestamp"] == ft["timestamp"]
    assert sorted(got["all_tags"]) == sorted(ft["all_tags"])
    assert got["tag_confidences"] == {t: ft["tag_confidences"].get(t, 1.0) for t in ft["all_tags"]}
    assert got["scene"]["road_type"] == ft["scene"]["road_type"] and got["maneuver"]["speed_kmh"] == ft["maneuver"]["speed_kmh"]
    assert got["interaction"]["min_ttc"] == ft["interaction"]["min_ttc"]
