"""TagDatabase -- drop-in surface of src/database/tag_database.py: auto-tagging results in an SQLite file.

The file format is the reference's: the tables sessions / tags / frames / frame_tags with its columns and indexes, so a file
written here opens in the reference's class and the other way round.  The per-frame methods (save_session, save_frame_tags,
save_all_tags, the searches, statistics, export, delete) behave as the reference's do, its INSERT OR REPLACE included: saving a
frame again gives it a new row id and leaves the old frame_tags rows behind, which the global statistics count and the
per-session ones do not.  This is host-side bookkeeping over a few strings per frame and has no kernel.

save_tag_log is this package's addition: a device-resident TagLog (tagging/tag_log.py) written in bulk, one session per stream.
It is defined as save_session + save_frame_tags(frame_dict(...)) per frame and implemented as one download of the log, NumPy
decoding and executemany inside one transaction.

Deviations.  frame_tags.confidence of a tag log's traffic-element and interaction-type tags is the column default 1.0 (the log
keeps no per-tag confidence for those; no query reads the column); a tag log's all_tags are in vocabulary order, not first-seen
order.  search_by_multiple_tags(match_all=False) does not append its SQL parameters to the caller's tag list as the reference
does, so QueryResult.tags is the list that was passed.
"""
import json
import sqlite3
from dataclasses import dataclass
from datetime import datetime
from pathlib import Path
from typing import Any, Dict, List

import numpy as np

_SCHEMA = (
    """CREATE TABLE IF NOT EXISTS sessions (
        session_id TEXT PRIMARY KEY, video_path TEXT NOT NULL, start_time TEXT NOT NULL, end_time TEXT,
        total_frames INTEGER DEFAULT 0, fps REAL DEFAULT 30.0, metadata TEXT)""",
    """CREATE TABLE IF NOT EXISTS tags (
        tag_id INTEGER PRIMARY KEY AUTOINCREMENT, tag_name TEXT UNIQUE NOT NULL, tag_category TEXT,
        created_at TEXT DEFAULT CURRENT_TIMESTAMP)""",
    """CREATE TABLE IF NOT EXISTS frames (
        id INTEGER PRIMARY KEY AUTOINCREMENT, session_id TEXT NOT NULL, frame_idx INTEGER NOT NULL, timestamp REAL NOT NULL,
        road_type TEXT, road_type_confidence REAL, lateral_maneuver TEXT, longitudinal_maneuver TEXT, turning_maneuver TEXT,
        speed_kmh REAL, acceleration REAL, risk_level TEXT, agent_count INTEGER DEFAULT 0, pedestrian_count INTEGER DEFAULT 0,
        vehicle_count INTEGER DEFAULT 0, min_ttc REAL, closest_distance REAL, full_data TEXT,
        FOREIGN KEY (session_id) REFERENCES sessions(session_id), UNIQUE(session_id, frame_idx))""",
    """CREATE TABLE IF NOT EXISTS frame_tags (
        frame_id INTEGER NOT NULL, tag_id INTEGER NOT NULL, confidence REAL DEFAULT 1.0, PRIMARY KEY (frame_id, tag_id),
        FOREIGN KEY (frame_id) REFERENCES frames(id), FOREIGN KEY (tag_id) REFERENCES tags(tag_id))""",
    "CREATE INDEX IF NOT EXISTS idx_frames_session ON frames(session_id)",
    "CREATE INDEX IF NOT EXISTS idx_frames_road_type ON frames(road_type)",
    "CREATE INDEX IF NOT EXISTS idx_frames_risk ON frames(risk_level)",
    "CREATE INDEX IF NOT EXISTS idx_tags_name ON tags(tag_name)",
)
_PUT_SESSION = ("INSERT OR REPLACE INTO sessions (session_id, video_path, start_time, end_time, total_frames, fps, metadata) "
                "VALUES (?, ?, ?, ?, ?, ?, ?)")
_FRAME_COLUMNS = ("session_id", "frame_idx", "timestamp", "road_type", "road_type_confidence", "lateral_maneuver",
                  "longitudinal_maneuver", "turning_maneuver", "speed_kmh", "acceleration", "risk_level", "agent_count",
                  "pedestrian_count", "vehicle_count", "min_ttc", "closest_distance", "full_data")
_PUT_FRAME = "INSERT OR REPLACE INTO frames (%s) VALUES (%s)" % (", ".join(_FRAME_COLUMNS), ", ".join("?" * len(_FRAME_COLUMNS)))
_PUT_TAG = "INSERT OR IGNORE INTO tags (tag_name) VALUES (?)"
_PUT_FRAME_TAG = "INSERT OR REPLACE INTO frame_tags (frame_id, tag_id, confidence) VALUES (?, ?, ?)"
# what every search returns of a frame
_HIT = ("f.session_id, s.video_path, f.frame_idx, f.timestamp, f.road_type, f.lateral_maneuver, f.risk_level, f.speed_kmh "
        "FROM frames f JOIN sessions s ON f.session_id = s.session_id")
_TAGGED = _HIT + " JOIN frame_tags ft ON f.id = ft.frame_id JOIN tags t ON ft.tag_id = t.tag_id"


@dataclass
class QueryResult:
    """One frame found by a search."""
    session_id: str
    video_path: str
    frame_idx: int
    timestamp: float
    tags: List[str]
    road_type: str
    maneuver: str
    risk_level: str
    speed_kmh: float


def _session_row(d):
    return (d.get('session_id'), d.get('video_path'), d.get('start_time'), d.get('end_time'), d.get('total_frames', 0),
            d.get('fps', 30.0), json.dumps(d))


def _frame_row(session_id, ft, full_data=True):
    """The frames row of one FrameTags.to_dict(), with the reference's defaults for what the dict lacks."""
    scene, man, inter = ft.get('scene', {}), ft.get('maneuver', {}), ft.get('interaction', {})
    return (session_id, ft.get('frame_idx', 0), ft.get('timestamp', 0), scene.get('road_type', 'unknown'),
            scene.get('road_type_confidence', 0), man.get('lateral', 'lane_keeping'), man.get('longitudinal', 'cruising'),
            man.get('turning', 'straight'), man.get('speed_kmh', 0), man.get('acceleration', 0), inter.get('overall_risk', 'low'),
            inter.get('agent_count', 0), inter.get('pedestrian_count', 0), inter.get('vehicle_count', 0), inter.get('min_ttc'),
            inter.get('closest_agent_distance'), json.dumps(ft) if full_data else None)


def tag_log_session(session_id, video_path, start_time, n_frames, fps, stream, dropped):
    """The session dict save_tag_log stores for one stream of a TagLog (`dropped`: frames the full log turned away)."""
    return {'session_id': session_id, 'video_path': video_path, 'start_time': start_time.isoformat(), 'end_time': None,
            'total_frames': int(n_frames), 'fps': float(fps), 'stream': int(stream), 'dropped': int(dropped)}


class TagDatabase:
    """sessions (one per tagged video), frames (one row per frame), tags (the names) and frame_tags (which frame carries which)."""

    def __init__(self, db_path: str = "tags.db"):
        self.db_path = Path(db_path)
        self.conn = sqlite3.connect(str(self.db_path), check_same_thread=False)
        self.conn.row_factory = sqlite3.Row
        for statement in _SCHEMA:
            self.conn.execute(statement)
        self.conn.commit()

    # ---- writing ---------------------------------------------------------------------------------------------------
    def save_session(self, session_data: Dict) -> str:
        self.conn.execute(_PUT_SESSION, _session_row(session_data))
        self.conn.commit()
        return session_data.get('session_id')

    def _tag_id(self, cur, name):
        cur.execute(_PUT_TAG, (name,))
        return cur.execute("SELECT tag_id FROM tags WHERE tag_name = ?", (name,)).fetchone()[0]

    def save_frame_tags(self, session_id: str, frame_tags: Dict) -> int:
        """One FrameTags.to_dict(); returns the frame's row id.  A frame saved again gets a new row id."""
        cur = self.conn.cursor()
        cur.execute(_PUT_FRAME, _frame_row(session_id, frame_tags))
        frame_id = cur.lastrowid
        conf = frame_tags.get('tag_confidences', {})
        for name in frame_tags.get('all_tags', []):
            cur.execute(_PUT_FRAME_TAG, (frame_id, self._tag_id(cur, name), conf.get(name, 1.0)))
        self.conn.commit()
        return frame_id

    def save_all_tags(self, auto_tagger) -> int:
        """An AutoTagger's session and every FrameTags it holds; returns the number of frames."""
        self.save_session(auto_tagger.session.to_dict())
        for ft in auto_tagger.frame_tags:
            self.save_frame_tags(auto_tagger.session.session_id, ft.to_dict())
        return len(auto_tagger.frame_tags)

    def save_tag_log(self, log, video_paths=None, fps=30.0, session_ids=None, start_time=None, full_data=True) -> List[str]:
        """Every stream of a TagLog as a session of its own (default id <YYYYmmdd_HHMMSS>_s<stream:03d>); returns the ids.
        Equal, for every stream and frame, to save_session(tag_log_session(...)) followed by
        save_frame_tags(session_id, frame_dict(frame, mask, speed, record, fps)), but written as one transaction.
        full_data=False leaves frames.full_data NULL (export_session then rebuilds a frame from its row and tags): for logs
        whose JSON would dwarf the rest.  The frames a full log turned away are reported in the session's metadata."""
        from ..tagging import tag_log as T
        n = log.lengths()
        top = max(int(n.max()), 1)
        masks = log.mask[:, :top].cpu().numpy().view(np.uint64)
        speeds = log.speed[:, :top].cpu().numpy()
        cols = log.cols[:, :top].cpu().numpy().reshape(log.S, -1).view(T.COLS_DTYPE) if log.columns else None
        dropped = log.dropped.cpu().numpy()
        start_time = start_time or datetime.now()
        stamp = start_time.strftime("%Y%m%d_%H%M%S")
        ids = list(session_ids) if session_ids is not None else ["%s_s%03d" % (stamp, s) for s in range(log.S)]
        paths = list(video_paths) if video_paths is not None else ["stream_%03d" % s for s in range(log.S)]
        if len(ids) != log.S or len(paths) != log.S:
            raise ValueError("session_ids and video_paths name every stream of the log")
        cur = self.conn.cursor()
        try:
            for s in range(log.S):
                k = int(n[s])
                cur.execute(_PUT_SESSION, _session_row(tag_log_session(ids[s], paths[s], start_time, k, fps, s, dropped[s])))
                if k:
                    self._put_stream(cur, ids[s], masks[s, :k], speeds[s, :k], None if cols is None else cols[s, :k], fps,
                                     full_data, T)
            self.conn.commit()
        except Exception:
            self.conn.rollback()
            raise
        return ids

    def _put_stream(self, cur, session_id, masks, speeds, cols, fps, full_data, T):
        """One stream's frames rows, new tag names (in the order the per-frame path meets them) and frame_tags rows."""
        n = len(masks)
        frames = np.arange(n)
        has = lambda bit: ((masks >> np.uint64(bit)) & np.uint64(1)).astype(bool)           # noqa: E731
        scene, man, inter = has(T.HAS_SCENE), has(T.HAS_MANEUVER), has(T.HAS_INTERACTION)

        def group(base, count, names, present, default):
            """(name per frame, index of the group's highest set bit or -1): the enum a frame's dict names, the reference's
            default where the group is absent or carries no bit."""
            field = (masks >> np.uint64(base)) & np.uint64((1 << count) - 1)
            top = np.full(n, -1)
            for k in range(count):
                top[(field >> np.uint64(k)) != 0] = k
            top[~present] = -1
            return [names[k] if k >= 0 else default for k in top.tolist()], top
        tags = T.TAGS
        road, road_top = group(T.ROAD_TYPE, 6, tags[T.ROAD_TYPE:], scene, 'unknown')
        lat, lat_top = group(T.LATERAL, 4, tags[T.LATERAL:], man, 'lane_keeping')
        lon, lon_top = group(T.LONGITUDINAL, 5, tags[T.LONGITUDINAL:], man, 'cruising')
        trn, trn_top = group(T.TURNING, 6, tags[T.TURNING:], man, 'straight')
        risk_bits = ((masks >> np.uint64(T.RISK)) & np.uint64(7)).astype(np.int64)
        risk_idx = np.where(inter, np.floor(np.log2(np.maximum(risk_bits, 1))).astype(np.int64) + (risk_bits > 0), 0)
        risk = [T._RISKS[k] for k in risk_idx.tolist()]
        zero = [0] * n
        if cols is not None:
            col = lambda name, present: np.where(present, cols[name], 0).tolist()           # noqa: E731
            none_if_nan = lambda name: [None if (v != v or not p) else v                     # noqa: E731
                                        for v, p in zip(cols[name].tolist(), inter.tolist())]
            # (an absent group is the integer 0 in the per-frame path and 0.0 here: one value in a REAL column)
            road_conf, accel = col("road_type_confidence", scene), col("acceleration", man)
            agents, peds, vehicles = col("agent_count", inter), col("pedestrian_count", inter), col("vehicle_count", inter)
            ttc, dist = none_if_nan("min_ttc"), none_if_nan("closest_distance")
        else:
            road_conf = accel = agents = peds = vehicles = zero
            ttc = dist = [None] * n
        speed = np.where(man, speeds, 0.0).tolist()
        stamps = [k / float(fps) for k in range(n)]
        if full_data:
            full = [json.dumps(T.frame_dict(k, masks[k], speeds[k], None if cols is None else cols[k], fps)) for k in range(n)]
        else:
            full = [None] * n
        cur.executemany(_PUT_FRAME, zip([session_id] * n, frames.tolist(), stamps, road, road_conf, lat, lon, trn, speed, accel, risk,
                                        agents, peds, vehicles, ttc, dist, full))
        row_id = np.zeros(n, np.int64)
        for rid, k in cur.execute("SELECT id, frame_idx FROM frames WHERE session_id = ? AND frame_idx < ?", (session_id, n)):
            row_id[k] = rid
        # tags: bit b of frame k; new names enter the tags table ordered by (first frame, bit), as frame-by-frame saving does
        on = [np.flatnonzero(has(b)) for b in range(len(tags))]
        order = sorted((int(on[b][0]), b) for b in range(len(tags)) if len(on[b]))
        tag_id = {b: self._tag_id(cur, tags[b]) for _, b in order}
        conf_of = {}                         # bit -> per-frame confidences, for the tags frame_dict gives one
        if cols is not None:
            for base, top, name in ((T.ROAD_TYPE, road_top, "road_type_confidence"), (T.LATERAL, lat_top, "lateral_confidence"),
                                    (T.LONGITUDINAL, lon_top, "longitudinal_confidence"), (T.TURNING, trn_top, "turning_confidence")):
                for b in set((top[top >= 0] + base).tolist()):
                    conf_of[b] = np.where(top + base == b, cols[name], 1.0)
        for _, b in order:
            c = conf_of[b][on[b]].tolist() if b in conf_of else [1.0] * len(on[b])
            cur.executemany(_PUT_FRAME_TAG, zip(row_id[on[b]].tolist(), [tag_id[b]] * len(on[b]), c))

    # ---- searching -------------------------------------------------------------------------------------------------
    def _hits(self, query, params, session_id, limit, tags):
        if session_id:
            query += " AND f.session_id = ?"
            params = params + [session_id]
        rows = self.conn.execute(query + " ORDER BY f.session_id, f.frame_idx LIMIT ?", params + [limit]).fetchall()
        return [QueryResult(session_id=r['session_id'], video_path=r['video_path'], frame_idx=r['frame_idx'], timestamp=r['timestamp'],
                            tags=tags, road_type=r['road_type'], maneuver=r['lateral_maneuver'], risk_level=r['risk_level'],
                            speed_kmh=r['speed_kmh']) for r in rows]

    def search_by_tag(self, tag_name: str, session_id: str = None, limit: int = 100) -> List[QueryResult]:
        return self._hits("SELECT DISTINCT " + _TAGGED + " WHERE t.tag_name = ?", [tag_name], session_id, limit, [tag_name])

    def search_by_multiple_tags(self, tags: List[str], match_all: bool = True, session_id: str = None,
                                limit: int = 100) -> List[QueryResult]:
        """Frames carrying all of `tags` (as many distinct names as the list is long: a repeated tag matches nothing) or any."""
        marks = ",".join("?" * len(tags))
        if match_all:
            query = ("SELECT " + _HIT + " WHERE f.id IN (SELECT frame_id FROM frame_tags ft JOIN tags t ON ft.tag_id = t.tag_id "
                     "WHERE t.tag_name IN (%s) GROUP BY frame_id HAVING COUNT(DISTINCT t.tag_name) = ?)" % marks)
            return self._hits(query, list(tags) + [len(tags)], session_id, limit, tags)
        return self._hits("SELECT DISTINCT " + _TAGGED + " WHERE t.tag_name IN (%s)" % marks, list(tags), session_id, limit, tags)

    def search_high_risk(self, session_id: str = None, limit: int = 100) -> List[QueryResult]:
        return self._hits("SELECT " + _HIT + " WHERE f.risk_level IN ('high', 'critical')", [], session_id, limit, ['high_risk'])

    def get_tag_statistics(self, session_id: str = None) -> Dict:
        """Counts per tag and risk level, over one session or the whole file.  The whole-file tag counts go over every
        frame_tags row, those a re-saved frame left behind included; the per-session ones join the live frames."""
        one = (session_id,) if session_id else ()
        counts = ("SELECT t.tag_name, COUNT(*) AS count FROM tags t JOIN frame_tags ft ON t.tag_id = ft.tag_id %s"
                  "GROUP BY t.tag_name ORDER BY count DESC" % ("JOIN frames f ON ft.frame_id = f.id WHERE f.session_id = ? " if one else ""))
        only = " WHERE session_id = ?" if one else ""
        tag_counts = {r[0]: r[1] for r in self.conn.execute(counts, one)}
        risks = self.conn.execute("SELECT risk_level, COUNT(*) FROM frames%s GROUP BY risk_level" % only, one)
        return {'session_count': self.conn.execute("SELECT COUNT(*) FROM sessions").fetchone()[0],
                'frame_count': self.conn.execute("SELECT COUNT(*) FROM frames" + only, one).fetchone()[0],
                'tag_counts': tag_counts, 'risk_distribution': {r[0]: r[1] for r in risks}, 'unique_tags': len(tag_counts)}

    def get_sessions(self) -> List[Dict]:
        rows = self.conn.execute("SELECT session_id, video_path, start_time, total_frames, fps FROM sessions ORDER BY start_time DESC")
        return [dict(r) for r in rows]

    def _rebuilt_frame(self, row):
        """A frame's dict from its row and tags, for rows saved without full_data."""
        pairs = self.conn.execute("SELECT t.tag_name, ft.confidence FROM frame_tags ft JOIN tags t ON ft.tag_id = t.tag_id "
                                  "WHERE ft.frame_id = ? ORDER BY t.tag_id", (row['id'],)).fetchall()
        return {'frame_idx': row['frame_idx'], 'timestamp': row['timestamp'],
                'scene': {'road_type': row['road_type'], 'road_type_confidence': row['road_type_confidence']},
                'maneuver': {'lateral': row['lateral_maneuver'], 'longitudinal': row['longitudinal_maneuver'],
                             'turning': row['turning_maneuver'], 'speed_kmh': row['speed_kmh'], 'acceleration': row['acceleration']},
                'interaction': {'overall_risk': row['risk_level'], 'agent_count': row['agent_count'],
                                'pedestrian_count': row['pedestrian_count'], 'vehicle_count': row['vehicle_count'],
                                'closest_agent_distance': row['closest_distance'], 'min_ttc': row['min_ttc']},
                'all_tags': [p[0] for p in pairs], 'tag_confidences': {p[0]: p[1] for p in pairs}}

    def export_session(self, session_id: str, format: str = 'json') -> Any:
        """'json': a JSON text of {'session', 'frames'}; 'csv': the list of frame dicts; anything else: None."""
        session = self.conn.execute("SELECT * FROM sessions WHERE session_id = ?", (session_id,)).fetchone()
        if session is None:
            raise KeyError("no session %r" % (session_id,))
        rows = self.conn.execute("SELECT * FROM frames WHERE session_id = ? ORDER BY frame_idx", (session_id,)).fetchall()
        frames = [json.loads(r['full_data']) if r['full_data'] is not None else self._rebuilt_frame(r) for r in rows]
        if format == 'json':
            return json.dumps({'session': dict(session), 'frames': frames}, indent=2)
        return frames if format == 'csv' else None

    def delete_session(self, session_id: str):
        """The session, its frames and their frame_tags rows (tag names stay)."""
        self.conn.execute("DELETE FROM frame_tags WHERE frame_id IN (SELECT id FROM frames WHERE session_id = ?)", (session_id,))
        self.conn.execute("DELETE FROM frames WHERE session_id = ?", (session_id,))
        self.conn.execute("DELETE FROM sessions WHERE session_id = ?", (session_id,))
        self.conn.commit()

    def close(self):
        if getattr(self, "conn", None):
            self.conn.close()
            self.conn = None

    def __del__(self):
        self.close()
