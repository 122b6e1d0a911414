"""AutoTagger -- drop-in surface of src/tagging/auto_tagger.py.

Joins the port's three taggers per frame (SceneClassifier, ManeuverDetector, InteractionDetector, each on the GPU)
and keeps the reference's host-side bookkeeping (auto_tagger.py:74-372): the frame's tag list in first-seen order,
per-tag confidences (later writers win), tag counts, searches, event segments and the dict / JSON / CSV exports.
This part is aggregation over a few strings per frame and has no kernel.  Its batched counterpart, for S streams with the
tags kept and searched on the device, is tagging/tag_log.py (TagLog).
"""
import json
from dataclasses import dataclass, field
from datetime import datetime
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .interaction_detector import InteractionDetector, InteractionTags
from .maneuver_detector import ManeuverDetector, ManeuverTags
from .scene_classifier import SceneClassifier, SceneTags


@dataclass
class FrameTags:
    """Every tag of one frame (auto_tagger.py:18-49)."""
    frame_idx: int
    timestamp: float
    scene: SceneTags = None
    maneuver: ManeuverTags = None
    interaction: InteractionTags = None
    all_tags: List[str] = field(default_factory=list)
    tag_confidences: Dict[str, float] = field(default_factory=dict)

    def to_dict(self) -> Dict:
        return {'frame_idx': self.frame_idx, 'timestamp': self.timestamp,
                'scene': self.scene.to_dict() if self.scene else {},
                'maneuver': self.maneuver.to_dict() if self.maneuver else {},
                'interaction': self.interaction.to_dict() if self.interaction else {},
                'all_tags': self.all_tags, 'tag_confidences': self.tag_confidences}

    def get_summary_string(self) -> str:
        parts = []
        if self.scene:
            parts.append("Scene: %s" % self.scene.road_type.value)
        if self.maneuver:
            parts.append("Maneuver: %s, %s" % (self.maneuver.lateral.value, self.maneuver.longitudinal.value))
        if self.interaction and self.interaction.primary_interaction:
            parts.append("Interaction: %s" % self.interaction.primary_interaction.value)
        return " | ".join(parts) if parts else "No tags"


@dataclass
class TaggingSession:
    """Session metadata (auto_tagger.py:52-71)."""
    session_id: str
    video_path: str
    start_time: datetime
    end_time: Optional[datetime] = None
    total_frames: int = 0
    fps: float = 30.0

    def to_dict(self) -> Dict:
        return {'session_id': self.session_id, 'video_path': self.video_path, 'start_time': self.start_time.isoformat(),
                'end_time': self.end_time.isoformat() if self.end_time else None, 'total_frames': self.total_frames,
                'fps': self.fps}


def _new_session(video_path, fps):
    now = datetime.now()
    return TaggingSession(session_id=now.strftime("%Y%m%d_%H%M%S"), video_path=video_path, start_time=now, fps=fps)


class AutoTagger:
    """Scene + maneuver + interaction tags per frame, searchable (auto_tagger.py:74-372)."""

    def __init__(self, video_path: str = "unknown", fps: float = 30.0, device: int = 0):
        self.scene_classifier = SceneClassifier(device=device)
        self.maneuver_detector = ManeuverDetector(device=device)
        self.interaction_detector = InteractionDetector(device=device)
        self.session = _new_session(video_path, fps)
        self.frame_tags: List[FrameTags] = []
        self.tag_counts: Dict[str, int] = {}
        self.frame_count = 0

    def tag_frame(self, frame: np.ndarray, detections: List = None, tracks: List = None, lanes: Tuple = None,
                  vehicle_state=None) -> FrameTags:
        timestamp = self.frame_count / self.session.fps
        scene = self.scene_classifier.classify(frame, detections, lanes, vehicle_state)
        # the reference's placeholder lane offset: 0.0 when both lanes are present, else None (:134-140)
        offset = 0.0 if (lanes and lanes[0] is not None and lanes[1] is not None) else None
        maneuver = self.maneuver_detector.detect(vehicle_state, offset)
        interaction = self.interaction_detector.detect(tracks, vehicle_state, frame.shape[:2])
        tags, conf = [], {}
        if scene:
            tags += scene.get_tags_list()
            conf[scene.road_type.value] = scene.road_type_confidence
            conf.update((e.value, c) for e, c in scene.traffic_elements)
        if maneuver:
            tags += maneuver.get_tags_list()
            conf[maneuver.lateral.value] = maneuver.lateral_confidence
            conf[maneuver.longitudinal.value] = maneuver.longitudinal_confidence
            conf[maneuver.turning.value] = maneuver.turning_confidence
        if interaction:
            tags += interaction.get_tags_list()
            conf.update((i.type.value, i.confidence) for i in interaction.interactions)
        unique = list(dict.fromkeys(tags))
        ft = FrameTags(frame_idx=self.frame_count, timestamp=timestamp, scene=scene, maneuver=maneuver,
                       interaction=interaction, all_tags=unique, tag_confidences=conf)
        for t in unique:
            self.tag_counts[t] = self.tag_counts.get(t, 0) + 1
        self.frame_tags.append(ft)
        self.frame_count += 1
        self.session.total_frames = self.frame_count
        return ft

    def get_tag_statistics(self) -> Dict:
        if not self.frame_tags:
            return {}
        n = len(self.frame_tags)
        freq = sorted(((t, c / n) for t, c in self.tag_counts.items()), key=lambda kv: kv[1], reverse=True)
        speeds = [ft.maneuver.speed_kmh for ft in self.frame_tags if ft.maneuver]
        risk = {'low': 0, 'medium': 0, 'high': 0, 'critical': 0}
        for ft in self.frame_tags:
            if ft.interaction:
                risk[ft.interaction.overall_risk.value] += 1
        return {'total_frames': n, 'unique_tags': len(self.tag_counts), 'tag_frequency': dict(freq[:20]),
                'tag_counts': self.tag_counts,
                'speed_stats': {'min': min(speeds) if speeds else 0, 'max': max(speeds) if speeds else 0,
                                'avg': np.mean(speeds) if speeds else 0},
                'risk_distribution': risk, 'session_info': self.session.to_dict()}

    def search_by_tag(self, tag: str) -> List[FrameTags]:
        return [ft for ft in self.frame_tags if tag in ft.all_tags]

    def search_by_tags(self, tags: List[str], match_all: bool = True) -> List[FrameTags]:
        test = all if match_all else any
        return [ft for ft in self.frame_tags if test(t in ft.all_tags for t in tags)]

    def get_high_risk_frames(self) -> List[FrameTags]:
        return [ft for ft in self.frame_tags if ft.interaction and ft.interaction.overall_risk.value in ('high', 'critical')]

    def get_event_segments(self, event_tag: str, min_duration: int = 5) -> List[Tuple[int, int]]:
        """Maximal runs of frames carrying `event_tag`, at least min_duration long, as (first, last) frame indices."""
        segs, start = [], None
        for i, ft in enumerate(self.frame_tags + [None]):
            on = ft is not None and event_tag in ft.all_tags
            if on and start is None:
                start = i
            elif not on and start is not None:
                if i - start >= min_duration:
                    segs.append((start, i - 1))
                start = None
        return segs

    def export_tags(self, format: str = 'dict') -> Any:
        if format == 'dict':
            return {'session': self.session.to_dict(), 'statistics': self.get_tag_statistics(),
                    'frames': [ft.to_dict() for ft in self.frame_tags]}
        if format == 'json':
            return json.dumps(self.export_tags('dict'), indent=2)
        if format == 'csv':
            rows = []
            for ft in self.frame_tags:
                s, m, it = ft.scene, ft.maneuver, ft.interaction
                rows.append({'frame_idx': ft.frame_idx, 'timestamp': ft.timestamp,
                             'road_type': s.road_type.value if s else '',
                             'lateral_maneuver': m.lateral.value if m else '',
                             'longitudinal_maneuver': m.longitudinal.value if m else '',
                             'turning_maneuver': m.turning.value if m else '',
                             'speed_kmh': m.speed_kmh if m else 0,
                             'risk_level': it.overall_risk.value if it else 'low',
                             'agent_count': it.agent_count if it else 0,
                             'all_tags': '|'.join(ft.all_tags)})
            return rows
        return None

    def reset(self):
        self.scene_classifier.reset()
        self.maneuver_detector.reset()
        self.interaction_detector.reset()
        self.frame_tags = []
        self.tag_counts = {}
        self.frame_count = 0
        self.session = _new_session(self.session.video_path, self.session.fps)

    def finalize(self):
        self.session.end_time = datetime.now()
        self.session.total_frames = self.frame_count
