"""SceneClassifier -- drop-in surface of src/tagging/scene_classifier.py over libavhot.so.

classify() uploads the frame through a pinned staging buffer (as LaneDetector does) and runs av_scene_classify: one
read of the frame for gray / green mask / Laplacian sums, the lane chain's Canny and PPHT on the whole frame, and the
reference's scoring, condition and vote rules.  The 5-deep road-type history lives in a device record; `history`
mirrors it with the SceneTags objects returned, like the reference's list.  The traffic-element list is built here
from the detections (it only copies their confidences, in detection order).
"""
import ctypes as C
from dataclasses import dataclass, field
from enum import Enum
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _native as nat
from .._dev import Dev, Packed


class RoadType(Enum):
    UNKNOWN = "unknown"
    INTERSECTION = "intersection"
    HIGHWAY = "highway"
    URBAN = "urban"
    RESIDENTIAL = "residential"
    PARKING = "parking"


class TrafficElement(Enum):
    TRAFFIC_LIGHT = "traffic_light"
    STOP_SIGN = "stop_sign"
    CROSSWALK = "crosswalk"
    YIELD_SIGN = "yield_sign"
    SPEED_LIMIT = "speed_limit"


class Condition(Enum):
    CLEAR = "clear"
    CONGESTED = "congested"
    NIGHT = "night"
    DAY = "day"
    RAIN = "rain"
    FOG = "fog"


_ROAD, _COND = list(RoadType), list(Condition)
_ELEMENT_OF = {'traffic_light': TrafficElement.TRAFFIC_LIGHT, 'stop_sign': TrafficElement.STOP_SIGN}


@dataclass
class SceneTags:
    """Container for scene classification results (scene_classifier.py:43-73)."""
    road_type: RoadType = RoadType.UNKNOWN
    road_type_confidence: float = 0.0
    traffic_elements: List[Tuple[TrafficElement, float]] = field(default_factory=list)
    conditions: List[Tuple[Condition, float]] = field(default_factory=list)
    lane_count: int = 0
    has_pedestrian_area: bool = False
    timestamp: float = 0.0

    def to_dict(self) -> Dict:
        return {
            'road_type': self.road_type.value,
            'road_type_confidence': self.road_type_confidence,
            'traffic_elements': [(e.value, c) for e, c in self.traffic_elements],
            'conditions': [(c.value, conf) for c, conf in self.conditions],
            'lane_count': self.lane_count,
            'has_pedestrian_area': self.has_pedestrian_area,
            'timestamp': self.timestamp
        }

    def get_tags_list(self) -> List[str]:
        tags = [self.road_type.value]
        tags.extend([e.value for e, _ in self.traffic_elements])
        tags.extend([c.value for c, _ in self.conditions])
        if self.has_pedestrian_area:
            tags.append("pedestrian_area")
        return tags


def scene_category(class_name) -> int:
    """AV_SCENE_CAT_* bits of a class name, with the reference's comparisons (:160-170, :216, :226)."""
    c = 0
    if class_name in ('traffic_light', 'stop_sign'):
        c |= nat.SCENE_CAT_TRAFFIC
    if class_name in ('car', 'truck', 'bus'):
        c |= nat.SCENE_CAT_VEHICLE
    if class_name == 'pedestrian':
        c |= nat.SCENE_CAT_PEDESTRIAN
    return c


def category_table(class_names) -> np.ndarray:
    """Per-class-id category table (u8) from the detector's names (a list, or a dict id -> name)."""
    if isinstance(class_names, dict):
        n = max(class_names) + 1 if class_names else 0
        return np.array([scene_category(class_names.get(k)) for k in range(n)], np.uint8)
    return np.array([scene_category(c) for c in class_names], np.uint8)


def lane_input(frame_shape, lanes) -> Tuple[int, float, float]:
    """(mode, left_x, right_x) of a `lanes` argument, as av_scene_classify takes it: mode 0 = lanes falsy, 1 = a lane is
    None, 2 = both present, with each lane's x at the bottom row.  Sequences follow the reference (:270-272):
    lanes[k][1] * h + lanes[k][0], or w // 3 and 2 * w // 3 when shorter than 2.  A LaneLine (anything with a
    `polynomial`) is evaluated as np.polyval(polynomial, h): the reference raises TypeError on len(LaneLine), the port
    uses the fitted line's x at the bottom row."""
    if not lanes:
        return 0, 0.0, 0.0
    if lanes[0] is None or lanes[1] is None:
        return 1, 0.0, 0.0
    h, w = frame_shape[:2]

    def x_at(lane, fallback):
        if hasattr(lane, "polynomial"):
            return float(np.polyval(lane.polynomial, h))
        return float(lane[1] * h + lane[0]) if len(lane) >= 2 else float(fallback)

    return 2, x_at(lanes[0], w // 3), x_at(lanes[1], 2 * w // 3)


def estimate_lane_count(frame_shape, lanes) -> int:
    """_estimate_lane_count (:261-280) on the host, for a truthy `lanes` (the rule scene_decide applies)."""
    mode, lx, rx = lane_input(frame_shape, lanes)
    if mode != 2:
        return 2
    lw = abs(rx - lx)
    return 3 if lw > 200 else (2 if lw > 100 else 1)


def row_to_tags(row, detections=None) -> SceneTags:
    """SceneTags from an av_scene_row (+ the traffic elements of `detections`, in detection order)."""
    t = SceneTags()
    t.road_type = _ROAD[int(row["road_type"])]
    t.road_type_confidence = float(row["confidence"])
    if detections:
        t.traffic_elements = [(_ELEMENT_OF[d.class_name], d.confidence) for d in detections
                              if hasattr(d, 'class_name') and d.class_name in _ELEMENT_OF]
        t.has_pedestrian_area = bool(row["has_pedestrian"])
    t.conditions = [(_COND[int(row["conditions"][k])], float(row["condition_conf"][k])) for k in range(int(row["n_conditions"]))]
    t.lane_count = int(row["lane_count"])
    t.timestamp = float(row["timestamp"])
    return t


class SceneClassifier:
    """Classifies driving scenes from pixels, detections and lanes (scene_classifier.py:76-303) on the GPU."""
    MAX_SEGMENTS = 4096

    def __init__(self, device: int = 0, max_segments: int = MAX_SEGMENTS):
        self.frame_count = 0
        self.history: List[SceneTags] = []
        self.smoothing_window = 5
        self.max_segments = int(max_segments)
        self._dev = Dev(device)
        self._dcap = 0
        self._io = None
        self._shape = None
        self._ws = None
        self._stage = None
        self._alloc_io(64)

    def _alloc_io(self, dcap):
        d = self._dev
        old = self._io
        self._io = Packed(d, [("state", np.uint8, (nat.SCENE_STATE_BYTES,)), ("row", np.uint8, (nat.SCENE_ROW_BYTES,)),
                              ("det_n", np.int32, (1,)), ("det_cls", np.int32, (dcap,)), ("cat", np.uint8, (8,)),
                              ("speed", np.float64, (1,)), ("lanes", np.float64, (1, 4))])
        if old is not None:
            self._io.h["state"][:] = old.h["state"]
            old.close()
        self._io.h["cat"][:] = np.arange(8, dtype=np.uint8)          # detections carry their category as the class id
        self._dcap = dcap

    def _prepare(self, h, w):
        if self._shape == (h, w):
            return
        d = self._dev
        nbytes = int(d.lib.av_scene_workspace_bytes(1, h, w, self.max_segments))
        self._ws = d.empty(nbytes, torch.uint8)
        nat.check(d.lib.av_scene_workspace_init(d.ctx.handle, d.stream, 1, h, w, self.max_segments, nat.ptr(self._ws)))
        self._stage = Packed(d, [("frame", np.uint8, (1, h, w, 3))], mapped=False)
        self._shape = (h, w)

    def classify(self, frame: np.ndarray, detections: List = None, lanes: Tuple = None, vehicle_state=None) -> SceneTags:
        frame = np.ascontiguousarray(frame, np.uint8)
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("frame must be an HxWx3 uint8 BGR image, got shape %s" % (frame.shape,))
        h, w = frame.shape[:2]
        self._prepare(h, w)
        dets = list(detections) if detections else []
        if len(dets) > self._dcap:
            self._alloc_io(max(len(dets), 2 * self._dcap))
        io = self._io
        io.h["det_n"][0] = len(dets)
        for k, det in enumerate(dets):
            io.h["det_cls"][k] = scene_category(getattr(det, 'class_name', None))
        has_speed = bool(vehicle_state) and hasattr(vehicle_state, 'speed')
        io.h["speed"][0] = float(vehicle_state.speed) if has_speed else float("nan")
        io.h["lanes"][0, :3] = lane_input(frame.shape, lanes)
        d = self._dev
        self._stage.upload_from("frame", frame[None])
        nat.check(d.lib.av_scene_classify(d.ctx.handle, d.stream, 1, h, w, self._stage.ptr("frame"), nat.ptr(self._ws),
                                          self.max_segments, io.ptr("det_n"), io.ptr("det_cls"), self._dcap, io.ptr("cat"), 8,
                                          io.ptr("speed"), io.ptr("lanes"), None, None, io.ptr("state"), io.ptr("row")))
        io.download()
        row = io.h["row"].view(nat.SCENE_ROW_FIELDS)[0]
        if row["overflow"]:
            raise RuntimeError("SceneClassifier: more than %d Hough segments in one frame (raise max_segments)" % self.max_segments)
        tags = row_to_tags(row, dets)
        # the reference appends the unsmoothed object and _smooth_tags then mutates it in place (:116-125, :296)
        self.history.append(tags)
        if len(self.history) > self.smoothing_window:
            self.history.pop(0)
        self.frame_count += 1
        self.last_row = row.copy()
        return tags

    def _estimate_lane_count(self, frame: np.ndarray, lanes: Tuple) -> int:
        return estimate_lane_count(frame.shape, lanes)

    def reset(self):
        self.frame_count = 0
        self.history = []
        self._io.h["state"][:] = 0
