from .auto_tagger import AutoTagger, FrameTags, TaggingSession  # noqa: F401
from .interaction_detector import (Interaction, InteractionDetector, InteractionTags, InteractionType,  # noqa: F401
                                   RiskLevel)
from .maneuver_detector import (LateralManeuver, LongitudinalManeuver, ManeuverDetector, ManeuverTags,  # noqa: F401
                                TurningManeuver)
from .rig_interaction_detector import RigInteractionDetector  # noqa: F401
from .scene_classifier import Condition, RoadType, SceneClassifier, SceneTags, TrafficElement  # noqa: F401
from .tag_log import TAGS, TagLog, tag_mask, tags_of  # noqa: F401

__all__ = ["ManeuverDetector", "ManeuverTags", "LateralManeuver", "LongitudinalManeuver", "TurningManeuver",
           "InteractionDetector", "RigInteractionDetector", "InteractionTags", "Interaction", "InteractionType", "RiskLevel",
           "SceneClassifier", "SceneTags", "RoadType", "TrafficElement", "Condition",
           "AutoTagger", "FrameTags", "TaggingSession", "TagLog", "TAGS", "tag_mask", "tags_of"]
