from multimodal_autonomous_driving_perception_and_planning_amd.tagging import (  # noqa: F401
    AutoTagger, Condition, FrameTags, Interaction, InteractionDetector, InteractionTags, InteractionType, LateralManeuver,
    LongitudinalManeuver, ManeuverDetector, ManeuverTags, RiskLevel, RoadType, SceneClassifier, SceneTags, TaggingSession,
    TrafficElement, TurningManeuver)

__all__ = ["ManeuverDetector", "InteractionDetector", "SceneClassifier", "AutoTagger"]
