from multimodal_autonomous_driving_perception_and_planning_amd.tagging.scene_classifier import *  # noqa: F401,F403
from multimodal_autonomous_driving_perception_and_planning_amd.tagging.scene_classifier import (  # noqa: F401
    Condition, RoadType, SceneClassifier, SceneTags, TrafficElement)
