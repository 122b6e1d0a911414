from multimodal_autonomous_driving_perception_and_planning_amd.tagging.auto_tagger import (  # noqa: F401
    AutoTagger, FrameTags, TaggingSession)
