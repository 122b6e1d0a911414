from multimodal_autonomous_driving_perception_and_planning_amd.database import QueryResult, TagDatabase  # noqa: F401

__all__ = ["TagDatabase"]
