from multimodal_autonomous_driving_perception_and_planning_amd.tracking import MultiObjectTracker, RigTracker, Track, TrackFilter  # noqa: F401

__all__ = ["MultiObjectTracker", "Track", "TrackFilter", "RigTracker"]
