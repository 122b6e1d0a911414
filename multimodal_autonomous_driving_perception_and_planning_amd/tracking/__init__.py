from .multi_object_tracker import MultiObjectTracker, Track
from .rig_tracker import RigTracker
from .track_filter import TrackFilter

__all__ = ["MultiObjectTracker", "Track", "TrackFilter", "RigTracker"]
