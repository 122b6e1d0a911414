from .multi_object_tracker import MultiObjectTracker, Track
from .track_filter import TrackFilter

__all__ = ["MultiObjectTracker", "Track", "TrackFilter"]
