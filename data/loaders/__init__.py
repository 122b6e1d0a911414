from .video_loader import VideoDataLoader, Y4MWriter  # noqa: F401

__all__ = ["VideoDataLoader", "Y4MWriter"]
