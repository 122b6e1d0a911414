from .video_loader import VideoDataLoader, MJPEGWriter, VideoFeed, Y4MWriter  # noqa: F401

__all__ = ["VideoDataLoader", "VideoFeed", "Y4MWriter", "MJPEGWriter"]
