from .bev_renderer import BEVRenderer
from .overlays import OverlayRenderer
from .road_memory import RoadMemory
from .surround_view import SurroundView

__all__ = ["BEVRenderer", "OverlayRenderer", "RoadMemory", "SurroundView"]
