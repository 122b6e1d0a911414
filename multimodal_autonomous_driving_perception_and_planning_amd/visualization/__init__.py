from .bev_renderer import BEVRenderer
from .overlays import OverlayRenderer
from .surround_view import SurroundView

__all__ = ["BEVRenderer", "OverlayRenderer", "SurroundView"]
