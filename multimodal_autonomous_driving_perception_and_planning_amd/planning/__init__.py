from .lane_planner import LanePlanner
from .motion_planner import MotionPlanner, Trajectory, Waypoint

__all__ = ["LanePlanner", "MotionPlanner", "Trajectory", "Waypoint"]
