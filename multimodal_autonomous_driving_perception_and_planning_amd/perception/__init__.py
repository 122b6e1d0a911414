from .calibration import CameraCalibration, CameraRig, LensModel
from .detector import Detection, ObjectDetector
from .ground_odometry import GroundOdometry
from .lane_detector import LaneDetector, LaneLine
from .rig_odometry import RigOdometry
from .road_lanes import RoadLanes
from .road_marks import RoadMarks

__all__ = ["ObjectDetector", "LaneDetector", "Detection", "LaneLine", "CameraCalibration", "LensModel", "CameraRig", "GroundOdometry",
           "RigOdometry", "RoadLanes", "RoadMarks"]
