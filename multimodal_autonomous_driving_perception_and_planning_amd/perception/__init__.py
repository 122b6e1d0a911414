from .calibration import CameraCalibration, CameraRig, LensModel
from .detector import Detection, ObjectDetector
from .ground_odometry import GroundOdometry
from .lane_detector import LaneDetector, LaneLine
from .rig_odometry import RigOdometry

__all__ = ["ObjectDetector", "LaneDetector", "Detection", "LaneLine", "CameraCalibration", "LensModel", "CameraRig", "GroundOdometry",
           "RigOdometry"]
