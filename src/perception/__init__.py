from multimodal_autonomous_driving_perception_and_planning_amd.perception import (  # noqa: F401
    CameraCalibration, CameraRig, Detection, LaneDetector, LaneLine, LensModel, ObjectDetector)

__all__ = ["ObjectDetector", "LaneDetector", "CameraCalibration", "LensModel", "CameraRig"]
