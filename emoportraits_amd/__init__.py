from .controls import CropTracking, ExpressionControls, HeadPoseControls  # noqa: F401
