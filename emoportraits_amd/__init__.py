from .controls import ExpressionControls, HeadPoseControls  # noqa: F401
