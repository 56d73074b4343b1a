from .controls import ExpressionControls  # noqa: F401
