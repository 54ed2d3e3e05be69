from .triple import TripletLoss  # noqa: F401
from .pycda import PyramidCurriculumLoss  # noqa: F401
from .overlap import DiceLoss, JaccardLoss, TverskyLoss  # noqa: F401
