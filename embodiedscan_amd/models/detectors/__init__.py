from .embodied_occ import EmbodiedOccPredictor  # noqa: F401
from .embodied_det3d import Embodied3DDetector  # noqa: F401
