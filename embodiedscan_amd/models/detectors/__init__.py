from .embodied_occ import EmbodiedOccPredictor  # noqa: F401
