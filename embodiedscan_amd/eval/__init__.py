from .det_metric import IndoorDetMetric, gather_results
from .grounding_metric import GroundingMetric
from .indoor_eval import indoor_eval
from .occupancy_metric import OccupancyMetric

__all__ = ['GroundingMetric', 'IndoorDetMetric', 'OccupancyMetric', 'gather_results', 'indoor_eval']
