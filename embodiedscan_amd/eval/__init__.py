from .det_metric import IndoorDetMetric, gather_results
from .indoor_eval import indoor_eval

__all__ = ['IndoorDetMetric', 'gather_results', 'indoor_eval']
