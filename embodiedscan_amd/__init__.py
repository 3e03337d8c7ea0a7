from . import eval  # noqa: F401  (registers IndoorDetMetric in registry.METRICS)
