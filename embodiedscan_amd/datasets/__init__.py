from .embodiedscan_dataset import EmbodiedScanDataset
from .loader import ScanLoader, shard_indices
from .loading import ScanPipeline
from .mv_3dvg_dataset import MultiView3DGroundingDataset
from .scan_grouped import ScanGroupedGrounding

__all__ = ['EmbodiedScanDataset', 'MultiView3DGroundingDataset', 'ScanGroupedGrounding', 'ScanLoader', 'ScanPipeline', 'shard_indices']
