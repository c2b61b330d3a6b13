"""``ml3d.metrics``: detection scoring (the reference's ml3d/metrics package) on ``ops.det_match``."""
from ..ops import iou_bev, iou_3d   # noqa: F401
from .mAP import filter_data, precision_3d, sample_thresholds, mAP, ObjdetMetric   # noqa: F401

__all__ = ["precision_3d", "mAP", "iou_bev", "iou_3d", "filter_data", "sample_thresholds", "ObjdetMetric"]
