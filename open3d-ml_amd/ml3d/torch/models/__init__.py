"""The three inference hot-path models of the reference (``ml3d/torch/models/{randlanet,kpconv,point_pillars}.py``),
MI355X-native: same constructor arguments, parameter names / state_dict layout and data-path methods; plus PointTransformer
(``point_transformer.py``, inference) and PVCNN (``pvcnn.py``, inference), extensions beyond the original scope."""
from .kpconv import KPFCNN, KPConvBatch
from .point_pillars import PointPillars
from .point_transformer import PointTransformer
from .pvcnn import PVCNN
from .randlanet import RandLANet

__all__ = ["RandLANet", "KPFCNN", "KPConvBatch", "PointPillars", "PointTransformer", "PVCNN"]
