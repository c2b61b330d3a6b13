"""The three inference hot-path models of the reference (``ml3d/torch/models/{randlanet,kpconv,point_pillars}.py``),
MI355X-native: same constructor arguments, parameter names / state_dict layout and data-path methods; plus PointTransformer
(``point_transformer.py``, inference) PVCNN (``pvcnn.py``, inference) and SparseConvUnet (``sparseconvnet.py``, inference), extensions beyond the original scope, and PointRCNN's first stage
(``point_rcnn.py``: backbone, heads, region proposals; the RoI stage is not built, so the class is NOT registered over the reference's)."""
from .kpconv import KPFCNN, KPConvBatch
from .point_pillars import PointPillars
from .point_rcnn import PointRCNN
from .point_transformer import PointTransformer
from .pvcnn import PVCNN
from .randlanet import RandLANet
from .sparseconvunet import SparseConvUnet

__all__ = ["RandLANet", "KPFCNN", "KPConvBatch", "PointPillars", "PointTransformer", "PVCNN", "SparseConvUnet", "PointRCNN"]
