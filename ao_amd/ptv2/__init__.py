"""State_dict-compatible PT-v2m2 ("PT-v2m2") on the MI355X ops."""
from .model import (  # noqa: F401
    Block,
    BlockSequence,
    Decoder,
    Encoder,
    GridPool,
    GroupedLinear,
    GroupedVectorAttention,
    GVAPatchEmbed,
    PointBatchNorm,
    PointTransformerV2,
    PointTransformerV2M1,
    UnpoolWithSkip,
    build_from_cfg,
)
from .basket import LogitBasket  # noqa: F401
from .segmentor import DefaultSegmentor, DefaultSegmentorSAM_Image, S3DIS_BACKBONE, SCANNET_BACKBONE  # noqa: F401
from .losses import LovaszLoss, lovasz_softmax  # noqa: F401
from .cac import CACSegmentor  # noqa: F401
from .tester import SemSegTester, VoteTable, test_scene  # noqa: F401
from .refine import LabelRefiner, grid_cells, grid_prompts, refine_scene, scene_confidence  # noqa: F401
from .pp2s import (LabelPropagator, align_room, bridge_to_numpy, choose_weak_labels, pp2s_scene,  # noqa: F401
                   project_view)
