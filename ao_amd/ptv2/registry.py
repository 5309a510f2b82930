"""Registration of this package's classes under the reference's registries, with the reference's own idiom.

The reference builds its model, segmentor and optimizer from config dicts through `Registry` objects
(pointcept/utils/registry.py:59-): `MODELS` (pointcept/models/builder.py), `OPTIMIZERS` (pointcept/utils/optimizer.py:12-17,
`build_optimizer` ends in `OPTIMIZERS.build(cfg=cfg)`, :55).  `register(MODELS=..., OPTIMIZERS=...)` is what the one file a
maintainer adds calls:

    from pointcept.models.builder import MODELS
    from pointcept.utils.optimizer import OPTIMIZERS
    import ao_amd.ptv2.registry as mi355x
    mi355x.register(MODELS=MODELS, OPTIMIZERS=OPTIMIZERS)

after which `model = dict(type="DefaultSegmentor", backbone=dict(type="PT-v2m2", ...))` resolves to the MI355X classes and
`optimizer = dict(type="FlatAdamW", lr=0.006, weight_decay=0.05)` is a CONFIG edit (the reference's line is
`dict(type="AdamW", lr=0.006, weight_decay=0.05)`, configs/s3dis/semseg-pt-v2m2-0-base.py:42): no trainer code changes.
`FlatAdamW.step()` takes the `.grad`s autograd (or DistributedDataParallel) delivered; when they alias the native backward's
flat gradient buffer (the default delivery of ao_amd/ptv2/native_model.py) no copy is made.
"""


def _register(registry, cls, name, force):
    """`registry.register_module(module=cls, name=name)` -- pointcept/utils/optimizer.py:15-17 -- tolerant of a name that is
    already taken when `force` (the reference's Registry takes force=True to replace an entry, registry.py `_register_module`)."""
    try:
        registry.register_module(module=cls, name=name, force=force)
    except TypeError:  # a registry without the force keyword
        registry.register_module(module=cls, name=name)


def register(MODELS=None, OPTIMIZERS=None, force=True, LOSSES=None, TEST=None, HOOKS=None):
    """Put PT-v2m2, the three segmentors (CAC-v1m1 included) and FlatAdamW under the reference's registry names, and with LOSSES
    (pointcept/models/losses/builder.py) the HIP LovaszLoss under "LovaszLoss": a trainer that keeps the reference's own
    segmentor and `Criteria` then builds it from the same config entry; with TEST (pointcept/engines/test.py:26) the whole-scene
    tester of ao_amd/ptv2/tester.py under "SemSegTester", which `test = dict(type="SemSegTester")` then resolves to.  Every
    registry may be omitted.  MODELS also receives
    CACSegmentor under "CAC-v1m1", PointTransformerV2M1 under "PT-v2m1" and Point Transformer V1 under "PointTransformer-Seg26" / "-Seg38" / "-Seg50", SpUNetBase under "SpUNet-v1m1", PointGroup under "PG-v1m1", MaskedSceneContrast
    under "MSC-v1m1", MaskedSceneContrastCSC under "MSC-v1m2" and StratifiedTransformer under "ST-v1m2" and "STv1m2"; the returned
    list of names leaves those entries out (it predates them).  With HOOKS (pointcept/engines/hooks/builder.py) the instance
    evaluator of ao_amd/pointgroup/evaluate.py is filed under "InsSegEvaluator", likewise not listed."""
    done = []
    if MODELS is not None:
        from .model import PointTransformerV2
        from .cac import CACSegmentor
        from .segmentor import DefaultSegmentor, DefaultSegmentorSAM_Image

        for cls, name in ((PointTransformerV2, "PT-v2m2"), (DefaultSegmentor, "DefaultSegmentor"),
                          (DefaultSegmentorSAM_Image, "DefaultSegmentorSAM_Image")):
            _register(MODELS, cls, name, force)
            done.append(name)
        # (filed under MODELS as well, but not listed in the return value: callers compare that list with the names above)
        _register(MODELS, CACSegmentor, "CAC-v1m1", force)
        # PT-v2m1 (GroupedLinear + position multiplier), likewise filed and not listed
        from .model import PointTransformerV2M1

        _register(MODELS, PointTransformerV2M1, "PT-v2m1", force)
        # Point Transformer V1 (ao_amd/ptv1), likewise filed and not listed
        from ..ptv1 import PointTransformerSeg26, PointTransformerSeg38, PointTransformerSeg50

        for cls, name in ((PointTransformerSeg26, "PointTransformer-Seg26"), (PointTransformerSeg38, "PointTransformer-Seg38"),
                          (PointTransformerSeg50, "PointTransformer-Seg50")):
            _register(MODELS, cls, name, force)
        # SpUNet-v1m1 (ao_amd/spunet), likewise filed and not listed
        from ..spunet import SpUNetBase

        _register(MODELS, SpUNetBase, "SpUNet-v1m1", force)
        # PointGroup (ao_amd/pointgroup), likewise filed and not listed
        from ..pointgroup import PointGroup

        _register(MODELS, PointGroup, "PG-v1m1", force)
        # Masked Scene Contrast (ao_amd/msc), likewise filed and not listed
        from ..msc import MaskedSceneContrast, MaskedSceneContrastCSC

        _register(MODELS, MaskedSceneContrast, "MSC-v1m1", force)
        _register(MODELS, MaskedSceneContrastCSC, "MSC-v1m2", force)
        # Stratified Transformer (ao_amd/stratified) under both spellings the reference's configs use, likewise
        from ..stratified import StratifiedTransformer

        _register(MODELS, StratifiedTransformer, "ST-v1m2", force)
        _register(MODELS, StratifiedTransformer, "STv1m2", force)
    if OPTIMIZERS is not None:
        from .optim import FlatAdamW

        _register(OPTIMIZERS, FlatAdamW, "FlatAdamW", force)
        done.append("FlatAdamW")
    if LOSSES is not None:
        from .losses import LovaszLoss

        _register(LOSSES, LovaszLoss, "LovaszLoss", force)
        done.append("LovaszLoss")
    if TEST is not None:
        from .tester import SemSegTester

        _register(TEST, SemSegTester, "SemSegTester", force)
        done.append("SemSegTester")
    if HOOKS is not None:
        from ..pointgroup.evaluate import InsSegEvaluator

        _register(HOOKS, InsSegEvaluator, "InsSegEvaluator", force)
    return done
