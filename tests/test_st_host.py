"""Host (no GPU): what of Stratified Transformer can be checked without a device: the state-dict manifest against the one the
reference produced, the registry names, tests/st_ref.py's pair lists against the fixtures', and the two ways the reference
computes the sizes of a sampled level."""
import json
import os

import numpy as np
import pytest
import torch

from tests import st_cases as SC
from tests import st_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_manifest_matches_key_for_key():
    from ao_amd.stratified import StratifiedTransformer

    with open(os.path.join(GOLDEN, "st_manifest.json")) as f:
        manifest = json.load(f)
    for name, kwargs in (("default", dict(in_channels=6, num_classes=20)), ("small", SC.MODEL_CONFIG)):
        ours = {k: list(v.shape) for k, v in StratifiedTransformer(**kwargs).state_dict().items()}
        assert list(ours) == list(manifest[name]), name
        assert ours == manifest[name], name


def test_registry_names_resolve():
    import ao_amd.ptv2.registry as registry
    from ao_amd.stratified import StratifiedTransformer

    class Registry(dict):
        def register_module(self, module=None, name=None, force=False):
            self[name] = module

    models = Registry()
    registry.register(MODELS=models)
    assert models["ST-v1m2"] is StratifiedTransformer and models["STv1m2"] is StratifiedTransformer


def test_kernel_points_are_the_reference_restatement():
    from ao_amd.stratified import kernel_points

    for influence in (0.02, 0.2):
        ours = kernel_points(influence)
        assert ours.shape == (15, 3) and torch.equal(ours, R.kernel_points(influence))
        radius = ours.norm(dim=1)
        assert radius[0] == 0 and torch.allclose(radius[1:], torch.full((14,), influence), rtol=1e-6)   # 2/3 of 1.5 x influence


def _reference_new_offsets(offset, ratio):
    """BasicLayer.forward :340-347 and TransitionDown.forward :449-455, the statements as they stand"""
    new_offset = [int(offset[0].item() * ratio) + 1]
    count = int(offset[0].item() * ratio) + 1
    for i in range(1, offset.shape[0]):
        count += int((offset[i].item() - offset[i - 1].item()) * ratio) + 1
        new_offset.append(count)
    truncated = torch.IntTensor(new_offset)
    new_offset, count = [int(offset[0].item() * ratio) + 1], int(offset[0].item() * ratio) + 1
    for i in range(1, offset.shape[0]):
        count += ((offset[i].item() - offset[i - 1].item()) * ratio) + 1
        new_offset.append(count)
    return truncated.tolist(), torch.IntTensor(new_offset).tolist()


@pytest.mark.parametrize("sizes", [(150, 90), (120, 70, 102), (10, 10, 10), (7, 9, 13, 6, 11), (31, 18, 27), (5,)])
def test_new_offset_quirk(sizes):
    from ao_amd.stratified.model import new_offset_accumulated, new_offset_truncated

    offset = torch.tensor(np.cumsum(sizes), dtype=torch.int32)
    for ratio in (0.25, 0.3):
        want_truncated, want_accumulated = _reference_new_offsets(offset, ratio)
        assert new_offset_truncated(offset, ratio) == want_truncated
        assert new_offset_accumulated(offset, ratio) == want_accumulated


def test_the_three_cloud_batch_covers_the_quirk():
    from ao_amd.stratified.model import new_offset_accumulated, new_offset_truncated

    offset = torch.tensor(np.cumsum(SC.MODEL_CLOUDS["st3"]), dtype=torch.int32)
    assert new_offset_truncated(offset, 0.25) == [31, 49, 75] and new_offset_accumulated(offset, 0.25) == [31, 49, 76]


@pytest.mark.parametrize("name", list(SC.MODEL_CLOUDS))
def test_st_ref_pair_lists_equal_the_fixtures(name):
    """the first BasicLayer's two blocks: its points come from the stem's TransitionDown (farthest point sampling by the oracle)"""
    from oracle import pointops_ref as P
    from ao_amd.stratified.model import new_offset_accumulated, new_offset_truncated

    z = np.load(os.path.join(GOLDEN, "st_model_%s.npz" % name))
    batch = SC.model_batch(name)
    coord, offset = torch.from_numpy(batch["coord"]), torch.from_numpy(batch["offset"])
    ratio = 0.25
    level = torch.tensor(new_offset_accumulated(offset, ratio), dtype=torch.int32)
    coords = coord[P.farthest_point_sampling(coord, offset, level).long()]
    sampled = torch.tensor(new_offset_truncated(level, ratio), dtype=torch.int32)
    down_idx = P.farthest_point_sampling(coords, level, sampled)
    for block, shifted in ((0, False), (1, True)):
        i0, i1 = R.pair_lists(coords, level, down_idx, SC.MODEL_CONFIG["window_size"][0], shifted)
        want = z["pairs/%d" % block].astype(np.int64)
        want = want[np.lexsort((want[:, 1], want[:, 0]))]
        assert np.array_equal(torch.stack([i0, i1], 1).numpy(), want), (name, block)


def test_unprovided_pointops2_names_raise():
    from ao_amd.pointops2 import pointops as P2

    for name in ("attention_step1", "attention_step2", "attention_step2_v2", "dot_prod_with_idx", "dot_prod_with_idx_v2",
                 "attention_step2_with_rel_pos_value"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(P2, name)()
    import importlib.util

    spec = importlib.util.spec_from_file_location("dropin_pointops2", os.path.join(os.path.dirname(GOLDEN), "..", "dropin", "pointops2",
                                                                                  "__init__.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    for name in ("attention_step1_v2", "dot_prod_with_idx_v3", "attention_step2_with_rel_pos_value_v2"):
        assert callable(getattr(dropin.pointops, name))
