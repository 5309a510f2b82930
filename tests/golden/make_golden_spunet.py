"""tests/golden/make_golden_spunet.py -- the SpUNet-v1m1 fixture, produced by CONSTRUCTING the reference's model on the CPU:

    spunet_manifest.json   keys and shapes of SpUNetBase(6, 13) ("num_classes_13") and SpUNetBase(6, 0) ("num_classes_0")

The reference's pointcept/models/sparse_unet/spconv_unet_v1m1_base.py is imported by path under stub packages: `spconv.pytorch`
declares modules with spconv 2.x's parameter shapes (a weight is (Cout, k, k, k, Cin), KRSC) and nothing else -- spconv has no
build for this platform, so the model is constructed, never run --, `torch_geometric.utils.scatter` and
`timm.models.layers.trunc_normal_` are torch's, `pointcept.models.builder.MODELS` a registry that only records.  Nothing of the
reference is copied: only names and shapes are written.

usage:  python tests/golden/make_golden_spunet.py <reference root>     writes the file
        python tests/golden/make_golden_spunet.py --seeds              prints the first seeds whose float64 ReLU pre-activations
                                                                        keep spunet_cases.MARGIN (the model batch, the two blocks)
"""
import importlib.util
import json
import os
import sys
import types

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import spunet_cases as SC  # noqa: E402
from tests import spunet_ref as R  # noqa: E402


def _stub_spconv():
    mod = types.ModuleType("spconv.pytorch")

    class SparseModule(nn.Module):
        pass

    class _Conv(SparseModule):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
            super().__init__()
            k = kernel_size
            self.weight = nn.Parameter(torch.zeros(out_channels, k, k, k, in_channels))  # KRSC
            if bias:
                self.bias = nn.Parameter(torch.zeros(out_channels))
            else:
                self.register_parameter("bias", None)

    class SubMConv3d(_Conv):
        pass

    class SparseConv3d(_Conv):
        pass

    class SparseInverseConv3d(_Conv):
        def __init__(self, in_channels, out_channels, kernel_size, bias=True, indice_key=None):
            super().__init__(in_channels, out_channels, kernel_size, bias=bias, indice_key=indice_key)

    class SparseSequential(nn.Sequential, SparseModule):
        pass

    class Identity(nn.Identity):
        pass

    for cls in (SparseModule, SubMConv3d, SparseConv3d, SparseInverseConv3d, SparseSequential, Identity):
        setattr(mod, cls.__name__, cls)
    mod.SparseConvTensor = object
    top = types.ModuleType("spconv")
    top.pytorch = mod
    sys.modules["spconv"], sys.modules["spconv.pytorch"] = top, mod


def load_reference(ref):
    models = {}

    class Registry:
        def register_module(self, name=None, **_):
            def deco(cls):
                models[name or cls.__name__] = cls
                return cls
            return deco

    _stub_spconv()
    for name, attrs in (("torch_geometric", {}), ("torch_geometric.utils", {"scatter": None}), ("timm", {}), ("timm.models", {}),
                        ("timm.models.layers", {"trunc_normal_": nn.init.trunc_normal_})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    folder = os.path.join(ref, "pointcept", "models", "sparse_unet")
    for name, path in (("pointcept", None), ("pointcept.models", None), ("pointcept.models.sparse_unet", folder)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path] if path else []
        sys.modules[name] = pkg
    builder = types.ModuleType("pointcept.models.builder")
    builder.MODELS = Registry()
    sys.modules["pointcept.models.builder"] = builder
    utils = types.ModuleType("pointcept.models.utils")
    utils.offset2batch = None
    sys.modules["pointcept.models.utils"] = utils
    name = "pointcept.models.sparse_unet.spconv_unet_v1m1_base"
    spec = importlib.util.spec_from_file_location(name, os.path.join(folder, "spconv_unet_v1m1_base.py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return models


def model_margin(seed):
    """the smallest float64 |ReLU pre-activation| of one training forward of the model batch with the state of `seed`"""
    batch = {k: torch.from_numpy(v) for k, v in SC.model_batch(seed).items()}
    model = R.SpUNet()
    model.load_state_dict(SC.fill_state(SC.shapes_of(model), seed), strict=True)
    model = model.double().train()
    R.Margin.reset()
    model(dict(batch, feat=batch["feat"].double()))
    return R.Margin.value


def block_margin(form, seed):
    coord, offset, x, _ = SC.block_inputs(form, seed)
    cin, cout = SC.BLOCK_WIDTHS[form]
    block = R.Block(cin, cout)
    block.load_state_dict(SC.fill_state(SC.shapes_of(block), 300 + seed), strict=True)
    block = block.double().train()
    tables = R.tables_to(R.build_tables(coord, offset), "cpu")
    R.Margin.reset()
    block(torch.from_numpy(x).double(), tables, 0)
    return R.Margin.value


def find_seeds():
    for name, fn in (("model", model_margin), ("block same", lambda s: block_margin("same", s)),
                     ("block proj", lambda s: block_margin("proj", s))):
        for seed in range(1000):
            margin = fn(seed)
            if margin > SC.MARGIN:
                break
        print(name, "seed", seed, "margin %.3e" % margin)


def main():
    if sys.argv[1:] == ["--seeds"]:
        return find_seeds()
    # the seeds the tests use keep every ReLU pre-activation clear of its kink in float64
    assert model_margin(SC.MODEL_SEED) > SC.MARGIN, "spunet_cases.MODEL_SEED: run --seeds"
    for form, seed in SC.BLOCK_SEEDS.items():
        assert block_margin(form, seed) > SC.MARGIN, "spunet_cases.BLOCK_SEEDS[%r]: run --seeds" % form
    models = load_reference(sys.argv[1])
    cls = models["SpUNet-v1m1"]
    manifest = {"num_classes_%d" % c: {k: list(v.shape) for k, v in cls(6, c).state_dict().items()} for c in (13, 0)}
    path = os.path.join(HERE, "spunet_manifest.json")
    with open(path, "w") as f:  # compact, one key per line
        text = [" %s: {\n%s\n }" % (json.dumps(name), ",\n".join(
            "  %s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in keys.items()))
            for name, keys in manifest.items()]
        f.write("{\n%s\n}\n" % ",\n".join(text))
    print("spunet_manifest.json", os.path.getsize(path), "bytes,", [len(v) for v in manifest.values()], "keys")


if __name__ == "__main__":
    main()
