"""CPU: PT-v2m1 above the kernels -- the host logic of ao_amd/ptv2/gva.py with the multiplier logits stage, the model class,
the registry name, the twelfth header and the case list of the GPU tests.

1. grouped_vector_attention(..., impl=TorchImplM1) on a float64 PT-v2m1 attention module equals the literal op sequence
   (GroupedVectorAttention.gva_unfused, its pointops.grouping answered by the oracle's plain-torch one) in float64 to 1e-10
   relative L2, the bound of tests/test_gva_ref64_host.py: output, input gradient, every parameter gradient, the running
   statistics of both position BatchNorms; train and eval.
2. PointTransformerV2M1 has the reference's state-dict keys and shapes for the three reference configs
   (tests/golden/ptv2m1_manifest.json), loads the fixture's seeded state strictly, prints, and is filed as "PT-v2m1".
3. include/ptv2_v2m1_hip.h parses through ao_amd/_abi.py; its symbols are in the built library with the declared arity, and
   refuse a shape outside the contract with a status before anything is enqueued.
4. Every case of tests/ptv2m1_cases.py meets its own exactness assertions.
Every test here fails on the parent commit: the name, the class and the symbols do not exist there."""
import copy
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import pointops_ref as P
from tests import ptv2m1_cases as C
from tests import synth
from tests.ptv2m1_ref import TorchImplM1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _attention(c, g, seed):
    from ao_amd.ptv2.model import GroupedVectorAttention, use_grouped_linear

    mod = use_grouped_linear(GroupedVectorAttention(c, g, pe_multiplier=True, pe_bias=True))
    mod.load_state_dict(C.init_state({k: v.shape for k, v in mod.state_dict().items()}, seed), strict=True)
    return mod


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("c,g,k", [(48, 6, 16), (96, 12, 8)])
def test_host_logic_in_float64_equals_the_literal_sequence(monkeypatch, mode, c, g, k):
    from ao_amd.ptv2 import gva
    from ao_amd.ptv2 import model as model_py

    n = 700
    xyz = torch.from_numpy(synth.room_cloud(n, seed=3))
    off = torch.tensor([300, n], dtype=torch.int32)
    idx, _ = P.knn_query(k, xyz, off)
    idx = idx.clone()
    idx[3::11, k - 3:] = -1
    xyz = xyz.double()
    gen = torch.Generator().manual_seed(9)
    feat0 = torch.randn(n, c, dtype=torch.float64, generator=gen)
    gout = torch.randn(n, c, dtype=torch.float64, generator=gen)

    lit = _attention(c, g, seed=5).double().train(mode == "train")
    mod = copy.deepcopy(lit)
    monkeypatch.setattr(model_py, "pointops", types.SimpleNamespace(grouping=P.grouping))
    f1 = feat0.clone().requires_grad_(True)
    ref = lit.gva_unfused(lit.linear_q(f1), lit.linear_k(f1), lit.linear_v(f1), xyz, idx)
    assert ref.dtype == torch.float64
    names = [name for name, _ in lit.named_parameters()]
    rgrads = torch.autograd.grad(ref, [f1] + list(lit.parameters()), gout)

    f2 = feat0.clone().requires_grad_(True)
    out = gva.grouped_vector_attention(mod, mod.linear_q(f2), mod.linear_k(f2), mod.linear_v(f2), xyz, idx, impl=TorchImplM1)
    assert out.dtype == torch.float64
    assert _rel(out.detach(), ref.detach()) < 1e-10, _rel(out.detach(), ref.detach())
    grads = torch.autograd.grad(out, [f2] + list(mod.parameters()), gout)
    assert "weight_encoding.0.weight" in names and "linear_p_multiplier.3.weight" in names
    scale = max(float(r.abs().max()) for r in rgrads)
    for name, gr, rg in zip(["feat"] + names, grads, rgrads):
        assert gr.dtype == torch.float64
        if float(rg.abs().max()) < 1e-9 * scale:  # a bias in front of a training-mode BatchNorm: the true gradient is 0
            assert float(gr.abs().max()) < 1e-9 * scale, (name, float(gr.abs().max()))
            continue
        assert _rel(gr, rg) < 1e-10, (name, _rel(gr, rg))
    sd, rsd = mod.state_dict(), lit.state_dict()
    stats = [key for key in rsd if key.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert sum(key.startswith(("linear_p_multiplier.1", "linear_p_bias.1")) for key in stats) == 6
    for key in stats:
        if key.endswith("num_batches_tracked"):
            assert int(sd[key]) == int(rsd[key]) == (1 if mode == "train" else 0), key
        else:
            assert _rel(sd[key], rsd[key]) < 1e-10, key


def test_grouped_linear_is_the_references_layer():
    from ao_amd.ptv2 import GroupedLinear

    lin = GroupedLinear(48, 6, 6)
    assert {k: tuple(v.shape) for k, v in lin.state_dict().items()} == {"weight": (1, 48)}
    x = torch.randn(5, 7, 48)
    want = (x * lin.weight).reshape(5, 7, 6, 8).sum(-1)
    assert torch.equal(lin(x), want)
    assert "bias" not in repr(lin) and "groups=6" in repr(lin)
    with pytest.raises(AssertionError):
        GroupedLinear(50, 6, 6)  # 50 & 6 == 2 passes neither check; 48 % 6 == 0 and 48 & 6 == 0 pass both


def _manifest():
    with open(os.path.join(GOLDEN, "ptv2m1_manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("tag", ["s3dis", "scannet", "scannet200"])
def test_state_dict_layout_equals_the_references(tag):
    from ao_amd.ptv2 import PointTransformerV2M1

    man = _manifest()
    model = PointTransformerV2M1(**man[tag + "_cfg"])
    have = {k: list(v.shape) for k, v in model.state_dict().items()}
    want = man[tag] if tag in man else dict(man["scannet"], **man[tag + "_except"])  # (scannet200: what differs from scannet)
    assert have == want
    assert sum(p.numel() for p in model.parameters()) == man[tag + "_num_params"]


def test_fixture_state_loads_strictly_and_the_model_prints():
    from ao_amd.ptv2 import GroupedLinear, PointTransformerV2M1

    model = PointTransformerV2M1(**C.MODEL_CFG)
    st = C.init_state({k: v.shape for k, v in model.state_dict().items()}, C.MODEL_SEED)
    with np.load(os.path.join(GOLDEN, "ptv2m1.npz")) as g:
        assert C.state_digest(st) == str(g["model_digest"])
    model.load_state_dict(st, strict=True)
    text = repr(model)
    assert "GroupedLinear(in_features=48, out_features=6, groups=6)" in text
    assert sum(isinstance(m, GroupedLinear) for m in model.modules()) == 3


def test_registry_files_the_name():
    import ao_amd.ptv2.registry as registry
    from ao_amd.ptv2 import PointTransformerV2M1

    class Registry:
        def __init__(self):
            self.table = {}

        def register_module(self, module=None, name=None, force=False):
            self.table[name] = module

    models = Registry()
    done = registry.register(MODELS=models)
    assert models.table["PT-v2m1"] is PointTransformerV2M1
    assert "PT-v2m1" not in done and "PT-v2m2" in done
    from ao_amd.ptv2.model import build_from_cfg

    assert isinstance(build_from_cfg(dict(C.MODEL_CFG, type="PT-v2m1")), PointTransformerV2M1)


NAMES = ("gva_mul_workspace_bytes", "gva_mul_logits_forward_hip_launcher", "gva_mul_logits_backward_hip_launcher")


def test_header_parses_and_the_symbols_have_the_declared_arity():
    from ao_amd import _abi, _lib

    assert set(NAMES) <= set(_abi.v2m1_signatures)
    txt = re.sub(r"/\*.*?\*/", "", open(_abi.V2M1_HEADER).read(), flags=re.S)
    L = _lib.lib()
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, txt, flags=re.S)
        assert m, name
        declared = len([a for a in m.group(1).split(",") if a.strip()])
        fn = getattr(L, name)
        assert len(fn.argtypes) == declared == len(_abi.v2m1_signatures[name][1]), name
    assert L.ptv2_v2m1_abi_version() == _lib.EXPECTED_V2M1_ABI


def test_launchers_refuse_shapes_outside_the_contract():
    from ao_amd import _lib

    L = _lib.lib()
    assert L.gva_mul_workspace_bytes(100, 16, 48, 6) > 0
    for n, k, c, g in ((100, 16, 50, 6), (100, 16, 48, 8), (100, 12, 48, 6), (100, 128, 48, 6), (100, 1, 48, 6), (0, 16, 48, 6),
                       (2 ** 27, 16, 48, 6)):
        assert L.gva_mul_workspace_bytes(n, k, c, g) == 0, (n, k, c, g)
        p = 4096  # (never dereferenced: the status comes before anything is enqueued)
        rc = L.gva_mul_logits_forward_hip_launcher(n, k, c, g, *([p] * 19), 1 << 30, 0)
        assert rc == 1, (n, k, c, g, rc)
        rc = L.gva_mul_logits_backward_hip_launcher(n, k, c, g, *([p] * 30), 1 << 30, 0)
        assert rc == 1, (n, k, c, g, rc)


def test_shape_predicate_follows_the_contract():
    from ao_amd.ptv2 import gva

    for c, g in C.SHAPES:
        want = (c, g) not in gva.MUL_LITERAL_SHAPES
        assert gva.mul_supported(c, g, 1000, 16) == want and gva.mul_supported(c, g, 1, 2) == want
        assert not gva.mul_supported(c, g, 1000, 12) and not gva.mul_supported(c, g, 1000, 128)
    assert not gva.mul_supported(64, 8, 1000, 16)


def _cpu_knn(k, coord, offset):
    return P.knn_query(k, coord, offset)[0]


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_every_gpu_case_has_exact_preactivations(case):
    t = C.build_inputs(case, _cpu_knn)
    counts = C.check_inputs(case, t)
    assert counts["zeros_pos"] >= case.n and counts["zeros_pos_m"] >= case.n  # an exact zero at each kink in every row


def test_the_case_list_covers_the_shapes_and_edges():
    std = [x for x in C.CASES if x.kind == "std"]
    assert {(x.c, x.g) for x in std if x.k == 16} == set(C.SHAPES)
    assert {x.k for x in std if (x.c, x.g) == (48, 6)} == {2, 4, 8, 16, 32, 64}
    for (c, g), edge in C.ROUND_EDGES.items():
        ns = {x.n for x in std if (x.c, x.g, x.k) == (c, g, 16)}
        assert {1, 5, 1074} | set(edge) <= ns
    assert sum(x.kind == "hub" for x in C.CASES) == 1
    assert len({x.name for x in C.CASES}) == len(C.CASES)
