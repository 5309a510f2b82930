"""CPU: what the float64 comparisons of tests/test_gpu_gva_f64.py rest on.

1. The reference.  tests/gva_torch_ref.py::TorchImpl behind the host logic of ao_amd/ptv2/gva.py on a float64 module equals the
   oracle's literal GroupedVectorAttention (oracle/ptv2_ref.py::_gva) in float64, forward and every gradient, train and eval,
   to 1e-10 relative L2: both sides are float64 torch on one machine and differ by re-association only (about 1e-15 per
   operation, sums of at most n k = 11 200 terms).
2. The inputs.  Every case of the GPU case list is built here (CPU kNN) and held to the properties of
   tests/gva_ref64.py::check_inputs: pre-activations bit-equal in fp32 and float64, exact zeros at both kinks, -1 slots."""
import pytest
import torch

from oracle import pointops_ref as P
from oracle import ptv2_ref as M
from tests import gva_ref64 as R
from tests import synth
from tests.gva_torch_ref import TorchImpl


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("c,g,k", [(48, 6, 16), (96, 12, 8)])
def test_torch_statement_in_float64_equals_the_oracle(mode, c, g, k):
    from ao_amd.ptv2 import gva
    from ao_amd.ptv2.model import GroupedVectorAttention

    torch.manual_seed(0)
    n = 700
    xyz = torch.from_numpy(synth.room_cloud(n, seed=3))
    off = torch.tensor([300, n], dtype=torch.int32)
    idx, _ = P.knn_query(k, xyz, off)
    idx = idx.clone()
    idx[3::11, k - 3:] = -1
    xyz = xyz.double()
    cfg = dict(M.S3DIS_CFG, patch_embed_depth=1, patch_embed_channels=c, patch_embed_groups=g, enc_depths=(),
               enc_channels=(), enc_groups=(), enc_neighbours=(), dec_depths=(), dec_channels=(), dec_groups=(),
               dec_neighbours=(), grid_sizes=(), num_classes=0)
    st = M.init_state(cfg, seed=5)
    pre = "patch_embed.blocks.blocks.0.attn."
    ast = {k_[len(pre):]: (v.double() if v.is_floating_point() else v) for k_, v in st.items() if k_.startswith(pre)}
    feat0 = torch.randn(n, c, dtype=torch.float64)
    gout = torch.randn(n, c, dtype=torch.float64)

    ost = {"a." + k_: (v.clone().requires_grad_(True) if M.is_param(k_) else v.clone()) for k_, v in ast.items()}
    cx = M.Ctx(ost, mode == "train", update_stats=True)
    f1 = feat0.clone().requires_grad_(True)
    ref = M._gva(cx, "a", f1, xyz, idx, g)
    assert ref.dtype == torch.float64
    names = [k_ for k_ in ost if M.is_param(k_[2:])]
    rgrads = torch.autograd.grad(ref, [f1] + [ost[k_] for k_ in names], gout)

    mod = GroupedVectorAttention(c, g).double()
    mod.load_state_dict(ast, strict=True)
    mod.train(mode == "train")
    f2 = feat0.clone().requires_grad_(True)
    q, kk, v = mod.linear_q(f2), mod.linear_k(f2), mod.linear_v(f2)
    out = gva.grouped_vector_attention(mod, q, kk, v, xyz, idx, impl=TorchImpl)
    assert out.dtype == torch.float64
    assert _rel(out.detach(), ref.detach()) < 1e-10, _rel(out.detach(), ref.detach())
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad(out, [f2] + [params[k_[2:]] for k_ in names], gout)
    scale = max(float(r.abs().max()) for r in rgrads)
    for k_, gr, rg in zip(["feat"] + names, grads, rgrads):
        assert gr.dtype == torch.float64
        if float(rg.abs().max()) < 1e-9 * scale:  # a bias in front of a training-mode BatchNorm: the true gradient is 0
            assert float(gr.abs().max()) < 1e-9 * scale, (k_, float(gr.abs().max()))
            continue
        assert _rel(gr, rg) < 1e-10, (k_, _rel(gr, rg))
    if mode == "train":
        sd = mod.state_dict()
        for k_ in ast:
            if k_.endswith(("running_mean", "running_var")):
                assert _rel(sd[k_], ost["a." + k_]) < 1e-10, k_


def _cpu_knn(k, coord, offset):
    return P.knn_query(k, coord, offset)[0]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_every_gpu_case_has_exact_preactivations(case):
    t = R.build_inputs(case, _cpu_knn)
    counts = R.check_inputs(case, t)
    assert counts["zeros_pos"] >= case.n  # b[::5] = 0 meets the self slot's pos = 0 in every row
    if case.kind == "spread":
        z = torch.relu(t["W1"].double() * t["sc"].double() + t["sh"].double()) @ t["Ww2"].double().t()
        assert 59.0 < float(z.abs().max()) < 61.0


def test_the_case_list_covers_the_instances_and_edges():
    shapes = {(c.c, c.g, c.k) for c in R.CASES if c.kind == "std"}
    assert shapes == {(48, 6, 16), (48, 6, 8), (96, 12, 16), (192, 24, 16), (384, 48, 16), (512, 64, 16)}
    for c, g in ((96, 12), (192, 24)):
        ns = {x.n for x in R.CASES if (x.c, x.g, x.kind) == (c, g, "std")}
        assert {1, 5, 17, 127, 128, 129, 4096, 4097, 4501, 6144, 6152, 6500} <= ns
    ns = {x.n for x in R.CASES if (x.c, x.g, x.kind) == (384, 48, "std")}
    assert {1024, 1025, 1074, 127, 128, 129, 1, 5, 17} <= ns
    assert {x.n for x in R.CASES if x.kind == "std"} >= {18905, 4501, 1074}
    assert {(x.c, x.g) for x in R.CASES if x.kind == "spread"} == {(48, 6), (96, 12), (192, 24), (384, 48), (512, 64)}
    assert sum(x.kind == "hub" for x in R.CASES) == 1
    assert len({x.name for x in R.CASES}) == len(R.CASES)


def test_reference_statement_has_every_key_and_fp32_is_close():
    """statement() returns the full key list in both precisions, the fp32 eager statement is within rounding of float64 on
    these inputs (no flipped mask: otherwise gradients would differ by whole terms), and the true-zero gradient is zero."""
    case = next(c for c in R.CASES if c.name == "std-n1074-c96-g12-k16")
    t = R.build_inputs(case, _cpu_knn)
    ref, eager = R.statement(t, torch.float64), R.statement(t, torch.float32)
    assert set(ref) == set(eager) == set(R.ALL_KEYS)
    for key in R.ALL_KEYS:
        assert ref[key].dtype == torch.float64
        if key in R.ZERO_KEYS:
            assert float(ref[key].abs().max()) < 1e-12 and float(eager[key].abs().max()) < 1e-3
            continue
        assert R.errors(eager[key], ref[key])[0] < 2e-6, (key, R.errors(eager[key], ref[key]))
