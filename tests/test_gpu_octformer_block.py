"""GPU: one OctFormerBlock(96, 6, 26, dilation) of ao_amd.octformer in training mode on 245 nodes of two clouds: forward, input
gradient and every parameter gradient against the float64 restatement of OctFormerBlock.forward (tests/octformer_ref.py: block),
under the rule of tests/test_gpu_octformer_ops.py.  The eager switch AO_AMD_OCTFORMER=torch runs the same test in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octformer_cases as OC
from tests import octformer_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLOOR = 2.0 ** -24
# M: 2 x the worst e_kernel / max(e_eager, 2^-24) over both dilations and both paths, as a power of two;
# "g_param" is shared by the parameter gradients
M = {"out": 2, "g_data": 4, "g_param": 4}


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("dilation", [1, 4])
def test_block_against_float64(dilation):
    from ao_amd.octformer import OctFormerBlock, octree_level

    torch.manual_seed(dilation)
    block = OctFormerBlock(96, 6, 26, dilation).cuda().train()
    with torch.no_grad():   # a bias that matters, and BatchNorm / LayerNorm affine terms away from (1, 0)
        block.attention.rpe.rpe_table.normal_(std=0.5)
        for m in (block.cpe.bn, block.norm1, block.norm2):
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(std=0.2)
    xyz, batch = OC.cloud((100, 145), seed=11)
    rng = np.random.default_rng(dilation)
    data, g_out = (torch.from_numpy(rng.standard_normal((245, 96)).astype(np.float32)).cuda() for _ in range(2))
    xyz, batch = torch.from_numpy(xyz).cuda(), torch.from_numpy(batch).cuda()
    level = octree_level(xyz, batch, OC.DEPTH)
    assert torch.equal(level.order, torch.arange(245, device="cuda"))
    names = [k for k, _ in block.named_parameters()]

    def grads(out, leaves):
        return dict(zip(["out", "g_data"] + ["g_" + k for k in names], (out.detach(),) + torch.autograd.grad(out, leaves, g_out.to(out.dtype))))

    x = data.clone().requires_grad_(True)
    res = grads(block(x, level), [x] + [p for _, p in block.named_parameters()])
    runs = []
    for dtype in (torch.float64, torch.float32):
        p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in block.named_parameters()}
        x = data.to(dtype).requires_grad_(True)
        runs.append(grads(R.block(x, p, xyz, batch, 2, level.nbr, 26, dilation, 6), [x] + [p[k] for k in names]))
    f64, f32 = runs
    assert set(res) == set(f64) == set(f32) == {"out", "g_data"} | {"g_" + k for k in names} and len(names) == 16
    bad = []
    for key in sorted(res):
        got, eager, m = _l2(res[key], f64[key]), _l2(f32[key], f64[key]), M.get(key, M["g_param"])
        print("oct-block-ratio D=%d %-32s kernel %.3e  eager %.3e  ratio %.3f" % (dilation, key, got, eager, got / max(eager, FLOOR)))
        if not got <= m * max(eager, FLOOR):
            bad.append((key, got, m * max(eager, FLOOR)))
    assert not bad, bad


def test_block_with_the_eager_switch():
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_block_against_float64",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, AO_AMD_OCTFORMER="torch"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-500:]
