"""GPU: SPVCNN(6, 13, layers=(1,) * 8) of ao_amd.spvcnn on the two clouds of tests/spvcnn_cases.py: model_batch (1206 points in a
48^3 box, with repeated rows): logits in eval(), loss and every parameter gradient in train() with dropout off, against the
float64 restatement of the reference's forward (tests/spvcnn_ref.py: model) under the rule of tests/test_gpu_spvcnn_ops.py.  One
map build and one table build per forward.  The eager switch AO_AMD_SPVCNN=torch runs the same test in a child process."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import spvcnn_cases as SC
from tests import spvcnn_ref as R
from tests.test_gpu_spvcnn_ops import check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# M: 2 x the worst e_kernel / max(e_eager, 2^-24) over both paths, as a power of two; "g_param" is
# shared by the 113 parameter gradients
M = {"logits": 4, "loss": 2, "g_param": 8}


def test_model_against_float64():
    from ao_amd.spunet import tables
    from ao_amd.spvcnn import SPVCNN, pvmap

    torch.manual_seed(3)
    model = SPVCNN(6, 13, layers=(1,) * 8).cuda()
    model.dropout.p = 0
    with torch.no_grad():   # BatchNorm affine terms away from (1, 0)
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(std=0.2)
    coord, offset, feat, label = (torch.from_numpy(a).cuda() for a in SC.model_batch())
    data = dict(discrete_coord=coord, offset=offset, feat=feat)
    names = [k for k, _ in model.named_parameters()]
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    builds = (tables.BUILDS, pvmap.BUILDS)
    res = {"logits": model.eval()(data).detach()}
    assert (tables.BUILDS, pvmap.BUILDS) == (builds[0] + 1, builds[1] + 1)
    loss = F.cross_entropy(model.train()(data), label)
    assert (tables.BUILDS, pvmap.BUILDS) == (builds[0] + 2, builds[1] + 2)
    res["loss"] = loss.detach()
    res.update(zip(["g_" + k for k in names], torch.autograd.grad(loss, [p for _, p in model.named_parameters()])))

    geo, runs = R.Geometry(coord.cpu().numpy(), offset.cpu().numpy(), device="cuda"), []
    for dtype in (torch.float64, torch.float32):
        P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()}
        for k in names:
            P[k].requires_grad_(True)
        with torch.no_grad():
            run = {"logits": R.model(P, geo, feat.to(dtype), False)}
        loss = F.cross_entropy(R.model(P, geo, feat.to(dtype), True), label)
        run["loss"] = loss.detach()
        run.update(zip(["g_" + k for k in names], torch.autograd.grad(loss, [P[k] for k in names])))
        runs.append(run)
    f64, f32 = runs
    assert set(res) == set(f64) == {"logits", "loss"} | {"g_" + k for k in names} and len(names) == 113
    check("model", res, f64, f32, set(res), lambda key: M.get(key, M["g_param"]))


def test_model_with_the_eager_switch():
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_model_against_float64",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=dict(os.environ, AO_AMD_SPVCNN="torch"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-500:]


def test_the_registry_builds_it():
    import types

    from ao_amd.ptv2 import registry
    from ao_amd.spvcnn import SPVCNN

    models = {}
    registry.register(MODELS=types.SimpleNamespace(register_module=lambda module, name, force=True: models.update({name: module})))
    assert models["SPVCNN"] is SPVCNN
