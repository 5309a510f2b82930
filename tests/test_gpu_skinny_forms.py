"""GPU: the two forms of the G-wide projection kernels (ao_amd/csrc/skinny.hip) give the same bits.

The default forms stage their operands in LDS (skinny_fwd_tile_kernel: tiles of R rows; skinny_bn_bwd_reduce_staged_kernel: W and the
sg rows of a trip, where W's image leaves four workgroups per CU); AO_AMD_SKINNY=lanes (read on every call) selects the lane forms everywhere.  Both keep the same fmaf
chain per output, so everything is compared with torch.equal: the public forward launchers on NaN-filled outputs (an unwritten
tail row shows), and a native Block's forward + backward -- every output, every parameter gradient, the running statistics."""
import copy
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_rows(cin):
    """R of skinny_fwd_tile_kernel (skinny_tile_rows in skinny.hip): four float4 per lane of a 256-lane workgroup."""
    return 4 * 256 // (cin // 4)


def _forward_cases():
    out = []
    for cin, cout in ((48, 6), (96, 12), (192, 24), (384, 48), (512, 64)):
        r = tile_rows(cin)
        out += [(n, cin, cout) for n in (1, r - 1, r + 1, 5 * r + 3)]
    return out + [(4501, 192, 24)]


def _set_form(monkeypatch, form):
    if form == "lanes":
        monkeypatch.setenv("AO_AMD_SKINNY", "lanes")
    else:
        monkeypatch.delenv("AO_AMD_SKINNY", raising=False)


@pytest.mark.parametrize("n,cin,cout", _forward_cases())
def test_forward_launchers_give_the_same_bits_in_both_forms(monkeypatch, n, cin, cout):
    from ao_amd import _lib

    L = _lib.lib()
    torch.manual_seed(n + cin)
    x = torch.randn(n, cin, device="cuda")
    w = torch.randn(cout, cin, device="cuda") / cin ** 0.5
    sc = torch.rand(cin, device="cuda") + 0.5
    sh = torch.randn(cin, device="cuda") * 0.3
    got = {}
    for form in ("default", "lanes"):
        _set_form(monkeypatch, form)
        ys = [torch.full((n, cout), float("nan"), device="cuda") for _ in range(3)]
        s = _lib.stream_ptr()
        _lib.check(L.skinny_linear_forward_hip_launcher(n, cin, cout, x.data_ptr(), w.data_ptr(), ys[0].data_ptr(), s), "skinny forward")
        _lib.check(L.skinny_linear_forward_xf_hip_launcher(n, cin, cout, x.data_ptr(), w.data_ptr(), 0, 0, ys[1].data_ptr(), s),
                   "skinny forward xf, no transform")
        _lib.check(L.skinny_linear_forward_xf_hip_launcher(n, cin, cout, x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                                           ys[2].data_ptr(), s), "skinny forward xf")
        got[form] = ys
    for a, b in zip(got["default"], got["lanes"]):
        assert not bool(torch.isnan(b).any()) and torch.equal(a, b)  # (the values themselves: tests/test_gpu_dense_f64.py)


def _block_step(c, g, n, k=16):
    """{form: [output, input gradient, parameter gradients ..., buffers ...]} of one training-mode native Block forward +
    backward under each setting of AO_AMD_SKINNY (the caller's process environment is changed and restored)."""
    from ao_amd import pointops, synth
    from ao_amd.ptv2 import block as native
    from tests.test_gpu_block import _block_pair

    coord = torch.from_numpy(synth.room_cloud(max(n, 64), seed=n + c)[:n]).cuda()
    offset = torch.tensor([n], dtype=torch.int32, device="cuda")
    idx, _ = pointops.knn_query(k, coord, offset)
    torch.manual_seed(7)
    x0 = torch.randn(n, c, device="cuda").relu_()
    go = torch.randn(n, c, device="cuda")
    blk0, _ = _block_pair(c, g, 0.0, seed=3)
    keep = {v: os.environ.get(v) for v in ("AO_AMD_SKINNY", "AO_AMD_BLOCK")}
    res = {}
    try:
        os.environ["AO_AMD_BLOCK"] = "native"
        for form in ("default", "lanes"):
            if form == "lanes":
                os.environ["AO_AMD_SKINNY"] = "lanes"
            else:
                os.environ.pop("AO_AMD_SKINNY", None)
            blk = copy.deepcopy(blk0).train()
            x = x0.clone().requires_grad_(True)
            if n < 2:  # one row has no batch statistics: the native runtime declines it and BatchNorm1d refuses it, in both forms
                assert not native.supported(blk, x, idx)
                with pytest.raises(ValueError, match="more than 1 value per channel"):
                    blk([coord, x, offset], idx)
                res[form] = []
                continue
            assert native.supported(blk, x, idx)
            y = blk([coord, x, offset], idx)[1]
            grads = torch.autograd.grad(y, [x] + list(blk.parameters()), go)
            res[form] = ([("y", y.detach()), ("grad x", grads[0])]
                         + [("grad " + nm, t) for (nm, _), t in zip(blk.named_parameters(), grads[1:])]
                         + [(nm, b.clone()) for nm, b in blk.named_buffers()])
    finally:
        for v, old in keep.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old
    return res


def _assert_same_bits(res, n=2):
    assert len(res["default"]) == len(res["lanes"]) > (10 if n >= 2 else -1)
    for (nm, a), (_, b) in zip(res["default"], res["lanes"]):
        assert torch.equal(a, b), (nm, float((a.double() - b.double()).abs().max()))


# n = 1: a training-mode Block of one point does not exist (no batch statistics) -- the case checks that both forms refuse it
# alike, and n = 2, the smallest Block there is, stands in for it.
# (11 000, 48, 6): K.nblk of the fused backward + reduce reaches its cap of 256 records and a lane visits more than one row
@pytest.mark.parametrize("c,g,n", [(c, g, n) for c, g in ((48, 6), (96, 12), (192, 24), (384, 48)) for n in (1, 2, 65, 1074)]
                         + [(48, 6, 11000)])
def test_native_block_gives_the_same_bits_in_both_forms(c, g, n):
    _assert_same_bits(_block_step(c, g, n), n)


def _child():
    res = _block_step(96, 12, 1074)
    _assert_same_bits(res)
    print("same bits: %d tensors" % len(res["default"]))


def test_unfused_backward_pair_gives_the_same_bits_in_both_forms():
    """AO_AMD_SKINNY_BN=0 is read once per process: a fresh child runs the Block with the q / k BatchNorm reduce as a launch of
    its own (skinny_bwd_kernel has one form; the forward still has two)."""
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_skinny_forms import _child; _child()"], cwd=ROOT,
                       env=dict(os.environ, AO_AMD_SKINNY_BN="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "same bits:" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
