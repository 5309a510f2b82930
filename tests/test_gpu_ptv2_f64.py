"""GPU: the native PT-v2m2 Block runtime (ao_amd/csrc/block.hip, gva_block.hip) and the native model runtime
(ao_amd/csrc/model.hip), and the staged python paths beside them, against the float64 run of tests/ptv2_ref64.py on the device.

The bound is the M-rule in its absolute form: |ours - f64| <= M[kind] * max(|eager fp32 - f64|, 2^-24 |f64|) in L2, for `out` and
`logits` also in the largest element; the eager float32 run is the same reference in float32 on the same inputs and tables, on
the host (ptv2_ref64.eager_host: torch's float32 training-mode BatchNorm on the device is 2 to 1000 times further from float64).
num_batches_tracked is compared exactly; two identical native calls give the same bits.  A gradient that is exactly zero in exact
arithmetic (ptv2_ref64.zero_keys) must vanish in float64 and is held to M["zero"] * max(|eager fp32|, 2^-24 |f64 gradient of the
layer's weight|).  M per class of output: twice the worst ratio measured on the MI355X over all cases and paths, rounded up to a
power of two, at least 1 and at most ptv2_ref64.M_CAP.

The cases (tests/ptv2_f64_cases.py) carry seeds under which no ReLU pre-activation and no pooling gap of the float64 run lies
within ptv2_ref64.RATIO times the float32 run's deviation; asserted again here, on the device's float64 run and tables.  The model cases have
exactly one Block (the runtime refuses a network without any); every other sequence has depth 0."""
import pytest
import torch
import torch.nn.functional as F

from tests import ptv2_f64_cases as C
from tests import ptv2_ref64 as R

pytestmark = pytest.mark.gpu

# M per class of output
M = {"out": 4, "logits": 4, "loss": 2, "g_x": 4, "grad": 8, "buffer": 4, "zero": 8}
assert all(1 <= v <= R.M_CAP for v in M.values())
_REF = {}


def _check(got, f64, f32, zeros, tag, keys=None):
    bad = R.compare(M, got, f64, f32, zeros, tag, keys=keys)
    assert not bad, bad


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ----------------------------------------------------------------------------------------------------------- the block ----
def _block_ref(name, mode):
    key = ("block", name, mode)
    if key not in _REF:
        from ao_amd import pointops

        case = C.BLOCK_CASES[name]
        coord, offset = (torch.from_numpy(a).cuda() for a in C.block_cloud(name))
        idx, _ = pointops.knn_query(case.k, coord, offset)
        f64, f32, margin, inp = C.block_reference(name, mode, C.BLOCK_SEEDS[name, mode], coord, idx)
        _REF[key] = dict(coord=coord, offset=offset, idx=idx, f64=f64, f32=f32, margin=margin, inp=inp)
    return _REF[key]


def _block_ours(name, mode, path, ref, go=None):
    from ao_amd.ptv2 import block as native
    from ao_amd.ptv2.model import Block

    case, inp = C.BLOCK_CASES[name], ref["inp"]
    blk = Block(case.c, case.g, qkv_bias=case.qkv_bias).cuda()
    blk.load_state_dict(inp["state"], strict=True)
    blk.train(mode == "train")
    x = inp["x"].clone().requires_grad_(True)
    if path == "native":
        assert native.supported(blk, x, ref["idx"])
    y = blk([ref["coord"], x, ref["offset"]], ref["idx"], inp["keep"])[1]
    named = list(blk.named_parameters())
    grads = torch.autograd.grad(y, [x] + [p for _, p in named], inp["go"] if go is None else go)
    res = {"out": y.detach(), "g_x": grads[0]}
    res.update({"g:" + k: g for (k, _), g in zip(named, grads[1:])})
    res.update({"b:" + k: v.detach().clone() for k, v in blk.named_buffers()})
    return res


@pytest.mark.parametrize("path", ["native", "python"])
@pytest.mark.parametrize("name,mode", [(n, m) for n, c in C.BLOCK_CASES.items() for m in c.modes])
def test_block_against_float64(name, mode, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_BLOCK", path)
    ref = _block_ref(name, mode)
    small, eps = ref["margin"]
    assert small >= R.RATIO * eps, "the seed puts a pre-activation %.2e from its kink, the float32 run deviates by %.2e" % (small, eps)
    got = _block_ours(name, mode, path, ref)
    masked = bool((ref["idx"] < 0).any())
    assert masked == (name == "short_clouds")
    zeros = R.zero_keys([k[2:] for k in got if k.startswith("g:")], mode == "train", masked)
    assert set(got) == set(ref["f64"]) == set(ref["f32"])
    if path == "native":
        _same_bits(got, _block_ours(name, mode, path, ref))
    _check(got, ref["f64"], ref["f32"], zeros, "block/%s/%s/%s" % (name, mode, path))
    keep = ref["inp"]["keep"]
    if keep is not None:
        # the rows that drew 0 return the identity bit for bit, and their branch gradient is 0: a gradient that arrives at
        # those rows alone reaches no parameter and passes through the identity's ReLU unchanged
        x, dropped = ref["inp"]["x"], keep == 0
        assert 0.3 < float(dropped.float().mean()) < 0.7
        assert torch.equal(got["out"][dropped], x[dropped])
        go = ref["inp"]["go"] * dropped.float().unsqueeze(1)
        only = _block_ours(name, mode, path, ref, go=go)
        assert torch.equal(only["g_x"], go * (x > 0).float())
        for k, v in only.items():
            if k.startswith("g:"):
                assert not bool(v.any()), k


# ----------------------------------------------------------------------------------------------------------- the model ----
def _levels(cfg, geo):
    ns = len(cfg["enc_depths"])
    ks = [{cfg["patch_embed_neighbours"], cfg["dec_neighbours"][0]}]
    for i in range(ns):
        ks.append({cfg["enc_neighbours"][i]} | ({cfg["dec_neighbours"][i + 1]} if i + 1 < ns else set()))
    return [dict(coord=lv.coord, knn={k: lv.neighbours(k) for k in ks[i]}, cluster=lv.cluster, order=lv.order32, idx_ptr=lv.idx_ptr32,
                 up_idx=lv.up_idx, up_weight=lv.up_weight) for i, lv in enumerate(geo.levels)]


def _model_ref(name, case, cfg, seed, grads=True):
    key = ("model", name)
    if key not in _REF:
        import ao_amd.ptv2 as ptv2

        coord, offset = (torch.from_numpy(a).cuda() for a in C.model_cloud(case.clouds))
        geo = ptv2.PointTransformerV2(**cfg).geometry(coord, offset)  # test_geometry_matches_oracle pins these tables
        levels = _levels(cfg, geo)
        f64, f32, margin, inp = C.model_reference(cfg, case.training, seed, coord, levels, grads=grads)
        _REF[key] = dict(coord=coord, offset=offset, geo=geo, levels=levels, f64=f64, f32=f32, margin=margin, inp=inp)
    return _REF[key]


def _model_ours(case, cfg, path, ref, pipelined=False, grads=True):
    import ao_amd.ptv2 as ptv2
    from ao_amd.ptv2 import native_model

    inp = ref["inp"]
    model = ptv2.PointTransformerV2(**cfg).cuda()
    model.load_state_dict(inp["state"], strict=True)
    model.train(case.training)
    data = dict(coord=ref["coord"], feat=inp["feat"], offset=ref["offset"])
    assert native_model.supported(model, inp["feat"]) == (path == "native")
    if path == "native":  # the native path really runs: the one Block is supported, and so is every level
        assert native_model.geometry_supported(ref["geo"]) and (native_model.pipelined_ok(model) or not pipelined)
        assert native_model.runtime(model).M.num_blocks == 1
    with torch.set_grad_enabled(grads):
        logits = model(data) if pipelined else model(data, geometry=ref["geo"])
        loss = F.cross_entropy(logits, inp["segment"], ignore_index=-1)
    res = {"logits": logits.detach(), "loss": loss.detach()}
    if grads:
        named = list(model.named_parameters())
        res.update({"g:" + k: g for (k, _), g in zip(named, torch.autograd.grad(loss, [p for _, p in named]))})
    res.update({"b:" + k: v.detach().clone() for k, v in model.named_buffers()})
    return res


MODEL_RUNS = [(name, "native", False) for name in C.MODEL_CASES] + [("seq0", "native", True), ("seq1", "python", False),
                                                                    ("map", "python", False)]


@pytest.mark.parametrize("name,path,pipelined", MODEL_RUNS, ids=["%s-%s%s" % (n, p, "-pipelined" if q else "") for n, p, q in MODEL_RUNS])
def test_model_against_float64(name, path, pipelined, monkeypatch):
    """pipelined: the default call, which builds the geometry itself behind the level-0 prefix (two forward graphs); needs
    the Block in sequence 0.  Otherwise the geometry is handed in."""
    monkeypatch.setenv("AO_AMD_MODEL", path)
    case, cfg = C.MODEL_CASES[name], C.model_cfg(name)
    ref = _model_ref(name, case, cfg, C.MODEL_SEEDS[name])
    small, eps = ref["margin"]
    assert small >= R.RATIO * eps, "the seed puts a pre-activation or a pooling gap %.2e from its kink, the float32 run deviates by %.2e" % (small, eps)
    assert [lv["coord"].shape[0] for lv in ref["levels"]] == ([110, 40, 9] if name == "seq0" else [170, 61, 10])
    got = _model_ours(case, cfg, path, ref, pipelined)
    assert set(got) == set(ref["f64"]) == set(ref["f32"])
    level = [0, 1, 2, 0, 1][case.seq]
    masked = bool((ref["levels"][level]["knn"][16] < 0).any())
    zeros = R.zero_keys([k[2:] for k in got if k.startswith("g:")], case.training, masked)
    if path == "native":
        _same_bits(got, _model_ours(case, cfg, path, ref, pipelined))
    _check(got, ref["f64"], ref["f32"], zeros, "model/%s/%s%s" % (name, path, "/pipelined" if pipelined else ""))


def test_model_forward_above_32768_points_against_float64():
    """n0 = 32 801: at more than 512 records of 64 rows linbn_forward leaves the GEMM-epilogue statistics for rows_gemm +
    bn_forward.  Forward only, logits and buffers: a flipped mask moves a forward value continuously, so no margin is needed."""
    case = C.BIG_CASE
    cfg = C.skeleton(case.seq, **case.over)
    ref = _model_ref("big", case, cfg, 0, grads=False)
    assert ref["coord"].shape[0] == 32801 > 512 * 64
    got = _model_ours(case, cfg, "native", ref, grads=False)
    keys = sorted(k for k in ref["f64"] if k == "logits" or k.startswith("b:"))
    assert len(keys) == 1 + len(list(k for k in got if k.startswith("b:")))
    _check(got, ref["f64"], ref["f32"], {}, "model/big/native", keys=keys)
