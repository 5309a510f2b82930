"""GPU: Point Transformer V1's vector-attention layer (ao_amd/csrc/ptv1.hip through ao_amd.ptv1.vector_attention) against
tests/ptv1_ref.py in float64 on the device, on both paths (HIP and AO_AMD_PTV1=torch).

Every output is compared, and the compared key set is asserted: out, the statistics the three norms used, their nine
buffers after the call, g x_q / g x_k / g x_v and the gradient of each of the 14 parameters of linear_p and linear_w.

The bound follows tests/test_gpu_gva_f64.py: e_kernel <= M[output] * e_eager, e_eager the fp32 run of tests/ptv1_ref.py's own
distance from float64 on the same inputs and device, in relative L2 for everything and in the largest element error over the
largest reference element for the forward outputs.  e_eager is floored at 2^-24: no fp32 result can be asked to lie closer to
float64 than half a unit in the last place.  The biases in front of a BatchNorm or the softmax (linear_p.0.bias,
linear_w.2.bias, linear_w.5.bias) have true gradient zero and are bounded by M x the eager run's absolute noise.
num_batches_tracked is compared exactly.  M per output: twice the worst ratio measured on the MI355X over all cases, rounded up
to a power of two (DESIGN.md section 10 holds the table).

The inputs of the training cases keep every ReLU pre-activation behind a norm at least ptv1_cases.MARGIN from its kink in
float64 (asserted): nearer, rounding decides the mask and the gradient is not a continuous function of the inputs."""
import pytest
import torch

from tests import ptv1_cases as PC
from tests import ptv1_ref as R

pytestmark = pytest.mark.gpu

PARAM_KEYS = tuple("linear_%s.%d.%s" % (seq, at, leaf) for seq, ats in (("p", (0, 1, 3)), ("w", (0, 2, 3, 5))) for at in ats
                   for leaf in ("weight", "bias"))
BUFFER_KEYS = tuple("linear_%s.%d.%s" % (seq, at, leaf) for seq, at in (("p", 1), ("w", 0), ("w", 3))
                    for leaf in ("running_mean", "running_var", "num_batches_tracked"))
FWD_KEYS = ("out",) + R.STAT_KEYS
ZERO_GRADS = ("g:linear_p.0.bias", "g:linear_w.2.bias", "g:linear_w.5.bias")
TRAIN_KEYS = set(FWD_KEYS) | set(BUFFER_KEYS) | {"g_xq", "g_xk", "g_xv"} | {"g:" + k for k in PARAM_KEYS}
EVAL_KEYS = set(FWD_KEYS) | set(BUFFER_KEYS)

# M per output: 2 x the worst e_kernel / e_eager over every case and both paths, as a power of two
M = {"out": 8, "mean3": 2, "var3": 2, "meanc": 8, "varc": 4, "meani": 4, "vari": 4, "running_mean": 8, "running_var": 4,
     "g_xq": 4, "g_xk": 4, "g_xv": 4, "g:linear_p.0.weight": 2, "g:linear_p.0.bias": 8, "g:linear_p.1.weight": 16,
     "g:linear_p.1.bias": 4, "g:linear_p.3.weight": 4, "g:linear_p.3.bias": 4, "g:linear_w.0.weight": 4,
     "g:linear_w.0.bias": 4, "g:linear_w.2.weight": 4, "g:linear_w.2.bias": 32, "g:linear_w.3.weight": 4,
     "g:linear_w.3.bias": 4, "g:linear_w.5.weight": 4, "g:linear_w.5.bias": 4}
FLOOR = 2.0 ** -24

_CACHE = {}


def _inputs(case):
    return {k: torch.from_numpy(v).cuda() for k, v in PC.layer_inputs(case).items()}


def _collect(module, out, stats, grads):
    res = {"out": out.detach()}
    res.update({k: stats[k].detach() for k in R.STAT_KEYS})
    state = module.state_dict()
    res.update({k: state["" + k].detach().clone() for k in BUFFER_KEYS})
    if grads is not None:
        res.update(zip(("g_xq", "g_xk", "g_xv") + tuple("g:" + k for k in PARAM_KEYS), (g.detach() for g in grads)))
    return res


def _params(module):
    named = dict(module.named_parameters())
    return [named[k] for k in PARAM_KEYS]


def run_ref(case, dtype, training):
    t = _inputs(case)
    layer = R.Layer(case.c, case.ns)
    layer.load_state_dict(PC.layer_state(layer, case))
    layer = layer.to(device="cuda", dtype=dtype).train(training)
    x = [t[k].to(dtype).requires_grad_(training) for k in ("x_q", "x_k", "x_v")]
    out = layer.attention(*x, t["coord"].to(dtype), t["idx"])
    grads = torch.autograd.grad(out, x + _params(layer), t["g_out"].to(dtype)) if training else None
    return _collect(layer, out, layer.stats(), grads), layer.margin()


def run_op(case, training):
    from ao_amd import ptv1

    t = _inputs(case)
    layer = ptv1.PointTransformerLayer(case.c, case.c, 8, case.ns)
    layer.load_state_dict(PC.layer_state(layer, case))
    layer = layer.cuda().train(training)
    x = [t[k].clone().requires_grad_(training) for k in ("x_q", "x_k", "x_v")]
    stats = {}
    out = ptv1.vector_attention(*x, t["coord"], t["idx"], layer.linear_p, layer.linear_w, stats)
    grads = torch.autograd.grad(out, x + _params(layer), t["g_out"]) if training else None
    return _collect(layer, out, stats, grads)


def reference(case, training):
    key = (case.name, training)
    if key not in _CACHE:
        _CACHE.clear()
        (f64, margin), (f32, _) = run_ref(case, torch.float64, training), run_ref(case, torch.float32, training)
        _CACHE[key] = (f64, f32, margin)
    return _CACHE[key]


def _l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def _peak(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def check(res, f64, f32, keys):
    assert set(res) == keys and set(f64) == keys and set(f32) == keys
    bad = []
    for key in sorted(keys):
        if key.endswith("num_batches_tracked"):
            assert int(res[key]) == int(f64[key]), key
            continue
        m = M[key.rsplit(".", 1)[1] if key.endswith(("running_mean", "running_var")) else key]
        assert torch.isfinite(res[key]).all(), key
        if key in ZERO_GRADS:
            got, allowed = float(res[key].double().norm()), m * max(float(f32[key].double().norm()), 1e-30)
            kinds = [("abs", got, allowed)]
        else:
            kinds = [("l2", _l2(res[key], f64[key]), m * max(_l2(f32[key], f64[key]), FLOOR))]
            if key in FWD_KEYS:
                kinds.append(("peak", _peak(res[key], f64[key]), m * max(_peak(f32[key], f64[key]), FLOOR)))
        for kind, got, allowed in kinds:
            print("ptv1-ratio %-24s %-4s kernel %.3e  allowed %.3e  ratio-to-eager %.3f" % (key, kind, got, allowed, got / (allowed / m)))
            if not got <= allowed:
                bad.append((key, kind, got, allowed))
    assert not bad, bad


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("name", [c.name for c in PC.LAYER_CASES])
def test_layer_training_against_float64(name, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_PTV1", path)
    case = PC.case(name)
    f64, f32, margin = reference(case, True)
    assert margin > PC.MARGIN, "the case's inputs put a ReLU pre-activation %.2e from its kink" % margin
    print("ptv1-case", name, path, "train")
    check(run_op(case, True), f64, f32, TRAIN_KEYS)


@pytest.mark.parametrize("path", ["hip", "torch"])
@pytest.mark.parametrize("name", PC.EVAL_CASES)
def test_layer_eval_against_float64(name, path, monkeypatch):
    monkeypatch.setenv("AO_AMD_PTV1", path)
    case = PC.case(name)
    f64, f32, _ = reference(case, False)
    print("ptv1-case", name, path, "eval")
    check(run_op(case, False), f64, f32, EVAL_KEYS)


def test_two_hip_runs_give_the_same_bits(monkeypatch):
    monkeypatch.setenv("AO_AMD_PTV1", "hip")
    case = PC.case("many")
    a, b = run_op(case, True), run_op(case, True)
    assert set(a) == TRAIN_KEYS
    for key in a:
        assert torch.equal(a[key], b[key]), key
