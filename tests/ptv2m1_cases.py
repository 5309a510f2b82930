"""Cases and inputs of the multiplier logits stage of PT-v2m1 (ao_amd/csrc/gva_mul.hip), on which no ReLU mask can flip.

Test infrastructure.  The inputs are those of tests/gva_ref64.py::build_inputs (coordinates in multiples of 2^-7, a in
multiples of 2^-5, b of 2^-6, exact zeros planted, -1 slots from the 9- and 21-point clouds, the hub) with the operands the
multiplier adds: a_m / b_m on the same grids as a / b (b_m[2::5] = 0 meets the self slot's pos = 0 in every row: an exact zero at
the kink of Pm), and generic random key, query, w, Wm2, bm2.  check_inputs() holds both pre-activations, pos a^T + b and
pos a_m^T + b_m, to tests/gva_ref64.py::check_inputs: bit-equal in fp32 and float64, every mask bit equal.

The case list names the edges of the kernels (rows = n k slots, tiles of 16 slots, one wavefront per tile):
  k = 16: a point is a tile.  k = 8: two points per tile, an odd n leaves half a tile.  k = 2, 4: 8 / 4 points per tile (the
  segment sums of g_query).  k = 32, 64: a point is 2 / 4 tiles of one wavefront (g_query accumulated across them).
  n = 1, 5, 17: a cloud shorter than k in every row; fewer tiles than wavefronts of a workgroup.
  rows pass of the backward, grid cap x wavefronts = tiles of one round: (48,6), (96,12): 1024 x 4 -> n = 4096 | 4097;
  (192,24): 441 x 4 -> 1764 | 1765; (384,48): 112 x 2 -> 224 | 225; (512,64): 63 x 1 -> 63 | 64.
  forward and key pass, 2048 workgroups x 4 (C <= 192) or x 2 wavefronts: n = 8192 | 8193 at (48,6), 4096 | 4097 at (384,48).
  n = 1074 (a benchmark level size): several workgroups everywhere, more than one round at (384,48) and (512,64), the
  cross-workgroup sum of the g_Wm2 records; Wm2 is streamed in 24 / 32 chunks of 16 columns at C = 384 / 512 at every n.
  hub: slot 1 of every row of the first cloud names ONE point, whose inverse list is as long as that cloud."""
import torch

from tests import gva_ref64 as R

SHAPES = ((48, 6), (96, 12), (192, 24), (384, 48), (512, 64))
ROUND_EDGES = {(48, 6): (4096, 4097), (96, 12): (4096, 4097), (192, 24): (1764, 1765), (384, 48): (224, 225), (512, 64): (63, 64)}


def _cases():
    out = []

    def add(n, c, g, k=16, kind="std"):
        out.append(R.Case("%s-n%d-c%d-g%d-k%d" % (kind, n, c, g, k), n, c, g, k, kind))

    for c, g in SHAPES:
        for n in (1, 5, 17) + ROUND_EDGES[(c, g)] + (1074,):
            add(n, c, g)
    add(8192, 48, 6)
    add(8193, 48, 6)
    add(4096, 384, 48)
    add(4097, 384, 48)
    for n in (5, 17, 1000):
        add(n, 48, 6, k=8)
    for k in (2, 4, 32, 64):
        add(37, 48, 6, k=k)
        add(100, 48, 6, k=k)
    add(1074, 192, 24, kind="hub")
    return out


CASES = _cases()


def build_inputs(case, knn, device="cpu"):
    """fp32 inputs of the stage for `case` on `device`: those of gva_ref64.build_inputs plus the multiplier's operands"""
    t = R.build_inputs(case, knn, device)
    n, c = case.n, case.c
    gen = torch.Generator().manual_seed(77 + n + 3 * c + case.k)
    r = lambda *s: torch.randn(*s, generator=gen)
    m = dict(key=r(n, c), query=r(n, c), w=r(c) / 8 ** 0.5,
             a_m=R._dyadic(2.0 * r(c, 3), 2.0 ** -5, -8.0, 8.0), b_m=R._dyadic(0.25 * r(c), 2.0 ** -6),
             Wm2=r(c, c) / c ** 0.5, bm2=1.0 + 0.1 * r(c))
    m["b_m"][2::5] = 0.0
    t.update({key: val.to(device).contiguous() for key, val in m.items()})
    return t


def check_inputs(case, t):
    """Both ReLU pre-activations of the stage meet gva_ref64.check_inputs; returns its counts for pos a^T + b and, under
    "zeros_pos_m", the exact zeros of pos a_m^T + b_m."""
    counts = R.check_inputs(case, t)
    counts_m = R.check_inputs(case, dict(t, a=t["a_m"], b=t["b_m"]))
    counts["zeros_pos_m"] = counts_m["zeros_pos"]
    assert t["key"].shape == t["query"].shape == (case.n, case.c) and t["Wm2"].shape == (case.c, case.c)
    return counts


# ---- the model and module fixtures (tests/golden/make_golden_ptv2m1.py writes them, tests/test_gpu_ptv2m1_model.py reads them)
# widths cut down to one encoder / decoder stage; pe_multiplier = True as in the three reference configs; drop_path 0
MODEL_CFG = dict(in_channels=6, num_classes=13, patch_embed_depth=1, patch_embed_channels=48, patch_embed_groups=6,
                 patch_embed_neighbours=8, enc_depths=(1,), enc_channels=(96,), enc_groups=(12,), enc_neighbours=(16,),
                 dec_depths=(1,), dec_channels=(48,), dec_groups=(6,), dec_neighbours=(16,), grid_sizes=(0.25,),
                 attn_qkv_bias=True, pe_multiplier=True, pe_bias=True, attn_drop_rate=0.0, drop_path_rate=0.0,
                 enable_checkpoint=False, unpool_backend="map")
MODEL_SEED, MODEL_POINTS = 41, (240, 360)
MODULE_POINTS = (15, 9)     # two clouds shorter than k = 16: -1 slots in every row
MODULE_SEED = 43


def init_state(shapes, seed):
    """A state dict for {key: shape} drawn from one seeded CPU generator in sorted key order (the fixture files hold no
    weights: both sides build them with this function and compare digests).  BatchNorm affine and running statistics are
    away from their defaults."""
    gen = torch.Generator().manual_seed(seed)
    st = {}
    for key in sorted(shapes):
        shape = tuple(shapes[key])
        if key.endswith("num_batches_tracked"):
            st[key] = torch.zeros(shape, dtype=torch.long)
        elif key.endswith("running_mean"):
            st[key] = 0.2 * torch.randn(shape, generator=gen)
        elif key.endswith("running_var"):
            st[key] = 0.5 + torch.rand(shape, generator=gen)
        elif key.endswith("norm.weight"):
            st[key] = 1.0 + 0.2 * torch.randn(shape, generator=gen)
        elif key.endswith(".bias"):
            st[key] = 0.1 * torch.randn(shape, generator=gen)
        else:
            fan_in = 8 if (len(shape) == 2 and shape[0] == 1) else shape[-1]  # (GroupedLinear: 8 channels per output)
            st[key] = torch.randn(shape, generator=gen) / fan_in ** 0.5
    return st


def state_digest(state):
    import hashlib

    h = hashlib.sha256()
    for key in sorted(state):
        h.update(key.encode())
        h.update(state[key].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def module_inputs(c, k=16):
    """(coord (n,3), offset, feat (n,c), gout (n,c)) of the attention-module case of width c; the neighbour table comes from
    the caller's kNN"""
    import numpy as np

    from tests import synth

    n = sum(MODULE_POINTS)
    pts = np.concatenate([synth.room_cloud(64, seed=MODULE_SEED + i)[:m] for i, m in enumerate(MODULE_POINTS)])
    gen = torch.Generator().manual_seed(MODULE_SEED + c)
    return (torch.from_numpy(pts), torch.tensor(np.cumsum(MODULE_POINTS), dtype=torch.int32), torch.randn(n, c, generator=gen),
            torch.randn(n, c, generator=gen))


def model_inputs():
    """(coord, offset, feat, label) of the small-model case"""
    import numpy as np

    from tests import synth

    n = sum(MODEL_POINTS)
    coord = torch.from_numpy(np.concatenate([synth.room_cloud(m, seed=MODEL_SEED + 100 * i) for i, m in enumerate(MODEL_POINTS)]))
    offset = torch.tensor(np.cumsum(MODEL_POINTS), dtype=torch.int32)
    gen = torch.Generator().manual_seed(MODEL_SEED)
    feat = torch.cat([coord, torch.rand(n, 3, generator=gen) * 2 - 1], 1).contiguous()
    label = torch.randint(0, MODEL_CFG["num_classes"], (n,), generator=gen)
    label[torch.rand(n, generator=gen) < 0.1] = -1
    return coord, offset, feat, label
