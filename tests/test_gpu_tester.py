"""GPU: whole-scene test-time inference (ao_amd/ptv2/tester.py on ao_amd/csrc/vote.hip, the test-time transforms and
test_fragments of ao_amd/ptv2/transform.py).

Bound of the vote (DESIGN.md section 3.4's rule): `e_kernel <= M * e_eager` per table, in relative L2 and in the largest element
error over the largest reference element.  The reference is tests/tester_cases.votes64 evaluated on the device: float64
softmax of the logits as given, float64 sums.  `e_eager` is the distance of the eager fp32 loop (test.py:107-113, the
AO_AMD_VOTE=torch path) from it.  M = twice the worst ratio measured on the MI355X, rounded up to a power of two; the
measured ratios are in DESIGN.md section 3.8d.

Guard band of the prediction: a point whose float64 top-two vote margin is below BAND_FACTOR * M * (largest element error of
the eager table) is left out of the comparison (two entries may each be off by the bound); at most 0.5 % of a case's points
may be left out, and the synthetic inputs plant a leading class with margin >= 1 (share 0; tests/test_tester_host.py checks
that on the CPU).
"""
import os

import numpy as np
import pytest
import torch

from tests import tester_cases as TC
from tests.gva_ref64 import errors

pytestmark = pytest.mark.gpu

M_VOTE = 2        # the measured worst e_kernel / e_eager is 1.00: twice that, a power of two
BAND_FACTOR = 2
CAP = 0.005
DEV = "cuda"


def _table(n_total, c, sets, logits, eager, monkeypatch, batched=False):
    from ao_amd.ptv2 import VoteTable

    if eager:
        monkeypatch.setenv("AO_AMD_VOTE", "torch")
    else:
        monkeypatch.delenv("AO_AMD_VOTE", raising=False)
    t = VoteTable(n_total, c, DEV)
    if batched:
        ends = torch.tensor([s.numel() for s in sets]).cumsum(0).int()
        t.add(torch.cat(logits), torch.cat(sets), ends.to(DEV), offset_host=ends.tolist())
    else:
        for idx, x in zip(sets, logits):
            t.add(x, idx)
    return t


def _votes64_dev(n_total, c, sets, logits):
    v = torch.zeros(n_total, c, dtype=torch.float64, device=DEV)
    for idx, x in zip(sets, logits):
        v[idx.long()] += torch.softmax(x.double(), -1)
    return v


def _case(c, n, dtype, itype, frags, seed):
    n_total = n + n // 2 + 1
    g = torch.Generator(device=DEV).manual_seed(seed)
    sets, logits = [], []
    for f in range(frags):
        sets.append(torch.randperm(n_total, device=DEV, generator=g)[:n].to(itype))
        x = (torch.rand(n, c, device=DEV, generator=g) * 2 - 1) * 60.0
        x[::3] = x[::3] / 30
        logits.append(x.to(dtype))
    return n_total, sets, logits


def hold(tag, got, eager, ref):
    ek, mk = errors(got, ref)
    ee, me = errors(eager, ref)
    print("vote %s e_kernel %.4e e_eager %.4e ratio %.3f | max %.4e %.4e ratio %.3f | elements that differ from eager %d of %d"
          % (tag, ek, ee, ek / max(ee, 1e-300) if ek else 0.0, mk, me, mk / max(me, 1e-300) if mk else 0.0,
             int((got != eager).sum()), got.numel()))
    assert bool(torch.isfinite(got).all()), tag
    assert ek <= M_VOTE * ee, (tag, "relative L2", ek, ee)
    assert mk <= M_VOTE * me, (tag, "largest element", mk, me)
    return me * float(ref.abs().max())


CS = (2, 13, 20, 32, 33, 64, 200, 256)
NS = (1, 63, 64, 65, 4097, 120000)
FORMS = [(torch.float32, torch.int64, 1), (torch.bfloat16, torch.int32, 12)]
CROSS = [(torch.float32, torch.int32, 12), (torch.bfloat16, torch.int64, 1)]
CASES = [(c, n) + f for c in CS for n in NS for f in FORMS] + [(c, n) + f for c in (13, 200) for n in NS for f in CROSS]


@pytest.mark.parametrize("c,n,dtype,itype,frags", CASES,
                         ids=["c%d-n%d-%s-%s-f%d" % (c, n, str(d)[6:], str(i)[6:], f) for c, n, d, i, f in CASES])
def test_vote_against_float64(c, n, dtype, itype, frags, monkeypatch):
    n_total, sets, logits = _case(c, n, dtype, itype, frags, seed=c * 1000 + n % 997)
    ref = _votes64_dev(n_total, c, sets, logits)
    eager = _table(n_total, c, sets, logits, True, monkeypatch).votes
    hip = _table(n_total, c, sets, logits, False, monkeypatch)
    hold("c%d n%d %s %s f%d" % (c, n, dtype, itype, frags), hip.votes, eager, ref)
    again = _table(n_total, c, sets, logits, False, monkeypatch)
    assert torch.equal(hip.votes, again.votes), "two runs differ"
    if frags > 1:
        batched = _table(n_total, c, sets, logits, False, monkeypatch, batched=True)
        assert torch.equal(hip.votes, batched.votes), "batched add differs from one-by-one add"
    # rows no fragment named stay zero
    seen = torch.zeros(n_total, dtype=torch.bool, device=DEV)
    for s in sets:
        seen[s.long()] = True
    assert float(hip.votes[~seen].abs().sum()) == 0.0


@pytest.mark.parametrize("c", [2, 13, 20, 32, 33, 200, 256])
def test_predict_outside_the_guard_band(c, monkeypatch):
    n_total, frags = 20000, 12
    sets, logits, leader = TC.planted(n_total, c, frags, seed=c)
    sets, logits = [s.to(DEV) for s in sets], [x.to(DEV) for x in logits]
    ref = _votes64_dev(n_total, c, sets, logits)
    eager = _table(n_total, c, sets, logits, True, monkeypatch).votes
    hip = _table(n_total, c, sets, logits, False, monkeypatch)
    band = BAND_FACTOR * M_VOTE * hold("planted c%d" % c, hip.votes, eager, ref)
    keep = TC.margin(ref) >= band
    left_out = 1.0 - float(keep.double().mean())
    print("predict c%d band %.3e left out %.5f" % (c, band, left_out))
    assert left_out <= CAP
    pred = hip.predict()
    assert pred.dtype == torch.int64 and pred.shape == (n_total,)
    assert torch.equal(pred[keep], ref.max(1)[1][keep])
    assert torch.equal(pred, leader.to(DEV))  # (every point was visited and its leader planted)


@pytest.mark.parametrize("c", [2, 13, 32, 33, 200, 256])
def test_argmax_ties_go_to_the_lowest_class(c, monkeypatch):
    from ao_amd.ptv2 import VoteTable

    monkeypatch.delenv("AO_AMD_VOTE", raising=False)
    n = 1000
    t = VoteTable(n, c, DEV)
    g = torch.Generator().manual_seed(c)
    v = torch.rand(n, c, generator=g)
    first = torch.randint(0, c, (n,), generator=g)
    second = torch.randint(0, c, (n,), generator=g)
    v[torch.arange(n), first] = 2.0
    v[torch.arange(n), second] = 2.0   # an exact tie between two classes (or one maximum where they coincide)
    v[:10] = 0.25                      # equal rows: every class ties
    t.votes.copy_(v)
    pred = t.predict().cpu()
    want = torch.minimum(first, second)
    want[:10] = 0
    assert torch.equal(pred, want)


def test_out_of_range_index_is_an_error_and_writes_nothing(monkeypatch):
    from ao_amd import _lib
    from ao_amd.ptv2 import VoteTable

    monkeypatch.delenv("AO_AMD_VOTE", raising=False)
    n_total, c, n = 5000, 13, 3000
    sets = TC.fragments(n_total, n, 2, seed=1)
    x = TC.spread_logits(n, c, seed=2).to(DEV)
    t = VoteTable(n_total, c, DEV)
    t.add(x, sets[0].to(DEV))
    before = t.votes.clone()
    for bad_value in (n_total, -1, 1 << 40):
        bad = sets[1].clone()
        bad[n // 2] = bad_value
        t.add(x, bad.to(DEV))
        rc = _lib.lib().seg_vote_status_hip_launcher(t._status.data_ptr(), _lib.stream_ptr())
        assert rc == 1  # PTV2_ERR_ARG
        assert torch.equal(t.votes, before), "a segment with a bad row wrote to the table"
    bad = sets[1].clone()
    bad[0] = n_total + 5
    t.add(x, bad.to(DEV))
    with pytest.raises(IndexError):
        t.raise_if_invalid()
    assert torch.equal(t.votes, before)
    with pytest.raises(IndexError):
        t.add(x, bad.to(DEV), check=True)
    t.add(x, sets[1].to(DEV))  # the table stays usable once the error has been reported
    t.raise_if_invalid()
    assert not torch.equal(t.votes, before)


def test_check_raises_on_a_planted_duplicate(monkeypatch):
    from ao_amd.ptv2 import VoteTable

    monkeypatch.delenv("AO_AMD_VOTE", raising=False)
    idx = TC.fragments(4000, 1000, 1, seed=3)[0]
    idx[17] = idx[700]
    t = VoteTable(4000, 20, DEV)
    with pytest.raises(ValueError, match="twice"):
        t.add(torch.zeros(1000, 20, device=DEV), idx.to(DEV), check=True)
    assert float(t.votes.abs().sum()) == 0.0


def test_no_host_synchronisation_in_add(monkeypatch):
    from ao_amd.ptv2 import VoteTable

    monkeypatch.delenv("AO_AMD_VOTE", raising=False)
    n_total, c = 50000, 13
    sets = [s.to(DEV) for s in TC.fragments(n_total, 20000, 4, seed=4)]
    x = torch.cat([TC.spread_logits(20000, c, seed=5 + i) for i in range(4)]).to(DEV)
    ends = [20000, 40000, 60000, 80000]
    off = torch.tensor(ends, dtype=torch.int32, device=DEV)
    t = VoteTable(n_total, c, DEV)
    t.add(x, torch.cat(sets), off, offset_host=ends)  # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.add(x, torch.cat(sets), off, offset_host=ends)
        pred = t.predict()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert pred.shape == (n_total,)


# ---- transforms and fragments against the reference's outputs (tests/golden/tester.npz) ------------------------------------------

def test_transforms_against_the_fixture(golden):
    from tests.test_tester_host import check_transforms

    check_transforms(golden("tester.npz"), DEV)


def _check_partition(tag, z, frag, n_aug):
    """the partition of prepare_test_data, not its order: per augmentation, every fragment holds exactly one point of every
    voxel, and a point of a voxel with m points is in fragments j, j + m, ... for one residue j"""
    sizes = z[tag + "_sizes"]
    ref_index = np.split(z[tag + "_index"], np.cumsum(sizes)[:-1])
    per_aug = z[tag + "_per_aug"]
    got = [f["index"].cpu().numpy() for f in frag["fragment_list"]]
    assert len(got) == len(ref_index) == int(per_aug.sum())
    n = int(z[tag + "_coord"].shape[0])
    at = 0
    for a in range(n_aug):
        cnt = int(per_aug[a])
        ref_parts, got_parts = ref_index[at:at + cnt], got[at:at + cnt]
        at += cnt
        # the voxels, from the reference's fragments: fragment 0 names one point per voxel; the points that share a fragment
        # slot pattern with it are found through the reference's own membership table
        vox_of = np.full(n, -1, np.int64)
        nvox = ref_parts[0].shape[0]
        member = np.zeros((n, cnt), bool)
        for j, p in enumerate(ref_parts):
            assert p.shape[0] == nvox
            member[p, j] = True
        # reference fragments list the voxels in the same (sorted key) order: column v of every fragment is voxel v
        for p in ref_parts:
            vox_of[p] = np.arange(nvox)
        assert (vox_of >= 0).all()
        size = np.bincount(vox_of, minlength=nvox)
        gmember = np.zeros((n, cnt), bool)
        for j, p in enumerate(got_parts):
            assert p.shape[0] == nvox, (tag, a, j, p.shape[0], nvox)
            assert np.array_equal(np.sort(vox_of[p]), np.arange(nvox)), "a fragment must hold one point of every voxel"
            gmember[p, j] = True
        m = size[vox_of]
        first = gmember.argmax(1)
        assert (first < m).all()
        want = (np.arange(cnt)[None, :] % m[:, None]) == first[:, None]
        assert np.array_equal(gmember, want), "a point of a voxel with m points is in fragments j, j + m, ..."
        # and the residues of a voxel's points are a permutation of 0 .. m - 1
        order = np.lexsort((first, vox_of))
        start = np.cumsum(size) - size
        assert np.array_equal(first[order], np.arange(n) - start[vox_of[order]])


@pytest.mark.parametrize("tag", ["s3dis", "scannet"])
def test_fragments_against_the_fixture(golden, tag):
    from ao_amd.ptv2 import transform as T

    z = golden("tester.npz")
    data = dict(coord=torch.from_numpy(z[tag + "_coord"]).to(DEV), color=torch.from_numpy(z[tag + "_color"]).to(DEV),
                segment=torch.from_numpy(z[tag + "_segment"]).to(DEV), name=tag)
    if tag == "s3dis":
        cfg, n_aug = TC.s3dis_cfg([0, 7]), 2
    else:
        data["normal"] = torch.from_numpy(z[tag + "_normal"]).to(DEV)
        cfg, n_aug = dict(TC.SCANNET_TEST_CFG, aug_transform=TC.SCANNET_TEST_CFG["aug_transform"][:2]), 2
    frag = T.test_fragments(data, cfg, transform=TC.S3DIS_BASE_TRANSFORM)
    assert frag["name"] == tag and torch.equal(frag["segment"].cpu(), torch.from_numpy(z[tag + "_segment"]))
    _check_partition(tag, z, frag, n_aug)
    f0 = frag["fragment_list"][0]
    assert set(f0) == set(cfg["post_transform"][2]["keys"]) | {"offset", "feat"}
    assert f0["feat"].shape[1] == (6 if tag == "s3dis" else 9) and f0["feat"].dtype == torch.float32
    # a fragment's rows against the reference's augmented cloud: colour (and normal) exactly, coord up to the fragment's own
    # CenterShift(apply_z=False), which depends on which point of a voxel the fragment holds.  The rotation is rounded to
    # fp32 once here and stays float64 until ToTensor in the reference: 1 ulp of a coordinate of a few metres is 5e-7.
    at = 0
    for a in range(n_aug):
        aug_coord = z[tag + "_aug_coord"][a]
        for f in frag["fragment_list"][at:at + int(z[tag + "_per_aug"][a])]:
            idx, feat = f["index"].cpu().numpy(), f["feat"].cpu().numpy()
            assert np.array_equal(feat[:, :3], f["coord"].cpu().numpy())
            assert np.array_equal(feat[:, 3:6], z[tag + "_base_color"][idx])
            src = aug_coord[idx]
            shift = np.array([(src[:, 0].min() + src[:, 0].max()) / 2, (src[:, 1].min() + src[:, 1].max()) / 2, 0], np.float32)
            np.testing.assert_allclose(feat[:, :3], src - shift, rtol=0, atol=2e-6)
            if tag == "scannet":
                np.testing.assert_allclose(feat[:, 6:9], z[tag + "_aug_normal"][a][idx], rtol=0, atol=1e-6)
        at += int(z[tag + "_per_aug"][a])


# ---- end to end --------------------------------------------------------------------------------------------------------------

class _Cfg:
    def __init__(self, save_path, k):
        self.save_path, self.test_epoch, self.dataset_type, self.empty_cache = str(save_path), 7, "S3DISDataset", False
        self.data = type("D", (), dict(num_classes=k, ignore_index=-1, names=["class%d" % i for i in range(k)]))()


class _Loader(list):
    batch_size = 1
    dataset = None


@pytest.fixture(scope="module")
def scene():
    import ao_amd.ptv2 as ptv2
    from ao_amd.ptv2 import transform as T
    from oracle import ptv2_ref

    cfg = dict(ptv2.S3DIS_BACKBONE, drop_path_rate=0.0)
    model = ptv2.DefaultSegmentor(backbone=ptv2.PointTransformerV2(**cfg)).to(DEV)
    model.backbone.load_state_dict(ptv2_ref.init_state(cfg, seed=5), strict=True)
    model.eval()
    room = TC.synthetic_room(30000, seed=11)
    data = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in room.items()}
    frag = T.test_fragments(data, TC.s3dis_cfg([0, 2, 7]), transform=TC.S3DIS_BASE_TRANSFORM)
    return model, frag, int(room["coord"].shape[0])


def _run_tester(model, frag, tmp_path, fragment_batch, autocast=None):
    from ao_amd.ptv2 import SemSegTester

    tester = SemSegTester(fragment_batch=fragment_batch, autocast=autocast)
    result = tester(_Cfg(tmp_path, 13), _Loader([[dict(frag)]]), model)
    pred = np.load(os.path.join(str(tmp_path), "result", "test_epoch7", "room_pred.npy"))
    return result, pred


def test_scene_against_the_literal_loop(scene, tmp_path, monkeypatch):
    """SemSegTester (fragment_batch 1 and 4) against test.py:94-123 written out with the same model."""
    from ao_amd.ptv2 import evaluate, test_scene
    from ao_amd.ptv2.transform import point_collate

    monkeypatch.delenv("AO_AMD_VOTE", raising=False)
    model, frag, n = scene
    fl = frag["fragment_list"]
    assert len(fl) >= 9
    eager, kept = TC.literal_loop(model, fl, n, 13, DEV, point_collate)
    ref = _votes64_dev(n, 13, [i for i, _ in kept], [x for _, x in kept])
    ref_pred = ref.max(1)[1]
    for fb in (1, 4):
        table = test_scene(model, fl, n, 13, fragment_batch=fb)
        band = BAND_FACTOR * M_VOTE * hold("scene fb%d" % fb, table.votes, eager, ref)
        keep = TC.margin(ref) >= band
        left_out = 1.0 - float(keep.double().mean())
        print("scene fb%d: %d fragments, band %.3e, left out %.5f" % (fb, len(fl), band, left_out))
        assert left_out <= CAP
        result, pred = _run_tester(model, frag, tmp_path / ("fb%d" % fb), fb)
        pred = torch.from_numpy(pred).to(DEV)
        assert torch.equal(pred, table.predict())
        assert torch.equal(pred[keep], ref_pred[keep])
        if left_out == 0.0:
            want = evaluate.confusion_counts(ref_pred, frag["segment"], 13, -1).cpu().numpy()
            s = evaluate.summarize(want[0], want[1] + want[2] - want[0], want[2])
            assert np.array_equal(result["iou_class"], s["iou_class"]) and result["mIoU"] == s["mIoU"]


# test_gpu_bf16.py holds the logits of this configuration under autocast to a relative L2 distance below LOGIT_REL from the
# fp32 logits.  What that implies for the vote: softmax has a Jacobian of norm <= 1/2, so a logit error d_f of a point in
# fragment f moves the difference of two of its votes by at most |d_f| / sqrt(2); over the F fragments that visit the point
# (Cauchy-Schwarz) a margin m can only be overturned when sum_f |d_f|^2 >= 2 m^2 / F.  The errors of all points together are
# at most LOGIT_REL^2 * |logits|^2, so the points that can disagree are at most the K with the smallest 2 m^2 / F whose sum
# stays below that budget.  K comes from the fp32 run and the bound alone, not from the bf16 run.  (Measured for the seeded,
# untrained model of this file: 0 of 30 000 points differ, and the bound allows all of them -- an untrained network's margins
# are far below what an 8 % logit error may move; with a trained network the bound bites.)
LOGIT_REL = 8.4e-2


def test_scene_under_autocast_bf16(scene, tmp_path, monkeypatch):
    from ao_amd.ptv2.transform import point_collate

    monkeypatch.delenv("AO_AMD_VOTE", raising=False)
    model, frag, n = scene
    votes, kept = TC.literal_loop(model, frag["fragment_list"], n, 13, DEV, point_collate)
    visits = torch.zeros(n, device=DEV)
    for idx, _ in kept:
        visits[idx] += 1
    budget = LOGIT_REL ** 2 * sum(float(x.double().square().sum()) for _, x in kept)
    cost = torch.where(visits > 0, 2 * TC.margin(votes.double()) ** 2 / visits.clamp_min(1), torch.full_like(visits, float("inf")).double())
    allowed = int((torch.cumsum(torch.sort(cost)[0], 0) <= budget).sum())
    _, p32 = _run_tester(model, frag, tmp_path / "fp32", 1)
    _, p16 = _run_tester(model, frag, tmp_path / "bf16", 1, autocast=torch.bfloat16)
    assert np.array_equal(p32, votes.max(1)[1].cpu().numpy())
    differ = int((p32 != p16).sum())
    print("autocast bf16: %d of %d points differ from fp32; the logit bound allows %d (agreement %.4f, implied %.4f)"
          % (differ, n, allowed, 1 - differ / n, 1 - allowed / n))
    assert differ <= allowed
