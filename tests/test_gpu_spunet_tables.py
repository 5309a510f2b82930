"""GPU: the tables of ao_amd.spunet.build_tables (ao_amd/csrc/spconv_tables.hip), integer-exact against the brute-force builder
of tests/spunet_ref.py (a dict from voxel to row), on the smallest inputs at which a table can go wrong
(tests/spunet_cases.table_cases), and the three kinds of bad input."""
import numpy as np
import pytest
import torch

from tests import spunet_cases as SC
from tests import spunet_ref as R

pytestmark = pytest.mark.gpu

CASES = SC.table_cases()
FIELDS = ("coord", "offset", "nbr3", "child", "parent", "slot")


def _build(coord, offset):
    from ao_amd import spunet

    return spunet.build_tables(torch.from_numpy(coord).cuda(), torch.from_numpy(offset).cuda())


def _same(got, want):
    assert got.n == want["n"]
    assert torch.equal(got.nbr5.cpu(), torch.from_numpy(want["nbr5"]))
    for field in FIELDS:
        have = getattr(got, field)
        assert len(have) == len(want[field]), field
        for level, (a, b) in enumerate(zip(have, want[field])):
            assert a.dtype == torch.int32 and tuple(a.shape) == tuple(b.shape), (field, level, tuple(a.shape), b.shape)
            assert torch.equal(a.cpu(), torch.from_numpy(b)), (field, level)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_equal_the_brute_force_builder(name):
    coord, offset = CASES[name]
    want = R.build_tables(coord, offset)
    _same(_build(coord, offset), want)
    # what the case was made for
    if name == "two_clouds":
        a, b = {tuple(v) for v in coord[:70]}, {tuple(v) for v in coord[70:]}
        assert a & b, "the same coordinate in both clouds"
        assert int(want["nbr3"][0][:70].max()) < 70 and int(want["nbr3"][0][70:][want["nbr3"][0][70:] >= 0].min()) >= 70
    if name == "zero_and_isolated":
        zero = int(np.nonzero((coord == 0).all(1))[0][0])
        far = int(np.nonzero((coord == 500).all(1))[0][0])
        lows = [k for k in range(125) if min(k // 25, (k // 5) % 5, k % 5) < 2]
        assert (want["nbr5"][zero][lows] == -1).all()
        assert (want["nbr3"][0][far] >= 0).sum() == 1 and want["nbr3"][0][far][13] == far
    if name == "full_block5":
        assert (want["nbr5"] >= 0).all(1).sum() == 1
    if name == "one_voxel_cloud":
        assert want["nbr3"][0][0].tolist() == [-1] * 13 + [0] + [-1] * 13 and want["n"] == [3, 2, 2, 2, 2]
    if name == "upper_bound":
        assert want["nbr3"][0][0][13] == 0 and want["nbr3"][0][0][4] == 1 and (want["nbr3"][0][0][14:] == -1).all()
    if name == "eight_and_one":
        counts = sorted((want["child"][0] >= 0).sum(1).tolist())
        assert counts == [1, 8]
    if name == "to_one_voxel":
        assert want["n"][4] == 1 and want["n"][3] > 1


@pytest.mark.parametrize("kind", ["duplicate", "negative", "oversized", "duplicate_in_second_cloud"])
def test_bad_input_raises(kind):
    coord, offset = SC.lattice((70, 9), 0)
    coord = coord.copy()
    if kind == "duplicate":
        coord[5] = coord[40]
    elif kind == "duplicate_in_second_cloud":
        coord[78] = coord[72]
    elif kind == "negative":
        coord[3, 1] = -1
    else:
        coord[7, 2] = SC.COORD_MAX + 1
    with pytest.raises(ValueError, match={"duplicate": "same voxel", "duplicate_in_second_cloud": "same voxel",
                                          "negative": "negative", "oversized": "2\\^18"}[kind]):
        _build(coord, offset)
    # int64 coordinates beyond int32 are refused too, not wrapped
    if kind == "oversized":
        from ao_amd import spunet

        big = torch.from_numpy(coord).long().cuda()
        big[7, 2] = 1 << 40
        with pytest.raises(ValueError, match="2\\^18"):
            spunet.build_tables(big, torch.from_numpy(offset).cuda())
    # the same voxel in two clouds is no duplicate
    coord, offset = SC.lattice((70, 9), 0)
    coord[75] = coord[2]
    if len({tuple(v) for v in coord[70:]}) == 9:
        _build(coord, offset)


def test_two_runs_give_identical_tables():
    coord, offset = SC.lattice((3001, 200), 5)
    a, b = _build(coord, offset), _build(coord, offset)
    assert a.n == b.n and torch.equal(a.nbr5, b.nbr5)
    for field in FIELDS:
        for x, y in zip(getattr(a, field), getattr(b, field)):
            assert torch.equal(x, y), field
    # and a larger one equals the brute force too (many workgroups in every launch)
    _same(a, R.build_tables(coord, offset))
