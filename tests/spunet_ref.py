"""SpUNet-v1m1 as plain numpy / torch in a chosen dtype, written from the contract of DESIGN.md section 11:

    tables     a dict from (cloud, x, y, z) to row, by brute force; level l + 1 is the sorted set of (cloud, coord >> 1)
    subm       out[i]               = sum over kappa of W[kappa] in[nbr[i, kappa]]
    down       out[o]               = sum over kappa of W[kappa] in[child[o, kappa]]
    inverse    out[child[o, kappa]] = W[kappa] in[o]

with W (Cout, k, k, k, Cin) and kappa the row-major kernel offset along the three coordinate columns.  The modules carry the
reference's state-dict keys, so one state dict serves this file, ao_amd.spunet and the reference.  Runs on any device in any
dtype; nothing here imports the reference or ao_amd.
"""
import collections

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

LEVELS = 5
CHANNELS = (32, 64, 128, 256, 256, 128, 96, 96)
LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)


def _nbr(voxels, index, k):
    """(n, k^3) table of one level: voxels a list of (cloud, x, y, z), index their dict"""
    half = k // 2
    tab = np.full((len(voxels), k ** 3), -1, np.int32)
    for i, (s, x, y, z) in enumerate(voxels):
        kappa = 0
        for dx in range(-half, half + 1):
            for dy in range(-half, half + 1):
                for dz in range(-half, half + 1):
                    tab[i, kappa] = index.get((s, x + dx, y + dy, z + dz), -1)
                    kappa += 1
    return tab


def build_tables(coord, offset, levels=LEVELS):
    """coord (n, 3) integers, offset (b) cloud ends -> dict(n, coord, offset, nbr3, nbr5, child, parent, slot) of numpy arrays,
    the fields of ao_amd.spunet.SpconvTables"""
    coord, offset = np.asarray(coord), np.asarray(offset)
    cloud = np.searchsorted(offset, np.arange(coord.shape[0]), side="right")
    voxels = [(int(s), int(x), int(y), int(z)) for s, (x, y, z) in zip(cloud, coord)]
    out = dict(n=[], coord=[], offset=[], nbr3=[], child=[], parent=[], slot=[])
    for level in range(levels):
        index = {v: i for i, v in enumerate(voxels)}
        assert len(index) == len(voxels), "two rows on one voxel"
        out["n"].append(len(voxels))
        out["coord"].append(np.array([v[1:] for v in voxels], np.int32).reshape(-1, 3))
        out["offset"].append(np.array([sum(1 for v in voxels if v[0] <= s) for s in range(len(offset))], np.int32))
        out["nbr3"].append(_nbr(voxels, index, 3))
        if level == 0:
            out["nbr5"] = _nbr(voxels, index, 5)
        if level + 1 == levels:
            break
        coarse = sorted({(s, x >> 1, y >> 1, z >> 1) for s, x, y, z in voxels})
        cindex = {v: i for i, v in enumerate(coarse)}
        child = np.full((len(coarse), 8), -1, np.int32)
        parent, slot = np.empty(len(voxels), np.int32), np.empty(len(voxels), np.int32)
        for i, (s, x, y, z) in enumerate(voxels):
            parent[i] = cindex[(s, x >> 1, y >> 1, z >> 1)]
            slot[i] = ((x & 1) << 2) | ((y & 1) << 1) | (z & 1)
            child[parent[i], slot[i]] = i
        out["child"].append(child)
        out["parent"].append(parent)
        out["slot"].append(slot)
        voxels = coarse
    return out


def tables_to(tables, device):
    out = {"n": list(tables["n"]), "nbr5": torch.from_numpy(tables["nbr5"]).to(device)}
    for key in ("coord", "offset", "nbr3", "child", "parent", "slot"):
        out[key] = [torch.from_numpy(a).to(device) for a in tables[key]]
    return out


def gather(x, tab, weight):
    """out[r] = sum over kappa of W[kappa] in[tab[r, kappa]]; weight (Cout, k, k, k, Cin)"""
    w = weight.reshape(weight.shape[0], -1, weight.shape[-1])
    out = x.new_zeros((tab.shape[0], w.shape[0]))
    for kappa in range(tab.shape[1]):
        rows = torch.nonzero(tab[:, kappa] >= 0).squeeze(1)
        if rows.numel():
            out = out.index_add(0, rows, x[tab[rows, kappa].long()] @ w[:, kappa].t())
    return out


def scatter(x, tab, weight, n_out):
    """out[tab[r, kappa]] = W[kappa] in[r]"""
    w = weight.reshape(weight.shape[0], -1, weight.shape[-1])
    out = x.new_zeros((n_out, w.shape[0]))
    for kappa in range(tab.shape[1]):
        rows = torch.nonzero(tab[:, kappa] >= 0).squeeze(1)
        if rows.numel():
            out = out.index_add(0, tab[rows, kappa].long(), x[rows] @ w[:, kappa].t())
    return out


class Conv(nn.Module):
    """kind: "subm" (k 1, 3, 5), "down", "inverse"; the parameter names and shapes of spconv's modules"""

    def __init__(self, kind, cin, cout, k, bias=False):
        super().__init__()
        self.kind, self.k = kind, k
        self.weight = nn.Parameter(torch.zeros(cout, k, k, k, cin))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

    def forward(self, x, tables, level):
        if self.kind == "down":
            return gather(x, tables["child"][level], self.weight), level + 1
        if self.kind == "inverse":
            return scatter(x, tables["child"][level - 1], self.weight, tables["n"][level - 1]), level - 1
        if self.k == 1:
            return F.linear(x, self.weight.reshape(self.weight.shape[0], -1), self.bias), level
        tab = tables["nbr5"] if self.k == 5 else tables["nbr3"][level]
        return gather(x, tab, self.weight), level


def norm(c):
    return nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)


class Margin:
    """the smallest |pre-activation| any ReLU has seen since reset()"""
    value = float("inf")

    @classmethod
    def relu(cls, x):
        if x.numel():
            cls.value = min(cls.value, float(x.detach().abs().min()))
        return F.relu(x)

    @classmethod
    def reset(cls):
        cls.value = float("inf")


class Block(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.proj = nn.Sequential(nn.Identity()) if cin == cout else nn.Sequential(Conv("subm", cin, cout, 1), norm(cout))
        self.conv1 = Conv("subm", cin, cout, 3)
        self.bn1 = norm(cout)
        self.conv2 = Conv("subm", cout, cout, 3)
        self.bn2 = norm(cout)

    def forward(self, x, tables, level):
        out = Margin.relu(self.bn1(self.conv1(x, tables, level)[0]))
        out = self.bn2(self.conv2(out, tables, level)[0])
        res = x if len(self.proj) == 1 else self.proj[1](self.proj[0](x, tables, level)[0])
        return Margin.relu(out + res)


class SpUNet(nn.Module):
    def __init__(self, in_channels=6, num_classes=13, base_channels=32, channels=CHANNELS, layers=LAYERS):
        super().__init__()
        self.num_stages, self.num_classes = len(layers) // 2, num_classes
        self.conv_input = nn.Sequential(Conv("subm", in_channels, base_channels, 5), norm(base_channels), nn.ReLU())
        enc, dec = base_channels, channels[-1]
        self.down, self.up, self.enc, self.dec = nn.ModuleList(), nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for s in range(self.num_stages):
            self.down.append(nn.Sequential(Conv("down", enc, channels[s], 2), norm(channels[s]), nn.ReLU()))
            self.enc.append(nn.Sequential(collections.OrderedDict(
                ("block%d" % i, Block(channels[s], channels[s])) for i in range(layers[s]))))
            self.up.append(nn.Sequential(Conv("inverse", channels[len(channels) - s - 2], dec, 2), norm(dec), nn.ReLU()))
            self.dec.append(nn.Sequential(collections.OrderedDict(
                ("block%d" % i, Block(dec + enc if i == 0 else dec, dec)) for i in range(layers[len(channels) - s - 1]))))
            enc, dec = channels[s], channels[len(channels) - s - 2]
        self.final = Conv("subm", channels[-1], num_classes, 1, bias=True) if num_classes > 0 else nn.Identity()

    @staticmethod
    def _head(seq, x, tables, level):
        x, level = seq[0](x, tables, level)
        return Margin.relu(seq[1](x)), level

    def forward(self, input_dict, tables=None):
        feat = input_dict["feat"]
        if tables is None:
            tables = tables_to(build_tables(input_dict["discrete_coord"].cpu().numpy(), input_dict["offset"].cpu().numpy()),
                               feat.device)
        x, level = self._head(self.conv_input, feat, tables, 0)
        skips = [x]
        for s in range(self.num_stages):
            x, level = self._head(self.down[s], x, tables, level)
            for blk in self.enc[s]:
                x = blk(x, tables, level)
            skips.append(x)
        x = skips.pop(-1)
        for s in reversed(range(self.num_stages)):
            x, level = self._head(self.up[s], x, tables, level)
            x = torch.cat((x, skips.pop(-1)), 1)
            for blk in self.dec[s]:
                x = blk(x, tables, level)
        return self.final(x, tables, level)[0] if self.num_classes > 0 else x
