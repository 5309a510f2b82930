"""A plain restatement of SPVCNN's arithmetic (include/ptv2_spv_hip.h states the formulas; DESIGN.md section 20 the kernel offset
orders) in the dtype and on the device of its operands: float64 for the reference, fp32 for the eager distance.  All geometry
comes from a Python dictionary of (cloud, x, y, z) -> row, the rows of a level being the distinct voxels in ascending order; none
of the library's tables is read."""
import numpy as np
import torch
import torch.nn.functional as F

CUBE3 = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
CUBE2 = [(jx, jy, jz) for jx in (0, 1) for jy in (0, 1) for jz in (0, 1)]


class Geometry:
    """per level l: keys[l] the sorted (cloud, x, y, z) voxels, row[l] (n), corner[l] (n, 8), frac[l] (n, 3) float64, nbr[l]
    (n_l, 27), child[l] (n_l, 8) rows of level l - 1 (l >= 1); long tensors on `device`"""

    def __init__(self, coord, offset, device="cpu", levels=5):
        coord = np.asarray(coord, np.int64)
        cloud = np.searchsorted(np.asarray(offset), np.arange(len(coord)), side="right")
        dev = lambda a: torch.as_tensor(np.asarray(a), device=device)  # noqa: E731
        self.n, self.keys, self.row, self.corner, self.frac, self.nbr, self.child = len(coord), [], [], [], [], [], [None]
        for l in range(levels):
            of_point = [(int(b),) + tuple(int(v) >> l for v in p) for b, p in zip(cloud, coord)]
            keys = sorted(set(of_point))
            rows = {k: i for i, k in enumerate(keys)}
            look = lambda k, d, table=rows: table.get((k[0], k[1] + d[0], k[2] + d[1], k[3] + d[2]), -1)  # noqa: E731
            if l:
                self.child.append(dev([[self._rows.get((k[0], 2 * k[1] + d[0], 2 * k[2] + d[1], 2 * k[3] + d[2]), -1) for d in CUBE2] for k in keys]))
            self._rows = rows
            self.keys.append(keys)
            self.row.append(dev([rows[k] for k in of_point]))
            self.corner.append(dev([[look(k, d) for d in CUBE2] for k in of_point]))
            self.frac.append(dev((coord & ((1 << l) - 1)) / float(1 << l)))
            self.nbr.append(dev([[look(k, d) for d in CUBE3] for k in keys]))


def _rows_of(x, index):  # x[index], zeros where index is -1
    return x[index.clamp(min=0)] * (index >= 0).to(x.dtype).unsqueeze(-1)


def devoxelize(feat, geo, level, add=None):
    idx, f = geo.corner[level], geo.frac[level].to(feat.dtype)
    w = torch.stack([torch.stack([f[:, a] if j[a] else 1 - f[:, a] for a in range(3)]).prod(0) for j in CUBE2], 1)
    w = w * (idx >= 0).to(feat.dtype)
    w = w / (w.sum(1, keepdim=True) + 1e-8)
    out = (_rows_of(feat, idx) * w.unsqueeze(-1)).sum(1)
    return out if add is None else out + add


def voxelize(x, geo, level):
    row, m = geo.row[level], len(geo.keys[level])
    total = torch.zeros((m, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, row, x)
    return total / torch.bincount(row, minlength=m).to(x.dtype).unsqueeze(1)


def model(P, geo, feat, training):
    """SPVCNN.forward (ts_spvcnn.py:384-436) with dropout off; P: state dict in the working dtype"""

    def bn(name, x, relu=True):
        y = F.batch_norm(x, P[name + ".running_mean"].clone(), P[name + ".running_var"].clone(), P[name + ".weight"], P[name + ".bias"],
                         training, 0.1, 1e-5)
        return F.relu(y) if relu else y

    def conv3(name, x, l):
        K = P[name + ".kernel"]
        return sum(_rows_of(x, geo.nbr[l][:, kappa]) @ K[(d[0] + 1) + 3 * (d[1] + 1) + 9 * (d[2] + 1)] for kappa, d in enumerate(CUBE3))

    def down(name, x, l):  # level l -> l + 1
        return sum(_rows_of(x, geo.child[l + 1][:, k]) @ P[name + ".kernel"][k] for k in range(8))

    def up(name, x, l):  # level l -> l - 1
        out = torch.zeros((len(geo.keys[l - 1]), P[name + ".kernel"].shape[2]), dtype=x.dtype, device=x.device)
        for k in range(8):
            j = geo.child[l][:, k]
            out = out.index_add(0, j[j >= 0], (x @ P[name + ".kernel"][k])[j >= 0])
        return out

    def residual(name, x, l):
        y = bn(name + ".net.4", conv3(name + ".net.3", bn(name + ".net.1", conv3(name + ".net.0", x, l)), l), relu=False)
        if name + ".downsample.0.kernel" in P:
            x = bn(name + ".downsample.1", x @ P[name + ".downsample.0.kernel"], relu=False)
        return F.relu(y + x)

    def blocks(name, x, l, first):
        while "%s.%d.net.0.kernel" % (name, first) in P:
            x, first = residual("%s.%d" % (name, first), x, l), first + 1
        return x

    def stage(s, x):  # stage s: level s - 1 -> s
        return blocks("stage%d" % s, bn("stage%d.0.net.1" % s, down("stage%d.0.net.0" % s, x, s - 1)), s, 1)

    def decoder(s, x, skip, l):  # up s: level l -> l - 1
        y = bn("up%d.0.net.1" % s, up("up%d.0.net.0" % s, x, l))
        return blocks("up%d.1" % s, torch.cat((y, skip), 1), l - 1, 0)

    def transform(i, z):
        return bn("point_transforms.%d.1" % i, z @ P["point_transforms.%d.0.weight" % i].t() + P["point_transforms.%d.0.bias" % i])

    x0 = bn("stem.4", conv3("stem.3", bn("stem.1", conv3("stem.0", voxelize(feat, geo, 0), 0)), 0))
    z0 = devoxelize(x0, geo, 0)
    x1 = stage(1, voxelize(z0, geo, 0))
    x2 = stage(2, x1)
    x3 = stage(3, x2)
    x4 = stage(4, x3)
    z1 = devoxelize(x4, geo, 4, transform(0, z0))
    y2 = decoder(2, decoder(1, voxelize(z1, geo, 4), x3, 4), x2, 3)
    z2 = devoxelize(y2, geo, 2, transform(1, z1))
    y4 = decoder(4, decoder(3, voxelize(z2, geo, 2), x1, 2), x0, 1)
    z3 = devoxelize(y4, geo, 0, transform(2, z2))
    return z3 @ P["classifier.0.weight"].t() + P["classifier.0.bias"]
