"""tests/msc_csc_ref.py -- the partitioned InfoNCE loss of Masked Scene Contrast v1m2 (CSC;
pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m2_csc.py:182-254) restated in torch on the CPU, independent of
ao_amd/msc/ops.py: the class of an element in the reference's fp32 arithmetic, the loss and its gradients in float64 over five
fixed classes (none, 0, 1, 2, 3).  The reference loops over `part.unique()`; a class that is absent from a scene would add a
cross-entropy over the diagonal alone, which is exactly 0, and "none" is always there because the diagonal is (matched pairs lie
within the matching radius, below r1) -- so five fixed classes give the reference's value.

Index convention, the reference's: S_ij = a_i.b_j with a from view 1 and b from view 2, and the class of (i, j) comes from
rel = x_j - y_i, x the view-1 and y the view-2 coordinate of a pair (`coord1.unsqueeze(0) - coord2.unsqueeze(1)`)."""
import numpy as np
import torch

NONE = 4
CLASSES = 5


def offset2batch(offset, n):
    return np.searchsorted(np.asarray(offset, np.int64), np.arange(n), side="right")


def classes(x, y, r1, r2, dtype=torch.float32):
    """(M, M) int64 in {0, 1, 2, 3, NONE}: element (i, j) from x[j] - y[i].  dtype float32 is the reference's arithmetic,
    statement by statement; float64 evaluates the same formula on the same fp32 inputs and radii without rounding error (the
    two differ only for an element whose distance lies within fp32 rounding of r1 or r2)."""
    x = torch.as_tensor(np.asarray(x, np.float32)).to(dtype)
    y = torch.as_tensor(np.asarray(y, np.float32)).to(dtype)
    r1 = torch.tensor(float(np.float32(r1)), dtype=dtype)
    r2 = torch.tensor(float(np.float32(r2)), dtype=dtype)
    rel = x.unsqueeze(0) - y.unsqueeze(1)
    up, down = rel[:, :, 2] > 0.0, rel[:, :, 2] < 0.0
    d = torch.sqrt(torch.sum(rel.pow(2), 2).add(1e-7))
    out = torch.full(d.shape, NONE, dtype=torch.int64)
    mask = (d > r1) & (d <= r2)
    out[mask & up] = 0
    out[mask & down] = 1
    mask = d > r2
    out[mask & up] = 2
    out[mask & down] = 3
    return out


def distances64(x, y):
    """(M, M) float64: sqrt(|x_j - y_i|^2 + 1e-7)"""
    x, y = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    rel = x[None, :, :] - y[:, None, :]
    return np.sqrt((rel * rel).sum(2) + 1e-7)


def recorded_to_classes(part):
    """the reference's partition matrix (fp32: -1e7, 0, 1, 2, 3) as class ids"""
    part = np.asarray(part)
    out = np.full(part.shape, NONE, np.int64)
    for k in range(4):
        out[part == k] = k
    assert ((part == np.float32(-1e7)) == (out == NONE)).all()
    return out


def scenes_of(pairs, offset1, n1):
    """the scene of every pair: that of its view-1 row"""
    return offset2batch(offset1, n1)[np.asarray(pairs, np.int64)[:, 0]]


def class_counts(o1, o2, offset1, pairs, r1, r2):
    """per scene with a pair (ascending): (M_s, CLASSES) int64, the number of off-diagonal elements of every class in each row"""
    pairs = np.asarray(pairs, np.int64)
    scene = scenes_of(pairs, offset1, len(o1))
    out = []
    for s in np.unique(scene):
        rows = np.nonzero(scene == s)[0]
        cls = classes(np.asarray(o1)[pairs[rows, 0]], np.asarray(o2)[pairs[rows, 1]], r1, r2).numpy()
        np.fill_diagonal(cls, -1)
        out.append(np.stack([(cls == k).sum(1) for k in range(CLASSES)], 1))
    return out


def csc_nce(f1, f2, o1, o2, offset1, pairs, t, r1, r2, partitions=4, g=1.0):
    """float64: dict(loss, pos_sim, neg_sim, df1, df2) with the gradients those of g * loss, and the terms a relative error is
    measured against where a result is a difference that cancels (M_s = 1 or 2): loss_pos, the positive term of the loss,
    sum_s 5 mean_i S_ii / t / (B partitions); neg_sub, what neg_sim subtracts, sum_s pos_s / M_s / B; df1_pos, df2_pos, the
    gradients of -g * loss_pos."""
    pairs = np.asarray(pairs, np.int64)
    b = len(offset1)
    x1 = torch.tensor(np.asarray(f1, np.float64), requires_grad=True)
    x2 = torch.tensor(np.asarray(f2, np.float64), requires_grad=True)
    index = torch.from_numpy(pairs)
    u, v = x1[index[:, 0]], x2[index[:, 1]]
    a = u / (torch.norm(u, p=2, dim=1, keepdim=True) + 1e-7)
    bb = v / (torch.norm(v, p=2, dim=1, keepdim=True) + 1e-7)
    scene = scenes_of(pairs, offset1, len(f1))
    loss = torch.zeros((), dtype=torch.float64)
    loss_pos = torch.zeros((), dtype=torch.float64)
    pos = neg = neg_sub = 0.0
    for s in np.unique(scene):
        rows = np.nonzero(scene == s)[0]
        ms = len(rows)
        sim = a[torch.from_numpy(rows)] @ bb[torch.from_numpy(rows)].T
        pos += float(torch.diagonal(sim).detach().mean())
        neg += float(sim.detach().mean()) - pos / ms
        neg_sub += pos / ms
        cls = classes(np.asarray(o1)[pairs[rows, 0]], np.asarray(o2)[pairs[rows, 1]], r1, r2)
        eye = torch.eye(ms, dtype=torch.bool)
        diag = torch.diagonal(sim) / t
        for k in range(CLASSES):
            masked = torch.where((cls == k) | eye, sim / t, torch.full_like(sim, -float("inf")))
            loss = loss + (torch.logsumexp(masked, 1) - diag).mean()
        loss_pos = loss_pos + CLASSES * diag.mean()
    loss, loss_pos = loss / (b * partitions), loss_pos / (b * partitions)
    df1, df2 = torch.autograd.grad(loss * g, (x1, x2), retain_graph=True)
    df1_pos, df2_pos = torch.autograd.grad(-loss_pos * g, (x1, x2))
    return dict(loss=float(loss.detach()), pos_sim=pos / b, neg_sim=neg / b, df1=df1.numpy(), df2=df2.numpy(), loss_pos=float(loss_pos.detach()),
                neg_sub=neg_sub / b, df1_pos=df1_pos.numpy(), df2_pos=df2_pos.numpy())


def loss_of_counts(counts, b, partitions=4):
    """S == 1 everywhere: loss = sum_s mean_i sum_k log(1 + n_ki) / (B partitions), from the integer class counts alone"""
    return sum(float(np.log1p(c.astype(np.float64)).sum(1).mean()) for c in counts) / (b * partitions)
