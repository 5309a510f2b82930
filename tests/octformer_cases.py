"""Small seeded clouds for the OctFormer tests: unique coordinates in [0, 512) per cloud (depth 9), in (cloud, Morton key) order."""
import numpy as np

DEPTH = 9

# name: (nodes per cloud, K, D, H, hd) -- named by what it can break
ATTENTION = {
    "two-clouds-dilated": ((100, 145), 26, 4, 6, 16),   # a patch that spans two clouds; a padded tail; H not a multiple of 4
    "two-clouds": ((100, 145), 26, 1, 6, 16),           # same clouds, undilated
    "less-than-a-patch": ((19,), 26, 4, 6, 16),         # four patches of 5 / 5 / 5 / 4 real slots
    "full-tile-wide-heads": ((60, 70, 70), 32, 2, 3, 32),
    "tiny-patch-one-head": ((70,), 8, 3, 1, 16),
}


def morton(x, y, z, depth=DEPTH):
    key = np.zeros(len(x), np.int64)
    for i in range(depth):
        key |= ((x >> i) & 1) << (3 * i + 2) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i)
    return key


def cloud(counts, seed):
    """(xyz (n, 3) int64, batch (n) int64) sorted by (cloud, key); a third of each cloud is a dense blob so that neighbours exist"""
    rng = np.random.default_rng(seed)
    xyz, batch = [], []
    for b, m in enumerate(counts):
        blob = rng.integers(200, 206, (4 * m, 3))
        wide = rng.integers(0, 512, (4 * m, 3))
        pts = np.unique(np.concatenate([blob[: m // 3 * 4], wide]), axis=0)
        pts = pts[rng.permutation(len(pts))[:m]].astype(np.int64)
        pts = pts[np.argsort(morton(pts[:, 0], pts[:, 1], pts[:, 2]))]
        xyz.append(pts)
        batch.append(np.full(m, b, np.int64))
    return np.concatenate(xyz), np.concatenate(batch)


def attention_inputs(name):
    counts, K, D, H, hd = ATTENTION[name]
    xyz, batch = cloud(counts, seed=sorted(ATTENTION).index(name))
    rng = np.random.default_rng(100 + len(xyz))
    n, C, R = len(xyz), H * hd, 2 * int(0.8 * K * D ** 0.5) + 1
    return dict(xyz=xyz, batch=batch, qkv=rng.standard_normal((n, 3 * C)).astype(np.float32),
                table=(0.5 * rng.standard_normal((3 * R, H))).astype(np.float32),
                g_out=rng.standard_normal((n, C)).astype(np.float32))
