"""The inputs of the SPVCNN tests: one batch of three clouds that holds every edge the kernels have, and the model's batch."""
import numpy as np

LEVELS_TESTED = (0, 2, 4)
DEVOX_C = (32, 96, 256)
VOX_C = (6, 32, 96, 256)


def batch():
    """(coord (n, 3) int64, offset (3)).  Cloud 0: 330 points in one stride-16 cell (more than a workgroup's 256 threads); 150
    scattered ones; points on cell faces (multiples of 16: f = 0 at every level); a voxel at 400 whose seven other corners are
    empty at every level; five repeated rows (several points in one level-0 voxel).  Cloud 1: the first 200 rows of cloud 0 again (identical
    coordinates in another cloud) and 100 more.  Cloud 2: one point, on a voxel of clouds 0 and 1."""
    rng = np.random.default_rng(20)
    crowd = rng.integers(64, 80, (330, 3))
    scattered = rng.integers(0, 48, (150, 3))
    faces = np.array([[16, 32, 7], [32, 16, 16], [0, 0, 0], [64, 64, 64]])
    c0 = np.concatenate([crowd, scattered, faces, [[400, 400, 400]], crowd[:5]])
    c1 = np.concatenate([c0[:200], rng.integers(0, 48, (100, 3))])
    c2 = crowd[:1]
    coord = np.concatenate([c0, c1, c2]).astype(np.int64)
    offset = np.cumsum([len(c0), len(c1), len(c2)]).astype(np.int64)
    assert len(coord) == 791 and all(len(coord) % t for t in (2, 4, 8, 32, 64))
    return coord, offset


def model_batch():
    """two clouds of 600 and 611 points in a 48^3 box, every tenth row repeated; six input features; labels in 0..12"""
    rng = np.random.default_rng(21)
    clouds = []
    for m in (540, 550):
        pts = rng.integers(0, 48, (m, 3))
        clouds.append(np.concatenate([pts, pts[::10] if m == 540 else pts[::9]]))
    coord = np.concatenate(clouds).astype(np.int64)
    offset = np.cumsum([len(c) for c in clouds]).astype(np.int64)
    feat = rng.standard_normal((len(coord), 6)).astype(np.float32)
    return coord, offset, feat, rng.integers(0, 13, len(coord)).astype(np.int64)
