"""Small seeded clouds for the Swin3D tests, named by what they break.  A case lists the member counts of its windows; window w
gets that many distinct slots of its ws^3, so with the case's own shift the partition is known by construction.  Voxels come in a
shuffled order."""
import numpy as np

ROWS = {"XYZ": 1, "XYZ_RGB": 2, "XYZ_RGB_NORM": 3}
QUANT = 4

# name: (window_size, shift, H, hd, cRSE, clouds, member counts of the windows of one cloud)
CASES = {
    # windows of exactly one voxel; their table gradients are exactly 0, so four small windows keep the relative error defined
    "single-member": (5, 0, 6, 16, "XYZ_RGB", 1, [1] * 196 + [2, 3, 5, 2]),
    "tile-edge": (5, 0, 5, 8, "XYZ", 1, [16, 17] * 8),                             # one full tile; one tile and one key more
    "dense-5": (5, 0, 6, 16, "XYZ_RGB_NORM", 1, [125] + [9, 33, 48]),              # r_d reaches 0 and 2 L - 1
    "dense-7": (7, 0, 5, 8, "XYZ_RGB", 1, [343, 20]),                              # the largest window; 22 tiles
    "two-clouds": (5, 0, 6, 8, "XYZ_RGB_NORM", 2, [30, 7, 19, 40, 12, 3, 25, 14]),  # identical coordinates: must not merge
    "shifted": (5, 2, 5, 16, "XYZ_RGB_NORM", 1, [21, 1, 16, 60, 35, 18, 64]),      # coordinates 0 and negative
}


def table_rows(name):
    ws, cRSE = CASES[name][0], CASES[name][4]
    return [ws * QUANT, 4 * QUANT, 4 * QUANT][:ROWS[cRSE]]


def cloud(name):
    """grid_coord (n, 3) int64, batch (n) int64, local_xyz (n, 3) in [0, 1), colors (n, 6) in [-1, 1]"""
    ws, shift, _, _, _, clouds, counts = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    corners = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    corners = corners[(corners != 0).any(1)]
    corners = corners[rng.permutation(len(corners))[:len(counts)]]
    if name == "shifted":
        corners[0] = 0   # slot (shift, shift, shift) of window 0 is the voxel (0, 0, 0)
    grid = []
    for corner, m in zip(corners, counts):
        slots = np.sort(rng.permutation(ws ** 3)[:m])
        if name == "shifted" and (corner == 0).all():
            slots = np.union1d(slots[1:], [shift * (ws * ws + ws + 1)])
        grid.append(corner * ws - shift + np.stack([slots // (ws * ws), slots // ws % ws, slots % ws], -1))
    grid = np.concatenate(grid)
    grid, batch = np.concatenate([grid] * clouds), np.repeat(np.arange(clouds), len(grid))
    perm = rng.permutation(len(grid))
    n = len(grid)
    return dict(grid_coord=grid[perm].astype(np.int64), batch=batch[perm].astype(np.int64),
                local_xyz=rng.random((n, 3), dtype=np.float32), colors=rng.uniform(-1, 1, (n, 6)).astype(np.float32))


def partition(grid_coord, batch, ws, shift):
    """{(cloud, wx, wy, wz): rows sorted by w_w_id} from a dictionary, and w_w_xyz (n, 3)"""
    slot = (grid_coord + shift) % ws
    wid = slot[:, 0] * ws * ws + slot[:, 1] * ws + slot[:, 2]
    parts = {}
    for i, (b, w) in enumerate(zip(batch.tolist(), ((grid_coord + shift) // ws).tolist())):
        parts.setdefault((b,) + tuple(w), []).append(i)
    return {k: sorted(v, key=lambda i: wid[i]) for k, v in parts.items()}, slot


def attention_inputs(name):
    """the cloud, its partition under the case's shift, signals (n, 3 S) in the voxels' own order, qkv, the flat tables, g_out"""
    ws, shift, H, hd, cRSE, _, _ = CASES[name]
    t = cloud(name)
    parts, slot = partition(t["grid_coord"], t["batch"], ws, shift)
    S, rows, n = ROWS[cRSE], table_rows(name), len(slot)
    sig = np.concatenate([(slot.astype(np.float32) + t["local_xyz"]) * np.float32(QUANT), t["colors"] * np.float32(2 * QUANT)], 1)[:, :3 * S]
    rng = np.random.default_rng(100 + n)
    R = 6 * sum(rows)
    t.update(parts=list(parts.values()), signals=np.ascontiguousarray(sig), qkv=rng.standard_normal((n, 3 * H * hd)).astype(np.float32),
             g_out=rng.standard_normal((n, H * hd)).astype(np.float32),
             **{k: (0.5 * rng.standard_normal(R * H * hd)).astype(np.float32) for k in ("q_table", "k_table", "v_table")})
    return t
