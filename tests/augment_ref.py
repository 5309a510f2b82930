"""A numpy restatement of the augmentation program's interpreter (ao_amd/csrc/augment.hip) and of its noise: Philox4x32-10 +
Box-Muller.  No test in here.  The interpreter follows the kernel's step semantics one rounding at a time (numpy's float64 /
float32 scalars and arrays round every operation on its own), so what it computes for a plan of `transform.fuse_plan` is what
the kernel must compute; the noise functions are the float64 statement the kernel's fp32 normals are measured against."""
import numpy as np

from ao_amd import _abi

K = _abi.data_consts
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32-valued, key: (k0, k1) -> (..., 4) uint64 array of 32-bit words"""
    c = [np.asarray(counter[..., j], np.uint64) for j in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        a, b = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(b >> np.uint64(32)) ^ c[1] ^ k0, b & np.uint64(M32), (a >> np.uint64(32)) ^ c[3] ^ k1, a & np.uint64(M32)]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32), (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
    return np.stack(c, -1)


def normals64(n, seed, stream, first=0):
    """the three normals of points first .. first + n - 1 in float64: uniforms ((x >> 8) + 0.5) 2^-24, r = sqrt(-2 ln u0)"""
    i = np.arange(first, first + n, dtype=np.uint64)
    counter = np.stack([i & np.uint64(M32), i >> np.uint64(32), np.full(n, stream, np.uint64), np.zeros(n, np.uint64)], -1)
    seed = int(seed) & ((1 << 64) - 1)
    w = philox4x32_10(counter, (seed & M32, seed >> 32))
    u = ((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r0, r1 = np.sqrt(-2 * np.log(u[:, 0])), np.sqrt(-2 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]), r1 * np.cos(2 * np.pi * u[:, 3])], -1)


def blur3(grid, axis):
    """one pass of the kernel's 3-tap blur: ((in[-1] w + in[0] w) + in[+1] w) in float64, w = float32(1/3), zero outside"""
    g = np.moveaxis(np.asarray(grid, np.float64), axis, 0)
    w = np.float64(np.float32(1) / np.float32(3))
    zero = np.zeros_like(g[:1])
    acc = np.concatenate([zero, g[:-1]]) * w
    acc = acc + g * w
    acc = acc + np.concatenate([g[1:], zero]) * w
    return np.moveaxis(acc, 0, axis).astype(np.float32)


def blurred(grid):
    for axis in (0, 1, 2, 0, 1, 2):
        grid = blur3(grid, axis)
    return grid


def bounds_of(coord, color):
    b = np.zeros(12)
    b[0:3], b[3:6] = coord.min(0), coord.max(0)
    if color is not None:
        b[6:9], b[9:12] = color.min(0), color.max(0)
    return b


def centre(lo, hi, fp32):
    if fp32:
        return np.float64((np.float32(lo) + np.float32(hi)) * np.float32(0.5))
    return (np.float64(lo) + np.float64(hi)) * 0.5


def trilinear(field, x, start, spacing):
    """the kernel's lookup: t = (x - start) / spacing per axis, corners in the order 000, 001, 010, ..., weights
    ((wx wy) wz), float64"""
    dims = field.shape[:3]
    t = (x - np.asarray(start)) / np.asarray(spacing)
    inside = ((t >= 0) & (t <= np.asarray(dims) - 1)).all(1)
    cell = np.clip(np.floor(t).astype(np.int64), 0, np.asarray(dims) - 2)
    cell[~inside] = 0
    f = t - cell
    acc = np.zeros_like(x)
    for corner in range(8):
        o = np.array([corner >> 2, (corner >> 1) & 1, corner & 1])
        wgt = np.where(o[0], f[:, 0], 1.0 - f[:, 0])
        wgt = wgt * np.where(o[1], f[:, 1], 1.0 - f[:, 1])
        wgt = wgt * np.where(o[2], f[:, 2], 1.0 - f[:, 2])
        v = field[cell[:, 0] + o[0], cell[:, 1] + o[1], cell[:, 2] + o[2]].astype(np.float64)
        acc = acc + v * wgt[:, None]
    acc[~inside] = 0
    return acc


def run_plan(segs, coord, color, seed=0, elastic_grid=None):
    """coord (n, 3) float32 / float64, color (n, 3) float32 or None through the segments of a plan, as the kernel does.
    elastic_grid: transform.elastic_grid (passed in so that this module imports no torch)."""
    x = np.asarray(coord, np.float64).copy()
    in_f32 = np.asarray(coord).dtype == np.float32
    c = None if color is None else np.asarray(color, np.float32).copy()
    n = x.shape[0]
    for si, seg in enumerate(segs):
        if seg["bounds"]:
            b = bounds_of(x, c)
        for step in seg["steps"]:
            kind, p, fp32 = step["kind"], [np.float64(v) for v in step.get("p", ())], bool(step["flags"] & K["PTV2_AUG_FLAG_FP32"])
            g = None
            if kind in (K["PTV2_AUG_JITTER"], K["PTV2_AUG_COLOR_JITTER"]):
                g = step.get("noise")
                g = normals64(n, seed, step.get("stream", 0)).astype(np.float32) if g is None else np.asarray(g, np.float32)
                g = g.astype(np.float64)
            if kind == K["PTV2_AUG_CENTER_SHIFT"]:
                x[:, 0] = x[:, 0] - centre(b[0], b[3], fp32)
                x[:, 1] = x[:, 1] - centre(b[1], b[4], fp32)
                if step["flags"] & K["PTV2_AUG_FLAG_APPLY_Z"]:
                    x[:, 2] = x[:, 2] - b[2]
            elif kind == K["PTV2_AUG_ROTATE"]:
                if step["flags"] & K["PTV2_AUG_FLAG_BOUNDS_CENTER"]:
                    ctr = np.array([centre(b[d], b[3 + d], fp32) for d in range(3)])
                else:
                    ctr = np.array(p[9:12])
                t = x - ctr
                if fp32:
                    t = t.astype(np.float32).astype(np.float64)
                x = np.stack([((t[:, 0] * p[3 * j] + t[:, 1] * p[3 * j + 1]) + t[:, 2] * p[3 * j + 2]) + ctr[j] for j in range(3)], 1)
            elif kind == K["PTV2_AUG_SCALE"]:
                x = x * np.array(p[:3])
            elif kind == K["PTV2_AUG_SHIFT"]:
                x = x + np.array(p[:3])
            elif kind == K["PTV2_AUG_CLIP"]:
                x = np.minimum(np.maximum(x, np.array(p[:3])), np.array(p[3:6]))
            elif kind == K["PTV2_AUG_JITTER"]:
                x = x + np.minimum(np.maximum(p[0] * g, -p[1]), p[1])
            elif kind == K["PTV2_AUG_ELASTIC"]:
                dims, start, spacing = elastic_grid(b[0:3], b[3:6], fp32, step["granularity"])
                grid = np.asarray(step["grid"](dims) if callable(step["grid"]) else step["grid"], np.float32)
                assert grid.shape == tuple(dims) + (3,), (grid.shape, dims)
                x = x + trilinear(blurred(grid), x, start, spacing) * np.float64(step["magnitude"])
            elif kind == K["PTV2_AUG_ROUND_F32"]:
                x = x.astype(np.float32).astype(np.float64)
            elif kind == K["PTV2_AUG_COLOR_CONTRAST"]:
                lo, hi = b[6:9].astype(np.float32), b[9:12].astype(np.float32)
                stretched = (c - lo) * (np.float32(255) / (hi - lo))
                c = np.float32(p[0]) * c + np.float32(p[1]) * stretched
            elif kind == K["PTV2_AUG_COLOR_TRANSLATE"]:
                c = np.minimum(np.maximum(np.array(p[:3]) + c.astype(np.float64), 0.0), 255.0).astype(np.float32)
            elif kind == K["PTV2_AUG_COLOR_JITTER"]:
                c = np.minimum(np.maximum(g * p[0] + c.astype(np.float64), 0.0), 255.0).astype(np.float32)
            elif kind == K["PTV2_AUG_COLOR_MUL"]:
                c = c * np.float32(p[0])
            else:
                raise ValueError(kind)
        if not seg["out_f64"]:
            x = x.astype(np.float32).astype(np.float64)
    out_f32 = not segs[-1]["out_f64"] if segs else in_f32
    return (x.astype(np.float32) if out_f32 else x), c
