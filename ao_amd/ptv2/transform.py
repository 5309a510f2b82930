"""Device-side counterparts of the three input-pipeline transforms that set the size of a training scene
(SURVEY.md §8f row 3): GridSample, SphereCrop, Collect + the point collate.

Same constructor arguments, dictionary keys and results as pointcept/datasets/transform.py:27-50 (Collect),
:769-897 (GridSample), :899-999 (SphereCrop) and pointcept/datasets/utils.py:14-54 (collate), but on CUDA tensors:
the reference runs these in numpy on 16 CPU workers per GPU; here a raw scan is voxelised and cropped on the GPU
that trains on it (voxel keys / squared distances: ao_amd/csrc/dataops.hip; sort / run-length: torch = rocPRIM).

The test-time pipeline (pointcept/datasets/s3dis.py:212-236) is here too: the transforms the PT-v2m2 test configs name
(CenterShift :129-142, NormalizeColor :100-104, RandomScale :285-296, RandomFlip :300-315, RandomRotateTargetAngle :246-281,
ToTensor, Compose :1107-1117) and `test_fragments`, which builds the reference's `fragment_list` from them.  These are plain
torch on whatever device the data is on.  Arithmetic: the reference works on fp32 numpy arrays and multiplies / rotates with
float64 operands, so `coord *= scale` is one float64 product rounded to fp32 -- done the same way here (bitwise equal).  Its
rotation `np.dot(coord, rot_t.T)` turns `coord` into a float64 array that stays float64 until ToTensor; here the rotation
(and the centre shift around it) is computed in float64 with the same matrix and rounded to fp32 ONCE, right after it, so
that GridSample sees fp32 as everywhere else in this module: the coordinates equal the reference's final fp32 values to
1 ulp, and a point within that distance of a voxel border can land in the neighbouring voxel.

Where the reference's result depends on numpy's unstable argsort (which point of a voxel a given draw selects, the
order of equidistant points) the order here is the stable one -- ascending original index among equals.  Random
choices come from a torch.Generator (or are passed in), not from numpy's global RNG.
"""
import copy
import math

import torch

from .. import _lib

_SIGN = -(1 << 63)


def _dev_f32(x):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("ao_amd.ptv2.transform works on CUDA tensors (no CPU fallback)")
    return x.contiguous().float()


class GridSample:
    def __init__(self, grid_size=0.05, hash_type="fnv", mode="train", keys=("coord", "color", "normal", "segment"),
                 return_discrete_coord=False, return_min_coord=False, return_displacement=False,
                 project_displacement=False):
        assert mode in ["train", "test"]
        self.grid_size, self.ravel, self.mode, self.keys = grid_size, hash_type != "fnv", mode, keys
        self.return_discrete_coord, self.return_min_coord = return_discrete_coord, return_min_coord
        self.return_displacement, self.project_displacement = return_displacement, project_displacement

    def _grid(self):
        g = self.grid_size
        g = [float(g)] * 3 if not isinstance(g, (list, tuple)) else [float(v) for v in g]
        assert len(g) == 3
        return g

    def voxelise(self, coord):
        """(idx_sort, start, count, cell - min, min cell): points ordered by voxel key (unsigned, as np.argsort of the
        uint64 keys), run start and length of every voxel."""
        coord = _dev_f32(coord)
        n = coord.shape[0]
        cell = torch.empty((n, 3), dtype=torch.int32, device=coord.device)
        rng = torch.empty(6, dtype=torch.int32, device=coord.device)
        key = torch.empty(n, dtype=torch.int64, device=coord.device)
        g = self._grid()
        rc = _lib.lib().grid_sample_keys_hip_launcher(n, coord.data_ptr(), g[0], g[1], g[2], int(self.ravel), cell.data_ptr(),
                                                      rng.data_ptr(), key.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "grid_sample_keys_hip_launcher")
        skey, idx_sort = torch.sort(key ^ _SIGN, stable=True)  # signed order of key ^ 2^63 == unsigned order of key
        _, count = torch.unique_consecutive(skey, return_counts=True)
        start = torch.cumsum(count, 0) - count
        lo = rng[:3].long()
        return idx_sort, start, count, cell.long() - lo, lo, (skey ^ _SIGN)

    def _extras(self, data_dict, coord, cell, lo):
        out = {}
        g = torch.tensor(self._grid(), dtype=torch.float32, device=coord.device)
        if self.return_min_coord:
            out["min_coord"] = (lo.float() * g).reshape(1, 3)
        if self.return_displacement:
            disp = coord / g - cell.float() - 0.5  # transform.py:822: against the min-shifted cell, as the reference
            if self.project_displacement:
                disp = (disp * data_dict["normal"]).sum(-1, keepdim=True)
            out["displacement"] = disp
        return out

    def __call__(self, data_dict, generator=None, draws=None):
        assert "coord" in data_dict.keys()
        coord = _dev_f32(data_dict["coord"])
        idx_sort, start, count, cell, lo, _ = self.voxelise(coord)
        extras = self._extras(data_dict, coord, cell, lo)
        if self.mode == "train":
            if draws is None:
                # transform.py:805: randint(0, count.max(), count.size) % count
                draws = torch.randint(0, int(count.max()), (count.numel(),), device=coord.device, generator=generator)
            draws = torch.as_tensor(draws, device=coord.device).long()
            idx_unique = idx_sort[start + draws % count]
            if "sampled_index" in data_dict:
                # transform.py:807-815 (ScanNet data-efficient): the labelled points are kept whatever the draw selected; the
                # selection becomes the SORTED union (np.unique) and sampled_index is re-expressed in the new numbering
                sampled = torch.as_tensor(data_dict["sampled_index"], device=coord.device).long()
                idx_unique = torch.unique(torch.cat([idx_unique, sampled]))
                mask = torch.zeros(coord.shape[0], dtype=torch.bool, device=coord.device)
                mask[sampled] = True
                data_dict["sampled_index"] = torch.nonzero(mask[idx_unique]).reshape(-1)
            if self.return_discrete_coord:
                data_dict["discrete_coord"] = cell[idx_unique]
            if self.return_min_coord:
                data_dict["min_coord"] = extras["min_coord"]
            if self.return_displacement:
                data_dict["displacement"] = extras["displacement"][idx_unique]
            for key in self.keys:
                data_dict[key] = data_dict[key][idx_unique]
            return data_dict
        parts = []
        for i in range(int(count.max())):
            idx_part = idx_sort[start + i % count]
            part = dict(index=idx_part)
            if self.return_discrete_coord:
                part["discrete_coord"] = cell[idx_part]
            if self.return_min_coord:
                part["min_coord"] = extras["min_coord"]
            if self.return_displacement:
                data_dict["displacement"] = extras["displacement"][idx_part]  # transform.py:848 writes it to data_dict
            for key in data_dict.keys():
                part[key] = data_dict[key][idx_part] if key in self.keys else data_dict[key]
            parts.append(part)
        return parts


class SphereCrop:
    CROPPED = ("coord", "origin_coord", "discrete_coord", "color", "normal", "segment", "instance", "displacement",
               "strength")  # transform.py:982-999

    def __init__(self, point_max=80000, sample_rate=None, mode="random"):
        assert mode in ["random", "center", "all"]
        self.point_max, self.sample_rate, self.mode = point_max, sample_rate, mode

    @staticmethod
    def dist2(coord, centre):
        """Squared distances of every point to `centre` (3 floats on the device), rounded as numpy's
        np.sum(np.square(coord - centre), 1) (ao_amd/csrc/dataops.hip)."""
        coord = _dev_f32(coord)
        n = coord.shape[0]
        d2 = torch.empty(n, dtype=torch.float32, device=coord.device)
        centre = centre.contiguous().float()
        rc = _lib.lib().center_dist2_hip_launcher(n, coord.data_ptr(), centre.data_ptr(), d2.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "center_dist2_hip_launcher")
        return d2

    @classmethod
    def nearest(cls, coord, centre, point_max):
        """Indices of the point_max points nearest to `centre`, ascending distance."""
        return torch.sort(cls.dist2(coord, centre), stable=True)[1][:point_max]

    PART_KEYS = ("coord", "discrete_coord", "normal", "color", "displacement", "strength")  # transform.py:933-948

    def _all(self, data_dict, point_max, generator, priority):
        """mode="all" (transform.py:914-968): overlapping crops of point_max points until every point is in one.  Each crop is
        centred on the point of lowest priority; a crop raises the priority of its members by (1 - d2 / max d2)^2."""
        coord = _dev_f32(data_dict["coord"])
        n = coord.shape[0]
        if "index" not in data_dict.keys():
            data_dict["index"] = torch.arange(n, device=coord.device)
        if n <= point_max:
            part = dict(data_dict)
            part["weight"] = torch.zeros(n, dtype=torch.float64, device=coord.device)
            part["index"] = data_dict["index"]
            return [part]
        if priority is None:  # np.random.rand(n) * 1e-3
            priority = torch.rand(n, dtype=torch.float64, device=coord.device, generator=generator) * 1e-3
        coord_p = torch.as_tensor(priority, device=coord.device).double().clone()
        covered = torch.zeros(n, dtype=torch.bool, device=coord.device)
        parts = []
        while not bool(covered.all()):
            init_idx = torch.argmin(coord_p)
            d2 = self.dist2(coord, coord[init_idx])
            idx_crop = torch.sort(d2, stable=True)[1][:point_max]
            part = {key: data_dict[key][idx_crop] for key in self.PART_KEYS if key in data_dict.keys()}
            part["weight"] = d2[idx_crop]
            part["index"] = data_dict["index"][idx_crop]
            parts.append(part)
            w = part["weight"]  # (fp32 arithmetic, as numpy's on the fp32 distances; the priorities are fp64)
            coord_p[idx_crop] += torch.square(1 - w / w.max()).double()
            covered[idx_crop] = True
        return parts

    def __call__(self, data_dict, generator=None, center_index=None, priority=None):
        assert "coord" in data_dict.keys()
        n = data_dict["coord"].shape[0]
        point_max = int(self.sample_rate * n) if self.sample_rate is not None else self.point_max
        if self.mode == "all":
            return self._all(data_dict, point_max, generator, priority)
        return self._one(data_dict, n, point_max, generator, center_index)

    def _one(self, data_dict, n, point_max, generator, center_index):
        if n <= point_max:
            return data_dict
        coord = _dev_f32(data_dict["coord"])
        if center_index is None:
            center_index = (torch.randint(0, n, (1,), device=coord.device, generator=generator)[0] if self.mode == "random"
                            else n // 2)
        idx_crop = self.nearest(coord, coord[center_index], point_max)
        for key in self.CROPPED:
            if key in data_dict.keys():
                data_dict[key] = data_dict[key][idx_crop]
        return data_dict


class Collect:
    def __init__(self, keys, offset_keys_dict=None, **kwargs):
        self.keys = [keys] if isinstance(keys, str) else keys
        self.offset_keys = dict(offset="coord") if offset_keys_dict is None else offset_keys_dict
        self.kwargs = kwargs

    def __call__(self, data_dict):
        data = {key: data_dict[key] for key in self.keys}
        for key, value in self.offset_keys.items():
            data[key] = torch.tensor([data_dict[value].shape[0]])
        for name, keys in self.kwargs.items():
            data[name.replace("_keys", "")] = torch.cat([data_dict[key].float() for key in keys], dim=1)
        return data


class CenterShift:
    def __init__(self, apply_z=True):
        self.apply_z = apply_z

    def __call__(self, data_dict):
        if "coord" in data_dict.keys():
            coord = data_dict["coord"]
            lo, hi = coord.min(dim=0)[0], coord.max(dim=0)[0]
            shift = torch.stack([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, lo[2] if self.apply_z else torch.zeros_like(lo[2])])
            data_dict["coord"] = coord - shift
        return data_dict


class NormalizeColor:
    def __call__(self, data_dict):
        if "color" in data_dict.keys():
            color = data_dict["color"]
            # (a tensor divisor: with a python scalar torch multiplies by the rounded reciprocal on the GPU, 1 ulp off
            # numpy's IEEE division)
            data_dict["color"] = color / torch.full((1,), 127.5, dtype=color.dtype, device=color.device) - 1
        return data_dict


def _uniform(lo, hi, size, generator):
    """np.random.uniform(lo, hi, size) from a torch.Generator: float64 on the host; lo == hi gives lo exactly"""
    return float(lo) + (float(hi) - float(lo)) * torch.rand(size, dtype=torch.float64, generator=generator)


class RandomScale:
    def __init__(self, scale=None, anisotropic=False):
        self.scale = scale if scale is not None else [0.95, 1.05]
        self.anisotropic = anisotropic

    def __call__(self, data_dict, generator=None, scale=None):
        if "coord" in data_dict.keys():
            if scale is None:
                scale = _uniform(self.scale[0], self.scale[1], 3 if self.anisotropic else 1, generator)
            coord = data_dict["coord"]
            scale = torch.as_tensor(scale, dtype=torch.float64).to(coord.device)
            data_dict["coord"] = (coord.double() * scale).to(coord.dtype)  # a float64 product rounded once, as numpy's *=
        return data_dict


class RandomFlip:
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, data_dict, generator=None, draws=None):
        if draws is None:
            draws = torch.rand(2, dtype=torch.float64, generator=generator).tolist()
        for axis, u in enumerate(draws):
            if u < self.p:
                for key in ("coord", "normal"):
                    if key in data_dict.keys():
                        v = data_dict[key].clone()
                        v[:, axis] = -v[:, axis]
                        data_dict[key] = v
        return data_dict


class RandomRotateTargetAngle:
    def __init__(self, angle=(1 / 2, 1, 3 / 2), center=None, axis="z", always_apply=False, p=0.75):
        self.angle, self.axis, self.always_apply, self.center = angle, axis, always_apply, center
        self.p = p if not always_apply else 1

    def matrix(self, angle):
        """rot_t of transform.py:260-266 for `angle` (in units of pi), float64"""
        a = angle * math.pi
        c, s = math.cos(a), math.sin(a)
        if self.axis == "x":
            rows = [[1, 0, 0], [0, c, -s], [0, s, c]]
        elif self.axis == "y":
            rows = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        elif self.axis == "z":
            rows = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        else:
            raise NotImplementedError
        return torch.tensor(rows, dtype=torch.float64)

    def __call__(self, data_dict, generator=None, angle=None):
        if float(torch.rand((), dtype=torch.float64, generator=generator)) > self.p:
            return data_dict
        if angle is None:
            angle = self.angle[int(torch.randint(0, len(self.angle), (), generator=generator))]
        if "coord" in data_dict.keys():
            coord = data_dict["coord"]
            rot = self.matrix(angle).to(coord.device)
            if self.center is None:
                centre = (coord.min(dim=0)[0] + coord.max(dim=0)[0]) / 2  # fp32, as the reference's scalars
            else:
                centre = torch.tensor([float(v) for v in self.center], dtype=torch.float64, device=coord.device)
            moved = (coord.double() - centre.double()).to(coord.dtype)  # `coord -= center` rounds to fp32 in place
            data_dict["coord"] = (moved.double() @ rot.t() + centre.double()).to(coord.dtype)
        if "normal" in data_dict.keys():
            normal = data_dict["normal"]
            data_dict["normal"] = (normal.double() @ self.matrix(angle).to(normal.device).t()).to(normal.dtype)
        return data_dict


class ToTensor:
    """The data is tensors already: a pass-through (numpy arrays, which the reference converts here, are converted too)."""

    def __call__(self, data):
        if torch.is_tensor(data) or isinstance(data, str):
            return data
        if isinstance(data, dict):
            return {k: self(v) for k, v in data.items()}
        if isinstance(data, (list, tuple)):
            return [self(v) for v in data]
        if isinstance(data, int):
            return torch.tensor([data], dtype=torch.int64)
        if isinstance(data, float):
            return torch.tensor([data], dtype=torch.float32)
        t = torch.as_tensor(data)
        return t.float() if t.is_floating_point() else (t if t.dtype == torch.bool else t.long())


def build_transform(cfg):
    """`TRANSFORMS.build(cfg)` against this module's classes: dict(type="GridSample", ...) -> GridSample(...)."""
    args = dict(cfg)
    kind = args.pop("type")
    cls = _TRANSFORMS.get(kind)
    if cls is None:
        raise KeyError("%s is not a transform of ao_amd.ptv2.transform (%s)" % (kind, sorted(_TRANSFORMS)))
    return cls(**args)


class Compose:
    def __init__(self, cfg=None):
        self.cfg = cfg if cfg is not None else []
        self.transforms = [t if callable(t) else build_transform(t) for t in self.cfg]

    def __call__(self, data_dict):
        for t in self.transforms:
            data_dict = t(data_dict)
        return data_dict


def test_fragments(data_dict, test_cfg, transform=None):
    """S3DISDataset.prepare_test_data (datasets/s3dis.py:212-236) on device tensors: `dict(fragment_list, segment, name)`.
    data_dict: coord (+ color, normal), segment, optional name; test_cfg: the config's own dict (voxelize, crop,
    post_transform, aug_transform), its `type=` entries resolved against this module; transform: the dataset's base
    transform as a list of configs or a callable."""
    get = (lambda k: test_cfg.get(k)) if isinstance(test_cfg, dict) else (lambda k: getattr(test_cfg, k, None))
    data_dict = dict(data_dict)
    segment = data_dict.pop("segment")
    name = data_dict.pop("name", "scene")
    if transform is not None:
        data_dict = (transform if callable(transform) else Compose(transform))(data_dict)
    voxelize = build_transform(get("voxelize"))
    crop = build_transform(get("crop")) if get("crop") else None
    post = Compose(get("post_transform"))
    fragment_list = []
    for aug in get("aug_transform"):
        data = Compose(aug)(copy.deepcopy(data_dict))
        for part in voxelize(data):
            fragment_list += crop(part) if crop is not None else [part]
    return dict(fragment_list=[post(part) for part in fragment_list], segment=segment, name=name)


test_fragments.__test__ = False  # (a library function, not a pytest case, whatever module imports it)

_TRANSFORMS = dict(GridSample=GridSample, SphereCrop=SphereCrop, Collect=Collect, CenterShift=CenterShift,
                   NormalizeColor=NormalizeColor, RandomScale=RandomScale, RandomFlip=RandomFlip,
                   RandomRotateTargetAngle=RandomRotateTargetAngle, ToTensor=ToTensor)


def point_collate(batch):
    """datasets/utils.py:14-54 for a list of Collect()-ed dicts: tensors concatenated along dim 0, every '*offset*'
    entry turned into the running end index (int32 on the coord's device, what pointops expects)."""
    out = {}
    for key in batch[0]:
        vals = [d[key] for d in batch]
        if torch.is_tensor(vals[0]):
            out[key] = torch.cat(vals)
        else:
            out[key] = list(vals)
    dev = out["coord"].device if "coord" in out else None
    host = {}
    for key in out:
        if "offset" in key and torch.is_tensor(out[key]):
            ends = torch.cumsum(out[key], dim=0).int()
            if not ends.is_cuda:  # Collect() makes the counts on the host: keep the bounds there too, so that callers
                host[key + "_host"] = ends.tolist()  # that slice per scene (DefaultSegmentorSAM_Image) need no read-back
            out[key] = ends.to(dev)
    out.update(host)
    return out
