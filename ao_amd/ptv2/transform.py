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

The training augmentations (Copy :54, RandomShift :146, PointClip :160, RandomRotate :209, RandomJitter :319,
ChromaticAutoContrast :358, ChromaticTranslation :379, ChromaticJitter :392, RandomColorDrop :692, ElasticDistortion :709,
ShufflePoint :1002) and the Mix3D switch of the collate (datasets/utils.py:43-54) are here as well.  The per-point ones do
not compute in torch: each class describes itself as step records (`steps(draws)`), `fuse_plan` turns the records of one or
of many consecutive transforms into segments of a program (include/ptv2_data_hip.h), and ao_amd/csrc/augment.hip runs a
segment once per point in one kernel.  Calling a class on its own runs a one-transform program through the same kernel.
A tensor's dtype is the reference's array dtype: `coord` is float32 until the first applied rotation (or PointClip) and
float64 afterwards, so a class called alone on a float32 coord returns what numpy returns, float64 included;
`Compose(cfg, fuse=True)` carries float64 between its segments and rounds to float32 once at the end of each run of
per-point transforms.  Every host-side random decision (gate, angle, scale, blend, translation, permutation) comes from a
torch.Generator or is passed by keyword; per-point normals come from a 64-bit `seed` (in-kernel Philox4x32-10, counter =
point index and the step's stream number) or from a `noise=` tensor.

Not here, on purpose: RandomDropout, HueSaturationTranslation, RandomColorGrayScale (commented out in every PT-v2m2 config, or
active only in one ScanNet list with a ratio the data-efficient benchmarks use), NormalizeCoord, PositiveShift and CropBoundary,
which belong to other model families.

ContrastiveViewsGenerator (:1046-1067) and RandomColorJitter (:440-630) are here for Masked Scene Contrast (ao_amd/msc): with
them `Compose(cfg)` builds the whole transform list of both MSC-v1m1 ScanNet configs.  RandomColorJitter is plain torch on the
device, one tensor operation per numpy operation of the reference and in the dtype numpy gives that operation (the hue path is
float64 from the saturation on, as `maxc * (1 - eqc)` multiplies a float32 array by an int64 one): brightness, saturation and
hue equal the numpy results bit for bit, contrast to the order of its one mean.

`pair_views` is ScanNetPairDataset.prepare_train_data (datasets/scannet_pair.py:70-80) for the MSC-v1m2 (CSC) config, whose two
views come from two frames of a scene and go through a transform list each.

InstanceParser (:1071-1104) is here for PointGroup (ao_amd/pointgroup): torch segment reductions on whatever device the data
is on instead of the reference's loop over the instances.
"""
import copy
import ctypes
import inspect
import math
import numbers

import torch

from .. import _abi, _lib

_SIGN = -(1 << 63)
_K = _abi.data_consts


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

    def draw(self, generator=None):
        return {}

    def steps(self, draws=None):
        return [dict(kind=_K["PTV2_AUG_CENTER_SHIFT"], flags=_K["PTV2_AUG_FLAG_APPLY_Z"] if self.apply_z else 0, bounds="coord")]


class NormalizeColor:
    def __call__(self, data_dict):
        if "color" in data_dict.keys():
            color = data_dict["color"]
            # (a tensor divisor: with a python scalar torch multiplies by the rounded reciprocal on the GPU, 1 ulp off
            # numpy's IEEE division)
            data_dict["color"] = color / torch.full((1,), 127.5, dtype=color.dtype, device=color.device) - 1
        return data_dict


class InstanceParser:
    """`instance` renumbered 0 .. I - 1 in ascending order of the original ids over the points whose `segment` is not ignored
    (the others get instance_ignore_index); `instance_center` (n, 3): the mean coordinate of a point's instance, the ignore
    value on ignored rows; `bbox` (I, 6): minimum and maximum coordinate per instance.  The mean is summed in float64 and
    returned in coord's dtype (the reference sums fp32 and stores into a float64 array)."""

    def __init__(self, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1):
        self.segment_ignore_index = segment_ignore_index
        self.instance_ignore_index = instance_ignore_index

    def __call__(self, data_dict):
        coord, segment, instance = data_dict["coord"], data_dict["segment"], data_dict["instance"]
        mask = torch.ones_like(segment, dtype=torch.bool)
        for index in self.segment_ignore_index:
            mask &= segment != index
        unique, inverse = torch.unique(instance[mask], return_inverse=True)
        count = unique.numel()
        instance = torch.full_like(instance, self.instance_ignore_index)
        instance[mask] = inverse.to(instance.dtype)
        kept = coord[mask]
        rows = inverse[:, None].expand(-1, 3)
        total = torch.zeros((count, 3), dtype=torch.float64, device=coord.device).index_add_(0, inverse, kept.double())
        members = torch.bincount(inverse, minlength=count).double()
        mean = (total / members[:, None]).to(coord.dtype)
        lo = torch.full((count, 3), float("inf"), dtype=coord.dtype, device=coord.device).scatter_reduce_(0, rows, kept, "amin")
        hi = torch.full((count, 3), float("-inf"), dtype=coord.dtype, device=coord.device).scatter_reduce_(0, rows, kept, "amax")
        center = torch.full((coord.shape[0], 3), float(self.instance_ignore_index), dtype=coord.dtype, device=coord.device)
        center[mask] = mean[inverse]
        data_dict["instance"] = instance
        data_dict["instance_center"] = center
        data_dict["bbox"] = torch.cat([lo, hi], 1)
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

    def draw(self, generator=None):
        return dict(scale=_uniform(self.scale[0], self.scale[1], 3 if self.anisotropic else 1, generator).tolist())

    def steps(self, draws):
        s = [float(v) for v in torch.as_tensor(draws["scale"], dtype=torch.float64).reshape(-1).tolist()]
        return [dict(kind=_K["PTV2_AUG_SCALE"], p=s * 3 if len(s) == 1 else s)]


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

    def draw(self, generator=None):
        return dict(draws=torch.rand(2, dtype=torch.float64, generator=generator).tolist())

    def steps(self, draws):
        sign = [-1.0 if u < self.p else 1.0 for u in draws["draws"]] + [1.0]
        return [dict(kind=_K["PTV2_AUG_SCALE"], p=sign, normal=True)] if -1.0 in sign else []


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

    def draw(self, generator=None):
        gate = float(torch.rand((), dtype=torch.float64, generator=generator))
        if gate > self.p:
            return dict(gate=gate, angle=None)
        return dict(gate=gate, angle=self.angle[int(torch.randint(0, len(self.angle), (), generator=generator))])

    def steps(self, draws):
        if draws["gate"] > self.p:
            return []
        step = dict(kind=_K["PTV2_AUG_ROTATE"], p=self.matrix(draws["angle"]).reshape(-1).tolist(), normal=True)
        if self.center is None:
            return [dict(step, flags=_K["PTV2_AUG_FLAG_BOUNDS_CENTER"], bounds="coord", p=step["p"] + [0.0] * 3)]
        return [dict(step, p=step["p"] + [float(v) for v in self.center])]


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
    missing = [name for name, p in inspect.signature(cls).parameters.items()
               if p.default is p.empty and p.kind == p.POSITIONAL_OR_KEYWORD and name not in args]
    if missing:  # a config that leaves out a key its class needs is a KeyError too, naming the key
        raise KeyError("%s needs the config key(s) %s" % (kind, ", ".join(missing)))
    return cls(**args)


class Compose:
    """fuse=False: the transforms one after the other, as the reference's Compose.  fuse=True: every run of consecutive
    per-point transforms (those with `steps`) becomes one program (`fuse_plan`), carried in float64 between its segments and
    rounded to float32 at its end; the other transforms (GridSample, SphereCrop, ShufflePoint, Copy, NormalizeColor,
    ToTensor, Collect) run between the programs as they do unfused.  The host-side decisions (gates, angles, the seed of
    the per-point normals, ShufflePoint's permutation) come from `generator`; GridSample and SphereCrop draw on the device
    and take `device_generator` (a CUDA generator; None: torch's global one)."""

    def __init__(self, cfg=None, fuse=False, generator=None, device_generator=None):
        self.cfg = cfg if cfg is not None else []
        self.fuse, self.generator, self.device_generator = fuse, generator, device_generator
        self.transforms = [t if callable(t) else build_transform(self._views_cfg(t)) for t in self.cfg]

    def _views_cfg(self, cfg):
        """a ContrastiveViewsGenerator named by a config entry runs its inner list as this Compose runs its own"""
        if cfg.get("type") != "ContrastiveViewsGenerator":
            return cfg
        return dict(dict(fuse=self.fuse, generator=self.generator, device_generator=self.device_generator), **cfg)

    def groups(self):
        """[(is a per-point run, [indices into self.transforms])]"""
        out = []
        for i, t in enumerate(self.transforms):
            pointwise = hasattr(t, "steps")
            if pointwise and out and out[-1][0]:
                out[-1][1].append(i)
            else:
                out.append((pointwise, [i]))
        return out

    def draw(self):
        """one draw per transform (None for those that are not per-point) and the seed of the per-point normals"""
        seed = int(torch.randint(0, 1 << 62, (), generator=self.generator))
        return dict(seed=seed, per=[t.draw(self.generator) if hasattr(t, "steps") else None for t in self.transforms])

    def records(self, indices, draws):
        out = []
        for i in indices:
            for rec in self.transforms[i].steps(draws["per"][i]):
                out.append(dict(rec, stream=_STREAMS * i + rec.get("stream", 0)))
        return out

    def plan(self, draws, in_f64=False):
        """the segments of every per-point run for these draws: host only"""
        return [fuse_plan(self.records(idx, draws), in_f64=in_f64, final_round=True) for pointwise, idx in self.groups() if pointwise]

    def __call__(self, data_dict, draws=None):
        if not self.fuse:
            for t in self.transforms:
                data_dict = t(data_dict)
            return data_dict
        if draws is None:
            draws = self.draw()
        for pointwise, idx in self.groups():
            if pointwise:
                data_dict = _run_records(self.records(idx, draws), data_dict, draws["seed"], final_round=True)
                continue
            t = self.transforms[idx[0]]
            g = self.generator if isinstance(t, (ShufflePoint, RandomColorJitter)) else self.device_generator
            takes = g is not None and "generator" in inspect.signature(t.__call__).parameters
            data_dict = t(data_dict, generator=g) if takes else t(data_dict)
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

# ------------------------------------------------------------------------------------------ training augmentations --
_STREAMS = 8  # RNG stream numbers per transform of a list: transform i owns [8 i, 8 i + 8)
_COORD_KINDS = tuple(_K[k] for k in ("PTV2_AUG_CENTER_SHIFT", "PTV2_AUG_ROTATE", "PTV2_AUG_SCALE", "PTV2_AUG_SHIFT",
                                     "PTV2_AUG_CLIP", "PTV2_AUG_JITTER", "PTV2_AUG_ELASTIC"))
_TO_F64 = (_K["PTV2_AUG_ROTATE"], _K["PTV2_AUG_CLIP"])  # np.dot / np.clip with list bounds return a float64 array
_NOISE_KINDS = (_K["PTV2_AUG_JITTER"], _K["PTV2_AUG_COLOR_JITTER"])
_ROUND = _K["PTV2_AUG_ROUND_F32"]


def fuse_plan(records, in_f64=False, final_round=False):
    """Step records -> segments of one program each: [dict(bounds=bool, readback=bool, steps=[...], out_f64=bool)].
    Host only.  The reference's rounding is written in: while its `coord` array is float32, every coordinate step is
    followed by a ROUND_F32 step and centres are computed in fp32 (FLAG_FP32); a rotation or a clip makes the array
    float64 and the rounds stop.  A step that reads bounds of the current state which an earlier step of the segment has
    changed ends the segment (a bounds launch goes in front of the next); an elastic step always does, because the host
    reads the bounds back to size its noise grid.  final_round: a last ROUND_F32 and a float32 result."""
    f32 = not in_f64
    stale = dict(coord=True, color=True)
    segs = [dict(bounds=False, readback=False, steps=[])]
    for rec in records:
        kind, need = rec["kind"], rec.get("bounds")
        elastic = kind == _K["PTV2_AUG_ELASTIC"]
        cur = segs[-1]
        if elastic or (need and stale[need]) or len(cur["steps"]) + 3 > _K["PTV2_AUG_MAX_STEPS"]:
            if cur["steps"]:
                cur = dict(bounds=False, readback=False, steps=[])
                segs.append(cur)
            if need:
                cur["bounds"], cur["readback"] = True, cur["readback"] or elastic
                stale = dict(coord=False, color=False)
        step = {k: v for k, v in rec.items() if k not in ("bounds", "normal")}
        step["flags"] = rec.get("flags", 0) | (_K["PTV2_AUG_FLAG_FP32"] if f32 and kind in _COORD_KINDS else 0)
        cur["steps"].append(step)
        if kind in _COORD_KINDS:
            stale["coord"] = True
            f32 = f32 and kind not in _TO_F64
            if f32:
                cur["steps"].append(dict(kind=_ROUND, flags=0))
        else:
            stale["color"] = True
    if final_round and not f32 and segs[-1]["steps"]:
        segs[-1]["steps"].append(dict(kind=_ROUND, flags=0))
    segs = [s for s in segs if s["steps"]]
    for i, seg in enumerate(segs):
        seg["out_f64"] = i + 1 < len(segs) or not (f32 or final_round)
    return segs


def elastic_grid(lo, hi, fp32, granularity):
    """(noise_dim, axis start, axis spacing) of ElasticDistortion's noise grid for the bounding box lo..hi, with the dtypes
    of transform.py:726-752: on a float32 array the extent, its floor division and `coords_min - granularity` are float32."""
    import numpy as np

    dtype = np.float32 if fp32 else np.float64
    lo, hi = np.asarray(lo, dtype), np.asarray(hi, dtype)
    dims = ((hi - lo) // dtype(granularity)).astype(int) + 3
    start = (lo - dtype(granularity)).astype(np.float64)
    stop = lo.astype(np.float64) + granularity * (dims - 2)
    return [int(d) for d in dims], start.tolist(), ((stop - start) / (dims - 1)).tolist()


def _blurred_field(dims, grid, seed, stream):
    """the smoothed noise grid: normals (given, or the kernel's own for `stream`), blurred x, y, z, x, y, z"""
    L, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    cells = dims[0] * dims[1] * dims[2]
    if grid is None:
        a = torch.empty((cells, 3), dtype=torch.float32, device=dev)
        _lib.check(L.aug_noise_hip_launcher(cells, seed, stream, a.data_ptr(), _lib.stream_ptr()), "aug_noise_hip_launcher")
    else:
        if callable(grid):  # (the grid's size is known only here)
            grid = grid(dims)
        if tuple(grid.shape) != (dims[0], dims[1], dims[2], 3):
            raise ValueError("ElasticDistortion: the noise grid is %s here, the given one %s" % (tuple(dims) + (3,), tuple(grid.shape)))
        a = _dev_f32(grid).clone()
    b = torch.empty_like(a)
    for axis in (0, 1, 2, 0, 1, 2):
        _lib.check(L.aug_blur3_hip_launcher(dims[0], dims[1], dims[2], axis, a.data_ptr(), b.data_ptr(), _lib.stream_ptr()),
                   "aug_blur3_hip_launcher")
        a, b = b, a
    return a


def aug_bounds(coord, color=None):
    """per-axis (min, max) of coord and colour on the device: 24 doubles, [0:6] coord, [6:12] colour, the rest scratch"""
    out = torch.empty(24, dtype=torch.float64, device=coord.device)
    rc = _lib.lib().aug_bounds_hip_launcher(coord.shape[0], coord.data_ptr(), int(coord.dtype == torch.float64), _lib.ptr(color),
                                            out.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "aug_bounds_hip_launcher")
    return out


def _run_segments(segs, coord, color, seed):
    """coord (n, 3) float32 / float64 and colour (n, 3) float32 or None through the segments of one plan"""
    L = _lib.lib()
    n = coord.shape[0]
    if n == 0:
        return coord, color
    Program, keep = _abi.data_structs["ptv2_aug_program"], []
    for seg in segs:
        bounds = aug_bounds(coord, color) if seg["bounds"] else None
        host = bounds[:6].tolist() if seg["readback"] else None  # the one host read-back: an elastic grid's size
        prog = Program()
        prog.count, prog.coord_in_f64, prog.coord_out_f64 = len(seg["steps"]), int(coord.dtype == torch.float64), int(seg["out_f64"])
        planes, colour_steps = [], False
        for s, step in zip(prog.step, seg["steps"]):
            s.kind, s.flags, s.stream = step["kind"], step["flags"], step.get("stream", 0)
            p = list(step.get("p", ()))
            if step["kind"] == _K["PTV2_AUG_ELASTIC"]:
                dims, start, spacing = elastic_grid(host[:3], host[3:], bool(step["flags"] & _K["PTV2_AUG_FLAG_FP32"]), step["granularity"])
                field = _blurred_field(dims, step.get("grid"), seed, s.stream)
                keep.append(field)
                s.field, s.dims[0], s.dims[1], s.dims[2] = field.data_ptr(), dims[0], dims[1], dims[2]
                p = start + spacing + [float(step["magnitude"])]
            for j, v in enumerate(p):
                s.p[j] = v
            colour_steps = colour_steps or step["kind"] >= _K["PTV2_AUG_COLOR_CONTRAST"]
            if step["kind"] in _NOISE_KINDS:
                s.slot = len(planes)
                planes.append(step.get("noise"))
        noise = None
        if any(p is not None for p in planes):  # given normals; a step without them gets the kernel's own, as a plane
            noise = torch.empty((len(planes), n, 3), dtype=torch.float32, device=coord.device)
            for j, (plane, step) in enumerate(zip(planes, [s for s in seg["steps"] if s["kind"] in _NOISE_KINDS])):
                if plane is not None:
                    noise[j] = _dev_f32(plane).reshape(n, 3)
                else:
                    _lib.check(L.aug_noise_hip_launcher(n, seed, step.get("stream", 0), noise[j].data_ptr(), _lib.stream_ptr()),
                               "aug_noise_hip_launcher")
        if colour_steps and color is None:
            raise KeyError("a colour augmentation needs data_dict['color']")
        out = torch.empty((n, 3), dtype=torch.float64 if seg["out_f64"] else torch.float32, device=coord.device)
        color_out = torch.empty_like(color) if colour_steps else None
        rc = L.aug_points_hip_launcher(n, ctypes.addressof(prog), _lib.ptr(bounds), coord.data_ptr(),
                                       color.data_ptr() if colour_steps else 0, _lib.ptr(noise), seed, out.data_ptr(),
                                       _lib.ptr(color_out), _lib.stream_ptr())
        _lib.check(rc, "aug_points_hip_launcher")
        coord, color = out, (color_out if colour_steps else color)
    return coord, color


def _point_tensor(x):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("ao_amd.ptv2.transform works on CUDA tensors (no CPU fallback)")
    return x.contiguous() if x.dtype == torch.float64 else x.contiguous().float()


def _run_records(records, data_dict, seed, final_round=False):
    """the records' program on data_dict's coord and colour; rotations and flips also on its normal"""
    colour = any(r["kind"] >= _K["PTV2_AUG_COLOR_CONTRAST"] for r in records) and "color" in data_dict.keys()
    main = [r for r in records if "coord" in data_dict.keys() or r["kind"] >= _K["PTV2_AUG_COLOR_CONTRAST"]]
    if "coord" in data_dict.keys():
        coord = _point_tensor(data_dict["coord"])
        segs = fuse_plan([r for r in main if colour or r["kind"] < _K["PTV2_AUG_COLOR_CONTRAST"]], coord.dtype == torch.float64, final_round)
        coord, color = _run_segments(segs, coord, _dev_f32(data_dict["color"]) if colour else None, seed)
        data_dict["coord"] = coord
        if colour:
            data_dict["color"] = color
    elif colour:
        raise KeyError("the colour augmentations run in the point program, which needs data_dict['coord']")
    turns = [dict(r, p=r["p"][:9] + [0.0] * 3, flags=0, bounds=None) if r["kind"] == _K["PTV2_AUG_ROTATE"] else r
             for r in records if r.get("normal")]
    if turns and "normal" in data_dict.keys():
        normal = _point_tensor(data_dict["normal"])
        data_dict["normal"] = _run_segments(fuse_plan(turns, normal.dtype == torch.float64, final_round), normal, None, seed)[0]
    return data_dict


class _PointTransform:
    """A per-point augmentation: `draw(generator)` makes its host-side random decisions, `steps(draws)` states what they
    mean as step records, and a call on its own runs those records as a program of their own."""

    def draw(self, generator=None):
        return {}

    def __call__(self, data_dict, generator=None, seed=None, stream=0, **draws):
        drawn = dict(self.draw(generator), **draws)
        if seed is None:
            seed = int(torch.randint(0, 1 << 62, (), generator=generator))
        records = [dict(r, stream=stream + r.get("stream", 0)) for r in self.steps(drawn)]
        return _run_records(records, data_dict, seed)


class Copy:
    def __init__(self, keys_dict=None):
        self.keys_dict = dict(coord="origin_coord", segment="origin_segment") if keys_dict is None else keys_dict

    def __call__(self, data_dict):
        for key, value in self.keys_dict.items():
            v = data_dict[key]
            data_dict[value] = v.clone().detach() if torch.is_tensor(v) else copy.deepcopy(v)
        return data_dict


class ShufflePoint:
    KEYS = ("coord", "discrete_coord", "displacement", "color", "normal", "segment", "instance")  # transform.py:1007-1020

    def __call__(self, data_dict, generator=None, perm=None):
        assert "coord" in data_dict.keys()
        n = data_dict["coord"].shape[0]
        if perm is None:
            perm = torch.randperm(n, generator=generator)
        perm = torch.as_tensor(perm).long().to(data_dict["coord"].device)
        for key in self.KEYS:
            if key in data_dict.keys():
                data_dict[key] = data_dict[key][perm]
        return data_dict


class RandomRotate(_PointTransform):
    matrix = RandomRotateTargetAngle.matrix

    def __init__(self, angle=None, center=None, axis="z", always_apply=False, p=0.5):
        self.angle = [-1, 1] if angle is None else angle
        self.axis, self.always_apply, self.center = axis, always_apply, center
        self.p = p if not always_apply else 1

    def draw(self, generator=None):
        gate = float(torch.rand((), dtype=torch.float64, generator=generator))
        if gate > self.p:  # transform.py:218: `random.random() > self.p` skips
            return dict(gate=gate, angle=None)
        return dict(gate=gate, angle=float(_uniform(self.angle[0], self.angle[1], (), generator)))

    steps = RandomRotateTargetAngle.steps


class RandomShift(_PointTransform):
    def __init__(self, shift=((-0.2, 0.2), (-0.2, 0.2), (0, 0))):
        self.shift = shift

    def draw(self, generator=None):
        return dict(shift=[float(_uniform(lo, hi, (), generator)) for lo, hi in self.shift])

    def steps(self, draws):
        return [dict(kind=_K["PTV2_AUG_SHIFT"], p=[float(v) for v in draws["shift"]])]


class PointClip(_PointTransform):
    def __init__(self, point_cloud_range=(-80, -80, -3, 80, 80, 1)):
        self.point_cloud_range = point_cloud_range

    def steps(self, draws=None):
        return [dict(kind=_K["PTV2_AUG_CLIP"], p=[float(v) for v in self.point_cloud_range])]


class RandomJitter(_PointTransform):
    def __init__(self, sigma=0.01, clip=0.05):
        assert clip > 0
        self.sigma, self.clip = sigma, clip

    def draw(self, generator=None):
        return dict(noise=None)

    def steps(self, draws):
        return [dict(kind=_K["PTV2_AUG_JITTER"], p=[float(self.sigma), float(self.clip)], noise=draws.get("noise"))]


class ElasticDistortion(_PointTransform):
    """distortion_params has to be named (every config of the reference names it; None selects the reference's default
    pairs): a bare dict(type="ElasticDistortion") stays the KeyError it has always been in this module."""

    def __init__(self, distortion_params):
        self.distortion_params = [[0.2, 0.4], [0.8, 1.6]] if distortion_params is None else distortion_params

    def draw(self, generator=None):
        return dict(gate=float(torch.rand((), dtype=torch.float64, generator=generator)), grids=None)

    def steps(self, draws):
        """grids: the normals of each pair's noise grid, (dx, dy, dz, 3) fp32 (or a callable that makes them for the
        dims it is given), instead of the kernel's own"""
        if self.distortion_params is None or not draws["gate"] < 0.95:
            return []
        grids = draws.get("grids") or [None] * len(self.distortion_params)
        return [dict(kind=_K["PTV2_AUG_ELASTIC"], bounds="coord", granularity=float(g), magnitude=float(m), grid=grid, stream=1 + k)
                for k, ((g, m), grid) in enumerate(zip(self.distortion_params, grids))]


class ChromaticAutoContrast(_PointTransform):
    def __init__(self, p=0.2, blend_factor=None):
        self.p, self.blend_factor = p, blend_factor

    def draw(self, generator=None):
        gate = float(torch.rand((), dtype=torch.float64, generator=generator))
        blend = self.blend_factor
        if gate < self.p and blend is None:
            blend = float(torch.rand((), dtype=torch.float64, generator=generator))
        return dict(gate=gate, blend=blend)

    def steps(self, draws):
        if not draws["gate"] < self.p:
            return []
        blend = float(self.blend_factor if draws.get("blend") is None else draws["blend"])  # (a python scalar against a float32 array: both factors are rounded to fp32)
        return [dict(kind=_K["PTV2_AUG_COLOR_CONTRAST"], p=[1 - blend, blend], bounds="color")]


class ChromaticTranslation(_PointTransform):
    def __init__(self, p=0.95, ratio=0.05):
        self.p, self.ratio = p, ratio

    def draw(self, generator=None):
        gate = float(torch.rand((), dtype=torch.float64, generator=generator))
        return dict(gate=gate, uniform=torch.rand(3, dtype=torch.float64, generator=generator).tolist() if gate < self.p else None)

    def steps(self, draws):
        if not draws["gate"] < self.p:
            return []
        return [dict(kind=_K["PTV2_AUG_COLOR_TRANSLATE"], p=[(float(u) - 0.5) * 255 * 2 * self.ratio for u in draws["uniform"]])]


class ChromaticJitter(_PointTransform):
    def __init__(self, p=0.95, std=0.005):
        self.p, self.std = p, std

    def draw(self, generator=None):
        return dict(gate=float(torch.rand((), dtype=torch.float64, generator=generator)), noise=None)

    def steps(self, draws):
        if not draws["gate"] < self.p:
            return []
        return [dict(kind=_K["PTV2_AUG_COLOR_JITTER"], p=[self.std * 255], noise=draws.get("noise"))]


class RandomColorDrop(_PointTransform):
    def __init__(self, p=0.2, color_augment=0.0):
        self.p, self.color_augment = p, color_augment

    def draw(self, generator=None):
        return dict(gate=float(torch.rand((), dtype=torch.float64, generator=generator)))

    def steps(self, draws):
        return [dict(kind=_K["PTV2_AUG_COLOR_MUL"], p=[float(self.color_augment)])] if draws["gate"] < self.p else []


class RandomColorJitter:
    """transform.py:440-630 on a float32 `color` in [0, 255].  The host-side decisions come from `generator` in the reference's
    get_params order -- the order of the four adjustments (torch.randperm(4)), then the brightness, contrast, saturation and hue
    factor of those that are switched on -- followed by one gate per adjustment that is reached, in application order; or
    from `draws` = dict(order=(4 ints), factors=(b, c, s, h; None where switched off), gates=(4 floats, by position in order))."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, p=0.95):
        self.brightness = self._check_input(brightness, "brightness")
        self.contrast = self._check_input(contrast, "contrast")
        self.saturation = self._check_input(saturation, "saturation")
        self.hue = self._check_input(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        self.p = p

    @staticmethod
    def _check_input(value, name, center=1, bound=(0, float("inf")), clip_first_on_zero=True):
        if isinstance(value, numbers.Number):
            if value < 0:
                raise ValueError("If {} is a single number, it must be non negative.".format(name))
            value = [center - float(value), center + float(value)]
            if clip_first_on_zero:
                value[0] = max(value[0], 0.0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            if not bound[0] <= value[0] <= value[1] <= bound[1]:
                raise ValueError("{} values should be between {}".format(name, bound))
        else:
            raise TypeError("{} should be a single number or a list/tuple with length 2.".format(name))
        # if value is 0 or (1., 1.) for brightness/contrast/saturation or (0., 0.) for hue, do nothing
        if value[0] == value[1] == center:
            value = None
        return value

    @staticmethod
    def _scalar(value, like):
        """a python float against an array of `like`'s dtype: numpy rounds it to that dtype first.  (A tensor, not a python
        scalar: torch divides by a python scalar through its rounded reciprocal on the GPU.)"""
        return torch.full((1,), float(value), dtype=like.dtype, device=like.device)

    @classmethod
    def blend(cls, color1, color2, ratio):
        ratio = float(ratio)
        first = cls._scalar(ratio, color1) * color1
        second = cls._scalar(1.0 - ratio, color1) * color2
        return (first + second).clamp(0, 255.0).to(color1.dtype)

    @classmethod
    def rgb_to_grayscale(cls, color):
        r, g, b = color[..., 0], color[..., 1], color[..., 2]
        gray = cls._scalar(0.2989, color) * r + cls._scalar(0.587, color) * g
        gray = gray + cls._scalar(0.114, color) * b
        return gray.unsqueeze(-1)

    @classmethod
    def rgb2hsv(cls, rgb):
        r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        maxc = rgb.max(dim=-1)[0]
        minc = rgb.min(dim=-1)[0]
        eqc = maxc == minc
        cr = maxc - minc
        ones = (torch.ones_like(maxc) * eqc).double()
        neq = (1 - eqc.long()).double()  # (int64 in numpy; float32 * int64 is float64 there: everything from here on)
        wide = maxc.double()
        s = cr.double() / (ones + wide * neq)
        cr_divisor = ones + cr.double() * neq
        rc = (maxc - r).double() / cr_divisor
        gc = (maxc - g).double() / cr_divisor
        bc = (maxc - b).double() / cr_divisor
        hr = (maxc == r).double() * (bc - gc)
        hg = ((maxc == g) & (maxc != r)).double() * (2.0 + rc - bc)
        hb = ((maxc != g) & (maxc != r)).double() * (4.0 + gc - rc)
        h = hr + hg + hb
        h = torch.remainder(h / cls._scalar(6.0, h) + 1.0, 1.0)
        return torch.stack((h, s, wide), dim=-1)

    @staticmethod
    def hsv2rgb(hsv):
        h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
        i = torch.floor(h * 6.0)
        f = (h * 6.0) - i
        i = i.to(torch.int32)
        p = (v * (1.0 - s)).clamp(0.0, 1.0)
        q = (v * (1.0 - s * f)).clamp(0.0, 1.0)
        t = (v * (1.0 - s * (1.0 - f))).clamp(0.0, 1.0)
        i = torch.remainder(i, 6).long().unsqueeze(-1)
        # (the reference's einsum with a one-hot mask adds five zeros to the selected entry)
        a1 = torch.stack((v, q, p, p, t, v), dim=-1).gather(-1, i)
        a2 = torch.stack((t, v, v, q, p, p), dim=-1).gather(-1, i)
        a3 = torch.stack((p, p, t, v, v, q), dim=-1).gather(-1, i)
        return torch.cat((a1, a2, a3), dim=-1)

    def adjust_brightness(self, color, brightness_factor):
        if brightness_factor < 0:
            raise ValueError("brightness_factor ({}) is not non-negative.".format(brightness_factor))
        return self.blend(color, torch.zeros_like(color), brightness_factor)

    def adjust_contrast(self, color, contrast_factor):
        if contrast_factor < 0:
            raise ValueError("contrast_factor ({}) is not non-negative.".format(contrast_factor))
        mean = self.rgb_to_grayscale(color).mean()
        return self.blend(color, mean, contrast_factor)

    def adjust_saturation(self, color, saturation_factor):
        if saturation_factor < 0:
            raise ValueError("saturation_factor ({}) is not non-negative.".format(saturation_factor))
        return self.blend(color, self.rgb_to_grayscale(color), saturation_factor)

    def adjust_hue(self, color, hue_factor):
        if not (-0.5 <= hue_factor <= 0.5):
            raise ValueError("hue_factor ({}) is not in [-0.5, 0.5].".format(hue_factor))
        hsv = self.rgb2hsv(color / self._scalar(255.0, color))
        h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
        h = torch.remainder(h + float(hue_factor), 1.0)
        hsv = torch.stack((h, s, v), dim=-1)
        return (self.hsv2rgb(hsv) * 255.0).to(color.dtype)

    def get_params(self, generator=None):
        order = torch.randperm(4, generator=generator).tolist()
        factors = [None if r is None else float(_uniform(r[0], r[1], (), generator))
                   for r in (self.brightness, self.contrast, self.saturation, self.hue)]
        return order, factors

    def __call__(self, data_dict, generator=None, draws=None):
        if draws is None:
            order, factors = self.get_params(generator)
            gates = None
        else:
            order, factors, gates = [int(v) for v in draws["order"]], list(draws["factors"]), list(draws["gates"])
        adjust = (self.adjust_brightness, self.adjust_contrast, self.adjust_saturation, self.adjust_hue)
        for at, fn_id in enumerate(order):
            if factors[fn_id] is None:
                continue
            gate = float(torch.rand((), dtype=torch.float64, generator=generator)) if gates is None else float(gates[at])
            if gate < self.p:
                data_dict["color"] = adjust[fn_id](data_dict["color"], factors[fn_id])
        return data_dict


class ContrastiveViewsGenerator:
    """transform.py:1046-1067: the `view_keys` cloned twice, `view_trans_cfg` run over either copy, the results written back as
    `view1_*` and `view2_*`.  fuse, generator and device_generator go to the inner Compose; the two views take successive
    draws from the same generators."""

    def __init__(self, view_keys=("coord", "color", "normal", "origin_coord"), view_trans_cfg=None, fuse=False, generator=None,
                 device_generator=None):
        self.view_keys = view_keys
        self.view_trans = Compose(view_trans_cfg, fuse=fuse, generator=generator, device_generator=device_generator)

    def __call__(self, data_dict):
        view1_dict = dict()
        view2_dict = dict()
        for key in self.view_keys:
            view1_dict[key] = data_dict[key].clone()
            view2_dict[key] = data_dict[key].clone()
        view1_dict = self.view_trans(view1_dict)
        view2_dict = self.view_trans(view2_dict)
        for key, value in view1_dict.items():
            data_dict["view1_" + key] = value
        for key, value in view2_dict.items():
            data_dict["view2_" + key] = value
        return data_dict


def pair_views(view1_dict, view2_dict, view1_transform, view2_transform):
    """datasets/scannet_pair.py:70-80: either view through its own transform (a Compose, or any callable on a dict), the results
    under `view1_*` and `view2_*` in one dict -- what point_collate and MaskedSceneContrastCSC then take."""
    view1_dict = view1_transform(view1_dict)
    view2_dict = view2_transform(view2_dict)
    data_dict = dict()
    for key, value in view1_dict.items():
        data_dict["view1_" + key] = value
    for key, value in view2_dict.items():
        data_dict["view2_" + key] = value
    return data_dict


_TRANSFORMS = dict(GridSample=GridSample, SphereCrop=SphereCrop, Collect=Collect, CenterShift=CenterShift,
                   NormalizeColor=NormalizeColor, RandomScale=RandomScale, RandomFlip=RandomFlip,
                   RandomRotateTargetAngle=RandomRotateTargetAngle, ToTensor=ToTensor, Copy=Copy, RandomRotate=RandomRotate,
                   RandomShift=RandomShift, RandomJitter=RandomJitter, ElasticDistortion=ElasticDistortion,
                   ChromaticAutoContrast=ChromaticAutoContrast, ChromaticTranslation=ChromaticTranslation,
                   ChromaticJitter=ChromaticJitter, RandomColorDrop=RandomColorDrop, PointClip=PointClip,
                   ShufflePoint=ShufflePoint, RandomColorJitter=RandomColorJitter,
                   ContrastiveViewsGenerator=ContrastiveViewsGenerator)


def point_collate(batch, mix_prob=0, generator=None, mix=None):
    """datasets/utils.py:14-54 for a list of Collect()-ed dicts: tensors concatenated along dim 0, every '*offset*'
    entry turned into the running end index (int32 on the coord's device, what pointops expects).  mix_prob: Mix3D
    (utils.py:43-54) -- with that probability (`mix` decides when given) every two neighbouring scenes become one cloud:
    offset keeps its entries 1, 3, 5, ... short of the last, and the last."""
    out = {}
    for key in batch[0]:
        vals = [d[key] for d in batch]
        if torch.is_tensor(vals[0]):
            out[key] = torch.cat(vals)
        else:
            out[key] = list(vals)
    dev = out["coord"].device if "coord" in out else None
    if dev is None:  # (the contrastive lists collect view1_coord / view2_coord: the device of the first tensor that is on one)
        dev = next((v.device for v in out.values() if torch.is_tensor(v) and v.is_cuda), None)
    host = {}
    for key in out:
        if "offset" in key and torch.is_tensor(out[key]):
            ends = torch.cumsum(out[key], dim=0).int()
            if not ends.is_cuda:  # Collect() makes the counts on the host: keep the bounds there too, so that callers
                host[key + "_host"] = ends.tolist()  # that slice per scene (DefaultSegmentorSAM_Image) need no read-back
            out[key] = ends.to(dev)
    out.update(host)
    if "offset" in out and torch.is_tensor(out["offset"]):
        if mix is None:
            mix = float(torch.rand((), dtype=torch.float64, generator=generator)) < mix_prob
        if mix:
            out["offset"] = torch.cat([out["offset"][1:-1:2], out["offset"][-1:]])
            if "offset_host" in out:
                out["offset_host"] = out["offset_host"][1:-1:2] + out["offset_host"][-1:]
    return out
