"""SPVCNN (the reference's point-voxel network) on the MI355X: ao_amd/spvcnn/model.py, with the point branch -- the point-voxel
map (ao_amd/spvcnn/pvmap.py on ao_amd/csrc/spv_map.hip) and devoxelize / voxelize (ao_amd/spvcnn/ops.py on ao_amd/csrc/spv_ops.hip)
-- beside the sparse convolutions of ao_amd/spunet."""
from .model import (BasicConvolutionBlock, BasicDeconvolutionBlock, Conv3d, ResidualBlock, SPVCNN, krsc_weight)
from .ops import corner_table, devoxelize, devoxelize_torch, voxelize, voxelize_torch
from .pvmap import PointVoxelMap, point_voxel_map

__all__ = ["BasicConvolutionBlock", "BasicDeconvolutionBlock", "Conv3d", "ResidualBlock", "SPVCNN", "krsc_weight", "corner_table",
           "devoxelize", "devoxelize_torch", "voxelize", "voxelize_torch", "PointVoxelMap", "point_voxel_map"]
