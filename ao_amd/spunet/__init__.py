"""SpUNet-v1m1 (the reference's sparse U-Net) on the MI355X: ao_amd/spunet/model.py, with the sparse convolutions on
ao_amd/csrc/spconv.hip (ao_amd/spunet/conv.py) over the tables of ao_amd/csrc/spconv_tables.hip (ao_amd/spunet/tables.py)."""
from .conv import down_conv, gather_torch, inverse_conv, scatter_torch, subm_conv
from .model import (BasicBlock, SparseConv3d, SparseInverseConv3d, SparseSequential, SparseTensor, SpUNetBase, SubMConv3d)
from .tables import SpconvTables, build_tables

__all__ = ["down_conv", "gather_torch", "inverse_conv", "scatter_torch", "subm_conv", "BasicBlock", "SparseConv3d",
           "SparseInverseConv3d", "SparseSequential", "SparseTensor", "SpUNetBase", "SubMConv3d", "SpconvTables", "build_tables"]
