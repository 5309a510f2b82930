"""OctFormer-v1m1's octree attention blocks on HIP: everything between the reference model's patch_embed
and decoder.  The stem, Downsample, the decoder and OctreeInterp are ocnn modules and a follow-up."""
from .model import MLP, RPE, OctFormerBlock, OctFormerStage, OctreeAttention, OctreeDropPath, OctreeDWConv, OctreeDWConvBn
from .octree import OctreeLevel, octree_level, xyz2key
from .ops import octree_attention, octree_attention_torch, octree_dwconv, octree_dwconv_torch, pos_bnd_of

__all__ = ["MLP", "RPE", "OctFormerBlock", "OctFormerStage", "OctreeAttention", "OctreeDropPath", "OctreeDWConv",
           "OctreeDWConvBn", "OctreeLevel", "octree_level", "xyz2key", "octree_attention", "octree_attention_torch",
           "octree_dwconv", "octree_dwconv_torch", "pos_bnd_of"]
