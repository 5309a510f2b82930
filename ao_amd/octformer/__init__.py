"""OctFormer-v1m1 on HIP: the octree attention blocks and the stem, Downsample, the decoder and the model on
the matrix-core octree convolutions (section 23).  ocnn is not needed: its modules, tables and parameter names are restated."""
from .model import (MLP, RPE, Downsample, OctFormer, OctFormerBlock, OctFormerDecoder, OctFormerStage, OctreeAttention, OctreeConv,
                    OctreeConvBnRelu, OctreeDeconv, OctreeDeconvBnRelu, OctreeDropPath, OctreeDWConv, OctreeDWConvBn, OctreeUpsample,
                    PatchEmbed)
from .octree import OctreeLevel, OctreeLink, OctreePyramid, octree_level, octree_link, octree_pyramid, xyz2key
from .ops import (octree_attention, octree_attention_torch, octree_conv, octree_conv_torch, octree_deconv, octree_dwconv,
                  octree_dwconv_torch, pos_bnd_of)

__all__ = ["MLP", "RPE", "OctFormerBlock", "OctFormerStage", "OctreeAttention", "OctreeDropPath", "OctreeDWConv",
           "OctreeDWConvBn", "OctreeLevel", "octree_level", "xyz2key", "octree_attention", "octree_attention_torch",
           "octree_dwconv", "octree_dwconv_torch", "pos_bnd_of", "Downsample", "OctFormer", "OctFormerDecoder", "OctreeConv",
           "OctreeConvBnRelu", "OctreeDeconv", "OctreeDeconvBnRelu", "OctreeUpsample", "PatchEmbed", "OctreeLink",
           "OctreePyramid", "octree_link", "octree_pyramid", "octree_conv", "octree_conv_torch", "octree_deconv"]
