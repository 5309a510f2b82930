/*
 * include/ptv2_oct_hip.h -- C ABI of OctFormer's octree attention blocks (OctFormer-v1m1) in libptv2_hip.so (MI355X / gfx950):
 * the 27-neighbour table of a Morton-ordered node list, the fused dilated patch attention and the depthwise octree convolution
 * of the conditional position encoding.
 *
 * The fourteenth public header of the library (after ptv2_spconv_bf16_hip.h).  Same conventions as ptv2_st_hip.h: device
 * pointers unless stated, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE,
 * PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  No launcher allocates; PTV2_ERR_ARG is
 * returned before anything is enqueued.
 *
 * What it restates (pointcept/models/octformer/octformer_v1m1_base.py of the reference):
 *   partition  :93-99, :223, :244.  With G = patch * dilation, patch p = g * dilation + d has its slot j at node
 *              g * G + j * dilation + d of the node list; a slot whose node index is >= n is padding.  The kernels index the
 *              node list itself: no padded copy, no transposed copy.
 *   logits     :165-176, :232-237.  scale * q_i . k_j + sum_a table[a * R + clamp(xyz_i[a] - xyz_j[a], +-pos_bnd) + pos_bnd, h],
 *              R = 2 * pos_bnd + 1.
 *   mask       :66-78.  A pair takes part in the row softmax only if both slots are real and batch_i == batch_j; otherwise its
 *              weight is exactly 0.  The reference ADDS -1e3 to such a logit instead: exp(-1e3 + x - max) is 0 in fp32 and in
 *              float64 as long as the unmasked logits stay below about 100 in magnitude (fp32 underflows below e^-104, float64
 *              keeps a weight of at most e^-800), so the two are the same function there.  The reference's padded rows carry
 *              the qkv bias and attend only each other, and patch_reverse cuts them off; the kernels never read or write them.
 *   dwconv     y[i, c] = sum_k w[k, 0, c] x[nbr[i, k], c] over the 27 slots of the neighbour table, -1 skipped.
 *
 * Layouts: qkv (n, 3 C) fp32 exactly as the qkv Linear wrote it, columns ordered [3][h][hd]; table (3 R, h); out (n, C) with
 * column head * hd + e in the node's own row; lse (n, h) the row log-sum-exp; g_qkv (n, 3 C); nbr (n, 27) int32 with slot
 * (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1); dwconv weights (27, 1, C) read as (27, C).
 *
 * Every output but g_table is written by exactly one wavefront (or thread) in a fixed order and is bit-repeatable.  g_table is
 * accumulated per workgroup in LDS with atomic adds, one partial per workgroup, and the partials are summed in a fixed order:
 * the LDS adds are not ordered, so g_table is not bit-repeatable (ptv2_st_hip.h accepts the same of its table gradients).
 */
#ifndef PTV2_OCT_HIP_H
#define PTV2_OCT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define OCT_MAX_PATCH 32        /* slots of one patch (the logit tile is 32 x 32) */
#define OCT_MAX_HEADS 64
#define OCT_MAX_RPE 255         /* R = 2 * pos_bnd + 1: the table indices of a pair are kept as bytes */
#define OCT_MAX_CHANNELS 1024   /* of the depthwise convolution */
#define OCT_MAX_DEPTH 16        /* 3 * depth key bits; the sort key of python keeps the cloud id above them */

/* The operands of every launcher; one that a launcher does not name may be NULL. */
typedef struct oct_args {
    int n, clouds, depth;               /* nodes, clouds, octree depth: coordinates lie in [0, 2^depth) */
    int c, h, hd;                       /* channels, heads, channels per head (16 or 32); attention: c == h * hd */
    int patch, dilation, pos_bnd;       /* K, D, and R = 2 * pos_bnd + 1 */
    float scale;
    const int *xyz, *batch;             /* (n, 3), (n): in node order (cloud, then Morton key) */
    const long long *keys;              /* (n): the Morton key within the cloud, ascending within each cloud */
    const int *cloud_offsets;           /* (clouds + 1): the rows of each cloud */
    int *nbr_out;                       /* (n, 27), written by oct_neighbors_hip_launcher */
    const int *nbr;                     /* (n, 27), read by the convolution */
    const float *qkv, *table;           /* (n, 3 c), (3 R, h) */
    const float *g_out;                 /* (n, c) */
    float *out, *lse;                   /* (n, c), (n, h): written by the forward, read by the backward */
    float *g_qkv, *g_table;             /* (n, 3 c), (3 R, h): written, not added to */
    const float *x, *w, *g_y;           /* (n, c), (27, c), (n, c) */
    float *y, *g_x, *g_w;               /* (n, c), (n, c), (27, c) */
    void *workspace;                    /* the backwards' partial sums */
    long long workspace_bytes;
} oct_args;

/* 1: bumped with any change of a signature, constant or struct of THIS header */
int ptv2_oct_abi_version(void);
/* Host only: sizeof(oct_args) of the library. */
int ptv2_oct_struct_bytes(int which);
/* Host only: what oct_attention_bwd_hip_launcher needs behind `workspace` (one (3 R, h) partial per patch), and what
 * oct_dwconv_bwd_hip_launcher needs (one (27, c) partial per workgroup).  -1 for arguments outside the supported set. */
long long ptv2_oct_workspace_bytes(int n, int patch, int dilation, int h, int rpe);
long long ptv2_oct_dwconv_workspace_bytes(int n, int c);

/* args: HOST pointer in every launcher below.
 * nbr_out from n, clouds, depth, xyz, batch, keys, cloud_offsets: slot k = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) of row i holds the
 * row of the node of the same cloud at xyz_i + (dx, dy, dz), found by a binary search of that cloud's keys, or -1.  A
 * neighbour coordinate outside [0, 2^depth) is -1 before any key is formed.  1 <= depth <= OCT_MAX_DEPTH. */
int oct_neighbors_hip_launcher(const oct_args *args, void *stream);

/* out and lse from n, c, h, hd, patch, dilation, pos_bnd, scale, xyz, batch, qkv, table.  PTV2_ERR_ARG unless
 * 1 <= patch <= OCT_MAX_PATCH, hd in {16, 32}, 1 <= h <= OCT_MAX_HEADS, c == h * hd, dilation >= 1, 2 * pos_bnd + 1 <= OCT_MAX_RPE. */
int oct_attention_fwd_hip_launcher(const oct_args *args, void *stream);
/* g_qkv and g_table from the forward's operands, out, lse and g_out; workspace of ptv2_oct_workspace_bytes. */
int oct_attention_bwd_hip_launcher(const oct_args *args, void *stream);

/* y from n, c, nbr, x, w.  c % 4 == 0, c <= OCT_MAX_CHANNELS. */
int oct_dwconv_fwd_hip_launcher(const oct_args *args, void *stream);
/* g_x (the forward with the weights mirrored, w[26 - k]: nbr[i, k] == j exactly when nbr[j, 26 - k] == i) and
 * g_w[k, c] = sum_i x[nbr[i, k], c] g_y[i, c] from n, c, nbr, x, w, g_y; workspace of ptv2_oct_dwconv_workspace_bytes.  Either of
 * g_x, g_w may be NULL. */
int oct_dwconv_bwd_hip_launcher(const oct_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_OCT_HIP_H */
