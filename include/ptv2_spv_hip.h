/*
 * include/ptv2_spv_hip.h -- C ABI of SPVCNN's point branch in libptv2_hip.so (MI355X / gfx950): the point-voxel map of a
 * batch of points and the two operators that move features between its points and the voxels of the five levels of the sparse
 * convolutions: trilinear devoxelisation (voxel_to_point) and the per-voxel mean (initial_voxelize / point_to_voxel).
 *
 * The fifteenth public header of the library (after ptv2_oct_hip.h).  Same conventions as ptv2_spconv_hip.h: device pointers
 * unless stated, caller-owned workspace, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG,
 * PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  spv_map is a HOST
 * struct of device pointers, read during the call.  PTV2_ERR_ARG is returned before anything is enqueued.
 *
 * What it restates (pointcept/models/spvcnn/ts_spvcnn.py of the reference and the four torchsparse functions it calls:
 * spvoxelize with spcount, calc_ti_weights, spdevoxelize, get_kernel_offsets(2, s)).  At level l, s = 2^l:
 *   voxel       of a point p of cloud c: (c, p >> l).  Level l of the map numbers its voxels as level l of ptv2_spconv_hip.h does
 *               when level 0 is handed over in the map's order: ascending (cloud, x, y, z) at every level.
 *   voxelize    V[v] = (sum of X[i] over the points of voxel v) / count_v.
 *   devoxelize  f = (p - ((p >> l) << l)) / s in [0, 1)^3; corner j = 4 jx + 2 jy + jz is the voxel at (p >> l) + (jx, jy, jz) of the
 *               same cloud, column 9 (jx + 1) + 3 (jy + 1) + (jz + 1) of the k = 3 table; w_j = prod over the axes of (j_a ? f_a :
 *               1 - f_a), 0 where the corner has no voxel; W = sum_j w_j + 1e-8; out[i] = sum_j (w_j / W) F[corner_j] (+ add[i]).
 *
 * Memory: no (n, 8) index or weight tensor exists.  The forward forms the eight weights from the point's coordinate and its
 * table row and keeps one float per point (W); the backward re-forms them.  Every sum has a fixed order and no launcher uses an
 * atomic: two calls on the same inputs give the same bits.
 */
#ifndef PTV2_SPV_HIP_H
#define PTV2_SPV_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SPV_LEVELS 5          /* SPCONV_LEVELS */
#define SPV_COORD_BITS 18     /* SPCONV_COORD_BITS */
#define SPV_MAX_CLOUDS 1024
#define SPV_MAX_CHANNELS 384  /* devoxelize and voxelize: multiples of 32 up to this */
#define SPV_SMALL_CHANNELS 16 /* voxelize alone: also every width from 1 to this (the input features) */

/* the status array: word log2(bit) is set to 1 (a plain store, no atomic) */
#define SPV_BAD_NEGATIVE 1    /* a negative coordinate */
#define SPV_BAD_LARGE 2       /* a coordinate >= 2^SPV_COORD_BITS */
#define SPV_STATUS_WORDS 2

/* Everything spv_build_map_hip_launcher writes.  n points; level l has counts[l] voxels. */
typedef struct spv_map {
    int *row[SPV_LEVELS];    /* (n): the level-l voxel of each point */
    int *start[SPV_LEVELS];  /* (n + 1), the first counts[l] + 1 valid: the points of voxel v are order[l][start[l][v] .. start[l][v + 1]) */
    int *order[SPV_LEVELS];  /* (n): point indices by (voxel, index) */
    int *vcoord;             /* (n, 3), the first counts[0] rows valid: the coordinates of the level-0 voxels */
    int *voffset;            /* (b): the cloud ends of the level-0 voxels */
    int *counts;             /* (SPV_LEVELS) */
    int *status;             /* (SPV_STATUS_WORDS): zeroed by the caller */
} spv_map;

/* 1: bumped with any change of a signature, struct or constant of THIS header */
int ptv2_spv_abi_version(void);
/* sizeof of spv_map (0) as compiled; -1 otherwise */
int ptv2_spv_struct_bytes(int which);

/* Host only.  Workspace bytes of the map build for n points in b clouds; -1 for an argument error. */
long long ptv2_spv_map_workspace_bytes(long long n, int b);

/* coord (n, 3) int32 point coordinates, several points may share a voxel; offset (b) int32 cloud ends (ascending, the last is
 * n).  1 <= n < 2^30, 1 <= b <= SPV_MAX_CLOUDS.  Per level: a stable sort of (cloud, x >> l, y >> l, z >> l), the heads of its
 * runs and their ranks.  A bad coordinate is clamped into range and recorded in *status: the map is then not to be used, and
 * no kernel indexes outside a buffer.  Reads nothing back. */
int spv_build_map_hip_launcher(int n, int b, const int *coord, const int *offset, const spv_map *map, void *workspace,
                               long long workspace_bytes, void *stream);

/* out (n, c) and wsum (n) from feat (n_vox, c), add (n, c) or NULL, coord (n, 3), row (n) and nbr3 (n_vox, 27) of `level`.
 * c a multiple of 32, c <= SPV_MAX_CHANNELS; 0 <= level < SPV_LEVELS. */
int spv_devoxelize_fwd_hip_launcher(int n, int n_vox, int c, int level, const int *coord, const int *row, const int *nbr3,
                                    const float *feat, const float *add, float *out, float *wsum, void *stream);
/* g_feat (n_vox, c), every row written, from g (n, c), the forward's wsum and the level's start / order: row v sums, corner by
 * corner, the points of the voxel at column 13 - (9 jx + 3 jy + jz) of nbr3[v]. */
int spv_devoxelize_bwd_hip_launcher(int n, int n_vox, int c, int level, const int *coord, const int *nbr3, const int *start,
                                    const int *order, const float *wsum, const float *g, float *g_feat, void *stream);

/* v (n_vox, c) from x (n, c).  c a multiple of 32 up to SPV_MAX_CHANNELS, or 1 <= c <= SPV_SMALL_CHANNELS. */
int spv_voxelize_fwd_hip_launcher(int n, int n_vox, int c, int level, const int *start, const int *order, const float *x, float *v,
                                  void *stream);
/* g_x (n, c): g_x[i] = g_v[row[i]] / count of that voxel */
int spv_voxelize_bwd_hip_launcher(int n, int n_vox, int c, const int *row, const int *start, const float *g_v, float *g_x,
                                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_SPV_HIP_H */
