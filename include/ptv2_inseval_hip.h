/*
 * include/ptv2_inseval_hip.h -- C ABI of the instance-segmentation evaluator's association pass in libptv2_hip.so (MI355X /
 * gfx950): for every proposal the histogram of its set points over the ground-truth instances, its size and its overlap with
 * the void points.
 *
 * The tenth public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation,
 * ptv2_refine_hip.h: REAL's label refinement, ptv2_pp2s_hip.h: the PP2S label pipeline, ptv2_ptv1_hip.h: Point Transformer
 * V1, ptv2_spconv_hip.h: SpUNet-v1m1, ptv2_pg_hip.h: PointGroup, ptv2_msc_hip.h: Masked Scene Contrast, ptv2_st_hip.h:
 * Stratified Transformer).  Same conventions: device pointers, `void *stream` is a hipStream_t, int status return (PTV2_OK,
 * PTV2_ERR_ARG, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  The launcher allocates
 * nothing and needs no workspace; PTV2_ERR_ARG is returned before anything is enqueued.  Integer atomics only (shared-memory
 * bins per workgroup, flushed with global integer adds): every output is an exact count, the same on every call.
 *
 * What it restates (pointcept/engines/hooks/evaluator.py: InsSegEvaluator.associate_instances of the reference; DESIGN.md
 * section 15): with set(p, j) = masks[p, col(j)] != 0 and col(j) = nn_idx[j] (j itself without nn_idx),
 *   inter[p, g]     the number of points j with set(p, j) whose ground-truth column is g
 *   vert_count[p]   the number of points j with set(p, j)
 *   void_inter[p]   the number of points j with set(p, j) that are void
 */
#ifndef PTV2_INSEVAL_HIP_H
#define PTV2_INSEVAL_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define INSEVAL_BINS 256              /* ground-truth columns of one call: the shared-memory bins of one proposal */
#define INSEVAL_POINTS_PER_WG 2048    /* points of one workgroup */
#define INSEVAL_ROWS_PER_WG 8         /* proposals of one workgroup: the point's code and column are read once for them */
#define INSEVAL_MAX_PROPOSALS 65535

/* 1: bumped with any change of a signature or constant of THIS header */
int ptv2_inseval_abi_version(void);

/* The code of a point: 2 * (column + 1) + void, column in [-1, g) the ground-truth column of the point (-1: none), void 1 when
 * the point's segment label is ignored.  The two facts are independent: a void point may carry a column. */

/* masks (p, m) int32, an element is set when != 0; nn_idx (n) int32 or NULL (then n == m); gt_code (n) int32 as above, a
 * column outside [0, g) counts as none, an nn_idx outside [0, m) as not set.  inter (p, g) int32 (may be NULL when g == 0),
 * vert_count (p), void_inter (p) int32: every element written.  0 <= p <= INSEVAL_MAX_PROPOSALS, 0 <= g <= INSEVAL_BINS,
 * 0 <= n, 0 <= m; more columns are served by one call per window of INSEVAL_BINS columns, the codes re-based by the caller. */
int inseval_associate_hip_launcher(int p, int m, int n, int g, const int *masks, const int *nn_idx, const int *gt_code,
                                   int *inter, int *vert_count, int *void_inter, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_INSEVAL_HIP_H */
