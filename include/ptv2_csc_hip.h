/*
 * include/ptv2_csc_hip.h -- C ABI of the partitioned InfoNCE loss of Masked Scene Contrast v1m2 (CSC, contrastive scene
 * contexts) in libptv2_hip.so (MI355X / gfx950): forward and backward.
 *
 * The eleventh public header of the library (after ptv2_hip.h, ptv2_data_hip.h, ptv2_refine_hip.h, ptv2_pp2s_hip.h,
 * ptv2_ptv1_hip.h, ptv2_spconv_hip.h, ptv2_pg_hip.h, ptv2_msc_hip.h, ptv2_st_hip.h, ptv2_inseval_hip.h).  Same conventions:
 * device pointers unless stated, caller-owned workspace, `void *stream` is a hipStream_t, int status return (PTV2_OK,
 * PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  No
 * launcher allocates, PTV2_ERR_ARG is returned before anything is enqueued.  No float atomic is used anywhere: two calls on
 * the same inputs give the same bits.
 *
 * What it restates (pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m2_csc.py:182-264 of the reference;
 * DESIGN.md section 16).  The m pairs are grouped by scene: scene s owns the rows seg[s] .. seg[s + 1].  Inside a scene, with
 * a_i = f1[p_i0] / (|f1[p_i0]| + 1e-7), b_j likewise, S_ij = a_i.b_j, x_j = origin1[p_j0], y_i = origin2[p_i1]:
 *   class(i, j)   rel = x_j - y_i, d = sqrtf(rel.rel + 1e-7) in fp32; "none" unless rel_z != 0 and d > r1; then 0 (rel_z > 0)
 *                 or 1 (rel_z < 0) where d <= r2, and 2 or 3 where d > r2.  The diagonal belongs to every class;
 *   loss_s        sum over the CSC_CLASSES classes k of mean_i(logsumexp_{j: class(i, j) = k or j = i}(S_ij / t) - S_ii / t);
 *   scalars       over the scenes with a pair in ascending order: pos += mean_i S_ii, neg += mean_ij S_ij - pos / M_s with the
 *                 pos accumulated so far; loss = sum_s loss_s / (b partitions), pos_sim = pos / b, neg_sim = neg / b.
 * S is formed in 64 x 64 tiles on v_mfma_f32_32x32x2_f32 inside one scene's block and never stored: what lives between forward
 * and backward is O(m c).
 */
#ifndef PTV2_CSC_HIP_H
#define PTV2_CSC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CSC_MAX_PAIRS 16384     /* m of one call, all scenes together */
#define CSC_MAX_CHANNELS 256    /* c, a multiple of 4 */
#define CSC_MAX_SCENES 1024     /* b */
#define CSC_CLASSES 5           /* none, 0, 1, 2, 3: the rows of lse */
#define CSC_MAX_INV_T 40        /* 1 / t at most: the row sums shift by the constant 1 / t, and exp(-2 / t) stays normal */

/* 1: bumped with any change of a signature or constant of THIS header */
int ptv2_csc_abi_version(void);

/* Host only.  Workspace bytes of either direction for m pairs of c channels in b scenes; -1 for an argument error. */
long long ptv2_csc_nce_workspace_bytes(long long m, int c, int b);
/* f1 (n1, c), f2 (n2, c), origin1 (n1, 3), origin2 (n2, 3) fp32; pairs (m, 2) int64 grouped by scene; seg (b + 1) int32, the
 * ascending first rows of the scenes, seg[0] = 0 and seg[b] = m (a scene may be empty); t > 0 with 1 / t <= CSC_MAX_INV_T;
 * r1, r2 compared in fp32; partitions >= 1 only divides.  1 <= m <= CSC_MAX_PAIRS, 4 <= c <= CSC_MAX_CHANNELS, c % 4 == 0,
 * 1 <= b <= CSC_MAX_SCENES.
 * Written for the backward: a, bn (m, c) the normalised rows, norms (2, m) their norms before the epsilon, coords (2, m, 3)
 * the gathered x and y, lse (CSC_CLASSES, m) the log of the row sums of exp((S_ij - 1) / t).  out (3): loss, pos_sim, neg_sim.  *status (cleared by the caller) becomes 1
 * when a pair names a row outside f1 / f2 (that row then reads as zeros) or seg is not as described (it is then read clamped);
 * the three outputs are NaN in that case, so that a caller need not read the word back. */
int csc_nce_fwd_hip_launcher(int n1, int n2, int m, int c, int b, const float *f1, const float *f2, const float *origin1,
                             const float *origin2, const long long *pairs, const int *seg, float t, float r1, float r2,
                             int partitions, float *a, float *bn, float *norms, float *coords, float *lse, float *out,
                             int *status, void *workspace, long long workspace_bytes, void *stream);
/* df1 (n1, c), df2 (n2, c), every element written, from *g, the upstream gradient of the loss (a device scalar), and what the
 * forward left.  order (2, m) int32: for column 0 and column 1 of pairs the stable ascending argsort of that column; the rows
 * of one index are summed in that order.  A pair or an entry of order outside its range contributes nothing. */
int csc_nce_bwd_hip_launcher(int n1, int n2, int m, int c, int b, const long long *pairs, const int *seg, const int *order,
                             float t, float r1, float r2, int partitions, const float *a, const float *bn, const float *norms,
                             const float *coords, const float *lse, const float *g, float *df1, float *df2, void *workspace,
                             long long workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_CSC_HIP_H */
