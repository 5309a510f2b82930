/*
 * include/ptv2_msc_hip.h -- C ABI of Masked Scene Contrast (MSC-v1m1) in libptv2_hip.so (MI355X / gfx950): the InfoNCE loss over
 * matched pairs with its backward, the choice of one matched view-2 point per view-1 row, and the patch ids of the cross masks.
 *
 * The eighth public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation,
 * ptv2_refine_hip.h: REAL's label refinement, ptv2_pp2s_hip.h: the PP2S label pipeline, ptv2_ptv1_hip.h: Point Transformer
 * V1, ptv2_spconv_hip.h: SpUNet-v1m1, ptv2_pg_hip.h: PointGroup).  Same conventions: device pointers unless stated, caller-owned
 * workspace, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of
 * ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  No launcher allocates, PTV2_ERR_ARG is returned before
 * anything is enqueued.  No float atomic is used anywhere: two calls on the same inputs give the same bits.
 *
 * What it restates (pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py of the reference; DESIGN.md
 * section 13):
 *   InfoNCE    :179-193.  a_i = f1[p_i0] / (|f1[p_i0]| + 1e-7), b_i likewise, S = A B^T / t, loss = mean_i(lse_i - S_ii),
 *              pos_sim = mean_i a_i.b_i, neg_sim = mean(A B^T) - pos_sim / m.  S is formed in 32 x 32 tiles on
 *              v_mfma_f32_32x32x2_f32 and never stored: what lives between forward and backward is O(m c);
 *   matching   :154-169 after the kNN: per view-1 row the number of neighbours with idx >= 0 and sqrtf(dist2) < max_radius
 *              (strict, on the square-rooted fp32 distance) and the hit of rank count - 1 - draw % count in column order;
 *   patch ids  :94-98: voxel_grid(pos = floor(origin / grid), size = 1, batch = scene, start = 0) over the union of both views,
 *              id = sum_d cell_d prod_{e<d} n_e with n_e = trunc(max_e) + 1 and the scene as the last dimension.  The division
 *              is IEEE fp32.  Cells are not shifted to zero, so a negative cell can share its id with another one.
 */
#ifndef PTV2_MSC_HIP_H
#define PTV2_MSC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MSC_MAX_PAIRS 16384     /* m of one InfoNCE call */
#define MSC_MAX_CHANNELS 256    /* c, a multiple of 4 */
#define MSC_MAX_K 64            /* neighbours of one row in msc_match_hip_launcher */

/* 1: bumped with any change of a signature or constant of THIS header */
int ptv2_msc_abi_version(void);

/* Host only.  Workspace bytes of either direction of the InfoNCE loss of m pairs of c channels; -1 for an argument error. */
long long ptv2_msc_nce_workspace_bytes(long long m, int c);
/* f1 (n1, c), f2 (n2, c) fp32, pairs (m, 2) int64, t > 0.  1 <= m <= MSC_MAX_PAIRS, 4 <= c <= MSC_MAX_CHANNELS, c % 4 == 0.
 * Written for the backward: a, b (m, c) the normalised rows, norms (2, m) their norms before the epsilon, lse (m).
 * out (3): loss, pos_sim, neg_sim.  *status (cleared by the caller) becomes 1 when a pair names a row outside f1 / f2; that
 * row then reads as zeros and the three outputs are NaN, so that a caller need not read the word back. */
int msc_nce_fwd_hip_launcher(int n1, int n2, int m, int c, const float *f1, const float *f2, const long long *pairs, float t,
                             float *a, float *b, float *norms, float *lse, float *out, int *status, void *workspace,
                             long long workspace_bytes, void *stream);
/* df1 (n1, c), df2 (n2, c), every element written, from *g, the upstream gradient of the loss (a device scalar), and what the
 * forward left.  order (2, m) int32: for column 0 and column 1 of pairs the stable ascending argsort of that column; the rows
 * of one index are summed in that order.  A pair or an entry of order outside its range contributes nothing. */
int msc_nce_bwd_hip_launcher(int n1, int n2, int m, int c, const long long *pairs, const int *order, float t, const float *a,
                             const float *b, const float *norms, const float *lse, const float *g, float *df1, float *df2,
                             void *workspace, long long workspace_bytes, void *stream);

/* idx (n1, k) int32 and dist2 (n1, k) fp32 of a kNN of the view-1 points among n2 view-2 points, row_draws (n1) int64.
 * 1 <= k <= MSC_MAX_K.  chosen (n1) int64: the chosen view-2 index, -1 without a hit.  An idx outside [0, n2) is no hit; a
 * negative draw reads as 0. */
int msc_match_hip_launcher(int n1, int k, long long n2, const int *idx, const float *dist2, const long long *row_draws,
                           float max_radius, long long *chosen, void *stream);

/* origin1 (n1, 3), origin2 (n2, 3) fp32; offset1, offset2 (b) int32, the ascending scene ends of either view; cell_max (3) fp32
 * the maxima of floor(origin / grid) over both views.  ids (n1 + n2) int64: the view-1 points, then the view-2 points.  A point
 * past the last scene end counts to the last scene. */
int msc_patch_ids_hip_launcher(int n1, int n2, int b, const float *origin1, const int *offset1, const float *origin2,
                               const int *offset2, float grid, const float *cell_max, long long *ids, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_MSC_HIP_H */
