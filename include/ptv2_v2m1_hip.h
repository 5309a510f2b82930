/*
 * include/ptv2_v2m1_hip.h -- C ABI of the logits stage of Point Transformer V2 "mode 1" (PT-v2m1: GroupedLinear as the first
 * layer of weight_encoding, and the position multiplier linear_p_multiplier) in libptv2_hip.so (MI355X / gfx950).
 *
 * The twelfth public header of the library (after ptv2_hip.h, ptv2_data_hip.h, ptv2_refine_hip.h, ptv2_pp2s_hip.h,
 * ptv2_ptv1_hip.h, ptv2_spconv_hip.h, ptv2_pg_hip.h, ptv2_msc_hip.h, ptv2_st_hip.h, ptv2_inseval_hip.h, ptv2_csc_hip.h).
 * Same conventions: device pointers unless stated, caller-owned workspace, `void *stream` is a hipStream_t, int status
 * return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that
 * ao_amd/_abi.py reads.  No launcher allocates; PTV2_ERR_ARG is returned before anything is enqueued.  All reductions are
 * per-workgroup partial sums followed by a fixed-order final sum; no float atomic is used anywhere: two calls on the same
 * inputs give the same bits.
 *
 * What it restates (pointcept/models/point_transformer_v2/point_transformer_v2m1_origin.py:141-159 of the reference with
 * pe_multiplier = pe_bias = True; the notation is that of ao_amd/ptv2/gva.py).  n points, k neighbour
 * slots, c channels, g groups, 8 channels per group: g(ch) = ch / 8.  idx (n, k) int32 with -1 placeholders, coord (n, 3).
 *   mask       = idx >= 0
 *   pos[n,s]   = mask (coord[idx[n,s]] - coord[n])
 *   Pm[n,s,:]  = ReLU(pos a_m^T + b_m)          a_m (c,3), b_m (c): Linear(3,c) + BatchNorm of linear_p_multiplier, folded
 *   pem[n,s,ch]= sum_c' Pm[n,s,c'] Wm2[ch,c'] + bm2[ch]                                         (never stored)
 *   P[n,s,:]   = ReLU(pos a^T + b)              a (c,3), b (c): the same fold of linear_p_bias
 *   W1[n,s,j]  = sum_{ch in j} w[ch] (key[idx[n,s],ch] mask - query[n,ch]) pem[n,s,ch] + sum_c' P[n,s,c'] M[c',j] + cW[j]
 *                w (c) = GroupedLinear.weight[0];  M (c,g), cW (g) formed by the caller
 *   T1[j] = sum_{n,s} W1[n,s,j],  T2[j] = sum_{n,s} W1[n,s,j]^2     float64, over all n k slots, masked ones included
 * pem is a (rows x c) . (c x c) product on v_mfma_f32_16x16x4_f32 per tile of 16 slots, from a tile of Pm built in LDS, Wm2
 * streamed in chunks of 16 columns; it is formed again by the backward, not saved.  Nothing whose size grows with n k c is
 * read from or written to memory but the gathered key rows.
 *
 * Shapes: (c, g) in (48, 6), (96, 12), (192, 24), (384, 48), (512, 64); k a power of two, 2 <= k <= 64; n >= 1, n k < 2^31.
 * Anything else returns PTV2_ERR_ARG (the caller then evaluates the literal op sequence).
 */
#ifndef PTV2_V2M1_HIP_H
#define PTV2_V2M1_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: bumped with any change of a signature of THIS header */
int ptv2_v2m1_abi_version(void);

/* Host only.  Workspace bytes of either direction; 0 for a shape the launchers refuse. */
size_t gva_mul_workspace_bytes(int n, int k, int c, int g);
/* key, query (n, c); w, b_m, bm2, b (c); a_m, a (c, 3); Wm2 (c, c) row-major [ch][c']; M (c, g); cW (g).
 * Written: W1 (n, k, g) fp32, T1 (g), T2 (g) float64. */
int gva_mul_logits_forward_hip_launcher(int n, int k, int c, int g, const float *key, const float *query, const float *w,
                                        const float *a_m, const float *b_m, const float *Wm2, const float *bm2,
                                        const float *a, const float *b, const float *M, const float *cW,
                                        const float *coord, const int *idx, float *W1, double *T1, double *T2,
                                        void *workspace, size_t workspace_bytes, void *stream);
/* Given W1 as the forward left it and gW1 (n, k, g), gT1, gT2 (g, float64), with gWt = gW1 + gT1 + 2 gT2 W1 the gradient of
 * every slot.  inv_ptr (n + 1), inv_rows (n k): the inverse neighbour table of ptv2_hip.h (inverse_table_hip_launcher), both
 * required: g_key is the fixed-order sum over the list of every point.  Every element of every output is written:
 *   g_key (n, c), g_query (n, c)
 *   g_w (c)              the direct part only: M and cW depend on w in the caller
 *   g_Wm2 (c, c), g_bm2 (c), g_a_m (c, 3), g_b_m (c)    the last two through the ReLU of Pm
 *   g_a (c, 3), g_b (c), g_M (c, g), g_cW (g)           as gva_logits_backward_hip_launcher gives them */
int gva_mul_logits_backward_hip_launcher(int n, int k, int c, int g, const float *key, const float *query, const float *w,
                                         const float *a_m, const float *b_m, const float *Wm2, const float *bm2,
                                         const float *a, const float *b, const float *M, const float *coord,
                                         const int *idx, const float *W1, const float *gW1, const double *gT1,
                                         const double *gT2, const int *inv_ptr, const int *inv_rows, float *g_key,
                                         float *g_query, float *g_w, float *g_Wm2, float *g_bm2, float *g_a_m,
                                         float *g_b_m, float *g_a, float *g_b, float *g_M, float *g_cW, void *workspace,
                                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_V2M1_HIP_H */
