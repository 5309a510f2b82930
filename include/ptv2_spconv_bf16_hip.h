/*
 * include/ptv2_spconv_bf16_hip.h -- C ABI of the bf16-operand matrix-core forms of SpUNet-v1m1's sparse convolutions in
 * libptv2_hip.so (MI355X / gfx950): the gather / scatter and weight-gradient forms of ptv2_spconv_hip.h with both operands of
 * every product rounded to bf16 (nearest even) on their way into V_MFMA_F32_16X16X32_BF16.
 *
 * The thirteenth public header of the library (after ptv2_hip.h, ptv2_data_hip.h, ptv2_refine_hip.h, ptv2_pp2s_hip.h,
 * ptv2_ptv1_hip.h, ptv2_spconv_hip.h, ptv2_pg_hip.h, ptv2_msc_hip.h, ptv2_st_hip.h, ptv2_inseval_hip.h, ptv2_csc_hip.h,
 * ptv2_v2m1_hip.h).  Same conventions: device pointers unless stated, caller-owned workspace, `void *stream` is a hipStream_t,
 * int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C
 * that ao_amd/_abi.py reads.  No launcher allocates; PTV2_ERR_ARG is returned before anything is enqueued.
 *
 * Tables, weights, forms and their constants (SPCONV_GATHER, SPCONV_SCATTER, SPCONV_MAX_SPLITS) are those of
 * ptv2_spconv_hip.h; the tables come from spconv_build_tables_hip_launcher.  Activations, gradients and weights are fp32 in
 * memory on both sides; accumulation is fp32; every output row is stored once.  A launcher first writes the weight into its
 * workspace as bf16 in the layout [kappa][a][b], a the output channel and b the reduction index of that call, so the transposed
 * form is another packing of the same weight.  Every sum has a fixed order and no launcher uses an atomic: two calls on the
 * same inputs give the same bits.  The stem (Cin <= 16) and the 1 x 1 x 1 convolutions have no bf16 form.
 */
#ifndef PTV2_SPCONV_BF16_HIP_H
#define PTV2_SPCONV_BF16_HIP_H

#include "ptv2_spconv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: bumped with any change of a signature of THIS header */
int ptv2_spconv_bf16_abi_version(void);

/* Host only.  Workspace bytes of either launcher over a table of n rows and k columns: the packed weight (k * Cin * Cout
 * bf16) plus the weight gradient's partial sums; -1 for an argument error (n < 0, k outside [1, 27], a width that is not a
 * multiple of 32 in [32, 4096]).  Does not grow with n beyond SPCONV_MAX_SPLITS splits. */
long long ptv2_spconv_bf16_workspace_bytes(long long n, int k, int cin, int cout);

/* spconv_conv_hip_launcher with bf16 operands: the same form, transpose and reverse, the same shapes.  Cin and Cout are
 * multiples of 32, k <= 27, reverse with SPCONV_GATHER only; a table entry outside [0, n_other) is treated as -1.
 * workspace_bytes >= ptv2_spconv_bf16_workspace_bytes(n_tab, k, cin, cout), or PTV2_ERR_WORKSPACE. */
int spconv_bf16_conv_hip_launcher(int form, int n_tab, int n_other, int k, int cin, int cout, const float *in, const int *tab,
                                  const float *weight, int transpose, int reverse, float *out, void *workspace,
                                  long long workspace_bytes, void *stream);

/* spconv_wgrad_hip_launcher with x and g rounded to bf16: gW[co][kappa][ci] = sum over r of g[gr][co] x[xr][ci],
 * j = tab[r][kappa] in [0, n_other), (gr, xr) = (r, j), or (j, r) when gather_g != 0.  Cin and Cout multiples of 32, k <= 27.
 * Every element of gW is written; the sum runs in row order within each of the splits and then over the splits, whose
 * number depends on n_tab alone. */
int spconv_bf16_wgrad_hip_launcher(int n_tab, int n_other, int k, int cin, int cout, const float *x, const float *g,
                                   const int *tab, int gather_g, float *gW, void *workspace, long long workspace_bytes,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_SPCONV_BF16_HIP_H */
