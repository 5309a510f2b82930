/*
 * include/ptv2_octconv_bf16_hip.h -- C ABI of OctFormer's dense octree convolutions with bf16 matrix-core operands in
 * libptv2_hip.so (MI355X / gfx950): the one form of ptv2_octconv_hip.h,
 *   out[i, :] (cout) = bias + sum over s < slots with j = tab[i, reverse ? slots - 1 - s : s] >= 0 of x[j, :] (cin) . W[s]
 * with its `transpose`, `reverse` and table rows (that header's layer table; DESIGN.md sections 23 and 24), and the weight
 * gradient g_w[s] = sum_i x[tab[i, s], :]^T g[i, :], on V_MFMA_F32_16X16X32_BF16.
 *
 * The nineteenth public header of the library (after ptv2_octconv_hip.h, whose conventions, constants and tables it shares).
 * Written in the subset of C that ao_amd/_abi.py reads.  octconv_bf16_args is octconv_args of ptv2_octconv_hip.h field for
 * field under a name of its own (every header is read alone); the library checks that the two have one size.
 *
 * Roundings, and no others: every operand stays fp32 in memory; the rows of x (of g in the input and weight gradients) and W are
 * rounded to bf16, nearest even, once, on their way into LDS; products are exact, accumulation, bias and every output are fp32.
 * No bf16 tensor and no (n, slots, C) tensor is written to memory.  Every output is written by exactly one lane in a fixed
 * order; there are no atomics: two runs give the same bits.
 */
#ifndef PTV2_OCTCONV_BF16_HIP_H
#define PTV2_OCTCONV_BF16_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* The operands of the three launchers; one that a launcher does not name may be NULL. */
typedef struct octconv_bf16_args {
    int n_out, n_in, slots;             /* rows of out / g, rows of x, columns of tab: 8 or 27 */
    int cin, cout;                      /* the LAYER's channels: weights are (slots, cin, cout), a deconv's (slots, cout, cin) */
    int transpose, reverse;
    const int *tab;                     /* (n_out, slots): rows of x, or -1 */
    const float *x, *w, *bias;          /* (n_in, .), the layer's weights, (cout) or NULL */
    const float *g;                     /* (n_out, .): the weight gradient's second operand */
    float *out;                         /* (n_out, .) */
    float *g_w, *g_b;                   /* the layer's weight shape; (cout) or NULL */
    void *workspace;                    /* the weight gradient's partials */
    long long workspace_bytes;
} octconv_bf16_args;

/* 1: bumped with any change of a signature or struct of THIS header */
int ptv2_octconv_bf16_abi_version(void);
/* Host only: what oct_conv_bf16_gw_hip_launcher needs behind `workspace` (the partials of g_w, then 64 row strips of g_b: the
 * layout of ptv2_octconv_workspace_bytes); -1 for a pair outside the supported set. */
long long ptv2_octconv_bf16_workspace_bytes(int n_out, int slots, int cin, int cout);

/* args: HOST pointer in every launcher below.  The supported pairs are those of ptv2_octconv_hip.h without the stem:
 * cin % 4 == 0 and OCTCONV_STEM_CHANNELS < cin <= OCTCONV_MAX_CHANNELS; cout % 8 == 0 and 8 <= cout <= OCTCONV_MAX_CHANNELS;
 * slots 8 or 27.  All three launchers check the LAYER's pair and return PTV2_ERR_ARG before anything is enqueued.
 * out (n_out, cout) from tab, x (n_in, cin), w, bias, transpose, reverse. */
int oct_conv_bf16_fwd_hip_launcher(const octconv_bf16_args *args, void *stream);
/* The input gradient of a layer: out (n_out, cin) from tab, x = the output's gradient (n_in, cout), w, transpose, reverse as the
 * layer table names them. */
int oct_conv_bf16_gx_hip_launcher(const octconv_bf16_args *args, void *stream);
/* g_w from tab (the forward's), x (n_in, cin), g (n_out, cout), transpose; g_b (cout), the fp32 column sums of g, if not NULL.
 * workspace of ptv2_octconv_bf16_workspace_bytes. */
int oct_conv_bf16_gw_hip_launcher(const octconv_bf16_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_OCTCONV_BF16_HIP_H */
