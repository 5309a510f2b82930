/*
 * include/ptv2_st_hip.h -- C ABI of Stratified Transformer (ST-v1m2) in libptv2_hip.so (MI355X / gfx950): the window cells and
 * the pair lists of stratified attention, the relative-position index, the three pointops2 operators the model calls with a
 * row softmax between them, the fused window attention that replaces all of them, and the stem's KPConv.
 *
 * The ninth public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation,
 * ptv2_refine_hip.h: REAL's label refinement, ptv2_pp2s_hip.h: the PP2S label pipeline, ptv2_ptv1_hip.h: Point Transformer
 * V1, ptv2_spconv_hip.h: SpUNet-v1m1, ptv2_pg_hip.h: PointGroup, ptv2_msc_hip.h: Masked Scene Contrast).  Same conventions:
 * device pointers unless stated, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_LAUNCH of
 * ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  No launcher allocates; PTV2_ERR_ARG is returned before
 * anything is enqueued.
 *
 * What it restates (pointcept/models/stratified_transformer/stratified_transformer_v1m2_refine.py and libs/pointops2 of the
 * reference):
 *   cells      :351-364, :394-406.  cell = trunc(((p + shift) - start) / size) per axis in IEEE fp32, nothing contracted; the
 *              "same small window" coordinate of the large-window keys is trunc(((p - start) + half) / size), which is NOT the
 *              same sequence of roundings as the shifted small cell;
 *   pairs      :374-417 as a CSR by query: the points of the query's small window ascending, then the sampled points of its
 *              large window whose window coordinate differs in any axis, ascending;
 *   rel index  :145-151 as the device evaluates them: r = trunc(((rint((ci - cj) * 1e5) * (1 / 1e5) + 2w) - 1e-4) * (1 / quant))
 *              with both reciprocals rounded to fp32 (a division by a python scalar multiplies by its reciprocal on the device);
 *   operators  attention_step1_v2, dot_prod_with_idx_v3, attention_step2_with_rel_pos_value_v2 (libs/pointops2/src/attention_v2,
 *              rpe_v2), without the reference's cap of 1024 pairs per row.
 *
 * Tables are passed TRANSPOSED: (L, h, 3, hd) contiguous, i.e. table.permute(0, 1, 3, 2) of the reference's (L, h, hd, 3), so
 * that the hd values one pair reads per axis are contiguous.  Table gradients come back in the same layout and are ADDED to
 * what the buffer holds (the caller clears it).  They are summed through float atomics and are not bit-repeatable; every
 * other output is written by exactly one group of 16 lanes in a fixed order and is.
 */
#ifndef PTV2_ST_HIP_H
#define PTV2_ST_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ST_MAX_HEADS 64
#define ST_MAX_TABLE_ROWS 256   /* L = 2 * quant_grid_length of one table */
#define ST_KP_POINTS 15         /* kernel points of the stem's KPConv */

/* which operator st_op_hip_launcher runs */
enum {
    ST_OP_STEP1_FWD = 0,    /* attn_out[m, h] = q_i . k_j */
    ST_OP_STEP1_BWD_Q,      /* gq[i] = sum_m g_attn[m] k_j                                             (by query) */
    ST_OP_STEP1_BWD_K,      /* gk[j] = sum_m g_attn[m] q_i                                             (by key)   */
    ST_OP_DOT_FWD,          /* attn_out[m, h] = q_i . tq[rel_m] + k_j . tk[rel_m] */
    ST_OP_DOT_BWD_Q,        /* gq[i] = sum_m g_attn[m] tq[rel_m];  gtq += g_attn[m] q_i                (by query) */
    ST_OP_DOT_BWD_K,        /* gk[j] = sum_m g_attn[m] tk[rel_m];  gtk += g_attn[m] k_j                (by key)   */
    ST_OP_STEP2_FWD,        /* out[i] = sum_m attn[m] (v_j + tv[rel_m]) */
    ST_OP_STEP2_BWD_Q,      /* attn_out[m] = g_out[i] . (v_j + tv[rel_m]);  gtv += attn[m] g_out[i]    (by query) */
    ST_OP_STEP2_BWD_K,      /* gv[j] = sum_m attn[m] g_out[i]                                          (by key)   */
    ST_OP_SOFTMAX_FWD,      /* attn_out[m, h] = softmax over the pairs of one query of attn[m, h] */
    ST_OP_SOFTMAX_BWD,      /* attn_out[m] = attn[m] (g_attn[m] - sum_m' attn[m'] g_attn[m']), attn the softmax's output */
    ST_OP_FUSED_FWD,        /* out, lse of the whole window attention; coords instead of rel */
    ST_OP_FUSED_BWD_Q,      /* gq, gtq, gtv from g_out, lse, delta                                     (by query) */
    ST_OP_FUSED_BWD_K,      /* gk, gv, gtk from g_out, lse, delta                                      (by key)   */
    ST_OP_COUNT
};

/* The operands of every operator; one that an operator does not name may be NULL.  tq[rel_m] stands for
 * sum_a tq[rel[m, a], head, a, :], the sum over the three axes. */
typedef struct st_args {
    int n, h, hd, rows, m;          /* points (queries = keys), heads, channels per head (16 or 32), L, pairs */
    float two_w, inv_q;             /* fused: 2 * window_size and 1 / quant_size, both rounded to fp32 */
    const int *offsets, *index1;    /* (n + 1), (m): the pairs by query */
    const int *t_offsets, *t_query, *t_pair;   /* (n + 1), (m), (m): by key; slot -> query, slot -> pair */
    const int *rel;                 /* (m, 3) */
    const float *coords;            /* (n, 3), fused */
    const float *q, *k, *v;         /* (n, h, hd) */
    const float *tq, *tk, *tv;      /* (L, h, 3, hd) */
    const float *attn, *g_attn;     /* (m, h) */
    const float *g_out, *lse, *delta;   /* (n, h, hd), (n, h), (n, h); delta = sum_d g_out * out */
    float *out, *lse_out;           /* (n, h, hd), (n, h) */
    float *attn_out;                /* (m, h) */
    float *gq, *gk, *gv;            /* (n, h, hd) */
    float *gtq, *gtk, *gtv;         /* (L, h, 3, hd), added to */
} st_args;

/* 1: bumped with any change of a signature, constant or struct of THIS header */
int ptv2_st_abi_version(void);
/* Host only: sizeof(st_args) of the library. */
int ptv2_st_struct_bytes(int which);

/* args: HOST pointer.  An index1 / t_query entry outside [0, n) is skipped; a rel entry is clamped to [0, L).  The operators that
 * accumulate a table gradient keep the head's table slice(s) and 16 rows' sums in LDS: PTV2_ERR_ARG when
 * 4 * tables * 3 L * (hd + 1 + 16) bytes exceed 64 KiB (tables = 2 for ST_OP_FUSED_BWD_Q, else 1). */
int st_op_hip_launcher(int op, const st_args *args, void *stream);

/* coords (n, 3) fp32, start (3) fp32 (device), size the window size.  shift: 0 or 1.
 * cell (n, 3) int32 = trunc(((p + shift * size / 2) - start) / size); wcoord (n, 3) int32 = trunc((p - start) / size) for
 * shift 0 and trunc(((p - start) + size / 2) / size) for shift 1.  Either output may be NULL. */
int st_cells_hip_launcher(int n, const float *coords, const float *start, float size, int shift, int *cell, int *wcoord,
                          void *stream);

/* The pairs of one block.  order_s (n): the points sorted by small cell, ascending index within a cell; seg_s (n, 2): per
 * QUERY the [begin, end) of its small cell in order_s.  order_l (nd): the sampled points sorted by large cell, ascending
 * within a cell; seg_l (n, 2): per query the [begin, end) of its large cell in order_l (begin == end: none).  wcoord (n, 3).
 * fill == 0: counts (n) int32 is written.  fill == 1: offsets (n + 1) is read and index1 (m) written; a slot
 * outside [0, m) is not written. */
int st_pairs_hip_launcher(int n, int nd, int fill, const int *order_s, const int *seg_s, const int *order_l, const int *seg_l,
                          const int *wcoord, int *counts, const int *offsets, int m, int *index1, void *stream);

/* rel (m, 3) int32 of the pairs (index0[m], index1[m]), clamped to [0, rows). */
int st_rel_index_hip_launcher(int n, long long m, int rows, const float *coords, const int *index0, const int *index1,
                              float two_w, float inv_q, int *rel, void *stream);

/* The stem's KPConv (ao_amd/csrc/kpconv.hip): linear influence, sum aggregation.  xyz (n, 3), nbr (n, max_n) int64 with n for an
 * unused slot (anything outside [0, n) contributes nothing), feats (n, cin), kpoints (ST_KP_POINTS, 3), extent > 0.
 * weighted (n, ST_KP_POINTS, cin): sum_m max(0, 1 - |x_nbr(i,m) - x_i - K_k| / extent) feats[nbr(i,m)]; its product with the
 * (ST_KP_POINTS * cin, cout) weight is the caller's. */
int st_kpconv_fwd_hip_launcher(int n, int max_n, int cin, const float *xyz, const long long *nbr, const float *feats,
                               const float *kpoints, float extent, float *weighted, void *stream);
/* g_feats (n, cin) from g_weighted (n, ST_KP_POINTS, cin), gathered by neighbour: t_offsets (n + 1) and t_src (slots) list for
 * every point j the points i that hold j as a neighbour, once per slot, in a fixed order. */
int st_kpconv_bwd_hip_launcher(int n, int cin, long long slots, const float *xyz, const int *t_offsets, const int *t_src,
                               const float *kpoints, float extent, const float *g_weighted, float *g_feats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_ST_HIP_H */
