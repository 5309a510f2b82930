/*
 * include/ptv2_ptv1_hip.h -- C ABI of Point Transformer V1's vector-attention layer in libptv2_hip.so (MI355X / gfx950):
 * forward and backward of everything between the q / k / v Linears and the Bottleneck's bn2.
 *
 * The fifth public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation,
 * ptv2_refine_hip.h: REAL's label refinement, ptv2_pp2s_hip.h: the PP2S label pipeline).  Same conventions: device pointers
 * unless stated, caller-owned workspace, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG,
 * PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  The three structs
 * are HOST structs of device pointers, read during the call.  PTV2_ERR_ARG is returned before anything is enqueued: n < 0,
 * ns outside [1, PTV1_MAX_NS], c not one of 32, 64, 128, 256, 512, training with fewer than two rows, a NULL where one is
 * not allowed.  No launcher launches anything for n == 0.
 *
 * What it restates: pointcept/models/point_transformer/point_transformer_seg.py:45-78, with C = c, I = C / PTV1_SHARE,
 * per point n and slot s (j = idx[n][s], valid = j >= 0):
 *   rel  = valid ? coord[j] - coord[n] : 0                                   (3)
 *   a    = p0_w rel + p0_b                                                   (3)     linear_p.0
 *   h    = ReLU(BN3(a))                                                      (3)     linear_p.1 (a BatchNorm over the n * ns rows)
 *   p_r  = p3_w h + p3_b                                                     (C)     linear_p.3
 *   r    = (valid ? x_k[j] : 0) - x_q[n] + p_r                               (C)
 *   u    = w2_w ReLU(BN_C(r)) + w2_b                                         (I)     linear_w.0, linear_w.2
 *   z    = w5_w ReLU(BN_I(u)) + w5_b                                         (I)     linear_w.3, linear_w.5
 *   w    = softmax of z over the ns slots of the point, per i; -1 slots take part
 *   out[n][c] = sum over s of ((valid ? x_v[j][c] : 0) + p_r[s][c]) * w[s][c % I]
 * Training: the three norms use the biased batch statistics of the call, which are written to `mean*` / `var*`, and update
 * their running buffers (running = (1 - momentum) * running + momentum * batch, the variance unbiased; num_batches_tracked
 * += 1).  Eval: the caller passes the running buffers as `mean*` / `var*`; nothing is written to them.
 *
 * Memory: no buffer of n * ns * C elements exists in either direction.  `saved` holds u and w, (n, ns, I) each; the backward's
 * workspace holds one (n, ns, I) gradient, one (n, ns, 3) gradient and per-workgroup partial records.  r, p_r, x_k[idx] and
 * x_v[idx] are recomputed from x_*, coord and idx wherever they are needed.  Sums across workgroups are fixed-order partial
 * records reduced by a second launch (accumulated in fp64 for the statistics); g x_k and g x_v are fixed-order gathers over the
 * inverse neighbour table.  Two calls on the same inputs give the same bits.
 */
#ifndef PTV2_PTV1_HIP_H
#define PTV2_PTV1_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PTV1_SHARE 8   /* share_planes: I = C / 8 */
#define PTV1_MAX_NS 16
#define PTV1_MIN_C 32
#define PTV1_MAX_C 512

/* the layer's seven parameter groups, fp32, in the reference's layouts (Linear weights (out, in)) */
typedef struct ptv1_params {
    const float *p0_w, *p0_b; /* linear_p.0: (3, 3), (3) */
    const float *p1_g, *p1_b; /* linear_p.1: BN3 weight, bias (3) */
    const float *p3_w, *p3_b; /* linear_p.3: (C, 3), (C) */
    const float *w0_g, *w0_b; /* linear_w.0: BN_C weight, bias (C) */
    const float *w2_w, *w2_b; /* linear_w.2: (I, C), (I) */
    const float *w3_g, *w3_b; /* linear_w.3: BN_I weight, bias (I) */
    const float *w5_w, *w5_b; /* linear_w.5: (I, I), (I) */
} ptv1_params;

/* the three norms: the statistics the layer normalises with, and the running buffers a training forward updates */
typedef struct ptv1_norms {
    float *mean3, *var3; /* (3): written by a training forward, read otherwise */
    float *meanc, *varc; /* (C) */
    float *meani, *vari; /* (I) */
    float *run_mean3, *run_var3, *run_meanc, *run_varc, *run_meani, *run_vari; /* training forward only; NULL: not tracked */
    long long *batches3, *batchesc, *batchesi; /* num_batches_tracked, one int64 each; NULL: not tracked */
} ptv1_norms;

/* the gradient of every parameter, same shapes as ptv1_params; every element is written */
typedef struct ptv1_grads {
    float *p0_w, *p0_b, *p1_g, *p1_b, *p3_w, *p3_b, *w0_g, *w0_b, *w2_w, *w2_b, *w3_g, *w3_b, *w5_w, *w5_b;
} ptv1_grads;

/* 1: bumped with any change of a signature, struct or constant of THIS header */
int ptv2_ptv1_abi_version(void);
/* sizeof of ptv1_params (0), ptv1_norms (1), ptv1_grads (2) as compiled; -1 otherwise */
int ptv2_ptv1_struct_bytes(int which);

/* Host only.  Bytes of `workspace` (the larger of the forward's and the backward's) and of `saved` for these sizes; -1 for an
 * argument error. */
long long ptv1_attention_workspace_bytes(long long n, int ns, int c);
long long ptv1_attention_saved_bytes(long long n, int ns, int c);

/* x_q, x_k, x_v (n, c); coord (n, 3); idx (n, ns) int32, entries in [-1, n); out (n, c).  `saved` is written in both modes
 * and is what the backward takes. */
int ptv1_attention_forward_hip_launcher(int n, int ns, int c, const float *x_q, const float *x_k, const float *x_v,
                                        const float *coord, const int *idx, const ptv1_params *params,
                                        const ptv1_norms *norms, int training, float eps, float momentum, float *out,
                                        void *saved, long long saved_bytes, void *workspace, long long workspace_bytes,
                                        void *stream);

/* The same operands and `norms` (mean* / var* as the forward left or took them), `saved` as the forward wrote it, the inverse
 * table of idx (inverse_table_hip_launcher of ptv2_hip.h), g_out (n, c).  Writes g_xq, g_xk, g_xv (n, c) and every array of
 * `grads`.  training == 0: the gradient of the eval-mode forward (the statistics are constants). */
int ptv1_attention_backward_hip_launcher(int n, int ns, int c, const float *x_q, const float *x_k, const float *x_v,
                                         const float *coord, const int *idx, const int *inv_ptr, const int *inv_rows,
                                         const ptv1_params *params, const ptv1_norms *norms, int training, float eps,
                                         const float *g_out, const void *saved, long long saved_bytes, float *g_xq,
                                         float *g_xk, float *g_xv, const ptv1_grads *grads, void *workspace,
                                         long long workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_PTV1_HIP_H */
