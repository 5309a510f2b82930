/*
 * include/ptv2_swin_f16_hip.h -- C ABI of Swin3D's window attention with cRSE on half-precision storage in libptv2_hip.so
 * (MI355X / gfx950): the reference's fp16_mode 1, "fp16 forward and fp32 backward" (swin3d_layers.py:399-401, :544-553), as
 * the qkv Linear leaves its output under fp16 autocast.
 *
 * The seventeenth public header of the library (after ptv2_swin_hip.h, whose conventions, constants, window map and layouts it
 * shares).  Written in the subset of C that ao_amd/_abi.py reads; a pointer to
 * half-precision memory is a `void *` here, since that subset has no 16-bit float.
 *
 * The function is that of ptv2_swin_hip.h with these roundings and no others:
 *   qkv (n, 3 C), g_out (n, C)   IEEE binary16, read as the caller wrote them
 *   out (n, C), g_qkv (n, 3 C)   binary16, rounded once (nearest even) at the store
 *   lse (n, h), the three tables and their gradients   fp32
 *   a table value is rounded to binary16 once, where a workgroup stages its head's slice: the forward keeps the slice in LDS
 *   as half, the backward keeps the same rounded values widened to fp32 (it differentiates the function the forward computed)
 *   scale is applied in fp32: to the q . k product after its accumulation, and to q in registers for q . T_Q
 *   everything else is fp32 arithmetic: the row sums, the three logit terms, the softmax, p (v + T_V), delta, dP, dS and every
 *   accumulator.  delta = g_out . out is formed from the half-rounded out.
 * q . k is V_MFMA_F32_16X16X16_F16 in the forward (fp32 accumulation of exact half products) and the fp32 tile of
 * ptv2_swin_hip.h in the backward.  Repeatability is that of ptv2_swin_hip.h: out, lse and g_qkv bit for bit, the table
 * gradients not.
 */
#ifndef PTV2_SWIN_F16_HIP_H
#define PTV2_SWIN_F16_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SWIN_F16_MAX_GROUPS 3       /* SWIN_MAX_GROUPS of ptv2_swin_hip.h; the limits on h, hd, the window and R are that header's */

/* The operands of both launchers; the backward's may be NULL for the forward. */
typedef struct swin_f16_args {
    int n, windows;                     /* voxels; windows of the map */
    int c, h, hd;                       /* channels, heads, channels per head (8 or 16); c == h * hd */
    int groups;                         /* 1 .. 3: signals has 3 * groups columns */
    int rows[SWIN_F16_MAX_GROUPS];      /* L_s of each group */
    float scale;
    const int *order, *offsets;         /* (n), (windows + 1) */
    const float *signals;               /* (n, 3 * groups) fp32, sorted order */
    const void *qkv;                    /* (n, 3 c) half */
    const float *q_table, *k_table, *v_table;   /* (R, h, hd) fp32 each */
    const void *g_out;                  /* (n, c) half */
    void *out;                          /* (n, c) half: written by the forward, read by the backward */
    float *lse;                         /* (n, h) fp32: likewise */
    void *g_qkv;                        /* (n, 3 c) half: written, not added to */
    float *g_q_table, *g_k_table, *g_v_table;   /* (R, h, hd) fp32: written, not added to */
    void *workspace;                    /* the backward's delta and partial table gradients */
    long long workspace_bytes;
} swin_f16_args;

/* 1: bumped with any change of a signature, constant or struct of THIS header */
int ptv2_swin_f16_abi_version(void);
/* Host only: sizeof(swin_f16_args) of the library. */
int ptv2_swin_f16_struct_bytes(int which);
/* Host only: what swin_attention_f16_bwd_hip_launcher needs behind `workspace`: delta (n, h) and one fp32 (3, R, hd) partial per
 * workgroup of the largest grid it launches.  -1 for arguments outside the supported set. */
long long ptv2_swin_f16_workspace_bytes(int n, int windows, int h, int hd, int table_rows);
/* Host only, needs the device: the workgroups of the forward kernel of (hd, groups) that the current device holds at once with
 * the LDS of table_rows rows -- what the forward launcher sizes its grid from, before its cap (tools/bench_swin3d.py reports it
 * per compute unit).  -1 for arguments outside the supported set or when the runtime refuses the LDS. */
int ptv2_swin_f16_fwd_resident_blocks(int hd, int groups, int table_rows);

/* args: HOST pointer.  out and lse from n, windows, c, h, hd, groups, rows, scale, order, offsets, signals, qkv and the three
 * tables.  PTV2_ERR_ARG unless hd in {8, 16}, 1 <= h <= SWIN_MAX_HEADS, c == h * hd, 1 <= groups <= SWIN_F16_MAX_GROUPS,
 * rows[s] >= 1 and R <= SWIN_MAX_ROWS. */
int swin_attention_f16_fwd_hip_launcher(const swin_f16_args *args, void *stream);
/* g_qkv and the three table gradients from the forward's operands, out, lse and g_out; workspace of
 * ptv2_swin_f16_workspace_bytes. */
int swin_attention_f16_bwd_hip_launcher(const swin_f16_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_SWIN_F16_HIP_H */
