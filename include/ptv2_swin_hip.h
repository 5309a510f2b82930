/*
 * include/ptv2_swin_hip.h -- C ABI of Swin3D's window attention with contextual relative signal encoding (cRSE; Swin3D-v1m1) in
 * libptv2_hip.so (MI355X / gfx950): the window map of a voxel list and the fused sparse window attention, forward and backward.
 *
 * The sixteenth public header of the library (after ptv2_spv_hip.h).  Same conventions as ptv2_oct_hip.h: device pointers unless
 * stated, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of
 * ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  No launcher allocates; PTV2_ERR_ARG is returned before
 * anything is enqueued.
 *
 * What it restates (pointcept/models/swin3d/swin3d_layers.py of the reference):
 *   window map  :714-843.  The window of a voxel is floor_div(grid_coord + shift, window_size) per axis with the cloud as a
 *               fourth axis; its slot is w_w_xyz = (grid_coord + shift) mod window_size (never negative), w_w_id =
 *               x ws^2 + y ws + z.  The sort key is cloud << 48 | wx << 35 | wy << 22 | wz << 9 | w_w_id with the window
 *               coordinates biased by SWIN_WINDOW_BIAS, so one ascending sort orders the voxels by window, then by slot.
 *   attention   :432-470, :502-568 and the Swin3D paper; the extension that defines it is NOT available, so this is a restatement
 *               that is not checked against it.  For i, j of one window, head h, q already multiplied by scale, signal axis d
 *               of group s = d / 3 with L = rows[s]:
 *                   r_d(i, j) = clamp(floor(signals[i, d] - signals[j, d]) + L, 0, 2 L - 1)      (one fp32 subtraction)
 *                   T_X(i, j) = sum_d X_table[row0_d + r_d(i, j), h, :],   row0_d = sum_{s' < s} 6 rows[s'] + (d % 3) 2 L
 *                   e_ij = q_i . k_j + q_i . T_Q(i, j) + k_j . T_K(i, j),   p_i. = softmax_j e_ij over the window,
 *                   out_i = sum_j p_ij (v_j + T_V(i, j)).
 *
 * Layouts: qkv (n, 3 C) fp32 exactly as the qkv Linear wrote it, columns [3][h][hd], rows in the voxels' ORIGINAL order; order (n)
 * maps a sorted position to its original row; offsets (windows + 1) is a CSR over sorted positions; signals (n, 3 groups) in
 * SORTED order; each table is the flat concatenation of its groups' (3, 2 L_s, h, hd) blocks, which is (R, h, hd) with
 * R = sum_s 6 rows[s]; out (n, C), lse (n, h), g_qkv (n, 3 C) in original order; the table gradients in the tables' layout.
 *
 * out, lse and g_qkv are written once by one wavefront in a fixed order and are bit-repeatable.  The table gradients are
 * accumulated per workgroup in LDS with atomic adds, one partial per workgroup, and the partials are summed in a fixed order:
 * the LDS adds are not ordered, so the table gradients are not bit-repeatable (ptv2_st_hip.h, ptv2_oct_hip.h accept the same).
 */
#ifndef PTV2_SWIN_HIP_H
#define PTV2_SWIN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SWIN_MAX_WINDOW 7          /* window_size: a window has at most 343 members, w_w_id fits the 9 slot bits of the key */
#define SWIN_MAX_HEADS 64
#define SWIN_MAX_GROUPS 3          /* signal groups: position, colour, normal */
#define SWIN_MAX_ROWS 400          /* R = sum_s 6 rows[s]: six (R, 16) fp32 slices fill 150 KB of the 160 KB of LDS */
#define SWIN_WINDOW_BIAS 4096      /* window coordinates lie in [-4096, 4096) */
#define SWIN_MAX_CLOUDS 32768

/* The operands of every launcher; one that a launcher does not name may be NULL. */
typedef struct swin_args {
    int n, windows;                     /* voxels; windows of the map */
    int c, h, hd;                       /* channels, heads, channels per head (8 or 16); c == h * hd */
    int window_size, shift;
    int groups;                         /* 1 .. 3: signals has 3 * groups columns */
    int rows[SWIN_MAX_GROUPS];          /* L_s of each group */
    float scale;
    const int *grid_coord, *batch;      /* (n, 3), (n): the voxels as given */
    long long *keys_out;                /* (n): swin_map_keys_hip_launcher */
    const long long *keys;              /* (n): sorted ascending */
    int *head_out, *w_w_xyz_out;        /* (n), (n, 3): swin_map_heads_hip_launcher */
    const int *head, *wid;              /* (n): 1 at the first voxel of a window; the inclusive scan of head */
    int *offsets_out;                   /* (n + 1): the first windows + 1 entries are written */
    int *stat;                          /* (4): bad coordinate or cloud id, duplicate voxel, windows, largest window */
    const int *order, *offsets;         /* (n), (windows + 1) */
    const float *signals;               /* (n, 3 * groups), sorted order */
    const float *qkv;                   /* (n, 3 c) */
    const float *q_table, *k_table, *v_table;   /* (R, h, hd) each */
    const float *g_out;                 /* (n, c) */
    float *out, *lse;                   /* (n, c), (n, h): written by the forward, read by the backward */
    float *g_qkv;                       /* (n, 3 c): written, not added to */
    float *g_q_table, *g_k_table, *g_v_table;   /* (R, h, hd): written, not added to */
    void *workspace;                    /* the backward's delta and partial table gradients */
    long long workspace_bytes;
} swin_args;

/* 1: bumped with any change of a signature, constant or struct of THIS header */
int ptv2_swin_abi_version(void);
/* Host only: sizeof(swin_args) of the library. */
int ptv2_swin_struct_bytes(int which);
/* Host only: what swin_attention_bwd_hip_launcher needs behind `workspace`: delta (n, h) and one (3, R, hd) partial per
 * workgroup of the largest grid it launches.  -1 for arguments outside the supported set. */
long long ptv2_swin_workspace_bytes(int n, int windows, int h, int hd, int table_rows);

/* args: HOST pointer in every launcher below.
 * keys_out from n, window_size, shift, grid_coord, batch; stat[0] is set where a window coordinate leaves
 * [-SWIN_WINDOW_BIAS, SWIN_WINDOW_BIAS) or a cloud id [0, SWIN_MAX_CLOUDS).  stat must be zero on entry.  1 <= window_size <=
 * SWIN_MAX_WINDOW. */
int swin_map_keys_hip_launcher(const swin_args *args, void *stream);
/* head_out and w_w_xyz_out from n, window_size and the sorted keys; stat[1] is set where two keys are equal. */
int swin_map_heads_hip_launcher(const swin_args *args, void *stream);
/* offsets_out, stat[2] = windows and stat[3] = the largest window from n, head and wid. */
int swin_map_offsets_hip_launcher(const swin_args *args, void *stream);

/* out and lse from n, windows, c, h, hd, groups, rows, scale, order, offsets, signals, qkv and the three tables.  PTV2_ERR_ARG
 * unless hd in {8, 16}, 1 <= h <= SWIN_MAX_HEADS, c == h * hd, 1 <= groups <= SWIN_MAX_GROUPS, rows[s] >= 1 and
 * R <= SWIN_MAX_ROWS. */
int swin_attention_fwd_hip_launcher(const swin_args *args, void *stream);
/* g_qkv and the three table gradients from the forward's operands, out, lse and g_out; workspace of
 * ptv2_swin_workspace_bytes. */
int swin_attention_bwd_hip_launcher(const swin_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_SWIN_HIP_H */
