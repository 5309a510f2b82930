/*
 * include/ptv2_octconv_hip.h -- C ABI of OctFormer's dense octree convolutions (OctFormer-v1m1: the stem, Downsample and the
 * decoder) in libptv2_hip.so (MI355X / gfx950): the tables between two neighbouring octree depths and one fp32 matrix-core
 * gather-GEMM that is the forward, the input gradient and (with a second kernel) the weight gradient of all three layers.
 *
 * The eighteenth public header of the library (after ptv2_swin_f16_hip.h).  Same conventions as ptv2_oct_hip.h: device
 * pointers unless stated, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE,
 * PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  No launcher allocates; PTV2_ERR_ARG is
 * returned before anything is enqueued.
 *
 * The one form:
 *   out[i, :] (cout) = bias + sum over s < slots with j = tab[i, reverse ? slots - 1 - s : s] >= 0 of x[j, :] (cin) . W[s]
 * W[s] is (cin, cout) row-major, or with `transpose` (cout, cin) row-major read as its transpose.  ocnn's OctreeConv keeps
 * `weights` as (slots, Cin, Cout) and OctreeDeconv as (slots, Cout, Cin) (restated from its documentation; unpinned):
 *   layer                      forward                         input gradient
 *   k = 3, stride 1            tab = nbr                       tab = nbr, reverse, transpose
 *   k = 2, stride 2 (+ bias)   tab = child (8 slots)           tab = onehot (8 slots), transpose
 *   k = 3, stride 2 deconv     tab = up, transpose             tab = down3
 * The weight gradient is g_w[s] (cin, cout) = sum_i x[tab[i, s], :]^T g[i, :], stored (cout, cin) with `transpose`.
 *
 * Tables between the children (depth d, n rows) and the parents (depth d - 1, n_parent rows), both in (cloud, Morton key)
 * order, where the children of a parent are consecutive; octant o = key & 7 = 4 (x & 1) + 2 (y & 1) + (z & 1):
 *   parent (n)            the row of the parent
 *   child  (n_parent, 8)  the row of the child in octant o, or -1
 *   onehot (n, 8)         parent[j] in column o_j, -1 elsewhere: the transpose of `child`
 *   up     (n, 27)        entry k = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1): the parent q with 2 q + (dx, dy, dz) == xyz_j, or -1
 *   down3  (n_parent, 27) entry k: the child at 2 xyz_p + (dx, dy, dz), or -1: up[j, k] == p exactly when down3[p, k] == j
 *
 * Every output is written by exactly one lane in a fixed order; there are no atomics: two runs give the same bits.
 */
#ifndef PTV2_OCTCONV_HIP_H
#define PTV2_OCTCONV_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define OCTCONV_MAX_CHANNELS 384   /* of either side */
#define OCTCONV_STEM_CHANNELS 8    /* a contraction this narrow need not be a multiple of 4 (raw features) */
#define OCTCONV_MAX_SPLITS 8       /* row splits of the weight gradient: its partials */

/* The operands of the convolution launchers; one that a launcher does not name may be NULL. */
typedef struct octconv_args {
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
} octconv_args;

/* The operands of oct_conv_tables_hip_launcher. */
typedef struct octconv_tables {
    int n, n_parent;
    const long long *keys;              /* (n): the children's Morton keys */
    const int *xyz;                     /* (n, 3): the children's coordinates */
    const int *first;                   /* (n_parent + 1): the first child row of each parent; first[n_parent] == n */
    const int *parent_nbr;              /* (n_parent, 27): the neighbour table of the parents' level */
    int *parent, *child, *onehot;       /* (n), (n_parent, 8), (n, 8) */
    int *up, *down3;                    /* (n, 27), (n_parent, 27) */
} octconv_tables;

/* 1: bumped with any change of a signature, constant or struct of THIS header */
int ptv2_octconv_abi_version(void);
/* Host only: sizeof(octconv_args) for 0, sizeof(octconv_tables) for 1, else -1. */
int ptv2_octconv_struct_bytes(int which);
/* Host only: what oct_conv_gw_hip_launcher needs behind `workspace` (the partials of g_w, then 64 row strips of g_b); -1 for a
 * pair outside the supported set. */
long long ptv2_octconv_workspace_bytes(int n_out, int slots, int cin, int cout);

/* args: HOST pointer in every launcher below.
 * parent, child, onehot from n, n_parent, keys, first (one thread per parent walks its consecutive children: no search); then up
 * (through parent and parent_nbr) and down3 (through parent_nbr and child). */
int oct_conv_tables_hip_launcher(const octconv_tables *args, void *stream);

/* The supported pairs: cin % 4 == 0 and cin <= OCTCONV_MAX_CHANNELS, or 1 <= cin <= OCTCONV_STEM_CHANNELS; cout % 8 == 0 and
 * 8 <= cout <= OCTCONV_MAX_CHANNELS; slots 8 or 27.  All three launchers check the LAYER's pair.
 * out (n_out, cout) from tab, x (n_in, cin), w, bias, transpose, reverse. */
int oct_conv_fwd_hip_launcher(const octconv_args *args, void *stream);
/* The input gradient of a layer: out (n_out, cin) from tab, x = the output's gradient (n_in, cout), w, transpose, reverse as the
 * table above names them (`transpose` describes the read of this launch: cin and cout change places in the one form). */
int oct_conv_gx_hip_launcher(const octconv_args *args, void *stream);
/* g_w from tab (the forward's), x (n_in, cin), g (n_out, cout), transpose; g_b (cout), the column sums of g, if not NULL.
 * workspace of ptv2_octconv_workspace_bytes. */
int oct_conv_gw_hip_launcher(const octconv_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_OCTCONV_HIP_H */
