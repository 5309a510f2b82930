/*
 * include/ptv2_spconv_hip.h -- C ABI of the sparse 3D convolutions of SpUNet-v1m1 in libptv2_hip.so (MI355X / gfx950): the
 * neighbour tables of a voxelised batch and the gather / scatter / stem / weight-gradient forms of a convolution over them.
 *
 * The sixth public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation,
 * ptv2_refine_hip.h: REAL's label refinement, ptv2_pp2s_hip.h: the PP2S label pipeline, ptv2_ptv1_hip.h: Point Transformer
 * V1).  Same conventions: device pointers unless stated, caller-owned workspace, `void *stream` is a hipStream_t, int status
 * return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that
 * ao_amd/_abi.py reads.  spconv_tables is a HOST struct of device pointers, read during the call.  PTV2_ERR_ARG is returned
 * before anything is enqueued.
 *
 * What it restates (spconv 2.x's published semantics; DESIGN.md section 11 lists the assumptions):
 *   a weight is (Cout, k, k, k, Cin) fp32 (KRSC), the kernel axes follow the columns of the voxel coordinate, kappa is the
 *   row-major index of the kernel offset, a cross-correlation;
 *   SubMConv3d(k):           out[i] = sum over kappa of W[kappa] in[nbr[i][kappa]],  nbr[i][kappa] the row of the voxel at
 *                            coord[i] + (kappa - k / 2) in the same cloud, or -1;
 *   SparseConv3d(2, 2):      out[o] = sum over kappa of W[kappa] in[child[o][kappa]], o the coarse voxel coord >> 1,
 *                            kappa = coord - 2 (coord >> 1);
 *   SparseInverseConv3d(2):  out[child[o][kappa]] = W[kappa] in[o].
 * Level l + 1 holds one voxel per occupied coord >> 1 of level l, in ascending (cloud, x, y, z) order; level 0 is the
 * caller's rows in the caller's order.
 *
 * Memory: no buffer of n * K * C elements exists in either direction.  The launchers read integer tables and (n, C) float
 * rows; the weight gradient's workspace holds K * splits * Cout * Cin partial sums, splits <= SPCONV_MAX_SPLITS whatever n.
 * Every sum has a fixed order and no launcher uses an atomic: two calls on the same inputs give the same bits.
 */
#ifndef PTV2_SPCONV_HIP_H
#define PTV2_SPCONV_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SPCONV_LEVELS 5       /* level 0 and four downsamplings */
#define SPCONV_COORD_BITS 18  /* a voxel coordinate lies in [0, 2^18) */
#define SPCONV_MAX_CLOUDS 1024
#define SPCONV_MAX_SPLITS 8   /* row splits of the weight gradient */
#define SPCONV_MAX_K 125

/* the status array: word log2(bit) is set to 1 (a plain store, no atomic) */
#define SPCONV_BAD_NEGATIVE 1   /* a negative coordinate */
#define SPCONV_BAD_LARGE 2      /* a coordinate >= 2^SPCONV_COORD_BITS */
#define SPCONV_BAD_DUPLICATE 4  /* two rows of one cloud on one voxel */
#define SPCONV_STATUS_WORDS 3

/* forms of spconv_conv_hip_launcher */
#define SPCONV_GATHER 0   /* out[r] = sum over kappa of W[kappa] in[tab[r][kappa]] */
#define SPCONV_SCATTER 1  /* out[tab[r][kappa]] = W[kappa] in[r] */

/* Everything one forward needs, written by spconv_build_tables_hip_launcher.  Every array has room for n rows (n the number
 * of level-0 rows); the first counts[l] rows of level l are valid, counts[0] = n. */
typedef struct spconv_tables {
    int *nbr5;                        /* (n, 125): the stem's k = 5 table of level 0 */
    int *nbr3[SPCONV_LEVELS];         /* (n_l, 27) */
    int *child[SPCONV_LEVELS - 1];    /* (n_{l+1}, 8): the rows of level l under a voxel of level l + 1, or -1 */
    int *parent[SPCONV_LEVELS - 1];   /* (n_l): the row of level l + 1 above a row of level l */
    int *slot[SPCONV_LEVELS - 1];     /* (n_l): its column in child */
    int *coord[SPCONV_LEVELS - 1];    /* (n_{l+1}, 3): the coordinates of level l + 1 */
    int *offset[SPCONV_LEVELS - 1];   /* (b): the cloud ends of level l + 1 */
    int *counts;                      /* (SPCONV_LEVELS): n_l */
    int *status;                      /* (SPCONV_STATUS_WORDS): zeroed by the caller */
} spconv_tables;

/* 1: bumped with any change of a signature, struct or constant of THIS header */
int ptv2_spconv_abi_version(void);
/* sizeof of spconv_tables (0) as compiled; -1 otherwise */
int ptv2_spconv_struct_bytes(int which);

/* Host only.  Workspace bytes of the table build for n rows in b clouds; -1 for an argument error. */
long long ptv2_spconv_tables_workspace_bytes(long long n, int b);
/* Host only.  Workspace bytes of a convolution over a table of n rows and k columns (the weight gradient's partial sums; the
 * other forms need none); -1 for an argument error.  Does not grow with n beyond SPCONV_MAX_SPLITS splits. */
long long ptv2_spconv_workspace_bytes(long long n, int k, int cin, int cout);

/* coord (n, 3) int32, offset (b) int32 cloud ends (ascending, the last is n).  1 <= n, 1 <= b <= SPCONV_MAX_CLOUDS.  A bad
 * coordinate is clamped into range and recorded in *status: the tables are then not to be used, and no kernel indexes
 * outside a buffer.  Reads nothing back. */
int spconv_build_tables_hip_launcher(int n, int b, const int *coord, const int *offset, const spconv_tables *tables,
                                     void *workspace, long long workspace_bytes, void *stream);

/* The convolution over a table tab (n_tab, k) with entries in [-1, n_other).  weight (Cout, k, Cin).
 * form SPCONV_GATHER:  in (n_other, cin_eff), out (n_tab, cout_eff);  SPCONV_SCATTER: in (n_tab, cin_eff), out (n_other,
 * cout_eff), every row of out must appear exactly once in tab.
 * transpose == 0: cin_eff = Cin, cout_eff = Cout; transpose != 0: the transposed matrices W[kappa]^T, cin_eff = Cout,
 * cout_eff = Cin (the input gradients).  reverse != 0: column kappa of tab is read as column k - 1 - kappa (the input
 * gradient of a submanifold convolution over its own table; SPCONV_GATHER only).  Cin and Cout are multiples of 32, k <= 27. */
int spconv_conv_hip_launcher(int form, int n_tab, int n_other, int k, int cin, int cout, const float *in, const int *tab,
                             const float *weight, int transpose, int reverse, float *out, void *stream);

/* gW[co][kappa][ci] = sum over r of g[gr][co] x[xr][ci], j = tab[r][kappa] >= 0, (gr, xr) = (r, j), or (j, r) when
 * gather_g != 0; tab (n_tab, k) with entries in [-1, n_other).  x has Cin columns, g has Cout.  Cin and Cout multiples of 32,
 * or Cin <= 16 (the stem, any Cout multiple of 32).  Every element of gW is written; the sum runs in row order within
 * each of the splits and then over the splits, whose number depends on n_tab alone. */
int spconv_wgrad_hip_launcher(int n_tab, int n_other, int k, int cin, int cout, const float *x, const float *g, const int *tab,
                              int gather_g, float *gW, void *workspace, long long workspace_bytes, void *stream);

/* The stem: the gather form for Cin <= 16 and Cout 32 or 64 with k * Cin * Cout * 4 <= 147456 bytes of LDS.  transpose == 0:
 * out (n, Cout) from in (n, Cin); transpose != 0: the input gradient, out (n, Cin) from in (n, Cout) with the table's
 * columns reversed. */
int spconv_stem_hip_launcher(int n, int k, int cin, int cout, const float *in, const int *tab, const float *weight,
                             int transpose, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_SPCONV_HIP_H */
