/*
 * include/ptv2_pg_hip.h -- C ABI of PointGroup's (PG-v1m1) clustering stage in libptv2_hip.so (MI355X / gfx950): the batched
 * ball query, the clustering of its edge lists, the proposals with their scores and masks, and the offset ("bias") losses.
 *
 * The seventh public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation,
 * ptv2_refine_hip.h: REAL's label refinement, ptv2_pp2s_hip.h: the PP2S label pipeline, ptv2_ptv1_hip.h: Point Transformer
 * V1, ptv2_spconv_hip.h: SpUNet-v1m1).  Same conventions: device pointers unless stated, caller-owned workspace, `void *stream`
 * is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in
 * the subset of C that ao_amd/_abi.py reads.  No launcher allocates, every index output is int32, PTV2_ERR_ARG is returned
 * before anything is enqueued.  No float atomic is used anywhere: two calls on the same inputs give the same bits.
 *
 * What it restates (libs/pointgroup_ops and pointcept/models/point_group/point_group_v1m1_base.py of the reference; DESIGN.md
 * section 12):
 *   ball query   for point p of segment [batch_offsets[s], batch_offsets[s + 1]) the indices k of the same segment with
 *                d2(p, k) < radius * radius (strict; p itself included), ascending in k, cut after the first PG_BALL_CAP;
 *                start_len[p] = (start, len), start the exclusive prefix sum of len in point order, n_active their sum;
 *   clustering   no list cut: the connected components of the edges whose two ends carry the same label, those of at least
 *                min_points members kept and numbered in ascending order of their smallest member.  A list cut: the
 *                reference's directed breadth-first search, pg_bfs_cluster_host, on the host;
 *   proposals    the clusters of more than propose_points members, in cluster order: the label of the cluster's first point,
 *                the mean over its members of the class probability, a (P, N) 0 / 1 mask;
 *   offset loss  sum |pred - gt| and -cos(pred, gt) over the rows with instance != ignore, divided by their number + 1e-8.
 */
#ifndef PTV2_PG_HIP_H
#define PTV2_PG_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PG_BALL_CAP 1000     /* entries of one list; the reference's idx_temp[1000] */
#define PG_MAX_CLOUDS 1024
#define PG_MAX_CLASSES 1024

/* The edge lists of a ball query.  A HOST struct, read during the call; idx and start_len are device pointers for
 * pg_cluster_hip_launcher and host pointers for pg_bfs_cluster_host. */
typedef struct pg_csr {
    int *idx;             /* (n_active) */
    int *start_len;       /* (n, 2) */
    long long n_active;
} pg_csr;

/* 1: bumped with any change of a signature, struct or constant of THIS header */
int ptv2_pg_abi_version(void);
/* sizeof of pg_csr (0) as compiled; -1 otherwise */
int ptv2_pg_struct_bytes(int which);

/* Host only.  Workspace bytes of the ball query of n points in b segments: a grid of at most 4 cells per point, whatever the
 * bounding box; -1 for an argument error. */
long long ptv2_pg_ballquery_workspace_bytes(long long n, int b);
/* coords (n, 3) fp32, batch_offsets (b + 1) int32 ascending from 0 to n.  1 <= n, 1 <= b <= PG_MAX_CLOUDS, radius > 0.
 * Builds the grid in the workspace, counts, scans: start_len (n, 2), *n_active, *capped (1 when some point had a
 * (PG_BALL_CAP + 1)-th neighbour, else 0).  Reads nothing back. */
int pg_ballquery_count_hip_launcher(int n, int b, const float *coords, const int *batch_offsets, float radius, int *start_len,
                                    int *n_active, int *capped, void *workspace, long long workspace_bytes, void *stream);
/* The lists: idx (n_active), with the workspace and the start_len pg_ballquery_count_hip_launcher left for the same inputs. */
int pg_ballquery_fill_hip_launcher(int n, int b, const float *coords, const int *batch_offsets, float radius,
                                   const int *start_len, long long n_active, int *idx, void *workspace,
                                   long long workspace_bytes, void *stream);

/* Host only.  Workspace bytes of the clustering of n points; -1 for an argument error. */
long long ptv2_pg_cluster_workspace_bytes(long long n);
/* semantic_label (n) int32, csr the lists of a ball query in which NO list was cut.  point_cluster (n): the cluster of each
 * point or -1; cluster_size (n): the sizes of the first *n_cluster clusters; cluster_first (n): their smallest members. */
int pg_cluster_hip_launcher(int n, const int *semantic_label, const pg_csr *csr, int min_points, int *point_cluster,
                            int *cluster_size, int *cluster_first, int *n_cluster, void *workspace, long long workspace_bytes,
                            void *stream);
/* HOST pointers throughout, no GPU: the reference's search.  Seeds in ascending index, a queue, list entries in list order, an
 * entry followed when its label equals the current point's and it is unvisited; found sets of at least threshold points are
 * kept.  cluster_idxs (n, 2) receives (cluster, point) rows in search order, cluster_offsets (n + 1) the cluster starts and
 * the total, *n_cluster their number.  Returns the number of rows written, or -1 for an argument error (a list outside
 * idx, an entry outside [0, n)). */
long long pg_bfs_cluster_host(int n, const int *semantic_label, const pg_csr *csr, int threshold, int *cluster_idxs,
                              int *cluster_offsets, int *n_cluster);

/* Host only.  Workspace bytes of the proposals of n points in n_cluster clusters; -1 for an argument error. */
long long ptv2_pg_proposals_workspace_bytes(long long n, long long n_cluster);
/* proposal_of_cluster (n_cluster): the proposal of each cluster with cluster_size > propose_points, in cluster order, else -1;
 * *n_proposal their number. */
int pg_proposals_count_hip_launcher(int n_cluster, const int *cluster_size, int propose_points, int *proposal_of_cluster,
                                    int *n_proposal, void *workspace, long long workspace_bytes, void *stream);
/* point_cluster (n) in [-1, n_cluster), cluster_first (n_cluster), segment_pred (n) int64, prob (n, c) fp32 class
 * probabilities, or logits when is_logit != 0 (the softmax is then taken here, in fp32).  classes (n_proposal) int64, scores
 * (n_proposal) fp32, masks (n_proposal, n) int32, every element written; n_proposal <= 65535 (one grid row per proposal).  The
 * sum of a score runs in a fixed order. */
int pg_proposals_fill_hip_launcher(int n, int c, int n_cluster, int n_proposal, const int *point_cluster,
                                   const int *cluster_size, const int *cluster_first, const int *proposal_of_cluster,
                                   const long long *segment_pred, const float *prob, int is_logit, long long *classes,
                                   float *scores, int *masks, void *workspace, long long workspace_bytes, void *stream);

/* Host only.  Workspace bytes of pg_bias_loss_fwd_hip_launcher; -1 for an argument error. */
long long ptv2_pg_bias_loss_workspace_bytes(long long n);
/* bias_pred, coord, instance_center (n, 3) fp32, instance (n) int64.  out (3): bias_l1_loss, bias_cosine_loss, the number of
 * rows with instance != ignore.  Block partial sums, then one block in a fixed order. */
int pg_bias_loss_fwd_hip_launcher(int n, const float *bias_pred, const float *coord, const float *instance_center,
                                  const long long *instance, long long ignore, float *out, void *workspace,
                                  long long workspace_bytes, void *stream);
/* d_bias_pred (n, 3) from the upstream gradients g (2) of the two losses and out of the forward.  sign(0) = 0 in the L1 term,
 * the gradient of the norm at the zero vector is 0, ignored rows get 0. */
int pg_bias_loss_bwd_hip_launcher(int n, const float *bias_pred, const float *coord, const float *instance_center,
                                  const long long *instance, long long ignore, const float *out, const float *g,
                                  float *d_bias_pred, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_PG_HIP_H */
