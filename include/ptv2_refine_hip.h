/*
 * include/ptv2_refine_hip.h -- C ABI of REAL's epoch-end label refinement in libptv2_hip.so (MI355X / gfx950).
 *
 * The third public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation).  Same
 * conventions: device pointers unless stated, caller-owned workspace, `void *stream` is a hipStream_t, int status return
 * (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that
 * ao_amd/_abi.py reads.  PTV2_ERR_ARG is returned before anything is enqueued: c outside [PTV2_REFINE_MIN_C,
 * PTV2_REFINE_MAX_C], n < 0 or n > INT_MAX, a NULL where one is not allowed.
 *
 * What it restates: pointcept/engines/train_sam_real.py:332-391 (prediction, confidence, grid prompts), :453-472 (mask
 * votes), :488-512 (label update).  The mask predictor (SAM) is the caller's.
 *
 * `status` is a caller-owned, caller-zeroed device array of PTV2_REFINE_STATUS_WORDS ints that the kernels of one scene
 * share.  A value derived from input data that would index outside an array is never dereferenced: the element is skipped
 * and a PTV2_REFINE_BAD_* bit is or-ed into status[PTV2_REFINE_STATUS_ERROR].
 */
#ifndef PTV2_REFINE_HIP_H
#define PTV2_REFINE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PTV2_REFINE_MIN_C 2
#define PTV2_REFINE_MAX_C 32

#define PTV2_REFINE_STATUS_WORDS 4
enum {
    PTV2_REFINE_STATUS_ERROR = 0, /* PTV2_REFINE_BAD_* bits */
    PTV2_REFINE_STATUS_PROMPTS,   /* written by refine_prompts_hip_launcher: the number of prompts */
    PTV2_REFINE_STATUS_UPDATED    /* refine_update_hip_launcher adds the number of labels it changed */
};
#define PTV2_REFINE_BAD_PIXEL 1    /* a visible point's (u, v) outside [0, height] x [0, width] */
#define PTV2_REFINE_BAD_CLASS 2    /* a pred outside [-1, c) or a prompt class outside [0, c) */
#define PTV2_REFINE_BAD_CAPACITY 4 /* more prompts than `capacity` */

/* 1: bumped with any change of a signature or constant of THIS header */
int ptv2_refine_abi_version(void);

/* Bytes of workspace that refine_prompts_hip_launcher (cells = nx * ny) and refine_vote_hip_launcher (prompts) need for
 * these sizes: the larger of the two; -1 for an argument error. */
long long refine_workspace_bytes(long long n, int c, long long cells, int prompts);

/* pred[i] = first maximal class of logits[i, :], -1 where logits[i, 0] == -100 (a row the basket never saw);
 * conf[i] = top-two margin of the fp32 softmax exp(x - max) / sum.  logits (n, c) fp32.  No launch for n == 0. */
int refine_confidence_hip_launcher(long long n, int c, const float *logits, int *pred, float *conf, void *stream);

/* One prompt per (cell, class) of an nx x ny grid over x / y: the point of the largest conf (the lowest index among equals)
 * with pred == class, present[class], label != class and conf > threshold.  Cell (ix, iy) holds the points with
 * b(lo_x, ix) < x < b(lo_x, ix + 1) and b(lo_y, iy) < y < b(lo_y, iy + 1), b(lo, i) = lo + (float)(i * grid) in fp32.
 * prompt_idx / prompt_cls (capacity ints each) receive the prompts in (ix, iy, class) order, status[.._PROMPTS] their number.
 * coord (n, 3) fp32; present: c bytes.  nx == 0 or ny == 0: no launch over the table, a count of 0. */
int refine_prompts_hip_launcher(long long n, int c, const float *coord, const int *pred, const float *conf, const int *label,
                                const void *present, float lo_x, float lo_y, int nx, int ny, double grid, float threshold,
                                void *workspace, long long workspace_bytes, int capacity, int *prompt_idx, int *prompt_cls,
                                int *status, void *stream);

/* One view.  bridge (n, 3) int32 = (u, v, visible); point i is inside mask p when visible == 1 and
 * masks[p][wrap(u - 1)][wrap(v - 1)] != 0 and that element is not [0][0]; wrap(-1) is the last row / column.  When the
 * most frequent pred (the smallest among equals) over the inside points with conf > threshold is prompt_cls[p],
 * vote[i][prompt_cls[p]] += 1 for every inside point.  masks: (prompts, height, width) bytes; vote (n, c) int32,
 * accumulated.  No launch for n == 0 or prompts == 0. */
int refine_vote_hip_launcher(long long n, int c, const int *bridge, const int *pred, const float *conf, int prompts,
                             const int *prompt_cls, const void *masks, int height, int width, float threshold,
                             void *workspace, long long workspace_bytes, int *vote, int *status, void *stream);

/* result = first maximal class of vote[i, :]; where the votes are not all zero, result == pred[i] and pred[i] != -1:
 * status[.._UPDATED] += (label[i] != result), label[i] = result. */
int refine_update_hip_launcher(long long n, int c, const int *vote, const int *pred, int *label, int *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_REFINE_HIP_H */
