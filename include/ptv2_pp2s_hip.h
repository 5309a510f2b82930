/*
 * include/ptv2_pp2s_hip.h -- C ABI of the PP2S label pipeline in libptv2_hip.so (MI355X / gfx950): bridges between a room's
 * points and its camera views, one weak label per instance, and the propagation of those labels through the mask
 * predictor's masks.
 *
 * The fourth public header of the library (ptv2_hip.h: model / pointops, ptv2_data_hip.h: training augmentation,
 * ptv2_refine_hip.h: REAL's label refinement).  Same conventions: device pointers unless stated, caller-owned workspace,
 * `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG, PTV2_ERR_WORKSPACE, PTV2_ERR_LAUNCH of
 * ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.  PTV2_ERR_ARG is returned before anything is
 * enqueued: n < 0 or n > INT_MAX, c outside [PTV2_PP2S_MIN_C, PTV2_PP2S_MAX_C], an image without pixels, a bound above
 * PTV2_PP2S_MAX_BOUND, a NULL where one is not allowed.  No launcher launches anything for n == 0.
 *
 * What it restates: pointcept/utils/my_make_bridge_final.py:94-96 (alignment), :128-153 (one view's bridge),
 * my_choose_weak_label_final.py:59-88 (the weak mask), my_run_sam_final.py:83-114 (the votes of one view) and :47-60,
 * :117-122 (the labels).  The mask predictor (SAM) is the caller's.
 *
 * `status` is a caller-owned, caller-zeroed device array of PTV2_PP2S_STATUS_WORDS ints that the kernels of one room share.
 * A value derived from input data that would index outside an array is never dereferenced: the element is skipped and a
 * PTV2_PP2S_BAD_* bit is or-ed into status[PTV2_PP2S_STATUS_ERROR].
 */
#ifndef PTV2_PP2S_HIP_H
#define PTV2_PP2S_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PTV2_PP2S_MIN_C 2
#define PTV2_PP2S_MAX_C 32 /* a point's classes are one bit each of a 32-bit word */
#define PTV2_PP2S_MAX_BOUND 65535 /* the reference stores pixel coordinates as uint16 */

#define PTV2_PP2S_STATUS_WORDS 4
enum {
    PTV2_PP2S_STATUS_ERROR = 0, /* PTV2_PP2S_BAD_* bits */
    PTV2_PP2S_STATUS_VISIBLE    /* pp2s_project_hip_launcher adds the number of points the view sees */
};
#define PTV2_PP2S_BAD_PIXEL 1 /* a pixel outside the depth image (projection) or outside [0, width] x [0, height] (votes) */
#define PTV2_PP2S_BAD_CLASS 2 /* a prompt label outside [0, c) */

/* 1: bumped with any change of a signature or constant of THIS header */
int ptv2_pp2s_abi_version(void);

/* Bytes of workspace that pp2s_weak_hip_launcher (n points) and the pair pp2s_pixel_labels_hip_launcher /
 * pp2s_vote_hip_launcher (a height x width image) need for these sizes: the larger of the two; -1 for an argument error.
 * height == 0 or width == 0: no image. */
long long pp2s_workspace_bytes(long long n, int height, int width);

/* The room's alignment.  coord (n, 3) fp32, out (n, 3) fp64.  Per point, rounding for rounding as numpy on a float32 array:
 *   t = (float)((double)coord - center)        the float64 difference, rounded to float32
 *   out.x = fma(t.y, -sin, t.x * cos) + cx,   out.y = fma(t.y, cos, t.x * sin) + cy,   out.z = t.z + cz      in float64:
 * the product of t.x rounded, the product of t.y fused into the sum (the chain over k of a dgemm kernel with fused
 * multiply-add, which is what numpy's `coord @ rot_t.T` runs), the centre added with a rounding of its own. */
int pp2s_align_hip_launcher(long long n, const float *coord, double cx, double cy, double cz, double rot_cos, double rot_sin,
                            double *out, void *stream);

/* One view.  coord64 (n, 3) fp64; krt = K * RT and rt = RT, 3 x 4 row-major, by value; depth (depth_h, depth_w) fp64;
 * `height` = 2 K[0][2] - 1 bounds the first pixel coordinate and `width` = 2 K[1][2] - 1 the second (the reference's names).
 * A row m of a matrix times the point is ((m[0] * x + m[1] * y) + m[2] * z) + m[3], every product and sum rounded on its own.
 *   p = krt * (x, y, z, 1),  rx = rint(p.x / p.z),  ry = rint(p.y / p.z)      (round half to even)
 *   valid:    rx > 0, ry > 0, rx < height, ry < width      (a NaN or an infinity is not valid; points behind the camera are
 *                                                           not filtered: the depth test disposes of them)
 *   visible:  valid and |depth[(int)ry][(int)rx] - (rt[2] * (x, y, z, 1))| < tol
 * bridge (n, 3) int32 = (rx, ry, 1) for a visible point, (0, 0, 0) otherwise -- the layout refine_vote_hip_launcher takes;
 * seen_any[i] = 1 for a visible point (n bytes, otherwise untouched; may be NULL);
 * status[PTV2_PP2S_STATUS_VISIBLE] += the number of visible points.
 * A valid pixel outside the depth image is not read: the point is not visible and PTV2_PP2S_BAD_PIXEL is set. */
int pp2s_project_hip_launcher(long long n, const double *coord64, double k00, double k01, double k02, double k03, double k10,
                              double k11, double k12, double k13, double k20, double k21, double k22, double k23, double r00,
                              double r01, double r02, double r03, double r10, double r11, double r12, double r13, double r20,
                              double r21, double r22, double r23, const double *depth, int depth_h, int depth_w, double height,
                              double width, double tol, int *bridge, void *seen_any, int *status, void *stream);

/* One weak point per instance.  instance (n,) int32, any values (-1 is an instance like any other); seen_any n bytes; weak n
 * bytes, zeroed here.  For an instance with at least one seen point: the seen point of rank count_seen / 2 among its seen
 * points in ascending index; for any other instance: the point of rank count / 2 among all its points.  A radix sort of
 * (instance, index) keys, a scan of the seen flags in that order, a selection at the segment heads: the result does not
 * depend on execution order. */
int pp2s_weak_hip_launcher(long long n, const int *instance, const void *seen_any, void *weak, void *workspace,
                           long long workspace_bytes, void *stream);

/* One view, pass A.  masks (prompts, height, width) bytes; prompt_label (prompts,) int32.  Writes the (height, width) uint32
 * image pixbits[h][w] = OR over the prompts p with masks[p][h][w] != 0 of (1u << prompt_label[p]) to the start of the
 * workspace.  A label outside [0, c) contributes nothing and sets PTV2_PP2S_BAD_CLASS.  prompts == 0: an image of zeros.
 * masks[p][0][0] is NOT cleared (REAL's refinement clears it, my_run_sam_final.py does not). */
int pp2s_pixel_labels_hip_launcher(int prompts, int c, const int *prompt_label, const void *masks, int height, int width,
                                   void *workspace, long long workspace_bytes, int *status, void *stream);

/* One view, pass B, on the workspace pass A filled.  bridge (n, 3) int32 = (u, v, visible); for visible == 1:
 * seen_bits[i] |= pixbits[wrap(v - 1)][wrap(u - 1)], wrap(-1) the last row / column (the script swaps the bridge's first two
 * columns and indexes [b0 - 1][b1 - 1] with python integers).  u outside [0, width] or v outside [0, height]: skipped,
 * PTV2_PP2S_BAD_PIXEL.  seen_bits (n,) uint32, accumulated over the views. */
int pp2s_vote_hip_launcher(long long n, const int *bridge, int height, int width, const void *workspace,
                           long long workspace_bytes, unsigned *seen_bits, int *status, void *stream);

/* label[i] = the class whose bit is the only one set in seen_bits[i], -1 for no bit or several; then label[i] = gt[i] where
 * weak[i] != 0 and gt[i] != -1, whether or not any view saw the point.  gt, label (n,) int32; weak n bytes. */
int pp2s_labels_hip_launcher(long long n, const unsigned *seen_bits, const void *weak, const int *gt, int *label,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_PP2S_HIP_H */
