/*
 * include/ptv2_data_hip.h -- C ABI of the device-side training augmentation of libptv2_hip.so (MI355X / gfx950).
 *
 * The second public header of the library (the first, ptv2_hip.h, is the model / pointops boundary).  Same conventions:
 * device pointers unless stated, `void *stream` is a hipStream_t, int status return (PTV2_OK, PTV2_ERR_ARG,
 * PTV2_ERR_LAUNCH of ptv2_hip.h), written in the subset of C that ao_amd/_abi.py reads.
 *
 * What it replaces: the per-point transforms of the reference's training list (pointcept/datasets/transform.py), which run
 * in numpy on CPU workers.  A list of such transforms becomes a PROGRAM: up to PTV2_AUG_MAX_STEPS steps that one kernel
 * runs per point, the coordinate held in double and the colour in fp32 registers.  The python side (ao_amd/ptv2/transform.py)
 * writes the reference's rounding into the program: a PTV2_AUG_ROUND_F32 step after every coordinate step while the
 * reference's array is still float32, none once it is float64 (after its first np.dot rotation).
 */
#ifndef PTV2_DATA_HIP_H
#define PTV2_DATA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PTV2_AUG_MAX_STEPS 16
#define PTV2_AUG_NPARAM 12

/* step kinds; p[] is the step's parameter block */
enum {
    PTV2_AUG_CENTER_SHIFT = 0, /* coord -= ((min+max)/2 of x, of y, z min | 0) read from `bounds`; flags: FP32, APPLY_Z */
    PTV2_AUG_ROTATE,           /* coord = (coord - c) R^T + c; p[0..8] = R row major, p[9..11] = c (or BOUNDS_CENTER) */
    PTV2_AUG_SCALE,            /* coord[d] *= p[d] (a flip is -1) */
    PTV2_AUG_SHIFT,            /* coord[d] += p[d] */
    PTV2_AUG_CLIP,             /* coord[d] = min(max(coord[d], p[d]), p[3 + d]) */
    PTV2_AUG_JITTER,           /* coord[d] += min(max(p[0] * g[d], -p[1]), p[1]), g = the step's normals */
    PTV2_AUG_ELASTIC,          /* coord += p[6] * trilinear(field)(coord); axis d starts at p[d], spacing p[3 + d] */
    PTV2_AUG_ROUND_F32,        /* coord = (double)(float)coord */
    PTV2_AUG_COLOR_CONTRAST,   /* color = (float)p[0] * color + (float)p[1] * ((color - lo) * (255 / (hi - lo))), fp32 */
    PTV2_AUG_COLOR_TRANSLATE,  /* color[d] = (float)min(max(p[d] + color[d], 0), 255), the sum in double */
    PTV2_AUG_COLOR_JITTER,     /* color[d] = (float)min(max(p[0] * g[d] + color[d], 0), 255), in double */
    PTV2_AUG_COLOR_MUL,        /* color *= (float)p[0] */
    PTV2_AUG_KINDS
};

/* step flags.  FP32: the reference's array is float32 here -- the centre is computed in fp32, and ROTATE rounds the centred
 * coordinate to fp32 before the matrix product.  APPLY_Z: CENTER_SHIFT subtracts the z minimum.  BOUNDS_CENTER: ROTATE's
 * c is (min + max) / 2 of `bounds`, not p[9..11]. */
#define PTV2_AUG_FLAG_FP32 1
#define PTV2_AUG_FLAG_APPLY_Z 2
#define PTV2_AUG_FLAG_BOUNDS_CENTER 4

typedef struct ptv2_aug_step {
    int kind;
    int stream;     /* RNG stream number of the step's normals (third Philox counter word) */
    int slot;       /* which [n][3] plane of a caller-supplied noise buffer holds the step's normals */
    int flags;
    double p[PTV2_AUG_NPARAM];
    const float *field; /* ELASTIC: (dims[0], dims[1], dims[2], 3) fp32 displacement grid */
    int dims[3];
    int reserved;
} ptv2_aug_step;

typedef struct ptv2_aug_program {
    int count;         /* steps used, <= PTV2_AUG_MAX_STEPS */
    int coord_in_f64;  /* coord_in is double[n][3], not float[n][3] (the state between two segments of one list) */
    int coord_out_f64; /* coord_out likewise */
    int reserved;
    ptv2_aug_step step[PTV2_AUG_MAX_STEPS];
} ptv2_aug_program;

/* 1: bumped with any change of a signature or struct of THIS header (ptv2_abi_version() covers ptv2_hip.h) */
int ptv2_data_abi_version(void);
long long ptv2_data_struct_bytes(int which); /* 0: ptv2_aug_step, 1: ptv2_aug_program */

/* Runs `program` (host memory, read during the call) once per point, one lane per point.  color_in / color_out may be NULL
 * together (colour steps are then an argument error).  bounds: what aug_bounds_hip_launcher wrote, NULL when no step reads
 * it.  noise: NULL = in-kernel Philox4x32-10 normals, key = the 64 bits of seed, counter = (point lo, point hi, step.stream, 0); else
 * float[slots][n][3], the step's normals at plane step.slot.  In place (coord_out == coord_in of the same type, color
 * likewise) is allowed.  No launch for n == 0. */
int aug_points_hip_launcher(long long n, const ptv2_aug_program *program, const double *bounds, const void *coord_in,
                            const float *color_in, const float *noise, long long seed, void *coord_out,
                            float *color_out, void *stream);

/* bounds[0..2] / [3..5] = per-axis min / max of coord (float[n][3], or double[n][3] when coord_f64), [6..8] / [9..11] of
 * color (untouched when color is NULL), exact and order independent.  bounds has room for 24 doubles: [12..24) is scratch of
 * the call.  n >= 1. */
int aug_bounds_hip_launcher(long long n, const void *coord, int coord_f64, const float *color, double *bounds, void *stream);

/* out[i][0..2] = the three normals the point kernel uses for point i of a step with RNG stream `stream_no` */
int aug_noise_hip_launcher(long long n, long long seed, int stream_no, float *out, void *stream);

/* One 3-tap (1/3, 1/3, 1/3) pass along `axis` (0..2) of a (dx, dy, dz, 3) fp32 grid, zero outside, double accumulation */
int aug_blur3_hip_launcher(int dx, int dy, int dz, int axis, const float *in, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTV2_DATA_HIP_H */
