// ao_amd/csrc/augment.hip -- the per-point training augmentations of the input pipeline in one pass (gfx950),
// include/ptv2_data_hip.h.  What pointcept/datasets/transform.py does to `coord` and `color` with one numpy statement per
// transform (RandomRotate :209-242, RandomScale :285-296, RandomFlip :300-315, RandomJitter :319-333, ElasticDistortion
// :709-766, ChromaticAutoContrast :358-375, ChromaticTranslation :379-388, ChromaticJitter :392-404, ...) is here a PROGRAM
// of steps that one kernel runs per point: the coordinate lives in double registers, the colour in fp32 registers, one
// lane per point, HBM-streaming.  It is a rounding-for-rounding restatement, not an algebraic fusion: every product and
// sum is rounded on its own (the whole file is compiled with contraction off and spells the roundings out as dataops.hip
// does -- the Makefile passes -ffp-contract=off for this unit, because the pragma below does not reach the header
// intrinsics' bodies), and the python side places a ROUND_F32 step wherever the reference's in-place statement rounds to its float32
// array.
#pragma clang fp contract(off)
#include <limits.h>

#include "gva_common.h"
#include "../../include/ptv2_data_hip.h"

extern "C" int ptv2_data_abi_version(void) { return 1; }  // == EXPECTED_DATA_ABI in ao_amd/_lib.py
extern "C" long long ptv2_data_struct_bytes(int which) {
    switch (which) {
        case 0: return (long long)sizeof(ptv2_aug_step);
        case 1: return (long long)sizeof(ptv2_aug_program);
        default: return -1;
    }
}

namespace {

constexpr int ATPB = 256;
int stream_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + ATPB - 1) / ATPB, 256 * 8)); }

// ---------------------------------------------------------------------------------------------------------- noise --
// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long a = (unsigned long long)0xD2511F53u * c0, b = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(b >> 32) ^ c1 ^ k0, n1 = (unsigned)b, n2 = (unsigned)(a >> 32) ^ c3 ^ k1, n3 = (unsigned)a;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The three normals of point `i` in RNG stream `stream_no`: counter (i lo, i hi, stream_no, 0), four words -> uniforms
// u = ((x >> 8) + 0.5) * 2^-24 -> Box-Muller pairs (u0, u1) and (u2, u3); the second pair's sine is not used.  fp32
// throughout, but no uniform is ever ROUNDED to fp32: u >= 1/2 needs 25 bits, and rounding it loses up to a third of 1 - u,
// i.e. of -ln u, where the normal is small (measured before this form: 5.5e-5 absolute on normals of 4e-4).  Instead the
// lower half is kept as u and the upper half as 1 - u = (2^24 - (x >> 8) - 0.5) * 2^-24, both exact in fp32;
// -ln u = -log1p(-(1 - u)), and sin / cos of 2 pi u = sincospi(2 u) = sincospi(-2 (1 - u)): no rounded 2 pi either.
struct AugUniform { float v; bool upper; };  // u = upper ? 1 - v : v
__device__ __forceinline__ AugUniform aug_uniform(unsigned word) {
    const unsigned k = word >> 8;
    const bool upper = k >= (1u << 23);
    return AugUniform{(upper ? (float)((1u << 24) - k) - 0.5f : (float)k + 0.5f) * 0x1p-24f, upper};
}
__device__ __forceinline__ float aug_radius(AugUniform u) { return sqrtf(2.f * (u.upper ? -log1pf(-u.v) : -logf(u.v))); }
__device__ __forceinline__ void aug_normals(unsigned k0, unsigned k1, long long i, int stream_no, float g[3]) {
    unsigned w[4];
    philox4x32_10((unsigned)(unsigned long long)i, (unsigned)((unsigned long long)i >> 32), (unsigned)stream_no, 0u, k0, k1, w);
    const float r0 = aug_radius(aug_uniform(w[0])), r1 = aug_radius(aug_uniform(w[2]));
    const AugUniform a0 = aug_uniform(w[1]), a1 = aug_uniform(w[3]);
    float s0, c0, s1, c1;
    sincospif(a0.upper ? -2.f * a0.v : 2.f * a0.v, &s0, &c0);
    sincospif(a1.upper ? -2.f * a1.v : 2.f * a1.v, &s1, &c1);
    g[0] = r0 * c0;
    g[1] = r0 * s0;
    g[2] = r1 * c1;
}

__global__ __launch_bounds__(ATPB) void aug_noise_kernel(long long n, unsigned k0, unsigned k1, int stream_no, float *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * ATPB + threadIdx.x; i < n; i += (long long)gridDim.x * ATPB) {
        float g[3];
        aug_normals(k0, k1, i, stream_no, g);
        out[3 * i] = g[0]; out[3 * i + 1] = g[1]; out[3 * i + 2] = g[2];
    }
}

// --------------------------------------------------------------------------------------------------------- bounds --
// order-preserving double <-> int64 encoding: integer atomicMin / atomicMax are exact and order independent
__device__ __forceinline__ long long d2ord(double d) {
    const long long i = __double_as_longlong(d);
    return i >= 0 ? i : i ^ 0x7fffffffffffffffLL;
}
__device__ __forceinline__ double ord2d(long long i) { return __longlong_as_double(i >= 0 ? i : i ^ 0x7fffffffffffffffLL); }

__global__ void aug_bounds_init_kernel(long long *enc) {
    if (threadIdx.x < 12) enc[threadIdx.x] = (threadIdx.x % 6) < 3 ? LLONG_MAX : LLONG_MIN;
}
__global__ void aug_bounds_decode_kernel(const long long *enc, double *bounds, int count) {
    if ((int)threadIdx.x < count) bounds[threadIdx.x] = ord2d(enc[threadIdx.x]);
}

template <class T>
__global__ __launch_bounds__(ATPB) void aug_bounds_kernel(long long n, const T *__restrict__ coord, const float *__restrict__ color,
                                                          long long *enc) {
    double lo[6], hi[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) { lo[d] = __builtin_inf(); hi[d] = -__builtin_inf(); }
    for (long long i = (long long)blockIdx.x * ATPB + threadIdx.x; i < n; i += (long long)gridDim.x * ATPB) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double v = (double)coord[3 * i + d];
            lo[d] = fmin(lo[d], v); hi[d] = fmax(hi[d], v);
        }
        if (color) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double v = (double)color[3 * i + d];
                lo[3 + d] = fmin(lo[3 + d], v); hi[3 + d] = fmax(hi[3 + d], v);
            }
        }
    }
    const int nd = color ? 6 : 3;
    for (int d = 0; d < nd; ++d) {
        double a = lo[d], b = hi[d];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { a = fmin(a, __shfl_xor(a, m, WAVE)); b = fmax(b, __shfl_xor(b, m, WAVE)); }
        if ((threadIdx.x & 63) == 0) {
            const int slot = d < 3 ? d : 3 + d;  // coord: 0..2 / 3..5, colour: 6..8 / 9..11
            atomicMin(enc + slot, d2ord(a));
            atomicMax(enc + slot + 3, d2ord(b));
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- blur --
// out[x][y][z][c] = (float)(((in[-1] * w + in[0] * w) + in[+1] * w) along `axis`, w = (double)(1.f / 3), zero outside:
// scipy.ndimage.convolve(noise, ones(3) / 3 as float32, mode="constant", cval=0) accumulates in double in this order
__global__ __launch_bounds__(ATPB) void aug_blur3_kernel(int dx, int dy, int dz, int axis, const float *__restrict__ in,
                                                         float *__restrict__ out) {
    const long long total = (long long)dx * dy * dz * 3;
    const int dim = axis == 0 ? dx : axis == 1 ? dy : dz;
    const long long stride = axis == 0 ? (long long)dy * dz * 3 : axis == 1 ? (long long)dz * 3 : 3;
    const double w = (double)(1.f / 3.f);
    for (long long e = (long long)blockIdx.x * ATPB + threadIdx.x; e < total; e += (long long)gridDim.x * ATPB) {
        const int pos = (int)((e / stride) % dim);
        double acc = 0.0;
        acc = __dadd_rn(acc, __dmul_rn(pos > 0 ? (double)in[e - stride] : 0.0, w));
        acc = __dadd_rn(acc, __dmul_rn((double)in[e], w));
        acc = __dadd_rn(acc, __dmul_rn(pos + 1 < dim ? (double)in[e + stride] : 0.0, w));
        out[e] = (float)acc;
    }
}

// --------------------------------------------------------------------------------------------------------- points --
__device__ __forceinline__ double aug_centre(double lo, double hi, bool fp32) {
    return fp32 ? (double)__fmul_rn(__fadd_rn((float)lo, (float)hi), 0.5f) : __dmul_rn(__dadd_rn(lo, hi), 0.5);
}
// np.clip: a NaN stays a NaN (fmin / fmax alone would return the bound)
__device__ __forceinline__ double aug_clip(double v, double lo, double hi) { return v != v ? v : fmin(fmax(v, lo), hi); }

__global__ __launch_bounds__(ATPB) void aug_points_kernel(long long n, const ptv2_aug_program P, const double *__restrict__ bounds,
                                                          const void *cin, const float *colin, const float *__restrict__ noise,
                                                          unsigned k0, unsigned k1, void *cout, float *colout) {
    double b[12];
#pragma unroll
    for (int d = 0; d < 12; ++d) b[d] = bounds ? bounds[d] : 0.0;
    for (long long i = (long long)blockIdx.x * ATPB + threadIdx.x; i < n; i += (long long)gridDim.x * ATPB) {
        double x[3];
        float c[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x[d] = P.coord_in_f64 ? ((const double *)cin)[3 * i + d] : (double)((const float *)cin)[3 * i + d];
            if (colin) c[d] = colin[3 * i + d];
        }
        for (int s = 0; s < P.count; ++s) {
            const ptv2_aug_step &S = P.step[s];
            const bool fp32 = (S.flags & PTV2_AUG_FLAG_FP32) != 0;
            float g[3] = {0.f, 0.f, 0.f};
            if (S.kind == PTV2_AUG_JITTER || S.kind == PTV2_AUG_COLOR_JITTER) {
                if (noise) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) g[d] = noise[((long long)S.slot * n + i) * 3 + d];
                } else {
                    aug_normals(k0, k1, i, S.stream, g);
                }
            }
            switch (S.kind) {
                case PTV2_AUG_CENTER_SHIFT: {
                    x[0] = __dsub_rn(x[0], aug_centre(b[0], b[3], fp32));
                    x[1] = __dsub_rn(x[1], aug_centre(b[1], b[4], fp32));
                    if (S.flags & PTV2_AUG_FLAG_APPLY_Z) x[2] = __dsub_rn(x[2], b[2]);
                } break;
                case PTV2_AUG_ROTATE: {
                    double ctr[3], t[3];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        ctr[d] = (S.flags & PTV2_AUG_FLAG_BOUNDS_CENTER) ? aug_centre(b[d], b[3 + d], fp32) : S.p[9 + d];
                        t[d] = __dsub_rn(x[d], ctr[d]);
                        if (fp32) t[d] = (double)(float)t[d];
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        x[j] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(t[0], S.p[3 * j]), __dmul_rn(t[1], S.p[3 * j + 1])),
                                                   __dmul_rn(t[2], S.p[3 * j + 2])), ctr[j]);
                } break;
                case PTV2_AUG_SCALE:
#pragma unroll
                    for (int d = 0; d < 3; ++d) x[d] = __dmul_rn(x[d], S.p[d]);
                    break;
                case PTV2_AUG_SHIFT:
#pragma unroll
                    for (int d = 0; d < 3; ++d) x[d] = __dadd_rn(x[d], S.p[d]);
                    break;
                case PTV2_AUG_CLIP:
#pragma unroll
                    for (int d = 0; d < 3; ++d) x[d] = aug_clip(x[d], S.p[d], S.p[3 + d]);
                    break;
                case PTV2_AUG_JITTER:
#pragma unroll
                    for (int d = 0; d < 3; ++d) x[d] = __dadd_rn(x[d], aug_clip(__dmul_rn(S.p[0], (double)g[d]), -S.p[1], S.p[1]));
                    break;
                case PTV2_AUG_ELASTIC: {
                    int base[3];
                    double f[3];
                    bool inside = true;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const double t = __ddiv_rn(__dsub_rn(x[d], S.p[d]), S.p[3 + d]);
                        inside = inside && t >= 0.0 && t <= (double)(S.dims[d] - 1);  // (false for a NaN too)
                        const int cell = inside ? min(max((int)floor(t), 0), S.dims[d] - 2) : 0;
                        base[d] = cell;
                        f[d] = __dsub_rn(t, (double)cell);
                    }
                    if (inside) {  // outside the grid the reference's interpolator fills 0
                        double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
                        for (int corner = 0; corner < 8; ++corner) {
                            const int ox = corner >> 2, oy = (corner >> 1) & 1, oz = corner & 1;
                            double wgt = ox ? f[0] : __dsub_rn(1.0, f[0]);
                            wgt = __dmul_rn(wgt, oy ? f[1] : __dsub_rn(1.0, f[1]));
                            wgt = __dmul_rn(wgt, oz ? f[2] : __dsub_rn(1.0, f[2]));
                            const float *v = S.field + (((long long)(base[0] + ox) * S.dims[1] + (base[1] + oy)) * S.dims[2] + (base[2] + oz)) * 3;
#pragma unroll
                            for (int d = 0; d < 3; ++d) acc[d] = __dadd_rn(acc[d], __dmul_rn((double)v[d], wgt));
                        }
#pragma unroll
                        for (int d = 0; d < 3; ++d) x[d] = __dadd_rn(x[d], __dmul_rn(acc[d], S.p[6]));
                    }
                } break;
                case PTV2_AUG_ROUND_F32:
#pragma unroll
                    for (int d = 0; d < 3; ++d) x[d] = (double)(float)x[d];
                    break;
                case PTV2_AUG_COLOR_CONTRAST:
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float lo = (float)b[6 + d], hi = (float)b[9 + d];
                        const float stretched = __fmul_rn(__fsub_rn(c[d], lo), __fdiv_rn(255.f, __fsub_rn(hi, lo)));
                        c[d] = __fadd_rn(__fmul_rn((float)S.p[0], c[d]), __fmul_rn((float)S.p[1], stretched));
                    }
                    break;
                case PTV2_AUG_COLOR_TRANSLATE:
#pragma unroll
                    for (int d = 0; d < 3; ++d) c[d] = (float)aug_clip(__dadd_rn(S.p[d], (double)c[d]), 0.0, 255.0);
                    break;
                case PTV2_AUG_COLOR_JITTER:
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        c[d] = (float)aug_clip(__dadd_rn(__dmul_rn((double)g[d], S.p[0]), (double)c[d]), 0.0, 255.0);
                    break;
                case PTV2_AUG_COLOR_MUL:
#pragma unroll
                    for (int d = 0; d < 3; ++d) c[d] = __fmul_rn(c[d], (float)S.p[0]);
                    break;
                default: break;
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (P.coord_out_f64) ((double *)cout)[3 * i + d] = x[d];
            else ((float *)cout)[3 * i + d] = (float)x[d];
            if (colout) colout[3 * i + d] = c[d];
        }
    }
}

}  // namespace

extern "C" int aug_points_hip_launcher(long long n, const ptv2_aug_program *program, const double *bounds, const void *coord_in,
                                       const float *color_in, const float *noise, long long seed, void *coord_out,
                                       float *color_out, void *stream) {
    if (n < 0 || !program || program->count < 0 || program->count > PTV2_AUG_MAX_STEPS) return PTV2_ERR_ARG;
    if ((color_in == nullptr) != (color_out == nullptr)) return PTV2_ERR_ARG;
    for (int s = 0; s < program->count; ++s) {
        const ptv2_aug_step &S = program->step[s];
        if (S.kind < 0 || S.kind >= PTV2_AUG_KINDS) return PTV2_ERR_ARG;
        const bool reads_bounds = S.kind == PTV2_AUG_CENTER_SHIFT || S.kind == PTV2_AUG_COLOR_CONTRAST ||
                                  (S.kind == PTV2_AUG_ROTATE && (S.flags & PTV2_AUG_FLAG_BOUNDS_CENTER));
        if (reads_bounds && !bounds) return PTV2_ERR_ARG;
        if (S.kind >= PTV2_AUG_COLOR_CONTRAST && !color_in) return PTV2_ERR_ARG;
        if (S.kind == PTV2_AUG_ELASTIC && (!S.field || S.dims[0] < 2 || S.dims[1] < 2 || S.dims[2] < 2 || !(S.p[3] > 0.0) ||
                                           !(S.p[4] > 0.0) || !(S.p[5] > 0.0)))
            return PTV2_ERR_ARG;
        if (noise && S.slot < 0) return PTV2_ERR_ARG;
    }
    if (n == 0) return PTV2_OK;
    if (!coord_in || !coord_out) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long key = (unsigned long long)seed;
    {
        PtvScopedTimer timer(KID_AUG_POINTS, st, (double)n * (24.0 + (color_in ? 24.0 : 0.0)));
        hipLaunchKernelGGL(aug_points_kernel, dim3(stream_grid(n)), dim3(ATPB), 0, st, n, *program, bounds, coord_in, color_in, noise,
                           (unsigned)key, (unsigned)(key >> 32), coord_out, color_out);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int aug_bounds_hip_launcher(long long n, const void *coord, int coord_f64, const float *color, double *bounds, void *stream) {
    if (n < 1 || !coord || !bounds) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    long long *enc = (long long *)(bounds + 12);
    hipLaunchKernelGGL(aug_bounds_init_kernel, dim3(1), dim3(64), 0, st, enc);
    if (coord_f64)
        hipLaunchKernelGGL(aug_bounds_kernel<double>, dim3(stream_grid(n)), dim3(ATPB), 0, st, n, (const double *)coord, color, enc);
    else
        hipLaunchKernelGGL(aug_bounds_kernel<float>, dim3(stream_grid(n)), dim3(ATPB), 0, st, n, (const float *)coord, color, enc);
    hipLaunchKernelGGL(aug_bounds_decode_kernel, dim3(1), dim3(64), 0, st, (const long long *)enc, bounds, color ? 12 : 6);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int aug_noise_hip_launcher(long long n, long long seed, int stream_no, float *out, void *stream) {
    if (n < 0) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!out) return PTV2_ERR_ARG;
    const unsigned long long key = (unsigned long long)seed;
    hipLaunchKernelGGL(aug_noise_kernel, dim3(stream_grid(n)), dim3(ATPB), 0, (hipStream_t)stream, n, (unsigned)key,
                       (unsigned)(key >> 32), stream_no, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int aug_blur3_hip_launcher(int dx, int dy, int dz, int axis, const float *in, float *out, void *stream) {
    if (dx < 1 || dy < 1 || dz < 1 || axis < 0 || axis > 2 || !in || !out || in == out) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(aug_blur3_kernel, dim3(stream_grid((long long)dx * dy * dz * 3)), dim3(ATPB), 0, (hipStream_t)stream, dx, dy,
                       dz, axis, in, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
