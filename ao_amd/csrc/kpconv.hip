// ao_amd/csrc/kpconv.hip -- the stem of Stratified Transformer: KPConv with linear influence and sum aggregation (C ABI
// include/ptv2_st_hip.h).
//
// Forward: one thread per (point, kernel point, channel) walks the point's neighbour row and sums influence * feature, so neither
// an (N, max_n, 15) influence array nor an (N, max_n, cin) gathered-feature array exists; the product with the weight is a GEMM
// of the caller.  Backward: one thread per (neighbour, channel) walks the transposed neighbour lists and recomputes each
// influence: a gather in a fixed order, no atomics.  The influence is recomputed per channel: the stem has 3 to 12 input channels
// and runs twice per forward.
#include "common.h"
#include "../../include/ptv2_st_hip.h"

#define KP_TPB 256

__device__ __forceinline__ float kp_influence(float rx, float ry, float rz, const float *__restrict__ kp, int k, float extent) {
    const float dx = rx - kp[k * 3], dy = ry - kp[k * 3 + 1], dz = rz - kp[k * 3 + 2];
    const float dist = sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
    return fmaxf(0.f, 1.f - dist / extent);
}

__global__ __launch_bounds__(KP_TPB) void kpconv_fwd_kernel(int n, int max_n, int cin, const float *__restrict__ xyz,
                                                            const long long *__restrict__ nbr, const float *__restrict__ feats,
                                                            const float *__restrict__ kpoints, float extent,
                                                            float *__restrict__ weighted) {
    const long long e = (long long)blockIdx.x * KP_TPB + threadIdx.x;
    if (e >= (long long)n * ST_KP_POINTS * cin) return;
    const int c = (int)(e % cin), k = (int)((e / cin) % ST_KP_POINTS), i = (int)(e / ((long long)cin * ST_KP_POINTS));
    const float x = xyz[(long long)i * 3], y = xyz[(long long)i * 3 + 1], z = xyz[(long long)i * 3 + 2];
    float acc = 0.f;
    for (int m = 0; m < max_n; ++m) {
        const long long j = nbr[(long long)i * max_n + m];
        if (j < 0 || j >= n) continue;
        const float w = kp_influence(xyz[j * 3] - x, xyz[j * 3 + 1] - y, xyz[j * 3 + 2] - z, kpoints, k, extent);
        acc = __builtin_fmaf(w, feats[j * cin + c], acc);
    }
    weighted[e] = acc;
}

__global__ __launch_bounds__(KP_TPB) void kpconv_bwd_kernel(int n, int cin, long long slots, const float *__restrict__ xyz,
                                                            const int *__restrict__ t_offsets, const int *__restrict__ t_src,
                                                            const float *__restrict__ kpoints, float extent,
                                                            const float *__restrict__ g_weighted, float *__restrict__ g_feats) {
    const long long e = (long long)blockIdx.x * KP_TPB + threadIdx.x;
    if (e >= (long long)n * cin) return;
    const int c = (int)(e % cin), j = (int)(e / cin);
    const float x = xyz[(long long)j * 3], y = xyz[(long long)j * 3 + 1], z = xyz[(long long)j * 3 + 2];
    long long beg = t_offsets[j], end = t_offsets[j + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > slots ? slots : end;
    float acc = 0.f;
    for (long long s = beg; s < end; ++s) {
        const int i = t_src[s];
        if ((unsigned)i >= (unsigned)n) continue;
        const float rx = x - xyz[(long long)i * 3], ry = y - xyz[(long long)i * 3 + 1], rz = z - xyz[(long long)i * 3 + 2];
        const float *g = g_weighted + (long long)i * ST_KP_POINTS * cin + c;
#pragma unroll
        for (int k = 0; k < ST_KP_POINTS; ++k) acc = __builtin_fmaf(kp_influence(rx, ry, rz, kpoints, k, extent), g[(long long)k * cin], acc);
    }
    g_feats[e] = acc;
}

extern "C" int st_kpconv_fwd_hip_launcher(int n, int max_n, int cin, const float *xyz, const long long *nbr, const float *feats,
                                          const float *kpoints, float extent, float *weighted, void *stream) {
    if (n < 0 || max_n < 1 || cin < 1 || !xyz || !nbr || !feats || !kpoints || !(extent > 0.f) || !weighted) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    const long long total = (long long)n * ST_KP_POINTS * cin;
    if (total > 0x7fffffffLL * KP_TPB) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(kpconv_fwd_kernel, dim3(divup(total, KP_TPB)), dim3(KP_TPB), 0, (hipStream_t)stream, n, max_n, cin, xyz, nbr,
                       feats, kpoints, extent, weighted);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int st_kpconv_bwd_hip_launcher(int n, int cin, long long slots, const float *xyz, const int *t_offsets, const int *t_src,
                                          const float *kpoints, float extent, const float *g_weighted, float *g_feats, void *stream) {
    if (n < 0 || cin < 1 || slots < 0 || !xyz || !t_offsets || (slots > 0 && !t_src) || !kpoints || !(extent > 0.f) || !g_weighted ||
        !g_feats)
        return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    hipLaunchKernelGGL(kpconv_bwd_kernel, dim3(divup((long long)n * cin, KP_TPB)), dim3(KP_TPB), 0, (hipStream_t)stream, n, cin, slots,
                       xyz, t_offsets, t_src, kpoints, extent, g_weighted, g_feats);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
