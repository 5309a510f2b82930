// ao_amd/csrc/spv_ops.hip -- SPVCNN's point-voxel operators over the map of spv_map.hip and the k = 3 tables of
// spconv_tables.hip (include/ptv2_spv_hip.h).  gfx950 only.  Gathers bound by memory: no matrix
// instructions, lanes run along the channels in float4.
//
// devoxelize forward   A workgroup takes 32 points per step.  Stage 1: thread (point, corner) = (t >> 3, t & 7) reads the
//     point's row, ONE entry of its table row (the columns 13, 14, 16, 17, 22, 23, 25, 26 are the eight corners) and the
//     coordinate, and leaves the corner's row and raw weight in LDS (2 x 1 KiB): the (n, 8) index and weight tensors of the
//     reference live there, for 32 points at a time.  Stage 2: C / 4 lanes per point, 256 / (C / 4) points at once; W is the sum
//     of the eight LDS weights in corner order, every lane divides by it, and eight float4 rows are gathered.
// segmented sums       The devoxelize backward and the voxelize forward are one kernel: row v of the output is a sum over
//     up to eight runs of the level's CSR (the voxels at the MIRRORED corners of v, each with the weight its points give v; or
//     the voxel's own run with weight 1).  A workgroup is S = 256 / lanes slices; `sv` of them share one voxel, so S / sv
//     voxels are in flight per step.  Slice `sub` takes the items k = sub (mod sv) of the concatenated runs, whatever their
//     number -- a crowded voxel is spread over all its slices, a stride-16 voxel over the whole workgroup -- and the partials
//     are added in LDS in slice order.  sv depends on (C, level) alone, so the order of every sum is fixed.
// voxelize backward    one gather per element.
#include <algorithm>

#include "common.h"
#include "../../include/ptv2_spv_hip.h"

#define SPV_TPB 256
#define SPV_TILE 32        // points per step of the forward: 32 x 8 corners = one thread each
#define SPV_MAX_GROUP 32   // voxels in flight per step of the segmented sums: 32 x 8 runs = one thread each
#define SPV_MAX_BLOCKS 16384

// the raw trilinear weight of corner j = 4 jx + 2 jy + jz for a point at (px, py, pz): exact in fp32 (multiples of 2^-12)
__device__ __forceinline__ float spv_corner_weight(int px, int py, int pz, int level, int j) {
    const int m = (1 << level) - 1;
    const float inv = 1.f / (float)(1 << level);
    const float fx = (float)(px & m) * inv, fy = (float)(py & m) * inv, fz = (float)(pz & m) * inv;
    return ((j & 4) ? fx : 1.f - fx) * ((j & 2) ? fy : 1.f - fy) * ((j & 1) ? fz : 1.f - fz);
}

__device__ __forceinline__ void spv_fma(float4 &a, float w, const float4 &x) {
    a.x = __builtin_fmaf(w, x.x, a.x); a.y = __builtin_fmaf(w, x.y, a.y); a.z = __builtin_fmaf(w, x.z, a.z); a.w = __builtin_fmaf(w, x.w, a.w);
}
__device__ __forceinline__ void spv_fma(float &a, float w, const float &x) { a = __builtin_fmaf(w, x, a); }
__device__ __forceinline__ void spv_add(float4 &a, const float4 &x) { a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w; }
__device__ __forceinline__ void spv_add(float &a, const float &x) { a += x; }
__device__ __forceinline__ void spv_div(float4 &a, float d) { a.x /= d; a.y /= d; a.z /= d; a.w /= d; }
__device__ __forceinline__ void spv_div(float &a, float d) { a /= d; }
template <class V> __device__ __forceinline__ V spv_zero();
template <> __device__ __forceinline__ float4 spv_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <> __device__ __forceinline__ float spv_zero<float>() { return 0.f; }

__global__ __launch_bounds__(SPV_TPB) void spv_devox_fwd_kernel(int n, int nv, int c, int level, const int *__restrict__ coord,
                                                                const int *__restrict__ row, const int *__restrict__ nbr3,
                                                                const float *__restrict__ feat, const float *__restrict__ add,
                                                                float *__restrict__ out, float *__restrict__ wsum) {
    __shared__ int s_idx[SPV_TILE * 8];
    __shared__ float s_w[SPV_TILE * 8];
    const int c4 = c / 4, rpb = SPV_TPB / c4, r = threadIdx.x / c4, q = threadIdx.x % c4;
    const int tp = threadIdx.x >> 3, tj = threadIdx.x & 7;
    for (long long base = (long long)blockIdx.x * SPV_TILE; base < n; base += (long long)gridDim.x * SPV_TILE) {
        int idx = -1;
        float w = 0.f;
        const long long i = base + tp;
        if (i < n) {
            const int vr = row[i];
            if ((unsigned)vr < (unsigned)nv) {
                const int j = nbr3[(size_t)vr * 27 + 13 + 9 * (tj >> 2) + 3 * ((tj >> 1) & 1) + (tj & 1)];
                if ((unsigned)j < (unsigned)nv) {
                    idx = j;
                    w = spv_corner_weight(coord[3 * i], coord[3 * i + 1], coord[3 * i + 2], level, tj);
                }
            }
        }
        s_idx[threadIdx.x] = idx;
        s_w[threadIdx.x] = w;
        __syncthreads();
        if (r < rpb)
            for (int t = r; t < SPV_TILE && base + t < n; t += rpb) {
                float total = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) total += s_w[t * 8 + j];
                total += 1e-8f;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int v = s_idx[t * 8 + j];
                    const bool ok = v >= 0;
                    const float4 xv = ptv2_ld_or_zero((const float4 *)(feat + (size_t)(ok ? v : 0) * c) + q, ok);
                    spv_fma(acc, s_w[t * 8 + j] / total, xv);
                }
                const size_t at = (size_t)(base + t) * c;
                if (add) spv_add(acc, *((const float4 *)(add + at) + q));
                *((float4 *)(out + at) + q) = acc;
                if (q == 0) wsum[base + t] = total;
            }
        __syncthreads();
    }
}

// out[v] = sum over the runs j of voxel v, over the points i of run j, of weight_j(i) x[i]   (DEVOX: the gradient to F)
//        = (sum over the points i of voxel v of x[i]) / count_v                             (!DEVOX: the mean)
template <class V, bool DEVOX>
__global__ __launch_bounds__(SPV_TPB) void spv_segsum_kernel(int n, int nv, int c, int lanes, int level, int sv, int group,
                                                             const int *__restrict__ coord, const int *__restrict__ nbr3,
                                                             const int *__restrict__ start, const int *__restrict__ order,
                                                             const float *__restrict__ wsum, const float *__restrict__ x,
                                                             float *__restrict__ out) {
    __shared__ V part[SPV_TPB];
    __shared__ int s_begin[SPV_MAX_GROUP * 8], s_len[SPV_MAX_GROUP * 8];
    const int s = threadIdx.x / lanes, q = threadIdx.x % lanes, slot = s / sv, sub = s % sv;
    for (long long vbase = (long long)blockIdx.x * group; vbase < nv; vbase += (long long)gridDim.x * group) {
        if ((int)threadIdx.x < group * 8) {
            const int j = threadIdx.x & 7;
            const long long v = vbase + (threadIdx.x >> 3);
            int u = -1, b = 0, len = 0;
            if (v < nv) u = DEVOX ? nbr3[(size_t)v * 27 + 13 - (9 * (j >> 2) + 3 * ((j >> 1) & 1) + (j & 1))] : (j == 0 ? (int)v : -1);
            if ((unsigned)u < (unsigned)nv) {
                b = min(max(start[u], 0), n);
                len = min(max(start[u + 1], b), n) - b;
            }
            s_begin[threadIdx.x] = b;
            s_len[threadIdx.x] = len;
        }
        __syncthreads();
        const long long v = vbase + slot;
        const bool active = slot < group && v < nv;
        int total = 0;
        if (active) {
            V acc = spv_zero<V>();
#pragma unroll
            for (int j = 0; j < (DEVOX ? 8 : 1); ++j) {
                const int b = s_begin[slot * 8 + j], len = s_len[slot * 8 + j];
                // the items of this run are total .. total + len of the concatenation; this slice takes those = sub (mod sv)
                for (int k = (sub - total % sv + sv) % sv; k < len; k += sv) {
                    const int i = order[b + k];
                    if ((unsigned)i >= (unsigned)n) continue;
                    float w = 1.f;
                    if (DEVOX) w = spv_corner_weight(coord[3 * (size_t)i], coord[3 * (size_t)i + 1], coord[3 * (size_t)i + 2], level, j) / wsum[i];
                    spv_fma(acc, w, *((const V *)(x + (size_t)i * c) + q));
                }
                total += len;
            }
            part[threadIdx.x] = acc;
        }
        __syncthreads();
        if (active && sub == 0) {
            V sum = part[threadIdx.x];
            const int m = min(sv, total);
            for (int t = 1; t < m; ++t) spv_add(sum, part[threadIdx.x + t * lanes]);
            if (!DEVOX && total > 0) spv_div(sum, (float)total);
            *((V *)(out + (size_t)v * c) + q) = sum;
        }
        __syncthreads();
    }
}

template <class V>
__global__ __launch_bounds__(SPV_TPB) void spv_vox_bwd_kernel(int n, int nv, int lanes, const int *__restrict__ row,
                                                              const int *__restrict__ start, const float *__restrict__ gv,
                                                              float *__restrict__ gx) {
    const long long t = (long long)blockIdx.x * SPV_TPB + threadIdx.x;
    if (t >= (long long)n * lanes) return;
    const long long i = t / lanes;
    const int q = (int)(t - i * lanes), r = row[i];
    V g = spv_zero<V>();
    if ((unsigned)r < (unsigned)nv) {
        g = *((const V *)gv + (size_t)r * lanes + q);
        spv_div(g, (float)max(start[r + 1] - start[r], 1));
    }
    *((V *)gx + t) = g;
}

static bool spv_wide_ok(int c) { return c >= 32 && c % 32 == 0 && c <= SPV_MAX_CHANNELS; }
static bool spv_shape_ok(int n, int nv, int level) { return n >= 1 && nv >= 1 && nv <= n && level >= 0 && level < SPV_LEVELS; }

// slices per voxel: a stride-4 or stride-16 voxel holds tens to hundreds of points and gets the workgroup (up to 64 slices);
// below that a voxel holds a few
static int spv_slices_per_voxel(int slices, int level, bool devox) { return std::min(slices, level >= 2 ? 64 : (devox ? 8 : 4)); }

template <class V, bool DEVOX>
static int spv_segsum_launch(int n, int nv, int c, int lanes, int level, const int *coord, const int *nbr3, const int *start,
                             const int *order, const float *wsum, const float *x, float *out, hipStream_t st) {
    const int slices = SPV_TPB / lanes, sv = spv_slices_per_voxel(slices, level, DEVOX), group = std::min(slices / sv, SPV_MAX_GROUP);
    const int blocks = (int)std::min((long long)divup(nv, group), (long long)SPV_MAX_BLOCKS);
    hipLaunchKernelGGL((spv_segsum_kernel<V, DEVOX>), dim3(blocks), dim3(SPV_TPB), 0, st, n, nv, c, lanes, level, sv, group, coord,
                       nbr3, start, order, wsum, x, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int spv_devoxelize_fwd_hip_launcher(int n, int n_vox, int c, int level, const int *coord, const int *row, const int *nbr3,
                                               const float *feat, const float *add, float *out, float *wsum, void *stream) {
    if (!spv_shape_ok(n, n_vox, level) || !spv_wide_ok(c) || !coord || !row || !nbr3 || !feat || !out || !wsum) return PTV2_ERR_ARG;
    const int blocks = (int)std::min((long long)divup(n, SPV_TILE), (long long)SPV_MAX_BLOCKS);
    hipLaunchKernelGGL(spv_devox_fwd_kernel, dim3(blocks), dim3(SPV_TPB), 0, (hipStream_t)stream, n, n_vox, c, level, coord, row, nbr3,
                       feat, add, out, wsum);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int spv_devoxelize_bwd_hip_launcher(int n, int n_vox, int c, int level, const int *coord, const int *nbr3, const int *start,
                                               const int *order, const float *wsum, const float *g, float *g_feat, void *stream) {
    if (!spv_shape_ok(n, n_vox, level) || !spv_wide_ok(c) || !coord || !nbr3 || !start || !order || !wsum || !g || !g_feat)
        return PTV2_ERR_ARG;
    return spv_segsum_launch<float4, true>(n, n_vox, c, c / 4, level, coord, nbr3, start, order, wsum, g, g_feat, (hipStream_t)stream);
}

extern "C" int spv_voxelize_fwd_hip_launcher(int n, int n_vox, int c, int level, const int *start, const int *order, const float *x,
                                             float *v, void *stream) {
    const bool small = c >= 1 && c <= SPV_SMALL_CHANNELS;
    if (!spv_shape_ok(n, n_vox, level) || !(small || spv_wide_ok(c)) || !start || !order || !x || !v) return PTV2_ERR_ARG;
    if (small)
        return spv_segsum_launch<float, false>(n, n_vox, c, c, level, nullptr, nullptr, start, order, nullptr, x, v, (hipStream_t)stream);
    return spv_segsum_launch<float4, false>(n, n_vox, c, c / 4, level, nullptr, nullptr, start, order, nullptr, x, v, (hipStream_t)stream);
}

extern "C" int spv_voxelize_bwd_hip_launcher(int n, int n_vox, int c, const int *row, const int *start, const float *g_v, float *g_x,
                                             void *stream) {
    const bool small = c >= 1 && c <= SPV_SMALL_CHANNELS;
    if (!spv_shape_ok(n, n_vox, 0) || !(small || spv_wide_ok(c)) || !row || !start || !g_v || !g_x) return PTV2_ERR_ARG;
    const int lanes = small ? c : c / 4;
    const dim3 grid(divup((long long)n * lanes, SPV_TPB));
    if (small)
        hipLaunchKernelGGL(spv_vox_bwd_kernel<float>, grid, dim3(SPV_TPB), 0, (hipStream_t)stream, n, n_vox, lanes, row, start, g_v, g_x);
    else
        hipLaunchKernelGGL(spv_vox_bwd_kernel<float4>, grid, dim3(SPV_TPB), 0, (hipStream_t)stream, n, n_vox, lanes, row, start, g_v, g_x);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
