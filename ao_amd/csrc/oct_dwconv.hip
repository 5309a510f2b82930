// ao_amd/csrc/oct_dwconv.hip -- the 27-neighbour table of a Morton-ordered node list and the depthwise octree convolution of
// OctFormer's conditional position encoding (include/ptv2_oct_hip.h).  gfx950 only.
//
// The convolution is a gather bound by memory: lanes run along channels in float4, 256 / (C / 4) rows share a workgroup, the
// 27 x C weights sit in LDS, and Morton order keeps the 27 rows of a node close.  No matrix instructions.  The input gradient is
// the same kernel with the weights mirrored (nbr[i, k] == j exactly when nbr[j, 26 - k] == i); the weight gradient is one
// (27, C) partial per workgroup over a strip of rows and a finalize that adds the partials ascending.
#include "common.h"
#include "../../include/ptv2_oct_hip.h"

#define OCT_TPB 256
#define OCT_NBR 27
#define OCT_DW_MAX_BLOCKS 2048   // forward / input gradient: workgroups that stage the weights
#define OCT_GW_MAX_BLOCKS 256    // weight gradient: partials

// The Morton key of ocnn's xyz2key, restated from its documentation (python: ao_amd/octformer/octree.py xyz2key): bit i of x goes
// to key bit 3 i + 2, y to 3 i + 1, z to 3 i.
__device__ __forceinline__ long long oct_key(int x, int y, int z, int depth) {
    long long key = 0;
    for (int i = 0; i < depth; ++i)
        key |= (long long)(x >> i & 1) << (3 * i + 2) | (long long)(y >> i & 1) << (3 * i + 1) | (long long)(z >> i & 1) << (3 * i);
    return key;
}

__global__ __launch_bounds__(OCT_TPB) void oct_neighbors_kernel(oct_args a) {
    const long long t = (long long)blockIdx.x * OCT_TPB + threadIdx.x;
    if (t >= (long long)OCT_NBR * a.n) return;
    const int i = (int)(t / OCT_NBR), k = (int)(t % OCT_NBR);
    const int x = a.xyz[3 * (size_t)i] + k / 9 - 1, y = a.xyz[3 * (size_t)i + 1] + k / 3 % 3 - 1, z = a.xyz[3 * (size_t)i + 2] + k % 3 - 1;
    const int lim = 1 << a.depth, b = a.batch[i];
    int found = -1;
    // outside the cube there is no node: decided on the coordinates, the key arithmetic would wrap
    if (x >= 0 && x < lim && y >= 0 && y < lim && z >= 0 && z < lim && b >= 0 && b < a.clouds) {
        const long long key = oct_key(x, y, z, a.depth);
        int lo = max(a.cloud_offsets[b], 0);
        const int end = min(a.cloud_offsets[b + 1], a.n);
        int hi = end;
        while (lo < hi) {   // the first row of the cloud whose key is >= key
            const int mid = lo + ((hi - lo) >> 1);
            if (a.keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < end && a.keys[lo] == key) found = lo;
    }
    a.nbr_out[t] = found;
}

// y[i, c] = sum_k w[MIRROR ? 26 - k : k, c] x[nbr[i, k], c]
template <bool MIRROR>
__global__ __launch_bounds__(OCT_TPB) void oct_dwconv_kernel(int n, int c, const int *__restrict__ nbr, const float *__restrict__ x,
                                                             const float *__restrict__ w, float *__restrict__ y) {
    extern __shared__ float4 oct_w4[];
    float *ws = (float *)oct_w4;
    for (int e = threadIdx.x; e < OCT_NBR * c; e += OCT_TPB) {
        const int k = e / c;
        ws[e] = w[(MIRROR ? OCT_NBR - 1 - k : k) * c + e % c];
    }
    __syncthreads();
    const int c4 = c / 4, rpb = OCT_TPB / c4, r = threadIdx.x / c4, q = threadIdx.x % c4;
    if (r >= rpb) return;
    for (long long row = (long long)blockIdx.x * rpb + r; row < n; row += (long long)gridDim.x * rpb) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < OCT_NBR; ++k) {
            const int j = nbr[row * OCT_NBR + k];
            const bool ok = (unsigned)j < (unsigned)n;
            const float4 xv = ptv2_ld_or_zero((const float4 *)(x + (size_t)(ok ? j : 0) * c) + q, ok);
            const float4 wv = oct_w4[k * c4 + q];
            acc.x = __builtin_fmaf(wv.x, xv.x, acc.x); acc.y = __builtin_fmaf(wv.y, xv.y, acc.y);
            acc.z = __builtin_fmaf(wv.z, xv.z, acc.z); acc.w = __builtin_fmaf(wv.w, xv.w, acc.w);
        }
        *((float4 *)(y + (size_t)row * c) + q) = acc;
    }
}

// partial[block][k][c] = sum over the block's rows (ascending per thread, then the threads of a channel ascending) of
// x[nbr[i, k], c] g_y[i, c]
__global__ __launch_bounds__(OCT_TPB) void oct_dwconv_gw_kernel(int n, int c, const int *__restrict__ nbr, const float *__restrict__ x,
                                                                const float *__restrict__ gy, float *__restrict__ partial) {
    __shared__ float4 red[OCT_TPB];
    const int c4 = c / 4, rpb = OCT_TPB / c4, r = threadIdx.x / c4, q = threadIdx.x % c4;
    const bool active = r < rpb;
    float4 acc[OCT_NBR];
#pragma unroll
    for (int k = 0; k < OCT_NBR; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active)
        for (long long row = (long long)blockIdx.x * rpb + r; row < n; row += (long long)gridDim.x * rpb) {
            const float4 g = *((const float4 *)(gy + (size_t)row * c) + q);
#pragma unroll
            for (int k = 0; k < OCT_NBR; ++k) {
                const int j = nbr[row * OCT_NBR + k];
                const bool ok = (unsigned)j < (unsigned)n;
                const float4 xv = ptv2_ld_or_zero((const float4 *)(x + (size_t)(ok ? j : 0) * c) + q, ok);
                acc[k].x = __builtin_fmaf(xv.x, g.x, acc[k].x); acc[k].y = __builtin_fmaf(xv.y, g.y, acc[k].y);
                acc[k].z = __builtin_fmaf(xv.z, g.z, acc[k].z); acc[k].w = __builtin_fmaf(xv.w, g.w, acc[k].w);
            }
        }
#pragma unroll
    for (int k = 0; k < OCT_NBR; ++k) {
        red[threadIdx.x] = acc[k];   // (an active thread is r * c4 + q)
        __syncthreads();
        if (active && r == 0) {
            float4 s = red[q];
            for (int rr = 1; rr < rpb; ++rr) {
                const float4 o = red[rr * c4 + q];
                s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
            }
            *((float4 *)(partial + ((size_t)blockIdx.x * OCT_NBR + k) * c) + q) = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(OCT_TPB) void oct_dwconv_gw_finalize_kernel(int blocks, int elems, const float *__restrict__ partial,
                                                                         float *__restrict__ g_w) {
    const int e = blockIdx.x * OCT_TPB + threadIdx.x;
    if (e >= elems) return;
    float s = 0.f;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * elems + e];
    g_w[e] = s;
}

static bool oct_dwconv_shape_ok(int n, int c) { return n >= 1 && c >= 4 && c % 4 == 0 && c <= OCT_MAX_CHANNELS; }
static int oct_dwconv_blocks(int n, int c, int cap) { return (int)min((long long)divup(n, OCT_TPB / (c / 4)), (long long)cap); }

extern "C" long long ptv2_oct_dwconv_workspace_bytes(int n, int c) {
    if (!oct_dwconv_shape_ok(n, c)) return -1;
    return (long long)ptv2_align256(sizeof(float) * (size_t)oct_dwconv_blocks(n, c, OCT_GW_MAX_BLOCKS) * OCT_NBR * c);
}

extern "C" int oct_neighbors_hip_launcher(const oct_args *args, void *stream) {
    if (!args) return PTV2_ERR_ARG;
    const oct_args &a = *args;
    if (a.n < 1 || a.n > (1 << 26) || a.clouds < 1 || a.depth < 1 || a.depth > OCT_MAX_DEPTH || !a.xyz || !a.batch || !a.keys ||
        !a.cloud_offsets || !a.nbr_out)
        return PTV2_ERR_ARG;
    hipLaunchKernelGGL(oct_neighbors_kernel, dim3(divup((long long)OCT_NBR * a.n, OCT_TPB)), dim3(OCT_TPB), 0, (hipStream_t)stream, a);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

template <bool MIRROR>
static int oct_dwconv_launch(int n, int c, const int *nbr, const float *x, const float *w, float *y, hipStream_t st) {
    const size_t lds = sizeof(float) * OCT_NBR * (size_t)c;
    RUN(ptv2_kernel_lds((const void *)oct_dwconv_kernel<MIRROR>, lds));
    hipLaunchKernelGGL(oct_dwconv_kernel<MIRROR>, dim3(oct_dwconv_blocks(n, c, OCT_DW_MAX_BLOCKS)), dim3(OCT_TPB), lds, st, n, c, nbr, x, w, y);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int oct_dwconv_fwd_hip_launcher(const oct_args *args, void *stream) {
    if (!args || !oct_dwconv_shape_ok(args->n, args->c) || !args->nbr || !args->x || !args->w || !args->y) return PTV2_ERR_ARG;
    return oct_dwconv_launch<false>(args->n, args->c, args->nbr, args->x, args->w, args->y, (hipStream_t)stream);
}

extern "C" int oct_dwconv_bwd_hip_launcher(const oct_args *args, void *stream) {
    if (!args || !oct_dwconv_shape_ok(args->n, args->c) || !args->nbr || !args->g_y) return PTV2_ERR_ARG;
    const oct_args &a = *args;
    if ((a.g_x && !a.w) || (a.g_w && (!a.x || !a.workspace))) return PTV2_ERR_ARG;
    if (a.g_w && a.workspace_bytes < ptv2_oct_dwconv_workspace_bytes(a.n, a.c)) return PTV2_ERR_WORKSPACE;
    if (a.g_x) RUN(oct_dwconv_launch<true>(a.n, a.c, a.nbr, a.g_y, a.w, a.g_x, (hipStream_t)stream));
    if (a.g_w) {
        const int blocks = oct_dwconv_blocks(a.n, a.c, OCT_GW_MAX_BLOCKS), elems = OCT_NBR * a.c;
        hipLaunchKernelGGL(oct_dwconv_gw_kernel, dim3(blocks), dim3(OCT_TPB), 0, (hipStream_t)stream, a.n, a.c, a.nbr, a.x, a.g_y,
                           (float *)a.workspace);
        PTV2_CHECK_LAUNCH();
        hipLaunchKernelGGL(oct_dwconv_gw_finalize_kernel, dim3(divup(elems, OCT_TPB)), dim3(OCT_TPB), 0, (hipStream_t)stream, blocks,
                           elems, (const float *)a.workspace, a.g_w);
        PTV2_CHECK_LAUNCH();
    }
    return PTV2_OK;
}
