// ao_amd/csrc/msc_tile.h -- what the two Masked Scene Contrast units share (msc.hip: MSC-v1m1, msc_csc.hip: MSC-v1m2): the
// gather + normalise kernel, the 64 x 64 tile of S = A B^T on v_mfma_f32_32x32x2_f32, the fixed-order reductions, and the
// normalisation's backward with its sorted segment sum.  Everything has internal linkage: each unit compiles its own copy.
#pragma once
#include <cfloat>

#include "common.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int TPB = 256;
constexpr int TILE = 64;       // rows and columns of one workgroup tile: 2 x 2 wavefront tiles of 32 x 32
constexpr int KC = 32;         // channels staged per round
constexpr int KP = KC + 4;     // LDS pitch of a staged row (float4 aligned)
constexpr int PP = TILE + 1;   // LDS pitch of the P tile (read one float per lane down a column)
constexpr int MAX_SPLIT_BLOCKS = 1024;  // the column splits stop growing once the grid has this many workgroups
constexpr float EPS = 1e-7f;

__device__ __forceinline__ float wave_sum(float v) {
    // butterfly: every lane ends with the same bits (a + b == b + a)
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// row of accumulator register `reg` of a 32 x 32 tile in lane half h; the column is lane & 31
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// (m1, s1) <- (m1, s1) + (m2, s2), sums of exp(x - m)
__device__ __forceinline__ void lse_merge(float &m1, float &s1, float m2, float s2) {
    const float mx = fmaxf(m1, m2);
    s1 = s1 * expf(m1 - mx) + s2 * expf(m2 - mx);
    m1 = mx;
}

// ------------------------------------------------------------------------------------------------- gather + normalise ----
__global__ __launch_bounds__(64) void msc_gather_norm_kernel(int n1, int n2, int m, int c, const float *__restrict__ f1,
                                                             const float *__restrict__ f2, const long long *__restrict__ pairs,
                                                             float *__restrict__ A, float *__restrict__ B,
                                                             float *__restrict__ norms, float *__restrict__ pos, int *status) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const long long p0 = pairs[2 * (size_t)i], p1 = pairs[2 * (size_t)i + 1];
    const bool ok0 = p0 >= 0 && p0 < n1, ok1 = p1 >= 0 && p1 < n2;
    if (lane == 0 && !(ok0 && ok1)) *status = 1;
    const bool act = 4 * lane < c;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
    if (act && ok0) x = *(const float4 *)(f1 + (size_t)p0 * c + 4 * lane);
    if (act && ok1) y = *(const float4 *)(f2 + (size_t)p1 * c + 4 * lane);
    const float na = sqrtf(wave_sum(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w));
    const float nb = sqrtf(wave_sum(y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w));
    const float da = na + EPS, db = nb + EPS;
    x.x /= da; x.y /= da; x.z /= da; x.w /= da;
    y.x /= db; y.y /= db; y.z /= db; y.w /= db;
    const float dot = wave_sum(x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w);
    if (act) {
        *(float4 *)(A + (size_t)i * c + 4 * lane) = x;
        *(float4 *)(B + (size_t)i * c + 4 * lane) = y;
    }
    if (lane == 0) {
        norms[i] = na;
        norms[m + i] = nb;
        pos[i] = dot;
    }
}

// -------------------------------------------------------------------------------------------------------- the S tile ----
// The wavefront's 32 x 32 quadrant (rt, ct) of X[x0, x0 + 64) . Y[y0, y0 + 64)^T over all c channels, staged KC channels at a
// time through LDS by the whole workgroup (every thread of the workgroup calls this with the same x0, y0).  Rows past m read
// as zeros.  A lane feeds the k pairs (kk + j, kk + 4 + j), j = 0..3, of one float4 per operand: any order of k serves, as
// long as both operands use the same one.
__device__ __forceinline__ v16f s_tile(const float *__restrict__ X, int x0, const float *__restrict__ Y, int y0, int m, int c,
                                       float (*sX)[KP], float (*sY)[KP], int rt, int ct) {
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    v16f acc;
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int k0 = 0; k0 < c; k0 += KC) {
        __syncthreads();
        for (int e = tid; e < TILE * (KC / 4); e += TPB) {
            const int row = e >> 3, k = k0 + 4 * (e & 7);
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (k < c) {
                if (x0 + row < m) va = *(const float4 *)(X + (size_t)(x0 + row) * c + k);
                if (y0 + row < m) vb = *(const float4 *)(Y + (size_t)(y0 + row) * c + k);
            }
            *(float4 *)&sX[row][4 * (e & 7)] = va;
            *(float4 *)&sY[row][4 * (e & 7)] = vb;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KC; kk += 8) {
            const float4 a = *(const float4 *)&sX[32 * rt + r][kk + 4 * h];
            const float4 b = *(const float4 *)&sY[32 * ct + r][kk + 4 * h];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    return acc;
}

__device__ __forceinline__ double block_sum(double v, double *sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = TPB / 2; o; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    return sh[0];
}

// One wavefront per position s of the stable sort of column `col` of pairs.  The first position of a run sums the run in sort
// order: the gradient through x / (|x| + eps) of each of its rows, d / (n + eps) - a (d . a) / n (the norm's gradient at the
// zero vector is 0), into df[index].  df was cleared before.
__global__ __launch_bounds__(64) void msc_scatter_kernel(int n, int m, int c, int col, const long long *__restrict__ pairs,
                                                         const int *__restrict__ order, const float *__restrict__ dN,
                                                         const float *__restrict__ N, const float *__restrict__ norm,
                                                         float *__restrict__ df) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int r0 = order[s];
    if (r0 < 0 || r0 >= m) return;
    const long long idx = pairs[2 * (size_t)r0 + col];
    if (idx < 0 || idx >= n) return;
    if (s > 0) {
        const int rp = order[s - 1];
        if (rp >= 0 && rp < m && pairs[2 * (size_t)rp + col] == idx) return;
    }
    const bool act = 4 * lane < c;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = s; q < m; ++q) {
        const int row = order[q];
        if (row < 0 || row >= m || pairs[2 * (size_t)row + col] != idx) break;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f), a = d;
        if (act) {
            d = *(const float4 *)(dN + (size_t)row * c + 4 * lane);
            a = *(const float4 *)(N + (size_t)row * c + 4 * lane);
        }
        const float dot = wave_sum(d.x * a.x + d.y * a.y + d.z * a.z + d.w * a.w);
        const float nr = norm[row];
        const float inv = 1.f / (nr + EPS), w = nr > 0.f ? dot / nr : 0.f;
        acc.x += d.x * inv - a.x * w;
        acc.y += d.y * inv - a.y * w;
        acc.z += d.z * inv - a.z * w;
        acc.w += d.w * inv - a.w * w;
    }
    if (act) *(float4 *)(df + (size_t)idx * c + 4 * lane) = acc;
}

}  // namespace
