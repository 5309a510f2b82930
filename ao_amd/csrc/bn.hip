// ao_amd/csrc/bn.hip -- BatchNorm1d over the N rows of a per-point (N,C) tensor on gfx950 (training / eval), with the optional
// fused ReLU and the Block tail y = ReLU(residual + rowscale * BN(x)), forward and backward: statistics from a pass over x or
// from the tile records the producing GEMM / attention kernel left (one or two tensors per launch), apply, backward reduce /
// finalize / apply, and for few records the record sums inside the apply launch (bn_tiles_apply_residual_kernel,
// bn_bwd_finapply_kernel).  The q / k BatchNorms' reduce inside the skinny input-gradient launch is in skinny.hip.
//
// Why these exist.  PT-v2m2 wraps every Linear in PointBatchNorm (+ReLU)
// (point_transformer_v2m2_base.py:26-45,67-76,153-177): 86 BatchNorms per training step at S3DIS sizes.
// The stock channels-last BN kernels stream (N,48..384) fp32 at ~0.65 TB/s (profiles/r01_fused_v1_*): pure HBM streaming.
//   bn_stats / bn_backward_reduce  column sums over row chunks, float4 per lane, per-block partials +
//                                  fixed-order final (bitwise reproducible); the finalizer also writes
//                                  mean / rstd and updates the running statistics in place
//   bn_apply / bn_backward_apply   one read-modify-write pass each
#include "dense_common.h"

namespace dense {

// ------------------------------------------------------------------ BN: stats --
// lanes: (row lane, float4 column quad); requires c % 4 == 0
__global__ __launch_bounds__(TPB) void bn_stats_kernel(int n, int c, const float *__restrict__ x,
                                                       float *__restrict__ part) {
    extern __shared__ float4 lds4[];
    const int cq = c >> 2;
    const int rl = TPB / cq;                 // row lanes per block (>= 1 for c <= 1024)
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    // sums of (x - x[0,:]): shifting by one sample of the column removes the catastrophic cancellation of
    // E[x^2] - E[x]^2 when |mean| >> std, at no extra pass
    const float4 sft = ((const float4 *)x)[q];
    if (r < rl)
#pragma unroll 4
        for (long long row = (long long)blockIdx.x * rl + r; row < n; row += (long long)gridDim.x * rl) {
            float4 v = ((const float4 *)x)[row * cq + q];
            v.x -= sft.x; v.y -= sft.y; v.z -= sft.z; v.w -= sft.w;
            s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
            s2.x = __builtin_fmaf(v.x, v.x, s2.x); s2.y = __builtin_fmaf(v.y, v.y, s2.y);
            s2.z = __builtin_fmaf(v.z, v.z, s2.z); s2.w = __builtin_fmaf(v.w, v.w, s2.w);
        }
    float4 *sa = lds4, *sb = lds4 + TPB;
    sa[threadIdx.x] = s1;
    sb[threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x < cq) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        for (int k = 0; k < rl; ++k) {
            const float4 u = sa[k * cq + threadIdx.x], w = sb[k * cq + threadIdx.x];
            a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
            b.x += w.x; b.y += w.y; b.z += w.z; b.w += w.w;
        }
        float *p = part + (size_t)blockIdx.x * 2 * c;
        ((float4 *)p)[threadIdx.x] = a;
        ((float4 *)(p + c))[threadIdx.x] = b;
    }
}

// finalize: column sums of (x-x0) and (x-x0)^2 over the per-block partials -> mean, rstd, running statistics
template <int COLS>
__global__ __launch_bounds__(1024) void bn_finalize_kernel(
    const float *__restrict__ part, int nblk, int c, int n, const float *__restrict__ x0, float eps, float momentum,
    float *__restrict__ mean, float *__restrict__ rstd, float *run_mean, float *run_var, long long *batches,
    const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ sc, float *__restrict__ sh) {
    constexpr int SLICES = 1024 / COLS;
    __shared__ double s1[SLICES][COLS], s2[SLICES][COLS];
    const int col = threadIdx.x & (COLS - 1), sl = threadIdx.x / COLS;
    const int ch = blockIdx.x * COLS + col;
    double a = 0.0, b = 0.0, a2 = 0.0, b2 = 0.0;
    if (ch < c) {
        int k = sl;
        for (; k + SLICES < nblk; k += 2 * SLICES) {
            a += (double)part[(size_t)k * 2 * c + ch];
            b += (double)part[(size_t)k * 2 * c + c + ch];
            a2 += (double)part[(size_t)(k + SLICES) * 2 * c + ch];
            b2 += (double)part[(size_t)(k + SLICES) * 2 * c + c + ch];
        }
        for (; k < nblk; k += SLICES) {
            a += (double)part[(size_t)k * 2 * c + ch];
            b += (double)part[(size_t)k * 2 * c + c + ch];
        }
    }
    s1[sl][col] = a + a2;
    s2[sl][col] = b + b2;
    __syncthreads();
    if (sl == 0 && ch < c) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll 8
        for (int t = 0; t < SLICES; ++t) { t1 += s1[t][col]; t2 += s2[t][col]; }
        const double d = t1 / n;                       // mean of the shifted samples
        const double m = (double)x0[ch] + d;
        double var = t2 / n - d * d;
        var = var > 0.0 ? var : 0.0;
        mean[ch] = (float)m;
        rstd[ch] = (float)(1.0 / sqrt(var + (double)eps));
        if (sc) {  // y = x * sc + sh is the whole normalisation: consumers apply it on their operand load
            const float scale = rstd[ch] * gamma[ch];
            sc[ch] = scale;
            sh[ch] = beta[ch] - mean[ch] * scale;
        }
        if (run_mean) {
            const double unb = n > 1 ? var * ((double)n / (double)(n - 1)) : var;
            run_mean[ch] = (float)((1.0 - momentum) * (double)run_mean[ch] + momentum * m);
            run_var[ch] = (float)((1.0 - momentum) * (double)run_var[ch] + momentum * unb);
            if (ch == 0 && batches) *batches += 1;
        }
    }
}

// the same from the row GEMM's epilogue records part[nrb][2][c] (per 64-row block: column sums and sums of squares
// about the block mean), merged with the parallel-variance identity  M2 = sum_b (M2_b + S_b^2 / n_b) - n mean^2
// one or two BnTileSet (dense_common.h) per launch (blockIdx.z selects the set: the q / k BatchNorms of a Block are finished together)
__device__ __forceinline__ int bn_tile_rows(const BnTileSet &S, int k, int n) {  // rows of record k
    const int rb = S.rb ? S.rb : 64;
    return (n - k * rb) < rb ? (n - k * rb) : rb;
}

__device__ __forceinline__ void bn_tiles_emit(const BnTileSet &S, int ch, double t1, double t2, int n, float eps, float momentum) {
    const double m = t1 / n;
    double var = t2 / n - m * m;
    var = var > 0.0 ? var : 0.0;
    S.mean[ch] = (float)m;
    S.rstd[ch] = (float)(1.0 / sqrt(var + (double)eps));
    if (S.sc) {
        const float scale = S.rstd[ch] * S.gamma[ch];
        S.sc[ch] = scale;
        S.sh[ch] = S.beta[ch] - S.mean[ch] * scale;
    }
    if (S.run_mean) {
        const double unb = n > 1 ? var * ((double)n / (double)(n - 1)) : var;
        S.run_mean[ch] = (float)((1.0 - momentum) * (double)S.run_mean[ch] + momentum * m);
        S.run_var[ch] = (float)((1.0 - momentum) * (double)S.run_var[ch] + momentum * unb);
        if (ch == 0 && S.batches) *S.batches += 1;
    }
}

template <int COLS>
__global__ __launch_bounds__(1024) void bn_finalize_tiles_kernel(BnTileSet A, BnTileSet B, int nrb, int c, int n, float eps,
                                                                 float momentum) {
    constexpr int SLICES = 1024 / COLS;
    __shared__ double s1[SLICES][COLS], s2[SLICES][COLS];
    const BnTileSet &S = blockIdx.z ? B : A;
    const float *__restrict__ part = S.part;
    const int col = threadIdx.x & (COLS - 1), sl = threadIdx.x / COLS;
    const int ch = blockIdx.x * COLS + col;
    double a = 0.0, b = 0.0, a2 = 0.0, b2 = 0.0;
    if (ch < c) {
        auto rec = [&](int k, double &sa, double &sq) {
            const int cnt = bn_tile_rows(S, k, n);
            const double sb = (double)part[(size_t)k * 2 * c + ch];
            sa += sb;
            sq += (double)part[(size_t)k * 2 * c + c + ch] + sb * sb / (double)cnt;
        };
        int k = sl;
        // eight records (16 loads) in flight per trip, added in the order of the two-chain loop below (same bits): at the full
        // resolution (1 875 records, 3-6 workgroups) that loop was 15 dependent trips, 12.5 us on the critical path of every
        // BatchNorm of a level-0 Block
        for (; k + 7 * SLICES < nrb; k += 8 * SLICES) {
            float s[8], m[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s[u] = part[(size_t)(k + u * SLICES) * 2 * c + ch];
                m[u] = part[(size_t)(k + u * SLICES) * 2 * c + c + ch];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int kk = k + u * SLICES;
                const int cnt = bn_tile_rows(S, kk, n);
                const double sb = (double)s[u];
                if (u & 1) { a2 += sb; b2 += (double)m[u] + sb * sb / (double)cnt; }
                else { a += sb; b += (double)m[u] + sb * sb / (double)cnt; }
            }
        }
        for (; k + SLICES < nrb; k += 2 * SLICES) {  // two independent chains: the loads of both records are in flight
            rec(k, a, b);
            rec(k + SLICES, a2, b2);
        }
        for (; k < nrb; k += SLICES) rec(k, a, b);
    }
    s1[sl][col] = a + a2;
    s2[sl][col] = b + b2;
    __syncthreads();
    if (sl == 0 && ch < c) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll 8
        for (int t = 0; t < SLICES; ++t) { t1 += s1[t][col]; t2 += s2[t][col]; }
        bn_tiles_emit(S, ch, t1, t2, n, eps, momentum);
    }
}

// the same for MANY records (the full-resolution level: 1 875 records, c / 16 = 3 column blocks): 3 workgroups walking 29
// records per thread were 12 us of dependent round trips on the critical path of every BatchNorm of a level-0 Block.  Here
// NS workgroups per column block each fold a share of the records into one float64 partial (S.fold), and the last of them to
// arrive (one counter per column block and tensor; the workgroups are few and the partials 256 bytes, so the arrival protocol
// is cheap here) adds the NS partials in index order and emits.
constexpr int BNT_NS = 8;
__global__ __launch_bounds__(1024) void bn_finalize_tiles_split_kernel(BnTileSet A, BnTileSet B, int nrb, int c, int n, float eps,
                                                                       float momentum, unsigned *counters) {
    constexpr int COLS = 16, SLICES = 64;
    __shared__ double s1[SLICES][COLS], s2[SLICES][COLS];
    __shared__ int s_last;
    const BnTileSet &S = blockIdx.z ? B : A;
    const float *__restrict__ part = S.part;
    const int col = threadIdx.x & (COLS - 1), sl = threadIdx.x / COLS;
    const int ch = blockIdx.x * COLS + col;
    double a = 0.0, b = 0.0;
    if (ch < c) {
        for (int k = blockIdx.y * SLICES + sl; k < nrb; k += BNT_NS * SLICES) {
            const int cnt = bn_tile_rows(S, k, n);
            const double sb = (double)part[(size_t)k * 2 * c + ch];
            a += sb;
            b += (double)part[(size_t)k * 2 * c + c + ch] + sb * sb / (double)cnt;
        }
    }
    s1[sl][col] = a;
    s2[sl][col] = b;
    __syncthreads();
    double *fold = S.fold + ((size_t)blockIdx.y * 2) * c;  // [NS][2][c]
    if (sl == 0 && ch < c) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll 8
        for (int t = 0; t < SLICES; ++t) { t1 += s1[t][col]; t2 += s2[t][col]; }
        __hip_atomic_store(fold + ch, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(fold + c + ch, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the fold stores are acknowledged before the arrival is published (gva_common.h: last_block_arrives)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned *cnt = counters + blockIdx.z * gridDim.x + blockIdx.x;
        const unsigned prev = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == BNT_NS - 1;
        if (s_last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (sl == 0 && ch < c) {
        double t1 = 0.0, t2 = 0.0;
        for (int p = 0; p < BNT_NS; ++p) {
            t1 += __hip_atomic_load(S.fold + ((size_t)p * 2) * c + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t2 += __hip_atomic_load(S.fold + ((size_t)p * 2) * c + c + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        bn_tiles_emit(S, ch, t1, t2, n, eps, momentum);
    }
}

// ------------------------------------------------------------------ BN: apply --
__global__ __launch_bounds__(TPB) void bn_apply_kernel(long long total4, int cq, const float *__restrict__ x,
                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       int relu, float *__restrict__ y) {
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total4; e += (long long)gridDim.x * TPB) {
        const int q = (int)(e % cq);
        const float4 v = ((const float4 *)x)[e];
        const float4 m = ((const float4 *)mean)[q], r = ((const float4 *)rstd)[q];
        const float4 g = ((const float4 *)gamma)[q], b = ((const float4 *)beta)[q];
        float4 o;
        o.x = __builtin_fmaf((v.x - m.x) * r.x, g.x, b.x);
        o.y = __builtin_fmaf((v.y - m.y) * r.y, g.y, b.y);
        o.z = __builtin_fmaf((v.z - m.z) * r.z, g.z, b.z);
        o.w = __builtin_fmaf((v.w - m.w) * r.w, g.w, b.w);
        if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        ((float4 *)y)[e] = o;
    }
}

// Block tail fused into the last BatchNorm of a Block (point_transformer_v2m2_base.py:174-176):
//   y = ReLU(residual + rowscale[n] * BN(x))      rowscale = per-point DropPath factor (0 or 1/keep), may be NULL
__global__ __launch_bounds__(TPB) void bn_apply_residual_kernel(long long total4, int cq, const float *__restrict__ x,
                                                                const float *__restrict__ mean,
                                                                const float *__restrict__ rstd,
                                                                const float *__restrict__ gamma,
                                                                const float *__restrict__ beta,
                                                                const float *__restrict__ residual,
                                                                const float *__restrict__ rowscale,
                                                                float *__restrict__ y) {
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total4; e += (long long)gridDim.x * TPB) {
        const int q = (int)(e % cq);
        const float rsc = rowscale ? rowscale[e / cq] : 1.f;
        const float4 v = ((const float4 *)x)[e], res = ((const float4 *)residual)[e];
        const float4 m = ((const float4 *)mean)[q], r = ((const float4 *)rstd)[q];
        const float4 g = ((const float4 *)gamma)[q], b = ((const float4 *)beta)[q];
        float4 o;
        o.x = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.x - m.x) * r.x, g.x, b.x), res.x), 0.f);
        o.y = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.y - m.y) * r.y, g.y, b.y), res.y), 0.f);
        o.z = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.z - m.z) * r.z, g.z, b.z), res.z), 0.f);
        o.w = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.w - m.w) * r.w, g.w, b.w), res.w), 0.f);
        ((float4 *)y)[e] = o;
    }
}

// backward of the fused tail: d = gy * (y > 0) is the gradient of the residual; d * rowscale[n] enters the BN backward
__global__ __launch_bounds__(TPB) void bn_bwd_reduce_residual_kernel(int n, int c, const float *__restrict__ x,
                                                                     const float *__restrict__ gy,
                                                                     const float *__restrict__ y,
                                                                     const float *__restrict__ rowscale,
                                                                     const float *__restrict__ mean,
                                                                     const float *__restrict__ rstd,
                                                                     float *__restrict__ part) {
    extern __shared__ float4 lds4[];
    const int cq = c >> 2;
    const int rl = TPB / cq;
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    if (r < rl) {
        const float4 m = ((const float4 *)mean)[q], rs = ((const float4 *)rstd)[q];
#pragma unroll 4
        for (long long row = (long long)blockIdx.x * rl + r; row < n; row += (long long)gridDim.x * rl) {
            const float4 v = ((const float4 *)x)[row * cq + q], o = ((const float4 *)y)[row * cq + q];
            float4 d = ((const float4 *)gy)[row * cq + q];
            const float rsc = rowscale ? rowscale[row] : 1.f;
            d.x = o.x > 0.f ? d.x * rsc : 0.f; d.y = o.y > 0.f ? d.y * rsc : 0.f;
            d.z = o.z > 0.f ? d.z * rsc : 0.f; d.w = o.w > 0.f ? d.w * rsc : 0.f;
            s1.x += d.x; s1.y += d.y; s1.z += d.z; s1.w += d.w;
            s2.x = __builtin_fmaf(d.x, (v.x - m.x) * rs.x, s2.x); s2.y = __builtin_fmaf(d.y, (v.y - m.y) * rs.y, s2.y);
            s2.z = __builtin_fmaf(d.z, (v.z - m.z) * rs.z, s2.z); s2.w = __builtin_fmaf(d.w, (v.w - m.w) * rs.w, s2.w);
        }
    }
    float4 *sa = lds4, *sb = lds4 + TPB;
    sa[threadIdx.x] = s1;
    sb[threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x < cq) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b2 = a;
        for (int k = 0; k < rl; ++k) {
            const float4 u = sa[k * cq + threadIdx.x], w = sb[k * cq + threadIdx.x];
            a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
            b2.x += w.x; b2.y += w.y; b2.z += w.z; b2.w += w.w;
        }
        float *p = part + (size_t)blockIdx.x * 2 * c;
        ((float4 *)p)[threadIdx.x] = a;
        ((float4 *)(p + c))[threadIdx.x] = b2;
    }
}

__global__ __launch_bounds__(TPB) void bn_bwd_apply_residual_kernel(
    long long total4, int cq, float inv_n, const float *__restrict__ x, const float *__restrict__ gy,
    const float *__restrict__ y, const float *__restrict__ rowscale, const float *__restrict__ mean,
    const float *__restrict__ rstd, const float *__restrict__ gamma, const float *__restrict__ dbeta,
    const float *__restrict__ dgamma, int training, float *__restrict__ gx, float *__restrict__ g_residual) {
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total4; e += (long long)gridDim.x * TPB) {
        const int q = (int)(e % cq);
        const float rsc = rowscale ? rowscale[e / cq] : 1.f;
        const float4 v = ((const float4 *)x)[e], o = ((const float4 *)y)[e];
        float4 d = ((const float4 *)gy)[e];
        d.x = o.x > 0.f ? d.x : 0.f; d.y = o.y > 0.f ? d.y : 0.f; d.z = o.z > 0.f ? d.z : 0.f; d.w = o.w > 0.f ? d.w : 0.f;
        ((float4 *)g_residual)[e] = d;
        d.x *= rsc; d.y *= rsc; d.z *= rsc; d.w *= rsc;
        const float4 m = ((const float4 *)mean)[q], rs = ((const float4 *)rstd)[q], g = ((const float4 *)gamma)[q];
        float4 out;
        if (training) {
            const float4 db = ((const float4 *)dbeta)[q], dg = ((const float4 *)dgamma)[q];
            out.x = g.x * rs.x * (d.x - db.x * inv_n - (v.x - m.x) * rs.x * dg.x * inv_n);
            out.y = g.y * rs.y * (d.y - db.y * inv_n - (v.y - m.y) * rs.y * dg.y * inv_n);
            out.z = g.z * rs.z * (d.z - db.z * inv_n - (v.z - m.z) * rs.z * dg.z * inv_n);
            out.w = g.w * rs.w * (d.w - db.w * inv_n - (v.w - m.w) * rs.w * dg.w * inv_n);
        } else {
            out.x = g.x * rs.x * d.x; out.y = g.y * rs.y * d.y; out.z = g.z * rs.z * d.z; out.w = g.w * rs.w * d.w;
        }
        ((float4 *)gx)[e] = out;
    }
}

// a second, independent BatchNorm of the same shape handled by blockIdx.y == 1 of the same launches (linear_q and
// linear_k of a Block: their backward chains are independent, batching them saves three launches per Block)
struct BnSecond {
    const float *x, *gy, *mean, *rstd, *gamma, *beta;
    float *gx, *dgamma, *dbeta;
};

// -------------------------------------------------------- BN: backward reduce --
// partial columns [0,c): sum gy' ; [c,2c): sum gy' * xhat, with gy' = gy masked by the fused ReLU
__global__ __launch_bounds__(TPB) void bn_bwd_reduce_kernel(int n, int c, const float *x, const float *gy,
                                                            const float *mean, const float *rstd, const float *gamma,
                                                            const float *beta, int relu, float *__restrict__ part,
                                                            BnSecond second) {
    extern __shared__ float4 lds4[];
    if (blockIdx.y) { x = second.x; gy = second.gy; mean = second.mean; rstd = second.rstd; gamma = second.gamma; beta = second.beta; }
    const int cq = c >> 2;
    const int rl = TPB / cq;
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    if (r < rl) {
        const float4 m = ((const float4 *)mean)[q], rs = ((const float4 *)rstd)[q];
        const float4 g = ((const float4 *)gamma)[q], b = ((const float4 *)beta)[q];
#pragma unroll 4
        for (long long row = (long long)blockIdx.x * rl + r; row < n; row += (long long)gridDim.x * rl) {
            const float4 v = ((const float4 *)x)[row * cq + q];
            float4 d = ((const float4 *)gy)[row * cq + q];
            float4 h;
            h.x = (v.x - m.x) * rs.x; h.y = (v.y - m.y) * rs.y; h.z = (v.z - m.z) * rs.z; h.w = (v.w - m.w) * rs.w;
            if (relu) {
                if (__builtin_fmaf(h.x, g.x, b.x) <= 0.f) d.x = 0.f;
                if (__builtin_fmaf(h.y, g.y, b.y) <= 0.f) d.y = 0.f;
                if (__builtin_fmaf(h.z, g.z, b.z) <= 0.f) d.z = 0.f;
                if (__builtin_fmaf(h.w, g.w, b.w) <= 0.f) d.w = 0.f;
            }
            s1.x += d.x; s1.y += d.y; s1.z += d.z; s1.w += d.w;
            s2.x = __builtin_fmaf(d.x, h.x, s2.x); s2.y = __builtin_fmaf(d.y, h.y, s2.y);
            s2.z = __builtin_fmaf(d.z, h.z, s2.z); s2.w = __builtin_fmaf(d.w, h.w, s2.w);
        }
    }
    float4 *sa = lds4, *sb = lds4 + TPB;
    sa[threadIdx.x] = s1;
    sb[threadIdx.x] = s2;
    __syncthreads();
    if (threadIdx.x < cq) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b2 = a;
        for (int k = 0; k < rl; ++k) {
            const float4 u = sa[k * cq + threadIdx.x], w = sb[k * cq + threadIdx.x];
            a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
            b2.x += w.x; b2.y += w.y; b2.z += w.z; b2.w += w.w;
        }
        float *p = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 * c;  // record of a block: [set 0 | set 1]
        ((float4 *)p)[threadIdx.x] = a;
        ((float4 *)(p + c))[threadIdx.x] = b2;
    }
}

// gx = gamma * rstd * (gy' - dbeta/n - xhat * dgamma/n)   (training);   gamma * rstd * gy' (eval)
__global__ __launch_bounds__(TPB) void bn_bwd_apply_kernel(long long total4, int cq, float inv_n, const float *x,
                                                           const float *gy, const float *mean, const float *rstd,
                                                           const float *gamma, const float *beta, int relu,
                                                           const float *dbeta, const float *dgamma, int training, float *gx,
                                                           BnSecond second) {
    if (blockIdx.y) {
        x = second.x; gy = second.gy; mean = second.mean; rstd = second.rstd; gamma = second.gamma; beta = second.beta;
        dbeta = second.dbeta; dgamma = second.dgamma; gx = second.gx;
    }
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total4; e += (long long)gridDim.x * TPB) {
        const int q = (int)(e % cq);
        const float4 v = ((const float4 *)x)[e];
        float4 d = ((const float4 *)gy)[e];
        const float4 m = ((const float4 *)mean)[q], rs = ((const float4 *)rstd)[q];
        const float4 g = ((const float4 *)gamma)[q], b = ((const float4 *)beta)[q];
        float4 h;
        h.x = (v.x - m.x) * rs.x; h.y = (v.y - m.y) * rs.y; h.z = (v.z - m.z) * rs.z; h.w = (v.w - m.w) * rs.w;
        if (relu) {
            if (__builtin_fmaf(h.x, g.x, b.x) <= 0.f) d.x = 0.f;
            if (__builtin_fmaf(h.y, g.y, b.y) <= 0.f) d.y = 0.f;
            if (__builtin_fmaf(h.z, g.z, b.z) <= 0.f) d.z = 0.f;
            if (__builtin_fmaf(h.w, g.w, b.w) <= 0.f) d.w = 0.f;
        }
        float4 o;
        if (training) {
            const float4 db = ((const float4 *)dbeta)[q], dg = ((const float4 *)dgamma)[q];
            o.x = g.x * rs.x * (d.x - db.x * inv_n - h.x * dg.x * inv_n);
            o.y = g.y * rs.y * (d.y - db.y * inv_n - h.y * dg.y * inv_n);
            o.z = g.z * rs.z * (d.z - db.z * inv_n - h.z * dg.z * inv_n);
            o.w = g.w * rs.w * (d.w - db.w * inv_n - h.w * dg.w * inv_n);
        } else {
            o.x = g.x * rs.x * d.x; o.y = g.y * rs.y * d.y; o.z = g.z * rs.z * d.z; o.w = g.w * rs.w * d.w;
        }
        ((float4 *)gx)[e] = o;
    }
}

constexpr int FA_COLS = 32, FA_ROWS = 128;  // consumer-side record sums: stripe width (columns), rows per workgroup

// ------------------------------- BN forward tail: tile-record merge + residual apply in one launch --
// The Block tail y = ReLU(x + rowscale * BN3(h3)) at the deep levels: the workgroups of the apply kernel (64-column stripe x
// 128 rows) merge the stripe's tile records of the producing GEMM themselves (parallel-variance identity in float64, as
// bn_finalize_tiles_kernel) instead of waiting for a finalize launch; the row-chunk-0 workgroups deliver mean / rstd /
// folded affine / running statistics for the backward and the optimizer.
// RESIDUAL = false: y = ReLU(BN(x)) (`relu` = residual == NULL ... see the launcher) -- the Linear + BatchNorm + ReLU layers
// between the Blocks (GridPool.fc, UnpoolWithSkip.proj / proj_skip: model.hip linbn_forward)
template <int PLAIN>
__global__ __launch_bounds__(TPB) void bn_tiles_apply_residual_kernel(BnTileSet S, int nrb, int n, int c, float eps, float momentum,
                                                                      const float *__restrict__ x,
                                                                      const float *__restrict__ residual,
                                                                      const float *__restrict__ rowscale, float *__restrict__ y) {
    constexpr int SL = TPB / FA_COLS;  // record slices
    __shared__ double s_a[SL][FA_COLS], s_b[SL][FA_COLS];
    __shared__ __attribute__((aligned(16))) float s_mean[FA_COLS], s_rstd[FA_COLS];
    const int col0 = blockIdx.x * FA_COLS;
    const int ncol = (c - col0) < FA_COLS ? (c - col0) : FA_COLS;
    {
        const int cj = threadIdx.x & (FA_COLS - 1), sl = threadIdx.x / FA_COLS;
        double a = 0.0, b = 0.0;
        if (cj < ncol) {
            const float *p = S.part + col0 + cj;
            int k = sl;
            for (; k + 3 * SL < nrb; k += 4 * SL) {  // four records (eight loads) of this slice in flight
                float sv[4], mv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { sv[u] = p[(size_t)(k + u * SL) * 2 * c]; mv[u] = p[(size_t)(k + u * SL) * 2 * c + c]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int kk = k + u * SL;
                    const int cnt = bn_tile_rows(S, kk, n);
                    const double sb = (double)sv[u];
                    a += sb;
                    b += (double)mv[u] + sb * sb / (double)cnt;
                }
            }
            for (; k < nrb; k += SL) {
                const int cnt = bn_tile_rows(S, k, n);
                const double sb = (double)p[(size_t)k * 2 * c];
                a += sb;
                b += (double)p[(size_t)k * 2 * c + c] + sb * sb / (double)cnt;
            }
        }
        s_a[sl][cj] = a;
        s_b[sl][cj] = b;
    }
    __syncthreads();
    if (threadIdx.x < FA_COLS) {
        const int cj = threadIdx.x;
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int t = 0; t < SL; ++t) { t1 += s_a[t][cj]; t2 += s_b[t][cj]; }
        const double m = t1 / n;
        double var = t2 / n - m * m;
        var = var > 0.0 ? var : 0.0;
        s_mean[cj] = (float)m;
        s_rstd[cj] = (float)(1.0 / sqrt(var + (double)eps));
        if (blockIdx.y == 0 && cj < ncol) bn_tiles_emit(S, col0 + cj, t1, t2, n, eps, momentum);
    }
    __syncthreads();
    constexpr int QW = FA_COLS / 4, RL = TPB / QW;  // column quads of the stripe x row lanes
    const int cq = c >> 2, q = threadIdx.x % QW, rl = threadIdx.x / QW;
    const int qcol = (col0 >> 2) + q;
    if (4 * q >= ncol) return;
    const float4 m = *(const float4 *)(s_mean + 4 * q), r = *(const float4 *)(s_rstd + 4 * q);
    const float4 g = ((const float4 *)S.gamma)[qcol], b = ((const float4 *)S.beta)[qcol];
    const long long r0 = (long long)blockIdx.y * FA_ROWS;
    const long long r1 = (r0 + FA_ROWS) < (long long)n ? (r0 + FA_ROWS) : (long long)n;
    for (long long row = r0 + rl; row < r1; row += RL) {
        const long long e = row * cq + qcol;
        if (PLAIN) {
            const float4 v = ((const float4 *)x)[e];
            float4 o;
            o.x = fmaxf(__builtin_fmaf((v.x - m.x) * r.x, g.x, b.x), 0.f);
            o.y = fmaxf(__builtin_fmaf((v.y - m.y) * r.y, g.y, b.y), 0.f);
            o.z = fmaxf(__builtin_fmaf((v.z - m.z) * r.z, g.z, b.z), 0.f);
            o.w = fmaxf(__builtin_fmaf((v.w - m.w) * r.w, g.w, b.w), 0.f);
            ((float4 *)y)[e] = o;
            continue;
        }
        const float rsc = rowscale ? rowscale[row] : 1.f;
        const float4 v = ((const float4 *)x)[e], res = ((const float4 *)residual)[e];
        float4 o;
        o.x = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.x - m.x) * r.x, g.x, b.x), res.x), 0.f);
        o.y = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.y - m.y) * r.y, g.y, b.y), res.y), 0.f);
        o.z = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.z - m.z) * r.z, g.z, b.z), res.z), 0.f);
        o.w = fmaxf(__builtin_fmaf(rsc, __builtin_fmaf((v.w - m.w) * r.w, g.w, b.w), res.w), 0.f);
        ((float4 *)y)[e] = o;
    }
}

// ---------------------------------------- BN backward: finalize + apply in one launch --
// Deep levels (n <= ~8 k rows: a few dozen reduce records).  The BatchNorm backward was reduce -> finalize -> apply, the
// last two 5 us launches each of which is almost all launch boundary.  Here the apply kernel's workgroups own a 64-column
// stripe x a chunk of rows and first sum the stripe's 2 x 64 record columns themselves (nrec records of the reduce pass or
// of the producing GEMM's epilogue; <= 256 records x 128 columns = 128 KB of L2 reads per workgroup, a ~2 us prologue that
// every workgroup runs concurrently), then apply.  The row-chunk-0 workgroups also deliver dbeta / dgamma.  Column sums:
// thread (column, slice of 2) walks its records in float64, slices combined in slice order -- fixed association, bitwise
// reproducible.  blockIdx.z selects one of two independent BatchNorms of the same shape (linear_q / linear_k).
struct BnFinApply {
    const float *part; int nrec, rec_floats, off;   // record r, set columns: part[r * rec_floats + off + (0..c-1: dbeta, c..2c-1: dgamma)]
    const float *x, *gy, *mean, *rstd, *gamma, *beta;
    float *gx, *dbeta, *dgamma;
    // residual tail (bn_backward_residual): the ReLU mask comes from y > 0, d * rowscale enters the BatchNorm, d itself is
    // the residual gradient
    const float *y, *rowscale;
    float *g_residual;
};

template <bool RESIDUAL>
__global__ __launch_bounds__(TPB) void bn_bwd_finapply_kernel(int n, int c, int relu, int training, float inv_n, BnFinApply A0,
                                                              BnFinApply A1) {
    const BnFinApply &A = blockIdx.z ? A1 : A0;
    constexpr int SL = TPB / (2 * FA_COLS);  // record slices
    __shared__ double s_part[SL][2 * FA_COLS];
    __shared__ __attribute__((aligned(16))) float s_db[FA_COLS], s_dg[FA_COLS];
    const int col0 = blockIdx.x * FA_COLS;
    const int ncol = (c - col0) < FA_COLS ? (c - col0) : FA_COLS;
    {   // column sums of this stripe: thread -> (record column j of 2 * FA_COLS, slice sl of SL)
        const int j = threadIdx.x & (2 * FA_COLS - 1), sl = threadIdx.x / (2 * FA_COLS);
        const int which = j / FA_COLS, cj = j - which * FA_COLS;  // 0: dbeta, 1: dgamma
        double acc = 0.0;
        if (cj < ncol) {
            const float *p = A.part + A.off + (size_t)which * c + col0 + cj;
            const size_t rs = (size_t)A.rec_floats;
            int r = sl;
            for (; r + 7 * SL < A.nrec; r += 8 * SL) {  // eight records of this slice in flight (one chain: fixed order)
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + u * SL) * rs];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += (double)v[u];
            }
            for (; r < A.nrec; r += SL) acc += (double)p[(size_t)r * rs];
        }
        s_part[sl][j] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 2 * FA_COLS) {
        const int j = threadIdx.x, which = j / FA_COLS, cj = j - which * FA_COLS;
        double t = 0.0;
#pragma unroll
        for (int u = 0; u < SL; ++u) t += s_part[u][j];
        const float v = (float)t;
        (which ? s_dg : s_db)[cj] = v;
        if (blockIdx.y == 0 && cj < ncol) (which ? A.dgamma : A.dbeta)[col0 + cj] = v;
    }
    __syncthreads();
    constexpr int QW = FA_COLS / 4, RL = TPB / QW;  // column quads of the stripe x row lanes
    const int cq = c >> 2, q = threadIdx.x % QW, rl = threadIdx.x / QW;
    const int qcol = (col0 >> 2) + q;
    if (4 * q >= ncol) return;
    const float4 m = ((const float4 *)A.mean)[qcol], rs = ((const float4 *)A.rstd)[qcol], g = ((const float4 *)A.gamma)[qcol];
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!RESIDUAL && relu) b = ((const float4 *)A.beta)[qcol];
    const float4 db = *(const float4 *)(s_db + 4 * q), dg = *(const float4 *)(s_dg + 4 * q);
    const long long r0 = (long long)blockIdx.y * FA_ROWS;
    const long long r1 = (r0 + FA_ROWS) < (long long)n ? (r0 + FA_ROWS) : (long long)n;
    for (long long row = r0 + rl; row < r1; row += RL) {
        const long long e = row * cq + qcol;
        const float4 v = ((const float4 *)A.x)[e];
        float4 d = ((const float4 *)A.gy)[e];
        float4 h;
        h.x = (v.x - m.x) * rs.x; h.y = (v.y - m.y) * rs.y; h.z = (v.z - m.z) * rs.z; h.w = (v.w - m.w) * rs.w;
        if (RESIDUAL) {
            const float4 o = ((const float4 *)A.y)[e];
            const float rsc = A.rowscale ? A.rowscale[row] : 1.f;
            d.x = o.x > 0.f ? d.x : 0.f; d.y = o.y > 0.f ? d.y : 0.f; d.z = o.z > 0.f ? d.z : 0.f; d.w = o.w > 0.f ? d.w : 0.f;
            ((float4 *)A.g_residual)[e] = d;
            d.x *= rsc; d.y *= rsc; d.z *= rsc; d.w *= rsc;
        } else if (relu) {
            if (__builtin_fmaf(h.x, g.x, b.x) <= 0.f) d.x = 0.f;
            if (__builtin_fmaf(h.y, g.y, b.y) <= 0.f) d.y = 0.f;
            if (__builtin_fmaf(h.z, g.z, b.z) <= 0.f) d.z = 0.f;
            if (__builtin_fmaf(h.w, g.w, b.w) <= 0.f) d.w = 0.f;
        }
        float4 o;
        if (training) {
            o.x = g.x * rs.x * (d.x - db.x * inv_n - h.x * dg.x * inv_n);
            o.y = g.y * rs.y * (d.y - db.y * inv_n - h.y * dg.y * inv_n);
            o.z = g.z * rs.z * (d.z - db.z * inv_n - h.z * dg.z * inv_n);
            o.w = g.w * rs.w * (d.w - db.w * inv_n - h.w * dg.w * inv_n);
        } else {
            o.x = g.x * rs.x * d.x; o.y = g.y * rs.y * d.y; o.z = g.z * rs.z * d.z; o.w = g.w * rs.w * d.w;
        }
        ((float4 *)A.gx)[e] = o;
    }
}

// AO_AMD_BN_FINAPPLY=0 (the A/B switch of the tests, read on every call): the separate finalize + apply launches
static bool bn_finapply_off() { return ptv2_env_is("AO_AMD_BN_FINAPPLY", '0'); }
// records few enough for the consumer-side sum (and the switch is not off)
static bool finapply_ok(int n, int nrec) {
    // (n <= 32768 -- the second level of the bench scene, 19 k rows -- measured the same step to 0.01 ms: the separate finalize +
    // apply pair stays there)
    return nrec <= 640 && n <= 16384 && !bn_finapply_off();  // (640: the 16-row records of the k-split GEMM at <= 10 k rows)
}

static void launch_finapply(hipStream_t st, int n, int c, int relu, int training, bool residual, int sets, const BnFinApply &A0,
                            const BnFinApply &A1) {
    const dim3 grid((unsigned)((c + FA_COLS - 1) / FA_COLS), (unsigned)((n + FA_ROWS - 1) / FA_ROWS), (unsigned)sets);
    if (residual)
        hipLaunchKernelGGL(bn_bwd_finapply_kernel<true>, grid, dim3(TPB), 0, st, n, c, relu, training, 1.0f / (float)n, A0, A1);
    else
        hipLaunchKernelGGL(bn_bwd_finapply_kernel<false>, grid, dim3(TPB), 0, st, n, c, relu, training, 1.0f / (float)n, A0, A1);
}

}  // namespace dense

using namespace dense;

// statistics pass + finalize; gamma / beta / sc / sh != NULL additionally emit the folded affine
static int bn_stats_impl(int n, int c, const float *x, float *mean, float *rstd, float *running_mean, float *running_var,
                         long long *num_batches_tracked, float eps, float momentum, const float *gamma, const float *beta,
                         float *sc, float *sh, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 1 || c < 4 || c % 4 != 0 || c > 1024) return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < dense_workspace_bytes(n, c, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = bn_grid(n, c);
    float *part = (float *)workspace;
    {
        PtvScopedTimer t(KID_BN_STATS, st, 4.0 * n * c);
        hipLaunchKernelGGL(bn_stats_kernel, dim3(nblk), dim3(TPB), sizeof(float4) * 2 * TPB, st, n, c, x, part);
    }
    if (nblk >= 64)
        hipLaunchKernelGGL(bn_finalize_kernel<16>, dim3((c + 15) / 16), dim3(1024), 0, st, (const float *)part, nblk, c, n, x, eps,
                           momentum, mean, rstd, running_mean, running_var, num_batches_tracked, gamma, beta, sc, sh);
    else
        hipLaunchKernelGGL(bn_finalize_kernel<64>, dim3((c + 63) / 64), dim3(1024), 0, st, (const float *)part, nblk, c, n, x, eps,
                           momentum, mean, rstd, running_mean, running_var, num_batches_tracked, gamma, beta, sc, sh);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int bn_stats_hip_launcher(int n, int c, const float *x, float *mean, float *rstd, float *running_mean,
                                     float *running_var, long long *num_batches_tracked, float eps, float momentum,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    return bn_stats_impl(n, c, x, mean, rstd, running_mean, running_var, num_batches_tracked, eps, momentum, nullptr, nullptr,
                         nullptr, nullptr, workspace, workspace_bytes, stream);
}

// bn_stats that also emits the folded affine (sc = rstd * gamma, sh = beta - mean * sc) for consumers that apply the
// normalisation on their operand load (rows_gemm_fused, linear_wgrad_multi, skinny_linear_forward)
extern "C" int bn_stats_affine_hip_launcher(int n, int c, const float *x, const float *gamma, const float *beta, float *mean,
                                            float *rstd, float *sc, float *sh, float *running_mean, float *running_var,
                                            long long *num_batches_tracked, float eps, float momentum, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    if (!gamma || !beta || !sc || !sh) return PTV2_ERR_ARG;
    return bn_stats_impl(n, c, x, mean, rstd, running_mean, running_var, num_batches_tracked, eps, momentum, gamma, beta, sc, sh,
                         workspace, workspace_bytes, stream);
}

// first level for many records: block (x, y) folds records y, y + gridDim.y, ... of 64 columns into ONE record of
// the same form (sum; centred sum of squares; its row count is implied by the records it covers)
__global__ __launch_bounds__(gva::FIN_COLS *gva::FIN_SLICES) void bn_fold_tiles_kernel(BnTileSet A, BnTileSet B, int nrb, int c,
                                                                                       int n) {
    __shared__ double s1[gva::FIN_SLICES][gva::FIN_COLS], s2[gva::FIN_SLICES][gva::FIN_COLS];
    const BnTileSet &S = blockIdx.z ? B : A;
    const float *__restrict__ part = S.part;
    double *__restrict__ out = S.fold;
    const int col = threadIdx.x & (gva::FIN_COLS - 1), sl = threadIdx.x / gva::FIN_COLS;
    const int ch = blockIdx.x * gva::FIN_COLS + col;
    double a = 0.0, b = 0.0;
    if (ch < c) {
        for (int k = blockIdx.y * gva::FIN_SLICES + sl; k < nrb; k += gridDim.y * gva::FIN_SLICES) {
            const int cnt = bn_tile_rows(S, k, n);
            const double sb = (double)part[(size_t)k * 2 * c + ch];
            a += sb;
            b += (double)part[(size_t)k * 2 * c + c + ch] + sb * sb / (double)cnt;
        }
    }
    s1[sl][col] = a;
    s2[sl][col] = b;
    __syncthreads();
    if (sl == 0 && ch < c) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int t = 0; t < gva::FIN_SLICES; ++t) { t1 += s1[t][col]; t2 += s2[t][col]; }
        out[(size_t)blockIdx.y * 2 * c + ch] = t1;       // sum
        out[(size_t)blockIdx.y * 2 * c + c + ch] = t2;   // sum_b (M2_b + S_b^2 / n_b): only "- n mean^2" is missing
    }
}

// second level: nrec folded records (float64) -> mean, rstd, folded affine, running buffers
__global__ void bn_finalize_folded_kernel(BnTileSet A, BnTileSet B, int nrec, int c, int n, float eps, float momentum) {
    const BnTileSet &S = blockIdx.z ? B : A;
    const double *__restrict__ rec = S.fold;
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    double t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < nrec; ++k) { t1 += rec[(size_t)k * 2 * c + ch]; t2 += rec[(size_t)k * 2 * c + c + ch]; }
    bn_tiles_emit(S, ch, t1, t2, n, eps, momentum);
}

// statistics of a (n,c) tensor from the records its producing rows_gemm_fused launch left in `part`
extern "C" size_t bn_tiles_floats(int n, int c) {  // floats of a statistics record buffer (incl. the folding scratch)
    return (size_t)((n + 63) / 64) * 2 * c + 2 + 2 * (size_t)16 * 2 * c;
}
size_t bn_tiles_floats_rb(int n, int c, int rb) {  // the same for records of rb rows
    return (size_t)((n + rb - 1) / rb) * 2 * c + 2 + 2 * (size_t)16 * 2 * c;
}

// count (1 or 2) tensors of one shape in one launch (two for > 512 records: fold, then finish)
static int bn_tiles_finalize_sets(int n, int c, int count, BnTileSet *sets, float eps, float momentum, void *stream, int rb = 64) {
    const int nrb_all = (n + rb - 1) / rb;
    for (int i = 0; i < count; ++i) {
        BnTileSet &S = sets[i];
        S.rb = rb;
        if (!S.part || !S.mean || !S.rstd || ((S.sc != nullptr) && (!S.gamma || !S.beta || !S.sh))) return PTV2_ERR_ARG;
        // the folded records live behind the tile records (the GEMM wrote nrb * 2c floats; 16 * 2c doubles more are reserved)
        S.fold = (double *)(const_cast<float *>(S.part) + (((size_t)nrb_all * 2 * c + 1) & ~(size_t)1));
    }
    const BnTileSet A = sets[0], B = sets[count - 1];
    const unsigned cb = (unsigned)((c + gva::FIN_COLS - 1) / gva::FIN_COLS);
    if (nrb_all > 4096) {  // two levels: 16 folding blocks per 64 columns, then a one-thread-per-column finish
        const int ny = 16;
        hipLaunchKernelGGL(bn_fold_tiles_kernel, dim3(cb, ny, count), dim3(gva::FIN_COLS * gva::FIN_SLICES), 0, (hipStream_t)stream,
                           A, B, nrb_all, c, n);
        hipLaunchKernelGGL(bn_finalize_folded_kernel, dim3((c + 63) / 64, 1, count), dim3(64), 0, (hipStream_t)stream, A, B, ny, c, n,
                           eps, momentum);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    if (nrb_all >= 1024 && ((c + 15) / 16) * count <= 32) {
        unsigned *cnt = ptv2_stream_counters((hipStream_t)stream);
        if (!cnt) return PTV2_ERR_LAUNCH;
        hipLaunchKernelGGL(bn_finalize_tiles_split_kernel, dim3((c + 15) / 16, BNT_NS, count), dim3(1024), 0, (hipStream_t)stream, A, B,
                           nrb_all, c, n, eps, momentum, cnt + CNT_BN_TILES);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    if (nrb_all >= 64)  // many records: 16 columns x 64 record slices per workgroup
        hipLaunchKernelGGL(bn_finalize_tiles_kernel<16>, dim3((c + 15) / 16, 1, count), dim3(1024), 0, (hipStream_t)stream, A, B,
                           nrb_all, c, n, eps, momentum);
    else
        hipLaunchKernelGGL(bn_finalize_tiles_kernel<64>, dim3(cb, 1, count), dim3(1024), 0, (hipStream_t)stream, A, B, nrb_all, c, n,
                           eps, momentum);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int bn_tiles_finalize_hip_launcher(int n, int c, float *part, const float *gamma, const float *beta,
                                              float *mean, float *rstd, float *sc, float *sh, float *running_mean,
                                              float *running_var, long long *num_batches_tracked, float eps, float momentum,
                                              void *stream) {
    if (n < 1 || c < 4) return PTV2_ERR_ARG;
    BnTileSet S{part, mean, rstd, running_mean, running_var, num_batches_tracked, gamma, beta, sc, sh, nullptr, 64};
    return bn_tiles_finalize_sets(n, c, 1, &S, eps, momentum, stream);
}
// internal (block.hip): records of rb rows each (bn_tiles_floats_rb floats) -- the attention's tile kernel leaves 16-row records
int bn_tiles_finalize_rb(int n, int c, const BnTileSet &set, float eps, float momentum, void *stream) {
    const int rb = set.rb;
    if (n < 1 || c < 4 || (rb != 16 && rb != 64)) return PTV2_ERR_ARG;
    BnTileSet S = set;
    return bn_tiles_finalize_sets(n, c, 1, &S, eps, momentum, stream, rb);
}

// two tensors of one shape (internal to the block runtime: the q / k BatchNorms), records of sets[0].rb rows
int bn_tiles_finalize_pair(int n, int c, const BnTileSet (&sets)[2], float eps, float momentum, void *stream) {
    const int rb = sets[0].rb;
    if (n < 1 || c < 4 || (rb != 16 && rb != 64)) return PTV2_ERR_ARG;
    BnTileSet S[2] = {sets[0], sets[1]};
    return bn_tiles_finalize_sets(n, c, 2, S, eps, momentum, stream, rb);
}

// internal (block.hip): BatchNorm statistics from the producing GEMM's tile records AND the Block tail
// y = ReLU(residual + rowscale * BN(x)) in one launch when the records are few (deep levels); returns 0 when it declines
int bn_tiles_apply_residual(int n, int c, const BnTileSet &S, float eps, float momentum, const float *x, const float *residual,
                            const float *rowscale, float *y, void *stream) {
    const int rb = S.rb;
    const int nrb = (n + rb - 1) / rb;
    if (nrb > (rb == 16 ? 512 : 256) || c % 4 != 0 || bn_finapply_off() || (rb != 16 && rb != 64)) return 0;
    const dim3 grid((unsigned)((c + FA_COLS - 1) / FA_COLS), (unsigned)((n + FA_ROWS - 1) / FA_ROWS));
    {
        PtvScopedTimer t(KID_BN_APPLY, (hipStream_t)stream, 12.0 * n * c);
        hipLaunchKernelGGL(bn_tiles_apply_residual_kernel<0>, grid, dim3(TPB), 0, (hipStream_t)stream, S, nrb, n, c, eps, momentum, x,
                           residual, rowscale, y);
    }
    return 1;
}

// internal (model.hip): the same for y = ReLU(BN(x)) -- statistics from the producing GEMM's 64-row records and the apply pass in
// one launch (was bn_stats + bn_finalize + bn_apply); returns 0 when it declines (many records: the three launches stay)
int bn_tiles_apply_relu(int n, int c, const BnTileSet &set, float eps, float momentum, const float *x, float *y, void *stream) {
    const int nrb = (n + 63) / 64;
    if (nrb > 512 || c % 4 != 0 || bn_finapply_off()) return 0;
    BnTileSet S = set;  // (no folded affine asked for; 64-row records)
    S.sc = S.sh = nullptr; S.rb = 64;
    const dim3 grid((unsigned)((c + FA_COLS - 1) / FA_COLS), (unsigned)((n + FA_ROWS - 1) / FA_ROWS));
    {
        PtvScopedTimer t(KID_BN_APPLY, (hipStream_t)stream, 8.0 * n * c);
        hipLaunchKernelGGL(bn_tiles_apply_residual_kernel<1>, grid, dim3(TPB), 0, (hipStream_t)stream, S, nrb, n, c, eps, momentum, x,
                           (const float *)nullptr, (const float *)nullptr, y);
    }
    return 1;
}

extern "C" int bn_apply_hip_launcher(int n, int c, const float *x, const float *mean, const float *rstd,
                                     const float *gamma, const float *beta, int relu, float *y, void *stream) {
    if (n < 0 || c < 4 || c % 4 != 0) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    const long long total4 = (long long)n * (c >> 2);
    const int nblk = (int)std::min<long long>((total4 + TPB - 1) / TPB, 256 * 16);
    {
        PtvScopedTimer t(KID_BN_APPLY, (hipStream_t)stream, 8.0 * n * c);
        hipLaunchKernelGGL(bn_apply_kernel, dim3(nblk), dim3(TPB), 0, (hipStream_t)stream, total4, c >> 2, x, mean, rstd,
                           gamma, beta, relu, y);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// training-mode forward as one call (statistics + running buffers, then the apply pass; residual != NULL selects
// the Block tail y = ReLU(residual + rowscale * BN(x)))
extern "C" int bn_forward_hip_launcher(int n, int c, const float *x, const float *gamma, const float *beta, int relu,
                                       float *mean, float *rstd, float *running_mean, float *running_var,
                                       long long *num_batches_tracked, float eps, float momentum, const float *residual,
                                       const float *rowscale, float *y, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    const int rc = bn_stats_hip_launcher(n, c, x, mean, rstd, running_mean, running_var, num_batches_tracked, eps, momentum,
                                         workspace, workspace_bytes, stream);
    if (rc != PTV2_OK) return rc;
    if (residual) return bn_apply_residual_hip_launcher(n, c, x, mean, rstd, gamma, beta, residual, rowscale, y, stream);
    return bn_apply_hip_launcher(n, c, x, mean, rstd, gamma, beta, relu, y, stream);
}

extern "C" int bn_apply_residual_hip_launcher(int n, int c, const float *x, const float *mean, const float *rstd,
                                              const float *gamma, const float *beta, const float *residual,
                                              const float *rowscale, float *y, void *stream) {
    if (n < 0 || c < 4 || c % 4 != 0 || !residual) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    const long long total4 = (long long)n * (c >> 2);
    const int nblk = (int)std::min<long long>((total4 + TPB - 1) / TPB, 256 * 16);
    {
        PtvScopedTimer t(KID_BN_APPLY, (hipStream_t)stream, 12.0 * n * c);
        hipLaunchKernelGGL(bn_apply_residual_kernel, dim3(nblk), dim3(TPB), 0, (hipStream_t)stream, total4, c >> 2, x, mean,
                           rstd, gamma, beta, residual, rowscale, y);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int bn_backward_residual_hip_launcher(int n, int c, const float *x, const float *gy, const float *y,
                                                 const float *rowscale, const float *mean, const float *rstd,
                                                 const float *gamma, int training, float *gx, float *g_residual,
                                                 float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                                 void *stream) {
    if (n < 1 || c < 4 || c % 4 != 0 || c > 1024) return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < dense_workspace_bytes(n, c, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = bn_grid(n, c);
    float *part = (float *)workspace;
    {
        PtvScopedTimer t(KID_BN_BWD_REDUCE, st, 12.0 * n * c);
        hipLaunchKernelGGL(bn_bwd_reduce_residual_kernel, dim3(nblk), dim3(TPB), sizeof(float4) * 2 * TPB, st, n, c, x, gy, y,
                           rowscale, mean, rstd, part);
    }
    if (finapply_ok(n, nblk)) {
        PtvScopedTimer t(KID_BN_BWD_FINAPPLY, st, 20.0 * n * c);
        const BnFinApply A{part, nblk, 2 * c, 0, x, gy, mean, rstd, gamma, nullptr, gx, dbeta, dgamma, y, rowscale, g_residual};
        launch_finapply(st, n, c, 1, training, true, 1, A, A);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    launch_finalize(st, (const float *)part, nblk, 2 * c, gva::MapSplit2<float>{dbeta, dgamma, c});
    const long long total4 = (long long)n * (c >> 2);
    const int nb2 = (int)std::min<long long>((total4 + TPB - 1) / TPB, 256 * 16);
    {
        PtvScopedTimer t(KID_BN_BWD_APPLY_RES, st, 20.0 * n * c);
        hipLaunchKernelGGL(bn_bwd_apply_residual_kernel, dim3(nb2), dim3(TPB), 0, st, total4, c >> 2, 1.0f / (float)n, x, gy, y,
                           rowscale, mean, rstd, gamma, (const float *)dbeta, (const float *)dgamma, training, gx, g_residual);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int bn_backward_hip_launcher(int n, int c, const float *x, const float *gy, const float *mean,
                                        const float *rstd, const float *gamma, const float *beta, int relu,
                                        int training, float *gx, float *dgamma, float *dbeta, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    if (n < 1 || c < 4 || c % 4 != 0 || c > 1024) return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < dense_workspace_bytes(n, c, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = bn_grid(n, c);
    float *part = (float *)workspace;
    {
        PtvScopedTimer t(KID_BN_BWD_REDUCE, st, 8.0 * n * c);
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nblk), dim3(TPB), sizeof(float4) * 2 * TPB, st, n, c, x, gy, mean,
                           rstd, gamma, beta, relu, part, BnSecond{});
    }
    if (finapply_ok(n, nblk)) {
        PtvScopedTimer t(KID_BN_BWD_FINAPPLY, st, 12.0 * n * c);
        const BnFinApply A{part, nblk, 2 * c, 0, x, gy, mean, rstd, gamma, beta, gx, dbeta, dgamma, nullptr, nullptr, nullptr};
        launch_finapply(st, n, c, relu, training, false, 1, A, A);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    launch_finalize(st, (const float *)part, nblk, 2 * c, gva::MapSplit2<float>{dbeta, dgamma, c});
    const long long total4 = (long long)n * (c >> 2);
    const int nb2 = (int)std::min<long long>((total4 + TPB - 1) / TPB, 256 * 16);
    {
        PtvScopedTimer t(KID_BN_BWD_APPLY, st, 12.0 * n * c);
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nb2), dim3(TPB), 0, st, total4, c >> 2, 1.0f / (float)n, x, gy, mean,
                           rstd, gamma, beta, relu, (const float *)dbeta, (const float *)dgamma, training, gx, BnSecond{});
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// bn_backward whose reduce pass already ran in the epilogue of the GEMM that produced gy (rows_gemm_bnbwd_hip_launcher left
// nrec records of [2][c] in `records`): finalize + apply only
extern "C" int bn_backward_records_hip_launcher(int n, int c, const float *x, const float *gy, const float *mean,
                                                const float *rstd, const float *gamma, const float *beta, int relu,
                                                int training, float *gx, float *dgamma, float *dbeta, const float *records,
                                                int nrec, void *stream) {
    if (n < 1 || c < 4 || c % 4 != 0 || c > 1024 || !records || nrec < 1) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (finapply_ok(n, nrec)) {
        PtvScopedTimer t(KID_BN_BWD_FINAPPLY, st, 12.0 * n * c);
        const BnFinApply A{records, nrec, 2 * c, 0, x, gy, mean, rstd, gamma, beta, gx, dbeta, dgamma, nullptr, nullptr, nullptr};
        launch_finapply(st, n, c, relu, training, false, 1, A, A);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    launch_finalize(st, records, nrec, 2 * c, gva::MapSplit2<float>{dbeta, dgamma, c});
    const long long total4 = (long long)n * (c >> 2);
    const int nb2 = (int)std::min<long long>((total4 + TPB - 1) / TPB, 256 * 16);
    {
        PtvScopedTimer t(KID_BN_BWD_APPLY, st, 12.0 * n * c);
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nb2), dim3(TPB), 0, st, total4, c >> 2, 1.0f / (float)n, x, gy, mean,
                           rstd, gamma, beta, relu, (const float *)dbeta, (const float *)dgamma, training, gx, BnSecond{});
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

struct MapBnPair {  // record [dbeta0 c | dgamma0 c | dbeta1 c | dgamma1 c]
    float *db0, *dg0, *db1, *dg1;
    int c;
    __device__ void operator()(int j, double v) const {
        const int s = j / c, k = j - s * c;
        (s == 0 ? db0 : s == 1 ? dg0 : s == 2 ? db1 : dg1)[k] = (float)v;
    }
};

// two BatchNorm backwards of one shape (x[i], gy[i], ... i = 0, 1) in the three launches of one
// (workspace: dense_workspace_bytes(n, 2 * c, c))
extern "C" int bn_backward_pair_hip_launcher(int n, int c, const float *const *x, const float *const *gy,
                                             const float *const *mean, const float *const *rstd, const float *const *gamma,
                                             const float *const *beta, int relu, int training, float *const *gx,
                                             float *const *dgamma, float *const *dbeta, void *workspace, size_t workspace_bytes,
                                             void *stream) {
    if (n < 1 || c < 4 || c % 4 != 0 || c > 1024 || !x || !gy || !mean || !rstd || !gamma || !beta || !gx || !dgamma || !dbeta)
        return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < dense_workspace_bytes(n, 2 * c, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int nblk = bn_grid(n, c);
    float *part = (float *)workspace;
    const int left = ptv2_skinny_bn_take_records(n, c, part, gy);  // records of the launch that formed gy (skinny.hip), if any
    const bool reduced = left > 0;
    if (reduced) nblk = left;
    const BnSecond sec{x[1], gy[1], mean[1], rstd[1], gamma[1], beta[1], gx[1], dgamma[1], dbeta[1]};
    if (!reduced) {  // (else: the records are there already, left by the launch that formed gy -- skinny_backward_pair_bn_reduce)
        PtvScopedTimer t(KID_BN_BWD_REDUCE, st, 16.0 * n * c);
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nblk, 2), dim3(TPB), sizeof(float4) * 2 * TPB, st, n, c, x[0], gy[0], mean[0],
                           rstd[0], gamma[0], beta[0], relu, part, sec);
    }
    if (finapply_ok(n, nblk)) {  // record of a block: [set 0: dbeta c | dgamma c][set 1: ...]
        PtvScopedTimer t(KID_BN_BWD_FINAPPLY, st, 24.0 * n * c);
        const BnFinApply A0{part, nblk, 4 * c, 0, x[0], gy[0], mean[0], rstd[0], gamma[0], beta[0], gx[0], dbeta[0], dgamma[0], nullptr,
                            nullptr, nullptr};
        const BnFinApply A1{part, nblk, 4 * c, 2 * c, x[1], gy[1], mean[1], rstd[1], gamma[1], beta[1], gx[1], dbeta[1], dgamma[1],
                            nullptr, nullptr, nullptr};
        launch_finapply(st, n, c, relu, training, false, 2, A0, A1);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    launch_finalize(st, (const float *)part, nblk, 4 * c, MapBnPair{dbeta[0], dgamma[0], dbeta[1], dgamma[1], c});
    const long long total4 = (long long)n * (c >> 2);
    const int nb2 = (int)std::min<long long>((total4 + TPB - 1) / TPB, 256 * 16);
    {
        PtvScopedTimer t(KID_BN_BWD_APPLY, st, 24.0 * n * c);
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nb2, 2), dim3(TPB), 0, st, total4, c >> 2, 1.0f / (float)n, x[0], gy[0],
                           mean[0], rstd[0], gamma[0], beta[0], relu, (const float *)dbeta[0], (const float *)dgamma[0], training,
                           gx[0], sec);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
