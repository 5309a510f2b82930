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
// Where each thing is stated (once):
//   bn_math.h        the per-element formulas, a float4 at a time: xhat, the forward affine and its ReLU / residual tails, the
//                    two backward masks, the reduce step, the input gradient
//   dense_common.h   BnTileSet (a forward fed from tile records), BnBwdSet (the operands of one backward), the tail of a
//                    column-sum pass (column_sums_store), apply_grid
//   here             bn_moments (mean / variance / rstd from the sums), bn_merge (one tile record into the running pair;
//                    the loops around it keep their load batches and chains: the order of additions decides the bits),
//                    bn_tiles_emit; the residual and plain routes are one kernel each, templated on RESIDUAL; the host
//                    side has one reduce launch (bn_bwd_reduce) and one "records -> gx" tail (bn_bwd_finish) for the four
//                    backward launchers, one bn_apply_launch and one bn_tiles_apply for the forward entry points.
// The unit is compiled with the default contraction, and which products fuse depends on the shape of the code around them
// (bn_bwd_apply_kernel loads dbeta / dgamma INSIDE its `if (training)`: with the loads selected against zero in front of the
// branch the residual route's gx came out with other bits).  A change here is checked by comparing outputs bit for bit
// against the build before it, not by reading the source.
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
    column_sums_store(lds4, s1, s2, cq, rl, c, part + (size_t)blockIdx.x * 2 * c);
}

// mean, biased variance (clamped at 0) and rstd of n samples from their sum t1 and their sum of squares t2
struct BnMoments { double mean, var; float rstd; };
__device__ __forceinline__ BnMoments bn_moments(double t1, double t2, int n, float eps) {
    BnMoments M;
    M.mean = t1 / n;
    const double var = t2 / n - M.mean * M.mean;
    M.var = var > 0.0 ? var : 0.0;
    M.rstd = (float)(1.0 / sqrt(M.var + (double)eps));
    return M;
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
        const BnMoments M = bn_moments(t1, t2, n, eps);  // of the shifted samples
        const double m = (double)x0[ch] + M.mean, var = M.var;
        mean[ch] = (float)m;
        rstd[ch] = M.rstd;
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

// one record (column sum s, centred sum of squares m2, cnt rows) into the running pair: a += S_b, b += M2_b + S_b^2 / n_b
__device__ __forceinline__ void bn_merge(double &a, double &b, float s, float m2, int cnt) {
    const double sb = (double)s;
    a += sb;
    b += (double)m2 + sb * sb / (double)cnt;
}
// the same for record k of S, column ch of c, loaded here
__device__ __forceinline__ void bn_merge_record(const BnTileSet &S, int k, int n, int c, int ch, double &a, double &b) {
    bn_merge(a, b, S.part[(size_t)k * 2 * c + ch], S.part[(size_t)k * 2 * c + c + ch], bn_tile_rows(S, k, n));
}

__device__ __forceinline__ void bn_tiles_emit(const BnTileSet &S, int ch, double t1, double t2, int n, float eps, float momentum) {
    const BnMoments M = bn_moments(t1, t2, n, eps);
    const double m = M.mean, var = M.var;
    S.mean[ch] = (float)m;
    S.rstd[ch] = M.rstd;
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
                const int cnt = bn_tile_rows(S, k + u * SLICES, n);
                if (u & 1) bn_merge(a2, b2, s[u], m[u], cnt);
                else bn_merge(a, b, s[u], m[u], cnt);
            }
        }
        for (; k + SLICES < nrb; k += 2 * SLICES) {  // two independent chains: the loads of both records are in flight
            bn_merge_record(S, k, n, c, ch, a, b);
            bn_merge_record(S, k + SLICES, n, c, ch, a2, b2);
        }
        for (; k < nrb; k += SLICES) bn_merge_record(S, k, n, c, ch, a, b);
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
    const int col = threadIdx.x & (COLS - 1), sl = threadIdx.x / COLS;
    const int ch = blockIdx.x * COLS + col;
    double a = 0.0, b = 0.0;
    if (ch < c) {
        for (int k = blockIdx.y * SLICES + sl; k < nrb; k += BNT_NS * SLICES) bn_merge_record(S, k, n, c, ch, a, b);
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
// y = BN(x), with the fused ReLU if `relu`.  RESIDUAL: the Block tail fused into the last BatchNorm of a Block
// (point_transformer_v2m2_base.py:174-176):
//   y = ReLU(residual + rowscale[n] * BN(x))      rowscale = per-point DropPath factor (0 or 1/keep), may be NULL
template <bool RESIDUAL>
__global__ __launch_bounds__(TPB) void bn_apply_kernel(long long total4, int cq, const float *__restrict__ x,
                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       int relu, const float *__restrict__ residual,
                                                       const float *__restrict__ rowscale, float *__restrict__ y) {
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total4; e += (long long)gridDim.x * TPB) {
        const int q = (int)(e % cq);
        const float4 h = bn_xhat(((const float4 *)x)[e], ((const float4 *)mean)[q], ((const float4 *)rstd)[q]);
        const float4 o = bn_affine(h, ((const float4 *)gamma)[q], ((const float4 *)beta)[q]);
        if (RESIDUAL) ((float4 *)y)[e] = bn_residual_relu(o, rowscale ? rowscale[e / cq] : 1.f, ((const float4 *)residual)[e]);
        else ((float4 *)y)[e] = relu ? bn_relu(o) : o;
    }
}

// -------------------------------------------------------- BN: backward reduce --
// partial columns [0,c): sum gy' ; [c,2c): sum gy' * xhat, with gy' = gy masked by the fused ReLU.  RESIDUAL, the backward of
// the fused tail: gy' = gy * (y > 0) * rowscale[n] (gamma and beta are not read).  blockIdx.y == 1 works on A1, a second,
// independent BatchNorm of the same shape in the same launch (linear_q and linear_k of a Block: their backward chains are
// independent, batching them saves three launches per Block); record of a block: [set 0 | set 1]
template <bool RESIDUAL>
__global__ __launch_bounds__(TPB) void bn_bwd_reduce_kernel(int n, int c, int relu, float *__restrict__ part, BnBwdSet A0,
                                                            BnBwdSet A1) {
    extern __shared__ float4 lds4[];
    const BnBwdSet &A = blockIdx.y ? A1 : A0;
    const int cq = c >> 2;
    const int rl = TPB / cq;
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    if (r < rl) {
        const float4 m = ((const float4 *)A.mean)[q], rs = ((const float4 *)A.rstd)[q];
        float4 g = s1, b = s1;
        if (!RESIDUAL) { g = ((const float4 *)A.gamma)[q]; b = ((const float4 *)A.beta)[q]; }
#pragma unroll 4
        for (long long row = (long long)blockIdx.x * rl + r; row < n; row += (long long)gridDim.x * rl) {
            const float4 h = bn_xhat(((const float4 *)A.x)[row * cq + q], m, rs);
            float4 d = ((const float4 *)A.gy)[row * cq + q];
            if (RESIDUAL) d = bn_residual_mask(bn_scale(d, A.rowscale ? A.rowscale[row] : 1.f), ((const float4 *)A.y)[row * cq + q]);
            else if (relu) d = bn_relu_mask(d, h, g, b);
            bn_accumulate(s1, s2, d, h);
        }
    }
    column_sums_store(lds4, s1, s2, cq, rl, c, part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 * c);
}

// --------------------------------------------------------- BN: backward apply --
// the gradient that enters the BatchNorm at float4 e of row `row`: gy masked by the fused ReLU; RESIDUAL: masked by y > 0 (that
// is the residual's gradient, written here), then scaled by rowscale
template <bool RESIDUAL>
__device__ __forceinline__ float4 bn_bwd_masked(const BnBwdSet &A, long long e, long long row, const float4 h, const float4 g,
                                                const float4 b, int relu) {
    float4 d = ((const float4 *)A.gy)[e];
    if (RESIDUAL) {
        d = bn_residual_mask(d, ((const float4 *)A.y)[e]);
        ((float4 *)A.g_residual)[e] = d;
        d = bn_scale(d, A.rowscale ? A.rowscale[row] : 1.f);
    } else if (relu) {
        d = bn_relu_mask(d, h, g, b);
    }
    return d;
}

// the pass over all elements, dbeta / dgamma finalized by the launch before; blockIdx.y selects the set as in the reduce
template <bool RESIDUAL>
__global__ __launch_bounds__(TPB) void bn_bwd_apply_kernel(long long total4, int cq, float inv_n, int relu, int training,
                                                           BnBwdSet A0, BnBwdSet A1) {
    const BnBwdSet &A = blockIdx.y ? A1 : A0;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total4; e += (long long)gridDim.x * TPB) {
        const int q = (int)(e % cq);
        const float4 m = ((const float4 *)A.mean)[q], rs = ((const float4 *)A.rstd)[q], g = ((const float4 *)A.gamma)[q];
        const float4 b = RESIDUAL ? zero : ((const float4 *)A.beta)[q];
        const float4 h = bn_xhat(((const float4 *)A.x)[e], m, rs);
        const float4 d = bn_bwd_masked<RESIDUAL>(A, e, e / cq, h, g, b, relu);
        if (training) {
            const float4 db = ((const float4 *)A.dbeta)[q], dg = ((const float4 *)A.dgamma)[q];
            ((float4 *)A.gx)[e] = bn_gx(g, rs, d, db, dg, h, inv_n, 1);
        } else {
            ((float4 *)A.gx)[e] = bn_gx(g, rs, d, zero, zero, h, inv_n, 0);
        }
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
                for (int u = 0; u < 4; ++u) bn_merge(a, b, sv[u], mv[u], bn_tile_rows(S, k + u * SL, n));
            }
            for (; k < nrb; k += SL) bn_merge_record(S, k, n, c, col0 + cj, a, b);
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
        const BnMoments M = bn_moments(t1, t2, n, eps);
        s_mean[cj] = (float)M.mean;
        s_rstd[cj] = M.rstd;
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
        const float4 o = bn_affine(bn_xhat(((const float4 *)x)[e], m, r), g, b);
        if (PLAIN) ((float4 *)y)[e] = bn_relu(o);
        else ((float4 *)y)[e] = bn_residual_relu(o, rowscale ? rowscale[row] : 1.f, ((const float4 *)residual)[e]);
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
    BnBwdSet bn;
};

template <bool RESIDUAL>
__global__ __launch_bounds__(TPB) void bn_bwd_finapply_kernel(int n, int c, int relu, int training, float inv_n, BnFinApply A0,
                                                              BnFinApply A1) {
    const BnFinApply &A = blockIdx.z ? A1 : A0;
    const BnBwdSet &O = A.bn;
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
        if (blockIdx.y == 0 && cj < ncol) (which ? O.dgamma : O.dbeta)[col0 + cj] = v;
    }
    __syncthreads();
    constexpr int QW = FA_COLS / 4, RL = TPB / QW;  // column quads of the stripe x row lanes
    const int cq = c >> 2, q = threadIdx.x % QW, rl = threadIdx.x / QW;
    const int qcol = (col0 >> 2) + q;
    if (4 * q >= ncol) return;
    const float4 m = ((const float4 *)O.mean)[qcol], rs = ((const float4 *)O.rstd)[qcol], g = ((const float4 *)O.gamma)[qcol];
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!RESIDUAL && relu) b = ((const float4 *)O.beta)[qcol];
    const float4 db = *(const float4 *)(s_db + 4 * q), dg = *(const float4 *)(s_dg + 4 * q);
    const long long r0 = (long long)blockIdx.y * FA_ROWS;
    const long long r1 = (r0 + FA_ROWS) < (long long)n ? (r0 + FA_ROWS) : (long long)n;
    for (long long row = r0 + rl; row < r1; row += RL) {
        const long long e = row * cq + qcol;
        const float4 h = bn_xhat(((const float4 *)O.x)[e], m, rs);
        const float4 d = bn_bwd_masked<RESIDUAL>(O, e, row, h, g, b, relu);
        ((float4 *)O.gx)[e] = bn_gx(g, rs, d, db, dg, h, inv_n, training);
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
    double *__restrict__ out = S.fold;
    const int col = threadIdx.x & (gva::FIN_COLS - 1), sl = threadIdx.x / gva::FIN_COLS;
    const int ch = blockIdx.x * gva::FIN_COLS + col;
    double a = 0.0, b = 0.0;
    if (ch < c) {
        for (int k = blockIdx.y * gva::FIN_SLICES + sl; k < nrb; k += gridDim.y * gva::FIN_SLICES)
            bn_merge_record(S, k, n, c, ch, a, b);
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

// statistics from the producing launch's tile records and the apply pass in one launch when the records are few (at most
// max_records); returns 0 when it declines
static int bn_tiles_apply(int n, int c, const BnTileSet &S, int max_records, bool plain, float eps, float momentum, const float *x,
                          const float *residual, const float *rowscale, float *y, hipStream_t st) {
    const int nrb = (n + S.rb - 1) / S.rb;
    if (nrb > max_records || c % 4 != 0 || bn_finapply_off()) return 0;
    const dim3 grid((unsigned)((c + FA_COLS - 1) / FA_COLS), (unsigned)((n + FA_ROWS - 1) / FA_ROWS));
    PtvScopedTimer t(KID_BN_APPLY, st, (plain ? 8.0 : 12.0) * n * c);
    if (plain)
        hipLaunchKernelGGL(bn_tiles_apply_residual_kernel<1>, grid, dim3(TPB), 0, st, S, nrb, n, c, eps, momentum, x, residual, rowscale, y);
    else
        hipLaunchKernelGGL(bn_tiles_apply_residual_kernel<0>, grid, dim3(TPB), 0, st, S, nrb, n, c, eps, momentum, x, residual, rowscale, y);
    return 1;
}

// internal (block.hip): the Block tail y = ReLU(residual + rowscale * BN(x)) at the deep levels, records of 16 or 64 rows
int bn_tiles_apply_residual(int n, int c, const BnTileSet &S, float eps, float momentum, const float *x, const float *residual,
                            const float *rowscale, float *y, void *stream) {
    if (S.rb != 16 && S.rb != 64) return 0;
    return bn_tiles_apply(n, c, S, S.rb == 16 ? 512 : 256, false, eps, momentum, x, residual, rowscale, y, (hipStream_t)stream);
}

// internal (model.hip): the same for y = ReLU(BN(x)) from the producing GEMM's 64-row records (was bn_stats + bn_finalize +
// bn_apply, which stay for many records)
int bn_tiles_apply_relu(int n, int c, const BnTileSet &set, float eps, float momentum, const float *x, float *y, void *stream) {
    BnTileSet S = set;  // (no folded affine asked for; 64-row records)
    S.sc = S.sh = nullptr; S.rb = 64;
    return bn_tiles_apply(n, c, S, 512, true, eps, momentum, x, nullptr, nullptr, y, (hipStream_t)stream);
}

// the apply pass; residual != NULL: the Block tail y = ReLU(residual + rowscale * BN(x))
static int bn_apply_launch(int n, int c, const float *x, const float *mean, const float *rstd, const float *gamma,
                           const float *beta, int relu, const float *residual, const float *rowscale, float *y, void *stream) {
    if (n < 0 || c < 4 || c % 4 != 0) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long total4 = (long long)n * (c >> 2);
    const dim3 grid(apply_grid(total4));
    {
        PtvScopedTimer t(KID_BN_APPLY, st, (residual ? 12.0 : 8.0) * n * c);
        if (residual)
            hipLaunchKernelGGL(bn_apply_kernel<true>, grid, dim3(TPB), 0, st, total4, c >> 2, x, mean, rstd, gamma, beta, relu, residual, rowscale, y);
        else
            hipLaunchKernelGGL(bn_apply_kernel<false>, grid, dim3(TPB), 0, st, total4, c >> 2, x, mean, rstd, gamma, beta, relu, residual, rowscale, y);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int bn_apply_hip_launcher(int n, int c, const float *x, const float *mean, const float *rstd,
                                     const float *gamma, const float *beta, int relu, float *y, void *stream) {
    return bn_apply_launch(n, c, x, mean, rstd, gamma, beta, relu, nullptr, nullptr, y, stream);
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
    if (!residual) return PTV2_ERR_ARG;
    return bn_apply_launch(n, c, x, mean, rstd, gamma, beta, 1, residual, rowscale, y, stream);
}

struct MapBnPair {  // record [dbeta0 c | dgamma0 c | dbeta1 c | dgamma1 c]
    float *db0, *dg0, *db1, *dg1;
    int c;
    __device__ void operator()(int j, double v) const {
        const int s = j / c, k = j - s * c;
        (s == 0 ? db0 : s == 1 ? dg0 : s == 2 ? db1 : dg1)[k] = (float)v;
    }
};

// A BatchNorm backward is the reduce pass below (or the records another launch left) and bn_bwd_finish.  `sets` (1 or 2)
// BatchNorms of one shape share the launches: A[0 .. sets), record of a block [set 0: dbeta c | dgamma c][set 1: ...].  The
// residual route (one set) masks by y > 0 and also writes g_residual.  Algorithmic bytes per n * c: 8 / 12 (residual) / 16
// (pair) for the reduce, 12 / 20 / 24 for what follows.
static void bn_bwd_reduce(hipStream_t st, int n, int c, int relu, bool residual, int sets, const BnBwdSet *A, float *part, int nblk) {
    PtvScopedTimer t(KID_BN_BWD_REDUCE, st, (residual ? 12.0 : 8.0 * sets) * n * c);
    const dim3 grid(nblk, sets);
    const size_t lds = sizeof(float4) * 2 * TPB;
    if (residual) hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, grid, dim3(TPB), lds, st, n, c, relu, part, A[0], A[sets - 1]);
    else hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, grid, dim3(TPB), lds, st, n, c, relu, part, A[0], A[sets - 1]);
}

// the nrec records are in `part`: the record sums inside the apply launch when they are few (finapply_ok), else finalize + apply
static int bn_bwd_finish(hipStream_t st, int n, int c, int relu, int training, bool residual, int sets, const BnBwdSet *A,
                         const float *part, int nrec) {
    const int stride = sets * 2 * c;  // floats of a record
    const double bytes = (residual ? 20.0 : 12.0 * sets) * n * c;
    const float inv_n = 1.0f / (float)n;
    if (finapply_ok(n, nrec)) {
        PtvScopedTimer t(KID_BN_BWD_FINAPPLY, st, bytes);
        BnFinApply F[2];
        for (int i = 0; i < 2; ++i) {
            const int set = i < sets ? i : sets - 1;
            F[i].part = part; F[i].nrec = nrec; F[i].rec_floats = stride; F[i].off = set * 2 * c; F[i].bn = A[set];
        }
        const dim3 grid((unsigned)((c + FA_COLS - 1) / FA_COLS), (unsigned)((n + FA_ROWS - 1) / FA_ROWS), (unsigned)sets);
        if (residual) hipLaunchKernelGGL(bn_bwd_finapply_kernel<true>, grid, dim3(TPB), 0, st, n, c, relu, training, inv_n, F[0], F[1]);
        else hipLaunchKernelGGL(bn_bwd_finapply_kernel<false>, grid, dim3(TPB), 0, st, n, c, relu, training, inv_n, F[0], F[1]);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    if (sets == 2) launch_finalize(st, part, nrec, stride, MapBnPair{A[0].dbeta, A[0].dgamma, A[1].dbeta, A[1].dgamma, c});
    else launch_finalize(st, part, nrec, stride, gva::MapSplit2<float>{A[0].dbeta, A[0].dgamma, c});
    const long long total4 = (long long)n * (c >> 2);
    {
        PtvScopedTimer t(residual ? KID_BN_BWD_APPLY_RES : KID_BN_BWD_APPLY, st, bytes);
        const dim3 grid(apply_grid(total4), sets);
        if (residual) hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid, dim3(TPB), 0, st, total4, c >> 2, inv_n, relu, training, A[0], A[sets - 1]);
        else hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid, dim3(TPB), 0, st, total4, c >> 2, inv_n, relu, training, A[0], A[sets - 1]);
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
    BnBwdSet A{};  // (beta stays NULL: the mask comes from y)
    A.x = x; A.gy = gy; A.mean = mean; A.rstd = rstd; A.gamma = gamma; A.gx = gx; A.dbeta = dbeta; A.dgamma = dgamma;
    A.y = y; A.rowscale = rowscale; A.g_residual = g_residual;
    bn_bwd_reduce(st, n, c, 1, true, 1, &A, part, nblk);
    return bn_bwd_finish(st, n, c, 1, training, true, 1, &A, part, nblk);
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
    BnBwdSet A{};
    A.x = x; A.gy = gy; A.mean = mean; A.rstd = rstd; A.gamma = gamma; A.beta = beta; A.gx = gx; A.dbeta = dbeta; A.dgamma = dgamma;
    bn_bwd_reduce(st, n, c, relu, false, 1, &A, part, nblk);
    return bn_bwd_finish(st, n, c, relu, training, false, 1, &A, part, nblk);
}

// bn_backward whose reduce pass already ran in the epilogue of the GEMM that produced gy (rows_gemm_bnbwd_hip_launcher left
// nrec records of [2][c] in `records`): finalize + apply only
extern "C" int bn_backward_records_hip_launcher(int n, int c, const float *x, const float *gy, const float *mean,
                                                const float *rstd, const float *gamma, const float *beta, int relu,
                                                int training, float *gx, float *dgamma, float *dbeta, const float *records,
                                                int nrec, void *stream) {
    if (n < 1 || c < 4 || c % 4 != 0 || c > 1024 || !records || nrec < 1) return PTV2_ERR_ARG;
    BnBwdSet A{};
    A.x = x; A.gy = gy; A.mean = mean; A.rstd = rstd; A.gamma = gamma; A.beta = beta; A.gx = gx; A.dbeta = dbeta; A.dgamma = dgamma;
    return bn_bwd_finish((hipStream_t)stream, n, c, relu, training, false, 1, &A, records, nrec);
}

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
    BnBwdSet A[2] = {};
    for (int i = 0; i < 2; ++i) {
        A[i].x = x[i]; A[i].gy = gy[i]; A[i].mean = mean[i]; A[i].rstd = rstd[i]; A[i].gamma = gamma[i]; A[i].beta = beta[i];
        A[i].gx = gx[i]; A[i].dbeta = dbeta[i]; A[i].dgamma = dgamma[i];
    }
    // (reduced: the records are there already, left by the launch that formed gy -- skinny_backward_pair_bn_reduce)
    if (!reduced) bn_bwd_reduce(st, n, c, relu, false, 2, A, part, nblk);
    return bn_bwd_finish(st, n, c, relu, training, false, 2, A, part, nblk);
}
