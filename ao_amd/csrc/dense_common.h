// ao_amd/csrc/dense_common.h -- what the three units of the per-point (N,C) layers share: bn.hip (BatchNorm1d), wgrad.hip
// (the weight gradient of nn.Linear) and skinny.hip (the narrow Linear(c, G) in front of the attention logits).  The BatchNorm
// arithmetic itself is bn_math.h.
#pragma once
#include <algorithm>

#include "bn_math.h"
#include "gva_common.h"

namespace dense {

using gva::finalize_kernel;
using gva::launch_finalize;
constexpr int TPB = 256;
constexpr int MAX_BLK = 512;

// workgroups (= records) of a BatchNorm column-sum pass over (n, c)
static inline int bn_grid(int n, int c) {
    const int rl = std::max(1, TPB / (c >> 2));
    long long b = ((long long)n + rl * 4 - 1) / (rl * 4);  // (8 rows per lane: the same; 16: +0.1 ms per step)
    // deep levels: at most 128 records, which the apply kernel's workgroups then sum themselves (bn_bwd_finapply_kernel)
    return (int)std::max<long long>(1, std::min<long long>(b, n <= 16384 ? 128 : MAX_BLK));
}

// workgroups of a grid-stride pass over total4 float4 elements (the apply kernels)
static inline int apply_grid(long long total4) { return (int)std::min<long long>((total4 + TPB - 1) / TPB, 256 * 16); }

// The tail of a column-sum pass: every thread holds two float4 partial sums of its (row lane, column quad); they go to LDS
// (2 * TPB float4), the first cq threads add the rl row lanes in lane order and store the record rec = [sum (c) | sum2 (c)].
__device__ __forceinline__ void column_sums_store(float4 *lds4, const float4 s1, const float4 s2, int cq, int rl, int c, float *rec) {
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
        ((float4 *)rec)[threadIdx.x] = a;
        ((float4 *)(rec + c))[threadIdx.x] = b;
    }
}

// The operands of one BatchNorm backward.  y / rowscale / g_residual: the Block tail (bn_backward_residual), where the ReLU
// mask comes from y > 0, d * rowscale enters the BatchNorm and d itself is the residual's gradient; beta is not read there.
struct BnBwdSet {
    const float *x, *gy, *mean, *rstd, *gamma, *beta;
    float *gx, *dbeta, *dgamma;
    const float *y, *rowscale;
    float *g_residual;
};

// One BatchNorm fed from the statistics records its producing launch left in part[nrb][2][c] (per block of rb rows: column sums
// and sums of squares about the block mean): what the finalize writes (mean / rstd; the running buffers, NULL: not tracked; the
// folded affine sc / sh, NULL: not asked for) and gamma / beta.  A kernel argument of bn.hip: the layout is fixed.
struct BnTileSet {
    const float *part;
    float *mean, *rstd, *run_mean, *run_var;
    long long *batches;
    const float *gamma, *beta;
    float *sc, *sh;
    double *fold;  // two-level scratch (bn_fold_tiles_kernel)
    int rb;        // rows per record: 64 (the row GEMM's epilogue, the projection kernels) or 16 (gva_fwd_tile.hip); 0 = 64
};

}  // namespace dense
