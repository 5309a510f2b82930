// ao_amd/csrc/dense_common.h -- what the three units of the per-point (N,C) layers share: bn.hip (BatchNorm1d), wgrad.hip
// (the weight gradient of nn.Linear) and skinny.hip (the narrow Linear(c, G) in front of the attention logits).
#pragma once
#include <algorithm>

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
