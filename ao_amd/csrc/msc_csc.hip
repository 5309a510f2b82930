// ao_amd/csrc/msc_csc.hip -- the partitioned InfoNCE loss of Masked Scene Contrast v1m2 (CSC) for gfx950 (MI355X); C ABI
// include/ptv2_csc_hip.h, DESIGN.md section 16.
//
// Replaces compute_contrastive_loss / compute_partitions of masked_scene_contrast_v1m2_csc.py: per scene an (M, M) similarity
// matrix, an (M, M, 3) array of relative translations, a distance and a partition matrix and one masked cross-entropy per
// partition id.  Here the pairs arrive grouped by scene; a workgroup owns 64 rows of one scene and walks the 64 x 64 tiles of
// that scene's block of S = A B^T (msc_tile.h: v_mfma_f32_32x32x2_f32, never stored).  The class of an element is a function
// of the two gathered coordinates, so the tile's epilogue feeds one of five per-row sums: all partitioned log-sum-exps come
// out of one pass.  Rows are unit vectors, |S| <= 1, so every sum is shifted by the constant 1 / t (the launcher refuses a t
// where exp(-2 / t) would leave the normal fp32 range) and an element costs one exp.  Column splits are combined in split
// order, the scene recurrences of the three scalars run in one finishing workgroup.  Backward: each tile is recomputed; an
// off-diagonal element belongs to one class and needs one exp against that class's lse of its row.
//
// Compiled with -ffp-contract=off (Makefile): the relative translation, its squared length and the square root round once per
// statement, as the eager statements do.
#include "msc_tile.h"
#include "../../include/ptv2_csc_hip.h"

namespace {

constexpr int NCLS = CSC_CLASSES;
constexpr int LP = TILE + 1;  // LDS pitch of the staged lse rows: the five classes of one row fall into five banks

// class of the element whose column's view-1 coordinate is x and whose row's view-2 coordinate is y
// (compute_partitions: coord1.unsqueeze(0) - coord2.unsqueeze(1)); 4 is "none"
__device__ __forceinline__ int csc_class(float xx, float xy, float xz, float yx, float yy, float yz, float r1, float r2) {
    const float dx = xx - yx, dy = xy - yy, dz = xz - yz;
    const float d = sqrtf(((dx * dx + dy * dy) + dz * dz) + 1e-7f);
    const bool up = dz > 0.f, down = dz < 0.f;
    int cls = 4;
    if (d > r1 && d <= r2) cls = up ? 0 : down ? 1 : cls;
    if (d > r2) cls = up ? 2 : down ? 3 : cls;
    return cls;
}

// segc (b + 1): seg as the kernels read it, ascending within [0, m] and ending at m; blk (b + 1): the first 64-row block of
// every scene.  One thread.
__global__ void csc_plan_kernel(int m, int b, const int *__restrict__ seg, int *__restrict__ segc, int *__restrict__ blk,
                                int *status) {
    if (blockIdx.x || threadIdx.x) return;
    bool bad = seg[0] != 0;
    int prev = 0, nb = 0;
    segc[0] = 0;
    blk[0] = 0;
    for (int s = 0; s < b; ++s) {
        int e = seg[s + 1];
        if (e < prev || e > m || (s == b - 1 && e != m)) {
            bad = true;
            e = s == b - 1 ? m : min(max(e, prev), m);
        }
        segc[s + 1] = e;
        nb += (e - prev + TILE - 1) / TILE;
        blk[s + 1] = nb;
        prev = e;
    }
    if (bad) *status = 1;
}

struct RowBlock {
    int scene, lo, hi, x0;  // rows [lo, hi) of the scene, the first row of this block; scene < 0: a block past the last one
};

__device__ __forceinline__ RowBlock row_block(int bx, int b, const int *__restrict__ segc, const int *__restrict__ blk) {
    RowBlock rb;
    rb.scene = -1; rb.lo = rb.hi = rb.x0 = 0;
    if (bx >= blk[b]) return rb;
    int lo = 0, hi = b - 1;  // the first scene whose blocks end past bx (an empty scene has none)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (blk[mid + 1] > bx) hi = mid;
        else lo = mid + 1;
    }
    rb.scene = lo;
    rb.lo = segc[lo];
    rb.hi = segc[lo + 1];
    rb.x0 = rb.lo + (bx - blk[lo]) * TILE;
    return rb;
}

// coords (2, m, 3): x_i = origin1[p_i0], y_i = origin2[p_i1]; a pair outside its operand reads as zeros (the status word is
// set by the gather of the features)
__global__ __launch_bounds__(TPB) void csc_gather_coord_kernel(int n1, int n2, int m, const float *__restrict__ o1,
                                                               const float *__restrict__ o2, const long long *__restrict__ pairs,
                                                               float *__restrict__ coords) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const long long p0 = pairs[2 * (size_t)i], p1 = pairs[2 * (size_t)i + 1];
    const bool ok0 = p0 >= 0 && p0 < n1, ok1 = p1 >= 0 && p1 < n2;
    for (int k = 0; k < 3; ++k) {
        coords[3 * (size_t)i + k] = ok0 ? o1[3 * (size_t)p0 + k] : 0.f;
        coords[3 * ((size_t)m + i) + k] = ok1 ? o2[3 * (size_t)p1 + k] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------- partitioned row sums ----
// part (nsplit, NCLS, m): sum of exp((S_ij - 1) / t) of row i over the columns j of split blockIdx.y that are of class k or on
// the diagonal.  Every (split, class, row) is written by exactly one workgroup, zeros included.  sdiag (m): S_ii as the tile forms
// it, written by the one lane that holds it: the loss subtracts the very number its log-sum-exps contain, as the eager statements
// do with their one `sim` (the gather's a_i.b_i sums in another order, and the difference, over t, would not cancel).
__global__ __launch_bounds__(TPB) void csc_lse_kernel(int m, int c, int b, const float *__restrict__ A, const float *__restrict__ B,
                                                      const float *__restrict__ coords, const int *__restrict__ segc,
                                                      const int *__restrict__ blk, float inv_t, float r1, float r2,
                                                      float *__restrict__ part, float *__restrict__ sdiag) {
    __shared__ __attribute__((aligned(16))) float sX[TILE][KP];
    __shared__ __attribute__((aligned(16))) float sY[TILE][KP];
    __shared__ float sRow[TILE][3];
    __shared__ float sS[2][2][NCLS][32];
    const RowBlock rb = row_block(blockIdx.x, b, segc, blk);
    if (rb.scene < 0) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int rt = wave >> 1, ct = wave & 1;
    const int x0 = rb.x0, hi = rb.hi;
    const float *cx = coords, *cy = coords + 3 * (size_t)m;
    const int nchunks = (hi - rb.lo + TILE - 1) / TILE;
    const int chunks_per_split = (nchunks + gridDim.y - 1) / gridDim.y;
    const int ch_lo = blockIdx.y * chunks_per_split, ch_hi = min(nchunks, ch_lo + chunks_per_split);
    if (tid < TILE * 3) {
        const int row = tid / 3;
        sRow[row][tid % 3] = x0 + row < hi ? cy[3 * (size_t)(x0 + row) + tid % 3] : 0.f;
    }
    float sm[NCLS][16];
#pragma unroll
    for (int k = 0; k < NCLS; ++k)
#pragma unroll
        for (int e = 0; e < 16; ++e) sm[k][e] = 0.f;
    for (int ch = ch_lo; ch < ch_hi; ++ch) {
        const int y0 = rb.lo + ch * TILE;
        const v16f acc = s_tile(A, x0, B, y0, hi, c, sX, sY, rt, ct);  // (its barriers also publish sRow)
        const int yc = y0 + 32 * ct + r;
        if (yc < hi) {
            const float xx = cx[3 * (size_t)yc], xy = cx[3 * (size_t)yc + 1], xz = cx[3 * (size_t)yc + 2];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = 32 * rt + acc_row(e, h);
                const float ex = expf((acc[e] - 1.f) * inv_t);  // (S - 1 is exact near the largest terms)
                const int cls = csc_class(xx, xy, xz, sRow[row][0], sRow[row][1], sRow[row][2], r1, r2);
                const bool diag = x0 + row == yc;
                if (diag) sdiag[yc] = acc[e];
#pragma unroll
                for (int k = 0; k < NCLS; ++k) sm[k][e] += (diag || cls == k) ? ex : 0.f;
            }
        }
    }
    // the 32 lanes of a half hold the 32 columns of the same 16 rows
#pragma unroll
    for (int k = 0; k < NCLS; ++k) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float v = sm[k][e];
            for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
            if (r == 0) sS[rt][ct][k][acc_row(e, h)] = v;
        }
    }
    __syncthreads();
    if (tid < TILE && x0 + tid < hi) {
        for (int k = 0; k < NCLS; ++k)
            part[((size_t)blockIdx.y * NCLS + k) * m + x0 + tid] = sS[tid >> 5][0][k][tid & 31] + sS[tid >> 5][1][k][tid & 31];
    }
}

// the splits of a row in split order -> lse (NCLS, m), kept WITHOUT the shift: lse_ki = log sum_j exp((S_ij - 1) / t), a number
// of the size of log M whatever t is; rowterm[i] = sum_k (lse_ki + (1 - S_ii) / t), the row's loss terms, formed from two small
// numbers instead of two near 1 / t, with S_ii the tile's
__global__ __launch_bounds__(TPB) void csc_rows_kernel(int m, int nsplit, float t, const float *__restrict__ part,
                                                       const float *__restrict__ sdiag, float *__restrict__ lse,
                                                       double *__restrict__ rowterm) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const double p = (1.0 - (double)sdiag[i]) / (double)t;
    double tot = 0.0;
    for (int k = 0; k < NCLS; ++k) {
        float s = part[(size_t)k * m + i];
        for (int sp = 1; sp < nsplit; ++sp) s += part[((size_t)sp * NCLS + k) * m + i];
        const float l = logf(s);
        lse[(size_t)k * m + i] = l;
        tot += (double)l + p;
    }
    rowterm[i] = tot;
}

// column sums of A and B over the rows of a workgroup's block: colpart (blocks, 2, c) fp64
__global__ __launch_bounds__(TPB) void csc_colsum_kernel(int m, int c, int b, const float *__restrict__ A, const float *__restrict__ B,
                                                         const int *__restrict__ segc, const int *__restrict__ blk,
                                                         double *__restrict__ colpart) {
    const RowBlock rb = row_block(blockIdx.x, b, segc, blk);
    const int ch = threadIdx.x;
    if (rb.scene < 0 || ch >= c) return;
    const int hi = min(rb.hi, rb.x0 + TILE);
    double sa = 0.0, sb = 0.0;
    for (int i = rb.x0; i < hi; ++i) {
        sa += (double)A[(size_t)i * c + ch];
        sb += (double)B[(size_t)i * c + ch];
    }
    colpart[((size_t)blockIdx.x * 2 + 0) * c + ch] = sa;
    colpart[((size_t)blockIdx.x * 2 + 1) * c + ch] = sb;
}

// One workgroup: the scene recurrences of the three scalars, every sum in a fixed order (fp64 accumulators).
__global__ __launch_bounds__(TPB) void csc_finish_kernel(int m, int c, int b, int partitions, const int *__restrict__ segc,
                                                         const int *__restrict__ blk, const double *__restrict__ rowterm,
                                                         const float *__restrict__ pos, const double *__restrict__ colpart,
                                                         const int *__restrict__ status, float *__restrict__ out) {
    __shared__ double sh[TPB];
    const int tid = threadIdx.x;
    double loss = 0.0, pos_acc = 0.0, neg_acc = 0.0;
    for (int s = 0; s < b; ++s) {
        const int lo = segc[s], hi = segc[s + 1];
        if (hi <= lo) continue;  // a scene without pairs is skipped (the divisor stays b)
        const double ms = (double)(hi - lo);
        double rows = 0.0, ps = 0.0;
        for (int i = lo + tid; i < hi; i += TPB) {
            rows += rowterm[i];
            ps += (double)pos[i];
        }
        double dot = 0.0;
        if (tid < c) {
            double sa = 0.0, sb = 0.0;
            for (int q = blk[s]; q < blk[s + 1]; ++q) {
                sa += colpart[((size_t)q * 2 + 0) * c + tid];
                sb += colpart[((size_t)q * 2 + 1) * c + tid];
            }
            dot = sa * sb;
        }
        rows = block_sum(rows, sh);
        ps = block_sum(ps, sh);
        dot = block_sum(dot, sh);
        loss += rows / ms;
        pos_acc += ps / ms;
        neg_acc += dot / (ms * ms) - pos_acc / ms;  // (the pos accumulated so far, as the reference writes it)
    }
    if (tid == 0) {
        const bool bad = *status != 0;  // the caller reads nothing back, so the outputs say it
        out[0] = bad ? NAN : (float)(loss / ((double)b * partitions));
        out[1] = bad ? NAN : (float)(pos_acc / b);
        out[2] = bad ? NAN : (float)(neg_acc / b);
    }
}

// ----------------------------------------------------------------------------------------------------------- backward ----
// blockIdx.y = 0: dAn[x0 .. x0 + 64) = scale D B, own rows i, other rows j;  1: dBn = scale D^T A, own rows j, other rows i.
// D_ij = exp((S_ij - 1) / t - lse[class(i, j)][i]) off the diagonal, D_ii = sum_k exp((S_ii - 1) / t - lse[k][i]) - NCLS, lse
// being the shifted one of csc_rows_kernel.
// scale = g / (b partitions M_s t).
__global__ __launch_bounds__(TPB) void csc_nce_bwd_kernel(int m, int c, int b, const float *__restrict__ A, const float *__restrict__ B,
                                                          const float *__restrict__ coords, const int *__restrict__ segc,
                                                          const int *__restrict__ blk, const float *__restrict__ lse, float inv_t,
                                                          float r1, float r2, float inv_bp, const float *__restrict__ g,
                                                          float *__restrict__ dAn, float *__restrict__ dBn) {
    __shared__ __attribute__((aligned(16))) float sX[TILE][KP];
    __shared__ __attribute__((aligned(16))) float sY[TILE][KP];
    __shared__ float sP[TILE][PP];
    __shared__ float sL[NCLS][LP];
    __shared__ float sOwn[TILE][3];
    const RowBlock rb = row_block(blockIdx.x, b, segc, blk);
    if (rb.scene < 0) return;
    const int mode = blockIdx.y;
    const float *X = mode ? B : A, *Y = mode ? A : B;
    // mode 0 owns rows of S (their y), the lane's column brings x; mode 1 owns columns of S (their x), the lane brings y
    const float *own = mode ? coords : coords + 3 * (size_t)m, *oth = mode ? coords + 3 * (size_t)m : coords;
    float *out = mode ? dBn : dAn;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int rt = wave >> 1, ct = wave & 1;    // the S quadrant of this wavefront
    const int prt = wave & 1, pct = wave >> 1;  // its output tiles: rows prt, channel tiles pct, pct + 2, ...
    const int x0 = rb.x0, hi = rb.hi;
    const int nchunks = (hi - rb.lo + TILE - 1) / TILE, ctiles = (c + 31) / 32;
    if (tid < TILE * 3) sOwn[tid / 3][tid % 3] = x0 + tid / 3 < hi ? own[3 * (size_t)(x0 + tid / 3) + tid % 3] : 0.f;
    for (int e = tid; e < NCLS * TILE; e += TPB) {
        const int k = e / TILE, row = e % TILE;
        sL[k][row] = (mode == 0 && x0 + row < hi) ? lse[(size_t)k * m + x0 + row] : 0.f;
    }
    __syncthreads();
    v16f o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        for (int e = 0; e < 16; ++e) o[u][e] = 0.f;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int y0 = rb.lo + ch * TILE;
        const v16f acc = s_tile(X, x0, Y, y0, hi, c, sX, sY, rt, ct);
        const int yc = y0 + 32 * ct + r;
        const bool cok = yc < hi;
        float lc[NCLS], q0 = 0.f, q1 = 0.f, q2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCLS; ++k) lc[k] = (mode == 1 && cok) ? lse[(size_t)k * m + yc] : 0.f;
        if (cok) { q0 = oth[3 * (size_t)yc]; q1 = oth[3 * (size_t)yc + 1]; q2 = oth[3 * (size_t)yc + 2]; }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = 32 * rt + acc_row(e, h), xr = x0 + row;
            float p = 0.f;
            if (xr < hi && cok) {
                const float s = (acc[e] - 1.f) * inv_t;
                if (xr == yc) {
                    p = -(float)NCLS;
#pragma unroll
                    for (int k = NCLS - 1; k >= 0; --k) p += expf(s - (mode ? lc[k] : sL[k][row]));
                } else {
                    const float w0 = sOwn[row][0], w1 = sOwn[row][1], w2 = sOwn[row][2];
                    const int cls = mode ? csc_class(w0, w1, w2, q0, q1, q2, r1, r2) : csc_class(q0, q1, q2, w0, w1, w2, r1, r2);
                    float l = sL[cls][row];
                    if (mode) l = cls == 0 ? lc[0] : cls == 1 ? lc[1] : cls == 2 ? lc[2] : cls == 3 ? lc[3] : lc[4];
                    p = expf(s - l);
                }
            }
            sP[row][32 * ct + r] = p;  // (the staging barriers of s_tile separate this from the reads of the last round)
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tc = pct + 2 * u;
            if (tc < ctiles) {
                const int chn = 32 * tc + r;
                const bool chok = chn < c;
#pragma unroll 8
                for (int k = 0; k < TILE; k += 2) {
                    const int yr = y0 + k + h;
                    const float a = sP[32 * prt + r][k + h];
                    const float bv = (chok && yr < hi) ? Y[(size_t)yr * c + chn] : 0.f;
                    o[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, o[u], 0, 0, 0);
                }
            }
        }
    }
    const float scale = g[0] * inv_t * inv_bp / (float)(hi - rb.lo);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int chn = 32 * (pct + 2 * u) + r;
        if (chn < c) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int xr = x0 + 32 * prt + acc_row(e, h);
                if (xr < hi) out[(size_t)xr * c + chn] = o[u][e] * scale;
            }
        }
    }
}

struct CscPlan {
    int maxblocks, nsplit;
};

// depends on (m, b) alone, so that the order of every sum depends on (m, seg) alone
CscPlan csc_plan(int m, int b) {
    CscPlan p;
    p.maxblocks = m / TILE + b;  // sum_s ceil(M_s / 64) <= (m + 63 b) / 64
    const int rowblocks = divup(m, TILE);
    p.nsplit = std::min(rowblocks, std::max(1, divup(MAX_SPLIT_BLOCKS, rowblocks)));
    return p;
}

struct CscWs {
    float *part, *pos, *diag, *dAn, *dBn;
    double *colpart, *rowterm;
    int *segc, *blk;
    size_t bytes;
};

CscWs carve_csc(void *base, int m, int c, int b) {
    const CscPlan pl = csc_plan(m, b);
    CscWs w;
    PtvCarver cv{(char *)base, 0};
    w.part = cv.take_n<float>((size_t)pl.nsplit * NCLS * m);
    w.pos = cv.take_n<float>(m);
    w.diag = cv.take_n<float>(m);
    w.rowterm = cv.take_n<double>(m);
    w.colpart = cv.take_n<double>((size_t)pl.maxblocks * 2 * c);
    w.segc = cv.take_n<int>(b + 1);
    w.blk = cv.take_n<int>(b + 1);
    w.dAn = cv.take_n<float>((size_t)m * c);
    w.dBn = cv.take_n<float>((size_t)m * c);
    w.bytes = cv.off;
    return w;
}

bool csc_sizes_ok(long long m, int c, int b) {
    return m >= 1 && m <= CSC_MAX_PAIRS && c >= 4 && c <= CSC_MAX_CHANNELS && c % 4 == 0 && b >= 1 && b <= CSC_MAX_SCENES;
}

bool csc_scalars_ok(float t, int partitions) { return t > 0.f && 1.f / t <= (float)CSC_MAX_INV_T && partitions >= 1; }

}  // namespace

extern "C" int ptv2_csc_abi_version(void) { return 1; }

extern "C" long long ptv2_csc_nce_workspace_bytes(long long m, int c, int b) {
    if (!csc_sizes_ok(m, c, b)) return -1;
    return (long long)carve_csc(nullptr, (int)m, c, b).bytes;
}

extern "C" int csc_nce_fwd_hip_launcher(int n1, int n2, int m, int c, int b, const float *f1, const float *f2, const float *origin1,
                                        const float *origin2, const long long *pairs, const int *seg, float t, float r1, float r2,
                                        int partitions, float *a, float *bn, float *norms, float *coords, float *lse, float *out,
                                        int *status, void *workspace, long long workspace_bytes, void *stream) {
    if (!csc_sizes_ok(m, c, b) || !csc_scalars_ok(t, partitions) || n1 < 1 || n2 < 1 || !f1 || !f2 || !origin1 || !origin2 || !pairs ||
        !seg || !a || !bn || !norms || !coords || !lse || !out || !status)
        return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < ptv2_csc_nce_workspace_bytes(m, c, b)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const CscPlan pl = csc_plan(m, b);
    const CscWs w = carve_csc(workspace, m, c, b);
    const float inv_t = 1.f / t;
    hipLaunchKernelGGL(csc_plan_kernel, dim3(1), dim3(64), 0, st, m, b, seg, w.segc, w.blk, status);
    hipLaunchKernelGGL(msc_gather_norm_kernel, dim3(m), dim3(64), 0, st, n1, n2, m, c, f1, f2, pairs, a, bn, norms, w.pos, status);
    hipLaunchKernelGGL(csc_gather_coord_kernel, dim3(divup(m, TPB)), dim3(TPB), 0, st, n1, n2, m, origin1, origin2, pairs, coords);
    hipLaunchKernelGGL(csc_lse_kernel, dim3(pl.maxblocks, pl.nsplit), dim3(TPB), 0, st, m, c, b, a, bn, coords, w.segc, w.blk, inv_t,
                       r1, r2, w.part, w.diag);
    hipLaunchKernelGGL(csc_rows_kernel, dim3(divup(m, TPB)), dim3(TPB), 0, st, m, pl.nsplit, t, w.part, w.diag, lse, w.rowterm);
    hipLaunchKernelGGL(csc_colsum_kernel, dim3(pl.maxblocks), dim3(TPB), 0, st, m, c, b, a, bn, w.segc, w.blk, w.colpart);
    hipLaunchKernelGGL(csc_finish_kernel, dim3(1), dim3(TPB), 0, st, m, c, b, partitions, w.segc, w.blk, w.rowterm, w.pos, w.colpart,
                       status, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int csc_nce_bwd_hip_launcher(int n1, int n2, int m, int c, int b, const long long *pairs, const int *seg, const int *order,
                                        float t, float r1, float r2, int partitions, const float *a, const float *bn,
                                        const float *norms, const float *coords, const float *lse, const float *g, float *df1,
                                        float *df2, void *workspace, long long workspace_bytes, void *stream) {
    if (!csc_sizes_ok(m, c, b) || !csc_scalars_ok(t, partitions) || n1 < 1 || n2 < 1 || !pairs || !seg || !order || !a || !bn ||
        !norms || !coords || !lse || !g || !df1 || !df2)
        return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < ptv2_csc_nce_workspace_bytes(m, c, b)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const CscPlan pl = csc_plan(m, b);
    const CscWs w = carve_csc(workspace, m, c, b);
    if (hipMemsetAsync(df1, 0, sizeof(float) * (size_t)n1 * c, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    if (hipMemsetAsync(df2, 0, sizeof(float) * (size_t)n2 * c, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    // (the plan's status word: the forward has reported a malformed seg already; the part buffer is free in this direction)
    hipLaunchKernelGGL(csc_plan_kernel, dim3(1), dim3(64), 0, st, m, b, seg, w.segc, w.blk, (int *)w.part);
    hipLaunchKernelGGL(csc_nce_bwd_kernel, dim3(pl.maxblocks, 2), dim3(TPB), 0, st, m, c, b, a, bn, coords, w.segc, w.blk, lse,
                       1.f / t, r1, r2, 1.f / ((float)b * (float)partitions), g, w.dAn, w.dBn);
    hipLaunchKernelGGL(msc_scatter_kernel, dim3(m), dim3(64), 0, st, n1, m, c, 0, pairs, order, w.dAn, a, norms, df1);
    hipLaunchKernelGGL(msc_scatter_kernel, dim3(m), dim3(64), 0, st, n2, m, c, 1, pairs, order + m, w.dBn, bn, norms + m, df2);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
