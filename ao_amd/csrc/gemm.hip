// ao_amd/csrc/gemm.hip -- fp32 row GEMMs of the per-point Linear layers on the CDNA4 matrix cores.
//
// Every nn.Linear of a PT-v2m2 Block (point_transformer_v2m2_base.py:64-66 linear_q/k/v, :143-144 fc1/fc3)
// is Y (m,n) = X (m,k) W^T with m = points (1e3..1e6) and n, k = channels (48..512): 0.5 GFLOP and
// 2 m (n+k) floats of traffic, i.e. HBM-bound by a wide margin.  Library GEMMs spend 40-50 us on the
// m=120k, n=k=48 case whose traffic is worth 8 us, so the block runtime (block.hip) uses this kernel:
//   * V_MFMA_F32_16X16X4_F32 (true fp32, no tf32 rounding), one 16-row strip x BN columns per wavefront,
//     operands swapped (A := W tile, B := X tile) so each lane ends with 4 consecutive output columns of one
//     row and stores a float4;
//   * X / W chunks of 32 reduction indices staged through LDS (row pitch 36 floats: the ds_read_b128 of the
//     16 rows of a strip hit 64 distinct banks), next chunk prefetched into registers during the MFMAs;
//   * W either (n,k) row-major (the forward product) or (k,n) row-major (the input-gradient product
//     gX = gY W reads the same weight matrix with the roles of its two dimensions swapped);
//   * epilogue: + bias[n], optional accumulate onto Y (sums of several products, residual gradients).
#include <algorithm>

#include "common.h"

namespace gemm {

constexpr int BM = 64;        // rows per workgroup (4 wavefronts x 16)
constexpr int THREADS = 256;
// KC = reduction indices per LDS chunk (32, or 64 for k >= 192: half as many chunk hand-offs, twice the loads in
// flight -- with 24 MFMAs per chunk the prefetch distance of one chunk did not cover the memory latency and every
// chunk of the deep stages' k = 192 / 384 cost ~1 us).
// LDS image of a chunk: row pitch KC + 8 floats, and the 16-byte column slots of a row XOR-swizzled with the row index
// (slot ^= row & 1 at KC = 32, row & 3 at KC = 64).  ds_read_b128 is served in four NON-contiguous 16-lane groups
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...; guides/MI355X_MICROARCH.md, LDS): with the plain KC + 4 pitch of rounds
// 1-2 two of the sixteen 16-byte slots of every group were hit twice (SQ_LDS_BANK_CONFLICT 0.25-0.35 of the LDS-active
// cycles in all six variants, profiles/r02_final_sq_counters.jsonl).  This image is conflict-free for the operand reads
// (64 banks), for the ds_write_b128 stores of the staging (8-lane groups, 32 banks) and for the transposing scalar stores
// of the (k,n)-major weight tile; enumerated in tools/lds_layout_search.py.  The XOR only permutes the float4 slots a
// lane owns, so the contraction order -- and every result bit -- is unchanged.
template <int KC>
__device__ __forceinline__ int lds_slot(int row, int k4) {  // float offset of float4 slot k4 of `row`
    return row * (KC + 8) + 4 * (k4 ^ (row & (KC == 32 ? 1 : 3)));
}

// up to 3 products of one shape in one launch: independent (blockIdx.y selects X/W/bias/Y: the q, k, v projections
// of one input) or summed into one output (the reduction runs over the pairs back to back: g_f1 = sum_i gY_i W_i)
struct GemmMulti {
    const float *X[3], *W[3], *bias[3];
    float *Y[3];
    int count;  // 0: single product from the plain arguments
    int sum;    // != 0: Y[0] = sum_i X[i] op(W[i])
    // BatchNorm fused on either side (block.hip): the X operand passes through ReLU(x * xsc[k] + xsh[k]) on its way
    // into LDS (the normalise + ReLU of the BatchNorm in front of this Linear, never materialised), and/or the
    // epilogue leaves per-row-block column statistics of the output in stats[z] (records [row block][2][n]: sum and
    // centred sum of squares of the block's rows) for the BatchNorm behind it
    const float *xsc, *xsh;
    float *stats[3];
    // backward twin of `stats`: Y is the gradient entering a BatchNorm (+ ReLU) whose input was bnx (m,n); the epilogue
    // leaves per-row-block records [2][n] of sum g' and sum g' * xhat (g' = Y masked by the ReLU) in brec -- the reduce
    // pass of that BatchNorm's backward (bn.hip: bn_bwd_reduce_kernel) without its own launch and its two tensor reads
    const float *bnx, *bnm, *bnr, *bng, *bnb;
    int bnrelu;
    float *brec;
};

// Epilogue shared by the row GEMM kernels: bias / accumulate / store, then (optionally) the BatchNorm-backward reduce records
// and the BatchNorm-forward tile statistics of this 64-row block (see GemmMulti).  `sS`: >= 4 * 2 * BN floats of LDS scratch
// that no wavefront reads as an operand any more (the callers synchronise inside: every use below follows a barrier).
template <int BN>
__device__ __forceinline__ void gemm_epilogue(v4f (&acc)[BN / 16], const long long row0, const int rb, const int n0, const int z,
                                              const bool indep, const int m, const int n, const float *__restrict__ bias,
                                              float *__restrict__ Y, const int accumulate, const GemmMulti &multi, float *sS_) {
    constexpr int NT = BN / 16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float *sX = sS_;
    // D[i][j]: i = output column within the tile = (lane >> 4) * 4 + reg, j = row within the strip = lane & 15
    const long long row = row0 + wid * 16 + (lane & 15);
    float4 val[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = n0 + t * 16 + (lane >> 4) * 4;
        float4 v = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
        {
            const float4 bb = ptv2_ld_or_zero((const float4 *)(bias + col), bias && col < n);
            v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
        }
        val[t] = v;
        if (row < m && col < n) {
            float4 *dst = (float4 *)(Y + row * n + col);
            if (accumulate) {
                const float4 o = *dst;
                v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
            }
            *dst = v;
        }
    }
    if (multi.count && multi.brec) {
        float *sS = sX;  // [4 waves][2][BN]
        const bool rv = row < m;
        const int cl = (lane >> 4) * 4;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = n0 + t * 16 + cl;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f), e = d;
            if (rv && col < n) {
                const float4 xv = *(const float4 *)(multi.bnx + row * n + col);
                const float4 mm = *(const float4 *)(multi.bnm + col), rs = *(const float4 *)(multi.bnr + col);
                float4 h;
                h.x = (xv.x - mm.x) * rs.x; h.y = (xv.y - mm.y) * rs.y; h.z = (xv.z - mm.z) * rs.z; h.w = (xv.w - mm.w) * rs.w;
                d = val[t];
                if (multi.bnrelu) {
                    const float4 gg = *(const float4 *)(multi.bng + col), bb = *(const float4 *)(multi.bnb + col);
                    if (__builtin_fmaf(h.x, gg.x, bb.x) <= 0.f) d.x = 0.f;
                    if (__builtin_fmaf(h.y, gg.y, bb.y) <= 0.f) d.y = 0.f;
                    if (__builtin_fmaf(h.z, gg.z, bb.z) <= 0.f) d.z = 0.f;
                    if (__builtin_fmaf(h.w, gg.w, bb.w) <= 0.f) d.w = 0.f;
                }
                e = make_float4(d.x * h.x, d.y * h.y, d.z * h.z, d.w * h.w);
            }
            const float ax = row16_sum(d.x), ay = row16_sum(d.y), az = row16_sum(d.z), aw = row16_sum(d.w);
            const float bx = row16_sum(e.x), by = row16_sum(e.y), bz = row16_sum(e.z), bw = row16_sum(e.w);
            if ((lane & 15) == 0) {
                *(float4 *)(sS + (wid * 2 + 0) * BN + t * 16 + cl) = make_float4(ax, ay, az, aw);
                *(float4 *)(sS + (wid * 2 + 1) * BN + t * 16 + cl) = make_float4(bx, by, bz, bw);
            }
        }
        __syncthreads();
        for (int e = tid; e < 2 * BN; e += THREADS) {
            const int which = e / BN, cc = e - which * BN;
            if (n0 + cc < n) {
                float a = sS[which * BN + cc];
#pragma unroll
                for (int w = 1; w < 4; ++w) a += sS[(w * 2 + which) * BN + cc];
                multi.brec[(size_t)rb * 2 * n + (size_t)which * n + n0 + cc] = a;
            }
        }
    }
    float *stats = multi.count ? multi.stats[indep ? z : 0] : nullptr;
    if (stats) {
        // column statistics of this 64-row block: sum, then sum of squares about the block mean (two passes over
        // the register tile; the finalize merges blocks with the parallel-variance formula in double)
        float *sS = sX;  // [4 waves][BN]: the operand staging is no longer needed
        const bool rv = row < m;
        const int cnt = (int)((m - row0) < BM ? (m - row0) : BM);
        const int cl = (lane >> 4) * 4;  // my 4 columns within a 16-wide tile
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float sx = row16_sum(rv ? val[t].x : 0.f), sy = row16_sum(rv ? val[t].y : 0.f);
            const float sz = row16_sum(rv ? val[t].z : 0.f), sw = row16_sum(rv ? val[t].w : 0.f);
            if ((lane & 15) == 0) *(float4 *)(sS + wid * BN + t * 16 + cl) = make_float4(sx, sy, sz, sw);
        }
        __syncthreads();
        float4 mean[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float4 a = *(const float4 *)(sS + t * 16 + cl);
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float4 o = *(const float4 *)(sS + w * BN + t * 16 + cl);
                a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
            }
            mean[t] = a;  // block sums for now
        }
        __syncthreads();
        const float inv = 1.0f / (float)cnt;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = n0 + t * 16 + cl;
            if (wid == 0 && (lane & 15) == 0 && col < n) *(float4 *)(stats + (size_t)rb * 2 * n + col) = mean[t];
            const float dx = rv ? val[t].x - mean[t].x * inv : 0.f, dy = rv ? val[t].y - mean[t].y * inv : 0.f;
            const float dz = rv ? val[t].z - mean[t].z * inv : 0.f, dw = rv ? val[t].w - mean[t].w * inv : 0.f;
            const float qx = row16_sum(dx * dx), qy = row16_sum(dy * dy), qz = row16_sum(dz * dz), qw = row16_sum(dw * dw);
            if ((lane & 15) == 0) *(float4 *)(sS + wid * BN + t * 16 + cl) = make_float4(qx, qy, qz, qw);
        }
        __syncthreads();
        if (wid == 0 && (lane & 15) == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = n0 + t * 16 + cl;
                if (col < n) {
                    float4 a = *(const float4 *)(sS + t * 16 + cl);
#pragma unroll
                    for (int w = 1; w < 4; ++w) {
                        const float4 o = *(const float4 *)(sS + w * BN + t * 16 + cl);
                        a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
                    }
                    *(float4 *)(stats + (size_t)rb * 2 * n + n + col) = a;
                }
            }
        }
    }
}

// BF16: the same kernel with bf16 matrix-core operands.  A lane owns KC / 4 consecutive reduction indices of its row /
// column per chunk -- exactly the 8-per-lane operand layout of V_MFMA_F32_16X16X32_BF16 -- so the 8 fp32 MFMAs of
// a 32-index chunk become one instruction on operands rounded to bf16 (fp32 accumulation, fp32 in memory).
template <int BN, bool W_KMAJOR, int KC, bool BF16>
__global__ __launch_bounds__(THREADS) void rows_gemm_kernel(int m, int n, int k, const float *__restrict__ X0,
                                                            const float *__restrict__ W0,
                                                            const float *__restrict__ bias0, float *__restrict__ Y0,
                                                            int accumulate, int ncb, GemmMulti multi) {
    constexpr int PITCH = KC + 8;
    __shared__ __attribute__((aligned(16))) float sX[BM * PITCH];
    __shared__ __attribute__((aligned(16))) float sW[BN * PITCH];
    constexpr int NT = BN / 16;            // MFMA column tiles per wavefront
    constexpr int KQ = KC / 4;             // float4 per row of a chunk
    constexpr int XLOADS = BM * KQ / THREADS;
    constexpr int WQ = BN * KQ;            // float4 slots of the W chunk
    constexpr int WLOADS = (WQ + THREADS - 1) / THREADS;
    constexpr int RUN = KC / 16;           // float4 per lane and chunk (a lane owns KC / 4 consecutive reduction indices)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int rb = blockIdx.x / ncb, cb = blockIdx.x - rb * ncb;
    const long long row0 = (long long)rb * BM;
    const int n0 = cb * BN;
    const int z = blockIdx.y;
    const bool indep = multi.count && !multi.sum;
    const float *bias = indep ? multi.bias[z] : bias0;
    float *Y = multi.count ? multi.Y[indep ? z : 0] : Y0;
    const int npair = (multi.count && multi.sum) ? multi.count : 1;
    const float *X = multi.count ? multi.X[indep ? z : 0] : X0;
    const float *W = multi.count ? multi.W[indep ? z : 0] : W0;

    float4 rx[XLOADS], rw[WLOADS];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < XLOADS; ++j) {
            const int q = tid + j * THREADS, r = q / KQ, kq = (q % KQ) * 4;
            const long long row = row0 + r;
            rx[j] = ptv2_ld_or_zero((const float4 *)(X + row * k + k0 + kq), row < m && k0 + kq < k);
            if (multi.xsc && k0 + kq < k) {
                const float4 s4 = *(const float4 *)(multi.xsc + k0 + kq), h4 = *(const float4 *)(multi.xsh + k0 + kq);
                rx[j].x = fmaxf(__builtin_fmaf(rx[j].x, s4.x, h4.x), 0.f);
                rx[j].y = fmaxf(__builtin_fmaf(rx[j].y, s4.y, h4.y), 0.f);
                rx[j].z = fmaxf(__builtin_fmaf(rx[j].z, s4.z, h4.z), 0.f);
                rx[j].w = fmaxf(__builtin_fmaf(rx[j].w, s4.w, h4.w), 0.f);
            }
        }
#pragma unroll
        for (int j = 0; j < WLOADS; ++j) {
            const int q = tid + j * THREADS;
            {  // (every load unconditional: see ptv2_zero_pad)
                if (!W_KMAJOR) {
                    const int r = q / KQ, kq = (q % KQ) * 4;
                    rw[j] = ptv2_ld_or_zero((const float4 *)(W + (long long)(n0 + r) * k + k0 + kq), q < WQ && n0 + r < n && k0 + kq < k);
                } else {
                    // consecutive lanes take consecutive reduction indices of one column quad: the transposing LDS store
                    // below then writes consecutive addresses (conflict-free).  With the lanes along the columns (the
                    // coalesced order for this load) the four scalar stores hit two banks with every pitch that keeps
                    // ds_read_b128 aligned: SQ_LDS_BANK_CONFLICT was 0.6 of the LDS-active cycles of these kernels
                    // (profiles/r02_final_sq_counters.jsonl).  W is at most 1 MB and L2-resident; 16-byte pieces of it
                    // per lane cost less than the 6-way store conflict.
                    const int kk = q % KC, cq = (q / KC) * 4;
                    rw[j] = ptv2_ld_or_zero((const float4 *)(W + (long long)(k0 + kk) * n + n0 + cq), q < WQ && k0 + kk < k && n0 + cq < n);
                }
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < XLOADS; ++j) {
            const int q = tid + j * THREADS, r = q / KQ;
            *(float4 *)(sX + lds_slot<KC>(r, q % KQ)) = rx[j];
        }
#pragma unroll
        for (int j = 0; j < WLOADS; ++j) {
            const int q = tid + j * THREADS;
            if (q < WQ) {
                if (!W_KMAJOR) {
                    const int r = q / KQ;
                    *(float4 *)(sW + lds_slot<KC>(r, q % KQ)) = rw[j];
                } else {
                    const int kk = q % KC, cq = (q / KC) * 4;
                    sW[lds_slot<KC>(cq + 0, kk >> 2) + (kk & 3)] = rw[j].x; sW[lds_slot<KC>(cq + 1, kk >> 2) + (kk & 3)] = rw[j].y;
                    sW[lds_slot<KC>(cq + 2, kk >> 2) + (kk & 3)] = rw[j].z; sW[lds_slot<KC>(cq + 3, kk >> 2) + (kk & 3)] = rw[j].w;
                }
            }
        }
    };

    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};

    // lane (i = lane & 15, s = lane >> 4) owns reduction indices s*KC/4 .. (s+1)*KC/4-1 of row / column i in each
    // chunk: the contraction order differs from k-ascending, identically for both operands
    // (row & mask is the same for the rows l15, 16 + l15, 32 + l15 ...: one set of swizzled slot offsets serves X and W)
    const int l15 = lane & 15, sq = lane >> 4;
    int slot[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) slot[j] = lds_slot<KC>(l15, sq * RUN + j);
    const float *px = sX + wid * 16 * PITCH;
    const float *pw = sW;
    for (int pair = 0; pair < npair; ++pair) {
        if (pair > 0) {
            X = multi.X[pair];
            W = multi.W[pair];
            __syncthreads();  // the previous pair's last chunk is still being read
        }
        fetch(0);
        stash();
        __syncthreads();
        for (int k0 = 0; k0 < k; k0 += KC) {
            const bool more = k0 + KC < k;
            if (more) fetch(k0 + KC);
            float4 xr[RUN];
#pragma unroll
            for (int j = 0; j < RUN; ++j) xr[j] = *(const float4 *)(px + slot[j]);
            if constexpr (BF16) {
                ptv2_bf16x8 xb[RUN / 2];
#pragma unroll
                for (int j = 0; j < RUN / 2; ++j) xb[j] = ptv2_pack_bf16(xr[2 * j], xr[2 * j + 1]);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int j = 0; j < RUN / 2; ++j) {
                        const float4 w0 = *(const float4 *)(pw + t * 16 * PITCH + slot[2 * j]);
                        const float4 w1 = *(const float4 *)(pw + t * 16 * PITCH + slot[2 * j + 1]);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ptv2_pack_bf16(w0, w1), xb[j], acc[t], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int j = 0; j < RUN; ++j) {
                        const float4 w4 = *(const float4 *)(pw + t * 16 * PITCH + slot[j]);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.x, xr[j].x, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.y, xr[j].y, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.z, xr[j].z, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.w, xr[j].w, acc[t], 0, 0, 0);
                    }
                }
            }
            if (more) {
                __syncthreads();
                stash();
                __syncthreads();
            }
        }
    }
    gemm_epilogue<BN>(acc, row0, rb, n0, z, indep, m, n, bias, Y, accumulate, multi, sX);
}

// ---- the same product with X read straight into the MFMA operand registers ("direct" form, round 3) -----------------
// A wavefront's 16-row strip of X is used by that wavefront alone: staging it through LDS bought coalescing only, at the
// price of a store, a load and two workgroup barriers per 32- / 64-index chunk -- 44-58 % of these kernels' wave cycles were
// spent parked, 30-40 % in issue stalls (profiles/r02_final_sq_counters.jsonl).  Here lane (row l15, quarter q) loads the
// float4 at reduction indices 16 j + 4 q .. + 3 of ITS row for every j -- the four lanes of a row read 64 contiguous bytes
// per instruction, the access pattern that streams strided rows at 4.7 TB/s (tools/probes/read_pattern_probe.hip; a
// contiguous run per lane, round 1's split-K attempt, reads 64 distinct lines per instruction at 2.9 TB/s) -- all K / 16
// loads of the strip in flight at once, no chunk loop.  The BN x K weight block is staged in LDS once per workgroup (the
// only barrier before the epilogue; (k,n)-major weights are transposed on the way in) with row pitch K + 8 floats: the
// ds_read_b128 operand reads of a lane group fall on 16 distinct slots for every K in use.  Contraction index of lane
// quarter q in step (j, e): k = 16 j + 4 q + e, identically for both operands.
template <int BN, bool W_KMAJOR, int K, bool BF16>
__global__ __launch_bounds__(THREADS) void rows_gemm_direct_kernel(int m, int n, const float *__restrict__ X0,
                                                                   const float *__restrict__ W0, const float *__restrict__ bias0,
                                                                   float *__restrict__ Y0, int accumulate, int ncb, GemmMulti multi) {
    constexpr int NT = BN / 16, QF = K / 16, LDW = K + 8, KQ = K / 4;
    extern __shared__ float4 gd_lds4[];
    float *sW = (float *)gd_lds4;            // [BN][K + 8]
    float *sSc = sW + (size_t)BN * LDW;       // [K] scale, [K] shift of the fused BatchNorm + ReLU on X (when present)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const int rb = blockIdx.x / ncb, cb = blockIdx.x - rb * ncb;
    const long long row0 = (long long)rb * BM;
    const int n0 = cb * BN;
    const int z = blockIdx.y;
    const bool indep = multi.count && !multi.sum;
    const float *bias = indep ? multi.bias[z] : bias0;
    float *Y = multi.count ? multi.Y[indep ? z : 0] : Y0;
    const int npair = (multi.count && multi.sum) ? multi.count : 1;
    const float *X = multi.count ? multi.X[indep ? z : 0] : X0;
    const float *W = multi.count ? multi.W[indep ? z : 0] : W0;
    const long long row = row0 + wid * 16 + l15;
    const bool rv = row < m;

    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    if (multi.xsc)
        for (int e = tid; e < K; e += THREADS) { sSc[e] = multi.xsc[e]; sSc[K + e] = multi.xsh[e]; }
    for (int pair = 0; pair < npair; ++pair) {
        if (pair > 0) {
            X = multi.X[pair];
            W = multi.W[pair];
            __syncthreads();  // the previous pair's weight block is still being read
        }
        // my row of X: every load of the strip requested before anything waits
        float4 x[QF];
        const float *xr = rv ? X + row * K + 4 * q : ptv2_zero_pad;  // (rows past the end read the zero pad: no branch per load)
#pragma unroll
        for (int j = 0; j < QF; ++j) x[j] = *(const float4 *)(xr + 16 * j);
        // the weight block of this column block: unrolled in batches of up to 8 unconditional loads, then the LDS stores
        // (as a run-time loop every 16-byte piece was requested, waited for and stored on its own)
        if (!W_KMAJOR) {
            constexpr int WL = (BN * KQ + THREADS - 1) / THREADS;
#pragma unroll
            for (int b0 = 0; b0 < WL; b0 += 8) {
                float4 w4[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (b0 + i < WL) {
                        const int e = tid + (b0 + i) * THREADS, r = e / KQ, k4 = e - r * KQ;
                        w4[i] = ptv2_ld_or_zero((const float4 *)(W + (long long)(n0 + r) * K + 4 * k4), e < BN * KQ && n0 + r < n);
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (b0 + i < WL) {
                        const int e = tid + (b0 + i) * THREADS, r = e / KQ, k4 = e - r * KQ;
                        if (e < BN * KQ) *(float4 *)(sW + (size_t)r * LDW + 4 * k4) = w4[i];
                    }
                }
            }
        } else {
            constexpr int WL = ((BN / 4) * K + THREADS - 1) / THREADS;
#pragma unroll
            for (int b0 = 0; b0 < WL; b0 += 8) {
                float4 w4[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (b0 + i < WL) {
                        const int e = tid + (b0 + i) * THREADS;
                        const int kk = e % K, cq = (e / K) * 4;  // consecutive lanes: consecutive k of one column quad (conflict-free stores)
                        w4[i] = ptv2_ld_or_zero((const float4 *)(W + (long long)kk * n + n0 + cq), e < (BN / 4) * K && n0 + cq < n);
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (b0 + i < WL) {
                        const int e = tid + (b0 + i) * THREADS;
                        const int kk = e % K, cq = (e / K) * 4;
                        if (e < (BN / 4) * K) {
                            sW[(size_t)(cq + 0) * LDW + kk] = w4[i].x; sW[(size_t)(cq + 1) * LDW + kk] = w4[i].y;
                            sW[(size_t)(cq + 2) * LDW + kk] = w4[i].z; sW[(size_t)(cq + 3) * LDW + kk] = w4[i].w;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (multi.xsc) {
#pragma unroll
            for (int j = 0; j < QF; ++j) {
                const float4 s4 = *(const float4 *)(sSc + 16 * j + 4 * q), h4 = *(const float4 *)(sSc + K + 16 * j + 4 * q);
                x[j].x = fmaxf(__builtin_fmaf(x[j].x, s4.x, h4.x), 0.f); x[j].y = fmaxf(__builtin_fmaf(x[j].y, s4.y, h4.y), 0.f);
                x[j].z = fmaxf(__builtin_fmaf(x[j].z, s4.z, h4.z), 0.f); x[j].w = fmaxf(__builtin_fmaf(x[j].w, s4.w, h4.w), 0.f);
            }
        }
        const float *pw = sW + (size_t)l15 * LDW + 4 * q;
        if constexpr (BF16) {
#pragma unroll
            for (int j = 0; j < QF; j += 2) {
                const float4 x1 = j + 1 < QF ? x[j + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
                const ptv2_bf16x8 xb = ptv2_pack_bf16(x[j], x1);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float4 w0 = *(const float4 *)(pw + (size_t)t * 16 * LDW + 16 * j);
                    const float4 w1 = j + 1 < QF ? *(const float4 *)(pw + (size_t)t * 16 * LDW + 16 * (j + 1)) : make_float4(0.f, 0.f, 0.f, 0.f);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ptv2_pack_bf16(w0, w1), xb, acc[t], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < QF; ++j) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float4 w4 = *(const float4 *)(pw + (size_t)t * 16 * LDW + 16 * j);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.x, x[j].x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.y, x[j].y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.z, x[j].z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.w, x[j].w, acc[t], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();  // the weight block is dead: its LDS is the epilogue's scratch
    gemm_epilogue<BN>(acc, row0, rb, n0, z, indep, m, n, bias, Y, accumulate, multi, sW);
}

// ---- the deep levels' form: 16 rows per workgroup, the contraction split over its four wavefronts ("k-split", round 6) -----------
// At 1-20 k rows a launch of the kernels above is a few hundred workgroups that all run the same serial chain -- request a
// chunk, wait a memory round trip, stage it, barrier, 24-32 matrix instructions, again for the next chunk -- in lockstep: 9-23 us
// for 0.1-0.3 GFLOP (the matrix work itself is 2-3 us), a quarter of every deep Block.  Here a workgroup owns ONE 16-row strip x
// BN columns and each wavefront a quarter of the reduction indices: every operand of the workgroup -- its rows of X (64
// contiguous bytes per 4 lanes) and its BN x K / 4 piece of W, straight into the matrix-instruction operand registers, no LDS
// staging -- is requested at once, one round trip; K / 16 x BN / 16 matrix instructions per wavefront; the four partial tiles meet
// in LDS (added in wavefront order: fixed association) and each wavefront finishes every fourth column tile: bias, accumulate,
// store, and -- a wavefront holds all 16 rows of its tile -- the BatchNorm records of the strip without another exchange.  Four
// times the workgroups of the 64-row form (short ones, whose phases interleave on a compute unit); W (<= 1 MB) comes from L2.
// Records (forward statistics / backward reduce sums) are per 16-ROW block: rows_gemm_record_rows() tells the caller.
template <int BN, bool W_KMAJOR, int K>
__global__ __launch_bounds__(THREADS) void rows_gemm_ksplit_kernel(int m, int n, const float *__restrict__ X0, const float *__restrict__ W0,
                                                                   const float *__restrict__ bias0, float *__restrict__ Y0, int accumulate,
                                                                   int ncb, GemmMulti multi) {
    constexpr int NT = BN / 16, QF = K / 16, JW = (QF + 3) / 4;  // reduction steps of 16 indices: JW per wavefront
    __shared__ __attribute__((aligned(16))) float sRed[4][NT][64 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const int rb = blockIdx.x / ncb, cb = blockIdx.x - rb * ncb;
    const long long row0 = (long long)rb * 16;
    const int n0 = cb * BN;
    const int z = blockIdx.y;
    const bool indep = multi.count && !multi.sum;
    const float *bias = indep ? multi.bias[z] : bias0;
    float *Y = multi.count ? multi.Y[indep ? z : 0] : Y0;
    const int npair = (multi.count && multi.sum) ? multi.count : 1;
    const long long row = row0 + l15;
    const bool rv = row < m;
    const int j0 = wid * JW;
    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int pair = 0; pair < npair; ++pair) {
        const float *X = multi.count ? multi.X[indep ? z : pair] : X0;
        const float *W = multi.count ? multi.W[indep ? z : pair] : W0;
        // every operand of my quarter of the reduction, requested before anything waits (masked lanes read the zero pad)
        float4 x[JW], w[JW][NT], s4[JW], h4[JW];
        const float *xr = rv ? X + row * K + 4 * q : ptv2_zero_pad;
#pragma unroll
        for (int jj = 0; jj < JW; ++jj) {
            const int j = j0 + jj;
            const bool jok = j < QF;
            x[jj] = *(const float4 *)((jok && rv) ? xr + 16 * j : ptv2_zero_pad);
            if (multi.xsc) {
                s4[jj] = *(const float4 *)(jok ? multi.xsc + 16 * j + 4 * q : ptv2_zero_pad);
                h4[jj] = *(const float4 *)(jok ? multi.xsh + 16 * j + 4 * q : ptv2_zero_pad);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = n0 + 16 * t + l15;
                const bool ok = jok && col < n;
                if (!W_KMAJOR) {
                    w[jj][t] = *(const float4 *)(ok ? W + (long long)col * K + 16 * j + 4 * q : ptv2_zero_pad);
                } else {  // W (k, n): four reduction indices of my column, 64 contiguous bytes per quarter and index
                    const float *wp = ok ? W + (long long)(16 * j + 4 * q) * n + col : ptv2_zero_pad;
                    const long long st = ok ? n : 0;
                    w[jj][t] = make_float4(wp[0], wp[st], wp[2 * st], wp[3 * st]);
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < JW; ++jj) {
            if (multi.xsc) {  // ReLU(x * sc + sh): the BatchNorm + ReLU in front of this Linear (zero scale / shift past K: 0)
                x[jj].x = fmaxf(__builtin_fmaf(x[jj].x, s4[jj].x, h4[jj].x), 0.f); x[jj].y = fmaxf(__builtin_fmaf(x[jj].y, s4[jj].y, h4[jj].y), 0.f);
                x[jj].z = fmaxf(__builtin_fmaf(x[jj].z, s4[jj].z, h4[jj].z), 0.f); x[jj].w = fmaxf(__builtin_fmaf(x[jj].w, s4[jj].w, h4[jj].w), 0.f);
                if (!rv) x[jj] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[jj][t].x, x[jj].x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[jj][t].y, x[jj].y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[jj][t].z, x[jj].z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[jj][t].w, x[jj].w, acc[t], 0, 0, 0);
            }
        }
    }
    // ---- the four partial tiles meet in LDS; wavefront w finishes the column tiles t = w, w + 4, ...
#pragma unroll
    for (int t = 0; t < NT; ++t) *(float4 *)(&sRed[wid][t][4 * lane]) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    __syncthreads();
    float *stats = multi.count ? multi.stats[indep ? z : 0] : nullptr;
    const int cnt = (int)((m - row0) < 16 ? (m - row0) : 16);
    const float inv = 1.0f / (float)cnt;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if ((t & 3) != wid) continue;  // (uniform over the wavefront)
        const float4 a0 = *(const float4 *)(&sRed[0][t][4 * lane]), a1 = *(const float4 *)(&sRed[1][t][4 * lane]);
        const float4 a2 = *(const float4 *)(&sRed[2][t][4 * lane]), a3 = *(const float4 *)(&sRed[3][t][4 * lane]);
        // D[i][j]: i = output column within the tile = 4 q + reg, j = row within the strip = l15
        const int col = n0 + 16 * t + 4 * q;
        const bool cok = col < n;
        float4 v = make_float4(((a0.x + a1.x) + a2.x) + a3.x, ((a0.y + a1.y) + a2.y) + a3.y, ((a0.z + a1.z) + a2.z) + a3.z,
                               ((a0.w + a1.w) + a2.w) + a3.w);
        {
            const float4 bb = ptv2_ld_or_zero((const float4 *)(bias + col), bias && cok);
            v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
        }
        const float4 val = v;
        if (rv && cok) {
            float4 *dst = (float4 *)(Y + row * n + col);
            if (accumulate) {
                const float4 o = *dst;
                v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
            }
            *dst = v;
        }
        if (multi.count && multi.brec) {  // reduce records of the BatchNorm (+ ReLU) this gradient enters: sum g', sum g' xhat
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f), e = d;
            if (rv && cok) {
                const float4 xv = *(const float4 *)(multi.bnx + row * n + col);
                const float4 mm = *(const float4 *)(multi.bnm + col), rs = *(const float4 *)(multi.bnr + col);
                float4 h;
                h.x = (xv.x - mm.x) * rs.x; h.y = (xv.y - mm.y) * rs.y; h.z = (xv.z - mm.z) * rs.z; h.w = (xv.w - mm.w) * rs.w;
                d = val;
                if (multi.bnrelu) {
                    const float4 gg = *(const float4 *)(multi.bng + col), bb = *(const float4 *)(multi.bnb + col);
                    if (__builtin_fmaf(h.x, gg.x, bb.x) <= 0.f) d.x = 0.f;
                    if (__builtin_fmaf(h.y, gg.y, bb.y) <= 0.f) d.y = 0.f;
                    if (__builtin_fmaf(h.z, gg.z, bb.z) <= 0.f) d.z = 0.f;
                    if (__builtin_fmaf(h.w, gg.w, bb.w) <= 0.f) d.w = 0.f;
                }
                e = make_float4(d.x * h.x, d.y * h.y, d.z * h.z, d.w * h.w);
            }
            const float ax = row16_sum(d.x), ay = row16_sum(d.y), az = row16_sum(d.z), aw = row16_sum(d.w);
            const float bx = row16_sum(e.x), by = row16_sum(e.y), bz = row16_sum(e.z), bw = row16_sum(e.w);
            if (l15 == 0 && cok) {
                *(float4 *)(multi.brec + (size_t)rb * 2 * n + col) = make_float4(ax, ay, az, aw);
                *(float4 *)(multi.brec + (size_t)rb * 2 * n + n + col) = make_float4(bx, by, bz, bw);
            }
        }
        if (stats) {  // column statistics of this 16-row block: sum, sum of squares about the block mean
            const float sx = row16_sum(rv ? val.x : 0.f), sy = row16_sum(rv ? val.y : 0.f);
            const float sz = row16_sum(rv ? val.z : 0.f), sw = row16_sum(rv ? val.w : 0.f);
            const float dx = rv ? val.x - sx * inv : 0.f, dy = rv ? val.y - sy * inv : 0.f;
            const float dz = rv ? val.z - sz * inv : 0.f, dw = rv ? val.w - sw * inv : 0.f;
            const float qx = row16_sum(dx * dx), qy = row16_sum(dy * dy), qz = row16_sum(dz * dz), qw = row16_sum(dw * dw);
            if (l15 == 0 && cok) {
                *(float4 *)(stats + (size_t)rb * 2 * n + col) = make_float4(sx, sy, sz, sw);
                *(float4 *)(stats + (size_t)rb * 2 * n + n + col) = make_float4(qx, qy, qz, qw);
            }
        }
    }
}

}  // namespace gemm

template <int BN, bool KM, int K>
static int launch_direct(dim3 grid, hipStream_t st, int m, int n, const float *X, const float *W, const float *bias, float *Y,
                         int accumulate, int ncb, const gemm::GemmMulti &gm) {
    const size_t lds = sizeof(float) * ((size_t)BN * (K + 8) + 2 * K);
    auto kern = ptv2_matmul_bf16() ? gemm::rows_gemm_direct_kernel<BN, KM, K, true> : gemm::rows_gemm_direct_kernel<BN, KM, K, false>;
    RUN(ptv2_kernel_lds((const void *)kern, lds));
    hipLaunchKernelGGL(kern, grid, dim3(gemm::THREADS), lds, st, m, n, X, W, bias, Y, accumulate, ncb, gm);
    return PTV2_OK;
}

// the direct form exists for BN = 16 / 48 and K = 48 / 96 / 192 / 384 (every Linear of the S3DIS / ScanNet configurations
// except the 512-wide ScanNet level); AO_AMD_GEMM=lds selects the LDS-staged kernel (A/B switch of the tests)
// (false: not this form; true: launched, or refused with *rc)
static bool launch_gemm_direct(int bn, bool kmajor, dim3 grid, hipStream_t st, int m, int n, int k, const float *X, const float *W,
                               const float *bias, float *Y, int accumulate, int ncb, const gemm::GemmMulti &gm, int *rc) {
    const char *e = getenv("AO_AMD_GEMM");
    if ((e && e[0] == 'l') || (bn != 16 && bn != 48) || (k != 48 && k != 96 && k != 192 && k != 384)) return false;
    // Where it pays (per (kernel, grid) durations of one step, profiles/r03_*): k = 48 -- the full-resolution level, thousands
    // of short workgroups whose phases interleave (fc1 / fc3 18.9 -> 17.3 us, q/k/v 48 -> 39 us, input gradients 21.7 -> 19.7)
    // -- and the 48-column blocks of the q/k/v launch at the deeper levels (26.6 -> 22.6 us at 4.5 k x 192).  The few hundred
    // workgroups of a deep-level launch are all resident at once and run their load and compute phases in lockstep, where
    // the chunked loop's prefetch under the MFMAs wins (14.7 vs 20.2 us for the 3-pair input gradient at 4.5 k x 192):
    // those stay on the LDS-staged kernel.  AO_AMD_GEMM=direct forces the direct form wherever it exists (tests).
    if (!(e && e[0] == 'd') && !(k == 48 || (!kmajor && bn == 48 && k <= 192))) return false;
#define GD(BN, KM, KK) *rc = launch_direct<BN, KM, KK>(grid, st, m, n, X, W, bias, Y, accumulate, ncb, gm)
#define GDK(BN, KM)                                                                   \
    switch (k) { case 48: GD(BN, KM, 48); break; case 96: GD(BN, KM, 96); break; case 192: GD(BN, KM, 192); break; default: GD(BN, KM, 384); break; }
    if (bn == 16) { if (kmajor) { GDK(16, true) } else { GDK(16, false) } }
    else { if (kmajor) { GDK(48, true) } else { GDK(48, false) } }
#undef GDK
#undef GD
    return true;
}

template <int BN, bool KM, int KC>
static void launch_one(dim3 grid, hipStream_t st, int m, int n, int k, const float *X, const float *W, const float *bias, float *Y,
                       int accumulate, int ncb, const gemm::GemmMulti &gm) {
    if (ptv2_matmul_bf16())
        hipLaunchKernelGGL((gemm::rows_gemm_kernel<BN, KM, KC, true>), grid, dim3(gemm::THREADS), 0, st, m, n, k, X, W, bias, Y,
                           accumulate, ncb, gm);
    else
        hipLaunchKernelGGL((gemm::rows_gemm_kernel<BN, KM, KC, false>), grid, dim3(gemm::THREADS), 0, st, m, n, k, X, W, bias, Y,
                           accumulate, ncb, gm);
}

// Column-block width.  48 (or 64) columns per workgroup read X once per 48 outputs -- right when X is large.  At the deep
// levels (m ~ 1 000 - 5 000 rows) that makes 136 - 284 workgroups for 256 compute units: one and a bit rounds of a
// latency-bound workgroup (e.g. 284 = 256 + 28: the launch takes two workgroup lifetimes for 1.1 rounds of work).  There
// 16-column blocks give 3 x the workgroups (X, a few MB, is re-read from L2) and the rounds even out.
// `products`: independent products in the launch (blockIdx.y: the q / k / v projections run 3) -- they multiply the
// workgroup count, so the wide block stays affordable there (4.5 k points x 192: 852 workgroups of 48 columns instead of
// 2 556 of 16, each re-reading the X tile a third as often)
static int column_block(int m, int n, int products = 1) {
    const bool n48 = n % 48 == 0;
    const int wide = n48 ? 48 : 64;
    const long long rbs = ((long long)m + gemm::BM - 1) / gemm::BM, prod = products;
    const long long wgs = rbs * ((n + wide - 1) / wide) * prod;
    constexpr int wide_min = 768;
    if (wgs >= wide_min || n % 16 != 0) return wide;
    // in between: 32-column blocks when they still give a workgroup per compute unit -- every column block re-reads the X tile
    // from L2, 12 x with 16 columns at n = 192.  Measured at 120 k points (alternating runs on one box): 11.08 ms without
    // the 32-column form, 11.02 with the threshold at 512 workgroups, 10.98 at 256, 10.99 at 128
    constexpr int mid = 256;
    if (n % 32 == 0 && rbs * (n / 32) * prod >= mid) return 32;
    return 16;
}

// ---- k-split form (deep levels) ------------------------------------------------------------------------------------------
namespace {
thread_local int g_rb16_ok = 0;  // the caller understands records of 16 rows (block.hip sets it around its launches)
}
void ptv2_gemm_allow_rb16(int on) { g_rb16_ok = on; }
static bool ksplit_ok(int m, int n, int k, bool has_records) {
    // measured and rejected as the default (round 6, profiles/r06_rejected/gemm_ksplit.md): 7x the workgroups of the 64-row form
    // but 16-20 us per launch against 11-14 (4x the weight reads per row, an LDS reduce and a barrier per workgroup), +0.45 ms a
    // step.  AO_AMD_GEMM_KSPLIT=1 turns it on for A/B runs and keeps it under test.
    static const bool on = ptv2_env_is("AO_AMD_GEMM_KSPLIT", '1');
    // (AO_AMD_GEMM = lds / direct: the A/B switches of the older forms)
    if (!on || ptv2_env_set("AO_AMD_GEMM") || ptv2_matmul_bf16()) return false;
    if (has_records && !g_rb16_ok) return false;  // (the public launchers' records are per 64 rows: include/ptv2_hip.h)
    return m >= 1 && m <= 32768 && (k == 96 || k == 192 || k == 384) && n % 16 == 0 && n >= 16;
}
// rows per statistics / reduce record the fused launchers below will write for this shape (16: the k-split kernel; else 64)
int rows_gemm_record_rows(int m, int n, int k) { return ksplit_ok(m, n, k, true) ? 16 : 64; }

template <int BN, bool KM>
static void launch_ksplit_k(int k, dim3 grid, hipStream_t st, int m, int n, const float *X, const float *W, const float *bias, float *Y,
                            int accumulate, int ncb, const gemm::GemmMulti &gm) {
    switch (k) {
        case 96: hipLaunchKernelGGL((gemm::rows_gemm_ksplit_kernel<BN, KM, 96>), grid, dim3(gemm::THREADS), 0, st, m, n, X, W, bias, Y, accumulate, ncb, gm); break;
        case 192: hipLaunchKernelGGL((gemm::rows_gemm_ksplit_kernel<BN, KM, 192>), grid, dim3(gemm::THREADS), 0, st, m, n, X, W, bias, Y, accumulate, ncb, gm); break;
        default: hipLaunchKernelGGL((gemm::rows_gemm_ksplit_kernel<BN, KM, 384>), grid, dim3(gemm::THREADS), 0, st, m, n, X, W, bias, Y, accumulate, ncb, gm); break;
    }
}
// launches the k-split kernel when it applies; `products`: grid.y (independent products)
static bool try_ksplit(int m, int n, int k, bool kmajor, int products, hipStream_t st, const float *X, const float *W, const float *bias,
                       float *Y, int accumulate, const gemm::GemmMulti &gm, bool has_records) {
    if (!ksplit_ok(m, n, k, has_records)) return false;
    const int bn = n % 48 == 0 ? 48 : (n % 64 == 0 ? 64 : (n % 32 == 0 ? 32 : 16));
    const int ncb = n / bn;
    const long long wgs = (((long long)m + 15) / 16) * ncb;
    if (wgs > 2147483647LL) return false;
    const dim3 grid((unsigned)wgs, (unsigned)products);
#define KS(BNN) do { if (kmajor) launch_ksplit_k<BNN, true>(k, grid, st, m, n, X, W, bias, Y, accumulate, ncb, gm); \
                     else launch_ksplit_k<BNN, false>(k, grid, st, m, n, X, W, bias, Y, accumulate, ncb, gm); } while (0)
    if (bn == 48) KS(48); else if (bn == 64) KS(64); else if (bn == 32) KS(32); else KS(16);
#undef KS
    return true;
}

static int launch_gemm(int bn, bool kmajor, bool wide_k, dim3 grid, hipStream_t st, int m, int n, int k, const float *X,
                       const float *W, const float *bias, float *Y, int accumulate, int ncb, const gemm::GemmMulti &gm) {
    int rc = PTV2_OK;
    if (launch_gemm_direct(bn, kmajor, grid, st, m, n, k, X, W, bias, Y, accumulate, ncb, gm, &rc)) return rc;
#define GO(BN, KM, KC) launch_one<BN, KM, KC>(grid, st, m, n, k, X, W, bias, Y, accumulate, ncb, gm)
    if (bn == 16) {
        if (kmajor) { if (wide_k) GO(16, true, 64); else GO(16, true, 32); }
        else { if (wide_k) GO(16, false, 64); else GO(16, false, 32); }
    } else if (bn == 32) {
        if (kmajor) { if (wide_k) GO(32, true, 64); else GO(32, true, 32); }
        else { if (wide_k) GO(32, false, 64); else GO(32, false, 32); }
    } else if (bn == 48) {
        if (kmajor) { if (wide_k) GO(48, true, 64); else GO(48, true, 32); }
        else { if (wide_k) GO(48, false, 64); else GO(48, false, 32); }
    } else {
        if (kmajor) { if (wide_k) GO(64, true, 64); else GO(64, true, 32); }
        else { if (wide_k) GO(64, false, 64); else GO(64, false, 32); }
    }
#undef GO
    return PTV2_OK;
}

// Y (m,n) [+]= X (m,k) op(W) + bias.  w_kmajor == 0: W is (n,k) row-major (y = x W^T, nn.Linear forward);
// w_kmajor != 0: W is (k,n) row-major (gx = gy W).  n % 4 == 0, k % 4 == 0; bias may be NULL.
extern "C" int rows_gemm_hip_launcher(int m, int n, int k, const float *X, const float *W, int w_kmajor,
                                      const float *bias, float *Y, int accumulate, void *stream) {
    using namespace gemm;
    if (m < 0 || n < 4 || k < 4 || n % 4 != 0 || k % 4 != 0 || !X || !W || !Y) return PTV2_ERR_ARG;
    if (m == 0) return PTV2_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool n48 = n % 48 == 0;  // 48 / 96 / 192 / 384: column blocks of 48 waste nothing
    const int bn = column_block(m, n);
    const int ncb = (n + bn - 1) / bn;
    const long long nrb = ((long long)m + BM - 1) / BM;
    if (nrb * ncb > 2147483647LL) return PTV2_ERR_ARG;
    const dim3 grid((unsigned)(nrb * ncb));
    {
        PtvScopedTimer t(KID_ROWS_GEMM + (n48 ? 0 : 4) + (w_kmajor ? 2 : 0) + (k >= 192 ? 1 : 0), st,
                         4.0 * ((double)m * (n + k) + (double)n * k));
        if (!try_ksplit(m, n, k, w_kmajor != 0, 1, st, X, W, bias, Y, accumulate, GemmMulti{}, false))
            RUN(launch_gemm(bn, w_kmajor != 0, k >= 192, grid, st, m, n, k, X, W, bias, Y, accumulate, ncb, GemmMulti{}));
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// count (<= 3) products of one shape in one launch.  sum == 0: Y[i] = X[i] op(W[i]) + bias[i] (independent outputs);
// sum != 0: Y[0] (+)= sum_i X[i] op(W[i]) (+ bias[0]).
// as rows_gemm_multi, with BatchNorm fused on either side: xsc / xsh (k) != NULL: the X operand is ReLU(x * xsc + xsh);
// stats != NULL: stats[i] != NULL receives the per-row-block column statistics of Y[i] (ceil(m / 64) records of
// [2][n] floats: sum, centred sum of squares), to be merged by bn_tiles_finalize_hip_launcher
extern "C" int rows_gemm_fused_hip_launcher(int m, int n, int k, int count, int sum, const float *const *X,
                                            const float *const *W, int w_kmajor, const float *const *bias, float *const *Y,
                                            int accumulate, const float *xsc, const float *xsh, float *const *stats,
                                            void *stream) {
    using namespace gemm;
    if (m < 0 || n < 4 || k < 4 || n % 4 != 0 || k % 4 != 0 || count < 1 || count > 3 || !X || !W || !Y) return PTV2_ERR_ARG;
    if (m == 0) return PTV2_OK;
    GemmMulti gm{};
    gm.count = count;
    gm.sum = sum ? 1 : 0;
    for (int i = 0; i < count; ++i) {
        if (!X[i] || !W[i] || (!Y[i] && (i == 0 || !sum))) return PTV2_ERR_ARG;
        gm.X[i] = X[i]; gm.W[i] = W[i]; gm.bias[i] = bias ? bias[i] : nullptr; gm.Y[i] = Y[i];
        gm.stats[i] = stats ? stats[i] : nullptr;
    }
    if ((xsc == nullptr) != (xsh == nullptr)) return PTV2_ERR_ARG;
    gm.xsc = xsc;
    gm.xsh = xsh;
    hipStream_t st = (hipStream_t)stream;
    const bool n48 = n % 48 == 0;
    const int bn = column_block(m, n, sum ? 1 : count);
    const int ncb = (n + bn - 1) / bn;
    const long long nrb = ((long long)m + BM - 1) / BM;
    if (nrb * ncb > 2147483647LL) return PTV2_ERR_ARG;
    const dim3 grid((unsigned)(nrb * ncb), sum ? 1 : count);
    const float *b0 = sum ? gm.bias[0] : nullptr;
    {
        PtvScopedTimer t(KID_ROWS_GEMM + (n48 ? 0 : 4) + (w_kmajor ? 2 : 0) + (k >= 192 ? 1 : 0), st,
                         4.0 * count * ((double)m * (n + k) + (double)n * k));
        bool records = false;
        for (int i = 0; i < count; ++i) records = records || gm.stats[i] != nullptr;
        if (!try_ksplit(m, n, k, w_kmajor != 0, sum ? 1 : count, st, gm.X[0], gm.W[0], b0, gm.Y[0], accumulate, gm, records))
            RUN(launch_gemm(bn, w_kmajor != 0, k >= 192, grid, st, m, n, k, gm.X[0], gm.W[0], b0, gm.Y[0], accumulate, ncb, gm));
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int rows_gemm_multi_hip_launcher(int m, int n, int k, int count, int sum, const float *const *X,
                                            const float *const *W, int w_kmajor, const float *const *bias, float *const *Y,
                                            int accumulate, void *stream) {
    return rows_gemm_fused_hip_launcher(m, n, k, count, sum, X, W, w_kmajor, bias, Y, accumulate, nullptr, nullptr, nullptr,
                                        stream);
}

// rows_gemm_multi (sum or single) whose output Y[0] is the gradient entering a BatchNorm (+ ReLU) with input bn_x: also
// leaves that BatchNorm's backward-reduce records (ceil(m / 64) records of [2][n]: sum g', sum g' xhat) in `records`,
// to be finished by bn_backward_records_hip_launcher
extern "C" int rows_gemm_bnbwd_hip_launcher(int m, int n, int k, int count, const float *const *X, const float *const *W,
                                            int w_kmajor, float *Y, const float *bn_x, const float *bn_mean, const float *bn_rstd,
                                            const float *bn_gamma, const float *bn_beta, int relu, float *records, void *stream) {
    using namespace gemm;
    if (m < 0 || n < 4 || k < 4 || n % 4 != 0 || k % 4 != 0 || count < 1 || count > 3 || !X || !W || !Y) return PTV2_ERR_ARG;
    if (!bn_x || !bn_mean || !bn_rstd || !records || (relu && (!bn_gamma || !bn_beta))) return PTV2_ERR_ARG;
    if (m == 0) return PTV2_OK;
    GemmMulti gm{};
    gm.count = count;
    gm.sum = 1;
    for (int i = 0; i < count; ++i) {
        if (!X[i] || !W[i]) return PTV2_ERR_ARG;
        gm.X[i] = X[i]; gm.W[i] = W[i];
    }
    gm.Y[0] = Y;
    gm.bnx = bn_x; gm.bnm = bn_mean; gm.bnr = bn_rstd; gm.bng = bn_gamma; gm.bnb = bn_beta; gm.bnrelu = relu; gm.brec = records;
    hipStream_t st = (hipStream_t)stream;
    const bool n48 = n % 48 == 0;
    const int bn = column_block(m, n);
    const int ncb = (n + bn - 1) / bn;
    const long long nrb = ((long long)m + BM - 1) / BM;
    if (nrb * ncb > 2147483647LL) return PTV2_ERR_ARG;
    const dim3 grid((unsigned)(nrb * ncb), 1);
    {
        PtvScopedTimer t(KID_ROWS_GEMM + (n48 ? 0 : 4) + (w_kmajor ? 2 : 0) + (k >= 192 ? 1 : 0), st,
                         4.0 * ((double)m * (2 * n + count * k) + (double)count * n * k));
        if (!try_ksplit(m, n, k, w_kmajor != 0, 1, st, gm.X[0], gm.W[0], nullptr, Y, 0, gm, true))
            RUN(launch_gemm(bn, w_kmajor != 0, k >= 192, grid, st, m, n, k, gm.X[0], gm.W[0], nullptr, Y, 0, ncb, gm));
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
