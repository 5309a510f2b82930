// ao_amd/csrc/wgrad.hip -- the weight gradient of nn.Linear, dW = dY^T X (the bias gradient falls out of the same pass), as a
// split-K reduction over row chunks on gfx950: the direct and the LDS-staged MFMA forms (one product, a strided batch, up to six
// products of one shape, row-scaled bias sums) and the grouped projection's form on the vector ALUs.  Every entry point
// describes its call ONCE, as a WgradJob (wgrad_job.h) inside a WgradCall (plan_*), and hands it to wgrad_submit, which either
// launches it at once with its finalize -- the kernel takes the job by value -- or, inside a model backward, files it (WgradDefer,
// ptv2_wgrad_defer_*): the filed jobs of a backward are run at its end by one launch per kernel form through a job table.  The
// recompute form of gva_wgrad_tile.hip is planned there and submitted here too.
//
// Why these exist.  The weight gradients have a 48x48 .. 384x384 output with K = N up to 1.2e5, for which the BLAS picks a
// 9-workgroup kernel (353 us per call); this is a pure HBM streaming problem: each workgroup owns a 48x48 output tile for a
// chunk of rows (3x3 register patch per lane), partial tiles summed in fixed order.
#include <vector>

#include "dense_common.h"
#include "wgrad_job.h"

namespace dense {

// --------------------------------------------------------------- Linear wgrad --
// dW[b][o][i] = sum_n gY[n*ldy + b*sy + o] * X[n*ldx + b*sx + i];  db[b][o] = sum_n gY[...]   (b < batch)
// fp32 MFMA 16x16x4 (exact f32 FMA chain): the reduction index n is the MFMA k; both operand fragments are
// read straight from global memory -- lane l of a fragment holds element [row0 + (l>>4)][col0 + (l&15)],
// i.e. four 64-byte row segments per load, no LDS staging.  A workgroup = 4 waves = one (up to) 48x48
// output tile for one chunk of rows; the waves interleave k-steps and are summed through LDS.
constexpr int WG_MT = 3, WG_TILE = 16 * WG_MT, WG_CHUNK = 256, WG_CHUNK_MIN = 128;

// BF16: the U = 8 k-steps of a trip (8 rows per lane and fragment) are exactly the 8-per-lane operand of
// V_MFMA_F32_16X16X32_BF16: 8 fp32 MFMAs per tile pair become one instruction on bf16-rounded operands.
// (a function of the workgroup's coordinates, like wgrad_lds_tile below: the per-call kernel and the batched kernel share it)
template <bool BF16>
__device__ __forceinline__ void wgrad_direct_tile(const int n, const int cout, const int cin, const int tiles_i,
                                                  const float *__restrict__ A, const long long ldy,
                                                  const float *__restrict__ B, const long long ldx, float *__restrict__ part,
                                                  const bool part_b, const int batch, const float *__restrict__ xs,
                                                  const float *__restrict__ xh, const int chunk, const int bx, const int by,
                                                  const int bz) {
    __shared__ float sRed[TPB / WAVE][WG_MT * WG_MT * 4 + WG_MT][WAVE + 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int to = (by / tiles_i) * WG_TILE, ti = (by % tiles_i) * WG_TILE;
    const long long r0 = (long long)bx * chunk;
    const long long r1 = (r0 + chunk) < (long long)n ? (r0 + chunk) : (long long)n;
    const int lr = lane >> 4, lc = lane & 15;
    v4f acc[WG_MT][WG_MT];
    float bsum[WG_MT];
#pragma unroll
    for (int m = 0; m < WG_MT; ++m) {
        bsum[m] = 0.f;
#pragma unroll
        for (int t = 0; t < WG_MT; ++t) acc[m][t] = (v4f){0.f, 0.f, 0.f, 0.f};
    }
    // (measured and rejected, round 3: columns 3 lc + m per lane so that a lane's three operand values of a k-step are ONE
    // 12-byte load and a row is read as 192 contiguous bytes -- 16 instead of 48 vector-memory instructions per trip: slower at
    // every shape, 34 -> 38 us at 4.5 k x 192 x 5 products, 58 -> 71 us at 120 k x 48 x 5; three 64-byte segments stay)
    bool mo[WG_MT], mi[WG_MT];
    float xsc_[WG_MT], xsh_[WG_MT];
#pragma unroll
    for (int m = 0; m < WG_MT; ++m) {
        mo[m] = to + m * 16 + lc < cout;
        mi[m] = ti + m * 16 + lc < cin;
        xsc_[m] = (xs && mi[m]) ? xs[ti + m * 16 + lc] : 1.f;
        xsh_[m] = (xs && mi[m]) ? xh[ti + m * 16 + lc] : 0.f;
    }
    // U k-steps per trip: all 6 U fragment loads are issued before the first MFMA consumes one (a step-by-step loop
    // paid one memory latency per 4 rows: 2.5 us per 100 rows of chunk, independent of the problem size)
    constexpr int U = 8;
    for (long long rb = r0 + 4 * wid; rb < r1; rb += 4 * (TPB / WAVE) * U) {
        float a[U][WG_MT], b[U][WG_MT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long row = rb + (long long)u * 4 * (TPB / WAVE) + lr;
            const bool rok = row < r1;
#pragma unroll
            for (int m = 0; m < WG_MT; ++m) {
                a[u][m] = (rok && mo[m]) ? A[row * ldy + to + m * 16 + lc] : 0.f;
                b[u][m] = (rok && mi[m]) ? B[row * ldx + ti + m * 16 + lc] : 0.f;
            }
        }
        if (xs) {  // fused BatchNorm + ReLU on the X operand; rows past the end meet a == 0, so no masking is needed
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int m = 0; m < WG_MT; ++m) b[u][m] = fmaxf(__builtin_fmaf(b[u][m], xsc_[m], xsh_[m]), 0.f);
        }
        if constexpr (BF16) {
            ptv2_bf16x8 ab[WG_MT], bb[WG_MT];
#pragma unroll
            for (int m = 0; m < WG_MT; ++m) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bsum[m] += a[u][m];
                    ab[m][u] = (__bf16)a[u][m];
                    bb[m][u] = (__bf16)b[u][m];
                }
            }
#pragma unroll
            for (int m = 0; m < WG_MT; ++m)
#pragma unroll
                for (int t = 0; t < WG_MT; ++t)
                    acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ab[m], bb[t], acc[m][t], 0, 0, 0);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int m = 0; m < WG_MT; ++m) {
                    bsum[m] += a[u][m];
#pragma unroll
                    for (int t = 0; t < WG_MT; ++t)
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][m], b[u][t], acc[m][t], 0, 0, 0);
                }
        }
    }
    // combine the 4 waves (fixed order) and write the partial tile
#pragma unroll
    for (int m = 0; m < WG_MT; ++m) {
        float bs = bsum[m];
        bs += __shfl_xor(bs, 16, WAVE);
        bs += __shfl_xor(bs, 32, WAVE);
        sRed[wid][WG_MT * WG_MT * 4 + m][lane] = bs;
#pragma unroll
        for (int t = 0; t < WG_MT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) sRed[wid][(m * WG_MT + t) * 4 + r][lane] = acc[m][t][r];
    }
    __syncthreads();
    const size_t rec = (size_t)batch * cout * cin + (part_b ? (size_t)batch * cout : 0);
    float *p = part + (size_t)bx * rec + (size_t)bz * cout * cin;
    for (int e = threadIdx.x; e < WG_MT * WG_MT * 4 * WAVE; e += TPB) {
        const int q = e / WAVE, l = e - q * WAVE;
        const int mt = q / 4, r = q - mt * 4, m = mt / WG_MT, t = mt - m * WG_MT;
        const int o = to + m * 16 + (l >> 4) * 4 + r, i = ti + t * 16 + (l & 15);  // D: row=(lane>>4)*4+reg, col=lane&15
        if (o < cout && i < cin) {
            float v = 0.f;
#pragma unroll
            for (int wv = 0; wv < TPB / WAVE; ++wv) v += sRed[wv][q][l];
            p[(size_t)o * cin + i] = v;
        }
    }
    if (part_b && ti == 0 && threadIdx.x < WG_TILE) {
        const int m = threadIdx.x >> 4, l = threadIdx.x & 15, o = to + threadIdx.x;
        if (o < cout) {
            float v = 0.f;
#pragma unroll
            for (int wv = 0; wv < TPB / WAVE; ++wv) v += sRed[wv][WG_MT * WG_MT * 4 + m][l];
            part[(size_t)bx * rec + (size_t)batch * cout * cin + (size_t)bz * cout + o] = v;
        }
    }
}

// job + workgroup coordinates (bx: row chunk, by: output tile, bz: product) -> the tile; count > 0: the multi form, an operand
// pair per product (several independent products of one shape in one launch), else the strided form (gY + bz * sy, X + bz * sx)
template <bool BF16>
__device__ __forceinline__ void wgrad_direct_job(const WgradJob &J, const int bx, const int by, const int bz) {
    const bool multi = J.count > 0;
    wgrad_direct_tile<BF16>(J.n, J.cout, J.cin, J.tiles_i, multi ? J.mgY[bz] : J.gY + (long long)bz * J.sy, J.ldy,
                            multi ? J.mX[bz] : J.X + (long long)bz * J.sx, J.ldx, J.part, J.has_pb != 0, J.batch,
                            multi ? J.mxsc[bz] : nullptr, multi ? J.mxsh[bz] : nullptr, J.chunk, bx, by, bz);
}
// one call: the job by value, grid (chunks, tiles, products)
template <bool BF16>
__global__ __launch_bounds__(TPB) void linear_wgrad_kernel(WgradJob J) {
    wgrad_direct_job<BF16>(J, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

// ---- the same reduction with the operands staged through LDS (fp32 matrix cores) ---------------------------------------
// linear_wgrad_kernel reads its MFMA fragments straight from global memory: 48 four-byte loads per lane and trip (four
// 64-byte row segments per instruction), 72 MFMAs behind them; its waves sat in issue stalls for 60 % of their cycles with
// the matrix pipe 23 % busy (profiles/r02_final_sq_counters.jsonl).  Here a workgroup streams 64-row stages of both operand
// tiles (64 x 48 floats each) with 16-byte loads, every row a contiguous 192-byte run, into a double-buffered LDS image
// (row pitch 48 floats: the ds_read_b32 fragment reads of lanes (k = lane >> 4, column = lane & 15) fall on 32 distinct
// banks per half-wave); the next stage's loads are in flight in registers while the current one is on the matrix cores;
// each wavefront contracts 16 of the stage's 64 rows (4 k-steps x 9 tiles) and the four partial tiles are added through LDS
// at the end, exactly as in linear_wgrad_kernel (same records, same finalize).  The contraction order over the rows differs
// from that kernel's (wave w takes rows 16 w .. 16 w + 15 of every stage); results are bitwise reproducible run to run.
constexpr int WL_ROWS = 64;  // rows per stage
// RS != 0: the bias sums are WEIGHTED by a per-(row, product) scalar: db[b][o] = sum_n gY[n, b, o] * rowscale[n * lds_s + b]
// (the grouped projection's bias gradient, sum_n g_out[n, ch] sw[n, group(ch)], which was a kernel of its own per Block)
// (the body is a function of the workgroup's coordinates (bx: row chunk, by: output tile, bz: product) so that the same code
// serves the one-launch-per-call kernel below and the batched kernel that runs the deferred launches of a whole backward)
template <int RS>
__device__ __forceinline__ void wgrad_lds_tile(const int n, const int cout, const int cin, const int tiles_i,
                                               const float *__restrict__ A, const long long ldy,
                                               const float *__restrict__ B, const long long ldx,
                                               float *__restrict__ part, const bool part_b, const int batch,
                                               const float *__restrict__ xs, const float *__restrict__ xh, const int chunk,
                                               const float *__restrict__ rowscale, const long long lds_s, const int bx,
                                               const int by, const int bz) {
    extern __shared__ float4 wl_lds4[];
    float *sA = (float *)wl_lds4;                    // [2][WL_ROWS][WG_TILE]
    float *sB = sA + 2 * WL_ROWS * WG_TILE;           // [2][WL_ROWS][WG_TILE]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int to = (by / tiles_i) * WG_TILE, ti = (by % tiles_i) * WG_TILE;
    const long long r0 = (long long)bx * chunk;
    const long long r1 = (r0 + chunk) < (long long)n ? (r0 + chunk) : (long long)n;
    const int lr = lane >> 4, lc = lane & 15;
    v4f acc[WG_MT][WG_MT];
    float bsum[WG_MT];
#pragma unroll
    for (int m = 0; m < WG_MT; ++m) {
        bsum[m] = 0.f;
#pragma unroll
        for (int t = 0; t < WG_MT; ++t) acc[m][t] = (v4f){0.f, 0.f, 0.f, 0.f};
    }
    float xsc_[WG_MT], xsh_[WG_MT];
#pragma unroll
    for (int m = 0; m < WG_MT; ++m) {
        const bool mi = ti + m * 16 + lc < cin;
        xsc_[m] = (xs && mi) ? xs[ti + m * 16 + lc] : 1.f;
        xsh_[m] = (xs && mi) ? xh[ti + m * 16 + lc] : 0.f;
    }
    // loader: thread -> float4 slots f = tid + 256 j (j < 3) of a 64 x 12 stage tile, for both operands
    constexpr int Q = WG_TILE / 4, SLOTS = WL_ROWS * Q / TPB;  // 12 float4 per row, 3 slots per thread
    float4 ra[SLOTS], rb[SLOTS];
    // (cout and cin are multiples of 4 here -- wgrad_lds_ok: a 16-byte piece is inside the tile or outside it -- and every load
    // is unconditional: rows past the chunk / pieces past the edge read the zero pad of common.h)
    float sn[4], sc_[4];  // (RS) row scalars of the stage in flight / of the stage on the matrix cores: rows 16 wid + 4 ks + lr
    auto fetch = [&](long long rs) {
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int f = tid + TPB * j, row = f / Q, c4 = (f - row * Q) * 4;
            const long long r = rs + row;
            ra[j] = ptv2_ld_or_zero((const float4 *)(A + r * ldy + to + c4), r < r1 && to + c4 < cout);
            rb[j] = ptv2_ld_or_zero((const float4 *)(B + r * ldx + ti + c4), r < r1 && ti + c4 < cin);
        }
        if constexpr (RS != 0) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const long long r = rs + wid * 16 + ks * 4 + lr;
                sn[ks] = ptv2_ld_or_zero(rowscale + r * lds_s + bz, r < r1);
            }
        }
    };
    auto stash = [&](int buf) {
        if constexpr (RS != 0) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) sc_[ks] = sn[ks];
        }
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int f = tid + TPB * j;  // (row * Q + c4 / 4) * 4 floats = row * WG_TILE + c4: the image is the tile, row-major
            *(float4 *)(sA + (size_t)buf * WL_ROWS * WG_TILE + 4 * f) = ra[j];
            *(float4 *)(sB + (size_t)buf * WL_ROWS * WG_TILE + 4 * f) = rb[j];
        }
    };
    fetch(r0);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (long long rs = r0; rs < r1; rs += WL_ROWS, buf ^= 1) {
        const bool more = rs + WL_ROWS < r1;
        if (more) fetch(rs + WL_ROWS);
        const float *pa = sA + (size_t)buf * WL_ROWS * WG_TILE + (size_t)(wid * 16 + lr) * WG_TILE + lc;
        const float *pb = sB + (size_t)buf * WL_ROWS * WG_TILE + (size_t)(wid * 16 + lr) * WG_TILE + lc;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {  // rows 16 wid + 4 ks + lr of the stage
            float a[WG_MT], b[WG_MT];
#pragma unroll
            for (int m = 0; m < WG_MT; ++m) {
                a[m] = pa[ks * 4 * WG_TILE + m * 16];
                b[m] = pb[ks * 4 * WG_TILE + m * 16];
            }
            if (xs) {  // fused BatchNorm + ReLU on the X operand; rows past the end meet a == 0
#pragma unroll
                for (int m = 0; m < WG_MT; ++m) b[m] = fmaxf(__builtin_fmaf(b[m], xsc_[m], xsh_[m]), 0.f);
            }
#pragma unroll
            for (int m = 0; m < WG_MT; ++m) {
                if constexpr (RS != 0) bsum[m] = __builtin_fmaf(a[m], sc_[ks], bsum[m]);
                else bsum[m] += a[m];
#pragma unroll
                for (int t = 0; t < WG_MT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[t], acc[m][t], 0, 0, 0);
            }
        }
        if (more) {
            stash(buf ^ 1);  // (the other buffer's readers finished before the barrier that ended the previous trip)
            __syncthreads();
        }
    }
    // combine the 4 waves (fixed order) and write the partial tile: as linear_wgrad_kernel (the stage buffers are dead)
    __syncthreads();
    float(*sRed)[WG_MT * WG_MT * 4 + WG_MT][WAVE + 1] = (float(*)[WG_MT * WG_MT * 4 + WG_MT][WAVE + 1]) wl_lds4;
#pragma unroll
    for (int m = 0; m < WG_MT; ++m) {
        float bs = bsum[m];
        bs += __shfl_xor(bs, 16, WAVE);
        bs += __shfl_xor(bs, 32, WAVE);
        sRed[wid][WG_MT * WG_MT * 4 + m][lane] = bs;
#pragma unroll
        for (int t = 0; t < WG_MT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) sRed[wid][(m * WG_MT + t) * 4 + r][lane] = acc[m][t][r];
    }
    __syncthreads();
    const size_t rec = (size_t)batch * cout * cin + (part_b ? (size_t)batch * cout : 0);
    float *p = part + (size_t)bx * rec + (size_t)bz * cout * cin;
    for (int e = threadIdx.x; e < WG_MT * WG_MT * 4 * WAVE; e += TPB) {
        const int q = e / WAVE, l = e - q * WAVE;
        const int mt = q / 4, r = q - mt * 4, m = mt / WG_MT, t = mt - m * WG_MT;
        const int o = to + m * 16 + (l >> 4) * 4 + r, i = ti + t * 16 + (l & 15);  // D: row=(lane>>4)*4+reg, col=lane&15
        if (o < cout && i < cin) {
            float v = 0.f;
#pragma unroll
            for (int wv = 0; wv < TPB / WAVE; ++wv) v += sRed[wv][q][l];
            p[(size_t)o * cin + i] = v;
        }
    }
    if (part_b && ti == 0 && threadIdx.x < WG_TILE) {
        const int m = threadIdx.x >> 4, l = threadIdx.x & 15, o = to + threadIdx.x;
        if (o < cout) {
            float v = 0.f;
#pragma unroll
            for (int wv = 0; wv < TPB / WAVE; ++wv) v += sRed[wv][WG_MT * WG_MT * 4 + m][l];
            part[(size_t)bx * rec + (size_t)batch * cout * cin + (size_t)bz * cout + o] = v;
        }
    }
}

template <int RS>
__device__ __forceinline__ void wgrad_lds_job(const WgradJob &J, const int bx, const int by, const int bz) {
    const bool multi = J.count > 0;
    wgrad_lds_tile<RS>(J.n, J.cout, J.cin, J.tiles_i, multi ? J.mgY[bz] : J.gY + (long long)bz * J.sy, J.ldy,
                       multi ? J.mX[bz] : J.X + (long long)bz * J.sx, J.ldx, J.part, J.has_pb != 0, J.batch,
                       multi ? J.mxsc[bz] : nullptr, multi ? J.mxsh[bz] : nullptr, J.chunk, J.rowscale, J.lds_s, bx, by, bz);
}
template <int RS>
__global__ __launch_bounds__(TPB) void linear_wgrad_lds_kernel(WgradJob J) {
    wgrad_lds_job<RS>(J, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

// ---- the deferred launches of a whole backward in one launch ------------------------------------------------------------
// A Block's weight gradients are off its critical chain (nothing reads dW before the optimizer), and at the deep levels each
// of their launches is a handful of latency-bound workgroups: 28-38 us for 3 MB of operands, a third of it spent alone on the
// GPU.  Inside ptv2_model_backward the eligible launches (this LDS-staged kernel, fp32) are not issued where they are called:
// the call files a job -- operands, shape, its slice of a record arena -- and ONE launch at the end of the backward runs them
// all, workgroup -> (job, chunk, tile, product) through a job table in device memory, followed by ONE finalize over the
// records of all jobs.  Kernels, tile order and record layout are those of the per-call launch; a filed job's row chunks are
// longer (wg_chunk: the other jobs fill the GPU), so its sums agree with the per-call launch's to ~2e-6 of the gradient's norm.
constexpr int WGRAD_PACK = 8;  // jobs per table-writer launch (by value: the kernarg block holds 4 KB)
struct WgradJobPack { WgradJob j[WGRAD_PACK]; };
static_assert(sizeof(WgradJobPack) + 16 <= 4096, "the table writer's argument block must fit the 4 KB kernarg segment");
__global__ void wgrad_jobs_write_kernel(WgradJobPack pack, int count, WgradJob *table) {
    if ((int)threadIdx.x < count) table[threadIdx.x] = pack.j[threadIdx.x];
}

template <int RS>
__global__ __launch_bounds__(TPB) void linear_wgrad_lds_kernel_jobs(const WgradJob *__restrict__ jobs, int njobs) {
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].wg0) ++j;  // (uniform: scalar loads)
    const WgradJob &J = jobs[j];
    const int local = (int)blockIdx.x - J.wg0;
    const int rest = local / J.chunks;
    wgrad_lds_job<RS>(J, local % J.chunks, rest % J.tiles, rest / J.tiles);
}

// ---- the grouped projection's weight gradient on the vector ALUs ---------------------------------------------------------------
// dWp2[g][i][:] = sum_n g_out[n, 8 g + i] A[n, g, :] and db[g][i] = sum_n g_out[n, 8 g + i] sw[n, g] (eight output rows per group:
// c / g = 8 in every PT-v2m2 configuration).  As a strided batch of (8, c) products on the matrix cores (linear_wgrad_lds_kernel
// <1>) every workgroup streamed a 48-column piece of ONE group's rows of A -- 192 bytes every g c 4 = 18 KB -- and five sixths of
// its 48 x 48 tile were padding: 2.5 TB/s over the 1.27 GB of A a step reads.  Here a workgroup takes a row chunk and a block
// of `gw` consecutive groups, i.e. a contiguous gw c 4-byte piece of every row of A (3-4 KB), one float4 of it per thread and
// row, eight float4 accumulators per thread; the row slots of the workgroup are added through LDS in slot order and the result
// is one chunk record of the strided form's layout ([g][8][c] weights, then [g][8] bias sums): same finalize.
constexpr int GRP_I = 8;
__device__ __forceinline__ void grouped_wgrad_tile(const int n, const int c, const int g, const int gw, const int chunk,
                                                   const float *__restrict__ gY, const float *__restrict__ X,
                                                   const float *__restrict__ sw, float *__restrict__ part, const int rec,
                                                   const int bx, const int bg) {
    extern __shared__ float4 grp_lds4[];
    const int q = c >> 2, units = gw * q, R = max(1, TPB / units);
    const int tid = threadIdx.x, rs = tid / units, u = tid - rs * units;
    const bool active = rs < R;
    const int gl = u / q, qi = u - gl * q, grp = bg * gw + gl;
    const bool live = active && grp < g;
    float4 acc[GRP_I];
    float bacc[GRP_I];
#pragma unroll
    for (int i = 0; i < GRP_I; ++i) { acc[i] = make_float4(0.f, 0.f, 0.f, 0.f); bacc[i] = 0.f; }
    const long long r0 = (long long)bx * chunk, r1 = (r0 + chunk) < (long long)n ? (r0 + chunk) : (long long)n;
    if (live) {
        const float *xa = X + (size_t)grp * c + 4 * qi;  // + r * g * c
        const float *ya = gY + (size_t)grp * GRP_I;       // + r * c
        const float *sa = sw + grp;                       // + r * g
        const size_t xs = (size_t)g * c;
        constexpr int U = 4;  // rows in flight per thread
        long long r = r0 + rs;
        for (; r + (long long)(U - 1) * R < r1; r += (long long)U * R) {
            float4 a[U], y0[U], y1[U];
            float s[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const size_t rr = (size_t)(r + (long long)t * R);
                a[t] = *(const float4 *)(xa + rr * xs);
                y0[t] = *(const float4 *)(ya + rr * c);
                y1[t] = *(const float4 *)(ya + rr * c + 4);
                s[t] = qi == 0 ? sa[rr * g] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const float y[GRP_I] = {y0[t].x, y0[t].y, y0[t].z, y0[t].w, y1[t].x, y1[t].y, y1[t].z, y1[t].w};
#pragma unroll
                for (int i = 0; i < GRP_I; ++i) {
                    acc[i].x = __builtin_fmaf(y[i], a[t].x, acc[i].x); acc[i].y = __builtin_fmaf(y[i], a[t].y, acc[i].y);
                    acc[i].z = __builtin_fmaf(y[i], a[t].z, acc[i].z); acc[i].w = __builtin_fmaf(y[i], a[t].w, acc[i].w);
                    bacc[i] = __builtin_fmaf(y[i], s[t], bacc[i]);
                }
            }
        }
        for (; r < r1; r += R) {
            const size_t rr = (size_t)r;
            const float4 a = *(const float4 *)(xa + rr * xs), y0 = *(const float4 *)(ya + rr * c), y1 = *(const float4 *)(ya + rr * c + 4);
            const float sv = qi == 0 ? sa[rr * g] : 0.f;
            const float y[GRP_I] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
#pragma unroll
            for (int i = 0; i < GRP_I; ++i) {
                acc[i].x = __builtin_fmaf(y[i], a.x, acc[i].x); acc[i].y = __builtin_fmaf(y[i], a.y, acc[i].y);
                acc[i].z = __builtin_fmaf(y[i], a.z, acc[i].z); acc[i].w = __builtin_fmaf(y[i], a.w, acc[i].w);
                bacc[i] = __builtin_fmaf(y[i], sv, bacc[i]);
            }
        }
    }
    // row slots 1 .. R-1 through LDS, added to slot 0 in slot order: [slot][i][unit] float4, then [slot][i][gl] floats
    float4 *sAcc = grp_lds4;                                   // [R][GRP_I][units]
    float *sB = (float *)(sAcc + (size_t)R * GRP_I * units);   // [R][GRP_I][gw]
    if (active) {
#pragma unroll
        for (int i = 0; i < GRP_I; ++i) {
            sAcc[((size_t)rs * GRP_I + i) * units + u] = acc[i];
            if (qi == 0) sB[((size_t)rs * GRP_I + i) * gw + gl] = bacc[i];
        }
    }
    __syncthreads();
    if (rs == 0 && grp < g) {
        float *p = part + (size_t)bx * rec;
#pragma unroll
        for (int i = 0; i < GRP_I; ++i) {
            float4 v = sAcc[(size_t)i * units + u];
            for (int t = 1; t < R; ++t) {
                const float4 w = sAcc[((size_t)t * GRP_I + i) * units + u];
                v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
            }
            *(float4 *)(p + ((size_t)grp * GRP_I + i) * c + 4 * qi) = v;
            if (qi == 0) {
                float b = sB[(size_t)i * gw + gl];
                for (int t = 1; t < R; ++t) b += sB[((size_t)t * GRP_I + i) * gw + gl];
                p[(size_t)g * GRP_I * c + (size_t)grp * GRP_I + i] = b;
            }
        }
    }
}
inline size_t grouped_lds_bytes(int c, int gw) {
    const int units = gw * (c >> 2), R = std::max(1, TPB / units);
    return sizeof(float4) * (size_t)R * GRP_I * units + sizeof(float) * (size_t)R * GRP_I * gw;
}
// one call: the job by value
__global__ __launch_bounds__(TPB) void grouped_wgrad_kernel(WgradJob J) {
    const int bx = (int)blockIdx.x % J.chunks, bg = (int)blockIdx.x / J.chunks;
    grouped_wgrad_tile(J.n, J.cin, J.batch, J.gw, J.chunk, J.gY, J.X, J.rowscale, J.part, J.rec, bx, bg);
}
__global__ __launch_bounds__(TPB) void grouped_wgrad_kernel_jobs(const WgradJob *__restrict__ jobs, int njobs) {
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].wg0) ++j;
    const WgradJob &J = jobs[j];
    const int local = (int)blockIdx.x - J.wg0;
    grouped_wgrad_tile(J.n, J.cin, J.batch, J.gw, J.chunk, J.gY, J.X, J.rowscale, J.part, J.rec, local % J.chunks, local / J.chunks);
}

template <bool BF16>
__global__ __launch_bounds__(TPB) void linear_wgrad_kernel_jobs(const WgradJob *__restrict__ jobs, int njobs) {
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].wg0) ++j;
    const WgradJob &J = jobs[j];
    const int local = (int)blockIdx.x - J.wg0;
    const int rest = local / J.chunks;
    wgrad_direct_job<BF16>(J, local % J.chunks, rest % J.tiles, rest / J.tiles);
}

// the records of all jobs -> their outputs.  A job's slots are whole workgroups.  With up to 32 chunk records a thread sums one
// output element; with more (the full-resolution jobs have hundreds of records for a few thousand outputs: one thread per output
// walked them as a chain of dependent loads, 75 us per launch) the four wavefronts of a workgroup take every fourth record of the
// same 64 consecutive elements -- every load instruction reads 256 contiguous bytes of one record (16 lanes per element, each on
// a record of its own, touched 16 lines per instruction for 16 bytes of each: 43 us per launch on average) -- and their sums
// meet in LDS, added in wavefront order.  Double accumulation; written where the job's own finalize would have written it.
__global__ __launch_bounds__(256) void wgrad_jobs_finalize_kernel(const WgradJob *__restrict__ jobs, int njobs, int total) {
    __shared__ double s_sum[3][64];
    const int sidx = blockIdx.x * 256 + threadIdx.x;  // (total is a multiple of 256, and so is every job's fin0)
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x * 256 >= jobs[j + 1].fin0) ++j;  // (uniform)
    const WgradJob &J = jobs[j];
    const int lanes = J.fin_lanes, local = sidx - J.fin0;
    const int rg = lanes == 1 ? 0 : (int)threadIdx.x >> 6;
    const int col = lanes == 1 ? local : (local >> 8) * 64 + ((int)threadIdx.x & 63);
    const int nblk = J.chunks;
    const size_t len = (size_t)J.rec;
    const float *part = J.part;
    const bool ok = col < J.rec;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (ok) {
        int b = rg;
        for (; b + 3 * lanes < nblk; b += 4 * lanes) {
            a0 += (double)part[(size_t)b * len + col];
            a1 += (double)part[(size_t)(b + lanes) * len + col];
            a2 += (double)part[(size_t)(b + 2 * lanes) * len + col];
            a3 += (double)part[(size_t)(b + 3 * lanes) * len + col];
        }
        for (; b < nblk; b += lanes) a0 += (double)part[(size_t)b * len + col];
    }
    double acc = (a0 + a1) + (a2 + a3);
    if (lanes != 1) {  // (uniform over the workgroup)
        if (rg > 0) s_sum[rg - 1][threadIdx.x & 63] = acc;
        __syncthreads();
        if (rg > 0) return;
        acc = (acc + s_sum[0][threadIdx.x]) + (s_sum[1][threadIdx.x] + s_sum[2][threadIdx.x]);
    }
    if (!ok) return;
    const float v = (float)acc;
    const int wlen = J.cout * J.cin, wtot = J.batch * wlen;
    if (J.count > 0) {  // MapWgradMulti
        if (col < wtot) {
            const int p = col / wlen;
            J.mdW[p][col - p * wlen] = v;
        } else {
            const int r = col - wtot, p = r / J.cout;
            if (J.mdb[p]) J.mdb[p][r - p * J.cout] = v;
        }
    } else if (col < wtot) {
        J.dW[col] = v;
    } else if (J.db) {
        J.db[col - wtot] = v;
    }
}

// operands 16-byte aligned with row strides that keep them so: the LDS-staged form applies (fp32 products only)
static bool wgrad_lds_ok(const void *a, long long ldy, long long sy, const void *b, long long ldx, long long sx) {
    return ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0) && ldy % 4 == 0 && ldx % 4 == 0 && sy % 4 == 0 && sx % 4 == 0;
}
static bool wgrad_lds_shape_ok(int cout, int cin) { return cout % 4 == 0 && cin % 4 == 0; }
constexpr size_t WL_LDS_BYTES = sizeof(float) * std::max<size_t>(4 * (size_t)WL_ROWS * WG_TILE,
                                                                 (size_t)(TPB / WAVE) * (WG_MT * WG_MT * 4 + WG_MT) * (WAVE + 1));

}  // namespace dense

using namespace dense;

extern "C" size_t dense_workspace_bytes(int n, int cout, int cin) {  // cout*cin = total outputs over all batches
    const size_t chunks = (size_t)(n + WG_CHUNK_MIN - 1) / WG_CHUNK_MIN + 1;
    const size_t wg = sizeof(float) * chunks * ((size_t)cout * cin + cout);
    const size_t bn = sizeof(float) * (size_t)MAX_BLK * 2 * (size_t)std::max(cout, cin);
    return ptv2_align256(std::max(wg, bn)) + 1024;
}

// rows per split-K workgroup of the weight gradient
// `tiles` = output tiles x products of the launch.  A workgroup costs ~10 us of fixed work (operand latency, the
// 40 KB cross-wave reduction, its partial record) however few rows it sums, and three fit a compute unit: at the deep
// levels (n ~ 4 500, 80 tile-products) 256-row chunks made 1 440 workgroups = two full rounds of that fixed cost for 18
// records to finalize.  Target ~3 workgroups per compute unit in ONE round; never fewer than 256 rows per workgroup.
static int wg_chunk(int n, int tiles, bool filed = false) {
    // filed: the launch will run inside the batched launch of a whole backward (WgradJob), where the OTHER jobs fill the GPU:
    // longer chunks -- fewer records to write and to sum, the per-workgroup fixed cost paid less often
    // (bench step at 768 / 384 / 192 / 96 workgroups per job: 10.51 / 10.42 / 10.42 / 10.47 ms)
    const int target = filed ? 256 : 768;  // (768: swept in round 2, DESIGN.md / profiles/HISTORY.md)
    const int chunks = std::max(1, target / std::max(1, tiles));
    const long long rows = ((long long)n + chunks - 1) / chunks;
    long long chunk = std::max<long long>(WG_CHUNK, (rows + 127) / 128 * 128);
    // The grid is (chunks, tiles, products), x fastest, and workgroups go round-robin over the 8 XCDs: with a chunk count that
    // is a multiple of 8 all tile / product workgroups of a chunk -- which read the same operand rows at the same time --
    // land on ONE XCD and queue on the same L2 lines (measured with a grid built that way on purpose: 11.34 against 10.98 ms
    // per step).  Keep the count off the multiples of 8 when more than one workgroup shares a chunk.
    // (forcing the count ODD -- consecutive tiles walking through all eight XCDs -- measured 0.07-0.09 ms slower than the
    // counts the rule above produces: 469 / 235 / 134, 74 / 50 / 37, 18 / 12 / 9, 5 / 3 / 2 at the four levels)
    if (tiles > 1) {
        int guard = 0;
        while ((((long long)n + chunk - 1) / chunk) % 8 == 0 && ((long long)n + chunk - 1) / chunk > 1 && guard++ < 16) chunk += 128;
    }
    return (int)std::min<long long>(chunk, 1 << 20);
}

// ---- one description per call, one place that files or launches it ---------------------------------------------------------
namespace {
// the kernel forms: a table of filed jobs, a batched launch and a kernel-timer id each
enum WgradForm { WF_LDS = 0, WF_LDS_RS, WF_DIRECT, WF_DIRECT_BF16, WF_GROUPED, WF_RECOMPUTE, WGRAD_FORMS };
constexpr int wgrad_kid(WgradForm f) {
    return f == WF_RECOMPUTE ? KID_WGRAD_TILE : f == WF_GROUPED ? KID_WGRAD_GROUPED : (f == WF_LDS || f == WF_LDS_RS) ? KID_WGRAD_LDS : KID_WGRAD;
}
// a planned call: the job as the kernels and the finalize read it (part is set by wgrad_submit) and what only the host needs
struct WgradCall {
    WgradJob J;
    WgradForm form;
    double bytes;   // algorithmic bytes, strict: every operand read once, every result written once (the split-K partial
                    // records of this implementation are its own overhead, not the op's)
    size_t posrel;  // (recompute form, filed) floats of the relative-position buffer behind the records, written at the flush
};

struct WgradDefer {
    bool active = false;
    bool armed = false;          // the call in progress may be filed (set by the call sites whose operands outlive their Block)
    bool armed_rs = false;       // ... the row-scaled strided form (the grouped projection's weight gradient inside the attention)
    char *arena = nullptr;       // [a job table per form | kept operands and chunk records]
    size_t cap = 0, used = 0;
    std::vector<WgradJob> jobs[WGRAD_FORMS];  // filed since the last flush
    double bytes[WGRAD_FORMS] = {};           // their algorithmic bytes (kernel timer)
};
thread_local WgradDefer g_wdefer;
constexpr int WGRAD_MAX_JOBS = 64;
constexpr size_t WGRAD_TABLE_BYTES = ptv2_align256(sizeof(WgradJob) * WGRAD_MAX_JOBS);

// the caller armed the file for this call (rs: the row-scaled strided form and the recompute form)
bool may_file(bool rs) { return g_wdefer.active && (rs ? g_wdefer.armed_rs : g_wdefer.armed); }
}  // namespace

void ptv2_wgrad_defer_begin(void *arena, size_t bytes) {
    WgradDefer &D = g_wdefer;
    for (int f = 0; f < WGRAD_FORMS; ++f) { D.jobs[f].clear(); D.bytes[f] = 0.0; }
    D.armed = D.armed_rs = false;
    D.active = arena != nullptr && bytes > WGRAD_FORMS * WGRAD_TABLE_BYTES;
    D.arena = (char *)arena;
    D.cap = bytes;
    D.used = WGRAD_FORMS * WGRAD_TABLE_BYTES;
}
bool ptv2_wgrad_defer_active() { return g_wdefer.active; }
void ptv2_wgrad_defer_end() {
    g_wdefer.active = g_wdefer.armed = g_wdefer.armed_rs = false;
    for (auto &j : g_wdefer.jobs) j.clear();
}
void ptv2_wgrad_defer_arm(bool on) { g_wdefer.armed = on && g_wdefer.active; }
void ptv2_wgrad_defer_arm_rs(bool on) { g_wdefer.armed_rs = on && g_wdefer.active; }
bool ptv2_wgrad_defer_armed_rs() { return may_file(true); }
size_t ptv2_wgrad_defer_table_bytes() { return WGRAD_FORMS * WGRAD_TABLE_BYTES; }
// a slice of the arena that lives until the backward ends (operands a deferred job reads, its records); NULL: no room
float *ptv2_wgrad_defer_alloc(size_t floats) {
    WgradDefer &D = g_wdefer;
    const size_t bytes = ptv2_align256(sizeof(float) * floats);
    if (!D.active || D.used + bytes > D.cap) return nullptr;
    float *p = (float *)(D.arena + D.used);
    D.used += bytes;
    return p;
}
// runs the jobs filed so far: per kernel form the table writers, the batched kernel, the batched finalize
int ptv2_wgrad_defer_flush(void *stream) {
    WgradDefer &D = g_wdefer;
    if (!D.active) return PTV2_OK;
    hipStream_t st = (hipStream_t)stream;
    for (int f = 0; f < WGRAD_FORMS; ++f) {
        const WgradForm form = (WgradForm)f;
        std::vector<WgradJob> &jobs = D.jobs[form];
        if (jobs.empty()) continue;
        WgradJob *table = (WgradJob *)(D.arena + (size_t)form * WGRAD_TABLE_BYTES);
        const int njobs = (int)jobs.size();
        // the jobs whose workgroups run longest first (rows per workgroup x the row piece it reads): the backward files the
        // full-resolution patch-embedding Block LAST, and its 150 us workgroups starting at the end of the launch were its tail
        // (bench step 10.53 -> 10.49 ms)
        const bool row_pieces = form == WF_GROUPED || form == WF_RECOMPUTE;
        std::stable_sort(jobs.begin(), jobs.end(), [row_pieces](const WgradJob &a, const WgradJob &b) {
            const long long wa = (long long)a.chunk * (row_pieces ? a.gw * a.cin : 1), wb = (long long)b.chunk * (row_pieces ? b.gw * b.cin : 1);
            return wa > wb;
        });
        int wgs = 0, fin = 0;
        long long pos_wgs = 0;  // (recompute form: workgroups of the relative-position launch in front of the jobs)
        bool pos_all = form == WF_RECOMPUTE;
        for (WgradJob &J : jobs) {
            if (form == WF_RECOMPUTE) {
                J.ldy = pos_wgs;
                pos_wgs += ((long long)J.n * 16 + 255) / 256;
                pos_all = pos_all && J.mX[0] != nullptr;
            }
            J.wg0 = wgs; J.fin0 = fin;
            J.fin_lanes = J.chunks > 32 ? 4 : 1;
            wgs += J.wgs;
            fin += J.fin_lanes == 1 ? (J.rec + 255) / 256 * 256 : (J.rec + 63) / 64 * 256;  // whole workgroups
        }
        for (int at = 0; at < njobs; at += WGRAD_PACK) {
            WgradJobPack pack;
            const int cnt = std::min(WGRAD_PACK, njobs - at);
            for (int i = 0; i < WGRAD_PACK; ++i) pack.j[i] = jobs[(size_t)std::min(at + i, njobs - 1)];
            hipLaunchKernelGGL(wgrad_jobs_write_kernel, dim3(1), dim3(64), 0, st, pack, cnt, table + at);
        }
        {
            PtvScopedTimer t(wgrad_kid(form), st, D.bytes[form]);
            const dim3 grid((unsigned)wgs), block(TPB);
            const WgradJob *tab = table;
            switch (form) {
                case WF_LDS:  // (the LDS-staged kernels ask for more dynamic LDS than the default limit)
                    RUN(ptv2_kernel_lds((const void *)linear_wgrad_lds_kernel_jobs<0>, WL_LDS_BYTES));
                    hipLaunchKernelGGL(linear_wgrad_lds_kernel_jobs<0>, grid, block, WL_LDS_BYTES, st, tab, njobs);
                    break;
                case WF_LDS_RS:
                    RUN(ptv2_kernel_lds((const void *)linear_wgrad_lds_kernel_jobs<1>, WL_LDS_BYTES));
                    hipLaunchKernelGGL(linear_wgrad_lds_kernel_jobs<1>, grid, block, WL_LDS_BYTES, st, tab, njobs);
                    break;
                case WF_DIRECT: hipLaunchKernelGGL(linear_wgrad_kernel_jobs<false>, grid, block, 0, st, tab, njobs); break;
                case WF_DIRECT_BF16: hipLaunchKernelGGL(linear_wgrad_kernel_jobs<true>, grid, block, 0, st, tab, njobs); break;
                case WF_GROUPED: {
                    size_t lds = 0;
                    for (const WgradJob &J : jobs) lds = std::max(lds, grouped_lds_bytes(J.cin, J.gw));
                    hipLaunchKernelGGL(grouped_wgrad_kernel_jobs, grid, block, lds, st, tab, njobs);
                    break;
                }
                default:
                    if (gva_wgrad_tile_launch_jobs(tab, njobs, wgs, pos_all ? (int)pos_wgs : 0, st) != PTV2_OK) return PTV2_ERR_LAUNCH;
            }
        }
        hipLaunchKernelGGL(wgrad_jobs_finalize_kernel, dim3((unsigned)((fin + 255) / 256)), dim3(256), 0, st,
                           (const WgradJob *)table, njobs, fin);
        jobs.clear();
        D.bytes[form] = 0.0;
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// the multi form's finalize: record = [count][cout*cin] weights, then [count][cout] bias sums
struct MapWgradMulti {
    float *dW[6], *db[6];
    int count, wlen, cout;
    explicit MapWgradMulti(const WgradJob &J) : count(J.count), wlen(J.cout * J.cin), cout(J.cout) {
        for (int i = 0; i < 6; ++i) { dW[i] = J.mdW[i]; db[i] = J.mdb[i]; }
    }
    __device__ void operator()(int e, double v) const {
        const int wtot = count * wlen;
        if (e < wtot) {
            const int b = e / wlen;
            dW[b][e - b * wlen] = (float)v;
        } else {
            const int r = e - wtot, b = r / cout;
            if (db[b]) db[b][r - b * cout] = (float)v;
        }
    }
};

namespace gva {
template <> struct RiderOf<MapWgradMulti> {
    static constexpr bool ok = true;
    static PtvRider make(const MapWgradMulti &m) {
        PtvRider r{};
        r.kind = RIDER_WGRADN;
        for (int i = 0; i < 6; ++i) { r.p[i] = i < m.count ? m.dW[i] : nullptr; r.p[6 + i] = i < m.count ? m.db[i] : nullptr; }
        r.i0 = m.wlen; r.i1 = m.cout; r.i2 = m.count;
        return r;
    }
};
}  // namespace gva

// A planned call is filed -- `file`: the caller armed the file; the form's table and the arena have room: its records go to the
// arena (the caller's workspace is reused before the flush) -- or launched here with its finalize, records in the caller's
// workspace.  PTV2_ERR_WORKSPACE: not filed, and the workspace does not hold the call's records (nothing was launched)
static int wgrad_submit(WgradCall &C, bool file, void *workspace, size_t workspace_bytes, void *stream) {
    WgradDefer &D = g_wdefer;
    WgradJob &J = C.J;
    if (file && (int)D.jobs[C.form].size() < WGRAD_MAX_JOBS) {
        float *keep = ptv2_wgrad_defer_alloc((size_t)J.chunks * J.rec);
        float *pos = keep && C.posrel ? ptv2_wgrad_defer_alloc(C.posrel) : nullptr;
        if (keep && (pos || !C.posrel)) {
            J.part = keep;
            if (pos) J.mX[0] = pos;
            D.jobs[C.form].push_back(J);
            D.bytes[C.form] += C.bytes;
            return PTV2_OK;
        }
    }
    const size_t fit = workspace ? workspace_bytes / (sizeof(float) * (size_t)J.rec) : 0;
    // (the recompute form takes as many point splits as fit, never more than a filed job: the same bits either way)
    if (C.form == WF_RECOMPUTE && fit >= 1 && fit < (size_t)J.chunks) (void)gva_wgrad_tile_plan(&J, (int)fit);
    if (fit < (size_t)J.chunks) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    J.part = (float *)workspace;
    {
        PtvScopedTimer t(wgrad_kid(C.form), st, C.bytes);
        const dim3 grid(J.chunks, J.tiles, J.batch), block(TPB);
        switch (C.form) {
            case WF_LDS:
                RUN(ptv2_kernel_lds((const void *)linear_wgrad_lds_kernel<0>, WL_LDS_BYTES));
                hipLaunchKernelGGL(linear_wgrad_lds_kernel<0>, grid, block, WL_LDS_BYTES, st, J);
                break;
            case WF_LDS_RS:
                RUN(ptv2_kernel_lds((const void *)linear_wgrad_lds_kernel<1>, WL_LDS_BYTES));
                hipLaunchKernelGGL(linear_wgrad_lds_kernel<1>, grid, block, WL_LDS_BYTES, st, J);
                break;
            case WF_DIRECT: hipLaunchKernelGGL(linear_wgrad_kernel<false>, grid, block, 0, st, J); break;
            case WF_DIRECT_BF16: hipLaunchKernelGGL(linear_wgrad_kernel<true>, grid, block, 0, st, J); break;
            case WF_GROUPED:
                hipLaunchKernelGGL(grouped_wgrad_kernel, dim3((unsigned)J.wgs), block, grouped_lds_bytes(J.cin, J.gw), st, J);
                break;
            default:
                if (gva_wgrad_tile_launch_one(J, st) != PTV2_OK) return PTV2_ERR_LAUNCH;
        }
    }
    if (J.count > 0) launch_finalize(st, (const float *)J.part, J.chunks, J.rec, MapWgradMulti(J));
    else if (J.has_pb) launch_finalize(st, (const float *)J.part, J.chunks, J.rec, gva::MapSplit2<float>{J.dW, J.db, J.batch * J.cout * J.cin});
    else launch_finalize(st, (const float *)J.part, J.chunks, J.rec, gva::MapVec<float>{J.dW});
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// geometry of the matrix-core forms: 48 x 48 output tiles x products, row chunks by wg_chunk (`filed`: the armed state, whether
// or not the file then has room); has_pb and rec by the caller
static void plan_tiles(WgradJob &J, int n, int cout, int cin, int batch, bool filed) {
    J.n = n; J.cout = cout; J.cin = cin; J.batch = batch;
    J.tiles_i = (cin + WG_TILE - 1) / WG_TILE;
    J.tiles = (cout + WG_TILE - 1) / WG_TILE * J.tiles_i;
    J.chunk = wg_chunk(n, J.tiles * batch, filed);
    J.chunks = (n + J.chunk - 1) / J.chunk;
    J.wgs = J.chunks * J.tiles * batch;
}

// the strided batch on the matrix cores.  rowscale != NULL asks for weighted bias sums, which only the LDS-staged fp32 kernel
// forms (WF_LDS_RS); any other kernel leaves db alone (the caller forms the sums itself) and the call is a plain job
static WgradCall plan_strided(int n, int cout, int cin, int batch, const float *gY, long long ldy, long long sy, const float *X,
                              long long ldx, long long sx, float *dW, float *db, const float *rowscale, long long lds_s, bool filed) {
    WgradCall C{};
    WgradJob &J = C.J;
    plan_tiles(J, n, cout, cin, batch, filed);
    const bool use_lds = !ptv2_matmul_bf16() && wgrad_lds_shape_ok(cout, cin) && wgrad_lds_ok(gY, ldy, sy, X, ldx, sx);
    const bool rs = rowscale && db && use_lds;
    if (rowscale && !rs) db = nullptr;
    C.form = ptv2_matmul_bf16() ? WF_DIRECT_BF16 : rs ? WF_LDS_RS : use_lds ? WF_LDS : WF_DIRECT;
    C.bytes = 4.0 * batch * ((double)n * (cout + cin) + (double)cout * cin + (db ? cout : 0) + (rs ? (double)n : 0.0));
    J.has_pb = db ? 1 : 0;  // bias partials live behind the weight partials of each chunk record
    J.rec = batch * (cout * cin + (db ? cout : 0));
    J.ldy = ldy; J.sy = sy; J.ldx = ldx; J.sx = sx;
    J.gY = gY; J.X = X; J.dW = dW; J.db = db;
    if (rs) { J.rowscale = rowscale; J.lds_s = lds_s; }
    return C;
}

// the grouped projection's shape (eight output rows per group, operands as the attention backward passes them): the vector-ALU
// kernel that reads whole row pieces of X (grouped_wgrad_tile); AO_AMD_WP2_GROUPED=0: the strided matrix-core form
// (also when the matrix products run on bf16 operands: this one is a vector-ALU kernel, exact fp32 either way)
static bool plan_grouped(WgradCall *C, int n, int cout, int cin, int batch, const float *gY, long long ldy, long long sy,
                         const float *X, long long ldx, long long sx, float *dW, float *db, const float *rowscale, long long lds_s) {
    static const bool grouped_on = !ptv2_env_is("AO_AMD_WP2_GROUPED", '0');
    if (!(grouped_on && rowscale && db && cout == GRP_I && cin % 4 == 0 && cin / 4 <= TPB && ldy == (long long)batch * cout &&
          sy == cout && ldx == (long long)batch * cin && sx == cin && lds_s == batch && wgrad_lds_ok(gY, ldy, sy, X, ldx, sx)))
        return false;
    *C = WgradCall{};
    WgradJob &J = C->J;
    const int q = cin / 4;
    int gw = 1;
    for (int d = 1; d <= batch; ++d)
        if (batch % d == 0 && d * q <= TPB) gw = d;
    const int blocks_g = batch / gw;
    const int chunks = (int)std::max<long long>(1, std::min<long long>(((long long)n + 127) / 128, std::max(1, 768 / blocks_g)));
    J.n = n; J.cout = cout; J.cin = cin; J.tiles_i = 1; J.tiles = blocks_g; J.batch = batch; J.gw = gw;
    J.chunk = (n + chunks - 1) / chunks;
    J.chunks = (n + J.chunk - 1) / J.chunk;
    J.wgs = J.chunks * blocks_g;
    J.has_pb = 1;
    J.rec = batch * (cout * cin + cout);
    J.ldy = ldy; J.sy = sy; J.ldx = ldx; J.sx = sx; J.lds_s = lds_s;
    J.gY = gY; J.X = X; J.rowscale = rowscale; J.dW = dW; J.db = db;
    C->form = WF_GROUPED;
    C->bytes = 4.0 * batch * ((double)n * (cout + cin) + (double)cout * cin + cout + (double)n);
    return true;
}

// up to six products of one shape, an operand pair each; PTV2_ERR_ARG (geometry filled all the same) for a missing operand
static int plan_multi(WgradCall *C, int n, int cout, int cin, int count, const float *const *gY, const float *const *X,
                      float *const *dW, float *const *db, const float *const *xsc, const float *const *xsh, bool filed) {
    *C = WgradCall{};
    WgradJob &J = C->J;
    plan_tiles(J, n, cout, cin, count, filed);
    J.has_pb = 1;
    J.count = count;
    J.rec = count * (cout * cin + cout);
    J.ldy = cout; J.ldx = cin;
    bool lds_ok = !ptv2_matmul_bf16() && wgrad_lds_shape_ok(cout, cin);
    int distinct_x = 0;  // every DISTINCT X is read once (q, k, v share theirs)
    for (int i = 0; i < count; ++i) {
        if (!gY[i] || !X[i] || !dW[i]) return PTV2_ERR_ARG;
        J.mgY[i] = gY[i]; J.mX[i] = X[i]; J.mdW[i] = dW[i]; J.mdb[i] = db ? db[i] : nullptr;
        J.mxsc[i] = xsc ? xsc[i] : nullptr;
        J.mxsh[i] = xsh ? xsh[i] : nullptr;
        if ((J.mxsc[i] == nullptr) != (J.mxsh[i] == nullptr)) return PTV2_ERR_ARG;
        lds_ok = lds_ok && wgrad_lds_ok(gY[i], cout, 0, X[i], cin, 0);
        bool seen = false;
        for (int j = 0; j < i; ++j) seen |= J.mX[j] == J.mX[i] && J.mxsc[j] == J.mxsc[i];
        distinct_x += !seen;
    }
    C->form = ptv2_matmul_bf16() ? WF_DIRECT_BF16 : (lds_ok ? WF_LDS : WF_DIRECT);
    C->bytes = 4.0 * ((double)count * n * cout + (double)distinct_x * n * cin + (double)count * cout * (cin + 1));
    return PTV2_OK;
}

// internal (gva_block.hip): the grouped projection's weight gradient with A recomputed from the saved softmax weights
// (gva_wgrad_tile.hip): dW (g, 8, c) and db (g, 8) = sum_n g_out sw.  Filed when the caller's backward defers (the operands
// outlive the Block), else launched with its finalize; PTV2_ERR_ARG for shapes without an instance
int gva_wp2_wgrad_recompute(int n, int k, int c, int g, const gva::AttnIn &I, const gva::AttnBwdIn &X, float *dW, float *db,
                            void *workspace, size_t workspace_bytes, void *stream) {
    if (!gva_wgrad_tile_supported(k, c, g) || n < 1 || !X.g_out || !X.w || !X.sw || !I.a || !I.b || !I.coord || !I.idx || !dW || !db)
        return PTV2_ERR_ARG;
    WgradCall C{};
    WgradJob &J = C.J;
    J.n = n; J.cin = c; J.batch = g;
    J.gY = X.g_out; J.X = X.w; J.rowscale = X.sw; J.dW = dW; J.db = db;
    J.aux[0] = I.coord; J.aux[1] = I.idx; J.aux[2] = I.a; J.aux[3] = I.b;
    (void)gva_wgrad_tile_plan(&J, n / 128 + 1);
    C.form = WF_RECOMPUTE;
    C.bytes = 4.0 * ((double)n * (c + 16.0 * g + g + 16 + 3) + (double)c * c + c);  // g_out, w, sw, idx, coord in; dW, db out
    C.posrel = (size_t)n * 16 * 4;
    return wgrad_submit(C, may_file(true), workspace, workspace_bytes, stream);
}

// the public form of the above (include/ptv2_hip.h): the weight gradient that completes gva_attention_backward_hip_launcher,
// launched at once with its own finalize (no backward is deferring on a thread that calls it from outside the model runtime)
extern "C" int gva_attention_wgrad_hip_launcher(int n, int k, int c, int g, const float *g_out, const float *w, const float *sw,
                                                const float *a, const float *b, const float *coord, const int *idx, float *dWp2,
                                                float *dbp2, void *workspace, size_t workspace_bytes, void *stream) {
    if (!gva_wgrad_tile_supported(k, c, g) || n < 0) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    gva::AttnIn I{};
    I.a = a; I.b = b; I.coord = coord; I.idx = idx;
    gva::AttnBwdIn X{};
    X.g_out = g_out; X.w = w; X.sw = sw;
    return gva_wp2_wgrad_recompute(n, k, c, g, I, X, dWp2, dbp2, workspace, workspace_bytes, stream);
}

extern "C" int linear_wgrad_strided_hip_launcher(int n, int cout, int cin, int batch, const float *gY, long long ldy,
                                                 long long sy, const float *X, long long ldx, long long sx, float *dW,
                                                 float *db, void *workspace, size_t workspace_bytes, void *stream) {
    return linear_wgrad_strided_rowscale(n, cout, cin, batch, gY, ldy, sy, X, ldx, sx, dW, db, nullptr, 0, nullptr, workspace,
                                         workspace_bytes, stream);
}

extern "C" int linear_wgrad_strided_rowscale(int n, int cout, int cin, int batch, const float *gY, long long ldy, long long sy,
                                             const float *X, long long ldx, long long sx, float *dW, float *db,
                                             const float *rowscale, long long lds_s, int *weighted, void *workspace,
                                             size_t workspace_bytes, void *stream) {
    if (weighted) *weighted = 0;
    if (n < 1 || cout < 1 || cin < 1 || batch < 1) return PTV2_ERR_ARG;
    // (a row-scaled call is armed by the attention's caller, which keeps gY alive until the backward ends; a plain one by
    // the Linear + BatchNorm layers between the stages)
    const bool file = may_file(rowscale != nullptr);
    WgradCall C;
    if (plan_grouped(&C, n, cout, cin, batch, gY, ldy, sy, X, ldx, sx, dW, db, rowscale, lds_s)) {
        const int rc = wgrad_submit(C, file, workspace, workspace_bytes, stream);
        if (rc == PTV2_OK && weighted) *weighted = 1;
        if (rc != PTV2_ERR_WORKSPACE) return rc;  // (a workspace too small for its records: the matrix-core route)
    }
    C = plan_strided(n, cout, cin, batch, gY, ldy, sy, X, ldx, sx, dW, db, rowscale, lds_s, file);
    if (!workspace || workspace_bytes < sizeof(float) * (size_t)C.J.chunks * batch * ((size_t)cout * cin + cout)) return PTV2_ERR_WORKSPACE;
    if (C.form == WF_LDS_RS && weighted) *weighted = 1;
    return wgrad_submit(C, file, workspace, workspace_bytes, stream);
}

// count (<= 6) products dW[i] (cout,cin) = gY[i]^T X[i], db[i] = column sums of gY[i] (db[i] may be NULL), all of one
// shape and row count, in one launch + one finalize (workspace: dense_workspace_bytes(n, count * cout, cin))
extern "C" int linear_wgrad_multi_hip_launcher(int n, int cout, int cin, int count, const float *const *gY,
                                               const float *const *X, float *const *dW, float *const *db,
                                               const float *const *xsc, const float *const *xsh, void *workspace,
                                               size_t workspace_bytes, void *stream) {
    if (n < 1 || cout < 1 || cin < 1 || count < 1 || count > 6 || !gY || !X || !dW) return PTV2_ERR_ARG;
    const bool file = may_file(false);
    WgradCall C;
    const int prc = plan_multi(&C, n, cout, cin, count, gY, X, dW, db, xsc, xsh, file);
    if (!workspace || workspace_bytes < sizeof(float) * (size_t)C.J.chunks * C.J.rec) return PTV2_ERR_WORKSPACE;
    if (prc != PTV2_OK) return prc;
    return wgrad_submit(C, file, workspace, workspace_bytes, stream);
}

extern "C" int linear_wgrad_hip_launcher(int n, int cout, int cin, const float *gY, const float *X, float *dW,
                                         float *db, void *workspace, size_t workspace_bytes, void *stream) {
    return linear_wgrad_strided_hip_launcher(n, cout, cin, 1, gY, cout, 0, X, cin, 0, dW, db, workspace, workspace_bytes,
                                             stream);
}
