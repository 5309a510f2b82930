// ao_amd/csrc/inseval.hip -- the association pass of the instance-segmentation evaluator (include/ptv2_inseval_hip.h;
// DESIGN.md section 15): one read of the (P, M) proposal masks gives, per proposal, the histogram of its set points over the
// ground-truth instances, its size and its overlap with the void points.
//
// Blocked over POINTS: a workgroup owns INSEVAL_POINTS_PER_WG consecutive points and INSEVAL_ROWS_PER_WG consecutive
// proposals.  A thread reads the code and the mask column of its 8 points once, keeps them in registers, and walks the
// proposals: without nn_idx consecutive lanes read consecutive mask elements of one row (int4 per lane when the rows are
// 16-byte aligned, else 256 contiguous bytes per wave instruction); with nn_idx the lanes of a wave read wherever their
// nearest neighbours lie in the row: a gather, as local as the order of the origin points.
// A set element adds 1 to the shared-memory bin of its column; an unset lane issues no atomic.  The bins that are not zero are
// flushed with one global integer add each.
#include <algorithm>

#include "common.h"
#include "../../include/ptv2_inseval_hip.h"

namespace {

constexpr int ITPB = 256;
constexpr int PER_THREAD = INSEVAL_POINTS_PER_WG / ITPB;
constexpr int ROW_BATCH = 4;  // rows whose loads are in flight together
static_assert(INSEVAL_POINTS_PER_WG % (4 * ITPB) == 0, "whole runs of four points per thread");
static_assert(INSEVAL_ROWS_PER_WG % ROW_BATCH == 0, "whole batches of rows");

// every element of the three outputs is written: zeroed here, in one launch, then added to
__global__ __launch_bounds__(ITPB) void inseval_zero_kernel(int p, int g, int *__restrict__ inter, int *__restrict__ vert_count,
                                                           int *__restrict__ void_inter) {
    const size_t total = (size_t)p * (size_t)(g + 2);
    for (size_t e = (size_t)blockIdx.x * ITPB + threadIdx.x; e < total; e += (size_t)gridDim.x * ITPB) {
        const size_t row = e / (size_t)(g + 2);
        const int b = (int)(e % (size_t)(g + 2));
        if (b < g) inter[row * (size_t)g + b] = 0;
        else if (b == g) vert_count[row] = 0;
        else void_inter[row] = 0;
    }
}

// VEC: no nn_idx, m % 4 == 0 and 16-byte aligned rows: a thread's points are two runs of four, read as int4.
template <bool VEC>
__global__ __launch_bounds__(ITPB) void inseval_associate_kernel(int p, int m, int n, int g, const int *__restrict__ masks,
                                                                const int *__restrict__ nn, const int *__restrict__ code,
                                                                int *__restrict__ inter, int *__restrict__ vert_count,
                                                                int *__restrict__ void_inter) {
    __shared__ int s_bin[INSEVAL_ROWS_PER_WG][INSEVAL_BINS];
    __shared__ int s_cnt[INSEVAL_ROWS_PER_WG][2];  // set points, set void points
    for (int e = threadIdx.x; e < INSEVAL_ROWS_PER_WG * INSEVAL_BINS; e += ITPB) (&s_bin[0][0])[e] = 0;
    if (threadIdx.x < INSEVAL_ROWS_PER_WG * 2) (&s_cnt[0][0])[threadIdx.x] = 0;
    __syncthreads();

    // the thread's points: column of the masks (-1: reads nothing), ground-truth bin (-1: none), void
    int col[PER_THREAD], bin[PER_THREAD];
    unsigned is_void = 0u;
    const long long base = (long long)blockIdx.x * INSEVAL_POINTS_PER_WG;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const long long j = VEC ? base + ((long long)(k / 4) * ITPB + threadIdx.x) * 4 + (k % 4)
                                : base + (long long)k * ITPB + threadIdx.x;
        col[k] = -1;
        bin[k] = -1;
        if (j < n) {
            const int c = (!VEC && nn) ? nn[j] : (int)j;
            const int v = code[j];
            col[k] = (c >= 0 && c < m) ? c : -1;
            const int b = (v >> 1) - 1;
            bin[k] = (v >= 0 && b < g) ? b : -1;  // (v >= 0: b >= -1)
            if (v >= 0 && (v & 1)) is_void |= 1u << k;
        }
    }

    // ROW_BATCH rows at a time: every load of the batch is issued before its first count (a row past the last re-reads the
    // last and is not counted)
    const int row0 = blockIdx.y * INSEVAL_ROWS_PER_WG;
    for (int r0 = 0; r0 < INSEVAL_ROWS_PER_WG && row0 + r0 < p; r0 += ROW_BATCH) {  // (uniform over the workgroup)
        int val[ROW_BATCH][PER_THREAD];
#pragma unroll
        for (int r = 0; r < ROW_BATCH; ++r) {
            const int *__restrict__ mrow = masks + (size_t)min(row0 + r0 + r, p - 1) * (size_t)m;
            if (VEC) {
#pragma unroll
                for (int q = 0; q < PER_THREAD / 4; ++q) {  // (m % 4 == 0: col[4 q] < m covers the four)
                    const int4 v = col[4 * q] >= 0 ? *reinterpret_cast<const int4 *>(mrow + col[4 * q]) : make_int4(0, 0, 0, 0);
                    val[r][4 * q] = v.x; val[r][4 * q + 1] = v.y; val[r][4 * q + 2] = v.z; val[r][4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < PER_THREAD; ++k) val[r][k] = col[k] >= 0 ? mrow[col[k]] : 0;
            }
        }
#pragma unroll
        for (int r = 0; r < ROW_BATCH; ++r) {
            if (row0 + r0 + r >= p) continue;
            int n_set = 0, n_void = 0;
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                if (val[r][k] != 0) {
                    ++n_set;
                    n_void += (int)((is_void >> k) & 1u);
                    if (bin[k] >= 0) atomicAdd(&s_bin[r0 + r][bin[k]], 1);
                }
            }
            if (n_set) atomicAdd(&s_cnt[r0 + r][0], n_set);
            if (n_void) atomicAdd(&s_cnt[r0 + r][1], n_void);
        }
    }
    __syncthreads();

    for (int e = threadIdx.x; e < INSEVAL_ROWS_PER_WG * INSEVAL_BINS; e += ITPB) {
        const int r = e / INSEVAL_BINS, b = e % INSEVAL_BINS, row = row0 + r;
        const int c = s_bin[r][b];
        if (c && row < p && b < g) atomicAdd(inter + (size_t)row * (size_t)g + b, c);
    }
    if (threadIdx.x < INSEVAL_ROWS_PER_WG * 2) {
        const int r = threadIdx.x >> 1, which = threadIdx.x & 1, row = row0 + r;
        const int c = s_cnt[r][which];
        if (c && row < p) atomicAdd((which ? void_inter : vert_count) + row, c);
    }
}

}  // namespace

extern "C" int ptv2_inseval_abi_version(void) { return 1; }

extern "C" int inseval_associate_hip_launcher(int p, int m, int n, int g, const int *masks, const int *nn_idx, const int *gt_code,
                                              int *inter, int *vert_count, int *void_inter, void *stream) {
    if (p < 0 || p > INSEVAL_MAX_PROPOSALS || m < 0 || n < 0 || g < 0 || g > INSEVAL_BINS) return PTV2_ERR_ARG;
    if (!nn_idx && n != m) return PTV2_ERR_ARG;
    if (p > 0 && (!vert_count || !void_inter || (g > 0 && !inter))) return PTV2_ERR_ARG;
    if (p > 0 && n > 0 && (!gt_code || (m > 0 && !masks))) return PTV2_ERR_ARG;
    if (p == 0) return PTV2_OK;
    hipStream_t st = (hipStream_t)stream;
    const int zero_grid = (int)std::min<long long>(divup((long long)p * (g + 2), ITPB), 1024);
    hipLaunchKernelGGL(inseval_zero_kernel, dim3(zero_grid), dim3(ITPB), 0, st, p, g, inter, vert_count, void_inter);
    PTV2_CHECK_LAUNCH();
    if (n == 0 || m == 0) return PTV2_OK;
    dim3 grid(divup(n, INSEVAL_POINTS_PER_WG), divup(p, INSEVAL_ROWS_PER_WG));
    const bool vec = !nn_idx && m % 4 == 0 && (((uintptr_t)masks | (uintptr_t)gt_code) & 15) == 0;
    hipLaunchKernelGGL(vec ? inseval_associate_kernel<true> : inseval_associate_kernel<false>, grid, dim3(ITPB), 0, st, p, m, n, g,
                       masks, nn_idx, gt_code, inter, vert_count, void_inter);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
