// ao_amd/csrc/refine.hip -- REAL's epoch-end label refinement (gfx950), include/ptv2_refine_hip.h.  What
// pointcept/engines/train_sam_real.py does per whole scene on the host with numpy:
//   :333-338  prediction and softmax top-two margin ("confidence") of the basket's logits      -> refine_confidence
//   :353-391  a triple python loop (x cells, y cells, classes), a full-n boolean mask each:
//             one prompt per (cell, class)                                                     -> refine_prompts
//   :453-472  per SAM mask: gather over the visible points, a mode, a vote                     -> refine_vote
//   :488-512  argmax of the votes, agreement with the network, label rewrite                   -> refine_update
// Here: one pass over the logits, a segmented arg-max (one 64-bit atomicMax per candidate into an (nx, ny, c) table and
// an ordered single-workgroup compaction), a histogram and a vote pass per view, one pass over the votes.  Every
// accumulation is an integer atomic or an atomicMax: the results do not depend on execution order.
// Rows of (n, c) arrays are 52 / 80 bytes (c = 13 / 20); a workgroup reads its 256 rows as one contiguous span into LDS
// (row stride c | 1: odd, so that lane-per-row reads meet no bank twice) instead of c strided dwords per lane.
// Every index derived from input data is range checked; a bad one is skipped and recorded in the status word.
#include <limits.h>

#include <algorithm>

#include "common.h"
#include "../../include/ptv2_refine_hip.h"

extern "C" int ptv2_refine_abi_version(void) { return 1; }  // == EXPECTED_REFINE_ABI in ao_amd/_lib.py

namespace {

constexpr int RTPB = 256;                      // rows per workgroup pass == threads
constexpr int RMAXC = PTV2_REFINE_MAX_C;
constexpr int RSTRIDE = RMAXC | 1;
constexpr int RMAX_BLOCKS = 256 * 8;
constexpr int CTPB = 1024;                     // the compaction's one workgroup
constexpr int PTILE = 64;                      // prompts per workgroup of the vote kernels
typedef unsigned long long u64;

int row_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + RTPB - 1) / RTPB, RMAX_BLOCKS)); }

// rows [r0, r0 + RTPB) of a (n, c) dword array -> s[row][c | 1], lanes striding the flat span
__device__ __forceinline__ void stage_rows(const unsigned *__restrict__ src, long long r0, long long n, int c, unsigned *s) {
    const int cs = c | 1;
    const int count = (int)min((long long)RTPB, n - r0) * c;
    const unsigned *p = src + r0 * c;
    for (int e = threadIdx.x; e < count; e += RTPB) {
        const int r = e / c;
        s[r * cs + (e - r * c)] = p[e];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------ confidence --
__global__ __launch_bounds__(RTPB) void refine_confidence_kernel(long long n, int c, const float *__restrict__ logits,
                                                                 int *__restrict__ pred, float *__restrict__ conf) {
    __shared__ unsigned s[RTPB * RSTRIDE];
    const int cs = c | 1;
    for (long long r0 = (long long)blockIdx.x * RTPB; r0 < n; r0 += (long long)gridDim.x * RTPB) {  // uniform over the block
        stage_rows((const unsigned *)logits, r0, n, c, s);
        const long long i = r0 + threadIdx.x;
        if (i < n) {
            const float *x = (const float *)s + threadIdx.x * cs;
            float m = x[0];
            int k = 0;
            for (int j = 1; j < c; ++j)
                if (x[j] > m) { m = x[j]; k = j; }  // strict: the first maximum stays (np.argmax)
            float sum = 0.f;
            for (int j = 0; j < c; ++j) sum += expf(x[j] - m);
            float t1 = -1.f, t2 = -1.f;  // the two last entries of the sorted row: equal maxima give a margin of 0
            for (int j = 0; j < c; ++j) {
                const float p = __fdiv_rn(expf(x[j] - m), sum);
                if (p > t1) { t2 = t1; t1 = p; }
                else if (p > t2) t2 = p;
            }
            pred[i] = x[0] == -100.f ? -1 : k;
            conf[i] = t1 - t2;
        }
        __syncthreads();  // s is restaged by the next pass
    }
}

// --------------------------------------------------------------------------------------------------------- prompts --
// boundary i of an axis, in the reference's arithmetic: np.float32(min) + float32(i * grid)
__device__ __forceinline__ float cell_bound(float lo, int i, double grid) { return __fadd_rn(lo, (float)((double)i * grid)); }

// the cell of x, or -1: an arithmetic candidate, then the reference's own strict comparisons on it and its neighbours
__device__ __forceinline__ int cell_of(float x, float lo, int cells, double grid) {
    const float t = floorf((x - lo) / (float)grid);
    if (!(t >= -1.f && t <= (float)cells)) return -1;  // (a NaN too)
    const int i0 = (int)t;
    for (int i = i0 - 1; i <= i0 + 1; ++i)
        if (i >= 0 && i < cells && cell_bound(lo, i, grid) < x && x < cell_bound(lo, i + 1, grid)) return i;
    return -1;
}

__global__ __launch_bounds__(RTPB) void refine_prompt_scan_kernel(int n, int c, const float *__restrict__ coord,
                                                                  const int *__restrict__ pred, const float *__restrict__ conf,
                                                                  const int *__restrict__ label,
                                                                  const unsigned char *__restrict__ present, float lo_x, float lo_y,
                                                                  int nx, int ny, double grid, float threshold, u64 *table,
                                                                  int *status) {
    unsigned have = 0;
    for (int j = 0; j < c; ++j) have |= present[j] ? 1u << j : 0u;
    for (long long i = (long long)blockIdx.x * RTPB + threadIdx.x; i < n; i += (long long)gridDim.x * RTPB) {
        const int k = pred[i];
        if (k == -1) continue;
        if (k < 0 || k >= c) { atomicOr(status + PTV2_REFINE_STATUS_ERROR, PTV2_REFINE_BAD_CLASS); continue; }
        const float f = conf[i];
        if (!(f > threshold) || !(f >= 0.f) || !((have >> k) & 1u) || label[i] == k) continue;
        const int ix = cell_of(coord[3 * i], lo_x, nx, grid);
        if (ix < 0) continue;
        const int iy = cell_of(coord[3 * i + 1], lo_y, ny, grid);
        if (iy < 0) continue;
        // the larger conf wins (non-negative floats order as their bits), then the lower index (the larger ~index)
        const u64 key = ((u64)__float_as_uint(f) << 32) | (u64)(~(unsigned)i);
        atomicMax(table + ((long long)ix * ny + iy) * c + k, key);
    }
}

// the table's occupied entries in index order == (ix, iy, class) ascending, the reference's append order
__global__ __launch_bounds__(CTPB) void refine_prompt_compact_kernel(const u64 *__restrict__ table, long long entries, int c, int n,
                                                                     int capacity, int *__restrict__ prompt_idx,
                                                                     int *__restrict__ prompt_cls, int *status) {
    __shared__ int wave_count[CTPB / WAVE];
    __shared__ int running;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (threadIdx.x == 0) running = 0;
    __syncthreads();
    for (long long base = 0; base < entries; base += CTPB) {  // uniform over the block
        const long long e = base + threadIdx.x;
        const u64 key = e < entries ? table[e] : 0ull;
        const bool has = key != 0ull;
        const u64 b = __ballot(has);
        if (lane == 0) wave_count[wave] = __popcll(b);
        __syncthreads();
        int at = running;
        for (int w = 0; w < wave; ++w) at += wave_count[w];
        at += __popcll(b & ((1ull << lane) - 1ull));
        if (has) {
            const unsigned idx = ~(unsigned)key;
            if (at < capacity && idx < (unsigned)n) {
                prompt_idx[at] = (int)idx;
                prompt_cls[at] = (int)(e % c);
            } else {
                atomicOr(status + PTV2_REFINE_STATUS_ERROR, PTV2_REFINE_BAD_CAPACITY);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < CTPB / WAVE; ++w) t += wave_count[w];
            running += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) status[PTV2_REFINE_STATUS_PROMPTS] = min(running, capacity);
}

// ------------------------------------------------------------------------------------------------------------ vote --
// pix[i] = offset of the point's mask element, -1 when the point is inside no mask of this view (invisible, element [0][0],
// or a pixel outside the image: recorded)
__global__ __launch_bounds__(RTPB) void refine_pixel_kernel(long long n, const int *__restrict__ bridge, int height, int width,
                                                            int *__restrict__ pix, int *status) {
    for (long long i = (long long)blockIdx.x * RTPB + threadIdx.x; i < n; i += (long long)gridDim.x * RTPB) {
        int p = -1;
        if (bridge[3 * i + 2] == 1) {
            const int u = bridge[3 * i], v = bridge[3 * i + 1];
            if (u < 0 || u > height || v < 0 || v > width) {
                atomicOr(status + PTV2_REFINE_STATUS_ERROR, PTV2_REFINE_BAD_PIXEL);
            } else {
                const int r = u == 0 ? height - 1 : u - 1, q = v == 0 ? width - 1 : v - 1;  // numpy's index -1
                if (r != 0 || q != 0) p = r * width + q;                                   // mask_now[0, 0] = False
            }
        }
        pix[i] = p;
    }
}

// hist[p][pred[i]] += 1 over the confident points inside mask p; blockIdx.y: a tile of PTILE prompts
__global__ __launch_bounds__(RTPB) void refine_hist_kernel(long long n, int c, const int *__restrict__ pix, const int *__restrict__ pred,
                                                           const float *__restrict__ conf, int prompts,
                                                           const unsigned char *__restrict__ masks, long long hw, float threshold,
                                                           int *hist, int *status) {
    __shared__ int s[PTILE * RMAXC];
    const int p0 = blockIdx.y * PTILE, np = min(PTILE, prompts - p0);
    for (int e = threadIdx.x; e < np * c; e += RTPB) s[e] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * RTPB + threadIdx.x; i < n; i += (long long)gridDim.x * RTPB) {
        const int at = pix[i];
        if (at < 0 || !(conf[i] > threshold)) continue;
        const int k = pred[i];
        if (k < 0 || k >= c) {  // (-1, an unseen row, has conf 0 and does not get here for a threshold >= 0)
            if (k != -1) atomicOr(status + PTV2_REFINE_STATUS_ERROR, PTV2_REFINE_BAD_CLASS);
            continue;
        }
        const unsigned char *m = masks + (long long)p0 * hw + at;
        for (int p = 0; p < np; ++p)
            if (m[(long long)p * hw]) atomicAdd(&s[p * c + k], 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < np * c; e += RTPB)
        if (s[e]) atomicAdd(hist + (long long)p0 * c + e, s[e]);
}

// cast[p] = the prompt's class when the histogram is non-empty and its mode (the smallest class among the most frequent,
// scipy.stats.mode) is that class, else -1
__global__ __launch_bounds__(RTPB) void refine_mode_kernel(int prompts, int c, const int *__restrict__ hist,
                                                           const int *__restrict__ prompt_cls, int *__restrict__ cast, int *status) {
    const int p = blockIdx.x * RTPB + threadIdx.x;
    if (p >= prompts) return;
    int best = 0, mode = -1;
    for (int j = 0; j < c; ++j) {
        const int h = hist[(long long)p * c + j];
        if (h > best) { best = h; mode = j; }
    }
    const int cls = prompt_cls[p];
    if (cls < 0 || cls >= c) {
        atomicOr(status + PTV2_REFINE_STATUS_ERROR, PTV2_REFINE_BAD_CLASS);
        cast[p] = -1;
        return;
    }
    cast[p] = mode == cls ? cls : -1;
}

__global__ __launch_bounds__(RTPB) void refine_cast_kernel(long long n, int c, const int *__restrict__ pix, int prompts,
                                                           const int *__restrict__ cast, const unsigned char *__restrict__ masks,
                                                           long long hw, int *vote) {
    __shared__ int s_cast[PTILE];
    __shared__ int s_any;
    const int p0 = blockIdx.y * PTILE, np = min(PTILE, prompts - p0);
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    if ((int)threadIdx.x < np) {
        const int k = cast[p0 + threadIdx.x];
        s_cast[threadIdx.x] = k;
        if (k >= 0) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return;  // uniform over the block
    for (long long i = (long long)blockIdx.x * RTPB + threadIdx.x; i < n; i += (long long)gridDim.x * RTPB) {
        const int at = pix[i];
        if (at < 0) continue;
        const unsigned char *m = masks + (long long)p0 * hw + at;
        for (int p = 0; p < np; ++p) {
            const int k = s_cast[p];  // in [0, c) or -1: checked by refine_mode_kernel
            if (k >= 0 && m[(long long)p * hw]) atomicAdd(vote + i * c + k, 1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- update --
__global__ __launch_bounds__(RTPB) void refine_update_kernel(long long n, int c, const int *__restrict__ vote,
                                                             const int *__restrict__ pred, int *__restrict__ label, int *status) {
    __shared__ unsigned s[RTPB * RSTRIDE];
    const int cs = c | 1;
    for (long long r0 = (long long)blockIdx.x * RTPB; r0 < n; r0 += (long long)gridDim.x * RTPB) {  // uniform over the block
        stage_rows((const unsigned *)vote, r0, n, c, s);
        const long long i = r0 + threadIdx.x;
        bool changed = false;
        if (i < n) {
            const int *v = (const int *)s + threadIdx.x * cs;
            int best = v[0], result = 0;
            long long sum = v[0];
            for (int j = 1; j < c; ++j) {
                if (v[j] > best) { best = v[j]; result = j; }
                sum += v[j];
            }
            const int k = pred[i];
            if (sum != 0 && result == k && k != -1) {
                changed = label[i] != result;
                label[i] = result;
            }
        }
        const u64 b = __ballot(changed);
        if ((threadIdx.x & (WAVE - 1)) == 0 && b) atomicAdd(status + PTV2_REFINE_STATUS_UPDATED, __popcll(b));
        __syncthreads();
    }
}

bool bad_sizes(long long n, int c) { return n < 0 || n > INT_MAX || c < PTV2_REFINE_MIN_C || c > PTV2_REFINE_MAX_C; }

struct PromptSpace { u64 *table; };
size_t carve_prompts(char *ws, int c, long long cells, PromptSpace &s) {
    PtvCarver k{ws, 0};
    s.table = k.take_n<u64>((size_t)cells * c);
    return k.off;
}
struct VoteSpace { int *pix, *hist, *cast; };
size_t carve_vote(char *ws, long long n, int c, int prompts, VoteSpace &s) {
    PtvCarver k{ws, 0};
    s.pix = k.take_n<int>((size_t)n);
    s.hist = k.take_n<int>((size_t)prompts * c);
    s.cast = k.take_n<int>((size_t)prompts);
    return k.off;
}

}  // namespace

extern "C" long long refine_workspace_bytes(long long n, int c, long long cells, int prompts) {
    if (bad_sizes(n, c) || cells < 0 || cells > INT_MAX || prompts < 0) return -1;
    PromptSpace ps;
    VoteSpace vs;
    return (long long)std::max(carve_prompts(nullptr, c, cells, ps), carve_vote(nullptr, n, c, prompts, vs));
}

extern "C" int refine_confidence_hip_launcher(long long n, int c, const float *logits, int *pred, float *conf, void *stream) {
    if (bad_sizes(n, c)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!logits || !pred || !conf) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(refine_confidence_kernel, dim3(row_grid(n)), dim3(RTPB), 0, (hipStream_t)stream, n, c, logits, pred, conf);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int refine_prompts_hip_launcher(long long n, int c, const float *coord, const int *pred, const float *conf,
                                           const int *label, const void *present, float lo_x, float lo_y, int nx, int ny,
                                           double grid, float threshold, void *workspace, long long workspace_bytes, int capacity,
                                           int *prompt_idx, int *prompt_cls, int *status, void *stream) {
    if (bad_sizes(n, c) || nx < 0 || ny < 0 || capacity < 0 || !status || !(grid > 0.0) || !(threshold >= 0.f)) return PTV2_ERR_ARG;
    const long long cells = (long long)nx * ny;
    if (cells > INT_MAX || cells * c > INT_MAX) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const bool empty = n == 0 || cells == 0;
    if (!empty && (!coord || !pred || !conf || !label || !present || !workspace || !prompt_idx || !prompt_cls)) return PTV2_ERR_ARG;
    PromptSpace s;
    if (!empty && (long long)carve_prompts((char *)workspace, c, cells, s) > workspace_bytes) return PTV2_ERR_WORKSPACE;
    if (hipMemsetAsync(status + PTV2_REFINE_STATUS_PROMPTS, 0, sizeof(int), st) != hipSuccess) return PTV2_ERR_LAUNCH;
    if (empty) return PTV2_OK;
    const long long entries = cells * c;
    if (hipMemsetAsync(s.table, 0, sizeof(u64) * (size_t)entries, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(refine_prompt_scan_kernel, dim3(row_grid(n)), dim3(RTPB), 0, st, (int)n, c, coord, pred, conf, label,
                       (const unsigned char *)present, lo_x, lo_y, nx, ny, grid, threshold, s.table, status);
    hipLaunchKernelGGL(refine_prompt_compact_kernel, dim3(1), dim3(CTPB), 0, st, (const u64 *)s.table, entries, c, (int)n, capacity,
                       prompt_idx, prompt_cls, status);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int refine_vote_hip_launcher(long long n, int c, const int *bridge, const int *pred, const float *conf, int prompts,
                                        const int *prompt_cls, const void *masks, int height, int width, float threshold,
                                        void *workspace, long long workspace_bytes, int *vote, int *status, void *stream) {
    if (bad_sizes(n, c) || prompts < 0 || height < 1 || width < 1 || (long long)height * width > INT_MAX || !status) return PTV2_ERR_ARG;
    if (n == 0 || prompts == 0) return PTV2_OK;
    if (!bridge || !pred || !conf || !prompt_cls || !masks || !workspace || !vote) return PTV2_ERR_ARG;
    VoteSpace s;
    if ((long long)carve_vote((char *)workspace, n, c, prompts, s) > workspace_bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)height * width;
    const int tiles = (prompts + PTILE - 1) / PTILE;
    const dim3 grid((unsigned)std::min(row_grid(n), 1024), (unsigned)tiles);
    if (hipMemsetAsync(s.hist, 0, sizeof(int) * (size_t)prompts * c, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(refine_pixel_kernel, dim3(row_grid(n)), dim3(RTPB), 0, st, n, bridge, height, width, s.pix, status);
    hipLaunchKernelGGL(refine_hist_kernel, grid, dim3(RTPB), 0, st, n, c, (const int *)s.pix, pred, conf, prompts,
                       (const unsigned char *)masks, hw, threshold, s.hist, status);
    hipLaunchKernelGGL(refine_mode_kernel, dim3((prompts + RTPB - 1) / RTPB), dim3(RTPB), 0, st, prompts, c, (const int *)s.hist,
                       prompt_cls, s.cast, status);
    hipLaunchKernelGGL(refine_cast_kernel, grid, dim3(RTPB), 0, st, n, c, (const int *)s.pix, prompts, (const int *)s.cast,
                       (const unsigned char *)masks, hw, vote);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int refine_update_hip_launcher(long long n, int c, const int *vote, const int *pred, int *label, int *status,
                                          void *stream) {
    if (bad_sizes(n, c) || !status) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!vote || !pred || !label) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(refine_update_kernel, dim3(row_grid(n)), dim3(RTPB), 0, (hipStream_t)stream, n, c, vote, pred, label, status);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
