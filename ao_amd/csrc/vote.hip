// ao_amd/csrc/vote.hip -- the vote of whole-scene test-time inference (gfx950), pointcept/engines/test.py:94-123:
//   * votes[index[i], :] += softmax(logits[i, :])   for one fragment (test.py:107,112)
//   * pred[i] = first maximal class of votes[i, :]  (test.py:123, `pred.max(1)[1]`)
// Both stream HBM.  A row's maximum and sum are taken inside the wavefront (a butterfly of fixed shape: the same bits in
// every lane and in every run), every logit is read once and no (n, c) temporary exists.  A fragment holds a point at most
// once (GridSample(mode="test") takes one point per voxel, SphereCrop(mode="all") crops a fragment), so rows of one segment
// never meet in the table: plain load-add-store, no float atomics, and segments issued one after the other on a stream give
// the bits of adding the fragments one at a time.
//   c <= 32: lanes across classes, 64 / W rows per wavefront (W = c rounded up to a power of two);
//   c  > 32: one row per wavefront, lane l holds classes l, l + 64, ... in R registers (c <= 64 R).
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int VTPB = 256;           // 4 wavefronts
constexpr int VOTE_MAX_C = 1024;
constexpr int VOTE_MAX_BLOCKS = 256 * 8;

__device__ __forceinline__ float load_logit(const float *p, long long e) { return p[e]; }
__device__ __forceinline__ float load_logit(const unsigned short *p, long long e) {  // bf16: the upper half of an fp32
    return __uint_as_float((unsigned)p[e] << 16);
}

// status[0] |= 1 when a row of the segment points outside the table.  The add kernel of the same segment reads the word
// and writes nothing while it is set: a bad segment leaves the table as it was.
template <class I>
__global__ __launch_bounds__(VTPB) void vote_check_kernel(int n, const I *__restrict__ index, long long n_total, int *status) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * VTPB + threadIdx.x; i < n; i += (long long)gridDim.x * VTPB) {
        const long long t = (long long)index[i];
        bad |= t < 0 || t >= n_total;
    }
    if (__any(bad) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(status, 1);
}

template <int W, class T, class I>
__global__ __launch_bounds__(VTPB) void vote_add_narrow_kernel(int n, int c, const T *__restrict__ logits, const I *__restrict__ index,
                                                               float *votes, long long n_total, const int *__restrict__ status) {
    if (*status) return;
    constexpr int RPW = WAVE / W, RPB = RPW * (VTPB / WAVE);
    const int lane = threadIdx.x & (WAVE - 1), j = lane & (W - 1);
    const int sub = (threadIdx.x / WAVE) * RPW + lane / W;
    const bool live = j < c;
    for (long long r0 = (long long)blockIdx.x * RPB; r0 < n; r0 += (long long)gridDim.x * RPB) {  // uniform over the block
        const long long r = r0 + sub;
        const bool row = r < n;
        const float x = (row && live) ? load_logit(logits, r * c + j) : -INFINITY;
        float m = x;
#pragma unroll
        for (int o = W / 2; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
        const float e = (row && live) ? expf(x - m) : 0.f;
        float s = e;
#pragma unroll
        for (int o = W / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, WAVE);
        if (row && live) {
            const long long t = (long long)index[r];
            if (t >= 0 && t < n_total) {
                float *v = votes + t * c + j;
                *v = *v + __fdiv_rn(e, s);
            }
        }
    }
}

template <int R, class T, class I>
__global__ __launch_bounds__(VTPB) void vote_add_wide_kernel(int n, int c, const T *__restrict__ logits, const I *__restrict__ index,
                                                             float *votes, long long n_total, const int *__restrict__ status) {
    if (*status) return;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    constexpr int RPB = VTPB / WAVE;
    for (long long r = (long long)blockIdx.x * RPB + wave; r < n; r += (long long)gridDim.x * RPB) {  // uniform over the wave
        float x[R];
        float m = -INFINITY;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int j = lane + WAVE * u;
            x[u] = j < c ? load_logit(logits, r * c + j) : -INFINITY;
            m = fmaxf(m, x[u]);
        }
#pragma unroll
        for (int o = WAVE / 2; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            x[u] = lane + WAVE * u < c ? expf(x[u] - m) : 0.f;
            s += x[u];
        }
#pragma unroll
        for (int o = WAVE / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, WAVE);
        const long long t = (long long)index[r];
        if (t >= 0 && t < n_total) {
            float *v = votes + t * c;
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int j = lane + WAVE * u;
                if (j < c) v[j] = v[j] + __fdiv_rn(x[u], s);
            }
        }
    }
}

// (value, class) of the better of two candidates: the larger value, the lower class among equals
__device__ __forceinline__ void better(float &v, int &k, float ov, int ok) {
    if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
}

template <int W>
__global__ __launch_bounds__(VTPB) void vote_argmax_narrow_kernel(long long n, int c, const float *__restrict__ votes,
                                                                  long long *__restrict__ pred) {
    constexpr int RPW = WAVE / W, RPB = RPW * (VTPB / WAVE);
    const int lane = threadIdx.x & (WAVE - 1), j = lane & (W - 1);
    const int sub = (threadIdx.x / WAVE) * RPW + lane / W;
    for (long long r0 = (long long)blockIdx.x * RPB; r0 < n; r0 += (long long)gridDim.x * RPB) {
        const long long r = r0 + sub;
        const bool ok = r < n && j < c;
        float v = ok ? votes[r * c + j] : -INFINITY;
        int k = ok ? j : INT_MAX;
#pragma unroll
        for (int o = W / 2; o >= 1; o >>= 1) better(v, k, __shfl_xor(v, o, WAVE), __shfl_xor(k, o, WAVE));
        if (r < n && j == 0) pred[r] = k == INT_MAX ? 0 : k;
    }
}

__global__ __launch_bounds__(VTPB) void vote_argmax_wide_kernel(long long n, int c, const float *__restrict__ votes,
                                                                long long *__restrict__ pred) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    constexpr int RPB = VTPB / WAVE;
    for (long long r = (long long)blockIdx.x * RPB + wave; r < n; r += (long long)gridDim.x * RPB) {
        float v = -INFINITY;
        int k = INT_MAX;
        for (int j = lane; j < c; j += WAVE) better(v, k, votes[r * c + j], j);  // ascending j: the first maximum stays
#pragma unroll
        for (int o = WAVE / 2; o >= 1; o >>= 1) better(v, k, __shfl_xor(v, o, WAVE), __shfl_xor(k, o, WAVE));
        if (lane == 0) pred[r] = k == INT_MAX ? 0 : k;
    }
}

int vote_grid(long long rows, int rows_per_block) {
    return (int)std::max<long long>(1, std::min<long long>((rows + rows_per_block - 1) / rows_per_block, VOTE_MAX_BLOCKS));
}

template <class T, class I>
void launch_add(int n, int c, const T *logits, const I *index, float *votes, long long n_total, int *status, hipStream_t st) {
    hipLaunchKernelGGL((vote_check_kernel<I>), dim3(vote_grid(n, VTPB)), dim3(VTPB), 0, st, n, index, n_total, status);
#define VOTE_NARROW(W)                                                                                                      \
    hipLaunchKernelGGL((vote_add_narrow_kernel<W, T, I>), dim3(vote_grid(n, (WAVE / W) * (VTPB / WAVE))), dim3(VTPB), 0, st, n, c, \
                       logits, index, votes, n_total, (const int *)status)
#define VOTE_WIDE(R)                                                                                                      \
    hipLaunchKernelGGL((vote_add_wide_kernel<R, T, I>), dim3(vote_grid(n, VTPB / WAVE)), dim3(VTPB), 0, st, n, c, logits, index, \
                       votes, n_total, (const int *)status)
    if (c <= 2) VOTE_NARROW(2);
    else if (c <= 4) VOTE_NARROW(4);
    else if (c <= 8) VOTE_NARROW(8);
    else if (c <= 16) VOTE_NARROW(16);
    else if (c <= 32) VOTE_NARROW(32);
    else if (c <= 64) VOTE_WIDE(1);
    else if (c <= 128) VOTE_WIDE(2);
    else if (c <= 256) VOTE_WIDE(4);
    else VOTE_WIDE(16);
#undef VOTE_NARROW
#undef VOTE_WIDE
}

}  // namespace

extern "C" int seg_vote_add_hip_launcher(int n, int c, const void *logits, int logits_bf16, const void *index, int index_i64,
                                         float *votes, long long n_total, int *status, void *stream) {
    if (n < 0 || c < 2 || c > VOTE_MAX_C || n_total < 0 || !status) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!logits || !index || !votes) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (logits_bf16) {
        if (index_i64) launch_add(n, c, (const unsigned short *)logits, (const long long *)index, votes, n_total, status, st);
        else launch_add(n, c, (const unsigned short *)logits, (const int *)index, votes, n_total, status, st);
    } else {
        if (index_i64) launch_add(n, c, (const float *)logits, (const long long *)index, votes, n_total, status, st);
        else launch_add(n, c, (const float *)logits, (const int *)index, votes, n_total, status, st);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// The verdict on every seg_vote_add issued with this status word so far: one read-back (a host synchronisation).  The word
// is cleared when it was set, so that the table stays usable after the error has been reported.
extern "C" int seg_vote_status_hip_launcher(int *status, void *stream) {
    if (!status) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    int bad = 0;
    if (hipMemcpyAsync(&bad, status, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return PTV2_ERR_LAUNCH;
    if (!bad) return PTV2_OK;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) return PTV2_ERR_LAUNCH;
    return PTV2_ERR_ARG;
}

extern "C" int seg_vote_argmax_hip_launcher(long long n_total, int c, const float *votes, long long *pred, void *stream) {
    if (n_total < 0 || c < 1 || c > VOTE_MAX_C) return PTV2_ERR_ARG;
    if (n_total == 0) return PTV2_OK;
    if (!votes || !pred) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
#define VOTE_ARGMAX(W)                                                                                                         \
    hipLaunchKernelGGL((vote_argmax_narrow_kernel<W>), dim3(vote_grid(n_total, (WAVE / W) * (VTPB / WAVE))), dim3(VTPB), 0, st, \
                       n_total, c, votes, pred)
    if (c <= 2) VOTE_ARGMAX(2);
    else if (c <= 4) VOTE_ARGMAX(4);
    else if (c <= 8) VOTE_ARGMAX(8);
    else if (c <= 16) VOTE_ARGMAX(16);
    else if (c <= 32) VOTE_ARGMAX(32);
    else
        hipLaunchKernelGGL(vote_argmax_wide_kernel, dim3(vote_grid(n_total, VTPB / WAVE)), dim3(VTPB), 0, st, n_total, c, votes, pred);
#undef VOTE_ARGMAX
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
