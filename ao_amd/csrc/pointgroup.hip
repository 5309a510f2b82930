// ao_amd/csrc/pointgroup.hip -- PointGroup's (PG-v1m1) clustering stage for gfx950 (MI355X); C ABI include/ptv2_pg_hip.h.
//
// Replaces libs/pointgroup_ops of the reference (one thread per point scanning its whole cloud with a 1000-int array in scratch,
// re-launched until a guessed buffer fits; a host queue over the downloaded edge lists; a dense (nProposal, N) matrix; one
// gather and one mean per proposal from Python) with
//
//   ball query   a uniform grid per segment (bbox -> one grid per segment, cell edge >= radius and at most CELLS_PER_POINT
//                cells per point -> cell counts -> one scan; a stable radix sort by cell keeps a cell's members in ascending
//                index), then a count pass, one scan and a fill pass over the 27 cells around a point: the output is sized
//                exactly.  One wavefront per point; its hits are sorted in LDS (4 KB).  A point with more than PG_BALL_CAP
//                hits keeps the PG_BALL_CAP lowest indices: the index bound below which exactly that many hits lie is found
//                by bisection;
//   clustering   union-find with atomicMin hooking (a parent is always the smaller index, so a root is the smallest member of
//                its tree), sizes by integer atomics on the root, numbering by one scan over the root flags;
//   proposals    one scan over the cluster sizes; masks and score partial sums per (proposal, chunk of 4096 points), the
//                partial sums added in a fixed order;
//   offset loss  block partial sums (fp64 arithmetic on the fp32 inputs), one finishing block in a fixed order.
//
// Squared distances use the pinned rounding sequence ref_d2() (common.h).  Integer atomics only.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <queue>
#include <vector>

#include "common.h"
#include "../../include/ptv2_pg_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int CELLS_PER_POINT = 4;  // as knn.hip: the cell tables are bounded by the number of points, never by the bounding box
constexpr int HIT_BUF = 1024;       // hits of one point held in LDS (>= PG_BALL_CAP, a power of two)
constexpr float EDGE_SLACK = 1.001f;  // cell edge >= radius * EDGE_SLACK: covers the fp32 rounding of a cell coordinate (grids <= 1024 per axis)

struct PgSeg {
    float minx, miny, minz, inv_h;
    int gx, gy, gz, cell_base;
};

struct BallWs {
    int *bbox_lo, *bbox_hi;  // [3b] ordered-int encoded
    PgSeg *seg;              // [b]
    int *cell_count;         // [ncell + 1]
    int *cell_start;         // [ncell + 1]
    int *keys_in, *keys_out, *vals_in, *order;  // [n]
    float4 *sorted;          // [n]: x, y, z, index, in (cell, index) order
    int *len, *start;        // [n + 1]
    void *cub;
    size_t cub_bytes, ncell, bytes;
};

int key_bits(size_t ncell) {
    int bits = 1;
    while (((size_t)1 << bits) < ncell + 1) ++bits;
    return bits;
}

BallWs carve_ball(void *base, int n, int b) {
    BallWs w;
    w.ncell = (size_t)CELLS_PER_POINT * n + b + 1;
    PtvCarver cv{(char *)base, 0};
    w.bbox_lo = cv.take_n<int>(3 * b); w.bbox_hi = cv.take_n<int>(3 * b);
    w.seg = cv.take_n<PgSeg>(b);
    w.cell_count = cv.take_n<int>(w.ncell + 1); w.cell_start = cv.take_n<int>(w.ncell + 1);
    w.keys_in = cv.take_n<int>(n); w.keys_out = cv.take_n<int>(n); w.vals_in = cv.take_n<int>(n); w.order = cv.take_n<int>(n);
    w.sorted = cv.take_n<float4>(n);
    w.len = cv.take_n<int>(n + 1); w.start = cv.take_n<int>(n + 1);
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, s1, (const int *)nullptr, (int *)nullptr, (const int *)nullptr, (int *)nullptr,
                                             n, 0, key_bits(w.ncell), (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s2, (const int *)nullptr, (int *)nullptr, (int)(w.ncell + 1), (hipStream_t)0);
    w.cub_bytes = std::max(s1, s2) + 256;
    w.cub = cv.take(w.cub_bytes);
    w.bytes = cv.off;
    return w;
}

// ---------------------------------------------------------------- the grid --
__global__ void pg_ball_init_kernel(int b, int *bbox_lo, int *bbox_hi, int *cell_count, int ncell1, int *len_last, int *capped) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 3 * b) {
        bbox_lo[t] = 0x7fffffff;
        bbox_hi[t] = (int)0x80000000;
    }
    if (t == 0) {
        *len_last = 0;
        if (capped) *capped = 0;
    }
    for (int i = t; i < ncell1; i += gridDim.x * blockDim.x) cell_count[i] = 0;
}

__global__ __launch_bounds__(TPB) void pg_ball_bbox_kernel(int n, const float *__restrict__ xyz, const int *__restrict__ ends, int b,
                                                           int *bbox_lo, int *bbox_hi) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    const bool valid = t < n;
    const int s = seg_of(valid ? t : n - 1, ends, b);
    const int s0 = __shfl(s, 0, WAVE), s63 = __shfl(s, 63, WAVE);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = xyz[3 * (size_t)(valid ? t : n - 1) + a];
        int lo = f2ord(v), hi = lo;
        if (s0 == s63) {  // the wavefront lies in one segment: two atomics per axis
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                lo = min(lo, __shfl_xor(lo, o, WAVE));
                hi = max(hi, __shfl_xor(hi, o, WAVE));
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMin(&bbox_lo[s * 3 + a], lo);
                atomicMax(&bbox_hi[s * 3 + a], hi);
            }
        } else {
            atomicMin(&bbox_lo[s * 3 + a], lo);
            atomicMax(&bbox_hi[s * 3 + a], hi);
        }
    }
}

// One thread per segment.  Segment s owns the cells [CELLS_PER_POINT * start_s + s, ...): at most CELLS_PER_POINT per point
// (one for an empty segment), so an outlier widens the cells and never the table.  Cells wider than the radius are fine: a
// query still visits the 27 cells around its own.
__global__ void pg_ball_grid_kernel(int n, int b, const int *__restrict__ offsets, const int *bbox_lo, const int *bbox_hi, float radius,
                                    PgSeg *seg) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= b) return;
    // (offsets that do not ascend from 0 to n give wrong lists, never a cell outside the table)
    const int start = min(max(offsets[s], 0), n), cnt = min(max(offsets[s + 1] - start, 0), n - start);
    PgSeg g;
    g.minx = g.miny = g.minz = 0.f;
    g.inv_h = 0.f;  // (every point in cell 0)
    g.gx = g.gy = g.gz = 1;
    g.cell_base = CELLS_PER_POINT * start + s;
    if (cnt > 0) {
        float lo[3], ext[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = ord2f(bbox_lo[s * 3 + a]);
            ext[a] = fmaxf(ord2f(bbox_hi[s * 3 + a]) - lo[a], 0.f);
        }
        const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
        float h = fmaxf(radius * EDGE_SLACK, emax * (1.f / 1000.f));
        bool ok = emax < 1e30f && h < 1e30f && h > 0.f && lo[0] > -1e30f && lo[1] > -1e30f && lo[2] > -1e30f;  // (false for NaN too)
        int gx = 1, gy = 1, gz = 1;
        if (ok) {
            ok = false;
            for (int it = 0; it < 1000; ++it) {
                gx = (int)fminf(floorf(ext[0] / h) + 1.f, 1024.f);
                gy = (int)fminf(floorf(ext[1] / h) + 1.f, 1024.f);
                gz = (int)fminf(floorf(ext[2] / h) + 1.f, 1024.f);
                if ((long long)gx * gy * gz <= (long long)cnt * CELLS_PER_POINT) { ok = true; break; }
                h *= 1.1f;
                if (!(h < 1e30f)) break;
            }
        }
        if (ok) {
            g.gx = gx; g.gy = gy; g.gz = gz;
            g.inv_h = 1.f / h;
            g.minx = lo[0]; g.miny = lo[1]; g.minz = lo[2];
        }
    }
    seg[s] = g;
}

__device__ __forceinline__ int pg_cell_coord(float v, float lo, float inv_h, int g) {
    float c = floorf((v - lo) * inv_h);
    c = fminf(fmaxf(c, 0.f), (float)(g - 1));  // (a NaN becomes cell 0)
    return (int)c;
}

__global__ __launch_bounds__(TPB) void pg_ball_cell_kernel(int n, const float *__restrict__ xyz, const int *__restrict__ ends, int b,
                                                           const PgSeg *__restrict__ seg, int *cell_count, int *keys, int *vals) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    const PgSeg g = seg[seg_of(t, ends, b)];
    const int cx = pg_cell_coord(xyz[3 * (size_t)t], g.minx, g.inv_h, g.gx);
    const int cy = pg_cell_coord(xyz[3 * (size_t)t + 1], g.miny, g.inv_h, g.gy);
    const int cz = pg_cell_coord(xyz[3 * (size_t)t + 2], g.minz, g.inv_h, g.gz);
    const int cell = g.cell_base + (cz * g.gy + cy) * g.gx + cx;
    keys[t] = cell;
    vals[t] = t;
    atomicAdd(&cell_count[cell], 1);
}

__global__ __launch_bounds__(TPB) void pg_ball_gather_kernel(int n, const float *__restrict__ xyz, const int *__restrict__ order,
                                                             float4 *sorted) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    const int i = order[t];
    sorted[t] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __int_as_float(i));
}

// ---------------------------------------------------------------- the query --
// One wavefront (one workgroup of 64) per point, points taken in cell order.  The 27 cells are 9 runs of up to three cells
// that are contiguous in the sorted copy; lane j of a trip takes candidate j of their concatenation.
template <bool FILL>
__global__ __launch_bounds__(WAVE) void pg_ball_query_kernel(int n, const float4 *__restrict__ sorted, const int *__restrict__ ends,
                                                             int b, const PgSeg *__restrict__ seg,
                                                             const int *__restrict__ cell_start, float r2, int *len, int *capped,
                                                             const int *__restrict__ start_len, long long n_active, int *idx) {
    __shared__ int s_p0[9], s_cnt[9], s_cum[10];
    __shared__ int s_hit[FILL ? HIT_BUF : 1];
    const int lane = threadIdx.x;
    const float4 q = sorted[blockIdx.x];
    const int pid = __float_as_int(q.w);
    const int s = seg_of(pid, ends, b);
    const PgSeg g = seg[s];
    const int cx = pg_cell_coord(q.x, g.minx, g.inv_h, g.gx);
    const int cy = pg_cell_coord(q.y, g.miny, g.inv_h, g.gy);
    const int cz = pg_cell_coord(q.z, g.minz, g.inv_h, g.gz);
    if (lane < 9) {
        const int z = cz + lane / 3 - 1, y = cy + lane % 3 - 1;
        int p0 = 0, p1 = 0;
        if (z >= 0 && z < g.gz && y >= 0 && y < g.gy) {
            const int row = g.cell_base + (z * g.gy + y) * g.gx;
            p0 = cell_start[row + max(cx - 1, 0)];
            p1 = cell_start[row + min(cx + 1, g.gx - 1) + 1];
        }
        p0 = min(max(p0, 0), n);
        p1 = min(max(p1, p0), n);
        s_p0[lane] = p0;
        s_cnt[lane] = p1 - p0;
    }
    __syncthreads();
    if (lane == 0) {
        int cum = 0;
        for (int i = 0; i < 9; ++i) { s_cum[i] = cum; cum += s_cnt[i]; }
        s_cum[9] = cum;
    }
    __syncthreads();
    const int total = s_cum[9];
    // the number of hits with index < limit (wave-uniform); `store`: the first HIT_BUF of them go to s_hit
    auto scan = [&](int limit, bool store) -> int {
        int H = 0;
        for (int j0 = 0; j0 < total; j0 += WAVE) {
            const int j = j0 + lane;
            bool hit = false;
            int id = 0;
            if (j < total) {
                int r = 0;
                while (r < 8 && j >= s_cum[r + 1]) ++r;
                const float4 c = sorted[s_p0[r] + j - s_cum[r]];
                id = __float_as_int(c.w);
                hit = ref_d2(q.x, q.y, q.z, c.x, c.y, c.z) < r2 && id < limit;
            }
            const unsigned long long mask = __ballot(hit);
            if (FILL && store && hit) {
                const int pos = H + __popcll(mask & ((1ull << lane) - 1ull));
                if (pos < HIT_BUF) s_hit[pos] = id;
            }
            H += __popcll(mask);
        }
        return H;
    };
    if (!FILL) {
        const int H = scan(0x7fffffff, false);
        if (lane == 0) {
            len[pid] = min(H, PG_BALL_CAP);
            if (H > PG_BALL_CAP) *capped = 1;  // (a plain store of the same value from every such point)
        }
        return;
    }
    int H = scan(0x7fffffff, true);
    if (H > HIT_BUF) {
        // more hits than the buffer holds: the smallest bound T with PG_BALL_CAP hits below it; exactly PG_BALL_CAP lie below
        // it (indices are distinct), the PG_BALL_CAP lowest
        int lo = 1, hi = n;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (scan(mid, false) >= PG_BALL_CAP) hi = mid; else lo = mid + 1;
        }
        __syncthreads();
        H = scan(lo, true);
    }
    const int m = min(H, HIT_BUF);
    int P = WAVE;
    while (P < m) P <<= 1;
    __syncthreads();
    for (int i = m + lane; i < P; i += WAVE) s_hit[i] = 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += WAVE) {
                const int o = i ^ j;
                if (o > i) {
                    const int a = s_hit[i], c = s_hit[o];
                    if ((a > c) == ((i & k) == 0)) { s_hit[i] = c; s_hit[o] = a; }
                }
            }
            __syncthreads();
        }
    const int start = start_len[2 * (size_t)pid];
    const int cnt = min(min(m, PG_BALL_CAP), start_len[2 * (size_t)pid + 1]);
    if (start < 0 || cnt < 0 || (long long)start + cnt > n_active) return;  // (a start_len that is not this query's)
    for (int i = lane; i < cnt; i += WAVE) idx[(size_t)start + i] = s_hit[i];
}

__global__ __launch_bounds__(TPB) void pg_ball_startlen_kernel(int n, const int *__restrict__ start, const int *__restrict__ len,
                                                               int *start_len, int *n_active) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t < n) {
        start_len[2 * (size_t)t] = start[t];
        start_len[2 * (size_t)t + 1] = len[t];
    }
    if (t == 0) *n_active = start[n];
}

bool ball_args_ok(int n, int b, const void *coords, const void *offsets, float radius) {
    return n >= 1 && n <= 0x7fffffff / (CELLS_PER_POINT + 1) - PG_MAX_CLOUDS - 2 && b >= 1 && b <= PG_MAX_CLOUDS && coords &&
           offsets && radius > 0.f && radius < 1e18f;
}

// ---------------------------------------------------------------- clustering --
struct ClusterWs {
    int *parent, *root, *size, *flag, *number;
    void *cub;
    size_t cub_bytes, bytes;
};

ClusterWs carve_cluster(void *base, int n) {
    ClusterWs w;
    PtvCarver cv{(char *)base, 0};
    w.parent = cv.take_n<int>(n); w.root = cv.take_n<int>(n); w.size = cv.take_n<int>(n);
    w.flag = cv.take_n<int>(n + 1); w.number = cv.take_n<int>(n + 1);
    size_t s = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s, (const int *)nullptr, (int *)nullptr, n + 1, (hipStream_t)0);
    w.cub_bytes = s + 256;
    w.cub = cv.take(w.cub_bytes);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(TPB) void pg_cluster_init_kernel(int n, int *parent, int *size) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t < n) {
        parent[t] = t;
        size[t] = 0;
    }
}

__device__ __forceinline__ int pg_find(int *parent, int x) {
    int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

// parent[x] <= x always, so there is no cycle and a root is the smallest index of its tree.  atomicMin(parent[a], b) with b < a
// either hooks the root a under b, or finds a already hooked under some c: a then hangs under min(b, c) and the union goes on
// with c and b, so no link is lost.
__device__ __forceinline__ void pg_unite(int *parent, int a, int b) {
    for (;;) {
        a = pg_find(parent, a);
        b = pg_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// one wavefront per point; an edge is taken from its larger end (without a cut list the relation is symmetric)
__global__ __launch_bounds__(TPB) void pg_cluster_hook_kernel(int n, const int *__restrict__ label, const int *__restrict__ idx,
                                                              const int *__restrict__ start_len, long long n_active, int *parent) {
    const int p = blockIdx.x * (TPB / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n) return;
    const int start = start_len[2 * (size_t)p], len = start_len[2 * (size_t)p + 1];
    if (start < 0 || len < 0 || (long long)start + len > n_active) return;
    const int lp = label[p];
    for (int i = lane; i < len; i += WAVE) {
        const int k = idx[(size_t)start + i];
        if (k >= 0 && k < p && label[k] == lp) pg_unite(parent, p, k);
    }
}

__global__ __launch_bounds__(TPB) void pg_cluster_root_kernel(int n, int *parent, int *root, int *size) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    const int r = pg_find(parent, t);
    root[t] = r;
    atomicAdd(size + r, 1);
}

__global__ __launch_bounds__(TPB) void pg_cluster_flag_kernel(int n, const int *__restrict__ root, const int *__restrict__ size,
                                                              int min_points, int *flag) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t < n) flag[t] = (root[t] == t && size[t] >= min_points) ? 1 : 0;
    if (t == n) flag[t] = 0;
}

__global__ __launch_bounds__(TPB) void pg_cluster_number_kernel(int n, const int *__restrict__ root, const int *__restrict__ size,
                                                                const int *__restrict__ flag, const int *__restrict__ number,
                                                                int *point_cluster, int *cluster_size, int *cluster_first,
                                                                int *n_cluster) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    const int r = root[t];
    point_cluster[t] = flag[r] ? number[r] : -1;
    if (flag[t]) {
        cluster_size[number[t]] = size[t];
        cluster_first[number[t]] = t;
    }
    if (t == 0) *n_cluster = number[n];
}

// ---------------------------------------------------------------- proposals --
constexpr int CHUNK_ITEMS = 16, CHUNK = TPB * CHUNK_ITEMS;

struct PropWs {
    int *flag, *number, *cluster_of;
    float *partial;
    void *cub;
    size_t cub_bytes, bytes;
};

PropWs carve_prop(void *base, long long n, long long n_cluster) {
    PropWs w;
    PtvCarver cv{(char *)base, 0};
    w.flag = cv.take_n<int>(n_cluster + 1); w.number = cv.take_n<int>(n_cluster + 1); w.cluster_of = cv.take_n<int>(n_cluster + 1);
    w.partial = cv.take_n<float>((size_t)(n_cluster + 1) * divup(n > 0 ? n : 1, CHUNK));
    size_t s = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s, (const int *)nullptr, (int *)nullptr, (int)n_cluster + 1, (hipStream_t)0);
    w.cub_bytes = s + 256;
    w.cub = cv.take(w.cub_bytes);
    w.bytes = cv.off;
    return w;
}

__global__ __launch_bounds__(TPB) void pg_prop_flag_kernel(int nc, const int *__restrict__ cluster_size, int propose_points, int *flag) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t < nc) flag[t] = cluster_size[t] > propose_points ? 1 : 0;
    if (t == nc) flag[t] = 0;
}

__global__ __launch_bounds__(TPB) void pg_prop_number_kernel(int nc, const int *__restrict__ flag, const int *__restrict__ number,
                                                             int *proposal_of_cluster, int *n_proposal) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t < nc) proposal_of_cluster[t] = flag[t] ? number[t] : -1;
    if (t == 0) *n_proposal = number[nc];
}

__global__ __launch_bounds__(TPB) void pg_prop_inverse_kernel(int nc, int np, const int *__restrict__ proposal_of_cluster, int *cluster_of) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= nc) return;
    const int j = proposal_of_cluster[t];
    if (j >= 0 && j < np) cluster_of[j] = t;
}

__device__ __forceinline__ float pg_block_sum(float v, float *s_red) {  // the same tree for the same block size
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int o = TPB / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
        __syncthreads();
    }
    const float r = s_red[0];
    __syncthreads();
    return r;
}

// grid (chunks, proposals): the mask of 4096 points and the sum of their members' class probabilities
__global__ __launch_bounds__(TPB) void pg_prop_chunk_kernel(int n, int c, int nc, const int *__restrict__ point_cluster,
                                                            const int *__restrict__ cluster_first,
                                                            const int *__restrict__ cluster_of,
                                                            const long long *__restrict__ segment_pred,
                                                            const float *__restrict__ prob, int is_logit, int *masks, float *partial) {
    __shared__ float s_red[TPB];
    const int j = blockIdx.y, cl = cluster_of[j];
    int first = (cl >= 0 && cl < nc) ? cluster_first[cl] : 0;
    first = min(max(first, 0), n - 1);
    const long long cls_ll = segment_pred[first];
    const bool cls_ok = cls_ll >= 0 && cls_ll < c;
    const int cls = cls_ok ? (int)cls_ll : 0;
    float acc = 0.f;
    for (int u = 0; u < CHUNK_ITEMS; ++u) {
        const long long i = (long long)blockIdx.x * CHUNK + u * TPB + threadIdx.x;
        if (i >= n) break;
        const bool member = point_cluster[i] == cl;
        masks[(size_t)j * n + i] = member ? 1 : 0;
        if (member) {
            const float *row = prob + (size_t)i * c;
            float v = row[cls];
            if (is_logit) {
                float mx = row[0];
                for (int k = 1; k < c; ++k) mx = fmaxf(mx, row[k]);
                float sum = 0.f;
                for (int k = 0; k < c; ++k) sum += expf(row[k] - mx);
                v = expf(v - mx) / sum;
            }
            acc += cls_ok ? v : __int_as_float(0x7fc00000);
        }
    }
    const float total = pg_block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[(size_t)j * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(TPB) void pg_prop_finish_kernel(int n, int nc, int nchunk, const int *__restrict__ cluster_size,
                                                             const int *__restrict__ cluster_first,
                                                             const int *__restrict__ cluster_of,
                                                             const long long *__restrict__ segment_pred,
                                                             const float *__restrict__ partial, long long *classes, float *scores) {
    __shared__ float s_red[TPB];
    const int j = blockIdx.x, cl = cluster_of[j];
    float acc = 0.f;
    for (int k = threadIdx.x; k < nchunk; k += TPB) acc += partial[(size_t)j * nchunk + k];
    const float total = pg_block_sum(acc, s_red);
    if (threadIdx.x == 0) {
        const bool ok = cl >= 0 && cl < nc;
        const int first = ok ? min(max(cluster_first[cl], 0), n - 1) : 0;
        classes[j] = segment_pred[first];
        scores[j] = total / (float)(ok ? cluster_size[cl] : 0);
    }
}

// ---------------------------------------------------------------- offset loss --
constexpr int LOSS_BLOCKS = 1024;
constexpr double LOSS_EPS = 1e-8;

// The arithmetic of a row runs in fp64 on the fp32 inputs (the kernels are bound by their loads; the fp64 rate of the MI355X
// makes this free), so a loss or a gradient element is the correctly rounded fp32 of the exact statement to within one rounding
// of the upstream fp32 scalars: no cancellation between the L1 and the cosine term shows in the result.
struct BiasRow {
    double p[3], gt[3];
    bool used;
};

__device__ __forceinline__ BiasRow pg_bias_row(int i, const float *__restrict__ bias_pred, const float *__restrict__ coord,
                                               const float *__restrict__ center, const long long *__restrict__ instance,
                                               long long ignore) {
    BiasRow r;
    r.used = instance[i] != ignore;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.p[a] = (double)bias_pred[3 * (size_t)i + a];
        r.gt[a] = (double)center[3 * (size_t)i + a] - (double)coord[3 * (size_t)i + a];
    }
    return r;
}

__device__ __forceinline__ double pg_norm3(const double *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

__device__ __forceinline__ double pg_block_sum_f64(double v, double *s_red) {
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int o = TPB / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = s_red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(TPB) void pg_bias_partial_kernel(int n, const float *__restrict__ bias_pred, const float *__restrict__ coord,
                                                              const float *__restrict__ center,
                                                              const long long *__restrict__ instance, long long ignore,
                                                              double *partial) {
    __shared__ double s_red[TPB];
    double l1 = 0.0, cs = 0.0, cnt = 0.0;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        const BiasRow r = pg_bias_row((int)i, bias_pred, coord, center, instance, ignore);
        if (!r.used) continue;
        const double np = pg_norm3(r.p) + LOSS_EPS, ng = pg_norm3(r.gt) + LOSS_EPS;
        l1 += fabs(r.p[0] - r.gt[0]) + fabs(r.p[1] - r.gt[1]) + fabs(r.p[2] - r.gt[2]);
        cs -= (r.p[0] / np) * (r.gt[0] / ng) + (r.p[1] / np) * (r.gt[1] / ng) + (r.p[2] / np) * (r.gt[2] / ng);
        cnt += 1.0;
    }
    l1 = pg_block_sum_f64(l1, s_red);
    cs = pg_block_sum_f64(cs, s_red);
    cnt = pg_block_sum_f64(cnt, s_red);
    if (threadIdx.x == 0) {
        partial[3 * (size_t)blockIdx.x] = l1;
        partial[3 * (size_t)blockIdx.x + 1] = cs;
        partial[3 * (size_t)blockIdx.x + 2] = cnt;
    }
}

__global__ __launch_bounds__(TPB) void pg_bias_finish_kernel(int nb, const double *__restrict__ partial, float *out) {
    __shared__ double s_red[TPB];
    double v[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nb; k += TPB)
        for (int a = 0; a < 3; ++a) v[a] += partial[3 * (size_t)k + a];
    for (int a = 0; a < 3; ++a) v[a] = pg_block_sum_f64(v[a], s_red);
    if (threadIdx.x == 0) {
        out[0] = (float)(v[0] / (v[2] + LOSS_EPS));
        out[1] = (float)(v[1] / (v[2] + LOSS_EPS));
        out[2] = (float)v[2];
    }
}

__global__ __launch_bounds__(TPB) void pg_bias_bwd_kernel(int n, const float *__restrict__ bias_pred, const float *__restrict__ coord,
                                                          const float *__restrict__ center, const long long *__restrict__ instance,
                                                          long long ignore, const float *__restrict__ out, const float *__restrict__ g,
                                                          float *d_bias_pred) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const BiasRow r = pg_bias_row(i, bias_pred, coord, center, instance, ignore);
    double d[3] = {0.0, 0.0, 0.0};
    if (r.used) {
        const double denom = (double)out[2] + LOSS_EPS;
        const double g1 = (double)g[0] / denom, g2 = (double)g[1] / denom;
        const double np = pg_norm3(r.p), ng = pg_norm3(r.gt) + LOSS_EPS;
        const double a = np + LOSS_EPS;
        const double gn[3] = {r.gt[0] / ng, r.gt[1] / ng, r.gt[2] / ng};
        const double dot = r.p[0] * gn[0] + r.p[1] * gn[1] + r.p[2] * gn[2];
        // d/dp of p . gn / (|p| + eps): gn / a - (p . gn) (p / |p|) / a^2; the gradient of |p| at p = 0 is 0
        const double back = np > 0.0 ? dot / (np * a * a) : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double diff = r.p[k] - r.gt[k];
            const double sgn = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
            d[k] = g1 * sgn - g2 * (gn[k] / a - back * r.p[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) d_bias_pred[3 * (size_t)i + k] = (float)d[k];
}

}  // namespace

extern "C" int ptv2_pg_abi_version(void) { return 1; }
extern "C" int ptv2_pg_struct_bytes(int which) { return which == 0 ? (int)sizeof(pg_csr) : -1; }

extern "C" long long ptv2_pg_ballquery_workspace_bytes(long long n, int b) {
    if (n < 1 || n > 0x7fffffff / (CELLS_PER_POINT + 1) - PG_MAX_CLOUDS - 2 || b < 1 || b > PG_MAX_CLOUDS) return -1;
    return (long long)carve_ball(nullptr, (int)n, b).bytes + 1024;
}

extern "C" int pg_ballquery_count_hip_launcher(int n, int b, const float *coords, const int *batch_offsets, float radius,
                                               int *start_len, int *n_active, int *capped, void *workspace,
                                               long long workspace_bytes, void *stream) {
    if (!ball_args_ok(n, b, coords, batch_offsets, radius) || !start_len || !n_active || !capped) return PTV2_ERR_ARG;
    BallWs w = carve_ball(workspace, n, b);
    if (!workspace || workspace_bytes < (long long)w.bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = divup(n, TPB), ncell1 = (int)w.ncell + 1;
    const int *ends = batch_offsets + 1;
    hipLaunchKernelGGL(pg_ball_init_kernel, dim3(std::min(divup(ncell1, TPB), 4096)), dim3(TPB), 0, st, b, w.bbox_lo, w.bbox_hi,
                       w.cell_count, ncell1, w.len + n, capped);
    hipLaunchKernelGGL(pg_ball_bbox_kernel, dim3(nb), dim3(TPB), 0, st, n, coords, ends, b, w.bbox_lo, w.bbox_hi);
    hipLaunchKernelGGL(pg_ball_grid_kernel, dim3(divup(b, 64)), dim3(64), 0, st, n, b, batch_offsets, (const int *)w.bbox_lo,
                       (const int *)w.bbox_hi, radius, w.seg);
    hipLaunchKernelGGL(pg_ball_cell_kernel, dim3(nb), dim3(TPB), 0, st, n, coords, ends, b, (const PgSeg *)w.seg, w.cell_count,
                       w.keys_in, w.vals_in);
    size_t cb = w.cub_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(w.cub, cb, (const int *)w.cell_count, w.cell_start, ncell1, st) != hipSuccess)
        return PTV2_ERR_LAUNCH;
    cb = w.cub_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, (const int *)w.keys_in, w.keys_out, (const int *)w.vals_in, w.order, n, 0,
                                           key_bits(w.ncell), st) != hipSuccess)
        return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(pg_ball_gather_kernel, dim3(nb), dim3(TPB), 0, st, n, coords, (const int *)w.order, w.sorted);
    hipLaunchKernelGGL(pg_ball_query_kernel<false>, dim3(n), dim3(WAVE), 0, st, n, (const float4 *)w.sorted, ends, b,
                       (const PgSeg *)w.seg, (const int *)w.cell_start, radius * radius, w.len, capped, (const int *)nullptr, 0LL,
                       (int *)nullptr);
    cb = w.cub_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(w.cub, cb, (const int *)w.len, w.start, n + 1, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(pg_ball_startlen_kernel, dim3(nb), dim3(TPB), 0, st, n, (const int *)w.start, (const int *)w.len, start_len,
                       n_active);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pg_ballquery_fill_hip_launcher(int n, int b, const float *coords, const int *batch_offsets, float radius,
                                              const int *start_len, long long n_active, int *idx, void *workspace,
                                              long long workspace_bytes, void *stream) {
    if (!ball_args_ok(n, b, coords, batch_offsets, radius) || !start_len || n_active < 0 || (n_active > 0 && !idx))
        return PTV2_ERR_ARG;
    BallWs w = carve_ball(workspace, n, b);
    if (!workspace || workspace_bytes < (long long)w.bytes) return PTV2_ERR_WORKSPACE;
    if (n_active == 0) return PTV2_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pg_ball_query_kernel<true>, dim3(n), dim3(WAVE), 0, st, n, (const float4 *)w.sorted, batch_offsets + 1, b,
                       (const PgSeg *)w.seg, (const int *)w.cell_start, radius * radius, (int *)nullptr, (int *)nullptr, start_len,
                       n_active, idx);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" long long ptv2_pg_cluster_workspace_bytes(long long n) {
    if (n < 1 || n > 0x7ffffff0) return -1;
    return (long long)carve_cluster(nullptr, (int)n).bytes + 1024;
}

extern "C" int pg_cluster_hip_launcher(int n, const int *semantic_label, const pg_csr *csr, int min_points, int *point_cluster,
                                       int *cluster_size, int *cluster_first, int *n_cluster, void *workspace,
                                       long long workspace_bytes, void *stream) {
    if (n < 1 || n > 0x7ffffff0 || !semantic_label || !csr || !csr->start_len || csr->n_active < 0 ||
        (csr->n_active > 0 && !csr->idx) || !point_cluster || !cluster_size || !cluster_first || !n_cluster)
        return PTV2_ERR_ARG;
    ClusterWs w = carve_cluster(workspace, n);
    if (!workspace || workspace_bytes < (long long)w.bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = divup(n, TPB);
    hipLaunchKernelGGL(pg_cluster_init_kernel, dim3(nb), dim3(TPB), 0, st, n, w.parent, w.size);
    hipLaunchKernelGGL(pg_cluster_hook_kernel, dim3(divup(n, TPB / WAVE)), dim3(TPB), 0, st, n, semantic_label,
                       (const int *)csr->idx, (const int *)csr->start_len, csr->n_active, w.parent);
    hipLaunchKernelGGL(pg_cluster_root_kernel, dim3(nb), dim3(TPB), 0, st, n, w.parent, w.root, w.size);
    hipLaunchKernelGGL(pg_cluster_flag_kernel, dim3(divup(n + 1, TPB)), dim3(TPB), 0, st, n, (const int *)w.root,
                       (const int *)w.size, min_points, w.flag);
    size_t cb = w.cub_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(w.cub, cb, (const int *)w.flag, w.number, n + 1, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(pg_cluster_number_kernel, dim3(nb), dim3(TPB), 0, st, n, (const int *)w.root, (const int *)w.size,
                       (const int *)w.flag, (const int *)w.number, point_cluster, cluster_size, cluster_first, n_cluster);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// Written from the semantics in the header: seeds in ascending index; a first-in first-out queue; the entries of the current
// point's list in list order; an entry joins when it carries the current point's label and has not been visited by any search.
extern "C" long long pg_bfs_cluster_host(int n, const int *semantic_label, const pg_csr *csr, int threshold, int *cluster_idxs,
                                         int *cluster_offsets, int *n_cluster) {
    if (n < 0 || !csr || csr->n_active < 0 || !cluster_offsets || !n_cluster) return -1;
    if (n > 0 && (!semantic_label || !csr->start_len || !cluster_idxs || (csr->n_active > 0 && !csr->idx))) return -1;
    const int *idx = csr->idx, *start_len = csr->start_len;
    for (int p = 0; p < n; ++p) {
        const long long start = start_len[2 * (size_t)p], len = start_len[2 * (size_t)p + 1];
        if (start < 0 || len < 0 || start + len > csr->n_active) return -1;
    }
    for (long long e = 0; e < csr->n_active; ++e)
        if (idx[e] < 0 || idx[e] >= n) return -1;
    std::vector<char> visited((size_t)n, 0);
    std::vector<int> found;
    long long rows = 0;
    int clusters = 0;
    cluster_offsets[0] = 0;
    for (int seed = 0; seed < n; ++seed) {
        if (visited[seed]) continue;
        found.clear();
        std::queue<int> todo;
        visited[seed] = 1;
        found.push_back(seed);
        todo.push(seed);
        while (!todo.empty()) {
            const int cur = todo.front();
            todo.pop();
            const int *list = idx + start_len[2 * (size_t)cur];
            const int len = start_len[2 * (size_t)cur + 1], lab = semantic_label[cur];
            for (int i = 0; i < len; ++i) {
                const int k = list[i];
                if (visited[k] || semantic_label[k] != lab) continue;
                visited[k] = 1;
                found.push_back(k);
                todo.push(k);
            }
        }
        if ((long long)found.size() < threshold) continue;
        for (size_t i = 0; i < found.size(); ++i) {
            cluster_idxs[2 * (size_t)(rows + (long long)i)] = clusters;
            cluster_idxs[2 * (size_t)(rows + (long long)i) + 1] = found[i];
        }
        rows += (long long)found.size();
        cluster_offsets[++clusters] = (int)rows;
    }
    *n_cluster = clusters;
    return rows;
}

extern "C" long long ptv2_pg_proposals_workspace_bytes(long long n, long long n_cluster) {
    if (n < 1 || n > 0x7ffffff0 || n_cluster < 0 || n_cluster > n) return -1;
    return (long long)carve_prop(nullptr, n, n_cluster).bytes + 1024;
}

extern "C" int pg_proposals_count_hip_launcher(int n_cluster, const int *cluster_size, int propose_points,
                                               int *proposal_of_cluster, int *n_proposal, void *workspace,
                                               long long workspace_bytes, void *stream) {
    if (n_cluster < 0 || n_cluster > 0x7ffffff0 || !n_proposal || (n_cluster > 0 && (!cluster_size || !proposal_of_cluster)))
        return PTV2_ERR_ARG;
    PropWs w = carve_prop(workspace, 1, n_cluster);
    if (!workspace || workspace_bytes < (long long)w.bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = divup(n_cluster + 1, TPB);
    hipLaunchKernelGGL(pg_prop_flag_kernel, dim3(nb), dim3(TPB), 0, st, n_cluster, cluster_size, propose_points, w.flag);
    size_t cb = w.cub_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(w.cub, cb, (const int *)w.flag, w.number, n_cluster + 1, st) != hipSuccess)
        return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(pg_prop_number_kernel, dim3(nb), dim3(TPB), 0, st, n_cluster, (const int *)w.flag, (const int *)w.number,
                       proposal_of_cluster, n_proposal);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pg_proposals_fill_hip_launcher(int n, int c, int n_cluster, int n_proposal, const int *point_cluster,
                                              const int *cluster_size, const int *cluster_first, const int *proposal_of_cluster,
                                              const long long *segment_pred, const float *prob, int is_logit, long long *classes,
                                              float *scores, int *masks, void *workspace, long long workspace_bytes, void *stream) {
    if (n < 1 || n > 0x7ffffff0 || c < 1 || c > PG_MAX_CLASSES || n_cluster < 0 || n_cluster > n || n_proposal < 0 ||
        n_proposal > n_cluster || n_proposal > 65535)
        return PTV2_ERR_ARG;
    if (n_proposal == 0) return PTV2_OK;
    if (!point_cluster || !cluster_size || !cluster_first || !proposal_of_cluster || !segment_pred || !prob || !classes || !scores ||
        !masks)
        return PTV2_ERR_ARG;
    PropWs w = carve_prop(workspace, n, n_cluster);
    if (!workspace || workspace_bytes < (long long)w.bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = divup(n, CHUNK);
    hipLaunchKernelGGL(pg_prop_inverse_kernel, dim3(divup(n_cluster, TPB)), dim3(TPB), 0, st, n_cluster, n_proposal,
                       proposal_of_cluster, w.cluster_of);
    hipLaunchKernelGGL(pg_prop_chunk_kernel, dim3(nchunk, n_proposal), dim3(TPB), 0, st, n, c, n_cluster, point_cluster,
                       cluster_first, (const int *)w.cluster_of, segment_pred, prob, is_logit, masks, w.partial);
    hipLaunchKernelGGL(pg_prop_finish_kernel, dim3(n_proposal), dim3(TPB), 0, st, n, n_cluster, nchunk, cluster_size, cluster_first,
                       (const int *)w.cluster_of, segment_pred, (const float *)w.partial, classes, scores);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" long long ptv2_pg_bias_loss_workspace_bytes(long long n) {
    if (n < 1 || n > 0x7ffffff0 / 3) return -1;
    return (long long)ptv2_align256(sizeof(double) * 3 * LOSS_BLOCKS) + 256;
}

extern "C" int pg_bias_loss_fwd_hip_launcher(int n, const float *bias_pred, const float *coord, const float *instance_center,
                                             const long long *instance, long long ignore, float *out, void *workspace,
                                             long long workspace_bytes, void *stream) {
    if (n < 1 || n > 0x7ffffff0 / 3 || !bias_pred || !coord || !instance_center || !instance || !out) return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < ptv2_pg_bias_loss_workspace_bytes(n)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = std::min(divup(n, TPB), LOSS_BLOCKS);
    hipLaunchKernelGGL(pg_bias_partial_kernel, dim3(nb), dim3(TPB), 0, st, n, bias_pred, coord, instance_center, instance, ignore,
                       (double *)workspace);
    hipLaunchKernelGGL(pg_bias_finish_kernel, dim3(1), dim3(TPB), 0, st, nb, (const double *)workspace, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pg_bias_loss_bwd_hip_launcher(int n, const float *bias_pred, const float *coord, const float *instance_center,
                                             const long long *instance, long long ignore, const float *out, const float *g,
                                             float *d_bias_pred, void *stream) {
    if (n < 1 || n > 0x7ffffff0 / 3 || !bias_pred || !coord || !instance_center || !instance || !out || !g || !d_bias_pred)
        return PTV2_ERR_ARG;
    hipLaunchKernelGGL(pg_bias_bwd_kernel, dim3(divup(n, TPB)), dim3(TPB), 0, (hipStream_t)stream, n, bias_pred, coord,
                       instance_center, instance, ignore, out, g, d_bias_pred);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
