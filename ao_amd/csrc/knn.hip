// ao_amd/csrc/knn.hip -- exact batched k-NN for gfx950 (MI355X).
//
// Replaces the reference's brute-force one-thread-per-query kernel
// (libs/pointops/src/knn_query/knn_query_cuda_kernel.cu:60-104) with
//
//   1. a per-call uniform grid over each batch segment of xyz (counting sort by cell:
//      bbox -> grid set-up + count + rank (one launch) -> one chained exclusive scan -> scatter),
//      everything on device, no host sync;
//   2. a grid query: one lane per query, neighbour cells visited in Chebyshev rings,
//      candidates read as float4 (x,y,z,id) from the cell-sorted copy, the KC = k+1
//      best kept sorted in registers; a ring search stops when the KC-th best squared
//      distance is provably smaller than anything outside the rings visited;
//   3. tie detection: the reference result is "the k smallest, ascending" whenever the
//      k+1 smallest squared distances of a query are pairwise distinct (SURVEY.md 8a,
//      tests/test_oracle_ops.py::test_knn_tie_rule_is_sufficient).  Queries that fail that
//      test are appended to a list and
//   4. re-run by an exact emulation of the reference's max-heap (reheap :15-30,
//      heap_sort :33-42, ascending index scan with strict `d2 < heap max` :88-97): one
//      wavefront per query, 64 candidates per step filtered with a ballot against the
//      current heap root, survivors pushed in index order.  Bit-identical by construction.
//
// Squared distances use the pinned rounding sequence ref_d2() (common.h).
#include <cstdlib>

#include "common.h"

namespace {

struct SegGrid {
    float minx, miny, minz, h, inv_h;
    int gx, gy, gz, cell_base, n_pts, start;
    int pad;
};

struct Workspace {
    int *tie_count;      // [1]
    int *bbox_lo;        // [3b] ordered-int encoded
    int *bbox_hi;        // [3b]
    SegGrid *seg;        // [b]
    int *block_sums;     // [scan blocks]
    int *cell_count;     // [ncell]
    int *cell_start;     // [ncell + 1]
    int *point_cell;     // [n]
    int *point_rank;     // [n]
    float4 *sorted;      // [n]
    int *tie_list;       // [m]
    size_t bytes;
};

// cells per point the grid may use: a segment of cnt points gets at most CELLS_PER_POINT * cnt cells (surface clouds leave
// most cells of their bounding volume empty: finer cells -> fewer candidates per query; the cell tables are 4 B per cell)
constexpr int CELLS_PER_POINT = 4;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_TILE = SCAN_ITEMS * SCAN_THREADS;

Workspace carve(void *base, int m, int n, int b) {
    Workspace w;
    size_t ncell = (size_t)CELLS_PER_POINT * n + b + 1;
    size_t ncell_pad = (size_t)divup(ncell + 1, SCAN_TILE) * SCAN_TILE;
    PtvCarver cv{(char *)base, 0};
    w.tie_count = cv.take_n<int>(4);
    w.bbox_lo = cv.take_n<int>(3 * b); w.bbox_hi = cv.take_n<int>(3 * b);
    w.seg = cv.take_n<SegGrid>(b);
    w.block_sums = cv.take_n<int>(ncell_pad / SCAN_TILE + 1);
    w.cell_count = cv.take_n<int>(ncell_pad); w.cell_start = cv.take_n<int>(ncell_pad + 1);
    w.point_cell = cv.take_n<int>(n); w.point_rank = cv.take_n<int>(n);
    w.sorted = cv.take_n<float4>(n);
    w.tie_list = cv.take_n<int>(m > 0 ? m : 1);
    w.bytes = cv.off;
    return w;
}

// ---------------------------------------------------------------- grid build --
__global__ void knn_init_kernel(int *tie_count, int *bbox_lo, int *bbox_hi, int b, int *cell_count,
                                int ncell_pad, int *block_sums, int ntiles) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    for (int i = t; i < ntiles; i += gridDim.x * blockDim.x) block_sums[i] = 0;  // (the scan's hand-off words)
    if (t < 4) tie_count[t] = 0;  // (one re-run list counter per query that shares this grid)
    if (t < 3 * b) {
        bbox_lo[t] = 0x7fffffff;
        bbox_hi[t] = (int)0x80000000;
    }
    for (int i = t; i < ncell_pad; i += gridDim.x * blockDim.x) cell_count[i] = 0;
}

__global__ __launch_bounds__(256) void knn_bbox_kernel(int n, const float *__restrict__ xyz,
                                                       const int *__restrict__ offset, int b,
                                                       int *bbox_lo, int *bbox_hi) {
    __shared__ int s_lo[3], s_hi[3];
    int t = blockIdx.x * 256 + threadIdx.x;
    int first = blockIdx.x * 256, last = min(first + 255, n - 1);
    int seg_first = seg_of(first, offset, b), seg_last = seg_of(last, offset, b);
    bool valid = t < n;
    float x = 0, y = 0, z = 0;
    if (valid) {
        x = xyz[3 * t];
        y = xyz[3 * t + 1];
        z = xyz[3 * t + 2];
    }
    if (seg_first == seg_last) {  // block lies in one segment: LDS reduce, 6 atomics per block
        if (threadIdx.x < 3) {
            s_lo[threadIdx.x] = 0x7fffffff;
            s_hi[threadIdx.x] = (int)0x80000000;
        }
        __syncthreads();
        float v[3] = {x, y, z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int lo = valid ? f2ord(v[a]) : 0x7fffffff, hi = valid ? f2ord(v[a]) : (int)0x80000000;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                lo = min(lo, __shfl_xor(lo, o, WAVE));
                hi = max(hi, __shfl_xor(hi, o, WAVE));
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMin(&s_lo[a], lo);
                atomicMax(&s_hi[a], hi);
            }
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            atomicMin(&bbox_lo[seg_first * 3 + threadIdx.x], s_lo[threadIdx.x]);
            atomicMax(&bbox_hi[seg_first * 3 + threadIdx.x], s_hi[threadIdx.x]);
        }
    } else if (valid) {  // block straddles a segment boundary (at most b-1 such blocks)
        int s = seg_of(t, offset, b);
        atomicMin(&bbox_lo[s * 3 + 0], f2ord(x));
        atomicMax(&bbox_hi[s * 3 + 0], f2ord(x));
        atomicMin(&bbox_lo[s * 3 + 1], f2ord(y));
        atomicMax(&bbox_hi[s * 3 + 1], f2ord(y));
        atomicMin(&bbox_lo[s * 3 + 2], f2ord(z));
        atomicMax(&bbox_hi[s * 3 + 2], f2ord(z));
    }
}

__device__ __forceinline__ int cell_coord(float v, float lo, float inv_h, int g) {
    float c = floorf((v - lo) * inv_h);
    c = fminf(fmaxf(c, 0.f), (float)(g - 1));
    return (int)c;
}

// The grid of one segment: the cell size is chosen so that cells <= CELLS_PER_POINT * points (then the cell tables of all
// segments fit CELLS_PER_POINT * n + b + 1 entries and segment s owns [CELLS_PER_POINT * start_s + s, ...)).
__device__ __forceinline__ SegGrid seg_grid_of(int s, const int *__restrict__ offset, const int *bbox_lo, const int *bbox_hi,
                                               float occupancy) {
    int start = s == 0 ? 0 : offset[s - 1];
    int cnt = offset[s] - start;
    SegGrid g;
    g.start = start;
    g.n_pts = cnt > 0 ? cnt : 0;
    g.cell_base = CELLS_PER_POINT * start + s;
    g.gx = g.gy = g.gz = 1;
    g.minx = g.miny = g.minz = 0.f;
    g.h = 1.f;
    g.inv_h = 1.f;
    g.pad = 0;
    if (cnt > 0) {
        float lo[3], ext[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = ord2f(bbox_lo[s * 3 + a]);
            ext[a] = fmaxf(ord2f(bbox_hi[s * 3 + a]) - lo[a], 0.f);
        }
        float emax = fmaxf(fmaxf(ext[0], ext[1]), fmaxf(ext[2], 1e-12f));
        // volume with degenerate axes floored at 1/64 of the largest extent (planar / linear clouds)
        float vol = 1.f;
        for (int a = 0; a < 3; ++a) vol *= fmaxf(ext[a], emax * (1.f / 64.f));
        float h = cbrtf(vol * occupancy / (float)cnt);
        h = fmaxf(h, emax * (1.f / 1000.f));
        int gx, gy, gz;
        for (int it = 0; it < 200; ++it) {
            gx = (int)fminf(floorf(ext[0] / h) + 1.f, 1024.f);
            gy = (int)fminf(floorf(ext[1] / h) + 1.f, 1024.f);
            gz = (int)fminf(floorf(ext[2] / h) + 1.f, 1024.f);
            if ((long long)gx * gy * gz <= (long long)cnt * CELLS_PER_POINT) break;
            h *= 1.08f;
        }
        if ((long long)gx * gy * gz > (long long)cnt * CELLS_PER_POINT) { gx = gy = gz = 1; h = emax * 2.f + 1.f; }
        g.gx = gx; g.gy = gy; g.gz = gz;
        g.h = h;
        g.inv_h = 1.f / h;
        g.minx = lo[0]; g.miny = lo[1]; g.minz = lo[2];
    }
    return g;
}

// Grid set-up + count in one launch (round 5: the set-up was a one-thread-per-segment launch of its own, 5 us of boundary in
// front of this one).  The bounding boxes are final when this kernel starts; a workgroup derives the grids of the segments
// ITS 256 points lie in (one thread per segment: usually one or two) into LDS, every thread then bins its point.  The grid a
// segment's queries read later (seg[s]) is stored by the workgroup that holds the segment's first point; workgroup 0 stores
// the grids of the empty segments (a cross query may still name them).
constexpr int COUNT_SEGS = 64;  // segments of one workgroup's points held in LDS; more (clouds of < 4 points) fall back to global
__global__ __launch_bounds__(256) void knn_cell_count_kernel(int n, const float *__restrict__ xyz,
                                                             const int *__restrict__ offset, int b,
                                                             const int *bbox_lo, const int *bbox_hi, float occupancy,
                                                             SegGrid *seg, int *cell_count, int *point_cell,
                                                             int *point_rank) {
    __shared__ SegGrid s_grid[COUNT_SEGS];
    const int first = blockIdx.x * 256, last = min(first + 255, n - 1);
    const int s0 = seg_of(first, offset, b), s1 = seg_of(last, offset, b);
    for (int s = s0 + (int)threadIdx.x; s <= s1; s += 256) {
        const SegGrid g = seg_grid_of(s, offset, bbox_lo, bbox_hi, occupancy);
        if (s - s0 < COUNT_SEGS) s_grid[s - s0] = g;
        if (g.n_pts > 0 && g.start >= first) seg[s] = g;  // (exactly one workgroup holds a non-empty segment's first point)
    }
    if (blockIdx.x == 0)  // the empty segments hold no point: workgroup 0 stores their (trivial) grids
        for (int s = (int)threadIdx.x; s < b; s += 256) {
            const int start = s == 0 ? 0 : offset[s - 1];
            if (offset[s] - start <= 0) seg[s] = seg_grid_of(s, offset, bbox_lo, bbox_hi, occupancy);
        }
    __syncthreads();
    int t = first + threadIdx.x;
    if (t >= n) return;
    int s = seg_of(t, offset, b);
    const SegGrid g = (s - s0 < COUNT_SEGS) ? s_grid[s - s0] : seg_grid_of(s, offset, bbox_lo, bbox_hi, occupancy);
    int cx = cell_coord(xyz[3 * t], g.minx, g.inv_h, g.gx);
    int cy = cell_coord(xyz[3 * t + 1], g.miny, g.inv_h, g.gy);
    int cz = cell_coord(xyz[3 * t + 2], g.minz, g.inv_h, g.gz);
    int cell = g.cell_base + (cz * g.gy + cy) * g.gx + cx;
    point_cell[t] = cell;
    point_rank[t] = atomicAdd(&cell_count[cell], 1);
}

// exclusive scan over ncell_pad ints.
// One pass: a tile sums itself, publishes the sum (bit 31 = "there"; the counts stay below 2^31), adds the sums of the tiles in
// front of it as they appear (tiles start in index order: the ones waited for are running or done) and scans itself.  The
// hand-off words are zeroed by knn_init_kernel.  (Two launches before -- a reduce and an apply that re-read the tile.)
__global__ __launch_bounds__(SCAN_THREADS) void knn_scan_kernel(const int *__restrict__ in, int *block_sums, int *out, int ntiles) {
    __shared__ int s_w[SCAN_THREADS / WAVE];
    __shared__ int s_base;
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    {
        const int4 *p = (const int4 *)(in + (size_t)blockIdx.x * SCAN_TILE) + threadIdx.x * 2;
        const int4 a = p[0], c = p[1];
        int v = a.x + a.y + a.z + a.w + c.x + c.y + c.z + c.w;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
        if (lane == 0) s_w[wid] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int i = 0; i < SCAN_THREADS / WAVE; ++i) t += s_w[i];
            __hip_atomic_store(block_sums + blockIdx.x, (int)(0x80000000u | (unsigned)t), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
    int part = 0;
    for (int i = threadIdx.x; i < (int)blockIdx.x; i += SCAN_THREADS) {
        int w;
        do {
            w = __hip_atomic_load(block_sums + i, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (w >= 0) __builtin_amdgcn_s_sleep(1);
        } while (w >= 0);
        part += w & 0x7fffffff;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, WAVE);
    if (lane == 0) s_w[wid] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < SCAN_THREADS / WAVE; ++i) t += s_w[i];
        s_base = t;
    }
    __syncthreads();
    int base = s_base;
    __syncthreads();
    const int4 *p = (const int4 *)(in + (size_t)blockIdx.x * SCAN_TILE) + threadIdx.x * 2;
    int4 a = p[0], c = p[1];
    int v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    int tot = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { int x = v[i]; v[i] = tot; tot += x; }
    int inc = tot;  // inclusive wave scan of per-thread totals
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        int y = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += y;
    }
    if (lane == 63) s_w[wid] = inc;
    __syncthreads();
    int wbase = 0;
    for (int i = 0; i < wid; ++i) wbase += s_w[i];
    int tbase = base + wbase + inc - tot;
    int4 *q = (int4 *)(out + (size_t)blockIdx.x * SCAN_TILE) + threadIdx.x * 2;
    q[0] = make_int4(tbase + v[0], tbase + v[1], tbase + v[2], tbase + v[3]);
    q[1] = make_int4(tbase + v[4], tbase + v[5], tbase + v[6], tbase + v[7]);
    if (blockIdx.x == ntiles - 1 && threadIdx.x == SCAN_THREADS - 1)
        out[(size_t)ntiles * SCAN_TILE] = tbase + tot;
}

__global__ __launch_bounds__(256) void knn_scatter_kernel(int n, const float *__restrict__ xyz,
                                                          const int *__restrict__ cell_start,
                                                          const int *__restrict__ point_cell,
                                                          const int *__restrict__ point_rank,
                                                          float4 *sorted) {
    int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int pos = cell_start[point_cell[t]] + point_rank[t];
    sorted[pos] = make_float4(xyz[3 * t], xyz[3 * t + 1], xyz[3 * t + 2], __int_as_float(t));
}

// ---------------------------------------------------------------- grid query --
template <int KC>
__device__ __forceinline__ void topk_insert(float (&bd)[KC], int (&bi)[KC], float d2, int id) {
    // sorted ascending; new element goes after all entries <= d2 (stable)
#pragma unroll
    for (int j = KC - 1; j > 0; --j) {
        bool shift = d2 < bd[j - 1];
        bool here = !shift && d2 < bd[j];
        float nd = shift ? bd[j - 1] : (here ? d2 : bd[j]);
        int ni = shift ? bi[j - 1] : (here ? id : bi[j]);
        bd[j] = nd;
        bi[j] = ni;
    }
    if (d2 < bd[0]) { bd[0] = d2; bi[0] = id; }
}

template <int KC>
__device__ __forceinline__ void scan_range(const float4 *__restrict__ sorted, int p0, int p1, float qx,
                                           float qy, float qz, float (&bd)[KC], int (&bi)[KC], unsigned &visited) {
    visited += (unsigned)(p1 - p0);  // (dead code unless the COUNT instantiation reads it)
    for (int p = p0; p < p1; ++p) {
        float4 c = sorted[p];
        float d2 = ref_d2(qx, qy, qz, c.x, c.y, c.z);
        if (d2 < bd[KC - 1]) topk_insert<KC>(bd, bi, d2, __float_as_int(c.w));
    }
}

// COUNT: the measurement twin (bench.py `ops`): also adds the number of candidate points this query evaluated a distance
// for to *pairs -- the pairs the grid method really computes, as opposed to the m * n_b pairs of
// the reference's brute-force scan.  The production instantiation (COUNT = false) carries no trace of it.
template <int KC, bool COUNT>
__global__ __launch_bounds__(256) void knn_grid_query_kernel(
    int m, int k, const float4 *__restrict__ sorted, const float *__restrict__ new_xyz,
    const int *__restrict__ offset, const int *__restrict__ new_offset, int b,
    const SegGrid *__restrict__ seg, const int *__restrict__ cell_start, int *__restrict__ idx,
    float *__restrict__ dist2, int pad_with_start, int self_mode, int *tie_count, int *tie_list,
    unsigned long long *pairs) {
    int t = blockIdx.x * 256 + threadIdx.x;
    unsigned visited = 0;
    if (t >= m) return;
    int qid, s;
    float qx, qy, qz;
    if (self_mode) {  // queries visited in cell order: neighbouring lanes share candidate cells
        float4 p = sorted[t];
        qx = p.x; qy = p.y; qz = p.z;
        qid = __float_as_int(p.w);
        s = seg_of(qid, offset, b);
    } else {
        qid = t;
        qx = new_xyz[3 * t]; qy = new_xyz[3 * t + 1]; qz = new_xyz[3 * t + 2];
        s = seg_of(t, new_offset, b);
    }
    const SegGrid g = seg[s];
    float bd[KC];
    int bi[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) { bd[j] = 1e10f; bi[j] = -1; }

    if (g.n_pts > 0) {
        const int cx = cell_coord(qx, g.minx, g.inv_h, g.gx);
        const int cy = cell_coord(qy, g.miny, g.inv_h, g.gy);
        const int cz = cell_coord(qz, g.minz, g.inv_h, g.gz);
        const int rmax = max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
        // Cell culling (round 3): a cell whose box is at least as far from the query as the current (k+1)-th best distance
        // cannot contribute (a candidate enters only with d2 < bd[KC-1]), so rows of cells are skipped and their x range
        // clipped before any point is read.  Distances in cell units from the query's UNclamped fractional cell position,
        // each gap shortened by the same 0.01 cell that covers the rounding of cell_coord() in the ring stop test below.
        // The list of the k+1 smallest distances -- and with it the tie test -- is unchanged; 135 -> ~80 candidate
        // distances per query on the 120 k-point scene (bench.py `ops`).
        const float fx = (qx - g.minx) * g.inv_h, fy = (qy - g.miny) * g.inv_h, fz = (qz - g.minz) * g.inv_h;
        const float h2 = g.h * g.h, inv_h2 = g.inv_h * g.inv_h;
        auto gap = [](float f, int c) { return fmaxf(fmaxf(fmaxf((float)c - f, f - (float)(c + 1)), 0.f) - 0.01f, 0.f); };
        for (int R = 1;; ++R) {
            const int z0 = max(cz - R, 0), z1 = min(cz + R, g.gz - 1);
            const int y0 = max(cy - R, 0), y1 = min(cy + R, g.gy - 1);
            const int xa = max(cx - R, 0), xb = min(cx + R, g.gx - 1);
            for (int z = z0; z <= z1; ++z) {
                const float dz = gap(fz, z);
                for (int y = y0; y <= y1; ++y) {
                    const float dy = gap(fy, y);
                    const float base2 = (dz * dz + dy * dy) * h2;  // lower bound of d2 for every point of this row of cells
                    if (base2 >= bd[KC - 1]) continue;
                    const int row = g.cell_base + (z * g.gy + y) * g.gx;
                    const bool full = (R == 1) || (z - cz == R) || (cz - z == R) || (y - cy == R) || (cy - y == R);
                    if (full) {
                        // cells x with gap(fx, x)^2 h^2 + base2 < bd[KC-1]: |x - fx| within r cells (r padded)
                        int xlo = xa, xhi = xb;
                        if (bd[KC - 1] < 1e10f) {  // (no clip while the list is not full: the sentinel is not a distance)
                            const float r = sqrtf((bd[KC - 1] - base2) * inv_h2) * 1.0001f + 0.03f;
                            xlo = max(xa, (int)floorf(fmaxf(fx - r, -1.f)));
                            xhi = min(xb, (int)floorf(fminf(fx + r, 1.0e6f)));
                        }
                        if (xlo <= xhi)
                            scan_range<KC>(sorted, cell_start[row + xlo], cell_start[row + xhi + 1], qx, qy, qz, bd, bi, visited);
                    } else {
                        if (cx - R >= 0) {
                            const float dx = gap(fx, cx - R);
                            if (dx * dx * h2 + base2 < bd[KC - 1])
                                scan_range<KC>(sorted, cell_start[row + cx - R], cell_start[row + cx - R + 1], qx, qy, qz, bd, bi, visited);
                        }
                        if (cx + R <= g.gx - 1) {
                            const float dx = gap(fx, cx + R);
                            if (dx * dx * h2 + base2 < bd[KC - 1])
                                scan_range<KC>(sorted, cell_start[row + cx + R], cell_start[row + cx + R + 1], qx, qy, qz, bd, bi, visited);
                        }
                    }
                }
            }
            if (R >= rmax) break;  // whole segment scanned
            // every unvisited point is farther than (R - eps) cells along some axis; eps covers the
            // fp32 rounding of cell_coord() (|error| << 0.01 cell for grids <= 1024 per axis)
            const float lim = ((float)R - 0.01f) * g.h;
            if (bd[KC - 1] < lim * lim) break;
        }
    }

    if (COUNT) atomicAdd(pairs, (unsigned long long)visited);  // one atomic per query: a measurement build, not the timed one
    bool tie = false;
#pragma unroll
    for (int j = 0; j + 1 < KC; ++j)
        if (j < k && bd[j] == bd[j + 1] && bd[j + 1] < 1e10f) tie = true;
    if (tie) tie_list[atomicAdd(tie_count, 1)] = qid;

    const int pad = pad_with_start ? g.start : -1;
    int *orow = idx + (size_t)qid * k;
    float *drow = dist2 + (size_t)qid * k;
    if (k == KC - 1 && (KC - 1) % 4 == 0) {
#pragma unroll
        for (int j = 0; j < KC - 1; j += 4) {
            int4 iv = make_int4(bd[j] < 1e10f ? bi[j] : pad, bd[j + 1] < 1e10f ? bi[j + 1] : pad,
                                bd[j + 2] < 1e10f ? bi[j + 2] : pad, bd[j + 3] < 1e10f ? bi[j + 3] : pad);
            *(int4 *)(orow + j) = iv;
            *(float4 *)(drow + j) = make_float4(bd[j], bd[j + 1], bd[j + 2], bd[j + 3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < KC - 1; ++j)
            if (j < k) {
                orow[j] = bd[j] < 1e10f ? bi[j] : pad;
                drow[j] = bd[j];
            }
    }
}

// ---------------------------------------------------------- grid query, 16 lanes per query --
// k <= 16 (every call of the PT-v2m2 path: k = 16 / 8 self queries, k = 3 interpolation, k = 1 label transfer).
// A "row" = 16 consecutive lanes serves one query, four queries per wavefront:
//   * the k best candidates live SORTED ACROSS the lanes of the row (lane j holds the j-th smallest distance and its point);
//   * candidates are read 16 at a time (one float4 per lane: a 256-byte contiguous piece of the cell-sorted copy), every lane
//     evaluates one distance, and a wave ballot against the row's current k-th best keeps the survivors;
//   * a survivor is broadcast to its row and inserted by ONE compare + shift across the lanes (DPP row_shr:1), i.e. a
//     constant handful of instructions for all four queries of the wave, instead of a k-long compare / select chain per
//     lane and candidate in the one-lane-per-query form above (which spent most of its time there, and whose 64 lanes
//     diverged over 64 different cell walks);
//   * `e` tracks the smallest distance that is NOT in the list (rejected candidates and evicted entries), i.e. the
//     (k+1)-th smallest: a tie between it and the k-th, or between neighbours of the list, sends the query to the exact
//     re-run exactly as before.  Cells are pruned only when their lower bound EXCEEDS the k-th best (strictly), so a
//     point at exactly that distance is always evaluated and the tie test sees it.
// The result (k smallest by squared distance, ascending; ties re-run) is identical to the one-lane kernel's.
__device__ __forceinline__ float row_shr1_f(float x, float fill) {  // lane j <- lane j-1 of its row; lane 0 <- fill
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x111, 0xf, 0xf, false));
}
__device__ __forceinline__ int row_shr1_i(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x111, 0xf, 0xf, false); }
__device__ __forceinline__ float row_shl1_f(float x, float fill) {  // lane j <- lane j+1 of its row; lane 15 <- fill
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x101, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_min16(float x) {  // minimum over the 16 lanes of the row, in every lane (row_ror 1, 2, 4, 8)
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x121, 0xf, 0xf, false)));
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x122, 0xf, 0xf, false)));
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xf, 0xf, false)));
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, false)));
    return x;
}

struct RowList {
    float v;    // entry of this lane: the 16 lanes of a row hold an ascending list; lanes < k are the k best so far
    int vi;
    float tau;  // row-uniform: v of lane k-1, the k-th best so far
    float e;    // PER LANE: smallest distance this lane saw leave or miss the 16-lane list (reduced over the row at the end)
};
// v of lane K - 1 in every lane of the row: DPP row_newbcast for the compile-time K of the hot call sites, ds_bpermute otherwise
template <int K>
__device__ __forceinline__ float row_kth(float v, int km1) {
    if constexpr (K > 0) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + (K - 1), 0xf, 0xf, false));
    else return __shfl(v, km1, 16);
}

// one compare-exchange stage of a bitonic network across the lanes of a row: partner = lane ^ STRIDE (ds_swizzle, no memory),
// `up` = this lane keeps the smaller of the pair.  Equal keys: both lanes keep their own.
template <int STRIDE>
__device__ __forceinline__ void row_cmpx(float &d, int &id, bool up) {
    const float od = __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(d), (STRIDE << 10) | 0x1f));
    const int oi = __builtin_amdgcn_ds_swizzle(id, (STRIDE << 10) | 0x1f);
    const bool take = up ? (od < d) : (od > d);
    d = take ? od : d;
    id = take ? oi : id;
}
// ascending sort of 16 (d, id) pairs across the lanes of a row
__device__ __forceinline__ void row_sort16(float &d, int &id, int r) {
    row_cmpx<1>(d, id, ((r & 1) == 0) == ((r & 2) == 0));
    row_cmpx<2>(d, id, ((r & 2) == 0) == ((r & 4) == 0));
    row_cmpx<1>(d, id, ((r & 1) == 0) == ((r & 4) == 0));
    row_cmpx<4>(d, id, ((r & 4) == 0) == ((r & 8) == 0));
    row_cmpx<2>(d, id, ((r & 2) == 0) == ((r & 8) == 0));
    row_cmpx<1>(d, id, ((r & 1) == 0) == ((r & 8) == 0));
    row_cmpx<8>(d, id, (r & 8) == 0);
    row_cmpx<4>(d, id, (r & 4) == 0);
    row_cmpx<2>(d, id, (r & 2) == 0);
    row_cmpx<1>(d, id, (r & 1) == 0);
}

// candidates [p0, p1) of the cell-sorted copy against the row's list
template <int K>
__device__ __forceinline__ void row_scan_range(const float4 *__restrict__ sorted, int p0, int p1, float qx, float qy, float qz,
                                               int km1, int r, int lane, RowList &L, unsigned &visited) {
    visited += (unsigned)(p1 - p0);
    for (int p = p0; p < p1; p += 16) {
        const bool have = p + r < p1;
        const float4 c = ptv2_ld_or_zero(sorted + p + r, have);
        float d2 = have ? ref_d2(qx, qy, qz, c.x, c.y, c.z) : 3.0e38f;
        int id = __float_as_int(c.w);
        const bool surv = d2 < L.tau;
        unsigned my = (unsigned)((__ballot(surv) >> (lane & 48)) & 0xffffull);  // this row's survivors
        if (__popc(my) >= 7) {
            // many newcomers (the list is still filling up): sort the batch, then one bitonic merge with the list --
            // min(list[j], batch[15 - j]) over the lanes is the 16 smallest of the 32, a bitonic sequence, four more stages
            // sort it; what the merge drops (the larger of each pair) has left the list
            row_sort16(d2, id, r);
            const float rd = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d2), 0x140, 0xf, 0xf, false));  // row_mirror
            const int ri = __builtin_amdgcn_update_dpp(0, id, 0x140, 0xf, 0xf, false);
            const bool keep = L.v <= rd;
            L.e = fminf(L.e, keep ? rd : L.v);
            L.v = keep ? L.v : rd;
            L.vi = keep ? L.vi : ri;
            row_cmpx<8>(L.v, L.vi, (r & 8) == 0);
            row_cmpx<4>(L.v, L.vi, (r & 4) == 0);
            row_cmpx<2>(L.v, L.vi, (r & 2) == 0);
            row_cmpx<1>(L.v, L.vi, (r & 1) == 0);
            L.tau = row_kth<K>(L.v, km1);
            continue;
        }
        // rejected candidates bound the (k+1)-th best from above
        L.e = fminf(L.e, surv ? 3.0e38f : d2);
        while (my) {
            const int src = __builtin_ctz(my);
            my &= my - 1;
            const float cd = __shfl(d2, src, 16);
            const int ci = __shfl(id, src, 16);
            if (cd < L.tau) {  // (the k-th best may have dropped since the ballot)
                const bool gt = L.v > cd;  // entries that move one lane up; equal ones stay in front of the newcomer
                const float vp = row_shr1_f(L.v, cd);
                const int ip = row_shr1_i(L.vi, ci);
                const int gtp = row_shr1_i(gt ? 1 : 0, 0);
                if (r == 15) L.e = fminf(L.e, L.v);  // what falls off the end of the 16-lane list
                L.v = gt ? (gtp ? vp : cd) : L.v;
                L.vi = gt ? (gtp ? ip : ci) : L.vi;
                L.tau = row_kth<K>(L.v, km1);
            } else {
                L.e = fminf(L.e, cd);
            }
        }
    }
}

// One slot of ring R around cell (cx, cy, cz) as a candidate range: slot u -> row of cells (z, y); rows on the shell of the
// ring take their whole x run [cx - R, cx + R] (clipped by the k-th best), inner rows only their two end cells.  Returns
// p0 >= p1 for an empty slot; lb2 = lower bound of the squared distance of every point of the range.
struct RowRange { int p0, p1; float lb2; };
__device__ __forceinline__ RowRange ring_slot(const SegGrid &g, const int *__restrict__ cell_start, int R, int u, int cx, int cy, int cz,
                                              float fx, float fy, float fz, float tau) {
    RowRange out{0, 0, 3.0e38f};
    const int w = 2 * R + 1;
    int t, side;
    if (R == 1) { t = u; side = 0; } else { t = u >> 1; side = u & 1; }
    if (t >= w * w) return out;
    // nearest rows first inside a ring is not attempted: t enumerates z-major
    const int dz = t / w - R, dy = t - (t / w) * w - R;
    const int z = cz + dz, y = cy + dy;
    if (z < 0 || z >= g.gz || y < 0 || y >= g.gy) return out;
    auto gap = [](float f, int c) { return fmaxf(fmaxf(fmaxf((float)c - f, f - (float)(c + 1)), 0.f) - 0.01f, 0.f); };
    const float h2 = g.h * g.h;
    const float gz_ = gap(fz, z), gy_ = gap(fy, y);
    const float base2 = (gz_ * gz_ + gy_ * gy_) * h2;
    if (base2 > tau) return out;
    const int row = g.cell_base + (z * g.gy + y) * g.gx;
    const bool shell = (R == 1) || (dz == R) || (dz == -R) || (dy == R) || (dy == -R);
    if (shell) {
        if (side) return out;
        int xlo = max(cx - R, 0), xhi = min(cx + R, g.gx - 1);
        if (tau < 1e10f) {  // cells x with gap(fx, x)^2 h^2 + base2 <= tau (no clip while the list is not full)
            const float rr = sqrtf((tau - base2) * g.inv_h * g.inv_h) * 1.0001f + 0.03f;
            xlo = max(xlo, (int)floorf(fmaxf(fx - rr, -1.f)));
            xhi = min(xhi, (int)floorf(fminf(fx + rr, 1.0e6f)));
        }
        if (xlo > xhi) return out;
        out.p0 = cell_start[row + xlo];
        out.p1 = cell_start[row + xhi + 1];
        out.lb2 = base2;
    } else {
        const int x = side ? cx + R : cx - R;
        if (x < 0 || x >= g.gx) return out;
        const float gx_ = gap(fx, x);
        const float lb = gx_ * gx_ * h2 + base2;
        if (lb > tau) return out;
        out.p0 = cell_start[row + x];
        out.p1 = cell_start[row + x + 1];
        out.lb2 = lb;
    }
    return out;
}

template <int K, bool COUNT>
__global__ __launch_bounds__(256) void knn_row_query_kernel(
    int m, int k, const float4 *__restrict__ sorted, const float *__restrict__ new_xyz,
    const int *__restrict__ offset, const int *__restrict__ new_offset, int b,
    const SegGrid *__restrict__ seg, const int *__restrict__ cell_start, int *__restrict__ idx,
    float *__restrict__ dist2, int pad_with_start, int self_mode, int *tie_count, int *tie_list,
    unsigned long long *pairs) {
    const int lane = threadIdx.x & 63, r = lane & 15;
    const int t = (int)(((long long)blockIdx.x * 256 + threadIdx.x) >> 4);  // query ordinal of this row
    unsigned visited = 0;
    if (t >= m) return;  // (whole rows leave together)
    int qid, s;
    float qx, qy, qz;
    if (self_mode) {  // queries visited in cell order: the four rows of a wave walk neighbouring cells
        const float4 p = sorted[t];
        qx = p.x; qy = p.y; qz = p.z;
        qid = __float_as_int(p.w);
        s = seg_of(qid, offset, b);
    } else {
        qid = t;
        qx = new_xyz[3 * (size_t)t]; qy = new_xyz[3 * (size_t)t + 1]; qz = new_xyz[3 * (size_t)t + 2];
        s = seg_of(t, new_offset, b);
    }
    const SegGrid g = seg[s];
    const int km1 = k - 1;
    RowList L;
    L.v = 1e10f; L.vi = -1; L.tau = 1e10f; L.e = 1e10f;

    if (g.n_pts > 0) {
        const int cx = cell_coord(qx, g.minx, g.inv_h, g.gx);
        const int cy = cell_coord(qy, g.miny, g.inv_h, g.gy);
        const int cz = cell_coord(qz, g.minz, g.inv_h, g.gz);
        const int rmax = max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
        // distances in cell units from the query's UNclamped fractional cell position, as in the one-lane kernel; culling against
        // the k-th best and STRICT (see above)
        const float fx = (qx - g.minx) * g.inv_h, fy = (qy - g.miny) * g.inv_h, fz = (qz - g.minz) * g.inv_h;
        for (int R = 1;; ++R) {
            const int w = 2 * R + 1;
            const int slots = R == 1 ? w * w : 2 * w * w;
            for (int u0 = 0; u0 < slots; u0 += 16) {
                // the 16 lanes of the row set up 16 slots at once (their cell_start loads are in flight together) ...
                const RowRange mine = ring_slot(g, cell_start, R, u0 + r, cx, cy, cz, fx, fy, fz, L.tau);
                unsigned todo = (unsigned)((__ballot(mine.p0 < mine.p1) >> (lane & 48)) & 0xffffull);
                // ... and walk the non-empty ones in turn
                while (todo) {
                    const int j = __builtin_ctz(todo);
                    todo &= todo - 1;
                    const float lb2 = __shfl(mine.lb2, j, 16);
                    if (lb2 > L.tau) continue;  // (the k-th best has dropped since the slot was set up)
                    const int p0 = __shfl(mine.p0, j, 16), p1 = __shfl(mine.p1, j, 16);
                    row_scan_range<K>(sorted, p0, p1, qx, qy, qz, km1, r, lane, L, visited);
                }
            }
            if (R >= rmax) break;  // whole segment scanned
            // every unvisited point is farther than (R - eps) cells along some axis (eps: rounding of cell_coord())
            const float lim = ((float)R - 0.01f) * g.h;
            if (L.tau < lim * lim) break;
        }
    }

    if (COUNT && r == 0) atomicAdd(pairs, (unsigned long long)visited);  // a measurement build, not the timed one
    // ties inside the k + 1 smallest distances: neighbours inside the list, or the k-th against the best outside it (lane k of
    // the list when k < 16, and whatever left or missed the 16 lanes)
    const float vn = row_shl1_f(L.v, 3.0e38f);
    const float e = row_min16(fminf(L.e, r >= k ? L.v : 3.0e38f));
    bool tie = (r + 1 < k && L.v == vn && vn < 1e10f) || (r == km1 && L.v == e && e < 1e10f);
    const unsigned any = (unsigned)((__ballot(tie) >> (lane & 48)) & 0xffffull);
    if (any && r == 0) tie_list[atomicAdd(tie_count, 1)] = qid;
    if (r < k) {
        const int pad = pad_with_start ? g.start : -1;
        idx[(size_t)qid * k + r] = L.v < 1e10f ? L.vi : pad;
        dist2[(size_t)qid * k + r] = L.v;
    }
}

// ------------------------------------------------- exact reference emulation --
// One wavefront per listed query.  The heap lives in LDS; every lane executes the same
// (wave-uniform) heap code, so LDS accesses are broadcasts and no lane diverges.
constexpr int EX_WAVES = 4;

__device__ __forceinline__ void ex_reheap(volatile float *hd, volatile int *hi, int k) {
    int root = 0, child = 1;
    while (child < k) {
        if (child + 1 < k && hd[child + 1] > hd[child]) child++;
        if (hd[root] > hd[child]) return;
        float td = hd[root]; hd[root] = hd[child]; hd[child] = td;
        int ti = hi[root]; hi[root] = hi[child]; hi[child] = ti;
        root = child;
        child = root * 2 + 1;
    }
}

__global__ __launch_bounds__(EX_WAVES *WAVE) void knn_exact_kernel(
    int m, int k, const float *__restrict__ xyz, const float *__restrict__ new_xyz,
    const int *__restrict__ offset, const int *__restrict__ new_offset, int b, int *__restrict__ idx,
    float *__restrict__ dist2, int pad_with_start, const int *__restrict__ tie_count,
    const int *__restrict__ tie_list, int all_queries) {
    __shared__ float s_d[EX_WAVES][128];
    __shared__ int s_i[EX_WAVES][128];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    volatile float *hd = s_d[wid];
    volatile int *hi = s_i[wid];
    const int total = all_queries ? m : *tie_count;
    const int nwaves = gridDim.x * EX_WAVES;
    for (int w = blockIdx.x * EX_WAVES + wid; w < total; w += nwaves) {
        const int q = all_queries ? w : tie_list[w];
        const int s = seg_of(q, new_offset, b);
        const int start = s == 0 ? 0 : offset[s - 1];
        const int end = offset[s];
        const float qx = new_xyz[3 * q], qy = new_xyz[3 * q + 1], qz = new_xyz[3 * q + 2];
        for (int j = lane; j < k; j += WAVE) {
            hd[j] = 1e10f;
            hi[j] = pad_with_start ? start : -1;
        }
        for (int base = start; base < end; base += WAVE) {
            const int i = base + lane;
            float d2 = 3.0e38f;
            if (i < end) d2 = ref_d2(qx, qy, qz, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
            unsigned long long mask = __ballot(d2 < hd[0]);  // root only ever decreases: safe prefilter
            while (mask) {
                const int l = __builtin_ctzll(mask);
                mask &= mask - 1;
                const float cd = __shfl(d2, l, WAVE);
                if (cd < hd[0]) {  // knn_query_cuda_kernel.cu:93-97
                    hd[0] = cd;
                    hi[0] = base + l;
                    ex_reheap(hd, hi, k);
                }
            }
        }
        for (int i = k - 1; i > 0; --i) {  // heap_sort (:33-42)
            float td = hd[0]; hd[0] = hd[i]; hd[i] = td;
            int ti = hi[0]; hi[0] = hi[i]; hi[i] = ti;
            ex_reheap(hd, hi, i);
        }
        for (int j = lane; j < k; j += WAVE) {
            idx[(size_t)q * k + j] = hi[j];
            dist2[(size_t)q * k + j] = hd[j];
        }
    }
}

// The same emulation for the LISTED queries (ties) with a whole workgroup per query: the heap's history is every
// candidate that beat the root at its turn, in ascending index order -- a few hundred of a 120 000-point segment -- and
// a single wavefront spends its 48 us streaming the other 119 800 past the root test (one dependent load round trip per
// 64 points).  Here 16 wavefronts test a chunk of 4 096 points each trip against the root value at the chunk's start
// (the root only decreases: a superset of what the sequential scan accepts), the survivors are compacted in index
// order through LDS, and wavefront 0 replays them through the heap exactly as above.
constexpr int EXW_WAVES = 16, EXW_PER_LANE = 4, EXW_CHUNK = EXW_WAVES * WAVE * EXW_PER_LANE, EXW_CAP = 1024;

// The heap of wavefront 0 lives ACROSS ITS LANES (node j in lane j of one register pair; k <= 32 here) and is walked with
// v_readlane / a one-lane select on wave-uniform node numbers: a handful of cycles per access, where the LDS heap of the
// one-wave kernel pays an LDS round trip for each (the replay of the ~150 accepted candidates was most of its 48 us).
__device__ __forceinline__ float lane_get_f(float v, int node) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), node)); }
__device__ __forceinline__ int lane_get_i(int v, int node) { return __builtin_amdgcn_readlane(v, node); }
__device__ __forceinline__ void lane_set_f(float &v, int node, float x) { v = ((int)(threadIdx.x & 63) == node) ? x : v; }
__device__ __forceinline__ void lane_set_i(int &v, int node, int x) { v = ((int)(threadIdx.x & 63) == node) ? x : v; }
// reheap (knn_query_cuda_kernel.cu:15-30) with the root's (new) value handed in and written where it settles
__device__ __forceinline__ void lanes_reheap(float &hd, int &hi, int k, float rd, int ri) {
    int root = 0, child = 1;
    while (child < k) {
        float cd = lane_get_f(hd, child);
        if (child + 1 < k) {
            const float c1 = lane_get_f(hd, child + 1);
            if (c1 > cd) { child++; cd = c1; }
        }
        if (rd > cd) break;
        lane_set_f(hd, root, cd);
        lane_set_i(hi, root, lane_get_i(hi, child));
        root = child;
        child = __builtin_amdgcn_readfirstlane(root * 2 + 1);
    }
    lane_set_f(hd, root, rd);
    lane_set_i(hi, root, ri);
}

__global__ __launch_bounds__(EXW_WAVES *WAVE) void knn_exact_wide_kernel(
    int k, const float *__restrict__ xyz, const float *__restrict__ new_xyz, const int *__restrict__ offset,
    const int *__restrict__ new_offset, int b, int *__restrict__ idx, float *__restrict__ dist2, int pad_with_start,
    const int *__restrict__ tie_count, const int *__restrict__ tie_list) {
    __shared__ float s_root;
    __shared__ float s_cd[EXW_CAP];
    __shared__ int s_ci[EXW_CAP];
    __shared__ int s_cnt[EXW_WAVES * EXW_PER_LANE + 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int total = *tie_count;
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int q = tie_list[w];
        const int s = seg_of(q, new_offset, b);
        const int start = s == 0 ? 0 : offset[s - 1];
        const int end = offset[s];
        const float qx = new_xyz[3 * q], qy = new_xyz[3 * q + 1], qz = new_xyz[3 * q + 2];
        float hd = 1e10f;                        // (wavefront 0) heap node `lane`
        int hi = pad_with_start ? start : -1;
        __syncthreads();  // (the previous query is done with s_root and the candidate buffers)
        if (threadIdx.x == 0) s_root = 1e10f;
        __syncthreads();
        // the distances of a chunk are formed one trip ahead: their loads are in flight while the previous chunk's survivors
        // go through the barriers and the heap
        float dn[EXW_PER_LANE];
        auto fetch = [&](int cb) {
#pragma unroll
            for (int u = 0; u < EXW_PER_LANE; ++u) {
                const int i = cb + (wid * EXW_PER_LANE + u) * WAVE + lane;
                const bool ok = i < end;
                const size_t ii = ok ? (size_t)i : (size_t)start;
                const float d = ref_d2(qx, qy, qz, xyz[3 * ii], xyz[3 * ii + 1], xyz[3 * ii + 2]);
                dn[u] = ok ? d : 3.0e38f;
            }
        };
        fetch(start);
        for (int cbase = start; cbase < end; cbase += EXW_CHUNK) {
            const float root = s_root;
            // sub-batch u of wave wid covers points cbase + (wid * PER_LANE + u) * 64 + lane: ascending in (wid, u, lane)
            float d2[EXW_PER_LANE];
            unsigned long long mk[EXW_PER_LANE];
#pragma unroll
            for (int u = 0; u < EXW_PER_LANE; ++u) d2[u] = dn[u];
            if (cbase + EXW_CHUNK < end) fetch(cbase + EXW_CHUNK);
#pragma unroll
            for (int u = 0; u < EXW_PER_LANE; ++u) {
                mk[u] = __ballot(d2[u] < root);
                if (lane == 0) s_cnt[wid * EXW_PER_LANE + u] = __popcll(mk[u]);
            }
            __syncthreads();
            if (wid == 0) {  // exclusive scan of the 64 sub-batch counts: one per lane of wavefront 0
                static_assert(EXW_WAVES * EXW_PER_LANE == WAVE, "one count per lane");
                const int c = s_cnt[lane];
                int inc = c;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const int y = __shfl_up(inc, o, WAVE);
                    if (lane >= o) inc += y;
                }
                s_cnt[lane] = inc - c;
                if (lane == WAVE - 1) s_cnt[WAVE] = inc;
            }
            __syncthreads();
            const int nsurv = s_cnt[EXW_WAVES * EXW_PER_LANE];
            if (nsurv <= EXW_CAP) {
#pragma unroll
                for (int u = 0; u < EXW_PER_LANE; ++u)
                    if ((mk[u] >> lane) & 1ull) {
                        const int pos = s_cnt[wid * EXW_PER_LANE + u] + __popcll(mk[u] & ((1ull << lane) - 1ull));
                        s_cd[pos] = d2[u];
                        s_ci[pos] = cbase + (wid * EXW_PER_LANE + u) * WAVE + lane;
                    }
            }
            __syncthreads();
            if (wid == 0) {
                float rootv = lane_get_f(hd, 0);
                if (nsurv <= EXW_CAP) {
                    for (int j0 = 0; j0 < nsurv; j0 += WAVE) {  // ascending index order, 64 survivors per read
                        const float cdv = j0 + lane < nsurv ? s_cd[j0 + lane] : 3.0e38f;
                        const int civ = j0 + lane < nsurv ? s_ci[j0 + lane] : 0;
                        const int cnt = min(WAVE, nsurv - j0);
                        for (int j = 0; j < cnt; ++j) {
                            const float cd = lane_get_f(cdv, j);
                            if (cd < rootv) {  // knn_query_cuda_kernel.cu:93-97
                                lanes_reheap(hd, hi, k, cd, lane_get_i(civ, j));
                                rootv = lane_get_f(hd, 0);
                            }
                        }
                    }
                } else {  // (only the first chunks of a scan, while the heap still holds its 1e10 fillers: the one-wave walk)
                    const int cend = min(cbase + EXW_CHUNK, end);
                    for (int base = cbase; base < cend; base += WAVE) {
                        const int i = base + lane;
                        float d = 3.0e38f;
                        if (i < cend) d = ref_d2(qx, qy, qz, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
                        unsigned long long mask = __ballot(d < rootv);
                        while (mask) {
                            const int l = __builtin_ctzll(mask);
                            mask &= mask - 1;
                            const float cd = lane_get_f(d, l);
                            if (cd < rootv) {
                                lanes_reheap(hd, hi, k, cd, base + l);
                                rootv = lane_get_f(hd, 0);
                            }
                        }
                    }
                }
                if (lane == 0) s_root = rootv;
            }
            __syncthreads();
        }
        if (wid == 0) {
            for (int i = k - 1; i > 0; --i) {  // heap_sort (:33-42): swap root and node i, reheap the first i nodes
                const float ld = lane_get_f(hd, i), rd = lane_get_f(hd, 0);
                const int li = lane_get_i(hi, i), ri = lane_get_i(hi, 0);
                lane_set_f(hd, i, rd);
                lane_set_i(hi, i, ri);
                lanes_reheap(hd, hi, i, ld, li);
            }
            if (lane < k) {
                idx[(size_t)q * k + lane] = hi;
                dist2[(size_t)q * k + lane] = hd;
            }
        }
    }
}

thread_local unsigned long long *g_pair_counter = nullptr;

template <int KC>
void launch_query(hipStream_t st, int m, int k, const Workspace &w, const float *new_xyz,
                  const int *offset, const int *new_offset, int b, int *idx, float *dist2,
                  int pad_with_start, int self_mode) {
    if (g_pair_counter)
        hipLaunchKernelGGL((knn_grid_query_kernel<KC, true>), dim3(divup(m, 256)), dim3(256), 0, st, m, k, w.sorted,
                           new_xyz, offset, new_offset, b, w.seg, w.cell_start, idx, dist2, pad_with_start,
                           self_mode, w.tie_count, w.tie_list, g_pair_counter);
    else
        hipLaunchKernelGGL((knn_grid_query_kernel<KC, false>), dim3(divup(m, 256)), dim3(256), 0, st, m, k, w.sorted,
                           new_xyz, offset, new_offset, b, w.seg, w.cell_start, idx, dist2, pad_with_start,
                           self_mode, w.tie_count, w.tie_list, (unsigned long long *)nullptr);
}

}  // namespace

// measurement hook (bench.py `ops`): while `device_counter` != NULL the calling thread's grid queries run the counting twin
// of the query kernel, which adds the candidate distances it evaluates to *device_counter (zeroed by the caller)
extern "C" int knn_query_count_pairs(unsigned long long *device_counter) {
    g_pair_counter = device_counter;
    return PTV2_OK;
}

extern "C" size_t knn_query_hip_workspace_bytes(int m, int n, int b) {
    if (m < 0 || n < 0 || b < 1) return 0;
    return carve(nullptr, m, n, b).bytes;
}

// grid_mode 0: build the cell grid of (xyz, offset) in `workspace`, then query.  grid_mode 1: `workspace` still holds the grid
// an earlier call (on the same stream, same xyz / offset / n / b) built there -- query only; `slot` (1 .. 3) numbers the queries
// that share a grid (each has its own re-run counter).  A scene asks for up to three tables over the points of one level
// (the interpolation table from the finer level and one or two self tables): one grid instead of three.
extern "C" int knn_query_grid_hip_launcher(int m, int nsample, const float *xyz, const float *new_xyz,
                                           const int *offset, const int *new_offset, int *idx, float *dist2,
                                           int n, int b, int pad_with_start, int grid_mode, int slot, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    if (nsample < 1 || nsample > 128 || m < 0 || n < 0 || b < 1) return PTV2_ERR_ARG;
    if (grid_mode < 0 || grid_mode > 1 || slot < 0 || slot > 3 || (grid_mode == 0 && slot != 0)) return PTV2_ERR_ARG;
    if (m == 0) return PTV2_OK;
    if (!xyz || !new_xyz || !offset || !new_offset || !idx || !dist2) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int k = nsample;
    if (k > 32 || n == 0) {  // large k: exact emulation for every query (heap does not fit registers)
        hipLaunchKernelGGL(knn_exact_kernel, dim3(min(divup(m, EX_WAVES), 4096)), dim3(EX_WAVES * WAVE), 0, st, m,
                           k, xyz, new_xyz, offset, new_offset, b, idx, dist2, pad_with_start, (const int *)nullptr,
                           (const int *)nullptr, 1);
        PTV2_CHECK_LAUNCH();
        return PTV2_OK;
    }
    Workspace w = carve(workspace, m, n, b);
    if (!workspace || workspace_bytes < w.bytes) return PTV2_ERR_WORKSPACE;
    const long long ncell_ll = (long long)CELLS_PER_POINT * n + b + 1;
    if (ncell_ll + SCAN_TILE > 0x7fffffffLL) return PTV2_ERR_ARG;
    const int ncell = (int)ncell_ll;
    const int ntiles = divup(ncell + 1, SCAN_TILE);
    const int ncell_pad = ntiles * SCAN_TILE;
    const int self_mode = (new_xyz == xyz && new_offset == offset && m == n) ? 1 : 0;

    w.tie_count += slot;
    if (grid_mode == 0) {
    hipLaunchKernelGGL(knn_init_kernel, dim3(min(divup(ncell_pad, 256), 1024)), dim3(256), 0, st, w.tie_count,
                       w.bbox_lo, w.bbox_hi, b, w.cell_count, ncell_pad, w.block_sums, ntiles);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(divup(n, 256)), dim3(256), 0, st, n, xyz, offset, b, w.bbox_lo,
                       w.bbox_hi);
    // target points per cell of the bounding volume (surface clouds fill a fraction of their cells: several times as many per
    // occupied one).  Swept at 120 k points with the 16-lane query: 2.0 -> 86 us, 1.0 -> 73, 0.5 -> 73, 0.25 -> 78 (k = 16)
    static const float occupancy = [] { const char *e = getenv("AO_AMD_KNN_OCC"); const float v = e ? (float)atof(e) : 0.f; return v > 0.f ? v : 0.7f; }();
    hipLaunchKernelGGL(knn_cell_count_kernel, dim3(divup(n, 256)), dim3(256), 0, st, n, xyz, offset, b, (const int *)w.bbox_lo,
                       (const int *)w.bbox_hi, occupancy, w.seg, w.cell_count, w.point_cell, w.point_rank);
    hipLaunchKernelGGL(knn_scan_kernel, dim3(ntiles), dim3(SCAN_THREADS), 0, st, (const int *)w.cell_count, w.block_sums,
                       w.cell_start, ntiles);
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(divup(n, 256)), dim3(256), 0, st, n, xyz, w.cell_start, w.point_cell,
                       w.point_rank, w.sorted);
    }
    {
    PtvScopedTimer qt(KID_KNN_QUERY, st, 12.0 * n + 12.0 * m + 8.0 * (double)m * k);
    if (k <= 16) {
        const dim3 grid(divup((long long)m * 16, 256)), blk(256);
#define ROWQ(KK)                                                                                                                   \
        do {                                                                                                                       \
            if (g_pair_counter)                                                                                                    \
                hipLaunchKernelGGL((knn_row_query_kernel<KK, true>), grid, blk, 0, st, m, k, w.sorted, new_xyz, offset, new_offset, b, \
                                   w.seg, w.cell_start, idx, dist2, pad_with_start, self_mode, w.tie_count, w.tie_list,            \
                                   g_pair_counter);                                                                                \
            else                                                                                                                   \
                hipLaunchKernelGGL((knn_row_query_kernel<KK, false>), grid, blk, 0, st, m, k, w.sorted, new_xyz, offset, new_offset, b, \
                                   w.seg, w.cell_start, idx, dist2, pad_with_start, self_mode, w.tie_count, w.tie_list,            \
                                   (unsigned long long *)nullptr);                                                                 \
        } while (0)
        if (k == 16) ROWQ(16);
        else if (k == 8) ROWQ(8);
        else if (k == 3) ROWQ(3);
        else if (k == 1) ROWQ(1);
        else ROWQ(0);
#undef ROWQ
    }
    else launch_query<33>(st, m, k, w, new_xyz, offset, new_offset, b, idx, dist2, pad_with_start, self_mode);
    }
    hipLaunchKernelGGL(knn_exact_wide_kernel, dim3(128), dim3(EXW_WAVES * WAVE), 0, st, k, xyz, new_xyz, offset, new_offset, b, idx,
                       dist2, pad_with_start, (const int *)w.tie_count, (const int *)w.tie_list);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int knn_query_hip_launcher(int m, int nsample, const float *xyz, const float *new_xyz,
                                      const int *offset, const int *new_offset, int *idx, float *dist2,
                                      int n, int b, int pad_with_start, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    return knn_query_grid_hip_launcher(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2, n, b, pad_with_start, 0, 0,
                                       workspace, workspace_bytes, stream);
}
