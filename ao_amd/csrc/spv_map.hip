// ao_amd/csrc/spv_map.hip -- the point-voxel map of SPVCNN (include/ptv2_spv_hip.h).  gfx950 only.
//
// Level l of the map is one stable sort of the points by key_l = cloud << 54 | (x >> l) << 36 | (y >> l) << 18 | (z >> l), the
// key of spconv_tables.hip: the distinct keys in ascending order are that unit's rows of level l >= 1, and the map hands level
// 0 over in the same order, so a run's rank IS the voxel's row at every level and nothing waits for the tables.  Per level:
//   sort    hipCUB radix sort of (key_l, i), stable: within a voxel the points stay in ascending index  -> order[l]
//   heads   key != the one before -> inclusive scan -> rank
//   runs    row[l][order[p]] = rank[p] - 1;  a head writes start[l][rank - 1] = p;  the last position closes the CSR
// Every element is written by exactly one thread: no atomics, two runs give identical maps.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "common.h"
#include "../../include/ptv2_spv_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int CB = SPV_COORD_BITS;
constexpr int CMAX = (1 << CB) - 1;
typedef unsigned long long u64;

__global__ __launch_bounds__(TPB) void spv_keys_kernel(int n, int b, int level, const int *__restrict__ coord,
                                                       const int *__restrict__ offset, u64 *__restrict__ keys, int *__restrict__ vals,
                                                       int *__restrict__ status) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    int c[3], bad = 0;
    for (int a = 0; a < 3; ++a) {
        int v = coord[3 * (size_t)i + a];
        if (v < 0) { bad |= SPV_BAD_NEGATIVE; v = 0; }
        if (v > CMAX) { bad |= SPV_BAD_LARGE; v = CMAX; }
        c[a] = v >> level;
    }
    if (level == 0) {  // (plain stores of one value: a benign race, no atomic)
        if (bad & SPV_BAD_NEGATIVE) status[0] = 1;
        if (bad & SPV_BAD_LARGE) status[1] = 1;
    }
    keys[i] = ((u64)seg_of(i, offset, b) << (3 * CB)) | ((u64)c[0] << (2 * CB)) | ((u64)c[1] << CB) | (u64)c[2];
    vals[i] = i;
}

__global__ __launch_bounds__(TPB) void spv_heads_kernel(int n, const u64 *__restrict__ keys, int *__restrict__ flags) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// one thread per sorted position p; at level 0 also one per cloud: the number of voxels of clouds 0 .. p
__global__ __launch_bounds__(TPB) void spv_runs_kernel(int n, int b, int level, const u64 *__restrict__ keys,
                                                       const int *__restrict__ flags, const int *__restrict__ rank,
                                                       const int *__restrict__ order, int *__restrict__ row, int *__restrict__ start,
                                                       int *__restrict__ vcoord, int *__restrict__ voffset, int *__restrict__ counts) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p < n) {
        const int r = min(max(rank[p] - 1, 0), n - 1), i = order[p];
        if ((unsigned)i < (unsigned)n) row[i] = r;
        if (flags[p]) {
            start[r] = p;
            if (level == 0) {
                const u64 key = keys[p];
                vcoord[3 * (size_t)r] = (int)((key >> (2 * CB)) & CMAX);
                vcoord[3 * (size_t)r + 1] = (int)((key >> CB) & CMAX);
                vcoord[3 * (size_t)r + 2] = (int)(key & CMAX);
            }
        }
        if (p == n - 1) { start[r + 1] = n; counts[level] = r + 1; }
    }
    if (level == 0 && p < b) {
        const u64 bound = (u64)(p + 1) << (3 * CB);
        int lo = 0, hi = n;
        while (lo < hi) {   // the first sorted position of a later cloud
            const int mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < bound) lo = mid + 1; else hi = mid;
        }
        voffset[p] = lo == 0 ? 0 : rank[lo - 1];
    }
}

struct Ws {
    u64 *keys_in, *keys_out;
    int *vals_in, *flags, *rank;
    void *cub;
    size_t cub_bytes, bytes;
};

Ws carve(void *base, int n) {
    Ws w;
    PtvCarver cv{(char *)base, 0};
    w.keys_in = cv.take_n<u64>(n); w.keys_out = cv.take_n<u64>(n);
    w.vals_in = cv.take_n<int>(n); w.flags = cv.take_n<int>(n); w.rank = cv.take_n<int>(n);
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, s1, (const u64 *)nullptr, (u64 *)nullptr, (const int *)nullptr,
                                             (int *)nullptr, n, 0, 64, (hipStream_t)0);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, s2, (const int *)nullptr, (int *)nullptr, n, (hipStream_t)0);
    w.cub_bytes = std::max(s1, s2) + 256;
    w.cub = cv.take(w.cub_bytes);
    w.bytes = cv.off;
    return w;
}

bool shape_ok(long long n, int b) { return n >= 1 && n < (1 << 30) && b >= 1 && b <= SPV_MAX_CLOUDS; }

}  // namespace

extern "C" int ptv2_spv_abi_version(void) { return 1; }
extern "C" int ptv2_spv_struct_bytes(int which) { return which == 0 ? (int)sizeof(spv_map) : -1; }

extern "C" long long ptv2_spv_map_workspace_bytes(long long n, int b) {
    if (!shape_ok(n, b)) return -1;
    return (long long)carve(nullptr, (int)n).bytes + 1024;
}

extern "C" int spv_build_map_hip_launcher(int n, int b, const int *coord, const int *offset, const spv_map *M, void *workspace,
                                          long long workspace_bytes, void *stream) {
    if (!shape_ok(n, b) || !coord || !offset || !M || !M->vcoord || !M->voffset || !M->counts || !M->status) return PTV2_ERR_ARG;
    for (int l = 0; l < SPV_LEVELS; ++l)
        if (!M->row[l] || !M->start[l] || !M->order[l]) return PTV2_ERR_ARG;
    Ws w = carve(workspace, n);
    if (!workspace || workspace_bytes < (long long)w.bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = divup(n, TPB);
    for (int l = 0; l < SPV_LEVELS; ++l) {
        hipLaunchKernelGGL(spv_keys_kernel, dim3(nb), dim3(TPB), 0, st, n, b, l, coord, offset, w.keys_in, w.vals_in, M->status);
        size_t cb = w.cub_bytes;
        if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, (const u64 *)w.keys_in, w.keys_out, (const int *)w.vals_in, M->order[l], n,
                                               0, 64, st) != hipSuccess)
            return PTV2_ERR_LAUNCH;
        hipLaunchKernelGGL(spv_heads_kernel, dim3(nb), dim3(TPB), 0, st, n, (const u64 *)w.keys_out, w.flags);
        cb = w.cub_bytes;
        if (hipcub::DeviceScan::InclusiveSum(w.cub, cb, (const int *)w.flags, w.rank, n, st) != hipSuccess) return PTV2_ERR_LAUNCH;
        hipLaunchKernelGGL(spv_runs_kernel, dim3(divup(std::max(n, b), TPB)), dim3(TPB), 0, st, n, b, l, (const u64 *)w.keys_out,
                           (const int *)w.flags, (const int *)w.rank, (const int *)M->order[l], M->row[l], M->start[l], M->vcoord,
                           M->voffset, M->counts);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
