// ao_amd/csrc/spconv_tables.hip -- the neighbour tables of SpUNet-v1m1's sparse convolutions (include/ptv2_spconv_hip.h).
//
// Every level's voxel set comes straight from the level-0 coordinates: level l holds the distinct values of
// (cloud, x >> l, y >> l, z >> l).  So no level waits for the count of the one before it, and the host reads nothing back:
//   key_l[i]  = cloud << 54 | (x >> l) << 36 | (y >> l) << 18 | (z >> l)                 one 64-bit key per level-0 row
//   sort      hipCUB radix sort of (key_l, i) over the key's 64 bits (a library sort, as gridpool.hip's)
//   heads     key != the one before -> inclusive scan -> the distinct keys U_l in ascending order; n_l = their count
// Level 0 keeps the caller's row order (U_0 is the sorted keys, `row0` the row of each); a level above numbers its rows by
// rank in U_l.  Every table entry is then one bisection of a sorted key array:
//   nbr[r][kappa]   the row of key(coord_r + kappa - k / 2), or -1
//   child[o][kappa] the row of level l with key(2 coord_o + kappa), or -1;  parent / slot the same the other way
// No atomics: every table element is written by exactly one thread, so two runs give identical tables.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "common.h"
#include "../../include/ptv2_spconv_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int CB = SPCONV_COORD_BITS;
constexpr int CMAX = (1 << CB) - 1;
typedef unsigned long long u64;

__device__ __forceinline__ u64 make_key(int s, int x, int y, int z) {
    return ((u64)s << (3 * CB)) | ((u64)x << (2 * CB)) | ((u64)y << CB) | (u64)z;
}
__device__ __forceinline__ void split_key(u64 key, int &s, int &x, int &y, int &z) {
    z = (int)(key & CMAX); y = (int)((key >> CB) & CMAX); x = (int)((key >> (2 * CB)) & CMAX); s = (int)(key >> (3 * CB));
}
// position of `key` in the ascending keys[0 .. m), or -1
__device__ __forceinline__ int find_key(const u64 *__restrict__ keys, int m, u64 key) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < m && keys[lo] == key) ? lo : -1;
}

__global__ __launch_bounds__(TPB) void keys_kernel(int n, int b, int level, const int *__restrict__ coord,
                                                   const int *__restrict__ offset, u64 *__restrict__ keys,
                                                   int *__restrict__ vals, int *__restrict__ status) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    int c[3], bad = 0;
    for (int a = 0; a < 3; ++a) {
        int v = coord[3 * (size_t)i + a];
        if (v < 0) { bad |= SPCONV_BAD_NEGATIVE; v = 0; }
        if (v > CMAX) { bad |= SPCONV_BAD_LARGE; v = CMAX; }
        c[a] = v >> level;
    }
    if (level == 0) {  // (plain stores of one value: a benign race, no atomic)
        if (bad & SPCONV_BAD_NEGATIVE) status[0] = 1;
        if (bad & SPCONV_BAD_LARGE) status[1] = 1;
    }
    keys[i] = make_key(seg_of(i, offset, b), c[0], c[1], c[2]);
    vals[i] = i;
}

__global__ __launch_bounds__(TPB) void heads_kernel(int n, const u64 *__restrict__ keys, int *__restrict__ flags) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// ukeys[rank - 1] = the distinct keys in order; counts[level] = their number
__global__ __launch_bounds__(TPB) void unique_kernel(int n, int level, const u64 *__restrict__ keys, const int *__restrict__ flags,
                                                     const int *__restrict__ rank, u64 *__restrict__ ukeys,
                                                     int *__restrict__ counts, int *__restrict__ status) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    if (level == 0) {
        ukeys[i] = keys[i];  // level 0: one row per input row, duplicates are an error
        if (!flags[i]) status[2] = 1;
        if (i == n - 1) counts[0] = n;
        return;
    }
    if (flags[i]) ukeys[rank[i] - 1] = keys[i];
    if (i == n - 1) counts[level] = rank[i];
}

// one thread per (sorted position p, kappa): row = rows ? rows[p] : p
template <int KS>
__global__ __launch_bounds__(TPB) void nbr_kernel(int cap, const int *__restrict__ count, const u64 *__restrict__ ukeys,
                                                  const int *__restrict__ rows, int *__restrict__ nbr) {
    constexpr int K = KS * KS * KS;
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    const int m = min(*count, cap);
    const long long p = t / K;
    if (p >= m) return;
    const int kappa = (int)(t - p * K);
    int s, x, y, z;
    split_key(ukeys[p], s, x, y, z);
    const int nx = x + kappa / (KS * KS) - KS / 2, ny = y + (kappa / KS) % KS - KS / 2, nz = z + kappa % KS - KS / 2;
    int j = -1;
    if (nx >= 0 && ny >= 0 && nz >= 0 && nx <= CMAX && ny <= CMAX && nz <= CMAX) {
        const int q = find_key(ukeys, m, make_key(s, nx, ny, nz));
        if (q >= 0) j = rows ? rows[q] : q;
    }
    const int row = rows ? rows[p] : (int)p;
    if (row >= 0 && row < cap) nbr[(size_t)row * K + kappa] = j;
}

// one thread per (coarse row o, kappa)
__global__ __launch_bounds__(TPB) void child_kernel(int cap, const int *__restrict__ count_fine, const int *__restrict__ count_coarse,
                                                    const u64 *__restrict__ fine, const int *__restrict__ fine_rows,
                                                    const u64 *__restrict__ coarse, int *__restrict__ child) {
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    const int mc = min(*count_coarse, cap), mf = min(*count_fine, cap);
    const long long o = t >> 3;
    if (o >= mc) return;
    const int kappa = (int)(t & 7);
    int s, x, y, z;
    split_key(coarse[o], s, x, y, z);
    const int fx = 2 * x + (kappa >> 2), fy = 2 * y + ((kappa >> 1) & 1), fz = 2 * z + (kappa & 1);
    int j = -1;
    if (fx <= CMAX && fy <= CMAX && fz <= CMAX) {
        const int q = find_key(fine, mf, make_key(s, fx, fy, fz));
        if (q >= 0) j = fine_rows ? fine_rows[q] : q;
    }
    child[(size_t)o * 8 + kappa] = j;
}

// one thread per sorted position of the fine level: parent, slot; per coarse row: its coordinate; per cloud: its end
__global__ __launch_bounds__(TPB) void parent_kernel(int cap, int b, const int *__restrict__ count_fine,
                                                     const int *__restrict__ count_coarse, const u64 *__restrict__ fine,
                                                     const int *__restrict__ fine_rows, const u64 *__restrict__ coarse,
                                                     int *__restrict__ parent, int *__restrict__ slot, int *__restrict__ coord,
                                                     int *__restrict__ offset) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    const int mc = min(*count_coarse, cap), mf = min(*count_fine, cap);
    if (p < mf) {
        int s, x, y, z;
        split_key(fine[p], s, x, y, z);
        const int q = find_key(coarse, mc, make_key(s, x >> 1, y >> 1, z >> 1));  // (always found: the coarse keys are these)
        const int row = fine_rows ? fine_rows[p] : p;
        if (row >= 0 && row < cap) {
            parent[row] = q < 0 ? 0 : q;
            slot[row] = ((x & 1) << 2) | ((y & 1) << 1) | (z & 1);
        }
    }
    if (p < mc) {
        int s, x, y, z;
        split_key(coarse[p], s, x, y, z);
        coord[3 * (size_t)p] = x; coord[3 * (size_t)p + 1] = y; coord[3 * (size_t)p + 2] = z;
    }
    if (p < b) {  // the number of coarse keys of clouds 0 .. p
        const u64 bound = (u64)(p + 1) << (3 * CB);
        int lo = 0, hi = mc;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (coarse[mid] < bound) lo = mid + 1; else hi = mid;
        }
        offset[p] = lo;
    }
}

struct Ws {
    u64 *keys_in, *keys_out, *ukeys[SPCONV_LEVELS];
    int *vals_in, *order, *flags, *rank, *rows0;
    void *cub;
    size_t cub_bytes, bytes;
};

Ws carve(void *base, int n) {
    Ws w;
    PtvCarver cv{(char *)base, 0};
    w.keys_in = cv.take_n<u64>(n); w.keys_out = cv.take_n<u64>(n);
    for (int l = 0; l < SPCONV_LEVELS; ++l) w.ukeys[l] = cv.take_n<u64>(n);
    w.vals_in = cv.take_n<int>(n); w.order = cv.take_n<int>(n); w.flags = cv.take_n<int>(n); w.rank = cv.take_n<int>(n);
    w.rows0 = cv.take_n<int>(n);
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, s1, (const u64 *)nullptr, (u64 *)nullptr, (const int *)nullptr,
                                             (int *)nullptr, n, 0, 64, (hipStream_t)0);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, s2, (const int *)nullptr, (int *)nullptr, n, (hipStream_t)0);
    w.cub_bytes = std::max(s1, s2) + 256;
    w.cub = cv.take(w.cub_bytes);
    w.bytes = cv.off;
    return w;
}

}  // namespace

extern "C" int ptv2_spconv_abi_version(void) { return 1; }
extern "C" int ptv2_spconv_struct_bytes(int which) { return which == 0 ? (int)sizeof(spconv_tables) : -1; }

extern "C" long long ptv2_spconv_tables_workspace_bytes(long long n, int b) {
    if (n < 1 || n > 0x3fffffff / SPCONV_MAX_K || b < 1 || b > SPCONV_MAX_CLOUDS) return -1;
    return (long long)carve(nullptr, (int)n).bytes + 1024;
}

extern "C" int spconv_build_tables_hip_launcher(int n, int b, const int *coord, const int *offset, const spconv_tables *T,
                                                void *workspace, long long workspace_bytes, void *stream) {
    if (n < 1 || n > 0x3fffffff / SPCONV_MAX_K || b < 1 || b > SPCONV_MAX_CLOUDS || !coord || !offset || !T || !T->nbr5 ||
        !T->counts || !T->status)
        return PTV2_ERR_ARG;
    for (int l = 0; l < SPCONV_LEVELS; ++l)
        if (!T->nbr3[l]) return PTV2_ERR_ARG;
    for (int l = 0; l + 1 < SPCONV_LEVELS; ++l)
        if (!T->child[l] || !T->parent[l] || !T->slot[l] || !T->coord[l] || !T->offset[l]) return PTV2_ERR_ARG;
    Ws w = carve(workspace, n);
    if (!workspace || workspace_bytes < (long long)w.bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int nb = divup(n, TPB);
    for (int l = 0; l < SPCONV_LEVELS; ++l) {
        hipLaunchKernelGGL(keys_kernel, dim3(nb), dim3(TPB), 0, st, n, b, l, coord, offset, w.keys_in, w.vals_in, T->status);
        size_t cb = w.cub_bytes;
        if (hipcub::DeviceRadixSort::SortPairs(w.cub, cb, (const u64 *)w.keys_in, w.keys_out, (const int *)w.vals_in, w.order, n, 0,
                                               64, st) != hipSuccess)
            return PTV2_ERR_LAUNCH;
        hipLaunchKernelGGL(heads_kernel, dim3(nb), dim3(TPB), 0, st, n, (const u64 *)w.keys_out, w.flags);
        cb = w.cub_bytes;
        if (hipcub::DeviceScan::InclusiveSum(w.cub, cb, (const int *)w.flags, w.rank, n, st) != hipSuccess) return PTV2_ERR_LAUNCH;
        hipLaunchKernelGGL(unique_kernel, dim3(nb), dim3(TPB), 0, st, n, l, (const u64 *)w.keys_out, (const int *)w.flags,
                           (const int *)w.rank, w.ukeys[l], T->counts, T->status);
        if (l == 0) {
            // `order` of level 0 is the row of every sorted key: kept for the table launches below
            if (hipMemcpyAsync(w.rows0, w.order, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return PTV2_ERR_LAUNCH;
        }
    }
    const int *rows0 = w.rows0;
    hipLaunchKernelGGL(nbr_kernel<5>, dim3(divup((long long)n * 125, TPB)), dim3(TPB), 0, st, n, (const int *)T->counts,
                       (const u64 *)w.ukeys[0], rows0, T->nbr5);
    for (int l = 0; l < SPCONV_LEVELS; ++l)
        hipLaunchKernelGGL(nbr_kernel<3>, dim3(divup((long long)n * 27, TPB)), dim3(TPB), 0, st, n, (const int *)(T->counts + l),
                           (const u64 *)w.ukeys[l], l == 0 ? rows0 : (const int *)nullptr, T->nbr3[l]);
    for (int l = 0; l + 1 < SPCONV_LEVELS; ++l) {
        const int *fr = l == 0 ? rows0 : (const int *)nullptr;
        hipLaunchKernelGGL(child_kernel, dim3(divup((long long)n * 8, TPB)), dim3(TPB), 0, st, n, (const int *)(T->counts + l),
                           (const int *)(T->counts + l + 1), (const u64 *)w.ukeys[l], fr, (const u64 *)w.ukeys[l + 1], T->child[l]);
        hipLaunchKernelGGL(parent_kernel, dim3(divup(std::max(n, b), TPB)), dim3(TPB), 0, st, n, b, (const int *)(T->counts + l),
                           (const int *)(T->counts + l + 1), (const u64 *)w.ukeys[l], fr, (const u64 *)w.ukeys[l + 1], T->parent[l],
                           T->slot[l], T->coord[l], T->offset[l]);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
