// ao_amd/csrc/swin_map.hip -- the window map of Swin3D's window attention (include/ptv2_swin_hip.h).
// gfx950 only.
//
// Three small passes around one sort and one scan that python runs between them:
//   keys     voxel -> cloud << 48 | wx << 35 | wy << 22 | wz << 9 | w_w_id, the window coordinates by FLOOR division of
//            grid_coord + shift, so that an ascending sort orders the voxels by window and, inside a window, by slot;
//   heads    sorted keys -> 1 at the first voxel of every window, the slot's (x, y, z), and the duplicate flag;
//   offsets  the inclusive scan of the heads -> the CSR over the windows, their count and the largest one.
// No (windows, ws^3) tensor, mask or pair list is formed.
#include "common.h"
#include "../../include/ptv2_swin_hip.h"

#define SWIN_MAP_TPB 256
#define SWIN_SLOT_BITS 9
#define SWIN_COORD_BITS 13

__device__ __forceinline__ int swin_floor_div(int a, int b) {
    const int q = a / b;
    return a % b < 0 ? q - 1 : q;
}

__global__ __launch_bounds__(SWIN_MAP_TPB) void swin_map_keys_kernel(swin_args a) {
    const int i = blockIdx.x * SWIN_MAP_TPB + threadIdx.x;
    if (i >= a.n) return;
    const int ws = a.window_size, b = a.batch[i];
    bool bad = b < 0 || b >= SWIN_MAX_CLOUDS;
    long long key = (long long)(bad ? 0 : b);
    int slot = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int g = a.grid_coord[3 * (size_t)i + ax];
        // (the sum cannot wrap for a coordinate that passes the range check below)
        const int w = g > -(1 << 20) && g < (1 << 20) ?swin_floor_div(g + a.shift, ws) : SWIN_WINDOW_BIAS;
        bad |= w < -SWIN_WINDOW_BIAS || w >= SWIN_WINDOW_BIAS;
        key = key << SWIN_COORD_BITS | (long long)((w + SWIN_WINDOW_BIAS) & (2 * SWIN_WINDOW_BIAS - 1));
        slot = slot * ws + (bad ? 0 : g + a.shift - w * ws);
    }
    a.keys_out[i] = key << SWIN_SLOT_BITS | slot;
    if (bad) a.stat[0] = 1;
}

__global__ __launch_bounds__(SWIN_MAP_TPB) void swin_map_heads_kernel(swin_args a) {
    const int i = blockIdx.x * SWIN_MAP_TPB + threadIdx.x;
    if (i >= a.n) return;
    const int ws = a.window_size;
    const long long key = a.keys[i], before = i ? a.keys[i - 1] : -1;
    a.head_out[i] = i == 0 || (key >> SWIN_SLOT_BITS) != (before >> SWIN_SLOT_BITS);
    if (key == before) a.stat[1] = 1;
    const int slot = (int)(key & ((1 << SWIN_SLOT_BITS) - 1));
    a.w_w_xyz_out[3 * (size_t)i] = slot / (ws * ws);
    a.w_w_xyz_out[3 * (size_t)i + 1] = slot / ws % ws;
    a.w_w_xyz_out[3 * (size_t)i + 2] = slot % ws;
}

// wid is the inclusive scan of head: the window of sorted position i is wid[i] - 1
__global__ __launch_bounds__(SWIN_MAP_TPB) void swin_map_offsets_kernel(swin_args a) {
    const int i = blockIdx.x * SWIN_MAP_TPB + threadIdx.x;
    if (i >= a.n) return;
    if (a.head[i]) a.offsets_out[a.wid[i] - 1] = i;
    if (i == a.n - 1) {
        a.offsets_out[a.wid[i]] = a.n;
        a.stat[2] = a.wid[i];
    }
}

__global__ __launch_bounds__(SWIN_MAP_TPB) void swin_map_largest_kernel(swin_args a) {
    const int i = blockIdx.x * SWIN_MAP_TPB + threadIdx.x;
    if (i >= a.n) return;
    if (i == a.n - 1 || a.head[i + 1]) atomicMax(&a.stat[3], i + 1 - a.offsets_out[a.wid[i] - 1]);
}

static int swin_map_check(const swin_args *a) {
    if (!a || a->n < 1 || a->window_size < 1 || a->window_size > SWIN_MAX_WINDOW || !a->stat) return PTV2_ERR_ARG;
    return PTV2_OK;
}

#define SWIN_MAP_LAUNCH(kernel) \
    hipLaunchKernelGGL(kernel, dim3(divup(args->n, SWIN_MAP_TPB)), dim3(SWIN_MAP_TPB), 0, (hipStream_t)stream, *args); \
    PTV2_CHECK_LAUNCH()

extern "C" int swin_map_keys_hip_launcher(const swin_args *args, void *stream) {
    RUN(swin_map_check(args));
    if (!args->grid_coord || !args->batch || !args->keys_out || abs(args->shift) > (1 << 20)) return PTV2_ERR_ARG;
    SWIN_MAP_LAUNCH(swin_map_keys_kernel);
    return PTV2_OK;
}

extern "C" int swin_map_heads_hip_launcher(const swin_args *args, void *stream) {
    RUN(swin_map_check(args));
    if (!args->keys || !args->head_out || !args->w_w_xyz_out) return PTV2_ERR_ARG;
    SWIN_MAP_LAUNCH(swin_map_heads_kernel);
    return PTV2_OK;
}

extern "C" int swin_map_offsets_hip_launcher(const swin_args *args, void *stream) {
    RUN(swin_map_check(args));
    if (!args->head || !args->wid || !args->offsets_out) return PTV2_ERR_ARG;
    SWIN_MAP_LAUNCH(swin_map_offsets_kernel);
    SWIN_MAP_LAUNCH(swin_map_largest_kernel);
    return PTV2_OK;
}
