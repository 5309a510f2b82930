// ao_amd/csrc/pp2s.hip -- the PP2S label pipeline (gfx950), include/ptv2_pp2s_hip.h.  What three numpy scripts of the
// reference do per room on the host:
//   pointcept/utils/my_make_bridge_final.py:94-96      the room's alignment                              -> pp2s_align
//                                          :128-153    per view: projection, bounds, depth test, bridge   -> pp2s_project
//   my_choose_weak_label_final.py:71-88                one labelled point per instance                    -> pp2s_weak
//   my_run_sam_final.py:83-114                         per view and prompt: a python loop over every visible point with a
//                                                      dict of dicts as vote table                       -> pp2s_pixel_labels, pp2s_vote
//                      :47-60, :117-122                the labels, the weak points written over           -> pp2s_labels
// A point's final label depends only on the SET of classes it collected, so the votes are one bit per class: pass A folds
// a view's masks into one (H, W) word image (P * H * W bytes streamed once), pass B is one gather per visible point.
// Floating point is restated one rounding at a time (the unit is compiled with contraction off, see the Makefile);
// everything else is integer and does not depend on execution order.  Every index derived from input data is range
// checked; a bad one is skipped and recorded in the status word.
#include <limits.h>

#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "common.h"
#include "../../include/ptv2_pp2s_hip.h"

extern "C" int ptv2_pp2s_abi_version(void) { return 1; }  // == EXPECTED_PP2S_ABI in ao_amd/_lib.py

namespace {

constexpr int PTPB = 256;
constexpr int PMAX_BLOCKS = 256 * 8;
typedef unsigned long long u64;

int point_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + PTPB - 1) / PTPB, PMAX_BLOCKS)); }

struct Mat34 { double m[12]; };

// row r of m times (x, y, z, 1): ((m0 x + m1 y) + m2 z) + m3
__device__ __forceinline__ double row_dot(const Mat34 &a, int r, double x, double y, double z) {
    const double s = __dadd_rn(__dmul_rn(a.m[4 * r], x), __dmul_rn(a.m[4 * r + 1], y));
    return __dadd_rn(__dadd_rn(s, __dmul_rn(a.m[4 * r + 2], z)), a.m[4 * r + 3]);
}

// ----------------------------------------------------------------------------------------------------------- align --
// the rotation's row is the fused chain a dgemm kernel runs over k: round(t.x * m0), then fma(t.y, m1, .); the third term
// (t.z * 0, or 0 * t.x + 0 * t.y for z) adds nothing
__global__ __launch_bounds__(PTPB) void pp2s_align_kernel(long long n, const float *__restrict__ coord, double cx, double cy,
                                                          double cz, double rc, double rs, double *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * PTPB + threadIdx.x; i < n; i += (long long)gridDim.x * PTPB) {
        const double tx = (double)(float)__dsub_rn((double)coord[3 * i], cx);
        const double ty = (double)(float)__dsub_rn((double)coord[3 * i + 1], cy);
        const double tz = (double)(float)__dsub_rn((double)coord[3 * i + 2], cz);
        out[3 * i] = __dadd_rn(__fma_rn(ty, -rs, __dmul_rn(tx, rc)), cx);
        out[3 * i + 1] = __dadd_rn(__fma_rn(ty, rc, __dmul_rn(tx, rs)), cy);
        out[3 * i + 2] = __dadd_rn(tz, cz);
    }
}

// --------------------------------------------------------------------------------------------------------- project --
__global__ __launch_bounds__(PTPB) void pp2s_project_kernel(long long n, const double *__restrict__ coord, Mat34 krt, Mat34 rt,
                                                            const double *__restrict__ depth, int depth_h, int depth_w,
                                                            double height, double width, double tol, int *__restrict__ bridge,
                                                            unsigned char *__restrict__ seen_any, int *status) {
    // (the trip count is uniform over the wave: the ballot below is reached by all 64 lanes)
    const long long step = (long long)gridDim.x * PTPB;
    for (long long base = (long long)blockIdx.x * PTPB; base < n; base += step) {
        const long long i = base + threadIdx.x;
        bool visible = false;
        int bx = 0, by = 0;
        if (i < n) {
            const double x = coord[3 * i], y = coord[3 * i + 1], z = coord[3 * i + 2];
            const double pz = row_dot(krt, 2, x, y, z);
            const double rx = rint(__ddiv_rn(row_dot(krt, 0, x, y, z), pz));
            const double ry = rint(__ddiv_rn(row_dot(krt, 1, x, y, z), pz));
            if (rx > 0.0 && ry > 0.0 && rx < height && ry < width) {  // height, width <= 65535: the casts are exact
                bx = (int)rx;
                by = (int)ry;
                if (bx >= depth_w || by >= depth_h) {
                    atomicOr(status + PTV2_PP2S_STATUS_ERROR, PTV2_PP2S_BAD_PIXEL);
                } else {
                    const double d = depth[(long long)by * depth_w + bx];
                    visible = fabs(__dsub_rn(d, row_dot(rt, 2, x, y, z))) < tol;
                }
            }
            bridge[3 * i] = visible ? bx : 0;
            bridge[3 * i + 1] = visible ? by : 0;
            bridge[3 * i + 2] = visible ? 1 : 0;
            if (visible && seen_any) seen_any[i] = 1;
        }
        const u64 b = __ballot(visible);
        if ((threadIdx.x & (WAVE - 1)) == 0 && b) atomicAdd(status + PTV2_PP2S_STATUS_VISIBLE, __popcll(b));
    }
}

// ------------------------------------------------------------------------------------------------------------ weak --
__global__ __launch_bounds__(PTPB) void pp2s_weak_keys_kernel(int n, const int *__restrict__ instance, u64 *__restrict__ keys) {
    for (long long i = (long long)blockIdx.x * PTPB + threadIdx.x; i < n; i += (long long)gridDim.x * PTPB)
        keys[i] = ((u64)((unsigned)instance[i] ^ 0x80000000u) << 32) | (u64)(unsigned)i;  // signed order, then index
}

__global__ __launch_bounds__(PTPB) void pp2s_weak_flags_kernel(int n, const u64 *__restrict__ keys,
                                                               const unsigned char *__restrict__ seen_any, int *__restrict__ flags) {
    for (long long j = (long long)blockIdx.x * PTPB + threadIdx.x; j < n; j += (long long)gridDim.x * PTPB) {
        const unsigned i = (unsigned)keys[j];  // a permutation of [0, n): written by pp2s_weak_keys_kernel
        flags[j] = i < (unsigned)n && seen_any[i] ? 1 : 0;
    }
}

// one lane per sorted position; the head of a segment (the first key of an instance) finds the segment's end and the
// position of its weak point by bisection.  seen[j]: inclusive sum of the flags
__global__ __launch_bounds__(PTPB) void pp2s_weak_select_kernel(int n, const u64 *__restrict__ keys, const int *__restrict__ flags,
                                                                const int *__restrict__ seen, unsigned char *__restrict__ weak) {
    for (long long j = (long long)blockIdx.x * PTPB + threadIdx.x; j < n; j += (long long)gridDim.x * PTPB) {
        const unsigned inst = (unsigned)(keys[j] >> 32);
        if (j > 0 && (unsigned)(keys[j - 1] >> 32) == inst) continue;
        long long lo = j + 1, hi = n;  // the first position whose instance is another one
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if ((unsigned)(keys[mid] >> 32) == inst) lo = mid + 1; else hi = mid;
        }
        const long long end = lo;
        const int before = seen[j] - flags[j], count_seen = seen[end - 1] - before;
        long long at = j + (end - j) / 2;
        if (count_seen > 0) {
            const int target = before + count_seen / 2 + 1;  // the first position whose inclusive sum reaches it is a seen one
            lo = j, hi = end - 1;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (seen[mid] >= target) hi = mid; else lo = mid + 1;
            }
            at = lo;
        }
        const unsigned i = (unsigned)keys[at];
        if (i < (unsigned)n) weak[i] = 1;
    }
}

// ----------------------------------------------------------------------------------------------------------- votes --
// the bit of prompt p, 0 for a label outside [0, c) (reported by block 0)
__device__ __forceinline__ unsigned prompt_bit(const int *__restrict__ prompt_label, int p, int c) {
    const int l = prompt_label[p];
    return (unsigned)l < (unsigned)c ? 1u << l : 0u;
}

__device__ __forceinline__ void report_labels(int prompts, int c, const int *__restrict__ prompt_label, int *status) {
    if (blockIdx.x != 0) return;
    for (int p = threadIdx.x; p < prompts; p += PTPB)
        if ((unsigned)prompt_label[p] >= (unsigned)c) atomicOr(status + PTV2_PP2S_STATUS_ERROR, PTV2_PP2S_BAD_CLASS);
}

// pass A, hw % 4 == 0 and masks 4-byte aligned: the image as a flat run of dwords, four pixels per lane
__global__ __launch_bounds__(PTPB) void pp2s_pixel_labels_quad_kernel(int prompts, int c, const int *__restrict__ prompt_label,
                                                                      const unsigned *__restrict__ masks, long long quads,
                                                                      uint4 *__restrict__ pixbits, int *status) {
    report_labels(prompts, c, prompt_label, status);
    for (long long q = (long long)blockIdx.x * PTPB + threadIdx.x; q < quads; q += (long long)gridDim.x * PTPB) {
        uint4 bits = make_uint4(0u, 0u, 0u, 0u);
        const unsigned *m = masks + q;
#pragma unroll 4
        for (int p = 0; p < prompts; ++p) {
            const unsigned w = m[(long long)p * quads], bit = prompt_bit(prompt_label, p, c);
            bits.x |= (w & 0x000000ffu) ? bit : 0u;
            bits.y |= (w & 0x0000ff00u) ? bit : 0u;
            bits.z |= (w & 0x00ff0000u) ? bit : 0u;
            bits.w |= (w & 0xff000000u) ? bit : 0u;
        }
        pixbits[q] = bits;
    }
}

// pass A, any size and alignment: four pixels per lane as bytes, the tail of the image by its last lane
__global__ __launch_bounds__(PTPB) void pp2s_pixel_labels_byte_kernel(int prompts, int c, const int *__restrict__ prompt_label,
                                                                      const unsigned char *__restrict__ masks, long long hw,
                                                                      unsigned *__restrict__ pixbits, int *status) {
    report_labels(prompts, c, prompt_label, status);
    const long long quads = (hw + 3) / 4;
    for (long long q = (long long)blockIdx.x * PTPB + threadIdx.x; q < quads; q += (long long)gridDim.x * PTPB) {
        const long long e0 = 4 * q;
        const int count = (int)min(4LL, hw - e0);
        unsigned bits[4] = {0u, 0u, 0u, 0u};
        for (int p = 0; p < prompts; ++p) {
            const unsigned char *m = masks + (long long)p * hw + e0;
            const unsigned bit = prompt_bit(prompt_label, p, c);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < count && m[k]) bits[k] |= bit;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < count) pixbits[e0 + k] = bits[k];
    }
}

// pass B
__global__ __launch_bounds__(PTPB) void pp2s_vote_kernel(long long n, const int *__restrict__ bridge, int height, int width,
                                                         const unsigned *__restrict__ pixbits, unsigned *__restrict__ seen_bits,
                                                         int *status) {
    for (long long i = (long long)blockIdx.x * PTPB + threadIdx.x; i < n; i += (long long)gridDim.x * PTPB) {
        if (bridge[3 * i + 2] != 1) continue;
        const int u = bridge[3 * i], v = bridge[3 * i + 1];
        if (u < 0 || u > width || v < 0 || v > height) {
            atomicOr(status + PTV2_PP2S_STATUS_ERROR, PTV2_PP2S_BAD_PIXEL);
            continue;
        }
        const int row = v == 0 ? height - 1 : v - 1, col = u == 0 ? width - 1 : u - 1;  // python's index -1
        const unsigned bits = pixbits[(long long)row * width + col];
        if (bits) seen_bits[i] |= bits;
    }
}

// ---------------------------------------------------------------------------------------------------------- labels --
__global__ __launch_bounds__(PTPB) void pp2s_labels_kernel(long long n, const unsigned *__restrict__ seen_bits,
                                                           const unsigned char *__restrict__ weak, const int *__restrict__ gt,
                                                           int *__restrict__ label) {
    for (long long i = (long long)blockIdx.x * PTPB + threadIdx.x; i < n; i += (long long)gridDim.x * PTPB) {
        const unsigned bits = seen_bits[i];
        int out = __popc(bits) == 1 ? __ffs(bits) - 1 : -1;  // (bit 31 too: __ffs takes the word as it is)
        const int g = gt[i];
        if (weak[i] && g != -1) out = g;
        label[i] = out;
    }
}

bool bad_n(long long n) { return n < 0 || n > INT_MAX; }
bool bad_image(int height, int width) { return height < 1 || width < 1 || (long long)height * width > INT_MAX; }

struct WeakSpace { u64 *keys_in, *keys_out; int *flags, *seen; void *cub; size_t cub_bytes; };
size_t carve_weak(char *ws, long long n, WeakSpace &s) {
    PtvCarver k{ws, 0};
    s.keys_in = k.take_n<u64>((size_t)n);
    s.keys_out = k.take_n<u64>((size_t)n);
    s.flags = k.take_n<int>((size_t)n);
    s.seen = k.take_n<int>((size_t)n);
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, s1, (const u64 *)nullptr, (u64 *)nullptr, (int)n, 0, 64, (hipStream_t)0);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, s2, (const int *)nullptr, (int *)nullptr, (int)n, (hipStream_t)0);
    s.cub_bytes = std::max(s1, s2) + 256;
    s.cub = k.take(s.cub_bytes);
    return k.off;
}
size_t image_bytes(int height, int width) { return ptv2_align256(sizeof(unsigned) * (size_t)height * (size_t)width); }

}  // namespace

extern "C" long long pp2s_workspace_bytes(long long n, int height, int width) {
    if (bad_n(n) || height < 0 || width < 0) return -1;
    const bool image = height > 0 && width > 0;
    if (image && bad_image(height, width)) return -1;
    WeakSpace s;
    const size_t weak = n ? carve_weak(nullptr, n, s) : 0;
    return (long long)std::max(weak, image ? image_bytes(height, width) : (size_t)0);
}

extern "C" int pp2s_align_hip_launcher(long long n, const float *coord, double cx, double cy, double cz, double rot_cos,
                                       double rot_sin, double *out, void *stream) {
    if (bad_n(n)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!coord || !out) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(pp2s_align_kernel, dim3(point_grid(n)), dim3(PTPB), 0, (hipStream_t)stream, n, coord, cx, cy, cz, rot_cos,
                       rot_sin, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pp2s_project_hip_launcher(long long n, const double *coord64, double k00, double k01, double k02, double k03,
                                         double k10, double k11, double k12, double k13, double k20, double k21, double k22,
                                         double k23, double r00, double r01, double r02, double r03, double r10, double r11,
                                         double r12, double r13, double r20, double r21, double r22, double r23,
                                         const double *depth, int depth_h, int depth_w, double height, double width, double tol,
                                         int *bridge, void *seen_any, int *status, void *stream) {
    if (bad_n(n) || bad_image(depth_h, depth_w) || !status) return PTV2_ERR_ARG;
    if (!(height <= (double)PTV2_PP2S_MAX_BOUND) || !(width <= (double)PTV2_PP2S_MAX_BOUND) || !(tol >= 0.0)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!coord64 || !depth || !bridge) return PTV2_ERR_ARG;
    const Mat34 krt = {{k00, k01, k02, k03, k10, k11, k12, k13, k20, k21, k22, k23}};
    const Mat34 rt = {{r00, r01, r02, r03, r10, r11, r12, r13, r20, r21, r22, r23}};
    hipLaunchKernelGGL(pp2s_project_kernel, dim3(point_grid(n)), dim3(PTPB), 0, (hipStream_t)stream, n, coord64, krt, rt, depth,
                       depth_h, depth_w, height, width, tol, bridge, (unsigned char *)seen_any, status);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pp2s_weak_hip_launcher(long long n, const int *instance, const void *seen_any, void *weak, void *workspace,
                                      long long workspace_bytes, void *stream) {
    if (bad_n(n)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!instance || !seen_any || !weak || !workspace) return PTV2_ERR_ARG;
    WeakSpace s;
    if ((long long)carve_weak((char *)workspace, n, s) > workspace_bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int count = (int)n, grid = point_grid(n);
    if (hipMemsetAsync(weak, 0, (size_t)n, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(pp2s_weak_keys_kernel, dim3(grid), dim3(PTPB), 0, st, count, instance, s.keys_in);
    size_t cb = s.cub_bytes;
    if (hipcub::DeviceRadixSort::SortKeys(s.cub, cb, (const u64 *)s.keys_in, s.keys_out, count, 0, 64, st) != hipSuccess)
        return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(pp2s_weak_flags_kernel, dim3(grid), dim3(PTPB), 0, st, count, (const u64 *)s.keys_out,
                       (const unsigned char *)seen_any, s.flags);
    cb = s.cub_bytes;
    if (hipcub::DeviceScan::InclusiveSum(s.cub, cb, (const int *)s.flags, s.seen, count, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(pp2s_weak_select_kernel, dim3(grid), dim3(PTPB), 0, st, count, (const u64 *)s.keys_out, (const int *)s.flags,
                       (const int *)s.seen, (unsigned char *)weak);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pp2s_pixel_labels_hip_launcher(int prompts, int c, const int *prompt_label, const void *masks, int height,
                                              int width, void *workspace, long long workspace_bytes, int *status, void *stream) {
    if (prompts < 0 || c < PTV2_PP2S_MIN_C || c > PTV2_PP2S_MAX_C || bad_image(height, width) || !status || !workspace)
        return PTV2_ERR_ARG;
    if (prompts > 0 && (!prompt_label || !masks)) return PTV2_ERR_ARG;
    if ((long long)image_bytes(height, width) > workspace_bytes) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long long hw = (long long)height * width;
    if (prompts == 0) {
        if (hipMemsetAsync(workspace, 0, sizeof(unsigned) * (size_t)hw, st) != hipSuccess) return PTV2_ERR_LAUNCH;
        return PTV2_OK;
    }
    const long long quads = (hw + 3) / 4;
    if (hw % 4 == 0 && ((uintptr_t)masks & 3) == 0 && ((uintptr_t)workspace & 15) == 0)
        hipLaunchKernelGGL(pp2s_pixel_labels_quad_kernel, dim3(point_grid(quads)), dim3(PTPB), 0, st, prompts, c, prompt_label,
                           (const unsigned *)masks, quads, (uint4 *)workspace, status);
    else
        hipLaunchKernelGGL(pp2s_pixel_labels_byte_kernel, dim3(point_grid(quads)), dim3(PTPB), 0, st, prompts, c, prompt_label,
                           (const unsigned char *)masks, hw, (unsigned *)workspace, status);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pp2s_vote_hip_launcher(long long n, const int *bridge, int height, int width, const void *workspace,
                                      long long workspace_bytes, unsigned *seen_bits, int *status, void *stream) {
    if (bad_n(n) || bad_image(height, width) || !status) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!bridge || !workspace || !seen_bits) return PTV2_ERR_ARG;
    if ((long long)image_bytes(height, width) > workspace_bytes) return PTV2_ERR_WORKSPACE;
    hipLaunchKernelGGL(pp2s_vote_kernel, dim3(point_grid(n)), dim3(PTPB), 0, (hipStream_t)stream, n, bridge, height, width,
                       (const unsigned *)workspace, seen_bits, status);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int pp2s_labels_hip_launcher(long long n, const unsigned *seen_bits, const void *weak, const int *gt, int *label,
                                        void *stream) {
    if (bad_n(n)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!seen_bits || !weak || !gt || !label) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(pp2s_labels_kernel, dim3(point_grid(n)), dim3(PTPB), 0, (hipStream_t)stream, n, seen_bits,
                       (const unsigned char *)weak, gt, label);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
