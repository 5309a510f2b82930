// ao_amd/csrc/spconv_bf16.hip -- the matrix-core forms of SpUNet-v1m1's sparse convolutions with bf16 operands
// (include/ptv2_spconv_bf16_hip.h): the semantics of spconv.hip, the operands rounded to bf16 (nearest even) on their way
// into V_MFMA_F32_16X16X32_BF16, fp32 accumulation, fp32 in memory on both sides.
//
//   pack_weight_kernel        W (Cout, K, Cin) fp32 -> [kappa][a][b] bf16 in the call's workspace, a the output channel of THIS
//                             call, b its reduction index, contiguous: the transposed form W[kappa]^T is another packing of
//                             the same weight (a 32 x 32 tile turned in LDS), not a strided read inside the convolution
//   conv_bf16_kernel<NT, F>   GATHER / SCATTER as conv_kernel: 64 table rows x 16 NT output channels per workgroup, the table
//                             tile in LDS, a kappa no row of the tile has is skipped by the workgroup, a kappa none of a wave's 16
//                             rows has costs that wave no matrix instruction; per kappa 64 reduction indices per LDS stage,
//                             the gathered fp32 rows rounded while they are written; one 16-byte LDS read per operand
//   wgrad_bf16_kernel<NJ>     gW[kappa] partial sums per (kappa, row split): the reduction index is the ROW, so both LDS
//                             images are written transposed ([channel][row]) while they are rounded; 64 rows per stage, 32
//                             per matrix instruction; wgrad_bf16_reduce_kernel adds the splits in order
// The stem and the 1 x 1 x 1 convolutions stay fp32 (spconv.hip, gemm.hip).  No atomics anywhere.
#include <algorithm>

#include "common.h"
#include "../../include/ptv2_spconv_bf16_hip.h"

namespace {

constexpr int TM = 64;     // table rows per workgroup
constexpr int KC = 64;     // reduction indices per LDS stage (spconv.hip: 32 floats; the same bytes, half the barriers)
// Pitch of an LDS row in bf16.  A lane reads 16 bytes: reduction indices 8 q .. 8 q + 7 (q = lane >> 4) of row lane & 15, at
// byte 144 r + 16 q.  The 64 banks are 256 bytes, i.e. 16 slots of 16 bytes, and a 16-byte read is served 16 lanes at a time:
// 144 r mod 256 = 16 (9 r mod 16), and 9 is odd, so the rows 0 .. 15 of one q fall on the 16 distinct slots.  Any pitch of
// 16 bytes mod 128 with an odd multiple of 16 does the same; 72 is the smallest one that holds KC.  144 is a multiple of 16:
// every read and every 16-byte write is aligned.
constexpr int PITCH = KC + 8;
constexpr int MAX_K = 27;  // columns of a table on the matrix-core forms
constexpr int SPLIT_ROWS = 1024;  // rows per split of the weight gradient, up to SPCONV_MAX_SPLITS splits (as spconv.hip)
static_assert((PITCH * 2) % 128 == 16 && PITCH >= KC, "bank-conflict-free 16-byte reads");

// W[co][kappa][ci] -> P[kappa][a][b]: (a, b) = (co, ci), or (ci, co) when transposed.  One 32 x 32 (co, ci) tile per block.
__global__ __launch_bounds__(256) void pack_weight_kernel(int K, int cin, int cout, const float *__restrict__ W, int transpose,
                                                          __bf16 *__restrict__ P) {
    __shared__ float tile[32][33];
    const int kap = blockIdx.x, co0 = blockIdx.y * 32, ci0 = blockIdx.z * 32;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = hi + 8 * i;
        tile[co][lo] = W[((size_t)(co0 + co) * K + kap) * cin + ci0 + lo];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = hi + 8 * i;
        if (transpose) P[((size_t)kap * cin + ci0 + row) * cout + co0 + lo] = (__bf16)tile[lo][row];
        else P[((size_t)kap * cout + co0 + row) * cin + ci0 + lo] = (__bf16)tile[row][lo];
    }
}

// cin, cout: the widths of THIS call (the transposed form swapped by the launcher); Wp [kappa][cout][cin] bf16
template <int NT, int FORM>
__global__ __launch_bounds__(256) void conv_bf16_kernel(int n_tab, int n_other, int K, int cin, int cout,
                                                        const float *__restrict__ in, const int *__restrict__ tab,
                                                        const __bf16 *__restrict__ Wp, int reverse, float *__restrict__ out) {
    constexpr int CN = NT * 16;
    __shared__ __attribute__((aligned(16))) __bf16 sX[TM * PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 sW[CN * PITCH];
    __shared__ int sTab[TM * MAX_K];
    __shared__ int sAny[MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row0 = blockIdx.x * TM, n0 = blockIdx.y * CN;
    for (int e = tid; e < TM * K; e += 256) {
        const int r = e / K, kap = e - r * K, row = row0 + r;
        int j = -1;
        if (row < n_tab) {
            j = tab[(size_t)row * K + (reverse ? K - 1 - kap : kap)];
            if (j >= n_other) j = -1;  // (never in a table the library built)
        }
        sTab[e] = j;
    }
    __syncthreads();
    if (tid < K) {
        int any = 0;
        for (int r = 0; r < TM; ++r) any |= sTab[r * K + tid] >= 0;
        sAny[tid] = any;
    }
    __syncthreads();
    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    const int my_row = 16 * w + (lane & 15), quad = lane >> 4;
    for (int kap = 0; kap < K; ++kap) {
        if (!sAny[kap]) continue;  // (the same for every thread of the workgroup)
        const int my_j = sTab[my_row * K + kap];
        // a row without the column is a row of zeros (GATHER) or is not stored (SCATTER): a wave whose 16 rows all lack it
        // has nothing to add, it only helps to load and meets the barriers
        const bool wave_has = __ballot(my_j >= 0) != 0;
        if (FORM == SPCONV_SCATTER) {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
        }
        for (int c0 = 0; c0 < cin; c0 += KC) {
            const int kc = min(KC, cin - c0);  // 64, or 32 in the last stage of a width that is 32 mod 64
#pragma unroll
            for (int i = 0; i < TM * KC / 8 / 256; ++i) {
                const int e = tid + 256 * i, r = e >> 3, o = e & 7;
                if (8 * o >= kc) continue;
                int src;
                if (FORM == SPCONV_GATHER) src = sTab[r * K + kap];
                else src = row0 + r < n_tab && sTab[r * K + kap] >= 0 ? row0 + r : -1;
                float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
                if (src >= 0) {
                    const float *p = in + (size_t)src * cin + c0 + 8 * o;
                    lo = *(const float4 *)p;
                    hi = *(const float4 *)(p + 4);
                }
                *(ptv2_bf16x8 *)(sX + r * PITCH + 8 * o) = ptv2_pack_bf16(lo, hi);
            }
            for (int e = tid; e < CN * (KC / 8); e += 256) {
                const int a = e >> 3, o = e & 7;
                if (8 * o >= kc) continue;
                *(ptv2_bf16x8 *)(sW + a * PITCH + 8 * o) = *(const ptv2_bf16x8 *)(Wp + ((size_t)kap * cout + n0 + a) * cin + c0 + 8 * o);
            }
            __syncthreads();
            if (wave_has) {
                for (int kk = 0; kk < kc / 32; ++kk) {
                    const ptv2_bf16x8 xv = *(const ptv2_bf16x8 *)(sX + my_row * PITCH + 32 * kk + 8 * quad);
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            *(const ptv2_bf16x8 *)(sW + (16 * t + (lane & 15)) * PITCH + 32 * kk + 8 * quad), xv, acc[t], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        if (FORM == SPCONV_SCATTER && my_j >= 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                *(float4 *)(out + (size_t)my_j * cout + n0 + 16 * t + 4 * quad) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
        }
    }
    if (FORM == SPCONV_GATHER && row0 + my_row < n_tab) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            *(float4 *)(out + (size_t)(row0 + my_row) * cout + n0 + 16 * t + 4 * quad) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient ----------
constexpr int RC = 64;  // rows per stage: two matrix instructions deep
// part[(kappa * splits + s)][co][ci]; a workgroup owns (kappa, s), 32 output and 32 NJ input channels.  The matrix instruction
// wants 8 consecutive reduction indices -- rows -- per lane, so the images are [channel][row], PITCH bf16 per channel, read as
// conv_bf16_kernel reads (conflict-free).  They are written two rows at a time: a thread holds channels 4 q .. 4 q + 3 of rows
// 2 p and 2 p + 1 and writes four 32-bit words, one per channel, at word 36 (4 q + c) + p; with q = tid & 7 (the global read of
// a row is one 128-byte line per 8 lanes) q and q + 4 share a bank: a two-way conflict on the write, none on the 16-byte reads.
template <int NJ>
__global__ __launch_bounds__(256) void wgrad_bf16_kernel(int n_tab, int n_other, int K, int cin, int cout,
                                                         const float *__restrict__ x, const float *__restrict__ g,
                                                         const int *__restrict__ tab, int gather_g, int splits,
                                                         int rows_per_split, float *__restrict__ part) {
    constexpr int XW = 32 * NJ;
    __shared__ __attribute__((aligned(16))) __bf16 sG[32 * PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 sXc[XW * PITCH];
    __shared__ int sJ[RC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int kap = blockIdx.x / splits, s = blockIdx.x - kap * splits;
    const int co0 = blockIdx.y * 32, ci0 = blockIdx.z * XW;
    const int r_begin = s * rows_per_split, r_end = min(n_tab, r_begin + rows_per_split);
    v4f acc[NJ];
#pragma unroll
    for (int u = 0; u < NJ; ++u) acc[u] = v4f{0.f, 0.f, 0.f, 0.f};
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    for (int rb = r_begin; rb < r_end; rb += RC) {
        int j = -1;
        if (tid < RC && rb + tid < r_end) {
            j = tab[(size_t)(rb + tid) * K + kap];
            if (j >= n_other) j = -1;
        }
        if (tid < RC) sJ[tid] = j;
        if (!__syncthreads_or(j >= 0)) continue;  // no row of this stage has the column
        {
            const int p = tid >> 3, q = tid & 7, j0 = sJ[2 * p], j1 = sJ[2 * p + 1];
            const long long r0 = rb + 2 * p, r1 = r0 + 1;
            const long long g0 = gather_g ? j0 : r0, g1 = gather_g ? j1 : r1, x0 = gather_g ? r0 : j0, x1 = gather_g ? r1 : j1;
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            float4 a = zero, b = zero;
            if (j0 >= 0) a = *(const float4 *)(g + (size_t)g0 * cout + co0 + 4 * q);
            if (j1 >= 0) b = *(const float4 *)(g + (size_t)g1 * cout + co0 + 4 * q);
            bf16x2 *dg = (bf16x2 *)sG + (4 * q) * (PITCH / 2) + p;
            dg[0] = bf16x2{(__bf16)a.x, (__bf16)b.x};
            dg[PITCH / 2] = bf16x2{(__bf16)a.y, (__bf16)b.y};
            dg[PITCH] = bf16x2{(__bf16)a.z, (__bf16)b.z};
            dg[3 * (PITCH / 2)] = bf16x2{(__bf16)a.w, (__bf16)b.w};
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                a = zero, b = zero;
                if (j0 >= 0) a = *(const float4 *)(x + (size_t)x0 * cin + ci0 + 32 * u + 4 * q);
                if (j1 >= 0) b = *(const float4 *)(x + (size_t)x1 * cin + ci0 + 32 * u + 4 * q);
                bf16x2 *dx = (bf16x2 *)sXc + (32 * u + 4 * q) * (PITCH / 2) + p;
                dx[0] = bf16x2{(__bf16)a.x, (__bf16)b.x};
                dx[PITCH / 2] = bf16x2{(__bf16)a.y, (__bf16)b.y};
                dx[PITCH] = bf16x2{(__bf16)a.z, (__bf16)b.z};
                dx[3 * (PITCH / 2)] = bf16x2{(__bf16)a.w, (__bf16)b.w};
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int id = w + 4 * u, co_sub = id & 1, ci_sub = id >> 1;
#pragma unroll
            for (int kk = 0; kk < RC / 32; ++kk)
                acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    *(const ptv2_bf16x8 *)(sG + (16 * co_sub + (lane & 15)) * PITCH + 32 * kk + 8 * (lane >> 4)),
                    *(const ptv2_bf16x8 *)(sXc + (16 * ci_sub + (lane & 15)) * PITCH + 32 * kk + 8 * (lane >> 4)), acc[u], 0, 0, 0);
        }
        __syncthreads();
    }
    float *p = part + (size_t)blockIdx.x * cout * cin;
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
        const int id = w + 4 * u, co_sub = id & 1, ci_sub = id >> 1;
        const int ci = ci0 + 16 * ci_sub + (lane & 15);
#pragma unroll
        for (int v = 0; v < 4; ++v) p[(size_t)(co0 + 16 * co_sub + 4 * (lane >> 4) + v) * cin + ci] = acc[u][v];
    }
}

// gW[co][kappa][ci] = the splits of part[(kappa, s)][co][ci] added in order (restated from spconv.hip, which stays as it is)
__global__ __launch_bounds__(256) void wgrad_bf16_reduce_kernel(int K, int cin, int cout, int splits, const float *__restrict__ part,
                                                                float *__restrict__ gW) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)cout * K * cin) return;
    const int ci = (int)(t % cin), kap = (int)((t / cin) % K), co = (int)(t / ((long long)cin * K));
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += part[((size_t)(kap * splits + s) * cout + co) * cin + ci];
    gW[t] = acc;
}

int splits_of(long long n) { return (int)std::min<long long>(SPCONV_MAX_SPLITS, std::max<long long>(1, (n + SPLIT_ROWS - 1) / SPLIT_ROWS)); }

bool widths_ok(int k, int cin, int cout) {
    return k >= 1 && k <= MAX_K && cin >= 32 && cout >= 32 && cin % 32 == 0 && cout % 32 == 0 && cin <= 4096 && cout <= 4096;
}
// the workspace: the packed weight, then the weight gradient's partial sums
size_t packed_bytes(int k, int cin, int cout) { return ptv2_align256((size_t)k * cin * cout * sizeof(__bf16)); }

template <int NT>
void launch_conv(int form, dim3 grid, hipStream_t st, int n_tab, int n_other, int k, int cin, int cout, const float *in,
                 const int *tab, const __bf16 *Wp, int reverse, float *out) {
    if (form == SPCONV_GATHER)
        hipLaunchKernelGGL((conv_bf16_kernel<NT, SPCONV_GATHER>), grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, in, tab, Wp,
                           reverse, out);
    else
        hipLaunchKernelGGL((conv_bf16_kernel<NT, SPCONV_SCATTER>), grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, in, tab, Wp,
                           reverse, out);
}

}  // namespace

extern "C" int ptv2_spconv_bf16_abi_version(void) { return 1; }

extern "C" long long ptv2_spconv_bf16_workspace_bytes(long long n, int k, int cin, int cout) {
    if (n < 0 || !widths_ok(k, cin, cout)) return -1;
    return (long long)packed_bytes(k, cin, cout) + (long long)k * splits_of(n) * cin * cout * 4 + 256;
}

extern "C" int spconv_bf16_conv_hip_launcher(int form, int n_tab, int n_other, int k, int cin, int cout, const float *in,
                                             const int *tab, const float *weight, int transpose, int reverse, float *out,
                                             void *workspace, long long workspace_bytes, void *stream) {
    if ((form != SPCONV_GATHER && form != SPCONV_SCATTER) || n_tab < 0 || n_other < 0 || !widths_ok(k, cin, cout) ||
        (form == SPCONV_SCATTER && reverse))
        return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < ptv2_spconv_bf16_workspace_bytes(n_tab, k, cin, cout)) return PTV2_ERR_WORKSPACE;
    if (n_tab == 0 || n_other == 0) return PTV2_OK;
    if (!in || !tab || !weight || !out) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    __bf16 *Wp = (__bf16 *)workspace;
    hipLaunchKernelGGL(pack_weight_kernel, dim3(k, cout / 32, cin / 32), dim3(256), 0, st, k, cin, cout, weight, transpose ? 1 : 0, Wp);
    const int cin_e = transpose ? cout : cin, cout_e = transpose ? cin : cout;
    const int nt = cout_e % 96 == 0 ? 6 : cout_e % 64 == 0 ? 4 : 2;
    const dim3 grid(divup(n_tab, TM), cout_e / (16 * nt));
    if (nt == 6) launch_conv<6>(form, grid, st, n_tab, n_other, k, cin_e, cout_e, in, tab, Wp, reverse, out);
    else if (nt == 4) launch_conv<4>(form, grid, st, n_tab, n_other, k, cin_e, cout_e, in, tab, Wp, reverse, out);
    else launch_conv<2>(form, grid, st, n_tab, n_other, k, cin_e, cout_e, in, tab, Wp, reverse, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int spconv_bf16_wgrad_hip_launcher(int n_tab, int n_other, int k, int cin, int cout, const float *x, const float *g,
                                              const int *tab, int gather_g, float *gW, void *workspace,
                                              long long workspace_bytes, void *stream) {
    if (n_tab < 0 || n_other < 0 || !widths_ok(k, cin, cout) || !gW) return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < ptv2_spconv_bf16_workspace_bytes(n_tab, k, cin, cout)) return PTV2_ERR_WORKSPACE;
    if (n_tab > 0 && (!x || !g || !tab)) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int splits = splits_of(n_tab), rows = std::max(1, divup(divup(n_tab, splits), RC) * RC);
    float *part = (float *)((char *)workspace + packed_bytes(k, cin, cout));
    const int nj = cin % 96 == 0 ? 3 : cin % 64 == 0 ? 2 : 1;
    const dim3 grid(k * splits, cout / 32, cin / (32 * nj));
    if (nj == 3)
        hipLaunchKernelGGL(wgrad_bf16_kernel<3>, grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, x, g, tab, gather_g, splits, rows, part);
    else if (nj == 2)
        hipLaunchKernelGGL(wgrad_bf16_kernel<2>, grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, x, g, tab, gather_g, splits, rows, part);
    else
        hipLaunchKernelGGL(wgrad_bf16_kernel<1>, grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, x, g, tab, gather_g, splits, rows, part);
    hipLaunchKernelGGL(wgrad_bf16_reduce_kernel, dim3(divup((long long)cout * k * cin, 256)), dim3(256), 0, st, k, cin, cout, splits,
                       (const float *)part, gW);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
