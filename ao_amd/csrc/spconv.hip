// ao_amd/csrc/spconv.hip -- the sparse 3D convolutions of SpUNet-v1m1 over the tables of spconv_tables.hip
// (include/ptv2_spconv_hip.h).  A table is (rows, K) int32 with -1 holes; a weight is (Cout, K, Cin) fp32.
//
//   conv_kernel<NT, GATHER>   out[r] = sum over kappa of W[kappa] in[tab[r][kappa]]: a workgroup owns 64 table rows and one
//                             chunk of 16 NT output channels, loops over kappa, skips a kappa no row of the tile has,
//                             gathers that kappa's 64 input rows and the weight slab through LDS 32 input channels at a time
//                             and feeds v_mfma_f32_16x16x4_f32 (exact fp32); every output row is stored once
//   conv_kernel<NT, SCATTER>  out[tab[r][kappa]] = W[kappa] in[r]: the same tile, the accumulator restarts per kappa and is
//                             stored to the row the table names (every output row has one parent: plain stores)
//   stem_kernel               Cin <= 16 on the vector ALU with the whole weight in LDS (125 x 6 x 32 floats = 96 KB)
//   wgrad_kernel<NJ>          gW[kappa] partial sums per (kappa, row split) on the matrix core, wgrad_small_kernel for the
//                             stem; wgrad_reduce_kernel adds the splits in order
// The transposed forms (input gradients) read the same weight through other strides.  No atomics anywhere.
#include <algorithm>

#include "common.h"
#include "../../include/ptv2_spconv_hip.h"

namespace {

constexpr int TM = 64;          // table rows per workgroup
constexpr int KC = 32;          // input channels per LDS stage
constexpr int PITCH = KC + 4;   // row r starts in bank 36 r mod 64: 16 rows x 4 columns hit 64 distinct banks
constexpr int MAX_K = 27;       // columns of a table on the matrix-core forms
constexpr int SPLIT_ROWS = 1024;  // rows per split of the weight gradient, up to SPCONV_MAX_SPLITS splits

// W element (a: output channel of this call, kappa, b: input channel of this call) is W[a * sa + kappa * sk + b * sb]
template <int NT, int FORM>
__global__ __launch_bounds__(256) void conv_kernel(int n_tab, int n_other, int K, int cin, int cout, const float *__restrict__ in,
                                                   const int *__restrict__ tab, const float *__restrict__ W, long long sa,
                                                   long long sk, long long sb, int reverse, float *__restrict__ out) {
    constexpr int CN = NT * 16;
    __shared__ __attribute__((aligned(16))) float sX[TM * PITCH];
    __shared__ __attribute__((aligned(16))) float sW[CN * PITCH];
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
        if (FORM == SPCONV_SCATTER) {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
        }
        for (int c0 = 0; c0 < cin; c0 += KC) {
#pragma unroll
            for (int i = 0; i < TM * KC / 4 / 256; ++i) {
                const int e = tid + 256 * i, r = e >> 3, q = e & 7;
                int src;
                if (FORM == SPCONV_GATHER) src = sTab[r * K + kap];
                else src = row0 + r < n_tab ? row0 + r : -1;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (src >= 0) v = *(const float4 *)(in + (size_t)src * cin + c0 + 4 * q);
                *(float4 *)(sX + r * PITCH + 4 * q) = v;
            }
            if (sb == 1) {
                for (int e = tid; e < CN * KC / 4; e += 256) {
                    const int a = e >> 3, q = e & 7;
                    *(float4 *)(sW + a * PITCH + 4 * q) = *(const float4 *)(W + (size_t)(n0 + a) * sa + (size_t)kap * sk + c0 + 4 * q);
                }
            } else {
                for (int e = tid; e < CN * KC; e += 256) {
                    const int a = e % CN, b = e / CN;
                    sW[a * PITCH + b] = W[(size_t)(n0 + a) * sa + (size_t)kap * sk + (size_t)(c0 + b) * sb];
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KC / 4; ++kk) {
                const float xv = sX[my_row * PITCH + 4 * kk + quad];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(sW[(16 * t + (lane & 15)) * PITCH + 4 * kk + quad], xv, acc[t], 0, 0, 0);
            }
            __syncthreads();
        }
        if (FORM == SPCONV_SCATTER) {
            const int j = sTab[my_row * K + kap];
            if (j >= 0) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    *(float4 *)(out + (size_t)j * cout + n0 + 16 * t + 4 * quad) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
            }
        }
    }
    if (FORM == SPCONV_GATHER && row0 + my_row < n_tab) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            *(float4 *)(out + (size_t)(row0 + my_row) * cout + n0 + 16 * t + 4 * quad) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
}

// ---------------------------------------------------------------------------------------------------------- stem ----------
// weight (Cout, K, Cin) -> LDS [kappa][ci][co]; thread = (row of the pass, co)
__global__ __launch_bounds__(256) void stem_kernel(int n, int K, int cin, int cout, const float *__restrict__ in,
                                                   const int *__restrict__ tab, const float *__restrict__ W,
                                                   float *__restrict__ out) {
    extern __shared__ float sWt[];
    const int tid = threadIdx.x, total = K * cin * cout;
    for (int e = tid; e < total; e += 256) {
        const int co = e / (K * cin), rest = e - co * (K * cin);
        sWt[rest * cout + co] = W[e];
    }
    __syncthreads();
    const int rp = 256 / cout, co = tid % cout, rr = tid / cout;
    for (long long row = (long long)blockIdx.x * rp + rr; row < n; row += (long long)gridDim.x * rp) {
        float acc = 0.f;
        for (int kap = 0; kap < K; ++kap) {
            const int j = tab[(size_t)row * K + kap];
            if (j < 0 || j >= n) continue;
            const float *xr = in + (size_t)j * cin;
            const float *wr = sWt + (size_t)kap * cin * cout + co;
            for (int ci = 0; ci < cin; ++ci) acc = __builtin_fmaf(wr[ci * cout], xr[ci], acc);
        }
        out[(size_t)row * cout + co] = acc;
    }
}

// the stem's input gradient (needed only when the features require one): one thread per (row, ci), the table reversed
__global__ __launch_bounds__(256) void stem_bwd_kernel(int n, int K, int cin, int cout, const float *__restrict__ g,
                                                       const int *__restrict__ tab, const float *__restrict__ W,
                                                       float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * cin) return;
    const long long row = t / cin;
    const int ci = (int)(t - row * cin);
    float acc = 0.f;
    for (int kap = 0; kap < K; ++kap) {
        const int j = tab[(size_t)row * K + (K - 1 - kap)];
        if (j < 0 || j >= n) continue;
        const float *gr = g + (size_t)j * cout;
        const float *wr = W + (size_t)kap * cin + ci;
        for (int co = 0; co < cout; ++co) acc = __builtin_fmaf(wr[(size_t)co * K * cin], gr[co], acc);
    }
    out[t] = acc;
}

// ------------------------------------------------------------------------------------------------ weight gradient ----------
constexpr int RC = 32;  // rows per stage
// part[(kappa * splits + s)][co][ci]; a workgroup owns (kappa, s), 32 output and 32 NJ input channels
template <int NJ>
__global__ __launch_bounds__(256) void wgrad_kernel(int n_tab, int n_other, int K, int cin, int cout, const float *__restrict__ x,
                                                    const float *__restrict__ g, const int *__restrict__ tab, int gather_g,
                                                    int splits, int rows_per_split, float *__restrict__ part) {
    constexpr int XW = 32 * NJ, GP = 32 + 16, XP = XW + 16;  // pitches: four consecutive rows start 16 banks apart
    __shared__ __attribute__((aligned(16))) float sG[RC * GP];
    __shared__ __attribute__((aligned(16))) float sXc[RC * XP];
    __shared__ int sJ[RC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int kap = blockIdx.x / splits, s = blockIdx.x - kap * splits;
    const int co0 = blockIdx.y * 32, ci0 = blockIdx.z * XW;
    const int r_begin = s * rows_per_split, r_end = min(n_tab, r_begin + rows_per_split);
    v4f acc[NJ];
#pragma unroll
    for (int u = 0; u < NJ; ++u) acc[u] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int rb = r_begin; rb < r_end; rb += RC) {
        int j = -1;
        if (tid < RC && rb + tid < r_end) {
            j = tab[(size_t)(rb + tid) * K + kap];
            if (j >= n_other) j = -1;
        }
        if (tid < RC) sJ[tid] = j;
        if (!__syncthreads_or(j >= 0)) continue;  // no row of this stage has the column
        {
            const int r = tid >> 3, q = tid & 7, jj = sJ[r];
            const long long grow = gather_g ? jj : rb + r, xrow = gather_g ? rb + r : jj;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (jj >= 0) v = *(const float4 *)(g + (size_t)grow * cout + co0 + 4 * q);
            *(float4 *)(sG + r * GP + 4 * q) = v;
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (jj >= 0) xv = *(const float4 *)(x + (size_t)xrow * cin + ci0 + 32 * u + 4 * q);
                *(float4 *)(sXc + r * XP + 32 * u + 4 * q) = xv;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int id = w + 4 * u, co_sub = id & 1, ci_sub = id >> 1;
#pragma unroll
            for (int kk = 0; kk < RC / 4; ++kk) {
                const int r = 4 * kk + (lane >> 4);
                acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(sG[r * GP + 16 * co_sub + (lane & 15)],
                                                              sXc[r * XP + 16 * ci_sub + (lane & 15)], acc[u], 0, 0, 0);
            }
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

// Cin <= 16: one thread per (co, ci) of a (kappa, split), rows in order
__global__ void wgrad_small_kernel(int n_tab, int n_other, int K, int cin, int cout, const float *__restrict__ x,
                                   const float *__restrict__ g, const int *__restrict__ tab, int gather_g, int splits,
                                   int rows_per_split, float *__restrict__ part) {
    const int kap = blockIdx.x / splits, s = blockIdx.x - kap * splits;
    const int t = blockIdx.y * blockDim.x + threadIdx.x;
    if (t >= cout * cin) return;
    const int co = t / cin, ci = t - co * cin;
    const int r_begin = s * rows_per_split, r_end = min(n_tab, r_begin + rows_per_split);
    float acc = 0.f;
    for (int r = r_begin; r < r_end; ++r) {
        const int j = tab[(size_t)r * K + kap];
        if (j < 0 || j >= n_other) continue;
        const long long grow = gather_g ? j : r, xrow = gather_g ? r : j;
        acc = __builtin_fmaf(g[(size_t)grow * cout + co], x[(size_t)xrow * cin + ci], acc);
    }
    part[(size_t)blockIdx.x * cout * cin + t] = acc;
}

// gW[co][kappa][ci] = the splits of part[(kappa, s)][co][ci] added in order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int K, int cin, int cout, int splits, const float *__restrict__ part,
                                                           float *__restrict__ gW) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)cout * K * cin) return;
    const int ci = (int)(t % cin), kap = (int)((t / cin) % K), co = (int)(t / ((long long)cin * K));
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += part[((size_t)(kap * splits + s) * cout + co) * cin + ci];
    gW[t] = acc;
}

int splits_of(long long n) { return (int)std::min<long long>(SPCONV_MAX_SPLITS, std::max<long long>(1, (n + SPLIT_ROWS - 1) / SPLIT_ROWS)); }

template <int NT>
void launch_conv(int form, dim3 grid, hipStream_t st, int n_tab, int n_other, int k, int cin, int cout, const float *in,
                 const int *tab, const float *W, long long sa, long long sk, long long sb, int reverse, float *out) {
    if (form == SPCONV_GATHER)
        hipLaunchKernelGGL((conv_kernel<NT, SPCONV_GATHER>), grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, in, tab, W, sa, sk,
                           sb, reverse, out);
    else
        hipLaunchKernelGGL((conv_kernel<NT, SPCONV_SCATTER>), grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, in, tab, W, sa, sk,
                           sb, reverse, out);
}

}  // namespace

extern "C" long long ptv2_spconv_workspace_bytes(long long n, int k, int cin, int cout) {
    if (n < 0 || k < 1 || k > SPCONV_MAX_K || cin < 1 || cout < 1 || cin > 4096 || cout > 4096) return -1;
    return (long long)k * splits_of(n) * cin * cout * 4 + 256;
}

extern "C" int spconv_conv_hip_launcher(int form, int n_tab, int n_other, int k, int cin, int cout, const float *in,
                                        const int *tab, const float *weight, int transpose, int reverse, float *out,
                                        void *stream) {
    if ((form != SPCONV_GATHER && form != SPCONV_SCATTER) || n_tab < 0 || n_other < 0 || k < 1 || k > MAX_K || cin < 32 ||
        cout < 32 || cin % 32 || cout % 32 || (form == SPCONV_SCATTER && reverse))
        return PTV2_ERR_ARG;
    if (n_tab == 0 || n_other == 0) return PTV2_OK;
    if (!in || !tab || !weight || !out) return PTV2_ERR_ARG;
    const int cin_e = transpose ? cout : cin, cout_e = transpose ? cin : cout;
    const long long sa = transpose ? 1 : (long long)k * cin, sk = cin, sb = transpose ? (long long)k * cin : 1;
    const int nt = cout_e % 96 == 0 ? 6 : cout_e % 64 == 0 ? 4 : 2;
    const dim3 grid(divup(n_tab, TM), cout_e / (16 * nt));
    hipStream_t st = (hipStream_t)stream;
    if (nt == 6) launch_conv<6>(form, grid, st, n_tab, n_other, k, cin_e, cout_e, in, tab, weight, sa, sk, sb, reverse, out);
    else if (nt == 4) launch_conv<4>(form, grid, st, n_tab, n_other, k, cin_e, cout_e, in, tab, weight, sa, sk, sb, reverse, out);
    else launch_conv<2>(form, grid, st, n_tab, n_other, k, cin_e, cout_e, in, tab, weight, sa, sk, sb, reverse, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int spconv_wgrad_hip_launcher(int n_tab, int n_other, int k, int cin, int cout, const float *x, const float *g,
                                         const int *tab, int gather_g, float *gW, void *workspace, long long workspace_bytes,
                                         void *stream) {
    const bool small = cin <= 16;
    if (n_tab < 0 || n_other < 0 || k < 1 || k > SPCONV_MAX_K || cin < 1 || cout < 32 || cout % 32 || cout > 4096 ||
        (!small && (cin % 32 || cin > 4096)) || !gW)
        return PTV2_ERR_ARG;
    const long long need = ptv2_spconv_workspace_bytes(n_tab, k, cin, cout);
    if (!workspace || workspace_bytes < need) return PTV2_ERR_WORKSPACE;
    if (n_tab > 0 && (!x || !g || !tab)) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int splits = splits_of(n_tab), rows = std::max(1, divup(divup(n_tab, splits), RC) * RC);
    float *part = (float *)workspace;
    if (small) {
        const int threads = std::min(256, divup(cout * cin, 64) * 64);
        hipLaunchKernelGGL(wgrad_small_kernel, dim3(k * splits, divup(cout * cin, threads)), dim3(threads), 0, st, n_tab, n_other, k,
                           cin, cout, x, g, tab, gather_g, splits, rows, part);
    } else {
        const int nj = cin % 96 == 0 ? 3 : cin % 64 == 0 ? 2 : 1;
        const dim3 grid(k * splits, cout / 32, cin / (32 * nj));
        if (nj == 3)
            hipLaunchKernelGGL(wgrad_kernel<3>, grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, x, g, tab, gather_g, splits, rows, part);
        else if (nj == 2)
            hipLaunchKernelGGL(wgrad_kernel<2>, grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, x, g, tab, gather_g, splits, rows, part);
        else
            hipLaunchKernelGGL(wgrad_kernel<1>, grid, dim3(256), 0, st, n_tab, n_other, k, cin, cout, x, g, tab, gather_g, splits, rows, part);
    }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(divup((long long)cout * k * cin, 256)), dim3(256), 0, st, k, cin, cout, splits,
                       (const float *)part, gW);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int spconv_stem_hip_launcher(int n, int k, int cin, int cout, const float *in, const int *tab, const float *weight,
                                        int transpose, float *out, void *stream) {
    const long long lds = (long long)k * cin * cout * 4;
    if (n < 0 || k < 1 || k > SPCONV_MAX_K || cin < 1 || cin > 16 || (cout != 32 && cout != 64) || lds > 147456) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!in || !tab || !weight || !out) return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (transpose) {
        hipLaunchKernelGGL(stem_bwd_kernel, dim3(divup((long long)n * cin, 256)), dim3(256), 0, st, n, k, cin, cout, in, tab, weight, out);
    } else {
        RUN(ptv2_kernel_lds((const void *)stem_kernel, 147456));  // (more dynamic LDS than the default 64 KB)
        const int rp = 256 / cout;
        hipLaunchKernelGGL(stem_kernel, dim3(std::min(divup(n, rp * 8), 1024)), dim3(256), (size_t)lds, st, n, k, cin, cout, in, tab,
                           weight, out);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
