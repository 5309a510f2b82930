// ao_amd/csrc/oct_conv.hip -- OctFormer's dense octree convolutions (the stem, Downsample, the decoder) on the fp32 matrix cores,
// and the tables between two neighbouring octree depths (include/ptv2_octconv_hip.h).  gfx950 only.
//
// One gather-GEMM, out[i] = bias + sum_s x[tab[i, s]] W[s], is the forward and the input gradient of the k = 3 stride 1
// convolution, of the k = 2 stride 2 convolution and of the k = 3 stride 2 deconvolution (the header's table).
//   oct_conv_kernel<NT>   a workgroup of four wavefronts owns 64 consecutive output rows (spatial neighbours in Morton order:
//       their gathered rows overlap in L2) and 16 NT output columns; wavefront w owns rows 16 w .. 16 w + 15 and keeps NT
//       accumulator tiles of V_MFMA_F32_16X16X4_F32 (mfma4: a lane gives A[m = lane & 15][k = lane >> 4] and
//       B[k = lane >> 4][n = lane & 15] and holds D[m = 4 (lane >> 4) + i][n = lane & 15]) in registers over all slots.  The
//       64 x slots table tile is read once into LDS; every wavefront ballots its 16 entries of every slot into a bit mask.  A
//       slot no wavefront needs is not staged at all; a wavefront skips the products of a slot none of its rows has.  Per slot
//       and per chunk of 32 contraction channels the workgroup stages the 64 gathered rows (float4, zeros for -1; pitch 36 = 4
//       mod 16) and the 32 x 16 NT block of W[s] (pitch = 16 mod 64): 34.5 KB of LDS whatever Cin and Cout are.  out is written
//       once, bias added in the epilogue.  No (n, slots, C) buffer, no atomics.
//   oct_conv_gw_kernel    g_w[s] = sum_i x[tab[i, s]]^T g[i]: a workgroup per (64 x 128 block of W[s], slot, row split), the
//       contraction over rows on the same instruction in stages of 32 rows (a stage without a valid entry is skipped).  At most
//       OCTCONV_MAX_SPLITS partials, added ascending by oct_conv_gw_finalize_kernel; one split writes g_w itself.
//   oct_conv_gb_kernel    the bias gradient: fixed-order column sums over 64 row strips, added ascending by a finalize.
#include "common.h"
#include "../../include/ptv2_octconv_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int ROWS = 64;        // output rows of a workgroup
constexpr int KC = 32;          // contraction channels per stage
constexpr int XP = KC + 4;      // pitch of the gathered rows: l15 * XP + quad touches 64 banks
constexpr int MAXS = 27;
constexpr int GR = 32;          // weight gradient: rows per stage
constexpr int GCI = 64, GCO = 128;   // ... its block of W[s]
constexpr int GXP = GCI + 16, GGP = GCO + 16;   // = 16 mod 64: quad * pitch + l15 touches 64 banks
constexpr int SPLIT_ROWS = 1024;
constexpr int GB_STRIPS = 64;   // bias gradient: row strips, one partial each
__host__ __device__ constexpr int wpitch(int nt) { return nt <= 4 ? 80 : 144; }   // >= 16 nt, = 16 mod 64

struct ConvOp {
    int n_out, n_in, S, cin, cout, transpose, reverse;   // cin: the contraction of THIS launch, cout: its output columns
    const int *tab;
    const float *x, *w, *bias;
    float *out;
};

struct GwOp {
    int n_out, n_in, S, cin, cout, transpose, rows_per_split;
    const int *tab;
    const float *x, *g;
    float *dst;
    size_t split_stride;
};

// columns c .. c + 3 of a row of `width` floats; columns >= width read 0.  vec: width % 4 == 0 (the row is 16-byte aligned)
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int c, int width, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) {
        if (c < width) v = *(const float4 *)(row + c);
    } else {
        if (c < width) v.x = row[c];
        if (c + 1 < width) v.y = row[c + 1];
        if (c + 2 < width) v.z = row[c + 2];
        if (c + 3 < width) v.w = row[c + 3];
    }
    return v;
}

template <int NT>
__global__ __launch_bounds__(TPB) void oct_conv_kernel(ConvOp a) {
    constexpr int WP = wpitch(NT);
    __shared__ int tabs[ROWS * MAXS];
    __shared__ unsigned wmask[TPB / WAVE];
    __shared__ __attribute__((aligned(16))) float xs[ROWS * XP];
    __shared__ __attribute__((aligned(16))) float ws[KC * WP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, quad = lane >> 4;
    const long long row0 = (long long)blockIdx.x * ROWS;
    const int col0 = blockIdx.y * 16 * NT, S = a.S;
    const int nt = min(NT, (a.cout - col0 + 15) / 16);

    for (int e = tid; e < ROWS * S; e += TPB) {
        const long long r = row0 + e / S;
        const int s = e % S;
        int j = -1;
        if (r < a.n_out) {
            j = a.tab[r * S + (a.reverse ? S - 1 - s : s)];
            if ((unsigned)j >= (unsigned)a.n_in) j = -1;
        }
        tabs[e] = j;
    }
    __syncthreads();
    unsigned mine = 0;   // the slots one of this wavefront's 16 rows has
    for (int s = 0; s < S; ++s)
        if (__ballot(lane < 16 && tabs[(16 * wave + lane) * S + s] >= 0)) mine |= 1u << s;
    if (lane == 0) wmask[wave] = mine;
    __syncthreads();
    const unsigned any = wmask[0] | wmask[1] | wmask[2] | wmask[3];

    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    const int cin4 = (a.cin + 3) & ~3;
    const bool xvec = (a.cin & 3) == 0, wvec = (a.cout & 3) == 0;
    for (int s = 0; s < S; ++s) {
        if (!(any >> s & 1)) continue;
        const float *wsl = a.w + (size_t)s * a.cin * a.cout;
        for (int k0 = 0; k0 < cin4; k0 += KC) {
            const int kn = min(KC, cin4 - k0);   // a multiple of 4
            __syncthreads();   // the previous stage has been read
            {
                const int r = tid >> 2, j = tabs[r * S + s];
                const float *row = a.x + (size_t)max(j, 0) * a.cin;
                for (int q = tid & 3; q < kn / 4; q += 4) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (j >= 0) v = load4(row, k0 + 4 * q, a.cin, xvec);
                    *(float4 *)(xs + r * XP + 4 * q) = v;
                }
            }
            if (!a.transpose) {   // W[s] is (cin, cout)
                const int nq = 4 * nt;
                for (int e = tid; e < kn * nq; e += TPB) {
                    const int ci = e / nq, q = e % nq;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k0 + ci < a.cin) v = load4(wsl + (size_t)(k0 + ci) * a.cout, col0 + 4 * q, a.cout, wvec);
                    *(float4 *)(ws + ci * WP + 4 * q) = v;
                }
            } else {              // W[s] is (cout, cin): lanes run along cin
                for (int e = tid; e < kn * 16 * nt; e += TPB) {
                    const int ci = e % kn, cl = e / kn, co = col0 + cl;
                    ws[ci * WP + cl] = (k0 + ci < a.cin && co < a.cout) ? wsl[(size_t)co * a.cin + k0 + ci] : 0.f;
                }
            }
            __syncthreads();
            if (mine >> s & 1) {
                const float *ap = xs + (16 * wave + l15) * XP + quad, *bp = ws + quad * WP + l15;
                for (int kk = 0; kk < kn; kk += 4) {
                    const float av = ap[kk];
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t < nt) acc[t] = mfma4(av, bp[kk * WP + 16 * t], acc[t]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = col0 + 16 * t + l15;
        if (t >= nt || col >= a.cout) continue;
        const float b = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = row0 + 16 * wave + 4 * quad + i;
            if (r < a.n_out) a.out[r * a.cout + col] = acc[t][i] + b;
        }
    }
}

// grid (blocks of W[s], slots, splits)
__global__ __launch_bounds__(TPB) void oct_conv_gw_kernel(GwOp a) {
    __shared__ int js[GR];
    __shared__ __attribute__((aligned(16))) float xs[GR * GXP];
    __shared__ __attribute__((aligned(16))) float gs[GR * GGP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, quad = lane >> 4;
    const int cbn = (a.cout + GCO - 1) / GCO;
    const int ci0 = (int)(blockIdx.x / cbn) * GCI, co0 = (int)(blockIdx.x % cbn) * GCO;
    const int s = blockIdx.y, sp = blockIdx.z, S = a.S;
    const int nt = min(GCO / 16, (a.cout - co0 + 15) / 16);
    const bool wave_on = ci0 + 16 * wave < a.cin;
    const bool xvec = (a.cin & 3) == 0, gvec = (a.cout & 3) == 0;
    const long long r_lo = (long long)sp * a.rows_per_split, r_hi = min((long long)a.n_out, r_lo + a.rows_per_split);

    v4f acc[GCO / 16];
#pragma unroll
    for (int t = 0; t < GCO / 16; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (long long r0 = r_lo; r0 < r_hi; r0 += GR) {
        int j = -1;
        if (tid < GR && r0 + tid < r_hi) {
            j = a.tab[(r0 + tid) * S + s];
            if ((unsigned)j >= (unsigned)a.n_in) j = -1;
        }
        if (tid < GR) js[tid] = j;   // (read only between the two barriers below: every wavefront is past that part)
        if (!__syncthreads_or(j >= 0)) continue;
        for (int e = tid; e < GR * (GCI / 4); e += TPB) {
            const int r = e / (GCI / 4), q = e % (GCI / 4), jj = js[r];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (jj >= 0) v = load4(a.x + (size_t)jj * a.cin, ci0 + 4 * q, a.cin, xvec);
            *(float4 *)(xs + r * GXP + 4 * q) = v;
        }
        for (int e = tid; e < GR * (GCO / 4); e += TPB) {
            const int r = e / (GCO / 4), q = e % (GCO / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (js[r] >= 0) v = load4(a.g + (size_t)(r0 + r) * a.cout, co0 + 4 * q, a.cout, gvec);
            *(float4 *)(gs + r * GGP + 4 * q) = v;
        }
        __syncthreads();
        if (wave_on) {
            const float *ap = xs + quad * GXP + 16 * wave + l15, *bp = gs + quad * GGP + l15;
#pragma unroll
            for (int kk = 0; kk < GR; kk += 4) {
                const float av = ap[kk * GXP];
#pragma unroll
                for (int t = 0; t < GCO / 16; ++t)
                    if (t < nt) acc[t] = mfma4(av, bp[kk * GGP + 16 * t], acc[t]);
            }
        }
    }
    if (!wave_on) return;
    float *dst = a.dst + (size_t)sp * a.split_stride + (size_t)s * a.cin * a.cout;
#pragma unroll
    for (int t = 0; t < GCO / 16; ++t) {
        const int co = co0 + 16 * t + l15;
        if (t >= nt || co >= a.cout) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ci = ci0 + 16 * wave + 4 * quad + i;
            if (ci < a.cin) dst[a.transpose ? (size_t)co * a.cin + ci : (size_t)ci * a.cout + co] = acc[t][i];
        }
    }
}

__global__ __launch_bounds__(TPB) void oct_conv_gw_finalize_kernel(int splits, long long elems, const float *__restrict__ partial,
                                                                   float *__restrict__ g_w) {
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    if (e >= elems) return;
    float s = 0.f;
    for (int b = 0; b < splits; ++b) s += partial[(size_t)b * elems + e];
    g_w[e] = s;
}

// g_b[c] = sum_i g[i, c] in two fixed-order steps: workgroup (x, y) adds the rows of strip y for 64 columns (four row classes
// i mod 4 ascending, then the classes ascending) into partial[y][c]; oct_conv_gb_finalize_kernel adds the GB_STRIPS strips ascending
__global__ __launch_bounds__(TPB) void oct_conv_gb_kernel(int n, int c, int rows_per_strip, const float *__restrict__ g,
                                                          float *__restrict__ partial) {
    __shared__ float red[TPB];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), cls = threadIdx.x >> 6;
    const long long lo = (long long)blockIdx.y * rows_per_strip, hi = min((long long)n, lo + rows_per_strip);
    float s = 0.f;
    if (col < c)
        for (long long r = lo + cls; r < hi; r += 4) s += g[r * c + col];
    red[threadIdx.x] = s;
    __syncthreads();
    if (cls == 0 && col < c)
        partial[(size_t)blockIdx.y * c + col] = ((red[threadIdx.x] + red[threadIdx.x + 64]) + red[threadIdx.x + 128]) + red[threadIdx.x + 192];
}

__global__ __launch_bounds__(TPB) void oct_conv_gb_finalize_kernel(int c, const float *__restrict__ partial, float *__restrict__ g_b) {
    const int col = blockIdx.x * TPB + threadIdx.x;
    if (col >= c) return;
    float s = 0.f;
    for (int y = 0; y < GB_STRIPS; ++y) s += partial[(size_t)y * c + col];
    g_b[col] = s;
}

// ------------------------------------------------------------------------------------------------------------ tables
// one thread per parent walks its consecutive children
__global__ __launch_bounds__(TPB) void oct_conv_link_kernel(octconv_tables a) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= a.n_parent) return;
    for (int o = 0; o < 8; ++o) a.child[8 * (size_t)p + o] = -1;
    const int lo = max(a.first[p], 0), hi = min(a.first[p + 1], a.n);
    for (int j = lo; j < hi; ++j) {
        const int o = (int)(a.keys[j] & 7);
        a.child[8 * (size_t)p + o] = j;
        a.parent[j] = p;
        for (int q = 0; q < 8; ++q) a.onehot[8 * (size_t)j + q] = q == o ? p : -1;
    }
}

__device__ __forceinline__ int slot_of(int x, int y, int z) { return (x + 1) * 9 + (y + 1) * 3 + (z + 1); }

// up[j, k]: q = (c - d) / 2 where integral.  Per axis with P = c >> 1: c even admits d = 0 (q = P); c odd admits d = +1 (q = P)
// and d = -1 (q = P + 1)
__global__ __launch_bounds__(TPB) void oct_conv_up_kernel(octconv_tables a) {
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    if (t >= (long long)MAXS * a.n) return;
    const int j = (int)(t / MAXS), k = (int)(t % MAXS);
    const int d[3] = {k / 9 - 1, k / 3 % 3 - 1, k % 3 - 1};
    int off[3];
    bool ok = true;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int odd = a.xyz[3 * (size_t)j + ax] & 1;
        ok = ok && (odd ? d[ax] != 0 : d[ax] == 0);
        off[ax] = (odd && d[ax] == -1) ? 1 : 0;
    }
    int found = -1;
    const int p = a.parent[j];
    if (ok && (unsigned)p < (unsigned)a.n_parent) found = a.parent_nbr[(size_t)p * MAXS + slot_of(off[0], off[1], off[2])];
    a.up[t] = found;
}

// down3[p, k]: the child at 2 p + d.  Per axis: d = -1 is octant bit 1 of the neighbour at -1, d = 0 bit 0 of p, d = +1 bit 1 of p
__global__ __launch_bounds__(TPB) void oct_conv_down3_kernel(octconv_tables a) {
    const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
    if (t >= (long long)MAXS * a.n_parent) return;
    const int p = (int)(t / MAXS), k = (int)(t % MAXS);
    const int dx = k / 9 - 1, dy = k / 3 % 3 - 1, dz = k % 3 - 1;
    const int q = a.parent_nbr[(size_t)p * MAXS + slot_of(dx < 0 ? -1 : 0, dy < 0 ? -1 : 0, dz < 0 ? -1 : 0)];
    const int o = 4 * (dx != 0) + 2 * (dy != 0) + (dz != 0);
    a.down3[t] = (unsigned)q < (unsigned)a.n_parent ? a.child[8 * (size_t)q + o] : -1;
}

// -------------------------------------------------------------------------------------------------------------- host
bool contraction_ok(int c) { return (c >= 1 && c <= OCTCONV_STEM_CHANNELS) || (c >= 4 && c % 4 == 0 && c <= OCTCONV_MAX_CHANNELS); }
bool output_ok(int c) { return c >= 8 && c % 8 == 0 && c <= OCTCONV_MAX_CHANNELS; }
// the LAYER's pair
bool pair_ok(const octconv_args &a) {
    return a.n_out >= 1 && a.n_in >= 1 && (a.slots == 8 || a.slots == MAXS) && contraction_ok(a.cin) && output_ok(a.cout);
}
int splits_of(int n_out) { return (int)min((long long)OCTCONV_MAX_SPLITS, (long long)divup(n_out, SPLIT_ROWS)); }

// the weight gradient's partials (none when one split writes g_w itself); the bias gradient's strips follow them
size_t gw_partial_bytes(int n_out, int slots, int cin, int cout) {
    const int splits = splits_of(n_out);
    return splits == 1 ? 0 : ptv2_align256(sizeof(float) * (size_t)splits * slots * cin * cout);
}

template <int NT>
int launch_conv(const ConvOp &op, hipStream_t st) {
    hipLaunchKernelGGL(oct_conv_kernel<NT>, dim3(divup(op.n_out, ROWS), divup(divup(op.cout, 16), NT)), dim3(TPB), 0, st, op);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// cin, cout of the launch (an input gradient has them exchanged)
int conv(const octconv_args &a, int cin, int cout, hipStream_t st) {
    const ConvOp op = {a.n_out, a.n_in, a.slots, cin, cout, a.transpose ? 1 : 0, a.reverse ? 1 : 0, a.tab, a.x, a.w, a.bias, a.out};
    const int tiles = divup(cout, 16), per = divup(tiles, divup(tiles, 8));   // column blocks of at most 8 tiles, evenly
    if (per <= 2) return launch_conv<2>(op, st);
    if (per <= 4) return launch_conv<4>(op, st);
    if (per <= 6) return launch_conv<6>(op, st);
    return launch_conv<8>(op, st);
}

}  // namespace

extern "C" int ptv2_octconv_abi_version(void) { return 1; }
extern "C" int ptv2_octconv_struct_bytes(int which) {
    return which == 0 ? (int)sizeof(octconv_args) : which == 1 ? (int)sizeof(octconv_tables) : -1;
}

extern "C" long long ptv2_octconv_workspace_bytes(int n_out, int slots, int cin, int cout) {
    if (n_out < 1 || (slots != 8 && slots != MAXS) || !contraction_ok(cin) || !output_ok(cout)) return -1;
    return (long long)(gw_partial_bytes(n_out, slots, cin, cout) + ptv2_align256(sizeof(float) * GB_STRIPS * (size_t)cout));
}

extern "C" int oct_conv_tables_hip_launcher(const octconv_tables *args, void *stream) {
    if (!args) return PTV2_ERR_ARG;
    const octconv_tables &a = *args;
    if (a.n < 1 || a.n > (1 << 26) || a.n_parent < 1 || a.n_parent > a.n || !a.keys || !a.xyz || !a.first || !a.parent_nbr ||
        !a.parent || !a.child || !a.onehot || !a.up || !a.down3)
        return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(oct_conv_link_kernel, dim3(divup(a.n_parent, TPB)), dim3(TPB), 0, st, a);
    PTV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(oct_conv_up_kernel, dim3(divup((long long)MAXS * a.n, TPB)), dim3(TPB), 0, st, a);
    PTV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(oct_conv_down3_kernel, dim3(divup((long long)MAXS * a.n_parent, TPB)), dim3(TPB), 0, st, a);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int oct_conv_fwd_hip_launcher(const octconv_args *args, void *stream) {
    if (!args || !pair_ok(*args) || !args->tab || !args->x || !args->w || !args->out) return PTV2_ERR_ARG;
    return conv(*args, args->cin, args->cout, (hipStream_t)stream);
}

extern "C" int oct_conv_gx_hip_launcher(const octconv_args *args, void *stream) {
    if (!args || !pair_ok(*args) || !args->tab || !args->x || !args->w || !args->out || args->bias) return PTV2_ERR_ARG;
    return conv(*args, args->cout, args->cin, (hipStream_t)stream);
}

extern "C" int oct_conv_gw_hip_launcher(const octconv_args *args, void *stream) {
    if (!args || !pair_ok(*args) || !args->tab || !args->x || !args->g || !args->g_w || !args->workspace) return PTV2_ERR_ARG;
    const octconv_args &a = *args;
    if (a.workspace_bytes < ptv2_octconv_workspace_bytes(a.n_out, a.slots, a.cin, a.cout)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int splits = splits_of(a.n_out);
    const long long elems = (long long)a.slots * a.cin * a.cout;
    const int rows_per_split = divup(divup(a.n_out, splits), GR) * GR;
    const GwOp op = {a.n_out, a.n_in, a.slots, a.cin, a.cout, a.transpose ? 1 : 0, rows_per_split, a.tab, a.x, a.g,
                     splits == 1 ? a.g_w : (float *)a.workspace, (size_t)elems};
    hipLaunchKernelGGL(oct_conv_gw_kernel, dim3(divup(a.cin, GCI) * divup(a.cout, GCO), a.slots, splits), dim3(TPB), 0, st, op);
    PTV2_CHECK_LAUNCH();
    return oct_conv_gw_finish(a.n_out, a.slots, a.cin, a.cout, a.g, a.g_w, a.g_b, a.workspace, stream);
}

int oct_conv_gw_splits(int n_out) { return splits_of(n_out); }

// what follows the partials of either operand form (internal.h): the splits of g_w added ascending, then the bias gradient
int oct_conv_gw_finish(int n_out, int slots, int cin, int cout, const float *g, float *g_w, float *g_b, void *workspace, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const int splits = splits_of(n_out);
    const long long elems = (long long)slots * cin * cout;
    if (splits > 1) {
        hipLaunchKernelGGL(oct_conv_gw_finalize_kernel, dim3(divup(elems, TPB)), dim3(TPB), 0, st, splits, elems,
                           (const float *)workspace, g_w);
        PTV2_CHECK_LAUNCH();
    }
    if (g_b) {
        float *strips = (float *)((char *)workspace + gw_partial_bytes(n_out, slots, cin, cout));
        hipLaunchKernelGGL(oct_conv_gb_kernel, dim3(divup(cout, 64), GB_STRIPS), dim3(TPB), 0, st, n_out, cout,
                           divup(divup(n_out, GB_STRIPS), 4) * 4, g, strips);
        PTV2_CHECK_LAUNCH();
        hipLaunchKernelGGL(oct_conv_gb_finalize_kernel, dim3(divup(cout, TPB)), dim3(TPB), 0, st, cout, (const float *)strips, g_b);
        PTV2_CHECK_LAUNCH();
    }
    return PTV2_OK;
}
