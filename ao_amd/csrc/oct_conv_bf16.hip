// ao_amd/csrc/oct_conv_bf16.hip -- OctFormer's dense octree convolutions with bf16 matrix-core operands
// (include/ptv2_octconv_bf16_hip.h): the one form of oct_conv.hip, out[i] = bias + sum_s x[tab[i, s]] W[s],
// on V_MFMA_F32_16X16X32_BF16.  Operands are fp32 in memory and are rounded (nearest even) once, while they are written to LDS;
// accumulation, bias and outputs are fp32.  gfx950 only.
//
// The instruction (mfma32 below): a lane gives A[m = lane & 15][k = 8 q .. 8 q + 7] and B[k = 8 q .. 8 q + 7][n = lane & 15],
// q = lane >> 4, as one 16-byte register group each, and holds D[m = 4 q + i][n = lane & 15].  Both LDS images of every kernel
// here are therefore [m or n][k] with k contiguous and PITCH = 72 bf16 (144 bytes) per row: a lane reads 16 bytes at
// 144 (lane & 15) + 16 q (+ 64 for the second 32 of a stage), 144 = 16 * 9 with 9 odd, so the 16 rows of one q fall on the 16
// distinct 16-byte slots of the 64 banks and neither operand read conflicts, whether W was stored plain or transposed: the
// transposition happens in the WRITE of the image, never in the read.
//
//   oct_conv_bf16_kernel<NT>  a workgroup of four wavefronts owns 64 consecutive output rows and 16 NT output columns.  A = W
//       (m: the output column), B = the gathered rows (n: the output row), so a lane ends with four consecutive columns of one
//       row: one float4 store.  Wavefront w owns row tiles 2 (w & 1), 2 (w & 1) + 1 and column tiles (w >> 1) NT / 2 ..: two
//       row fragments and NT / 2 column fragments feed NT instructions (one row tile per wavefront would read 1 + NT).  A stage is
//       one slot and 64 contraction channels (two instructions deep; the tail of a width that is no multiple of 64 is written as
//       zeros, global memory is never read past a row, and a last stage of at most 32 issues one instruction).  Two LDS buffers:
//       the next stage's global loads are issued into registers, the current stage is multiplied, the registers are rounded
//       and written to the other buffer, one barrier.  A slot no row of the workgroup has is never staged; a row tile whose 16
//       rows lack the slot issues nothing; a missing row inside a tile is a row of zeros.
//       W plain, (cin, cout): a lane loads columns 4 q .. 4 q + 3 of rows k = 2 p, 2 p + 1 (p = lane & 15) and writes four
//       32-bit words (one per column, two k each) at word 36 (4 q + c) + p: bank 16 q + p + const, the 64 lanes on 64 banks.
//       W transposed, (cout, cin): eight consecutive k of a column are one 16-byte write, as the gathered rows.
//   oct_conv_bf16_gw_kernel   g_w[s] = sum_i x[tab[i, s]]^T g[i]: the contraction runs over ROWS, so both images are written
//       transposed, [channel][row], by the word writes above (conflict-free), 64 rows per stage = two blocks of 32, the tail
//       and the rows without the slot as zeros; a stage with no valid row is skipped.  A workgroup per (96 x 96 block of W[s],
//       slot, row split): 6 x 6 tiles, 3 x 3 per wavefront (6 fragment reads for 9 instructions).  The operand that is
//       contiguous in g_w is A (g for a (cin, cout) weight, x for a deconvolution's (cout, cin)): float4 stores in both.
//       Splits, the fixed-order finalize and the bias gradient (fp32 column sums of g: no operand form) are oct_conv.hip's.
#include "common.h"
#include "../../include/ptv2_octconv_hip.h"
#include "../../include/ptv2_octconv_bf16_hip.h"

static_assert(sizeof(octconv_bf16_args) == sizeof(octconv_args), "octconv_bf16_args restates octconv_args");

namespace {

constexpr int TPB = 256;
constexpr int ROWS = 64;        // output rows of a workgroup
constexpr int KC = 64;          // contraction indices of a stage: two matrix instructions
constexpr int PITCH = KC + 8;   // bf16 per image row
constexpr int WP = PITCH / 2;   // ... in 32-bit words
constexpr int MAXS = 27;
constexpr int GB = 96;          // weight gradient: edge of its block of W[s]
static_assert((PITCH * 2) % 256 == 144 && PITCH % 8 == 0, "16-byte reads: aligned, rows of one q on distinct slots");

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct ConvOp {
    int n_out, n_in, S, cin, cout, transpose, reverse;   // cin: the contraction of THIS launch, cout: its output columns
    const int *tab;
    const float *x, *w, *bias;
    float *out;
};

struct GwOp {
    int n_out, n_in, S, cm, cn, x_is_m, rows_per_split;   // dst[s] is (cn, cm) row-major: m the contiguous side
    const int *tab;
    const float *x, *g;
    float *dst;
    size_t split_stride;
};

__device__ __forceinline__ v4f mfma32(ptv2_bf16x8 a, ptv2_bf16x8 b, v4f c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// rows a, b (consecutive contraction indices) of four consecutive channels -> one word per channel at img[channel][pair]
__device__ __forceinline__ void put_pairs(bf16x2 *d, float4 a, float4 b) {
    d[0] = bf16x2{(__bf16)a.x, (__bf16)b.x};
    d[WP] = bf16x2{(__bf16)a.y, (__bf16)b.y};
    d[2 * WP] = bf16x2{(__bf16)a.z, (__bf16)b.z};
    d[3 * WP] = bf16x2{(__bf16)a.w, (__bf16)b.w};
}

// the first slot above s that `any` has, or 32
__device__ __forceinline__ int next_slot(unsigned any, int s) {
    const unsigned rest = s >= 31 ? 0u : any >> (s + 1);
    return rest ? s + 1 + __builtin_ctz(rest) : 32;
}

template <int NT>
__global__ __launch_bounds__(TPB) void oct_conv_bf16_kernel(ConvOp a) {
    constexpr int HT = NT / 2;   // column tiles of a wavefront
    static_assert(NT % 2 == 0 && NT <= 8, "two buffers of 64 + 16 NT image rows and the table tile fit 64 KB");
    __shared__ int tabs[ROWS * MAXS];
    __shared__ unsigned tmask[ROWS / 16];
    __shared__ __attribute__((aligned(16))) __bf16 xs[2][ROWS * PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 ws[2][16 * NT * PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, quad = lane >> 4;
    const long long row0 = (long long)blockIdx.x * ROWS;
    const int col0 = blockIdx.y * 16 * NT, S = a.S;
    const int nt = min(NT, (a.cout - col0 + 15) / 16);
    const int rt0 = 2 * (wave & 1), ct0 = (wave >> 1) * HT;

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
    {
        unsigned m = 0;   // the slots one of the 16 rows of row tile `wave` has
        for (int s = 0; s < S; ++s)
            if (__ballot(lane < 16 && tabs[(16 * wave + lane) * S + s] >= 0)) m |= 1u << s;
        if (lane == 0) tmask[wave] = m;
    }
    __syncthreads();
    const unsigned mine[2] = {tmask[rt0], tmask[rt0 + 1]};
    const unsigned any = tmask[0] | tmask[1] | tmask[2] | tmask[3];

    v4f acc[2][HT];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int t = 0; t < HT; ++t) acc[r][t] = (v4f){0.f, 0.f, 0.f, 0.f};

    float4 xr[4], wr[NT];   // the next stage on its way from global memory to LDS
    // global loads of stage (s, k0); everything outside the row, the width or the table reads as zero
    auto load = [&](int s, int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + TPB * i, r = e >> 3, k = k0 + 8 * (e & 7), j = tabs[r * S + s];
            const float *row = a.x + (size_t)max(j, 0) * a.cin + k;
            xr[2 * i] = (j >= 0 && k < a.cin) ? *(const float4 *)row : zero4();
            xr[2 * i + 1] = (j >= 0 && k + 4 < a.cin) ? *(const float4 *)(row + 4) : zero4();
        }
        const float *wsl = a.w + (size_t)s * a.cin * a.cout;
        if (a.transpose) {   // W[s] is (cout, cin): k is contiguous
#pragma unroll
            for (int i = 0; i < HT; ++i) {
                const int e = tid + TPB * i, col = col0 + (e >> 3), k = k0 + 8 * (e & 7);
                const float *p = wsl + (size_t)min(col, a.cout - 1) * a.cin + k;
                wr[2 * i] = (col < a.cout && k < a.cin) ? *(const float4 *)p : zero4();
                wr[2 * i + 1] = (col < a.cout && k + 4 < a.cin) ? *(const float4 *)(p + 4) : zero4();
            }
        } else {             // W[s] is (cin, cout): rows k, k + 1 of four columns
#pragma unroll
            for (int i = 0; i < HT; ++i) {
                const int u = wave + 4 * i, k = k0 + 32 * (u & 1) + 2 * l15, col = col0 + 16 * (u >> 1) + 4 * quad;
                const float *p = wsl + (size_t)min(k, a.cin - 1) * a.cout + min(col, a.cout - 4);
                wr[2 * i] = (col < a.cout && k < a.cin) ? *(const float4 *)p : zero4();
                wr[2 * i + 1] = (col < a.cout && k + 1 < a.cin) ? *(const float4 *)(p + a.cout) : zero4();
            }
        }
    };
    auto store = [&](int b) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + TPB * i;
            *(ptv2_bf16x8 *)(xs[b] + (e >> 3) * PITCH + 8 * (e & 7)) = ptv2_pack_bf16(xr[2 * i], xr[2 * i + 1]);
        }
        if (a.transpose) {
#pragma unroll
            for (int i = 0; i < HT; ++i) {
                const int e = tid + TPB * i;
                *(ptv2_bf16x8 *)(ws[b] + (e >> 3) * PITCH + 8 * (e & 7)) = ptv2_pack_bf16(wr[2 * i], wr[2 * i + 1]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < HT; ++i) {
                const int u = wave + 4 * i;
                put_pairs((bf16x2 *)ws[b] + (16 * (u >> 1) + 4 * quad) * WP + 16 * (u & 1) + l15, wr[2 * i], wr[2 * i + 1]);
            }
        }
    };

    if (any) {
        int s = next_slot(any, -1), k0 = 0, b = 0;
        load(s, k0);
        store(0);
        __syncthreads();
        for (;;) {
            int ns = s, nk = k0 + KC;
            if (nk >= a.cin) nk = 0, ns = next_slot(any, s);
            const bool more = ns < S;
            if (more) load(ns, nk);
            if ((mine[0] | mine[1]) >> s & 1) {
                const int deep = a.cin - k0 > 32 ? 2 : 1;
                for (int kk = 0; kk < deep; ++kk) {
                    ptv2_bf16x8 wv[HT];
#pragma unroll
                    for (int t = 0; t < HT; ++t)
                        wv[t] = *(const ptv2_bf16x8 *)(ws[b] + (16 * (ct0 + t) + l15) * PITCH + 32 * kk + 8 * quad);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        if (!(mine[r] >> s & 1)) continue;
                        const ptv2_bf16x8 xv = *(const ptv2_bf16x8 *)(xs[b] + (16 * (rt0 + r) + l15) * PITCH + 32 * kk + 8 * quad);
#pragma unroll
                        for (int t = 0; t < HT; ++t)
                            if (ct0 + t < nt) acc[r][t] = mfma32(wv[t], xv, acc[r][t]);
                    }
                }
            }
            if (!more) break;
            store(b ^ 1);   // (read last before the previous barrier)
            __syncthreads();
            b ^= 1, s = ns, k0 = nk;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const long long row = row0 + 16 * (rt0 + r) + l15;
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const int col = col0 + 16 * (ct0 + t) + 4 * quad;   // col % 4 == 0 and cout % 4 == 0: four columns or none
            if (ct0 + t >= nt || col >= a.cout || row >= a.n_out) continue;
            const float4 bv = a.bias ? *(const float4 *)(a.bias + col) : zero4();
            *(float4 *)(a.out + row * a.cout + col) =
                make_float4(acc[r][t][0] + bv.x, acc[r][t][1] + bv.y, acc[r][t][2] + bv.z, acc[r][t][3] + bv.w);
        }
    }
}

// grid (blocks of W[s], slots, splits)
__global__ __launch_bounds__(TPB) void oct_conv_bf16_gw_kernel(GwOp a) {
    constexpr int GR = KC;   // rows per stage
    __shared__ int js[GR];
    __shared__ __attribute__((aligned(16))) __bf16 ms[GB * PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 ns[GB * PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, quad = lane >> 4;
    const int mbn = (a.cm + GB - 1) / GB;
    const int m0 = (int)(blockIdx.x % mbn) * GB, n0 = (int)(blockIdx.x / mbn) * GB;
    const int s = blockIdx.y, sp = blockIdx.z, S = a.S;
    const int mt0 = 3 * (wave & 1), nt0 = 3 * (wave >> 1);
    const long long r_lo = (long long)sp * a.rows_per_split, r_hi = min((long long)a.n_out, r_lo + a.rows_per_split);
    const float *msrc = a.x_is_m ? a.x : a.g, *nsrc = a.x_is_m ? a.g : a.x;

    v4f acc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};

    // 96 channels from c0 of 64 rows -> img[channel][row]; x rows are gathered through js, g rows are the table's own
    auto stage = [&](__bf16 *img, const float *src, int width, int c0, bool gathered, long long r0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int it = wave + 4 * i, p = 16 * (it & 1) + l15, q = 4 * (it >> 1) + quad, c = c0 + 4 * q;
            const int j0 = js[2 * p], j1 = js[2 * p + 1];
            float4 u = zero4(), v = zero4();
            if (c < width) {
                if (j0 >= 0) u = *(const float4 *)(src + (size_t)(gathered ? j0 : r0 + 2 * p) * width + c);
                if (j1 >= 0) v = *(const float4 *)(src + (size_t)(gathered ? j1 : r0 + 2 * p + 1) * width + c);
            }
            put_pairs((bf16x2 *)img + 4 * q * WP + p, u, v);
        }
    };

    for (long long r0 = r_lo; r0 < r_hi; r0 += GR) {
        int j = -1;
        if (tid < GR && r0 + tid < r_hi) {
            j = a.tab[(r0 + tid) * S + s];
            if ((unsigned)j >= (unsigned)a.n_in) j = -1;
        }
        if (tid < GR) js[tid] = j;   // (read only between the two barriers below: every wavefront is past that part)
        if (!__syncthreads_or(j >= 0)) continue;
        stage(ms, msrc, a.cm, m0, a.x_is_m != 0, r0);
        stage(ns, nsrc, a.cn, n0, a.x_is_m == 0, r0);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GR / 32; ++kk) {
            ptv2_bf16x8 nv[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) nv[t] = *(const ptv2_bf16x8 *)(ns + (16 * (nt0 + t) + l15) * PITCH + 32 * kk + 8 * quad);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (m0 + 16 * (mt0 + i) >= a.cm) continue;
                const ptv2_bf16x8 mv = *(const ptv2_bf16x8 *)(ms + (16 * (mt0 + i) + l15) * PITCH + 32 * kk + 8 * quad);
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    if (n0 + 16 * (nt0 + t) < a.cn) acc[i][t] = mfma32(mv, nv[t], acc[i][t]);
            }
        }
    }
    float *dst = a.dst + (size_t)sp * a.split_stride + (size_t)s * a.cm * a.cn;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int m = m0 + 16 * (mt0 + i) + 4 * quad;   // m % 4 == 0 and cm % 4 == 0: four or none
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int n = n0 + 16 * (nt0 + t) + l15;
            if (m < a.cm && n < a.cn)
                *(float4 *)(dst + (size_t)n * a.cm + m) = make_float4(acc[i][t][0], acc[i][t][1], acc[i][t][2], acc[i][t][3]);
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- host
// the LAYER's pair: ptv2_octconv_hip.h's set without the stem
bool widths_ok(int slots, int cin, int cout) {
    return (slots == 8 || slots == MAXS) && cin > OCTCONV_STEM_CHANNELS && cin % 4 == 0 && cin <= OCTCONV_MAX_CHANNELS &&
           cout >= 8 && cout % 8 == 0 && cout <= OCTCONV_MAX_CHANNELS;
}
bool pair_ok(const octconv_bf16_args &a) { return a.n_out >= 1 && a.n_in >= 1 && widths_ok(a.slots, a.cin, a.cout); }

template <int NT>
int launch_conv(const ConvOp &op, hipStream_t st) {
    hipLaunchKernelGGL(oct_conv_bf16_kernel<NT>, dim3(divup(op.n_out, ROWS), divup(divup(op.cout, 16), NT)), dim3(TPB), 0, st, op);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// cin, cout of the launch (an input gradient has them exchanged); column blocks of at most 8 tiles, cut evenly as oct_conv.hip's
int conv(const octconv_bf16_args &a, int cin, int cout, hipStream_t st) {
    const ConvOp op = {a.n_out, a.n_in, a.slots, cin, cout, a.transpose ? 1 : 0, a.reverse ? 1 : 0, a.tab, a.x, a.w, a.bias, a.out};
    const int tiles = divup(cout, 16), per = divup(tiles, divup(tiles, 8));
    if (per <= 2) return launch_conv<2>(op, st);
    if (per <= 4) return launch_conv<4>(op, st);
    if (per <= 6) return launch_conv<6>(op, st);
    return launch_conv<8>(op, st);
}

}  // namespace

extern "C" int ptv2_octconv_bf16_abi_version(void) { return 1; }

extern "C" long long ptv2_octconv_bf16_workspace_bytes(int n_out, int slots, int cin, int cout) {
    if (n_out < 1 || !widths_ok(slots, cin, cout)) return -1;
    return ptv2_octconv_workspace_bytes(n_out, slots, cin, cout);
}

extern "C" int oct_conv_bf16_fwd_hip_launcher(const octconv_bf16_args *args, void *stream) {
    if (!args || !pair_ok(*args) || !args->tab || !args->x || !args->w || !args->out) return PTV2_ERR_ARG;
    return conv(*args, args->cin, args->cout, (hipStream_t)stream);
}

extern "C" int oct_conv_bf16_gx_hip_launcher(const octconv_bf16_args *args, void *stream) {
    if (!args || !pair_ok(*args) || !args->tab || !args->x || !args->w || !args->out || args->bias) return PTV2_ERR_ARG;
    return conv(*args, args->cout, args->cin, (hipStream_t)stream);
}

extern "C" int oct_conv_bf16_gw_hip_launcher(const octconv_bf16_args *args, void *stream) {
    if (!args || !pair_ok(*args) || !args->tab || !args->x || !args->g || !args->g_w || !args->workspace) return PTV2_ERR_ARG;
    const octconv_bf16_args &a = *args;
    if (a.workspace_bytes < ptv2_octconv_bf16_workspace_bytes(a.n_out, a.slots, a.cin, a.cout)) return PTV2_ERR_WORKSPACE;
    const int splits = oct_conv_gw_splits(a.n_out);
    const int rows_per_split = divup(divup(a.n_out, splits), KC) * KC;
    // g_w[s] is (cin, cout), m = cout from g; a deconvolution's is (cout, cin), m = cin from x
    const GwOp op = {a.n_out, a.n_in, a.slots, a.transpose ? a.cin : a.cout, a.transpose ? a.cout : a.cin, a.transpose ? 1 : 0,
                     rows_per_split, a.tab, a.x, a.g, splits == 1 ? a.g_w : (float *)a.workspace, (size_t)a.slots * a.cin * a.cout};
    hipLaunchKernelGGL(oct_conv_bf16_gw_kernel, dim3(divup(a.cin, GB) * divup(a.cout, GB), a.slots, splits), dim3(TPB), 0,
                       (hipStream_t)stream, op);
    PTV2_CHECK_LAUNCH();
    return oct_conv_gw_finish(a.n_out, a.slots, a.cin, a.cout, a.g, a.g_w, a.g_b, a.workspace, stream);
}
