// ao_amd/csrc/oct_attention.hip -- OctFormer's dilated patch attention as one launch per direction (include/ptv2_oct_hip.h;
// DESIGN.md section 19).  gfx950 only.
//
// One workgroup of four wavefronts per patch; a wavefront takes one head at a time (h = wave, wave + 4, ...).  Once per patch,
// for all heads, the workgroup writes to LDS the slot -> node map, the validity bits of every pair and the three clamped table
// indices of every pair as bytes (OctPatch, 3.75 KB).  A wavefront keeps its head's table column (3 R floats) in LDS.
//
// The logit tile is V_MFMA_F32_32X32X2_F32.  In its accumulator lane l owns column l % 32, and its 16 registers hold the rows
// 8 (r / 4) + 4 (l / 32) + r % 4 (acc_row).  The A and the B operand are one value per lane: row / column l % 32, contraction
// index l / 32.  The contraction order is free, so:
//   * the q . k products take e = (l / 32) * hd / 2 + step: a lane reads hd / 2 CONTIGUOUS floats of its slot's q, k (v, g_out)
//     row straight from global memory into registers and feeds them step by step; q, k and v never pass through LDS;
//   * S^T = K Q^T puts query i = l % 32 in the lane and 16 keys in its registers: bias, mask, row maximum, exponent and row sum
//     are in-lane plus one exchange with lane l ^ 32;
//   * O^T = V^T P^T contracts over the keys: in step s each half-wave supplies as B operand the key it already holds in
//     register s, and the A operand V[key(s, l / 32)][e = l % 32] is read with the same assignment (oct_pv): no LDS round trip,
//     and lane l ends with its own query's output, 4 consecutive channels per register quad (float4 stores).
// The backward runs the same tile twice with the operands swapped: S^T (lane = query) gives g_q and the table gradient,
// S = Q K^T (lane = key) gives g_k and g_v through the same oct_pv.  The index bytes of the swapped tile are read through
// idx(i, j) = R - 1 - idx(j, i), so both tiles read LDS bytes [axis][register][lane] without bank conflicts.
#include <cfloat>

#include "common.h"
#include "../../include/ptv2_oct_hip.h"

typedef float v16f __attribute__((ext_vector_type(16)));

#define OCT_TPB 256
#define OCT_WAVES (OCT_TPB / WAVE)
#define OCT_T OCT_MAX_PATCH

__device__ __forceinline__ v16f mfma32(float a, float b, v16f c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// the accumulator row that register r of a lane of half-wave hw holds
__device__ __forceinline__ int acc_row(int r, int hw) { return 8 * (r >> 2) + 4 * hw + (r & 3); }

struct OctPatch {
    int node[OCT_T];                        // slot -> node, -1: padding
    int bat[OCT_T];
    int xyz[OCT_T][3];
    unsigned vm[OCT_T];                     // bit j of vm[i]: both slots real and of one cloud (symmetric)
    unsigned char idx[3][OCT_T][OCT_T];     // [axis][key j][query i]: clamp(xyz_i - xyz_j) + pos_bnd
};
static_assert(sizeof(OctPatch) % 16 == 0, "the wavefronts' floats follow the patch record");

// floats of one wavefront's LDS: the table column, and in the backward its gradient and the lse / delta of the 32 slots
__host__ __device__ static inline int oct_tb_floats(int pos_bnd) { return (3 * (2 * pos_bnd + 1) + 3) & ~3; }
static inline size_t oct_lds_bytes(int pos_bnd, bool bwd) {
    return sizeof(OctPatch) + sizeof(float) * OCT_WAVES * (size_t)(bwd ? 2 * oct_tb_floats(pos_bnd) + 2 * OCT_T : oct_tb_floats(pos_bnd));
}
static inline long long oct_patches(int n, int patch, int dilation) {
    const long long G = (long long)patch * dilation;
    return (n + G - 1) / G * dilation;
}

// the first node of patch p, and (uniformly) whether the patch has any real slot
__device__ __forceinline__ long long oct_first_node(const oct_args &a, int p) {
    return (long long)(p / a.dilation) * a.patch * a.dilation + p % a.dilation;
}

__device__ __forceinline__ void oct_patch_setup(OctPatch &P, const oct_args &a, int p) {
    const int t = threadIdx.x;
    if (t < OCT_T) {
        const long long node = oct_first_node(a, p) + (long long)t * a.dilation;
        const bool real = t < a.patch && node < a.n;
        P.node[t] = real ? (int)node : -1;
        P.bat[t] = real ? a.batch[node] : -1;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) P.xyz[t][ax] = real ? a.xyz[node * 3 + ax] : 0;
    }
    __syncthreads();
    for (int e = t; e < 3 * OCT_T * OCT_T; e += OCT_TPB) {
        const int ax = e / (OCT_T * OCT_T), j = (e / OCT_T) % OCT_T, i = e % OCT_T;
        const int d = min(max(P.xyz[i][ax] - P.xyz[j][ax], -a.pos_bnd), a.pos_bnd);
        P.idx[ax][j][i] = (unsigned char)(d + a.pos_bnd);
    }
    if (t < OCT_T) {
        unsigned m = 0;
        if (P.node[t] >= 0)
            for (int j = 0; j < OCT_T; ++j) m |= (P.node[j] >= 0 && P.bat[j] == P.bat[t]) ? 1u << j : 0u;
        P.vm[t] = m;
    }
    __syncthreads();
}

// N contiguous floats of a row (16-byte aligned), zeros where !ok
template <int N>
__device__ __forceinline__ void oct_load(float (&dst)[N], const float *p, bool ok) {
#pragma unroll
    for (int e = 0; e < N; e += 4) {
        const float4 v = ptv2_ld_or_zero((const float4 *)(ok ? p + e : nullptr), ok);
        dst[e] = v.x; dst[e + 1] = v.y; dst[e + 2] = v.z; dst[e + 3] = v.w;
    }
}

// the tile sum_e A_slot[e] B_slot[e]: rows = the slots of `a`, columns = the slots of `b` (the lane's own)
template <int HALF>
__device__ __forceinline__ v16f oct_tile(const float (&a)[HALF], const float (&b)[HALF]) {
    v16f acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < HALF; ++e) acc = mfma32(a[e], b[e], acc);
    return acc;
}

// acc^T[e][slot] = sum_j src[node_j][e] p_slot[j]: p holds, in register s, the weight of slot j = acc_row(s, hw) for the lane's
// own slot.  src points at the head's first column of row 0; rows are `pitch` floats apart.
template <int HD>
__device__ __forceinline__ v16f oct_pv(const float *__restrict__ src, size_t pitch, const OctPatch &P, const v16f &p, int x, int hw) {
    v16f acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int nj = P.node[acc_row(s, hw)];
        const bool ok = nj >= 0 && x < HD;
        const float av = ptv2_ld_or_zero(ok ? src + (size_t)nj * pitch + x : nullptr, ok);
        acc = mfma32(av, p[s], acc);
    }
    return acc;
}

// rows e = acc_row(r, hw) of acc, r < HD / 2, to dst[e]: 4 consecutive channels per register quad
template <int HD>
__device__ __forceinline__ void oct_store(float *dst, const v16f &acc, int hw, float mul) {
#pragma unroll
    for (int g = 0; g < HD / 8; ++g)
        *(float4 *)(dst + 8 * g + 4 * hw) = make_float4(mul * acc[4 * g], mul * acc[4 * g + 1], mul * acc[4 * g + 2], mul * acc[4 * g + 3]);
}

// the sum of the three table entries of the pair held in register r; swapped: the lane is the key
template <bool SWAPPED>
__device__ __forceinline__ float oct_bias(const OctPatch &P, const float *tb, int R, int row, int x) {
    int i0 = P.idx[0][row][x], i1 = P.idx[1][row][x], i2 = P.idx[2][row][x];
    if (SWAPPED) { i0 = R - 1 - i0; i1 = R - 1 - i1; i2 = R - 1 - i2; }
    return tb[i0] + tb[R + i1] + tb[2 * R + i2];
}

template <int HD>
__global__ __launch_bounds__(OCT_TPB) void oct_attn_fwd_kernel(oct_args a) {
    constexpr int HALF = HD / 2;
    extern __shared__ float4 oct_smem[];
    OctPatch &P = *(OctPatch *)oct_smem;
    const int p = blockIdx.x;
    if (oct_first_node(a, p) >= a.n) return;   // (uniform) no real slot
    oct_patch_setup(P, a, p);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, x = lane & 31, hw = lane >> 5;
    const int R = 2 * a.pos_bnd + 1, R3 = 3 * R;
    float *tb = (float *)oct_smem + sizeof(OctPatch) / 4 + wave * oct_tb_floats(a.pos_bnd);
    const int node = P.node[x];
    const bool real = node >= 0;
    const unsigned vm = P.vm[x];
    const size_t c3 = 3 * (size_t)a.c;
    for (int h = wave; h < a.h; h += OCT_WAVES) {
        wave_lds_sync();   // the previous head's reads of tb are done
        for (int r = lane; r < R3; r += WAVE) tb[r] = a.table[(size_t)r * a.h + h];
        wave_lds_sync();
        float q[HALF], k[HALF];
        const float *row = a.qkv + (size_t)(real ? node : 0) * c3 + h * HD + hw * HALF;
        oct_load(q, row, real);
        oct_load(k, row + a.c, real);
        v16f s = oct_tile<HALF>(k, q);   // S^T: the lane's query x against the keys acc_row(r, hw)
        float top = -FLT_MAX;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = acc_row(r, hw);
            s[r] = (vm >> j & 1u) ? __builtin_fmaf(a.scale, s[r], oct_bias<false>(P, tb, R, j, x)) : -FLT_MAX;
            top = fmaxf(top, s[r]);
        }
        top = fmaxf(top, __shfl_xor(top, 32, WAVE));
        if (top == -FLT_MAX) top = 0.f;   // a padding slot: every weight is 0
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = (vm >> acc_row(r, hw) & 1u) ? expf(s[r] - top) : 0.f;
            sum += s[r];
        }
        sum += __shfl_xor(sum, 32, WAVE);
        const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= inv;
        const v16f o = oct_pv<HD>(a.qkv + 2 * (size_t)a.c + h * HD, c3, P, s, x, hw);
        if (real) {
            oct_store<HD>(a.out + (size_t)node * a.c + h * HD, o, hw, 1.f);
            if (hw == 0) a.lse[(size_t)node * a.h + h] = top + logf(sum);
        }
    }
}

template <int HD>
__global__ __launch_bounds__(OCT_TPB) void oct_attn_bwd_kernel(oct_args a) {
    constexpr int HALF = HD / 2;
    extern __shared__ float4 oct_smem[];
    OctPatch &P = *(OctPatch *)oct_smem;
    const int p = blockIdx.x;
    const int R = 2 * a.pos_bnd + 1, R3 = 3 * R;
    float *part = (float *)a.workspace + (size_t)p * R3 * a.h;   // this patch's (3 R, h) partial of g_table
    if (oct_first_node(a, p) >= a.n) {   // (uniform) no real slot
        for (int e = threadIdx.x; e < R3 * a.h; e += OCT_TPB) part[e] = 0.f;
        return;
    }
    oct_patch_setup(P, a, p);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, x = lane & 31, hw = lane >> 5;
    const int tbf = oct_tb_floats(a.pos_bnd);
    float *tb = (float *)oct_smem + sizeof(OctPatch) / 4 + wave * (2 * tbf + 2 * OCT_T);
    float *gt = tb + tbf, *lse_s = gt + tbf, *delta_s = lse_s + OCT_T;
    const int node = P.node[x];
    const bool real = node >= 0;
    const unsigned vm = P.vm[x];
    const size_t c3 = 3 * (size_t)a.c, safe = real ? node : 0;
    for (int h = wave; h < a.h; h += OCT_WAVES) {
        wave_lds_sync();   // the previous head's reads of tb, gt, lse_s and delta_s are done
        for (int r = lane; r < R3; r += WAVE) { tb[r] = a.table[(size_t)r * a.h + h]; gt[r] = 0.f; }
        float q[HALF], k[HALF], v[HALF], go[HALF], o[HALF];
        const float *row = a.qkv + safe * c3 + h * HD + hw * HALF;
        oct_load(q, row, real);
        oct_load(k, row + a.c, real);
        oct_load(v, row + 2 * (size_t)a.c, real);
        oct_load(go, a.g_out + safe * a.c + h * HD + hw * HALF, real);
        oct_load(o, a.out + safe * a.c + h * HD + hw * HALF, real);
        float delta = 0.f;
#pragma unroll
        for (int e = 0; e < HALF; ++e) delta = __builtin_fmaf(go[e], o[e], delta);
        delta += __shfl_xor(delta, 32, WAVE);
        const float lse = real ? a.lse[safe * a.h + h] : 0.f;
        if (hw == 0) { lse_s[x] = lse; delta_s[x] = delta; }
        wave_lds_sync();

        // the lane is the query: g_q and the table gradient
        v16f s = oct_tile<HALF>(k, q), dp = oct_tile<HALF>(v, go);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = acc_row(r, hw);
            const bool ok = vm >> j & 1u;
            const float pr = ok ? expf(__builtin_fmaf(a.scale, s[r], oct_bias<false>(P, tb, R, j, x)) - lse) : 0.f;
            s[r] = pr * (dp[r] - delta);
            if (ok) {
                atomicAdd(&gt[P.idx[0][j][x]], s[r]);
                atomicAdd(&gt[R + P.idx[1][j][x]], s[r]);
                atomicAdd(&gt[2 * R + P.idx[2][j][x]], s[r]);
            }
        }
        v16f g = oct_pv<HD>(a.qkv + (size_t)a.c + h * HD, c3, P, s, x, hw);   // sum_j K[j] dS[x][j]
        if (real) oct_store<HD>(a.g_qkv + (size_t)node * c3 + h * HD, g, hw, a.scale);

        // the lane is the key: g_v and g_k
        s = oct_tile<HALF>(q, k);
        dp = oct_tile<HALF>(go, v);
        v16f ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = acc_row(r, hw);
            const bool ok = vm >> i & 1u;
            s[r] = ok ? expf(__builtin_fmaf(a.scale, s[r], oct_bias<true>(P, tb, R, i, x)) - lse_s[i]) : 0.f;
            ds[r] = s[r] * (dp[r] - delta_s[i]);
        }
        g = oct_pv<HD>(a.g_out + h * HD, (size_t)a.c, P, s, x, hw);           // sum_i g_out[i] P[i][x]
        if (real) oct_store<HD>(a.g_qkv + (size_t)node * c3 + 2 * (size_t)a.c + h * HD, g, hw, 1.f);
        g = oct_pv<HD>(a.qkv + h * HD, c3, P, ds, x, hw);                    // sum_i Q[i] dS[i][x]
        if (real) oct_store<HD>(a.g_qkv + (size_t)node * c3 + a.c + h * HD, g, hw, a.scale);

        wave_lds_sync();   // the LDS adds have landed
        for (int r = lane; r < R3; r += WAVE) part[(size_t)r * a.h + h] = gt[r];
    }
}

// g_table[e] = the sum over the patches' partials in a fixed order: 32 elements per workgroup, eight interleaved slices of the
// patches summed ascending by one thread each, then the slices ascending
#define OCT_RED_ELEMS 32
#define OCT_RED_SLICES (OCT_TPB / OCT_RED_ELEMS)
__global__ __launch_bounds__(OCT_TPB) void oct_table_reduce_kernel(int patches, int elems, const float *__restrict__ part, float *__restrict__ g_table) {
    __shared__ float red[OCT_RED_SLICES][OCT_RED_ELEMS];
    const int el = threadIdx.x % OCT_RED_ELEMS, sl = threadIdx.x / OCT_RED_ELEMS, e = blockIdx.x * OCT_RED_ELEMS + el;
    float s = 0.f;
    if (e < elems)
        for (int p = sl; p < patches; p += OCT_RED_SLICES) s += part[(size_t)p * elems + e];
    red[sl][el] = s;
    __syncthreads();
    if (sl == 0 && e < elems) {
        for (int k = 1; k < OCT_RED_SLICES; ++k) s += red[k][el];
        g_table[e] = s;
    }
}

extern "C" int ptv2_oct_abi_version(void) { return 1; }
extern "C" int ptv2_oct_struct_bytes(int which) { return which == 0 ? (int)sizeof(oct_args) : -1; }

static bool oct_attention_shape_ok(int n, int patch, int dilation, int h, int rpe) {
    return n >= 1 && patch >= 1 && patch <= OCT_MAX_PATCH && dilation >= 1 && h >= 1 && h <= OCT_MAX_HEADS && rpe >= 1 &&
           rpe <= OCT_MAX_RPE && rpe % 2 == 1 && oct_patches(n, patch, dilation) < (1LL << 30);
}

extern "C" long long ptv2_oct_workspace_bytes(int n, int patch, int dilation, int h, int rpe) {
    if (!oct_attention_shape_ok(n, patch, dilation, h, rpe)) return -1;
    return (long long)ptv2_align256(sizeof(float) * (size_t)oct_patches(n, patch, dilation) * 3 * rpe * h);
}

static int oct_attention_check(const oct_args *a) {
    if (!a || a->pos_bnd < 0 || a->pos_bnd > OCT_MAX_RPE / 2 || !oct_attention_shape_ok(a->n, a->patch, a->dilation, a->h, 2 * a->pos_bnd + 1))
        return PTV2_ERR_ARG;
    if ((a->hd != 16 && a->hd != 32) || a->c != a->h * a->hd || !a->xyz || !a->batch || !a->qkv || !a->table || !a->out || !a->lse)
        return PTV2_ERR_ARG;
    return PTV2_OK;
}

extern "C" int oct_attention_fwd_hip_launcher(const oct_args *args, void *stream) {
    RUN(oct_attention_check(args));
    const oct_args &a = *args;
    const dim3 grid((unsigned)oct_patches(a.n, a.patch, a.dilation));
    const size_t lds = oct_lds_bytes(a.pos_bnd, false);
    if (a.hd == 16) hipLaunchKernelGGL(oct_attn_fwd_kernel<16>, grid, dim3(OCT_TPB), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(oct_attn_fwd_kernel<32>, grid, dim3(OCT_TPB), lds, (hipStream_t)stream, a);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int oct_attention_bwd_hip_launcher(const oct_args *args, void *stream) {
    RUN(oct_attention_check(args));
    const oct_args &a = *args;
    if (!a.g_out || !a.g_qkv || !a.g_table || !a.workspace) return PTV2_ERR_ARG;
    if (a.workspace_bytes < ptv2_oct_workspace_bytes(a.n, a.patch, a.dilation, a.h, 2 * a.pos_bnd + 1)) return PTV2_ERR_WORKSPACE;
    const long long patches = oct_patches(a.n, a.patch, a.dilation);
    const int elems = 3 * (2 * a.pos_bnd + 1) * a.h;
    const size_t lds = oct_lds_bytes(a.pos_bnd, true);
    if (a.hd == 16) hipLaunchKernelGGL(oct_attn_bwd_kernel<16>, dim3((unsigned)patches), dim3(OCT_TPB), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(oct_attn_bwd_kernel<32>, dim3((unsigned)patches), dim3(OCT_TPB), lds, (hipStream_t)stream, a);
    PTV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(oct_table_reduce_kernel, dim3(divup(elems, OCT_RED_ELEMS)), dim3(OCT_TPB), 0, (hipStream_t)stream, (int)patches, elems,
                       (const float *)a.workspace, a.g_table);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
