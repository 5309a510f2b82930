// ao_amd/csrc/swin_core.h -- what the two units of Swin3D's window attention share (swin_attention.hip: fp32 storage;
// swin_attention_f16.hip: half storage; DESIGN.md sections 21 and 22): the index of a pair, the row loads and stores per storage
// type, the staging of a head's table slices, and the backward, which is one routine over the type of qkv, out, g_out and g_qkv.
//
// Every routine takes its operands as a struct A with the field names of swin_args (include/ptv2_swin_hip.h); the storage type T
// is the pointee of A::qkv.  With T = float nothing here rounds and the kernels of swin_attention.hip are the code they were.
// With T = _Float16 a row is widened to fp32 as it is loaded, a result is rounded to half once, as it is stored, and the staged
// table values are rounded to half and widened again (the function the half forward computed); all arithmetic stays fp32.
#pragma once
#include <algorithm>
#include <cfloat>
#include <type_traits>

#include "common.h"
#include "../../include/ptv2_swin_hip.h"

typedef float v4f __attribute__((ext_vector_type(4)));
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
typedef _Float16 v4h __attribute__((ext_vector_type(4)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

#define SWIN_TPB 256
#define SWIN_WAVES (SWIN_TPB / WAVE)
#define SWIN_TILE 16
#define SWIN_BWD_MAX_BLOCKS 512

template <class A>
using swin_storage_t = std::remove_cv_t<std::remove_pointer_t<decltype(A::qkv)>>;

__device__ __forceinline__ v4f mfma16(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// THE index of a pair on one signal axis: the row of the axis' table block that (i, j) reads (tests/swin3d_ref.py and
// ao_amd/swin3d/ops.py: crse_rows state the same).  The clamp is on the float so that no NaN or huge difference leaves the block.
__device__ __forceinline__ int swin_row(float si, float sj, int L) {
    return (int)fminf(fmaxf(floorf(si - sj) + (float)L, 0.f), (float)(2 * L - 1));
}

// per signal axis d: the first row of its block in the (R, hd) slice, and L
template <int D>
struct SwinAxes {
    int row0[D], L[D];
    template <class A>
    __device__ __forceinline__ SwinAxes(const A &a) {
        int base = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            L[d] = a.rows[d / 3];
            row0[d] = base + (d % 3) * 2 * L[d];
            if (d % 3 == 2) base += 6 * L[d];
        }
    }
    // the rows of the pair (i, j) in the slice
    __device__ __forceinline__ void rows(int (&idx)[D], const float (&si)[D], const float (&sj)[D]) const {
#pragma unroll
        for (int d = 0; d < D; ++d) idx[d] = row0[d] + swin_row(si[d], sj[d], L[d]);
    }
};

// N contiguous floats (N = 2: 8-byte, otherwise 16-byte aligned), times mul
template <int N>
__device__ __forceinline__ void swin_ld(float (&dst)[N], const float *p, float mul = 1.f) {
    if constexpr (N == 2) {
        const float2 v = *(const float2 *)p;
        dst[0] = mul * v.x; dst[1] = mul * v.y;
    } else {
#pragma unroll
        for (int e = 0; e < N; e += 4) {
            const float4 v = *(const float4 *)(p + e);
            dst[e] = mul * v.x; dst[e + 1] = mul * v.y; dst[e + 2] = mul * v.z; dst[e + 3] = mul * v.w;
        }
    }
}

// N contiguous halves (N = 2: 4-byte, N = 4: 8-byte, otherwise 16-byte aligned), widened, times mul in fp32
template <int N>
__device__ __forceinline__ void swin_ld(float (&dst)[N], const _Float16 *p, float mul = 1.f) {
    if constexpr (N == 2) {
        const v2h v = *(const v2h *)p;
        dst[0] = mul * (float)v[0]; dst[1] = mul * (float)v[1];
    } else if constexpr (N == 4) {
        const v4h v = *(const v4h *)p;
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[i] = mul * (float)v[i];
    } else {
#pragma unroll
        for (int e = 0; e < N; e += 8) {
            const v8h v = *(const v8h *)(p + e);
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[e + i] = mul * (float)v[i];
        }
    }
}

template <int HD>
__device__ __forceinline__ void swin_st(float *p, const float (&src)[HD], float mul) {
#pragma unroll
    for (int e = 0; e < HD; e += 4) *(float4 *)(p + e) = make_float4(mul * src[e], mul * src[e + 1], mul * src[e + 2], mul * src[e + 3]);
}

// the one rounding of a result: mul * src in fp32, to half (nearest even) in the 16-byte store
template <int HD>
__device__ __forceinline__ void swin_st(_Float16 *p, const float (&src)[HD], float mul) {
#pragma unroll
    for (int e = 0; e < HD; e += 8) {
        v8h v;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (_Float16)(mul * src[e + i]);
        *(v8h *)(p + e) = v;
    }
}

template <int D>
__device__ __forceinline__ void swin_signals(float (&s)[D], const float *signals, int pos) {
#pragma unroll
    for (int d = 0; d < D; ++d) s[d] = signals[(size_t)pos * D + d];
}

// t = the sum of the pair's D rows of one slice
template <int HD, int D>
__device__ __forceinline__ void swin_row_sum(float (&t)[HD], const float *slice, const int (&idx)[D]) {
#pragma unroll
    for (int e = 0; e < HD; ++e) t[e] = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float4 *row = (const float4 *)(slice + idx[d] * HD);
#pragma unroll
        for (int e = 0; e < HD / 4; ++e) {
            const float4 v = row[e];
            t[4 * e] += v.x; t[4 * e + 1] += v.y; t[4 * e + 2] += v.z; t[4 * e + 3] += v.w;
        }
    }
}

template <int HD>
__device__ __forceinline__ float swin_dot(const float (&a)[HD], const float (&b)[HD]) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < HD; ++e) s = __builtin_fmaf(a[e], b[e], s);
    return s;
}

// gradient slice rows of the pair += w * vec
template <int HD, int D>
__device__ __forceinline__ void swin_scatter(float *slice, const int (&idx)[D], float w, const float (&vec)[HD]) {
    float wv[HD];
#pragma unroll
    for (int e = 0; e < HD; ++e) wv[e] = w * vec[e];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int e = 0; e < HD; ++e) __hip_atomic_fetch_add(slice + idx[d] * HD + e, wv[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ float swin_half_rounded(float v) { return (float)(_Float16)v; }

// the head's (R, hd) slice of a (R, h, hd) table; ROUND: every value rounded to half and widened again
template <int HD, bool ROUND = false>
__device__ __forceinline__ void swin_stage(float *slice, const float *table, int R, int H, int h) {
    for (int e = threadIdx.x * 4; e < R * HD; e += SWIN_TPB * 4) {
        float4 v = *(const float4 *)(table + ((size_t)(e / HD) * H + h) * HD + e % HD);
        if constexpr (ROUND) v = make_float4(swin_half_rounded(v.x), swin_half_rounded(v.y), swin_half_rounded(v.z), swin_half_rounded(v.w));
        *(float4 *)(slice + e) = v;
    }
}

template <class A>
__host__ __device__ static inline int swin_table_rows(const A &a) {
    int R = 0;
    for (int s = 0; s < a.groups; ++s) R += 6 * a.rows[s];
    return R;
}

// the windows [w0, w1) of chunk c of `chunks`
__device__ __forceinline__ int swin_chunk_start(int windows, int chunks, int c) { return (int)((long long)windows * c / chunks); }

// One strip of the backward with `own` on the lane.  BYKEY false: own = query i, others = keys j; true: own = key j, others =
// queries i.  a1, a2 are the own side's vectors (scaled q, g_out | k, v), b1, b2 the other side's (k, v | scaled q, g_out):
//   e  = tile(b1, a1) + a1 . T_own + b1 . T_other          T_own = T_Q | T_K, T_other = T_K | T_Q
//   dP = g_out . (v + T_V)                                  (on the vector ALU, in the order of delta)
//   acc1 += dS (b1 + T_own)                                 g_q / scale | g_k
//   own gradient slice rows += dS a1                        g_q_table | g_k_table
//   BYKEY: acc2 += P b2 (g_v); otherwise v gradient slice rows += P a2
template <int HD, int S, bool BYKEY, class A>
__device__ __forceinline__ void swin_bwd_strip(const A &a, const SwinAxes<3 * S> &axes, const float *t_own, const float *t_other,
                                               const float *tv, float *g_own, float *g_tv, const float *delta, int h, int base, int m,
                                               int s0, int lane) {
    using T = swin_storage_t<A>;
    constexpr int D = 3 * S, Q = HD / 4;
    const int x = lane & 15, g = lane >> 4;
    const size_t c3 = 3 * (size_t)a.c;
    const T *q_h = a.qkv + h * HD, *k_h = q_h + a.c, *v_h = k_h + a.c, *go_h = a.g_out + h * HD;
    const bool own = s0 + x < m;
    const int po = base + min(s0 + x, m - 1), no = a.order[po];
    float a1[HD], a2[HD], a1b[Q], so[D];
    if (BYKEY) {
        swin_ld(a1, k_h + no * c3);
        swin_ld(a1b, k_h + no * c3 + g * Q);
        swin_ld(a2, v_h + no * c3);
    } else {
        swin_ld(a1, q_h + no * c3, a.scale);
        swin_ld(a1b, q_h + no * c3 + g * Q, a.scale);
        swin_ld(a2, go_h + (size_t)no * a.c);
    }
    swin_signals(so, a.signals, po);
    const float lse_o = a.lse[(size_t)no * a.h + h], delta_o = delta[(size_t)po * a.h + h];
    float acc1[HD], acc2[HD];
#pragma unroll
    for (int e = 0; e < HD; ++e) acc1[e] = acc2[e] = 0.f;
    for (int t0 = 0; t0 < m; t0 += SWIN_TILE) {
        const int na = a.order[base + min(t0 + x, m - 1)];
        float r1[Q];
        if (BYKEY) swin_ld(r1, q_h + na * c3 + g * Q, a.scale);
        else swin_ld(r1, k_h + na * c3 + g * Q);
        v4f s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < Q; ++e) s = mfma16(r1[e], a1b[e], s);   // s[r]: other member t0 + 4 g + r against the lane's own
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = t0 + 4 * g + r;
            if (!own || p >= m) continue;
            const int np = a.order[base + p];
            float sp[D], b1[HD], b2[HD], t[HD];
            int idx[D];
            swin_signals(sp, a.signals, base + p);
            if (BYKEY) {
                axes.rows(idx, sp, so);
                swin_ld(b1, q_h + np * c3, a.scale);
                swin_ld(b2, go_h + (size_t)np * a.c);
            } else {
                axes.rows(idx, so, sp);
                swin_ld(b1, k_h + np * c3);
                swin_ld(b2, v_h + np * c3);
            }
            // e_ij and dP in the forward's order of operations (q term, then k term; g_out . (v + T_V) as delta = g_out . out):
            // a window of one member then has P = 1 and dS = 0 exactly, as the eager statements have
            swin_row_sum<HD>(t, t_own, idx);
            const float d_own = swin_dot(a1, t);
            float b1t[HD], vt[HD];
#pragma unroll
            for (int e = 0; e < HD; ++e) b1t[e] = b1[e] + t[e];
            swin_row_sum<HD>(t, t_other, idx);
            const float d_other = swin_dot(b1, t);
            const float e_ij = BYKEY ? (s[r] + d_other) + d_own : (s[r] + d_own) + d_other;
            swin_row_sum<HD>(t, tv, idx);
#pragma unroll
            for (int e = 0; e < HD; ++e) vt[e] = (BYKEY ? a2[e] : b2[e]) + t[e];
            const float dpv = swin_dot(BYKEY ? b2 : a2, vt);
            const float lse = BYKEY ? a.lse[(size_t)np * a.h + h] : lse_o, del = BYKEY ? delta[(size_t)(base + p) * a.h + h] : delta_o;
            const float pr = expf(e_ij - lse), ds = pr * (dpv - del);
#pragma unroll
            for (int e = 0; e < HD; ++e) acc1[e] = __builtin_fmaf(ds, b1t[e], acc1[e]);
            swin_scatter<HD>(g_own, idx, ds, a1);
            if (BYKEY) {
#pragma unroll
                for (int e = 0; e < HD; ++e) acc2[e] = __builtin_fmaf(pr, b2[e], acc2[e]);
            } else {
                swin_scatter<HD>(g_tv, idx, pr, a2);
            }
        }
    }
#pragma unroll
    for (int off = 16; off < WAVE; off <<= 1)
#pragma unroll
        for (int e = 0; e < HD; ++e) {
            acc1[e] += __shfl_xor(acc1[e], off, WAVE);
            if (BYKEY) acc2[e] += __shfl_xor(acc2[e], off, WAVE);
        }
    if (own && g == 0) {
        T *row = a.g_qkv + no * c3 + h * HD;
        if (BYKEY) {
            swin_st<HD>(row + a.c, acc1, 1.f);
            swin_st<HD>(row + 2 * (size_t)a.c, acc2, 1.f);
        } else {
            swin_st<HD>(row, acc1, a.scale);
        }
    }
}

// floats of one workgroup's partial: the three gradient slices
static inline size_t swin_part_floats(int R, int hd) { return 3 * (size_t)R * hd; }

// The backward of one workgroup (head blockIdx.x % h, chunk blockIdx.x / h): the body of the kernel of either storage type, over
// the kernel's parameters (a, chunks, delta, part).  LDS: six (R, HD) fp32 slices, the staged tables and their zeroed gradients.
// (A macro, not a routine: written into swin_attn_bwd_kernel as it always was, the fp32 kernel compiles to the code it was.)
#define SWIN_BWD_KERNEL_BODY(ROUND)                                                                                              \
    constexpr int D = 3 * S;                                                                                                     \
    extern __shared__ float4 swin_smem[];                                                                                        \
    const int R = swin_table_rows(a), h = blockIdx.x % a.h, chunk = blockIdx.x / a.h;                                            \
    float *tq = (float *)swin_smem, *tk = tq + R * HD, *tv = tk + R * HD, *gq = tv + R * HD, *gk = gq + R * HD, *gv = gk + R * HD; \
    swin_stage<HD, ROUND>(tq, a.q_table, R, a.h, h);                                                                             \
    swin_stage<HD, ROUND>(tk, a.k_table, R, a.h, h);                                                                             \
    swin_stage<HD, ROUND>(tv, a.v_table, R, a.h, h);                                                                             \
    for (int e = threadIdx.x; e < 3 * R * HD; e += SWIN_TPB) gq[e] = 0.f;                                                        \
    const int w0 = swin_chunk_start(a.windows, chunks, chunk), w1 = swin_chunk_start(a.windows, chunks, chunk + 1);              \
    /* delta of the chunk's rows for this head (sorted positions) */                                                             \
    for (int pos = a.offsets[w0] + threadIdx.x; pos < a.offsets[w1]; pos += SWIN_TPB) {                                          \
        const size_t row = (size_t)a.order[pos] * a.c + h * HD;                                                                  \
        float go[HD], o[HD];                                                                                                     \
        swin_ld(go, a.g_out + row);                                                                                              \
        swin_ld(o, a.out + row);                                                                                                 \
        delta[(size_t)pos * a.h + h] = swin_dot(go, o);                                                                          \
    }                                                                                                                            \
    __syncthreads();                                                                                                             \
    const SwinAxes<D> axes(a);                                                                                                   \
    const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);                        \
    int item = 0;                                                                                                                \
    for (int w = w0; w < w1; ++w) {                                                                                              \
        const int base = a.offsets[w], m = a.offsets[w + 1] - base;                                                              \
        for (int s0 = 0; s0 < m; s0 += SWIN_TILE, ++item) {                                                                      \
            if (item % SWIN_WAVES != wave) continue;                                                                             \
            swin_bwd_strip<HD, S, false>(a, axes, tq, tk, tv, gq, gv, delta, h, base, m, s0, lane);                              \
            swin_bwd_strip<HD, S, true>(a, axes, tk, tq, tv, gk, gv, delta, h, base, m, s0, lane);                               \
        }                                                                                                                        \
    }                                                                                                                            \
    __syncthreads();                                                                                                             \
    float *mine = part + (size_t)blockIdx.x * 3 * R * HD; /* block = chunk * h + head */                                         \
    for (int e = threadIdx.x * 4; e < 3 * R * HD; e += SWIN_TPB * 4) *(float4 *)(mine + e) = *(const float4 *)(gq + e);

// ---- host --------------------------------------------------------------------------------------------------------------
static inline bool swin_shape_ok(int n, int windows, int h, int hd, int R) {
    return n >= 1 && windows >= 1 && windows <= n && h >= 1 && h <= SWIN_MAX_HEADS && (hd == 8 || hd == 16) && R >= 6 && R <= SWIN_MAX_ROWS &&
           (long long)n * 3 * h * hd < (1LL << 31);
}

// chunks of windows per head: the grid is h x chunks
static inline int swin_chunks(int windows, int h, int blocks) { return std::max(1, std::min(windows, blocks / h)); }

// what a backward launcher needs behind `workspace`: delta (n, h) and one partial per workgroup of the largest grid
static inline long long swin_bwd_workspace_bytes(int n, int windows, int h, int hd, int table_rows) {
    if (!swin_shape_ok(n, windows, h, hd, table_rows)) return -1;
    const size_t blocks = (size_t)h * swin_chunks(windows, h, SWIN_BWD_MAX_BLOCKS);
    return (long long)(ptv2_align256(sizeof(float) * (size_t)n * h) + ptv2_align256(sizeof(float) * blocks * swin_part_floats(table_rows, hd)));
}

// the instantiation of (hd, groups)
#define SWIN_DISPATCH(CALL)                                          \
    do {                                                             \
        if (a.hd == 8) {                                             \
            if (a.groups == 1) { CALL(8, 1); } else if (a.groups == 2) { CALL(8, 2); } else { CALL(8, 3); }    \
        } else {                                                     \
            if (a.groups == 1) { CALL(16, 1); } else if (a.groups == 2) { CALL(16, 2); } else { CALL(16, 3); } \
        }                                                            \
    } while (0)
