// ao_amd/csrc/swin_attention.hip -- Swin3D's sparse window attention with contextual relative signal encoding as one launch per
// direction (include/ptv2_swin_hip.h).  gfx950 only.
//
// Split by head first: a workgroup of four wavefronts owns one head and a contiguous chunk of the windows, on a grid of
// h x chunks that fills the device once.  It copies its head's slice of the three tables from the strided (R, h, hd) parameters
// into LDS once -- (R, hd) each, 69 KB at R = 360, hd = 16 -- and then walks its windows; no transposed table exists in memory.
// The backward keeps a second, zeroed copy of the three slices for the table gradients (138 KB of the 160 KB of a gfx950 CU).
//
// Inside a chunk the unit of work is a strip of 16 members of one window (its "own" side), dealt to the wavefronts in turn, so
// a chunk of small windows keeps all four busy and nothing but the tables is shared: a wavefront never waits for another one
// between the staging and the final partial.  A strip meets the window's members in tiles of 16 (the "other" side):
//   * the tile of dot products is V_MFMA_F32_16X16X4_F32, hd / 4 instructions.  Lane l supplies one value per operand: the
//     other side's member l % 16 as A, its own member l % 16 as B, both at contraction index (l / 16) hd / 4 + step, so a lane
//     reads hd / 4 contiguous floats of a row of qkv through `order`.  In the accumulator lane l holds own member l % 16 against
//     the other members 4 (l / 16) + r: a lane knows its pair, and the own side's vectors and running sums stay in its registers;
//   * the three table terms are added in that layout.  The lane recomputes the 3 groups row indices of its pair from the two
//     signal rows (swin_row: the one statement of the index), sums the rows of a table slice from LDS with 128-bit reads and
//     dots the sum with q or k;
//   * the forward keeps an online softmax per LANE over the keys it meets, and the four lanes of a query are merged once at the
//     end of the strip, so the key loop has no cross-lane step and P never leaves registers.  Members past the window's end are
//     excluded, not masked: their weight is exactly 0.
// The backward sweeps every strip twice with the same routine: own = query gives g_q and the gradients of q_table and v_table
// (the query's own vector is the common factor of its nine LDS adds), own = key gives g_k, g_v and the gradient of k_table.
// The probabilities are recomputed from the row log-sum-exp; delta = g_out . out is formed by the workgroup for its chunk's rows
// before the sweeps.  Every workgroup writes its gradient slices as one partial and swin_table_reduce_kernel sums the partials
// of a head in ascending chunk order.
#include <algorithm>
#include <cfloat>

#include "common.h"
#include "../../include/ptv2_swin_hip.h"

typedef float v4f __attribute__((ext_vector_type(4)));

#define SWIN_TPB 256
#define SWIN_WAVES (SWIN_TPB / WAVE)
#define SWIN_TILE 16
#define SWIN_FWD_MAX_BLOCKS 1024
#define SWIN_BWD_MAX_BLOCKS 512

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
    __device__ __forceinline__ SwinAxes(const swin_args &a) {
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

template <int HD>
__device__ __forceinline__ void swin_st(float *p, const float (&src)[HD], float mul) {
#pragma unroll
    for (int e = 0; e < HD; e += 4) *(float4 *)(p + e) = make_float4(mul * src[e], mul * src[e + 1], mul * src[e + 2], mul * src[e + 3]);
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

// the head's (R, hd) slice of a (R, h, hd) table
template <int HD>
__device__ __forceinline__ void swin_stage(float *slice, const float *table, int R, int H, int h) {
    for (int e = threadIdx.x * 4; e < R * HD; e += SWIN_TPB * 4)
        *(float4 *)(slice + e) = *(const float4 *)(table + ((size_t)(e / HD) * H + h) * HD + e % HD);
}

__host__ __device__ static inline int swin_table_rows(const swin_args &a) {
    int R = 0;
    for (int s = 0; s < a.groups; ++s) R += 6 * a.rows[s];
    return R;
}

// the windows [w0, w1) of chunk c of `chunks`
__device__ __forceinline__ int swin_chunk_start(int windows, int chunks, int c) { return (int)((long long)windows * c / chunks); }

template <int HD, int S>
__global__ __launch_bounds__(SWIN_TPB) void swin_attn_fwd_kernel(swin_args a, int chunks) {
    constexpr int D = 3 * S, Q = HD / 4;
    extern __shared__ float4 swin_smem[];
    const int R = swin_table_rows(a), h = blockIdx.x % a.h, chunk = blockIdx.x / a.h;
    float *tq = (float *)swin_smem, *tk = tq + R * HD, *tv = tk + R * HD;
    swin_stage<HD>(tq, a.q_table, R, a.h, h);
    swin_stage<HD>(tk, a.k_table, R, a.h, h);
    swin_stage<HD>(tv, a.v_table, R, a.h, h);
    __syncthreads();
    const SwinAxes<D> axes(a);
    const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), x = lane & 15, g = lane >> 4;
    const size_t c3 = 3 * (size_t)a.c;
    const float *q_h = a.qkv + h * HD, *k_h = q_h + a.c, *v_h = k_h + a.c;
    const int w1 = swin_chunk_start(a.windows, chunks, chunk + 1);
    int item = 0;
    for (int w = swin_chunk_start(a.windows, chunks, chunk); w < w1; ++w) {
        const int base = a.offsets[w], m = a.offsets[w + 1] - base;
        for (int s0 = 0; s0 < m; s0 += SWIN_TILE, ++item) {
            if (item % SWIN_WAVES != wave) continue;
            const bool own = s0 + x < m;
            const int pi = base + min(s0 + x, m - 1), ni = a.order[pi];
            float q[HD], qb[Q], si[D];
            swin_ld(q, q_h + ni * c3, a.scale);
            swin_ld(qb, q_h + ni * c3 + g * Q, a.scale);
            swin_signals(si, a.signals, pi);
            float top = -FLT_MAX, sum = 0.f, acc[HD];
#pragma unroll
            for (int e = 0; e < HD; ++e) acc[e] = 0.f;
            for (int t0 = 0; t0 < m; t0 += SWIN_TILE) {
                float ka[Q];
                swin_ld(ka, k_h + a.order[base + min(t0 + x, m - 1)] * c3 + g * Q);
                v4f s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < Q; ++e) s = mfma16(ka[e], qb[e], s);   // s[r]: key t0 + 4 g + r against the lane's query
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t0 + 4 * g + r;
                    if (!own || j >= m) continue;
                    const int nj = a.order[base + j];
                    float sj[D], k[HD], v[HD], t[HD];
                    int idx[D];
                    swin_signals(sj, a.signals, base + j);
                    axes.rows(idx, si, sj);
                    swin_ld(k, k_h + nj * c3);
                    swin_ld(v, v_h + nj * c3);
                    swin_row_sum<HD>(t, tq, idx);
                    float e_ij = s[r] + swin_dot(q, t);
                    swin_row_sum<HD>(t, tk, idx);
                    e_ij += swin_dot(k, t);
                    swin_row_sum<HD>(t, tv, idx);
                    if (e_ij > top) {
                        const float f = expf(top - e_ij);
                        sum *= f;
#pragma unroll
                        for (int e = 0; e < HD; ++e) acc[e] *= f;
                        top = e_ij;
                    }
                    const float p = expf(e_ij - top);
                    sum += p;
#pragma unroll
                    for (int e = 0; e < HD; ++e) acc[e] = __builtin_fmaf(p, v[e] + t[e], acc[e]);
                }
            }
            // the four lanes of a query (l % 16 equal) merge their softmax states; a lane that met no key holds (-FLT_MAX, 0, 0)
#pragma unroll
            for (int off = 16; off < WAVE; off <<= 1) {
                const float top_o = __shfl_xor(top, off, WAVE), sum_o = __shfl_xor(sum, off, WAVE);
                const float nt = fmaxf(top, top_o), f = expf(top - nt), f_o = expf(top_o - nt);
                sum = sum * f + sum_o * f_o;
#pragma unroll
                for (int e = 0; e < HD; ++e) acc[e] = acc[e] * f + __shfl_xor(acc[e], off, WAVE) * f_o;
                top = nt;
            }
            if (own && g == 0) {
                swin_st<HD>(a.out + (size_t)ni * a.c + h * HD, acc, 1.f / sum);
                a.lse[(size_t)ni * a.h + h] = top + logf(sum);
            }
        }
    }
}

// One strip of the backward with `own` on the lane.  BYKEY false: own = query i, others = keys j; true: own = key j, others =
// queries i.  a1, a2 are the own side's vectors (scaled q, g_out | k, v), b1, b2 the other side's (k, v | scaled q, g_out):
//   e  = tile(b1, a1) + a1 . T_own + b1 . T_other          T_own = T_Q | T_K, T_other = T_K | T_Q
//   dP = g_out . (v + T_V)                                  (on the vector ALU, in the order of delta)
//   acc1 += dS (b1 + T_own)                                 g_q / scale | g_k
//   own gradient slice rows += dS a1                        g_q_table | g_k_table
//   BYKEY: acc2 += P b2 (g_v); otherwise v gradient slice rows += P a2
template <int HD, int S, bool BYKEY>
__device__ __forceinline__ void swin_bwd_strip(const swin_args &a, const SwinAxes<3 * S> &axes, const float *t_own, const float *t_other,
                                               const float *tv, float *g_own, float *g_tv, const float *delta, int h, int base, int m,
                                               int s0, int lane) {
    constexpr int D = 3 * S, Q = HD / 4;
    const int x = lane & 15, g = lane >> 4;
    const size_t c3 = 3 * (size_t)a.c;
    const float *q_h = a.qkv + h * HD, *k_h = q_h + a.c, *v_h = k_h + a.c, *go_h = a.g_out + h * HD;
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
        float *row = a.g_qkv + no * c3 + h * HD;
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

template <int HD, int S>
__global__ __launch_bounds__(SWIN_TPB) void swin_attn_bwd_kernel(swin_args a, int chunks, float *delta, float *part) {
    constexpr int D = 3 * S;
    extern __shared__ float4 swin_smem[];
    const int R = swin_table_rows(a), h = blockIdx.x % a.h, chunk = blockIdx.x / a.h;
    float *tq = (float *)swin_smem, *tk = tq + R * HD, *tv = tk + R * HD, *gq = tv + R * HD, *gk = gq + R * HD, *gv = gk + R * HD;
    swin_stage<HD>(tq, a.q_table, R, a.h, h);
    swin_stage<HD>(tk, a.k_table, R, a.h, h);
    swin_stage<HD>(tv, a.v_table, R, a.h, h);
    for (int e = threadIdx.x; e < 3 * R * HD; e += SWIN_TPB) gq[e] = 0.f;
    const int w0 = swin_chunk_start(a.windows, chunks, chunk), w1 = swin_chunk_start(a.windows, chunks, chunk + 1);
    // delta of the chunk's rows for this head (sorted positions)
    for (int pos = a.offsets[w0] + threadIdx.x; pos < a.offsets[w1]; pos += SWIN_TPB) {
        const size_t row = (size_t)a.order[pos] * a.c + h * HD;
        float go[HD], o[HD];
        swin_ld(go, a.g_out + row);
        swin_ld(o, a.out + row);
        delta[(size_t)pos * a.h + h] = swin_dot(go, o);
    }
    __syncthreads();
    const SwinAxes<D> axes(a);
    const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    int item = 0;
    for (int w = w0; w < w1; ++w) {
        const int base = a.offsets[w], m = a.offsets[w + 1] - base;
        for (int s0 = 0; s0 < m; s0 += SWIN_TILE, ++item) {
            if (item % SWIN_WAVES != wave) continue;
            swin_bwd_strip<HD, S, false>(a, axes, tq, tk, tv, gq, gv, delta, h, base, m, s0, lane);
            swin_bwd_strip<HD, S, true>(a, axes, tk, tq, tv, gk, gv, delta, h, base, m, s0, lane);
        }
    }
    __syncthreads();
    float *mine = part + (size_t)blockIdx.x * 3 * R * HD;   // block = chunk * h + head
    for (int e = threadIdx.x * 4; e < 3 * R * HD; e += SWIN_TPB * 4) *(float4 *)(mine + e) = *(const float4 *)(gq + e);
}

// g_X_table[row, head, e] = the sum over the chunks' partials, ascending
__global__ __launch_bounds__(SWIN_TPB) void swin_table_reduce_kernel(int chunks, int R, int H, int hd, const float *__restrict__ part,
                                                                     float *gq, float *gk, float *gv) {
    const size_t per = (size_t)R * H * hd, el = (size_t)blockIdx.x * SWIN_TPB + threadIdx.x;
    if (el >= 3 * per) return;
    const int which = (int)(el / per), e = (int)(el % hd), head = (int)(el / hd % H), row = (int)(el % per / ((size_t)H * hd));
    const float *src = part + ((size_t)head * 3 + which) * R * hd + (size_t)row * hd + e;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += src[(size_t)c * H * 3 * R * hd];
    (which == 0 ? gq : which == 1 ? gk : gv)[el % per] = s;
}

extern "C" int ptv2_swin_abi_version(void) { return 1; }
extern "C" int ptv2_swin_struct_bytes(int which) { return which == 0 ? (int)sizeof(swin_args) : -1; }

static bool swin_shape_ok(int n, int windows, int h, int hd, int R) {
    return n >= 1 && windows >= 1 && windows <= n && h >= 1 && h <= SWIN_MAX_HEADS && (hd == 8 || hd == 16) && R >= 6 && R <= SWIN_MAX_ROWS &&
           (long long)n * 3 * h * hd < (1LL << 31);
}

// chunks of windows per head: the grid is h x chunks
static int swin_chunks(int windows, int h, int blocks) { return std::max(1, std::min(windows, blocks / h)); }

extern "C" long long ptv2_swin_workspace_bytes(int n, int windows, int h, int hd, int table_rows) {
    if (!swin_shape_ok(n, windows, h, hd, table_rows)) return -1;
    const size_t blocks = (size_t)h * swin_chunks(windows, h, SWIN_BWD_MAX_BLOCKS);
    return (long long)(ptv2_align256(sizeof(float) * (size_t)n * h) + ptv2_align256(sizeof(float) * blocks * swin_part_floats(table_rows, hd)));
}

static int swin_attention_check(const swin_args *a) {
    if (!a || a->groups < 1 || a->groups > SWIN_MAX_GROUPS) return PTV2_ERR_ARG;
    for (int s = 0; s < a->groups; ++s)
        if (a->rows[s] < 1 || a->rows[s] > SWIN_MAX_ROWS) return PTV2_ERR_ARG;
    if (!swin_shape_ok(a->n, a->windows, a->h, a->hd, swin_table_rows(*a)) || a->c != a->h * a->hd) return PTV2_ERR_ARG;
    if (!a->order || !a->offsets || !a->signals || !a->qkv || !a->q_table || !a->k_table || !a->v_table || !a->out || !a->lse) return PTV2_ERR_ARG;
    return PTV2_OK;
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

extern "C" int swin_attention_fwd_hip_launcher(const swin_args *args, void *stream) {
    RUN(swin_attention_check(args));
    const swin_args &a = *args;
    const size_t lds = sizeof(float) * swin_part_floats(swin_table_rows(a), a.hd);
#define SWIN_FWD(HD, S)                                                                                                          \
    {                                                                                                                            \
        const void *kern = (const void *)swin_attn_fwd_kernel<HD, S>;                                                            \
        RUN(ptv2_kernel_lds(kern, lds));                                                                                         \
        const int chunks = swin_chunks(a.windows, a.h, std::min(ptv2_resident_blocks(kern, SWIN_TPB, lds, 1), SWIN_FWD_MAX_BLOCKS)); \
        hipLaunchKernelGGL((swin_attn_fwd_kernel<HD, S>), dim3(a.h * chunks), dim3(SWIN_TPB), lds, (hipStream_t)stream, a, chunks);  \
    }
    SWIN_DISPATCH(SWIN_FWD);
#undef SWIN_FWD
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int swin_attention_bwd_hip_launcher(const swin_args *args, void *stream) {
    RUN(swin_attention_check(args));
    const swin_args &a = *args;
    if (!a.g_out || !a.g_qkv || !a.g_q_table || !a.g_k_table || !a.g_v_table || !a.workspace) return PTV2_ERR_ARG;
    const int R = swin_table_rows(a);
    if (a.workspace_bytes < ptv2_swin_workspace_bytes(a.n, a.windows, a.h, a.hd, R)) return PTV2_ERR_WORKSPACE;
    PtvCarver ws{(char *)a.workspace, 0};
    float *delta = ws.take_n<float>((size_t)a.n * a.h), *part = (float *)ws.take(0);
    const size_t lds = 2 * sizeof(float) * swin_part_floats(R, a.hd);
    int chunks = 0;
#define SWIN_BWD(HD, S)                                                                                                          \
    {                                                                                                                            \
        const void *kern = (const void *)swin_attn_bwd_kernel<HD, S>;                                                            \
        RUN(ptv2_kernel_lds(kern, lds));                                                                                         \
        chunks = swin_chunks(a.windows, a.h, std::min(ptv2_resident_blocks(kern, SWIN_TPB, lds, 1), SWIN_BWD_MAX_BLOCKS));       \
        hipLaunchKernelGGL((swin_attn_bwd_kernel<HD, S>), dim3(a.h * chunks), dim3(SWIN_TPB), lds, (hipStream_t)stream, a, chunks, delta, part); \
    }
    SWIN_DISPATCH(SWIN_BWD);
#undef SWIN_BWD
    PTV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(swin_table_reduce_kernel, dim3(divup(3LL * R * a.h * a.hd, SWIN_TPB)), dim3(SWIN_TPB), 0, (hipStream_t)stream, chunks, R,
                       a.h, a.hd, (const float *)part, a.g_q_table, a.g_k_table, a.g_v_table);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
