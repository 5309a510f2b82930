// ao_amd/csrc/stratified.hip -- Stratified Transformer (ST-v1m2): window cells, pair lists, the relative-position index, the
// three pointops2 operators with their row softmax, and the fused window attention (C ABI include/ptv2_st_hip.h; DESIGN.md
// section 14).
//
// One kernel template serves every operator: st_row_kernel<HD, OP>.  A group of 16 lanes owns one (row, head): a query with its
// pairs (offsets / index1) or, for the by-key backwards, a key with the pairs that name it (t_offsets / t_query / t_pair); a wave
// holds four rows of one head.  (A row of a ScanNet level has about 45 pairs: with a whole wave per row a third of the lanes idle
// and the 16 x 6 shuffles of the final fold cost as much as the row.)  A lane takes every 16th pair of the row, keeps its partial
// sums in registers, and the group folds them through xor shuffles in a fixed order, so q / k / v gradients and every forward
// output are written once, by one group, and are bit-repeatable.  No row length is special: a row of one pair and a row of 5000
// run the same loop.
//
// Table gradients.  A pair adds g * x[d] to table[rel_a, head, a, d] for the three axes a, where x is the ROW's own vector (q_i by
// query, k_j by key, dO_i for the value table by query).  The group therefore sums the scalar g per (rel, a) into 3 L LDS floats of
// its own, and after the row adds S[rel, a] * x[:] into the workgroup's copy of the head's table slice; the slice goes to memory
// once per workgroup.  Both steps use float atomics (LDS, then global): these three gradients are not bit-repeatable.
//
// The unit is compiled with -ffp-contract=off (Makefile): cells and the relative index must round as the eager statements do.
// Every multiply-add of the hot loops is an explicit fmaf.
#include <cfloat>

#include "common.h"
#include "../../include/ptv2_st_hip.h"

#define ST_TPB 256
#define ST_WAVES (ST_TPB / WAVE)
#define ST_GROUP 16                      // lanes that share one (row, head)
#define ST_GROUPS (WAVE / ST_GROUP)      // rows of one wave
#define ST_ROWS (ST_WAVES * ST_GROUPS)   // rows of one workgroup round
#define ST_MAX_LDS (64 * 1024)

// ------------------------------------------------------------------------------------------------------- helpers ----
// over the ST_GROUP lanes of one row, in a fixed order; every lane of the group ends with the result
__device__ __forceinline__ float st_group_sum(float v) {
#pragma unroll
    for (int m = ST_GROUP / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}
__device__ __forceinline__ float st_group_max(float v) {
#pragma unroll
    for (int m = ST_GROUP / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, WAVE));
    return v;
}
template <int HD>
__device__ __forceinline__ void st_ld(float (&r)[HD], const float *__restrict__ p) {
    const float4 *p4 = (const float4 *)p;
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
        const float4 t = p4[c];
        r[4 * c] = t.x; r[4 * c + 1] = t.y; r[4 * c + 2] = t.z; r[4 * c + 3] = t.w;
    }
}
template <int HD>
__device__ __forceinline__ void st_st(float *__restrict__ p, const float (&r)[HD]) {
    float4 *p4 = (float4 *)p;
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) p4[c] = make_float4(r[4 * c], r[4 * c + 1], r[4 * c + 2], r[4 * c + 3]);
}
template <int HD>
__device__ __forceinline__ float st_dot(const float (&x)[HD], const float (&y)[HD]) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) s = __builtin_fmaf(x[d], y[d], s);
    return s;
}
template <int HD>
__device__ __forceinline__ void st_zero(float (&x)[HD]) {
#pragma unroll
    for (int d = 0; d < HD; ++d) x[d] = 0.f;
}
// the sum over the three axes of one table for one pair: (t[r0, a=0] + t[r1, a=1]) + t[r2, a=2], the reference's order
template <int HD>
__device__ __forceinline__ void st_tsum(float (&r)[HD], const float *__restrict__ t, int h, int hh, const int (&rel)[3]) {
    float x[HD], y[HD], z[HD];
    st_ld<HD>(x, t + (((long long)rel[0] * h + hh) * 3 + 0) * HD);
    st_ld<HD>(y, t + (((long long)rel[1] * h + hh) * 3 + 1) * HD);
    st_ld<HD>(z, t + (((long long)rel[2] * h + hh) * 3 + 2) * HD);
#pragma unroll
    for (int d = 0; d < HD; ++d) r[d] = (x[d] + y[d]) + z[d];
}

// stratified_transformer_v1m2_refine.py:145-151 for one axis as the device evaluates them: torch divides by a python scalar
// through the scalar's fp32 reciprocal, `+ 2 * window_size` and `- 1e-4` are two roundings.  Clamped: the index addresses memory.
__device__ __forceinline__ int st_rel_axis(float ci, float cj, float two_w, float inv_q, int rows) {
    float rp = ci - cj;
    rp = rintf(rp * 100000.0f) * (1.0f / 100000.0f);
    const float t = truncf(((rp + two_w) - 1e-4f) * inv_q);
    const int r = (int)t;
    return min(max(r, 0), rows - 1);
}
__device__ __forceinline__ void st_rel_of(int (&rel)[3], const float *__restrict__ coords, int i, int j, float two_w, float inv_q,
                                          int rows) {
#pragma unroll
    for (int a = 0; a < 3; ++a) rel[a] = st_rel_axis(coords[(long long)i * 3 + a], coords[(long long)j * 3 + a], two_w, inv_q, rows);
}
__device__ __forceinline__ void st_rel_ld(int (&rel)[3], const int *__restrict__ p, long long m, int rows) {
#pragma unroll
    for (int a = 0; a < 3; ++a) rel[a] = min(max(p[m * 3 + a], 0), rows - 1);
}

// ------------------------------------------------------------------------------------------- cells, pairs, rel op ----
__global__ __launch_bounds__(ST_TPB) void st_cells_kernel(int n, const float *__restrict__ coords, const float *__restrict__ start,
                                                          float size, int shift, int *__restrict__ cell, int *__restrict__ wcoord) {
    const int i = blockIdx.x * ST_TPB + threadIdx.x;
    if (i >= n) return;
    const float half = size * 0.5f;  // exact
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = coords[(long long)i * 3 + a], s = start[a];
        // the grid: voxel_grid(coords + shift_size, size, start): ((p + half) - start) / size
        const float g = shift ? (p + half) - s : p - s;
        // :394-406: (coords - coords_min + 1 / 2 * window_size) / window_size
        const float c = shift ? (p - s) + half : p - s;
        if (cell) cell[(long long)i * 3 + a] = (int)truncf(__fdiv_rn(g, size));
        if (wcoord) wcoord[(long long)i * 3 + a] = (int)truncf(__fdiv_rn(c, size));
    }
}

template <bool FILL>
__global__ __launch_bounds__(ST_TPB) void st_pairs_kernel(int n, int nd, const int *__restrict__ order_s, const int *__restrict__ seg_s,
                                                          const int *__restrict__ order_l, const int *__restrict__ seg_l,
                                                          const int *__restrict__ wcoord, int *__restrict__ counts,
                                                          const int *__restrict__ offsets, int m, int *__restrict__ index1) {
    const int i = blockIdx.x * ST_TPB + threadIdx.x;
    if (i >= n) return;
    const int s0 = min(max(seg_s[2 * i], 0), n), s1 = min(max(seg_s[2 * i + 1], s0), n);
    const int l0 = min(max(seg_l[2 * i], 0), nd), l1 = min(max(seg_l[2 * i + 1], l0), nd);
    const int wx = wcoord[(long long)i * 3], wy = wcoord[(long long)i * 3 + 1], wz = wcoord[(long long)i * 3 + 2];
    int pos = FILL ? offsets[i] : 0;
    if (FILL) {
        for (int t = s0; t < s1; ++t, ++pos)
            if ((unsigned)pos < (unsigned)m) index1[pos] = order_s[t];
    } else {
        pos = s1 - s0;
    }
    for (int t = l0; t < l1; ++t) {
        const int j = order_l[t];
        if ((unsigned)j >= (unsigned)n) continue;
        if (wcoord[(long long)j * 3] != wx || wcoord[(long long)j * 3 + 1] != wy || wcoord[(long long)j * 3 + 2] != wz) {
            if (FILL && (unsigned)pos < (unsigned)m) index1[pos] = j;
            ++pos;
        }
    }
    if (!FILL) counts[i] = pos;
}

__global__ __launch_bounds__(ST_TPB) void st_rel_index_kernel(int n, long long m, int rows, const float *__restrict__ coords,
                                                              const int *__restrict__ index0, const int *__restrict__ index1,
                                                              float two_w, float inv_q, int *__restrict__ rel) {
    const long long t = (long long)blockIdx.x * ST_TPB + threadIdx.x;
    if (t >= m) return;
    const int i = index0[t], j = index1[t];
    int r[3] = {0, 0, 0};
    if ((unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n) st_rel_of(r, coords, i, j, two_w, inv_q, rows);
    rel[t * 3] = r[0]; rel[t * 3 + 1] = r[1]; rel[t * 3 + 2] = r[2];
}

// ------------------------------------------------------------------------------------------------- the row kernel ----
constexpr bool st_by_key(int op) {
    return op == ST_OP_STEP1_BWD_K || op == ST_OP_DOT_BWD_K || op == ST_OP_STEP2_BWD_K || op == ST_OP_FUSED_BWD_K;
}
// how many table slices the workgroup accumulates in LDS
constexpr int st_tables(int op) {
    return op == ST_OP_FUSED_BWD_Q ? 2 : (op == ST_OP_DOT_BWD_Q || op == ST_OP_DOT_BWD_K || op == ST_OP_STEP2_BWD_Q || op == ST_OP_FUSED_BWD_K) ? 1 : 0;
}
static size_t st_lds_bytes(int op_tables, int rows, int hd) {
    return sizeof(float) * ((size_t)op_tables * rows * 3 * (hd + 1) + (size_t)ST_ROWS * op_tables * rows * 3);
}

// the score of one pair of the fused attention: q . k + q . tq[rel] + k . tk[rel]
template <int HD>
__device__ __forceinline__ float st_score(const float (&q)[HD], const float (&k)[HD], const float (&tqs)[HD], const float (&tks)[HD]) {
    return (st_dot<HD>(q, k) + st_dot<HD>(q, tqs)) + st_dot<HD>(k, tks);
}

template <int HD, int OP>
__global__ __launch_bounds__(ST_TPB) void st_row_kernel(const st_args a) {
    constexpr bool BYKEY = st_by_key(OP);
    constexpr int NT = st_tables(OP);
    extern __shared__ float st_smem[];
    // `lane` is the lane within the row's group of ST_GROUP lanes, `w` the row's slot in the workgroup
    const int w = threadIdx.x / ST_GROUP, lane = threadIdx.x & (ST_GROUP - 1), hh = blockIdx.y, h = a.h;
    const int L3 = a.rows * 3;
    constexpr int GS = HD + 1;   // words of one (rel, axis) entry of the workgroup's table slice
    float *gT0 = st_smem, *gT1 = st_smem + (NT > 1 ? L3 * GS : 0);
    float *S0 = st_smem + NT * L3 * GS + w * NT * L3, *S1 = S0 + (NT > 1 ? L3 : 0);
    if (NT) {
        for (int e = threadIdx.x; e < NT * L3 * GS; e += ST_TPB) st_smem[e] = 0.f;
        __syncthreads();
    }
    const int *__restrict__ off = BYKEY ? a.t_offsets : a.offsets;

    // every row slot of the workgroup runs the same number of rounds: the table path synchronises the workgroup inside
    for (int base = blockIdx.x * ST_ROWS; base < a.n; base += gridDim.x * ST_ROWS) {
        const int self = base + w;
        const bool live = self < a.n;
        int beg = 0, end = 0;
        if (live) {
            beg = min(max(off[self], 0), a.m);
            end = min(max(off[self + 1], beg), a.m);
        }
        const long long rs = ((long long)(live ? self : 0) * h + hh) * HD;   // this row's vector in an (n, h, hd) array
        const long long rh = (long long)(live ? self : 0) * h + hh;         // ... in an (n, h) array
        if (NT) {
            for (int e = lane; e < NT * L3; e += ST_GROUP) S0[e] = 0.f;
            __syncthreads();
        }
        // the row's own vectors that multiply S0 / S1 when the row's table sums are spread (read again there)
        const float *xp0 = nullptr, *xp1 = nullptr;

        if constexpr (OP == ST_OP_STEP1_FWD || OP == ST_OP_DOT_FWD) {
            float q[HD];
            st_ld<HD>(q, a.q + rs);
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int j = a.index1[t];
                float s = 0.f;
                if ((unsigned)j < (unsigned)a.n) {
                    float k[HD];
                    st_ld<HD>(k, a.k + ((long long)j * h + hh) * HD);
                    if constexpr (OP == ST_OP_STEP1_FWD) {
                        s = st_dot<HD>(q, k);
                    } else {
                        int rel[3];
                        st_rel_ld(rel, a.rel, t, a.rows);
                        float tqs[HD], tks[HD];
                        st_tsum<HD>(tqs, a.tq, h, hh, rel);
                        st_tsum<HD>(tks, a.tk, h, hh, rel);
                        s = st_dot<HD>(q, tqs) + st_dot<HD>(k, tks);
                    }
                }
                a.attn_out[(long long)t * h + hh] = s;
            }
        } else if constexpr (OP == ST_OP_STEP1_BWD_Q || OP == ST_OP_DOT_BWD_Q) {
            float acc[HD];
            st_zero<HD>(acc);
            if constexpr (OP == ST_OP_DOT_BWD_Q) xp0 = a.q + rs;
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int j = a.index1[t];
                if ((unsigned)j >= (unsigned)a.n) continue;
                const float g = a.g_attn[(long long)t * h + hh];
                float y[HD];
                if constexpr (OP == ST_OP_STEP1_BWD_Q) {
                    st_ld<HD>(y, a.k + ((long long)j * h + hh) * HD);
                } else {
                    int rel[3];
                    st_rel_ld(rel, a.rel, t, a.rows);
                    st_tsum<HD>(y, a.tq, h, hh, rel);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) atomicAdd(S0 + rel[ax] * 3 + ax, g);
                }
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(g, y[d], acc[d]);
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = st_group_sum(acc[d]);
            if (live && lane == 0) st_st<HD>(a.gq + rs, acc);
        } else if constexpr (OP == ST_OP_STEP1_BWD_K || OP == ST_OP_DOT_BWD_K || OP == ST_OP_STEP2_BWD_K) {
            float acc[HD];
            st_zero<HD>(acc);
            if constexpr (OP == ST_OP_DOT_BWD_K) xp0 = a.k + rs;
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int i = a.t_query[t], m = a.t_pair[t];
                if ((unsigned)i >= (unsigned)a.n || (unsigned)m >= (unsigned)a.m) continue;
                const float g = OP == ST_OP_STEP2_BWD_K ? a.attn[(long long)m * h + hh] : a.g_attn[(long long)m * h + hh];
                float y[HD];
                if constexpr (OP == ST_OP_STEP1_BWD_K) {
                    st_ld<HD>(y, a.q + ((long long)i * h + hh) * HD);
                } else if constexpr (OP == ST_OP_STEP2_BWD_K) {
                    st_ld<HD>(y, a.g_out + ((long long)i * h + hh) * HD);
                } else {
                    int rel[3];
                    st_rel_ld(rel, a.rel, m, a.rows);
                    st_tsum<HD>(y, a.tk, h, hh, rel);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) atomicAdd(S0 + rel[ax] * 3 + ax, g);
                }
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(g, y[d], acc[d]);
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = st_group_sum(acc[d]);
            if (live && lane == 0) st_st<HD>(OP == ST_OP_STEP2_BWD_K ? a.gv + rs : a.gk + rs, acc);
        } else if constexpr (OP == ST_OP_STEP2_FWD) {
            float acc[HD];
            st_zero<HD>(acc);
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int j = a.index1[t];
                if ((unsigned)j >= (unsigned)a.n) continue;
                const float p = a.attn[(long long)t * h + hh];
                int rel[3];
                st_rel_ld(rel, a.rel, t, a.rows);
                float v[HD], tvs[HD];
                st_ld<HD>(v, a.v + ((long long)j * h + hh) * HD);
                st_tsum<HD>(tvs, a.tv, h, hh, rel);
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(p, v[d] + tvs[d], acc[d]);
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = st_group_sum(acc[d]);
            if (live && lane == 0) st_st<HD>(a.out + rs, acc);
        } else if constexpr (OP == ST_OP_STEP2_BWD_Q) {
            float x0[HD];
            st_ld<HD>(x0, a.g_out + rs);
            xp0 = a.g_out + rs;
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int j = a.index1[t];
                float ga = 0.f;
                if ((unsigned)j < (unsigned)a.n) {
                    int rel[3];
                    st_rel_ld(rel, a.rel, t, a.rows);
                    float v[HD], tvs[HD];
                    st_ld<HD>(v, a.v + ((long long)j * h + hh) * HD);
                    st_tsum<HD>(tvs, a.tv, h, hh, rel);
#pragma unroll
                    for (int d = 0; d < HD; ++d) ga = __builtin_fmaf(x0[d], v[d] + tvs[d], ga);
                    const float p = a.attn[(long long)t * h + hh];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) atomicAdd(S0 + rel[ax] * 3 + ax, p);
                }
                a.attn_out[(long long)t * h + hh] = ga;
            }
        } else if constexpr (OP == ST_OP_SOFTMAX_FWD) {
            float mx = -INFINITY;
            for (int t = beg + lane; t < end; t += ST_GROUP) mx = fmaxf(mx, a.attn[(long long)t * h + hh]);
            mx = st_group_max(mx);
            float l = 0.f;
            for (int t = beg + lane; t < end; t += ST_GROUP) l += expf(a.attn[(long long)t * h + hh] - mx);
            l = st_group_sum(l);
            for (int t = beg + lane; t < end; t += ST_GROUP)
                a.attn_out[(long long)t * h + hh] = expf(a.attn[(long long)t * h + hh] - mx) / l;
        } else if constexpr (OP == ST_OP_SOFTMAX_BWD) {
            float s = 0.f;
            for (int t = beg + lane; t < end; t += ST_GROUP)
                s = __builtin_fmaf(a.attn[(long long)t * h + hh], a.g_attn[(long long)t * h + hh], s);
            s = st_group_sum(s);
            for (int t = beg + lane; t < end; t += ST_GROUP)
                a.attn_out[(long long)t * h + hh] = a.attn[(long long)t * h + hh] * (a.g_attn[(long long)t * h + hh] - s);
        } else if constexpr (OP == ST_OP_FUSED_FWD) {
            float q[HD], acc[HD];
            st_ld<HD>(q, a.q + rs);
            st_zero<HD>(acc);
            float mx = -INFINITY, l = 0.f;
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int j = a.index1[t];
                if ((unsigned)j >= (unsigned)a.n) continue;
                int rel[3];
                st_rel_of(rel, a.coords, self, j, a.two_w, a.inv_q, a.rows);
                float k[HD], tqs[HD], tks[HD];
                st_ld<HD>(k, a.k + ((long long)j * h + hh) * HD);
                st_tsum<HD>(tqs, a.tq, h, hh, rel);
                st_tsum<HD>(tks, a.tk, h, hh, rel);
                const float s = st_score<HD>(q, k, tqs, tks);
                const float nm = fmaxf(mx, s);
                const float sc = expf(mx - nm), p = expf(s - nm);   // the first pair: exp(-inf) = 0
                float v[HD], tvs[HD];
                st_ld<HD>(v, a.v + ((long long)j * h + hh) * HD);
                st_tsum<HD>(tvs, a.tv, h, hh, rel);
                l = __builtin_fmaf(l, sc, p);
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(acc[d], sc, p * (v[d] + tvs[d]));
                mx = nm;
            }
            const float wm = st_group_max(mx);
            const float f = (mx == -INFINITY) ? 0.f : expf(mx - wm);   // a lane without a pair
            l = st_group_sum(l * f);
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = st_group_sum(acc[d] * f);
            if (live && lane == 0) {
                const float inv = l > 0.f ? 1.0f / l : 0.f;   // a row without a pair: zeros
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] *= inv;
                st_st<HD>(a.out + rs, acc);
                a.lse_out[rh] = l > 0.f ? wm + logf(l) : 0.f;
            }
        } else if constexpr (OP == ST_OP_FUSED_BWD_Q) {
            float q[HD], x1[HD], acc[HD];
            st_ld<HD>(q, a.q + rs);
            st_ld<HD>(x1, a.g_out + rs);
            xp0 = a.q + rs;
            xp1 = a.g_out + rs;
            st_zero<HD>(acc);
            const float lse = live ? a.lse[rh] : 0.f, delta = live ? a.delta[rh] : 0.f;
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int j = a.index1[t];
                if ((unsigned)j >= (unsigned)a.n) continue;
                int rel[3];
                st_rel_of(rel, a.coords, self, j, a.two_w, a.inv_q, a.rows);
                float k[HD], tqs[HD], tks[HD];
                st_ld<HD>(k, a.k + ((long long)j * h + hh) * HD);
                st_tsum<HD>(tqs, a.tq, h, hh, rel);
                st_tsum<HD>(tks, a.tk, h, hh, rel);
                const float p = expf(st_score<HD>(q, k, tqs, tks) - lse);
                float v[HD], tvs[HD];
                st_ld<HD>(v, a.v + ((long long)j * h + hh) * HD);
                st_tsum<HD>(tvs, a.tv, h, hh, rel);
                float dp = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) dp = __builtin_fmaf(x1[d], v[d] + tvs[d], dp);
                const float ds = p * (dp - delta);
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] = __builtin_fmaf(ds, k[d] + tqs[d], acc[d]);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    atomicAdd(S0 + rel[ax] * 3 + ax, ds);
                    atomicAdd(S1 + rel[ax] * 3 + ax, p);
                }
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = st_group_sum(acc[d]);
            if (live && lane == 0) st_st<HD>(a.gq + rs, acc);
        } else if constexpr (OP == ST_OP_FUSED_BWD_K) {
            float k[HD], v[HD], gk[HD], gv[HD];
            st_ld<HD>(k, a.k + rs);
            st_ld<HD>(v, a.v + rs);
            xp0 = a.k + rs;
            st_zero<HD>(gk); st_zero<HD>(gv);
            for (int t = beg + lane; t < end; t += ST_GROUP) {
                const int i = a.t_query[t];
                if ((unsigned)i >= (unsigned)a.n) continue;
                int rel[3];
                st_rel_of(rel, a.coords, i, self, a.two_w, a.inv_q, a.rows);
                const long long ri = ((long long)i * h + hh) * HD;
                float q[HD], go[HD], tqs[HD], tks[HD], tvs[HD];
                st_ld<HD>(q, a.q + ri);
                st_ld<HD>(go, a.g_out + ri);
                st_tsum<HD>(tqs, a.tq, h, hh, rel);
                st_tsum<HD>(tks, a.tk, h, hh, rel);
                st_tsum<HD>(tvs, a.tv, h, hh, rel);
                const float p = expf(st_score<HD>(q, k, tqs, tks) - a.lse[(long long)i * h + hh]);
                float dp = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) dp = __builtin_fmaf(go[d], v[d] + tvs[d], dp);
                const float ds = p * (dp - a.delta[(long long)i * h + hh]);
#pragma unroll
                for (int d = 0; d < HD; ++d) {
                    gk[d] = __builtin_fmaf(ds, q[d] + tks[d], gk[d]);
                    gv[d] = __builtin_fmaf(p, go[d], gv[d]);
                }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) atomicAdd(S0 + rel[ax] * 3 + ax, ds);
            }
#pragma unroll
            for (int d = 0; d < HD; ++d) { gk[d] = st_group_sum(gk[d]); gv[d] = st_group_sum(gv[d]); }
            if (live && lane == 0) { st_st<HD>(a.gk + rs, gk); st_st<HD>(a.gv + rs, gv); }
        }

        if (NT) {
            // spread the row's sums per (rel, axis) over the channels: gT[rel, axis, :] += S[rel, axis] * x[:], a lane per entry.
            // The slice is kept with a stride of HD + 1 words per entry, so that the lanes' atomics fall on distinct banks
            __syncthreads();
            float x0[HD], x1[HD];
            st_ld<HD>(x0, xp0);
            st_ld<HD>(x1, NT > 1 ? xp1 : xp0);
            for (int e = lane; e < L3; e += ST_GROUP) {
                const float s0 = S0[e];
                if (s0 != 0.f) {
#pragma unroll
                    for (int d = 0; d < HD; ++d) atomicAdd(gT0 + e * GS + d, s0 * x0[d]);
                }
                if (NT > 1) {
                    const float s1 = S1[e];
                    if (s1 != 0.f) {
#pragma unroll
                        for (int d = 0; d < HD; ++d) atomicAdd(gT1 + e * GS + d, s1 * x1[d]);
                    }
                }
            }
        }
    }

    if (NT) {
        __syncthreads();
        float *g0 = OP == ST_OP_DOT_BWD_Q || OP == ST_OP_FUSED_BWD_Q ? a.gtq : OP == ST_OP_STEP2_BWD_Q ? a.gtv : a.gtk;
        float *g1 = a.gtv;
        for (int t = threadIdx.x; t < L3 * HD; t += ST_TPB) {
            const int ent = t / HD, d = t % HD;   // ent = rel * 3 + axis
            const long long at = (((long long)(ent / 3) * h + hh) * 3 + ent % 3) * HD + d;
            const float v0 = gT0[ent * GS + d];
            if (v0 != 0.f) unsafeAtomicAdd(g0 + at, v0);
            if (NT > 1) {
                const float v1 = gT1[ent * GS + d];
                if (v1 != 0.f) unsafeAtomicAdd(g1 + at, v1);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ launchers ----
extern "C" int ptv2_st_abi_version(void) { return 1; }
extern "C" int ptv2_st_struct_bytes(int which) { return which == 0 ? (int)sizeof(st_args) : -1; }

template <int HD, int OP>
static int st_launch(const st_args &a, hipStream_t st) {
    const size_t lds = st_lds_bytes(st_tables(OP), a.rows, HD);
    if (lds > ST_MAX_LDS) return PTV2_ERR_ARG;
    // table operators: long-lived workgroups, because every workgroup ends by adding its whole table slice to memory with atomics
    // (128 and 1024 per head measured the same within 1 % at 30 000 points); the others: one round per workgroup
    const int rounds = divup(a.n, ST_ROWS);
    const int gx = st_tables(OP) ? min(rounds, 1024) : rounds;
    hipLaunchKernelGGL((st_row_kernel<HD, OP>), dim3(gx, a.h), dim3(ST_TPB), lds, st, a);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

template <int HD>
static int st_dispatch(int op, const st_args &a, hipStream_t st) {
    switch (op) {
    case ST_OP_STEP1_FWD: return st_launch<HD, ST_OP_STEP1_FWD>(a, st);
    case ST_OP_STEP1_BWD_Q: return st_launch<HD, ST_OP_STEP1_BWD_Q>(a, st);
    case ST_OP_STEP1_BWD_K: return st_launch<HD, ST_OP_STEP1_BWD_K>(a, st);
    case ST_OP_DOT_FWD: return st_launch<HD, ST_OP_DOT_FWD>(a, st);
    case ST_OP_DOT_BWD_Q: return st_launch<HD, ST_OP_DOT_BWD_Q>(a, st);
    case ST_OP_DOT_BWD_K: return st_launch<HD, ST_OP_DOT_BWD_K>(a, st);
    case ST_OP_STEP2_FWD: return st_launch<HD, ST_OP_STEP2_FWD>(a, st);
    case ST_OP_STEP2_BWD_Q: return st_launch<HD, ST_OP_STEP2_BWD_Q>(a, st);
    case ST_OP_STEP2_BWD_K: return st_launch<HD, ST_OP_STEP2_BWD_K>(a, st);
    case ST_OP_SOFTMAX_FWD: return st_launch<HD, ST_OP_SOFTMAX_FWD>(a, st);
    case ST_OP_SOFTMAX_BWD: return st_launch<HD, ST_OP_SOFTMAX_BWD>(a, st);
    case ST_OP_FUSED_FWD: return st_launch<HD, ST_OP_FUSED_FWD>(a, st);
    case ST_OP_FUSED_BWD_Q: return st_launch<HD, ST_OP_FUSED_BWD_Q>(a, st);
    case ST_OP_FUSED_BWD_K: return st_launch<HD, ST_OP_FUSED_BWD_K>(a, st);
    }
    return PTV2_ERR_ARG;
}

// the operands an operator reads or writes must be there
static bool st_has(int op, const st_args &a) {
    const bool q_csr = a.offsets && a.index1, k_csr = a.t_offsets && a.t_query && a.t_pair;
    switch (op) {
    case ST_OP_STEP1_FWD: return q_csr && a.q && a.k && a.attn_out;
    case ST_OP_STEP1_BWD_Q: return q_csr && a.k && a.g_attn && a.gq;
    case ST_OP_STEP1_BWD_K: return k_csr && a.q && a.g_attn && a.gk;
    case ST_OP_DOT_FWD: return q_csr && a.rel && a.q && a.k && a.tq && a.tk && a.attn_out;
    case ST_OP_DOT_BWD_Q: return q_csr && a.rel && a.q && a.tq && a.g_attn && a.gq && a.gtq;
    case ST_OP_DOT_BWD_K: return k_csr && a.rel && a.k && a.tk && a.g_attn && a.gk && a.gtk;
    case ST_OP_STEP2_FWD: return q_csr && a.rel && a.attn && a.v && a.tv && a.out;
    case ST_OP_STEP2_BWD_Q: return q_csr && a.rel && a.attn && a.v && a.tv && a.g_out && a.attn_out && a.gtv;
    case ST_OP_STEP2_BWD_K: return k_csr && a.attn && a.g_out && a.gv;
    case ST_OP_SOFTMAX_FWD: return a.offsets && a.attn && a.attn_out;
    case ST_OP_SOFTMAX_BWD: return a.offsets && a.attn && a.g_attn && a.attn_out;
    case ST_OP_FUSED_FWD: return q_csr && a.coords && a.q && a.k && a.v && a.tq && a.tk && a.tv && a.out && a.lse_out;
    case ST_OP_FUSED_BWD_Q:
        return q_csr && a.coords && a.q && a.k && a.v && a.tq && a.tk && a.tv && a.g_out && a.lse && a.delta && a.gq && a.gtq && a.gtv;
    case ST_OP_FUSED_BWD_K:
        return a.t_offsets && a.t_query && a.coords && a.q && a.k && a.v && a.tq && a.tk && a.tv && a.g_out && a.lse && a.delta &&
               a.gk && a.gv && a.gtk;
    }
    return false;
}

extern "C" int st_op_hip_launcher(int op, const st_args *args, void *stream) {
    if (!args || op < 0 || op >= ST_OP_COUNT) return PTV2_ERR_ARG;
    const st_args &a = *args;
    if (a.n < 0 || a.m < 0 || a.h < 1 || a.h > ST_MAX_HEADS || (a.hd != 16 && a.hd != 32) || a.rows < 1 || a.rows > ST_MAX_TABLE_ROWS)
        return PTV2_ERR_ARG;
    if (!st_has(op, a)) return PTV2_ERR_ARG;
    if (a.n == 0) return PTV2_OK;
    hipStream_t st = (hipStream_t)stream;
    return a.hd == 16 ? st_dispatch<16>(op, a, st) : st_dispatch<32>(op, a, st);
}

extern "C" int st_cells_hip_launcher(int n, const float *coords, const float *start, float size, int shift, int *cell, int *wcoord,
                                     void *stream) {
    if (n < 0 || !coords || !start || !(size > 0.f) || (shift != 0 && shift != 1) || (!cell && !wcoord)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    hipLaunchKernelGGL(st_cells_kernel, dim3(divup(n, ST_TPB)), dim3(ST_TPB), 0, (hipStream_t)stream, n, coords, start, size, shift,
                       cell, wcoord);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int st_pairs_hip_launcher(int n, int nd, int fill, const int *order_s, const int *seg_s, const int *order_l,
                                     const int *seg_l, const int *wcoord, int *counts, const int *offsets, int m, int *index1,
                                     void *stream) {
    if (n < 0 || nd < 0 || !order_s || !seg_s || !seg_l || !wcoord || (nd > 0 && !order_l)) return PTV2_ERR_ARG;
    if (fill ? (!offsets || m < 0 || (m > 0 && !index1)) : !counts) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (fill)
        hipLaunchKernelGGL(st_pairs_kernel<true>, dim3(divup(n, ST_TPB)), dim3(ST_TPB), 0, (hipStream_t)stream, n, nd, order_s, seg_s,
                           order_l, seg_l, wcoord, counts, offsets, m, index1);
    else
        hipLaunchKernelGGL(st_pairs_kernel<false>, dim3(divup(n, ST_TPB)), dim3(ST_TPB), 0, (hipStream_t)stream, n, nd, order_s, seg_s,
                           order_l, seg_l, wcoord, counts, offsets, m, index1);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int st_rel_index_hip_launcher(int n, long long m, int rows, const float *coords, const int *index0, const int *index1,
                                         float two_w, float inv_q, int *rel, void *stream) {
    if (n < 0 || m < 0 || rows < 1 || !coords || (m > 0 && (!index0 || !index1 || !rel))) return PTV2_ERR_ARG;
    if (m == 0) return PTV2_OK;
    hipLaunchKernelGGL(st_rel_index_kernel, dim3(divup(m, ST_TPB)), dim3(ST_TPB), 0, (hipStream_t)stream, n, m, rows, coords, index0,
                       index1, two_w, inv_q, rel);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
