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
#include "swin_core.h"

#define SWIN_FWD_MAX_BLOCKS 1024

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

// the backward is stated in swin_core.h, shared with the half-storage unit
template <int HD, int S>
__global__ __launch_bounds__(SWIN_TPB) void swin_attn_bwd_kernel(swin_args a, int chunks, float *delta, float *part) {
    SWIN_BWD_KERNEL_BODY(false)
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

int swin_table_reduce(int chunks, int R, int H, int hd, const float *part, float *gq, float *gk, float *gv, void *stream) {
    hipLaunchKernelGGL(swin_table_reduce_kernel, dim3(divup(3LL * R * H * hd, SWIN_TPB)), dim3(SWIN_TPB), 0, (hipStream_t)stream, chunks, R, H,
                       hd, part, gq, gk, gv);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int ptv2_swin_abi_version(void) { return 1; }
extern "C" int ptv2_swin_struct_bytes(int which) { return which == 0 ? (int)sizeof(swin_args) : -1; }

extern "C" long long ptv2_swin_workspace_bytes(int n, int windows, int h, int hd, int table_rows) {
    return swin_bwd_workspace_bytes(n, windows, h, hd, table_rows);
}

static int swin_attention_check(const swin_args *a) {
    if (!a || a->groups < 1 || a->groups > SWIN_MAX_GROUPS) return PTV2_ERR_ARG;
    for (int s = 0; s < a->groups; ++s)
        if (a->rows[s] < 1 || a->rows[s] > SWIN_MAX_ROWS) return PTV2_ERR_ARG;
    if (!swin_shape_ok(a->n, a->windows, a->h, a->hd, swin_table_rows(*a)) || a->c != a->h * a->hd) return PTV2_ERR_ARG;
    if (!a->order || !a->offsets || !a->signals || !a->qkv || !a->q_table || !a->k_table || !a->v_table || !a->out || !a->lse) return PTV2_ERR_ARG;
    return PTV2_OK;
}

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
    return swin_table_reduce(chunks, R, a.h, a.hd, part, a.g_q_table, a.g_k_table, a.g_v_table, stream);
}
