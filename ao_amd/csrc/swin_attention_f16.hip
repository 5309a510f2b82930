// ao_amd/csrc/swin_attention_f16.hip -- Swin3D's window attention with cRSE on half-precision storage: the reference's
// fp16_mode 1, "fp16 forward and fp32 backward" (include/ptv2_swin_f16_hip.h).  gfx950 only.
//
// The forward keeps the decomposition of swin_attention.hip -- a workgroup of four wavefronts per head and chunk of windows,
// strips of 16 members dealt to the wavefronts, an online softmax per lane, P in registers -- and differs where the type moves
// the trade-offs:
//   * the three table slices are staged as HALF: 3 R hd halves, 34.5 KB at R = 360, hd = 16 against 69 KB, converted on the fly
//     from the strided fp32 (R, h, hd) parameter (two 128-bit reads, one 128-bit LDS write per thread and step); no half copy
//     of a table exists in memory.  A row of a slice is hd / 8 128-bit LDS reads, widened and summed in fp32 registers.  Four
//     workgroups fit a compute unit where two did, and the grid is sized from ptv2_resident_blocks for THIS footprint;
//   * the q . k tile is ONE V_MFMA_F32_16X16X16_F16 per 16 x 16 tile: lane l supplies four contiguous halves of its row at
//     contraction index 4 (l / 16), one 8-byte load through `order`, for the other side's member l % 16 as A and its own member
//     l % 16 as B; at hd = 8 the lanes with l / 16 >= 2 supply zeros.  The products of halves are exact in fp32 and the
//     instruction accumulates in fp32.  The accumulator layout is that of the fp32 16x16x4 tile: lane l holds own member l % 16
//     against the others 4 (l / 16) + r, so everything behind the tile is laid out as in swin_attention.hip.  scale multiplies
//     the tile's result, in fp32, and the fp32 q that meets T_Q: q is never rounded a second time;
//   * the per-pair k and v rows are 16 or 32 bytes, widened in registers; out is rounded once, in its 16-byte stores.
// The backward is the body and the strip routine of swin_core.h over _Float16: the fp32 routine with half loads and stores and
// the staged table values rounded to half and widened (it differentiates the function this forward computes).  Its six slices
// stay fp32.
#include "swin_core.h"
#include "../../include/ptv2_swin_f16_hip.h"

static_assert(SWIN_F16_MAX_GROUPS == SWIN_MAX_GROUPS, "ptv2_swin_f16_hip.h restates the constant of ptv2_swin_hip.h");

// four workgroups per compute unit at the largest footprint, eight at hd = 8
#define SWIN_F16_FWD_MAX_BLOCKS 2048

// what the kernels take: swin_f16_args with its half pointers typed (the field names are those of swin_args: swin_core.h)
struct swin_h_view {
    int n, windows, c, h, hd, groups;
    int rows[SWIN_MAX_GROUPS];
    float scale;
    const int *order, *offsets;
    const float *signals;
    const _Float16 *qkv;
    const float *q_table, *k_table, *v_table;
    const _Float16 *g_out;
    _Float16 *out;
    float *lse;
    _Float16 *g_qkv;
};

__device__ __forceinline__ v4f mfma16h(v4h a, v4h b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }

// the head's (R, hd) slice of a fp32 (R, h, hd) table, as half: each value rounded once, to nearest even
template <int HD>
__device__ __forceinline__ void swin_stage_half(_Float16 *slice, const float *table, int R, int H, int h) {
    for (int e = threadIdx.x * 8; e < R * HD; e += SWIN_TPB * 8) {
        const float *src = table + ((size_t)(e / HD) * H + h) * HD + e % HD;
        const float4 lo = *(const float4 *)src, hi = *(const float4 *)(src + 4);
        const v8h v = {(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w,
                       (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
        *(v8h *)(slice + e) = v;
    }
}

// t = the sum of the pair's D rows of one half slice, in fp32
template <int HD, int D>
__device__ __forceinline__ void swin_row_sum(float (&t)[HD], const _Float16 *slice, const int (&idx)[D]) {
#pragma unroll
    for (int e = 0; e < HD; ++e) t[e] = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const v8h *row = (const v8h *)(slice + idx[d] * HD);
#pragma unroll
        for (int e = 0; e < HD / 8; ++e) {
            const v8h v = row[e];
#pragma unroll
            for (int i = 0; i < 8; ++i) t[8 * e + i] += (float)v[i];
        }
    }
}

// the lane's operand of the tile: halves [4 g, 4 g + 4) of a row of hd, zeros past hd
template <int HD>
__device__ __forceinline__ v4h swin_tile_operand(const _Float16 *row, int g) {
    const v4h zero = {0, 0, 0, 0};
    return 4 * g < HD ? *(const v4h *)(row + 4 * g) : zero;
}

template <int HD, int S>
__global__ __launch_bounds__(SWIN_TPB) void swin_attn_f16_fwd_kernel(swin_h_view a, int chunks) {
    constexpr int D = 3 * S;
    extern __shared__ float4 swin_smem[];
    const int R = swin_table_rows(a), h = blockIdx.x % a.h, chunk = blockIdx.x / a.h;
    _Float16 *tq = (_Float16 *)swin_smem, *tk = tq + R * HD, *tv = tk + R * HD;
    swin_stage_half<HD>(tq, a.q_table, R, a.h, h);
    swin_stage_half<HD>(tk, a.k_table, R, a.h, h);
    swin_stage_half<HD>(tv, a.v_table, R, a.h, h);
    __syncthreads();
    const SwinAxes<D> axes(a);
    const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), x = lane & 15, g = lane >> 4;
    const size_t c3 = 3 * (size_t)a.c;
    const _Float16 *q_h = a.qkv + h * HD, *k_h = q_h + a.c, *v_h = k_h + a.c;
    const int w1 = swin_chunk_start(a.windows, chunks, chunk + 1);
    int item = 0;
    for (int w = swin_chunk_start(a.windows, chunks, chunk); w < w1; ++w) {
        const int base = a.offsets[w], m = a.offsets[w + 1] - base;
        for (int s0 = 0; s0 < m; s0 += SWIN_TILE, ++item) {
            if (item % SWIN_WAVES != wave) continue;
            const bool own = s0 + x < m;
            const int pi = base + min(s0 + x, m - 1), ni = a.order[pi];
            float q[HD], si[D];
            swin_ld(q, q_h + ni * c3, a.scale);
            const v4h qb = swin_tile_operand<HD>(q_h + ni * c3, g);
            swin_signals(si, a.signals, pi);
            float top = -FLT_MAX, sum = 0.f, acc[HD];
#pragma unroll
            for (int e = 0; e < HD; ++e) acc[e] = 0.f;
            for (int t0 = 0; t0 < m; t0 += SWIN_TILE) {
                const v4h ka = swin_tile_operand<HD>(k_h + a.order[base + min(t0 + x, m - 1)] * c3, g);
                const v4f s = mfma16h(ka, qb, v4f{0.f, 0.f, 0.f, 0.f});   // s[r]: key t0 + 4 g + r against the lane's query, unscaled
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
                    float e_ij = a.scale * s[r] + swin_dot(q, t);
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

template <int HD, int S>
__global__ __launch_bounds__(SWIN_TPB) void swin_attn_f16_bwd_kernel(swin_h_view a, int chunks, float *delta, float *part) {
    SWIN_BWD_KERNEL_BODY(true)
}

extern "C" int ptv2_swin_f16_abi_version(void) { return 1; }
extern "C" int ptv2_swin_f16_struct_bytes(int which) { return which == 0 ? (int)sizeof(swin_f16_args) : -1; }

extern "C" long long ptv2_swin_f16_workspace_bytes(int n, int windows, int h, int hd, int table_rows) {
    return swin_bwd_workspace_bytes(n, windows, h, hd, table_rows);
}

// PTV2_OK and the kernels' view of the operands, or PTV2_ERR_ARG
static int swin_f16_view(const swin_f16_args *p, swin_h_view *v) {
    if (!p || p->groups < 1 || p->groups > SWIN_MAX_GROUPS) return PTV2_ERR_ARG;
    for (int s = 0; s < p->groups; ++s)
        if (p->rows[s] < 1 || p->rows[s] > SWIN_MAX_ROWS) return PTV2_ERR_ARG;
    if (!swin_shape_ok(p->n, p->windows, p->h, p->hd, swin_table_rows(*p)) || p->c != p->h * p->hd) return PTV2_ERR_ARG;
    if (!p->order || !p->offsets || !p->signals || !p->qkv || !p->q_table || !p->k_table || !p->v_table || !p->out || !p->lse) return PTV2_ERR_ARG;
    *v = swin_h_view{p->n, p->windows, p->c, p->h, p->hd, p->groups, {p->rows[0], p->rows[1], p->rows[2]}, p->scale, p->order, p->offsets,
                     p->signals, (const _Float16 *)p->qkv, p->q_table, p->k_table, p->v_table, (const _Float16 *)p->g_out,
                     (_Float16 *)p->out, p->lse, (_Float16 *)p->g_qkv};
    return PTV2_OK;
}

// the forward kernel of (a.hd, a.groups) and the workgroups of it that the device holds with `lds` bytes each
static int swin_f16_fwd_kernel_of(const swin_h_view &a, size_t lds, const void **kern, int *resident) {
#define SWIN_FWD(HD, S)                                              \
    {                                                                \
        *kern = (const void *)swin_attn_f16_fwd_kernel<HD, S>;       \
        RUN(ptv2_kernel_lds(*kern, lds));                            \
        *resident = ptv2_resident_blocks(*kern, SWIN_TPB, lds, 1);   \
    }
    SWIN_DISPATCH(SWIN_FWD);
#undef SWIN_FWD
    return PTV2_OK;
}

extern "C" int ptv2_swin_f16_fwd_resident_blocks(int hd, int groups, int table_rows) {
    if ((hd != 8 && hd != 16) || groups < 1 || groups > SWIN_MAX_GROUPS || table_rows < 6 || table_rows > SWIN_MAX_ROWS) return -1;
    swin_h_view a{};
    a.hd = hd; a.groups = groups;
    const void *kern;
    int resident = 0;
    return swin_f16_fwd_kernel_of(a, sizeof(_Float16) * swin_part_floats(table_rows, hd), &kern, &resident) == PTV2_OK ? resident : -1;
}

extern "C" int swin_attention_f16_fwd_hip_launcher(const swin_f16_args *args, void *stream) {
    swin_h_view a;
    RUN(swin_f16_view(args, &a));
    const size_t lds = sizeof(_Float16) * swin_part_floats(swin_table_rows(a), a.hd);
    const void *kern;
    int resident = 0;
    RUN(swin_f16_fwd_kernel_of(a, lds, &kern, &resident));
    const int chunks = swin_chunks(a.windows, a.h, std::min(resident, SWIN_F16_FWD_MAX_BLOCKS));
    void *params[] = {(void *)&a, (void *)&chunks};
    if (hipLaunchKernel(kern, dim3(a.h * chunks), dim3(SWIN_TPB), params, lds, (hipStream_t)stream) != hipSuccess) return PTV2_ERR_LAUNCH;
    return PTV2_OK;
}

extern "C" int swin_attention_f16_bwd_hip_launcher(const swin_f16_args *args, void *stream) {
    swin_h_view a;
    RUN(swin_f16_view(args, &a));
    if (!a.g_out || !a.g_qkv || !args->g_q_table || !args->g_k_table || !args->g_v_table || !args->workspace) return PTV2_ERR_ARG;
    const int R = swin_table_rows(a);
    if (args->workspace_bytes < swin_bwd_workspace_bytes(a.n, a.windows, a.h, a.hd, R)) return PTV2_ERR_WORKSPACE;
    PtvCarver ws{(char *)args->workspace, 0};
    float *delta = ws.take_n<float>((size_t)a.n * a.h), *part = (float *)ws.take(0);
    const size_t lds = 2 * sizeof(float) * swin_part_floats(R, a.hd);
    int chunks = 0;
#define SWIN_BWD(HD, S)                                                                                                          \
    {                                                                                                                            \
        const void *kern = (const void *)swin_attn_f16_bwd_kernel<HD, S>;                                                        \
        RUN(ptv2_kernel_lds(kern, lds));                                                                                         \
        chunks = swin_chunks(a.windows, a.h, std::min(ptv2_resident_blocks(kern, SWIN_TPB, lds, 1), SWIN_BWD_MAX_BLOCKS));       \
        hipLaunchKernelGGL((swin_attn_f16_bwd_kernel<HD, S>), dim3(a.h * chunks), dim3(SWIN_TPB), lds, (hipStream_t)stream, a, chunks, delta, part); \
    }
    SWIN_DISPATCH(SWIN_BWD);
#undef SWIN_BWD
    PTV2_CHECK_LAUNCH();
    return swin_table_reduce(chunks, R, a.h, a.hd, part, args->g_q_table, args->g_k_table, args->g_v_table, stream);
}
