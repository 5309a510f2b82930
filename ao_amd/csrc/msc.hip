// ao_amd/csrc/msc.hip -- Masked Scene Contrast (MSC-v1m1) for gfx950 (MI355X); C ABI include/ptv2_msc_hip.h.
//
// Replaces three eager stretches of masked_scene_contrast_v1m1_base.py:
//
//   InfoNCE    sim = A B^T (m x m fp32, 256 MB at m = 8192), its division by t, its log-softmax and their gradients, with
//              tiles of 64 x 64 on v_mfma_f32_32x32x2_f32 that are never stored.  Forward: gather + normalise (one wavefront
//              per pair), row logsumexp per (64 rows, split of the columns) with a (max, sum) per lane and accumulator register,
//              combined over lanes, waves and splits in a fixed order, then one finishing block.  Backward: every tile is
//              recomputed from A, B and lse; a workgroup owns 64 rows of dA (blockIdx.y = 0) or of dB (blockIdx.y = 1), turns
//              the tile into P - I in LDS and multiplies it into its accumulators, so nothing is added across workgroups.  The
//              normalisation's backward and the scatter run per index: one wavefront sums the rows of a run of a stable sort;
//   matching   one thread per view-1 row over its k neighbours;
//   patch ids  one thread per point of either view.
//
// The tile, the gather + normalise kernel and the normalisation's backward live in msc_tile.h, shared with msc_csc.hip.
// Compiled with -ffp-contract=off (Makefile): the patch ids divide in IEEE fp32, one rounding per statement.
#include "msc_tile.h"
#include "../../include/ptv2_msc_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------- row logsumexp ----
// part (nsplit, m, 2): (max, sum of exp(S - max)) of row i over the columns of split blockIdx.y.  FIXED: rows are unit vectors,
// so |S| <= 1 / t, and the shift is the constant 1 / t (the launcher chooses it where exp(-2 / t) is a normal fp32 number).
template <bool FIXED>
__global__ __launch_bounds__(TPB) void msc_lse_kernel(int m, int c, const float *__restrict__ A, const float *__restrict__ B,
                                                      float inv_t, int chunks_per_split, float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sX[TILE][KP];
    __shared__ __attribute__((aligned(16))) float sY[TILE][KP];
    __shared__ float sM[2][2][32], sS[2][2][32];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int rt = wave >> 1, ct = wave & 1;
    const int x0 = blockIdx.x * TILE;
    const int nchunks = (m + TILE - 1) / TILE;
    const int ch_lo = blockIdx.y * chunks_per_split, ch_hi = min(nchunks, ch_lo + chunks_per_split);
    float mx[16], sm[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { mx[e] = FIXED ? inv_t : -FLT_MAX; sm[e] = 0.f; }
    for (int ch = ch_lo; ch < ch_hi; ++ch) {
        const int y0 = ch * TILE;
        const v16f acc = s_tile(A, x0, B, y0, m, c, sX, sY, rt, ct);
        if (y0 + 32 * ct + r < m) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float x = acc[e] * inv_t;
                if (FIXED) {
                    sm[e] += expf(x - inv_t);
                } else {
                    const float nm = fmaxf(mx[e], x);
                    sm[e] = sm[e] * expf(mx[e] - nm) + expf(x - nm);
                    mx[e] = nm;
                }
            }
        }
    }
    // the 32 lanes of a half hold the 32 columns of the same 16 rows
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        for (int o = 1; o < 32; o <<= 1) {
            const float om = __shfl_xor(mx[e], o), os = __shfl_xor(sm[e], o);
            if (FIXED) {
                sm[e] += os;
            } else {
                // (both partners must take the same operand order: the lower lane's pair comes first)
                float m1 = (lane & o) ? om : mx[e], s1 = (lane & o) ? os : sm[e];
                const float m2 = (lane & o) ? mx[e] : om, s2 = (lane & o) ? sm[e] : os;
                lse_merge(m1, s1, m2, s2);
                mx[e] = m1; sm[e] = s1;
            }
        }
        if (r == 0) {
            sM[rt][ct][acc_row(e, h)] = mx[e];
            sS[rt][ct][acc_row(e, h)] = sm[e];
        }
    }
    __syncthreads();
    if (tid < TILE && x0 + tid < m) {
        float m1 = sM[tid >> 5][0][tid & 31], s1 = sS[tid >> 5][0][tid & 31];
        if (FIXED) s1 += sS[tid >> 5][1][tid & 31];
        else lse_merge(m1, s1, sM[tid >> 5][1][tid & 31], sS[tid >> 5][1][tid & 31]);
        float *dst = part + 2 * ((size_t)blockIdx.y * m + x0 + tid);
        dst[0] = m1;
        dst[1] = s1;
    }
}

// column sums of A and B over the 64 rows of a workgroup: colpart (nblocks, 2, c) fp64
__global__ __launch_bounds__(TPB) void msc_colsum_kernel(int m, int c, const float *__restrict__ A, const float *__restrict__ B,
                                                         double *__restrict__ colpart) {
    const int ch = threadIdx.x;
    if (ch >= c) return;
    const int lo = blockIdx.x * TILE, hi = min(m, lo + TILE);
    double sa = 0.0, sb = 0.0;
    for (int i = lo; i < hi; ++i) {
        sa += (double)A[(size_t)i * c + ch];
        sb += (double)B[(size_t)i * c + ch];
    }
    colpart[((size_t)blockIdx.x * 2 + 0) * c + ch] = sa;
    colpart[((size_t)blockIdx.x * 2 + 1) * c + ch] = sb;
}

// One workgroup: the splits of a row in split order -> lse; the three scalars, every sum in a fixed order (fp64 accumulators).
__global__ __launch_bounds__(TPB) void msc_nce_finish_kernel(int m, int c, int nsplit, int nblocks, float t,
                                                             const float *__restrict__ part, const float *__restrict__ pos,
                                                             const double *__restrict__ colpart, const int *__restrict__ status,
                                                             float *__restrict__ lse, float *__restrict__ out) {
    __shared__ double sh[TPB];
    const int tid = threadIdx.x;
    double loss = 0.0, ps = 0.0;
    for (int i = tid; i < m; i += TPB) {
        float m1 = part[2 * (size_t)i], s1 = part[2 * (size_t)i + 1];
        for (int s = 1; s < nsplit; ++s) lse_merge(m1, s1, part[2 * ((size_t)s * m + i)], part[2 * ((size_t)s * m + i) + 1]);
        const float l = m1 + logf(s1);
        lse[i] = l;
        loss += (double)(l - pos[i] / t);
        ps += (double)pos[i];
    }
    double dot = 0.0;
    if (tid < c) {
        double sa = 0.0, sb = 0.0;
        for (int b = 0; b < nblocks; ++b) {
            sa += colpart[((size_t)b * 2 + 0) * c + tid];
            sb += colpart[((size_t)b * 2 + 1) * c + tid];
        }
        dot = sa * sb;
    }
    loss = block_sum(loss, sh);
    ps = block_sum(ps, sh);
    dot = block_sum(dot, sh);
    if (tid == 0) {
        const double pm = ps / m;
        const bool bad = *status != 0;  // a pair outside its operand: the caller reads nothing back, so the outputs say it
        out[0] = bad ? NAN : (float)(loss / m);
        out[1] = bad ? NAN : (float)pm;
        out[2] = bad ? NAN : (float)(dot / ((double)m * m) - pm / m);
    }
}

// ----------------------------------------------------------------------------------------------------------- backward ----
// blockIdx.y = 0: dAn[x0 .. x0 + 64) = scale (P - I) B, own rows i, other rows j;  1: dBn = scale (P - I)^T A, own rows j,
// other rows i.  P_ij = exp(S_ij - lse_i) in both.  scale = g / (m t).
__global__ __launch_bounds__(TPB) void msc_nce_bwd_kernel(int m, int c, const float *__restrict__ A, const float *__restrict__ B,
                                                          const float *__restrict__ lse, float inv_t, const float *__restrict__ g,
                                                          float *__restrict__ dAn, float *__restrict__ dBn) {
    __shared__ __attribute__((aligned(16))) float sX[TILE][KP];
    __shared__ __attribute__((aligned(16))) float sY[TILE][KP];
    __shared__ float sP[TILE][PP];
    const int mode = blockIdx.y;
    const float *X = mode ? B : A, *Y = mode ? A : B;
    float *out = mode ? dBn : dAn;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int rt = wave >> 1, ct = wave & 1;    // the S quadrant of this wavefront
    const int prt = wave & 1, pct = wave >> 1;  // its output tiles: rows prt, channel tiles pct, pct + 2, ...
    const int x0 = blockIdx.x * TILE;
    const int nchunks = (m + TILE - 1) / TILE, ctiles = (c + 31) / 32;
    float lrow[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int xr = x0 + 32 * rt + acc_row(e, h);
        lrow[e] = (mode == 0 && xr < m) ? lse[xr] : 0.f;
    }
    v16f o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        for (int e = 0; e < 16; ++e) o[u][e] = 0.f;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int y0 = ch * TILE;
        const v16f acc = s_tile(X, x0, Y, y0, m, c, sX, sY, rt, ct);
        const int yc = y0 + 32 * ct + r;
        const float lcol = (mode == 1 && yc < m) ? lse[yc] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = 32 * rt + acc_row(e, h), xr = x0 + row;
            float p = 0.f;
            if (xr < m && yc < m) p = expf(acc[e] * inv_t - (mode ? lcol : lrow[e])) - (xr == yc ? 1.f : 0.f);
            sP[row][32 * ct + r] = p;  // (the staging barriers of s_tile separate this from the reads of the last round)
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tc = pct + 2 * u;
            if (tc < ctiles) {
                const int chn = 32 * tc + r;
                const bool cok = chn < c;
#pragma unroll 8
                for (int k = 0; k < TILE; k += 2) {
                    const int yr = y0 + k + h;
                    const float a = sP[32 * prt + r][k + h];
                    const float b = (cok && yr < m) ? Y[(size_t)yr * c + chn] : 0.f;
                    o[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, o[u], 0, 0, 0);
                }
            }
        }
    }
    const float scale = g[0] * inv_t / (float)m;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int chn = 32 * (pct + 2 * u) + r;
        if (chn < c) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int xr = x0 + 32 * prt + acc_row(e, h);
                if (xr < m) out[(size_t)xr * c + chn] = o[u][e] * scale;
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- matching ----
__global__ __launch_bounds__(TPB) void msc_match_kernel(int n1, int k, long long n2, const int *__restrict__ idx,
                                                        const float *__restrict__ dist2, const long long *__restrict__ draws,
                                                        float max_radius, long long *__restrict__ chosen) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n1) return;
    const int *ri = idx + (size_t)i * k;
    const float *rd = dist2 + (size_t)i * k;
    int cnt = 0;
    for (int j = 0; j < k; ++j)
        if (ri[j] >= 0 && ri[j] < n2 && sqrtf(rd[j]) < max_radius) ++cnt;
    long long pick = -1;
    if (cnt > 0) {
        const long long draw = draws[i] < 0 ? 0 : draws[i];
        const int want = cnt - 1 - (int)(draw % cnt);
        int rank = 0;
        for (int j = 0; j < k; ++j) {
            if (ri[j] >= 0 && ri[j] < n2 && sqrtf(rd[j]) < max_radius) {
                if (rank == want) { pick = ri[j]; break; }
                ++rank;
            }
        }
    }
    chosen[i] = pick;
}

// ---------------------------------------------------------------------------------------------------------- patch ids ----
__global__ __launch_bounds__(TPB) void msc_patch_ids_kernel(int n1, int n2, int b, const float *__restrict__ o1,
                                                            const int *__restrict__ off1, const float *__restrict__ o2,
                                                            const int *__restrict__ off2, float grid,
                                                            const float *__restrict__ cell_max, long long *__restrict__ ids) {
    const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
    if (p >= (long long)n1 + n2) return;
    const bool second = p >= n1;
    const int q = (int)(second ? p - n1 : p);
    const float *o = (second ? o2 : o1) + 3 * (size_t)q;
    const int *off = second ? off2 : off1;
    int lo = 0, hi = b - 1;  // the first scene whose end lies past q
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] > q) hi = mid;
        else lo = mid + 1;
    }
    const long long nx = (long long)cell_max[0] + 1, ny = (long long)cell_max[1] + 1, nz = (long long)cell_max[2] + 1;
    const long long cx = (long long)floorf(__fdiv_rn(o[0], grid));
    const long long cy = (long long)floorf(__fdiv_rn(o[1], grid));
    const long long cz = (long long)floorf(__fdiv_rn(o[2], grid));
    ids[p] = cx + cy * nx + cz * (nx * ny) + (long long)lo * (nx * ny * nz);
}

struct NceWs {
    float *part, *pos, *dAn, *dBn;
    double *colpart;
    size_t bytes;
};

struct NcePlan {
    int rowblocks, nsplit, chunks_per_split;
};

// depends on m alone, so that the order of every sum does
NcePlan nce_plan(int m) {
    NcePlan p;
    p.rowblocks = divup(m, TILE);
    const int want = std::min(p.rowblocks, std::max(1, divup(MAX_SPLIT_BLOCKS, p.rowblocks)));
    p.chunks_per_split = divup(p.rowblocks, want);
    p.nsplit = divup(p.rowblocks, p.chunks_per_split);
    return p;
}

NceWs carve_nce(void *base, int m, int c) {
    const NcePlan pl = nce_plan(m);
    NceWs w;
    PtvCarver cv{(char *)base, 0};
    w.part = cv.take_n<float>((size_t)pl.nsplit * m * 2);
    w.pos = cv.take_n<float>(m);
    w.colpart = cv.take_n<double>((size_t)pl.rowblocks * 2 * c);
    w.dAn = cv.take_n<float>((size_t)m * c);
    w.dBn = cv.take_n<float>((size_t)m * c);
    w.bytes = cv.off;
    return w;
}

bool nce_sizes_ok(long long m, int c) { return m >= 1 && m <= MSC_MAX_PAIRS && c >= 4 && c <= MSC_MAX_CHANNELS && c % 4 == 0; }

}  // namespace

extern "C" int ptv2_msc_abi_version(void) { return 1; }

extern "C" long long ptv2_msc_nce_workspace_bytes(long long m, int c) {
    if (!nce_sizes_ok(m, c)) return -1;
    return (long long)carve_nce(nullptr, (int)m, c).bytes;
}

extern "C" int msc_nce_fwd_hip_launcher(int n1, int n2, int m, int c, const float *f1, const float *f2, const long long *pairs,
                                        float t, float *a, float *b, float *norms, float *lse, float *out, int *status,
                                        void *workspace, long long workspace_bytes, void *stream) {
    if (!nce_sizes_ok(m, c) || n1 < 1 || n2 < 1 || !(t > 0.f) || !f1 || !f2 || !pairs || !a || !b || !norms || !lse || !out || !status)
        return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < ptv2_msc_nce_workspace_bytes(m, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const NcePlan pl = nce_plan(m);
    const NceWs w = carve_nce(workspace, m, c);
    const float inv_t = 1.f / t;
    hipLaunchKernelGGL(msc_gather_norm_kernel, dim3(m), dim3(64), 0, st, n1, n2, m, c, f1, f2, pairs, a, b, norms, w.pos, status);
    const dim3 grid(pl.rowblocks, pl.nsplit);
    if (2.f * inv_t <= 80.f)  // exp(-80) is a normal fp32 number
        hipLaunchKernelGGL(msc_lse_kernel<true>, grid, dim3(TPB), 0, st, m, c, a, b, inv_t, pl.chunks_per_split, w.part);
    else
        hipLaunchKernelGGL(msc_lse_kernel<false>, grid, dim3(TPB), 0, st, m, c, a, b, inv_t, pl.chunks_per_split, w.part);
    hipLaunchKernelGGL(msc_colsum_kernel, dim3(pl.rowblocks), dim3(TPB), 0, st, m, c, a, b, w.colpart);
    hipLaunchKernelGGL(msc_nce_finish_kernel, dim3(1), dim3(TPB), 0, st, m, c, pl.nsplit, pl.rowblocks, t, w.part, w.pos,
                       w.colpart, status, lse, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int msc_nce_bwd_hip_launcher(int n1, int n2, int m, int c, const long long *pairs, const int *order, float t,
                                        const float *a, const float *b, const float *norms, const float *lse, const float *g,
                                        float *df1, float *df2, void *workspace, long long workspace_bytes, void *stream) {
    if (!nce_sizes_ok(m, c) || n1 < 1 || n2 < 1 || !(t > 0.f) || !pairs || !order || !a || !b || !norms || !lse || !g || !df1 || !df2)
        return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < ptv2_msc_nce_workspace_bytes(m, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const NcePlan pl = nce_plan(m);
    const NceWs w = carve_nce(workspace, m, c);
    if (hipMemsetAsync(df1, 0, sizeof(float) * (size_t)n1 * c, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    if (hipMemsetAsync(df2, 0, sizeof(float) * (size_t)n2 * c, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(msc_nce_bwd_kernel, dim3(pl.rowblocks, 2), dim3(TPB), 0, st, m, c, a, b, lse, 1.f / t, g, w.dAn, w.dBn);
    hipLaunchKernelGGL(msc_scatter_kernel, dim3(m), dim3(64), 0, st, n1, m, c, 0, pairs, order, w.dAn, a, norms, df1);
    hipLaunchKernelGGL(msc_scatter_kernel, dim3(m), dim3(64), 0, st, n2, m, c, 1, pairs, order + m, w.dBn, b, norms + m, df2);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int msc_match_hip_launcher(int n1, int k, long long n2, const int *idx, const float *dist2, const long long *row_draws,
                                      float max_radius, long long *chosen, void *stream) {
    if (n1 < 1 || k < 1 || k > MSC_MAX_K || n2 < 0 || (long long)n1 * k > 0x7ffffff0 || !idx || !dist2 || !row_draws || !chosen)
        return PTV2_ERR_ARG;
    hipLaunchKernelGGL(msc_match_kernel, dim3(divup(n1, TPB)), dim3(TPB), 0, (hipStream_t)stream, n1, k, n2, idx, dist2, row_draws,
                       max_radius, chosen);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int msc_patch_ids_hip_launcher(int n1, int n2, int b, const float *origin1, const int *offset1, const float *origin2,
                                          const int *offset2, float grid, const float *cell_max, long long *ids, void *stream) {
    if (n1 < 0 || n2 < 0 || (long long)n1 + n2 < 1 || n1 > 0x7ffffff0 / 3 || n2 > 0x7ffffff0 / 3 || b < 1 || !(grid > 0.f) ||
        (n1 && !origin1) || (n2 && !origin2) || !offset1 || !offset2 || !cell_max || !ids)
        return PTV2_ERR_ARG;
    hipLaunchKernelGGL(msc_patch_ids_kernel, dim3(divup((long long)n1 + n2, TPB)), dim3(TPB), 0, (hipStream_t)stream, n1, n2, b,
                       origin1, offset1, origin2, offset2, grid, cell_max, ids);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
