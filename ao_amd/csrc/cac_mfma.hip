// ao_amd/csrc/cac_mfma.hip -- the context-aware classifier heads of cac.hip for wide backbones: 64 < C <= 128 (C % 4 == 0,
// K <= 256), the K x C and rows x K products on V_MFMA_F32_16X16X4_F32 (mfma4: a lane gives A[m = lane & 15][k = lane >> 4]
// and B[k = lane >> 4][n = lane & 15] and holds D[m = 4 (lane >> 4) + i][n = lane & 15], i = 0..3).  The contract is cac.hip's
// (include/ptv2_hip.h): the same slabs of 256 rows of one scene, the same workspace, partials added in a fixed order by a
// second launch, no float atomics, no host synchronisation, the same bits from run to run.  cac.hip's launchers forward here.
//
// Two tile cores:
//   rows contracted  (contract_rows)   a K x C partial of a chunk: W^T X (+ z) of the weighted sums, g^T xhat of the cosine
//                    backward.  Grid (chunks x class groups of 64, scenes); wavefront w owns classes 16 w .. 16 w + 15 of the
//                    group and all of C (<= 8 accumulator tiles); stages of 16 rows.
//   rows kept        (kept_nmajor, kept_kmajor)   16 rows per wavefront against an operand every row of the scene shares
//                    (qhat, dout), staged one class group of 64 at a time for a stage of 64 rows:
//                    kept_nmajor  rows x classes, contraction C     the cosine logits, dw = X dout^T
//                    kept_kmajor  rows x C, contraction classes     gx = g qhat, gx = (w / (z + eps)) dout
//                    Everything a row needs after the products (the projection through its norm, the softmax backward over
//                    all K of dw, kept in registers) stays inside its wavefront.
// LDS images: a 64 x C operand has pitch P = 16 ceil(C / 16) + 4 (= 4 mod 16: the reads l15 * P + quad and (c + 4 quad) * P +
// l15 both touch 64 distinct banks; kept_kmajor walks the classes of a group in the order that makes the second form),
// weights / g of a 16-row tile are class-major with pitch 20 for the same reason.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = 256;  // rows per workgroup (cac.hip's slab)
constexpr int TILE = 16;    // rows of a matrix tile
constexpr int STAGE = 64;   // rows per stage of the rows-kept kernels: one tile per wavefront
constexpr int GROUP = 64;   // classes per group
constexpr int MAXK = 256, MINC = 68, MAXC = 128;
constexpr int MAXG = MAXK / GROUP;
constexpr int WP = 20;      // pitch of a class-major 16-row tile
constexpr int XP = 144;     // row pitch of contract_rows' x tile (= 16 mod 64: quad * XP + l15 touches 64 banks)
constexpr float NORM_EPS = 1e-12f;

__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ void scene_rows(const int *offset, int s, long long &lo, long long &hi) {
    lo = s ? offset[s - 1] : 0;
    hi = offset[s];
}
__host__ __device__ constexpr int tiles_of(int c) { return (c + 15) / 16; }
__host__ __device__ constexpr int pitch_of(int c) { return 16 * tiles_of(c) + 4; }
__device__ __forceinline__ v4f zero4() { return (v4f){0.f, 0.f, 0.f, 0.f}; }

// ------------------------------------------------------------------------------------------------------------ tile cores
// acc[t] (classes 16 w .. x columns 16 t ..) += wT^T (16 rows x 16 classes: wT[class * WP + row]) xs (16 rows x C: xs[row * XP + c])
template <int NT>
__device__ __forceinline__ void contract_rows(const float *wT, const float *xs, v4f (&acc)[NT]) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, quad = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < TILE / 4; ++kk) {
        const float a = wT[l15 * WP + 4 * kk + quad];
        const float *b = xs + (4 * kk + quad) * XP + l15;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma4(a, b[16 * t], acc[t]);
    }
}

// acc[t] (16 rows x classes 16 t .. of the group) += xs (16 rows x C: xs[row * P + c]) op^T (64 classes x C: op[class * P + c])
__device__ __forceinline__ void kept_nmajor(const float *xs, const float *op, int C, int P, v4f (&acc)[GROUP / 16]) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, quad = lane >> 4;
    const float *a = xs + l15 * P + quad, *b = op + l15 * P + quad;
    for (int kk = 0; kk < C; kk += 4) {
        const float av = a[kk];
#pragma unroll
        for (int t = 0; t < GROUP / 16; ++t) acc[t] = mfma4(av, b[16 * t * P + kk], acc[t]);
    }
}

// acc[t] (16 rows x columns 16 t ..) += aT^T (16 rows x 64 classes: aT[class * WP + row], times asc[class] if given) op (64
// classes x C).  Step s takes the classes 16 (s >> 2) + (s & 3) + 4 quad: each class once, and four op rows 16 banks apart.
template <int NT>
__device__ __forceinline__ void kept_kmajor(const float *aT, const float *asc, const float *op, int P, v4f (&acc)[NT]) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, quad = lane >> 4;
#pragma unroll 4
    for (int s = 0; s < GROUP / 4; ++s) {
        const int cl = 16 * (s >> 2) + (s & 3) + 4 * quad;
        float a = aT[cl * WP + l15];
        if (asc) a *= asc[cl];
        const float *b = op + cl * P + l15;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma4(a, b[16 * t], acc[t]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- staging
// rows base .. base + 63 of src (rows >= end: zeros) into dst[64][P], columns C .. P - 1 zero; four lanes per row.  NORM: every
// row divided by max(|row|, 1e-12), |row| into nrm[row] if given
template <bool NORM>
__device__ __forceinline__ void stage64(const float *__restrict__ src, long long base, long long end, int C, int P, float *dst,
                                        float *nrm) {
    const int r = threadIdx.x >> 2, l4 = threadIdx.x & 3, CQ = C / 4, PQ = P / 4;
    const bool ok = base + r < end;
    const float4 *row = (const float4 *)src + (base + r) * CQ;
    float4 v[MAXC / 16];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < MAXC / 16; ++j) {
        const int q = l4 + 4 * j;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && q < CQ) v[j] = row[q];
        ss = __builtin_fmaf(v[j].x, v[j].x, ss); ss = __builtin_fmaf(v[j].y, v[j].y, ss);
        ss = __builtin_fmaf(v[j].z, v[j].z, ss); ss = __builtin_fmaf(v[j].w, v[j].w, ss);
    }
    if (NORM) {
        ss += dpp_mov<0xB1>(ss);  // the four lanes of a row: quad_perm [1,0,3,2], then [2,3,0,1]
        ss += dpp_mov<0x4E>(ss);
        const float nr = sqrtf(ss), den = fmaxf(nr, NORM_EPS);
#pragma unroll
        for (int j = 0; j < MAXC / 16; ++j) { v[j].x /= den; v[j].y /= den; v[j].z /= den; v[j].w /= den; }
        if (nrm && l4 == 0) nrm[r] = nr;
    }
    float4 *d = (float4 *)dst + r * PQ;
#pragma unroll
    for (int j = 0; j < MAXC / 16; ++j)
        if (l4 + 4 * j < CQ) d[l4 + 4 * j] = v[j];
    for (int q = CQ + l4; q < PQ; q += 4) d[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// weights of the tile rows rr0, rr0 + step, .. < 16 (row r0 + rr; rows >= rend: zero) and the classes k0 .. k0 + kn - 1 (kn %
// 64 == 0; classes >= K: zero) into wT[(k - k0) * WP + rr]: cac.hip's row_weights, one wavefront per row
__device__ void wide_row_weights(int mode, const float *__restrict__ logits, const long long *__restrict__ label, int K, float thr,
                                 long long r0, long long rend, int rr0, int step, int k0, int kn, float *wT) {
    const int lane = threadIdx.x & 63;
    for (int rr = rr0; rr < TILE; rr += step) {
        const long long row = r0 + rr;
        float w[MAXK / 64] = {0.f, 0.f, 0.f, 0.f};
        if (row < rend) {
            if (mode == 1) {
                const long long y = label[row];
#pragma unroll
                for (int i = 0; i < MAXK / 64; ++i) w[i] = y == lane + 64 * i ? 1.f : 0.f;
            } else {
                const float *l = logits + row * K;
                float m = -INFINITY;
#pragma unroll
                for (int i = 0; i < MAXK / 64; ++i) {
                    const int k = lane + 64 * i;
                    w[i] = k < K ? l[k] : -INFINITY;
                    m = fmaxf(m, w[i]);
                }
                m = wmax(m);
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < MAXK / 64; ++i) {
                    w[i] = lane + 64 * i < K ? expf(w[i] - m) : 0.f;
                    s += w[i];
                }
                s = wsum(s);
                // max_k p_k = exp(0) / s
                const float keep = (thr > 0.f && 1.f / s < thr) ? 0.f : 1.f;
#pragma unroll
                for (int i = 0; i < MAXK / 64; ++i) w[i] = lane + 64 * i < K ? w[i] / s * keep : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < MAXK / 64; ++i) {
            const int k = lane + 64 * i - k0;
            if (k >= 0 && k < kn) wT[k * WP + rr] = w[i];
        }
    }
}

// --------------------------------------------------------------------------------------------------------- rows contracted
// COS = false: part[slab][K * C + K] = sum_n w_nk x_n and sum_n w_nk over this workgroup's chunk (the classes of its group)
// COS = true:  part[slab][K * C] = sum_n scale dout_nk xhat_n
template <bool COS, int NT>
__global__ __launch_bounds__(TPB) void wide_partial_kernel(int mode, int K, int C, int J, const float *__restrict__ x,
                                                           const float *__restrict__ logits, const long long *__restrict__ label,
                                                           const int *__restrict__ offset, float thr, float scale,
                                                           const float *__restrict__ dout, float *__restrict__ part) {
    __shared__ float4 xs4[TILE * XP / 4];
    __shared__ float wT[GROUP * WP];
    float *xs = (float *)xs4;
    const int NG = (K + GROUP - 1) / GROUP, grp = blockIdx.x % NG, j = blockIdx.x / NG, s = blockIdx.y;  // (a chunk's groups run together)
    const int CQ = C / 4, k0 = GROUP * grp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, quad = lane >> 4;
    long long lo, hi;
    scene_rows(offset, s, lo, hi);
    const long long c0 = lo + (long long)j * CHUNK, c1 = min(hi, c0 + CHUNK);
    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = zero4();
    float z = 0.f;
    for (int e = threadIdx.x; e < TILE * (XP / 4 - CQ); e += TPB) {  // the columns no stage writes
        const int rr = e / (XP / 4 - CQ);
        xs4[rr * (XP / 4) + CQ + (e - rr * (XP / 4 - CQ))] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long r0 = c0; r0 < c1; r0 += TILE) {
        __syncthreads();
        for (int e = threadIdx.x; e < TILE * CQ; e += TPB) {
            const int rr = e / CQ, q = e - rr * CQ;
            const long long row = r0 + rr;
            xs4[rr * (XP / 4) + q] = row < c1 ? ((const float4 *)x)[row * CQ + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (COS) {
            for (int e = threadIdx.x; e < TILE * GROUP; e += TPB) {
                const int rr = e >> 6, cl = e & 63;
                const long long row = r0 + rr;
                wT[cl * WP + rr] = (row < c1 && k0 + cl < K) ? scale * dout[row * K + k0 + cl] : 0.f;
            }
            __syncthreads();
            // xhat: 16 lanes per row, each its own columns
            float *xr = xs + (threadIdx.x >> 4) * XP;
            float ss = 0.f;
            for (int c = l15; c < C; c += 16) ss = __builtin_fmaf(xr[c], xr[c], ss);
            const float den = fmaxf(sqrtf(row16_sum(ss)), NORM_EPS);
            for (int c = l15; c < C; c += 16) xr[c] = xr[c] / den;
        } else {
            wide_row_weights(mode, logits, label, K, thr, r0, c1, wave, TPB / 64, k0, GROUP, wT);
        }
        __syncthreads();
        contract_rows<NT>(wT + 16 * wave * WP, xs, acc);
        if (!COS && threadIdx.x < GROUP)
            for (int rr = 0; rr < TILE; ++rr) z += wT[threadIdx.x * WP + rr];
    }
    const long long stride = (long long)K * C + (COS ? 0 : K);
    float *p = part + ((long long)s * J + j) * stride;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int c = 16 * t + l15;
        if (c < C)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + 16 * wave + 4 * quad + i;
                if (k < K) p[(long long)k * C + c] = acc[t][i];
            }
    }
    if (!COS && threadIdx.x < GROUP && k0 + (int)threadIdx.x < K) p[(long long)K * C + k0 + threadIdx.x] = z;
}

// one workgroup of 128 threads per (set, k): cac.hip's cos_proto_finalize_kernel for C <= 128.  The slabs of the set in order ->
// d qhat_k, then through q / max(|q|, eps); the two wavefronts' sums meet in LDS, added in a fixed order
__global__ __launch_bounds__(128) void wide_cos_proto_finalize_kernel(int K, int C, int slabs_per_set, const float *__restrict__ part,
                                                                      const float *__restrict__ q, float *__restrict__ gq) {
    __shared__ float sh[4];
    const int k = blockIdx.x, set = blockIdx.y, c = threadIdx.x, wave = threadIdx.x >> 6;
    const long long stride = (long long)K * C;
    const float *p = part + (long long)set * slabs_per_set * stride + (long long)k * C;
    float da[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        int b = 0;
        for (; b + 8 <= slabs_per_set; b += 8)
#pragma unroll
            for (int u = 0; u < 8; ++u) da[u] += p[(b + u) * stride + c];
        for (; b < slabs_per_set; ++b) da[0] += p[b * stride + c];
    }
    const float d = ((da[0] + da[1]) + (da[2] + da[3])) + ((da[4] + da[5]) + (da[6] + da[7]));
    const float qv = c < C ? q[((long long)set * K + k) * C + c] : 0.f;
    const float ss = wsum(qv * qv);
    if ((threadIdx.x & 63) == 0) sh[wave] = ss;
    __syncthreads();
    const float nr = sqrtf(sh[0] + sh[1]);
    const float qh = qv / fmaxf(nr, NORM_EPS);
    const float dp = wsum(qh * d);
    if ((threadIdx.x & 63) == 0) sh[2 + wave] = dp;
    __syncthreads();
    const float dot = sh[2] + sh[3];
    if (c < C) gq[((long long)set * K + k) * C + c] = nr > NORM_EPS ? (d - qh * dot) / nr : d / NORM_EPS;
}

// --------------------------------------------------------------------------------------------------------------- rows kept
// dynamic LDS of the rows-kept kernels, in floats: xs[64][P] | op[64][P] | nrm[64] | (tiles) 4 x [64 NG][WP] | zinv, pd [64 NG] each
__host__ __device__ constexpr size_t kept_lds_floats(int K, int C, bool tiles, bool scales) {
    const size_t k64 = (size_t)GROUP * ((K + GROUP - 1) / GROUP);
    return (size_t)2 * STAGE * pitch_of(C) + STAGE + (tiles ? 4 * k64 * WP : 0) + (scales ? 2 * k64 : 0);
}

// BWD = false: out[n, k] = scale <xhat_n, qhat_k>
// BWD = true:  out = gx (N, C): dxn_n = sum_k scale dout_nk qhat_k taken through x / max(|x|, eps)
template <bool BWD, int NT>
__global__ __launch_bounds__(TPB) void wide_cos_rows_kernel(int K, int C, const float *__restrict__ x, const float *__restrict__ q,
                                                            int per_scene, const int *__restrict__ offset, float scale,
                                                            const float *__restrict__ dout, float *__restrict__ out) {
    extern __shared__ float4 smem4[];
    const int P = 16 * NT + 4, NG = (K + GROUP - 1) / GROUP, K64 = GROUP * NG;
    float *xs = (float *)smem4, *op = xs + STAGE * P, *nrm = op + STAGE * P;
    const int j = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, quad = lane >> 4;
    float *gT = nrm + STAGE + wave * K64 * WP;  // (BWD) this wavefront's scale * dout tile, class-major
    long long lo, hi;
    scene_rows(offset, s, lo, hi);
    const long long c0 = lo + (long long)j * CHUNK, c1 = min(hi, c0 + CHUNK);
    if (c0 >= c1) return;
    const float *qs = q + (per_scene ? (long long)s * K * C : 0);
    for (long long r0 = c0; r0 < c1; r0 += STAGE) {
        const long long w0 = r0 + TILE * wave;  // this wavefront's rows
        __syncthreads();
        stage64<true>(x, r0, c1, C, P, xs, nrm);
        if (BWD)
            for (int rr = 0; rr < TILE; ++rr)
                for (int k = lane; k < K64; k += 64) gT[k * WP + rr] = (w0 + rr < c1 && k < K) ? scale * dout[(w0 + rr) * K + k] : 0.f;
        v4f acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = zero4();
#pragma unroll
        for (int g = 0; g < MAXG; ++g) {
            if (g >= NG) break;
            __syncthreads();
            stage64<true>(qs, GROUP * g, K, C, P, op, nullptr);
            __syncthreads();
            if (BWD) {
                kept_kmajor<NT>(gT + GROUP * g * WP, nullptr, op, P, acc);
            } else {
                v4f o[GROUP / 16];
#pragma unroll
                for (int t = 0; t < GROUP / 16; ++t) o[t] = zero4();
                kept_nmajor(xs + TILE * wave * P, op, C, P, o);
#pragma unroll
                for (int t = 0; t < GROUP / 16; ++t) {
                    const int k = GROUP * g + 16 * t + l15;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const long long row = w0 + 4 * quad + i;
                        if (k < K && row < c1) out[row * K + k] = scale * o[t][i];
                    }
                }
            }
        }
        if (BWD) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = TILE * wave + 4 * quad + i;
                const float *xr = xs + rl * P + l15;
                float rd = 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) rd = __builtin_fmaf(xr[16 * t], acc[t][i], rd);
                rd = row16_sum(rd);
                const float nr = nrm[rl];
                const long long row = r0 + rl;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int c = 16 * t + l15;
                    if (c < C && row < c1)
                        out[row * C + c] = nr > NORM_EPS ? (acc[t][i] - xr[16 * t] * rd) / nr : acc[t][i] / NORM_EPS;
                }
            }
        }
    }
}

// gx_n = sum_k w_nk / (z_k + eps) dout_k; glogits (mode 0, optional): dw_nk = (<x_n, dout_k> - <out_k, dout_k>) / (z_k + eps), then
// the softmax backward of the row (a masked row has w = 0 everywhere and comes out zero)
template <int NT>
__global__ __launch_bounds__(TPB) void wide_wsum_backward_kernel(int mode, int K, int C, const float *__restrict__ x,
                                                                 const float *__restrict__ logits,
                                                                 const long long *__restrict__ label,
                                                                 const int *__restrict__ offset, float thr, float eps,
                                                                 const float *__restrict__ z, const float *__restrict__ out,
                                                                 const float *__restrict__ dout, float *__restrict__ gx,
                                                                 float *__restrict__ glogits) {
    extern __shared__ float4 smem4[];
    const int P = 16 * NT + 4, NG = (K + GROUP - 1) / GROUP, K64 = GROUP * NG;
    float *xs = (float *)smem4, *op = xs + STAGE * P, *tiles = op + STAGE * P + STAGE;
    float *zinv = tiles + 4 * K64 * WP, *pd = zinv + K64;
    const int j = blockIdx.x, s = blockIdx.y, set = mode == 0 ? s : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, quad = lane >> 4;
    float *wT = tiles + wave * K64 * WP;  // this wavefront's weights, class-major
    long long lo, hi;
    scene_rows(offset, s, lo, hi);
    const long long c0 = lo + (long long)j * CHUNK, c1 = min(hi, c0 + CHUNK);
    if (c0 >= c1) return;
    const float *ds = dout + (long long)set * K * C;
    for (int k = threadIdx.x; k < K64; k += TPB) {
        float a = 0.f;
        if (glogits && k < K) {
            const float *o = out + ((long long)set * K + k) * C, *d = ds + (long long)k * C;
            for (int c = 0; c < C; ++c) a = __builtin_fmaf(o[c], d[c], a);
        }
        zinv[k] = k < K ? 1.f / (z[(long long)set * K + k] + eps) : 0.f;
        pd[k] = a;
    }
    for (long long r0 = c0; r0 < c1; r0 += STAGE) {
        const long long w0 = r0 + TILE * wave;
        __syncthreads();
        stage64<false>(x, r0, c1, C, P, xs, nullptr);
        wide_row_weights(mode, logits, label, K, thr, w0, c1, 0, 1, 0, K64, wT);
        v4f acc[NT], dw[MAXG][GROUP / 16];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = zero4();
#pragma unroll
        for (int g = 0; g < MAXG; ++g) {
            if (g >= NG) break;
            __syncthreads();
            stage64<false>(ds, GROUP * g, K, C, P, op, nullptr);
            __syncthreads();
            kept_kmajor<NT>(wT + GROUP * g * WP, zinv + GROUP * g, op, P, acc);
            if (glogits) {
#pragma unroll
                for (int t = 0; t < GROUP / 16; ++t) dw[g][t] = zero4();
                kept_nmajor(xs + TILE * wave * P, op, C, P, dw[g]);
#pragma unroll
                for (int t = 0; t < GROUP / 16; ++t) {
                    const int k = GROUP * g + 16 * t + l15;
#pragma unroll
                    for (int i = 0; i < 4; ++i) dw[g][t][i] = (dw[g][t][i] - pd[k]) * zinv[k];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = 16 * t + l15;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long row = w0 + 4 * quad + i;
                if (c < C && row < c1) gx[row * C + c] = acc[t][i];
            }
        }
        if (glogits) {
            // lane: rows 4 quad .. 4 quad + 3 of the tile, classes l15 + 16 t of every group; the 16 lanes of a quad hold a row
            float tt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < MAXG; ++g) {
                if (g >= NG) break;
#pragma unroll
                for (int t = 0; t < GROUP / 16; ++t) {
                    const float4 w = *(const float4 *)&wT[(GROUP * g + 16 * t + l15) * WP + 4 * quad];
                    tt[0] = __builtin_fmaf(w.x, dw[g][t][0], tt[0]); tt[1] = __builtin_fmaf(w.y, dw[g][t][1], tt[1]);
                    tt[2] = __builtin_fmaf(w.z, dw[g][t][2], tt[2]); tt[3] = __builtin_fmaf(w.w, dw[g][t][3], tt[3]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) tt[i] = row16_sum(tt[i]);
#pragma unroll
            for (int g = 0; g < MAXG; ++g) {
                if (g >= NG) break;
#pragma unroll
                for (int t = 0; t < GROUP / 16; ++t) {
                    const int k = GROUP * g + 16 * t + l15;
                    const float4 w = *(const float4 *)&wT[k * WP + 4 * quad];
                    const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const long long row = w0 + 4 * quad + i;
                        if (k < K && row < c1) glogits[row * K + k] = wv[i] * (dw[g][t][i] - tt[i]);
                    }
                }
            }
        }
    }
}

int chunks_of(int max_rows) { return max_rows > 0 ? divup(max_rows, CHUNK) : 1; }

// the kernels are instantiated per column-tile count NT = ceil(C / 16) = 5 .. 8: accumulator tables without a predicate
#define WIDE_NT(c, CALL)            \
    switch (tiles_of(c)) {          \
    case 5: { CALL(5) } break;      \
    case 6: { CALL(6) } break;      \
    case 7: { CALL(7) } break;      \
    case 8: { CALL(8) } break;      \
    default: return PTV2_ERR_ARG;   \
    }
}  // namespace

int cac_wide_ok(int k, int c) { return k >= 1 && k <= MAXK && c >= MINC && c <= MAXC && c % 4 == 0; }

int cac_wide_wsum_partial(int mode, int b, int max_rows, int k, int c, const float *x, const float *logits, const long long *label,
                          const int *offset, float thr, float *part, void *stream) {
    const int J = chunks_of(max_rows);
#define CALL(NT)                                                                                                                  \
    hipLaunchKernelGGL((wide_partial_kernel<false, NT>), dim3(divup(k, GROUP) * J, b), dim3(TPB), 0, (hipStream_t)stream, mode, k, \
                       c, J, x, logits, label, offset, thr, 0.f, (const float *)nullptr, part);
    WIDE_NT(c, CALL)
#undef CALL
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

int cac_wide_wsum_backward(int mode, int b, int max_rows, int k, int c, const float *x, const float *logits, const long long *label,
                           const int *offset, float thr, float eps, const float *z, const float *out, const float *dout, float *gx,
                           float *glogits, void *stream) {
    const size_t lds = sizeof(float) * kept_lds_floats(k, c, true, true);
#define CALL(NT)                                                                                                          \
    RUN(ptv2_kernel_lds((const void *)wide_wsum_backward_kernel<NT>, lds));                                               \
    hipLaunchKernelGGL((wide_wsum_backward_kernel<NT>), dim3(chunks_of(max_rows), b), dim3(TPB), lds, (hipStream_t)stream, \
                       mode, k, c, x, logits, label, offset, thr, eps, z, out, dout, gx, glogits);
    WIDE_NT(c, CALL)
#undef CALL
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

int cac_wide_cos_forward(int b, int max_rows, int k, int c, const float *x, const float *q, int per_scene, const int *offset,
                         float scale, float *out, void *stream) {
    const size_t lds = sizeof(float) * kept_lds_floats(k, c, false, false);
#define CALL(NT)                                                                                                            \
    RUN(ptv2_kernel_lds((const void *)wide_cos_rows_kernel<false, NT>, lds));                                               \
    hipLaunchKernelGGL((wide_cos_rows_kernel<false, NT>), dim3(chunks_of(max_rows), b), dim3(TPB), lds, (hipStream_t)stream, \
                       k, c, x, q, per_scene, offset, scale, (const float *)nullptr, out);
    WIDE_NT(c, CALL)
#undef CALL
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

int cac_wide_cos_backward(int b, int max_rows, int k, int c, const float *x, const float *q, int per_scene, const int *offset,
                          float scale, const float *dout, float *gx, float *gq, float *part, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const int J = chunks_of(max_rows);
    const size_t lds = sizeof(float) * kept_lds_floats(k, c, true, false);
#define CALL(NT)                                                                                                                \
    RUN(ptv2_kernel_lds((const void *)wide_cos_rows_kernel<true, NT>, lds));                                                    \
    hipLaunchKernelGGL((wide_cos_rows_kernel<true, NT>), dim3(J, b), dim3(TPB), lds, st, k, c, x, q, per_scene, offset, scale,   \
                       dout, gx);                                                                                               \
    hipLaunchKernelGGL((wide_partial_kernel<true, NT>), dim3(divup(k, GROUP) * J, b), dim3(TPB), 0, st, 0, k, c, J, x,           \
                       (const float *)nullptr, (const long long *)nullptr, offset, 0.f, scale, dout, part);
    WIDE_NT(c, CALL)
#undef CALL
    hipLaunchKernelGGL(wide_cos_proto_finalize_kernel, dim3(k, per_scene ? b : 1), dim3(128), 0, st, k, c, per_scene ? J : b * J,
                       (const float *)part, q, gq);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
