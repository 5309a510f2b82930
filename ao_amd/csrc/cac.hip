// ao_amd/csrc/cac.hip -- the context-aware classifier heads (CAC-v1m1,
// pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py) at N-row scale: no python loop over
// scenes or classes, no host synchronisation, no float atomics.
//
//   weighted sums   mode 0 (soft prototypes, :97-150):  w_nk = softmax(logits_n)_k * [max_k p_nk >= thr]   (thr <= 0: no mask)
//                   out[s,k,:] = sum_{n in scene s} w_nk x_n / (z[s,k] + eps),  z[s,k] = sum_n w_nk
//                   mode 1 (class means, :72-95):        w_nk = [label_n == k], one set over the whole batch
//   cosine logits   out[n,k] = scale * <x_n / max(|x_n|, 1e-12), q_k / max(|q_k|, 1e-12)>  (get_pred :64-70), q per scene or shared
//   distillation    get_distill_loss (:152-198) with smoothness 0.5, eps 0
//
// Reductions over rows: every workgroup owns a chunk of CHUNK rows of ONE scene (grid = chunks per scene x scenes, the
// chunk count from the host's largest scene) and writes a partial slab; a second launch adds the slabs in a fixed order.
// Results are bitwise reproducible from run to run.  The softmax weights are recomputed in the backward (an N x K matrix
// is 240 MB at 300 k rows and K = 200).  Limits: K <= 256, C % 4 == 0, C <= 64.
#include <algorithm>

#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = 256;  // rows per workgroup
constexpr int TILE = 16;    // rows staged in LDS at a time
constexpr int COS_TILE = 64;  // (the cosine forward)
constexpr int MAXK = 256, MAXC = 64;
constexpr int NI = MAXK * (MAXC / 4) / TPB;  // float4 accumulators per thread of a K x C partial
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

// weights of rows r0 .. r0+TILE-1 (rows >= rend: zero) into ws[TILE][K]; one wavefront per row
__device__ void row_weights(int mode, const float *__restrict__ logits, const long long *__restrict__ label, int K, float thr,
                            long long r0, long long rend, float *ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int rr = wave; rr < TILE; rr += TPB / 64) {
        const long long row = r0 + rr;
        float *w = ws + rr * K;
        if (row >= rend) {
            for (int k = lane; k < K; k += 64) w[k] = 0.f;
            continue;
        }
        if (mode == 1) {
            const long long y = label[row];
            for (int k = lane; k < K; k += 64) w[k] = y == k ? 1.f : 0.f;
            continue;
        }
        const float *l = logits + row * K;
        float v[MAXK / 64], m = -INFINITY;
#pragma unroll
        for (int i = 0; i < MAXK / 64; ++i) {
            const int k = lane + 64 * i;
            v[i] = k < K ? l[k] : -INFINITY;
            m = fmaxf(m, v[i]);
        }
        m = wmax(m);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXK / 64; ++i) {
            v[i] = lane + 64 * i < K ? expf(v[i] - m) : 0.f;
            s += v[i];
        }
        s = wsum(s);
        // max_k p_k = exp(0) / s
        const float keep = (thr > 0.f && 1.f / s < thr) ? 0.f : 1.f;
#pragma unroll
        for (int i = 0; i < MAXK / 64; ++i) {
            const int k = lane + 64 * i;
            if (k < K) w[k] = v[i] / s * keep;
        }
    }
}

// x rows r0 .. r0+TILE-1 into xs[TILE][C] (zero past rend)
__device__ void load_rows(const float *__restrict__ x, int C, long long r0, long long rend, float *xs) {
    const int CQ = C / 4;
    for (int e = threadIdx.x; e < TILE * CQ; e += TPB) {
        const int rr = e / CQ, q = e - rr * CQ;
        const long long row = r0 + rr;
        ((float4 *)xs)[e] = row < rend ? ((const float4 *)x)[row * CQ + q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// partial[slab][K*C + K]: sum_n w_nk x_n and sum_n w_nk over this workgroup's chunk
__global__ __launch_bounds__(TPB) void wsum_partial_kernel(int mode, int K, int C, int J, const float *__restrict__ x,
                                                           const float *__restrict__ logits, const long long *__restrict__ label,
                                                           const int *__restrict__ offset, float thr, float *__restrict__ part) {
    __shared__ float4 xs4[TILE * MAXC / 4];
    __shared__ float ws[TILE * MAXK];
    float *xs = (float *)xs4;
    const int j = blockIdx.x, s = blockIdx.y, CQ = C / 4, items = K * CQ;
    long long lo, hi;
    scene_rows(offset, s, lo, hi);
    const long long c0 = lo + (long long)j * CHUNK, c1 = min(hi, c0 + CHUNK);
    float4 acc[NI];
    int kk[NI], qq[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int e = threadIdx.x + i * TPB;
        kk[i] = e / CQ;
        qq[i] = e - kk[i] * CQ;
    }
    float z = 0.f;
    for (long long r0 = c0; r0 < c1; r0 += TILE) {
        load_rows(x, C, r0, c1, xs);
        row_weights(mode, logits, label, K, thr, r0, c1, ws);
        __syncthreads();
        for (int rr = 0; rr < TILE; ++rr) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if (threadIdx.x + i * TPB < items) {
                    const float w = ws[rr * K + kk[i]];
                    const float4 a = xs4[rr * CQ + qq[i]];
                    acc[i].x = __builtin_fmaf(w, a.x, acc[i].x); acc[i].y = __builtin_fmaf(w, a.y, acc[i].y);
                    acc[i].z = __builtin_fmaf(w, a.z, acc[i].z); acc[i].w = __builtin_fmaf(w, a.w, acc[i].w);
                }
            }
            if ((int)threadIdx.x < K) z += ws[rr * K + threadIdx.x];
        }
        __syncthreads();
    }
    float *p = part + ((long long)s * J + j) * ((long long)K * C + K);
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (threadIdx.x + i * TPB < items) ((float4 *)p)[threadIdx.x + i * TPB] = acc[i];
    if ((int)threadIdx.x < K) p[(long long)K * C + threadIdx.x] = z;
}

// one thread per (set, k, c) and (set, k) (c == C): the slabs of a set added in order; out = sum / (z + eps)
__global__ __launch_bounds__(TPB) void wsum_finalize_kernel(int K, int C, int nsets, int slabs_per_set,
                                                            const float *__restrict__ part, float eps, float *__restrict__ z,
                                                            float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * TPB + threadIdx.x;
    if (e >= (long long)nsets * K * (C + 1)) return;
    const int set = (int)(e / ((long long)K * (C + 1)));
    const int r = (int)(e - (long long)set * K * (C + 1)), k = r / (C + 1), c = r - k * (C + 1);
    const long long stride = (long long)K * C + K;
    const float *p = part + (long long)set * slabs_per_set * stride;
    // eight independent chains (their loads in flight together), combined in a fixed order
    float za[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, aa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const long long zo = (long long)K * C + k, ao = (long long)k * C + (c < C ? c : 0);
    int b = 0;
    for (; b + 8 <= slabs_per_set; b += 8)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            za[u] += p[(b + u) * stride + zo];
            aa[u] += p[(b + u) * stride + ao];
        }
    for (; b < slabs_per_set; ++b) {
        za[0] += p[b * stride + zo];
        aa[0] += p[b * stride + ao];
    }
    const float zs = ((za[0] + za[1]) + (za[2] + za[3])) + ((za[4] + za[5]) + (za[6] + za[7]));
    const float a = ((aa[0] + aa[1]) + (aa[2] + aa[3])) + ((aa[4] + aa[5]) + (aa[6] + aa[7]));
    if (c == C) z[(long long)set * K + k] = zs;
    else out[((long long)set * K + k) * C + c] = a / (zs + eps);
}

// gx_n = sum_k w_nk / (z_k + eps) dout_k; glogits (mode 0, optional): dw_nk = mask_n (<x_n, dout_k> - <out_k, dout_k>) /
// (z_k + eps), then the softmax backward
__global__ __launch_bounds__(TPB) void wsum_backward_kernel(int mode, int K, int C, const float *__restrict__ x,
                                                            const float *__restrict__ logits, const long long *__restrict__ label,
                                                            const int *__restrict__ offset, float thr, float eps,
                                                            const float *__restrict__ z, const float *__restrict__ out,
                                                            const float *__restrict__ dout, float *__restrict__ gx,
                                                            float *__restrict__ glogits) {
    __shared__ float4 dq4[MAXK * MAXC / 4];
    __shared__ float4 xs4[TILE * MAXC / 4];
    __shared__ float ws[TILE * MAXK], dws[TILE * MAXK];
    __shared__ float zinv[MAXK], pd[MAXK];
    float *xs = (float *)xs4, *dq = (float *)dq4;
    const int j = blockIdx.x, s = blockIdx.y, CQ = C / 4;
    const int set = mode == 0 ? s : 0;
    long long lo, hi;
    scene_rows(offset, s, lo, hi);
    const long long c0 = lo + (long long)j * CHUNK, c1 = min(hi, c0 + CHUNK);
    if (c0 >= c1) return;
    const float4 *dsrc = (const float4 *)(dout + (long long)set * K * C);
    for (int e = threadIdx.x; e < K * CQ; e += TPB) dq4[e] = dsrc[e];
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += TPB) {
        zinv[k] = 1.f / (z[(long long)set * K + k] + eps);
        if (glogits) {
            const float *o = out + ((long long)set * K + k) * C;
            float a = 0.f;
            for (int c = 0; c < C; ++c) a = __builtin_fmaf(o[c], dq[k * C + c], a);
            pd[k] = a;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long r0 = c0; r0 < c1; r0 += TILE) {
        load_rows(x, C, r0, c1, xs);
        row_weights(mode, logits, label, K, thr, r0, c1, ws);
        __syncthreads();
        for (int e = threadIdx.x; e < TILE * CQ; e += TPB) {
            const int rr = e / CQ, q = e - rr * CQ;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < K; ++k) {
                const float w = ws[rr * K + k] * zinv[k];
                const float4 d = dq4[k * CQ + q];
                a.x = __builtin_fmaf(w, d.x, a.x); a.y = __builtin_fmaf(w, d.y, a.y);
                a.z = __builtin_fmaf(w, d.z, a.z); a.w = __builtin_fmaf(w, d.w, a.w);
            }
            if (r0 + rr < c1) ((float4 *)gx)[(r0 + rr) * CQ + q] = a;
        }
        if (glogits) {
            // (a masked row has w = 0 everywhere: its rows below come out zero without the mask itself)
            for (int e = threadIdx.x; e < TILE * K; e += TPB) {
                const int rr = e / K, k = e - rr * K;
                float a = 0.f;
                for (int q = 0; q < CQ; ++q) {
                    const float4 u = xs4[rr * CQ + q], d = dq4[k * CQ + q];
                    a = __builtin_fmaf(u.x, d.x, a); a = __builtin_fmaf(u.y, d.y, a);
                    a = __builtin_fmaf(u.z, d.z, a); a = __builtin_fmaf(u.w, d.w, a);
                }
                dws[e] = (a - pd[k]) * zinv[k];
            }
            __syncthreads();
            for (int rr = wave; rr < TILE; rr += TPB / 64) {
                const long long row = r0 + rr;
                if (row >= c1) continue;
                float t = 0.f;
                for (int k = lane; k < K; k += 64) t += ws[rr * K + k] * dws[rr * K + k];
                t = wsum(t);
                for (int k = lane; k < K; k += 64) {
                    const float p = ws[rr * K + k];
                    glogits[row * K + k] = p * (dws[rr * K + k] - t);
                }
            }
        }
        __syncthreads();
    }
}

// q_k / max(|q_k|, eps) of one prototype set into LDS rows (K, C)
__device__ void load_protos(const float *__restrict__ q, int K, int C, float *qn) {
    for (int k = threadIdx.x; k < K; k += TPB) {
        const float *r = q + (long long)k * C;
        float ss = 0.f;
        for (int c = 0; c < C; ++c) ss = __builtin_fmaf(r[c], r[c], ss);
        const float den = fmaxf(sqrtf(ss), NORM_EPS);
        for (int c = 0; c < C; ++c) qn[k * C + c] = r[c] / den;
    }
}

// thread (g, k): class k's normalised prototype in registers, rows g, g + G, ... of the tile (G = TPB / K groups); the x rows
// are LDS broadcasts, one b128 read per four FMAs
__global__ __launch_bounds__(TPB) void cos_forward_kernel(int K, int C, const float *__restrict__ x, const float *__restrict__ q,
                                                          int per_scene, const int *__restrict__ offset, float scale,
                                                          float *__restrict__ out) {
    __shared__ float4 xs4[COS_TILE * MAXC / 4];
    __shared__ float rden[COS_TILE];
    float *xs = (float *)xs4;
    const int j = blockIdx.x, s = blockIdx.y, CQ = C / 4;
    long long lo, hi;
    scene_rows(offset, s, lo, hi);
    const long long c0 = lo + (long long)j * CHUNK, c1 = min(hi, c0 + CHUNK);
    if (c0 >= c1) return;
    const int G = TPB / K, k = threadIdx.x % K, g = threadIdx.x / K;
    float4 qr[MAXC / 4];
    {
        const float4 *row = (const float4 *)(q + (per_scene ? (long long)s * K * C : 0) + (long long)k * C);
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < MAXC / 4; ++i) {
            qr[i] = i < CQ ? row[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            ss = __builtin_fmaf(qr[i].x, qr[i].x, ss); ss = __builtin_fmaf(qr[i].y, qr[i].y, ss);
            ss = __builtin_fmaf(qr[i].z, qr[i].z, ss); ss = __builtin_fmaf(qr[i].w, qr[i].w, ss);
        }
        const float den = fmaxf(sqrtf(ss), NORM_EPS);
#pragma unroll
        for (int i = 0; i < MAXC / 4; ++i) { qr[i].x /= den; qr[i].y /= den; qr[i].z /= den; qr[i].w /= den; }
    }
    for (long long r0 = c0; r0 < c1; r0 += COS_TILE) {
        for (int e = threadIdx.x; e < COS_TILE * CQ; e += TPB) {
            const int rr = e / CQ;
            xs4[e] = r0 + rr < c1 ? ((const float4 *)x)[(r0 + rr) * CQ + (e - rr * CQ)] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        if ((int)threadIdx.x < COS_TILE) {
            float ss = 0.f;
            for (int c = 0; c < C; ++c) ss = __builtin_fmaf(xs[threadIdx.x * C + c], xs[threadIdx.x * C + c], ss);
            rden[threadIdx.x] = fmaxf(sqrtf(ss), NORM_EPS);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < COS_TILE * C; e += TPB) xs[e] = xs[e] / rden[e / C];
        __syncthreads();
        if (g < G)
            for (int rr = g; rr < COS_TILE && r0 + rr < c1; rr += G) {
                float a = 0.f;
#pragma unroll
                for (int i = 0; i < MAXC / 4; ++i)
                    if (i < CQ) {
                        const float4 v = xs4[rr * CQ + i];
                        a = __builtin_fmaf(v.x, qr[i].x, a); a = __builtin_fmaf(v.y, qr[i].y, a);
                        a = __builtin_fmaf(v.z, qr[i].z, a); a = __builtin_fmaf(v.w, qr[i].w, a);
                    }
                out[(r0 + rr) * K + k] = scale * a;
            }
        __syncthreads();
    }
}

// gx (rows), and per workgroup the partial sum_n g_nk xhat_n (K x C) of the normalised prototypes' gradient
__global__ __launch_bounds__(TPB) void cos_backward_kernel(int K, int C, int J, const float *__restrict__ x,
                                                           const float *__restrict__ q, int per_scene,
                                                           const int *__restrict__ offset, float scale,
                                                           const float *__restrict__ dout, float *__restrict__ gx,
                                                           float *__restrict__ part) {
    __shared__ float4 qn4[MAXK * MAXC / 4];
    __shared__ float4 xn4[TILE * MAXC / 4], dxn4[TILE * MAXC / 4];
    __shared__ float g[TILE * MAXK];
    float *qn = (float *)qn4, *dxn = (float *)dxn4;
    __shared__ float rnorm[TILE], rdot[TILE];
    float *xn = (float *)xn4;
    const int j = blockIdx.x, s = blockIdx.y, CQ = C / 4, items = K * CQ;
    long long lo, hi;
    scene_rows(offset, s, lo, hi);
    const long long c0 = lo + (long long)j * CHUNK, c1 = min(hi, c0 + CHUNK);
    load_protos(q + (per_scene ? (long long)s * K * C : 0), K, C, qn);
    float4 acc[NI];
    int kk[NI], qq[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int e = threadIdx.x + i * TPB;
        kk[i] = e / CQ;
        qq[i] = e - kk[i] * CQ;
    }
    for (long long r0 = c0; r0 < c1; r0 += TILE) {
        load_rows(x, C, r0, c1, xn);
        for (int e = threadIdx.x; e < TILE * K; e += TPB) {
            const int rr = e / K, k = e - rr * K;
            g[e] = r0 + rr < c1 ? scale * dout[(r0 + rr) * K + k] : 0.f;
        }
        __syncthreads();
        if ((int)threadIdx.x < TILE) {
            float ss = 0.f;
            for (int c = 0; c < C; ++c) ss = __builtin_fmaf(xn[threadIdx.x * C + c], xn[threadIdx.x * C + c], ss);
            rnorm[threadIdx.x] = sqrtf(ss);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < TILE * C; e += TPB) xn[e] = xn[e] / fmaxf(rnorm[e / C], NORM_EPS);
        __syncthreads();
        for (int e = threadIdx.x; e < TILE * CQ; e += TPB) {
            const int rr = e / CQ, q4 = e - rr * CQ;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < K; ++k) {
                const float w = g[rr * K + k];
                const float4 v = qn4[k * CQ + q4];
                a.x = __builtin_fmaf(w, v.x, a.x); a.y = __builtin_fmaf(w, v.y, a.y);
                a.z = __builtin_fmaf(w, v.z, a.z); a.w = __builtin_fmaf(w, v.w, a.w);
            }
            dxn4[e] = a;
        }
        for (int rr = 0; rr < TILE; ++rr) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if (threadIdx.x + i * TPB < items) {
                    const float w = g[rr * K + kk[i]];
                    const float4 a = xn4[rr * CQ + qq[i]];
                    acc[i].x = __builtin_fmaf(w, a.x, acc[i].x); acc[i].y = __builtin_fmaf(w, a.y, acc[i].y);
                    acc[i].z = __builtin_fmaf(w, a.z, acc[i].z); acc[i].w = __builtin_fmaf(w, a.w, acc[i].w);
                }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < TILE) {
            float a = 0.f;
            for (int c = 0; c < C; ++c) a = __builtin_fmaf(xn[threadIdx.x * C + c], dxn[threadIdx.x * C + c], a);
            rdot[threadIdx.x] = a;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < TILE * C; e += TPB) {
            const int rr = e / C;
            if (r0 + rr >= c1) continue;
            const float nr = rnorm[rr];
            gx[(r0 + rr) * C + (e - rr * C)] = nr > NORM_EPS ? (dxn[e] - xn[e] * rdot[rr]) / nr : dxn[e] / NORM_EPS;
        }
        __syncthreads();
    }
    float *p = part + ((long long)s * J + j) * ((long long)K * C);
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (threadIdx.x + i * TPB < items) ((float4 *)p)[threadIdx.x + i * TPB] = acc[i];
}

// one wavefront per (set, k): the partial slabs of the set in order -> d qhat_k, then through q / max(|q|, eps)
__global__ __launch_bounds__(64) void cos_proto_finalize_kernel(int K, int C, int slabs_per_set, const float *__restrict__ part,
                                                                const float *__restrict__ q, float *__restrict__ gq) {
    const int k = blockIdx.x, set = blockIdx.y, c = threadIdx.x;
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
    const float nr = sqrtf(wsum(qv * qv));
    const float qh = qv / fmaxf(nr, NORM_EPS);
    const float dot = wsum(qh * d);
    if (c < C) gq[((long long)set * K + k) * C + c] = nr > NORM_EPS ? (d - qh * dot) / nr : d / NORM_EPS;
}

// one row of get_distill_loss: lse of pred, softmax of soft, the smoothed target; loss_n and the entropy weight
struct DistillRow {
    float v[MAXK / 64], sm[MAXK / 64], t[MAXK / 64];
    float lse, loss, ent;
    long long y;
};

__device__ void distill_row(int K, const float *__restrict__ pred, const float *__restrict__ soft,
                            const long long *__restrict__ label, long long row, DistillRow &d) {
    const int lane = threadIdx.x & 63;
    const float *pr = pred + row * K, *so = soft + row * K;
    float u[MAXK / 64], mp = -INFINITY, mu = -INFINITY;
#pragma unroll
    for (int i = 0; i < MAXK / 64; ++i) {
        const int k = lane + 64 * i;
        d.v[i] = k < K ? pr[k] : -INFINITY;
        u[i] = k < K ? so[k] : -INFINITY;
        mp = fmaxf(mp, d.v[i]);
        mu = fmaxf(mu, u[i]);
    }
    mp = wmax(mp);
    mu = wmax(mu);
    float sp = 0.f, su = 0.f;
#pragma unroll
    for (int i = 0; i < MAXK / 64; ++i) {
        const bool in = lane + 64 * i < K;
        sp += in ? expf(d.v[i] - mp) : 0.f;
        u[i] = in ? expf(u[i] - mu) : 0.f;
        su += u[i];
    }
    sp = wsum(sp);
    su = wsum(su);
    d.lse = mp + logf(sp);
    d.y = label[row];
    const long long hot = d.y == -1 ? 0 : d.y;  // an ignored row's one-hot lands on class 0 (its entropy weight is 0)
    float l = 0.f, e = 0.f;
#pragma unroll
    for (int i = 0; i < MAXK / 64; ++i) {
        const int k = lane + 64 * i;
        d.sm[i] = u[i] / su;
        d.t[i] = 0.5f * d.sm[i] + (k == hot ? 0.5f : 0.f);
        if (k < K) {
            l += (d.v[i] - d.lse) * d.t[i];
            e += d.sm[i] * logf(d.sm[i] + 1e-4f);
        }
    }
    d.loss = -wsum(l);
    d.ent = (d.y >= 0 && d.y < K) ? -wsum(e) : 0.f;
}

// per chunk of CHUNK rows: the per-class sums of loss * ent, ent and the row count, partial[chunk][3][K]
__global__ __launch_bounds__(TPB) void distill_partial_kernel(int n, int K, const float *__restrict__ pred,
                                                              const float *__restrict__ soft, const long long *__restrict__ label,
                                                              float *__restrict__ part) {
    __shared__ float le[CHUNK], en[CHUNK];
    __shared__ int yl[CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long c0 = (long long)blockIdx.x * CHUNK;
    for (int rr = wave; rr < CHUNK; rr += TPB / 64) {
        const long long row = c0 + rr;
        if (row >= n) {
            if (lane == 0) { le[rr] = 0.f; en[rr] = 0.f; yl[rr] = -1; }
            continue;
        }
        DistillRow d;
        distill_row(K, pred, soft, label, row, d);
        if (lane == 0) {
            le[rr] = d.loss * d.ent;
            en[rr] = d.ent;
            yl[rr] = (d.y >= 0 && d.y < K) ? (int)d.y : -1;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += TPB) {
        float a = 0.f, b = 0.f, c = 0.f;
        for (int rr = 0; rr < CHUNK; ++rr)
            if (yl[rr] == k) { a += le[rr]; b += en[rr]; c += 1.f; }
        float *p = part + (long long)blockIdx.x * 3 * K;
        p[k] = a;
        p[K + k] = b;
        p[2 * K + k] = c;
    }
}

// one wavefront per class: the chunks' partials (lane-strided, then a fixed shuffle tree) -> sums[3][K]
__global__ __launch_bounds__(64) void distill_class_kernel(int K, int chunks, const float *__restrict__ part,
                                                           float *__restrict__ sums) {
    const int k = blockIdx.x;
    float a = 0.f, b = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < chunks; i += 64) {
        const float *p = part + (long long)i * 3 * K;
        a += p[k];
        b += p[K + k];
        c += p[2 * K + k];
    }
    a = wsum(a); b = wsum(b); c = wsum(c);
    if (threadIdx.x == 0) { sums[k] = a; sums[K + k] = b; sums[2 * K + k] = c; }
}

// loss = sum over present classes (ascending) of num_k / (den_k + 1e-4), over (present count + 1e-4); coef_k = d loss / d
// (loss_n ent_n) of a row of class k
__global__ __launch_bounds__(64) void distill_finalize_kernel(int K, const float *__restrict__ sums, float *__restrict__ loss,
                                                              float *__restrict__ coef) {
    if (threadIdx.x != 0) return;
    float total = 0.f, present = 0.f;
    for (int k = 0; k < K; ++k)
        if (sums[2 * K + k] > 0.f) {
            total += sums[k] / (sums[K + k] + 1e-4f);
            present += 1.f;
        }
    loss[0] = total / (present + 1e-4f);
    for (int k = 0; k < K; ++k) coef[k] = sums[2 * K + k] > 0.f ? 1.f / (sums[K + k] + 1e-4f) / (present + 1e-4f) : 0.f;
}

// gpred_n = g * ent_n * coef_{y_n} * (softmax(pred_n) * sum(t_n) - t_n)
__global__ __launch_bounds__(TPB) void distill_backward_kernel(int n, int K, const float *__restrict__ pred,
                                                               const float *__restrict__ soft, const long long *__restrict__ label,
                                                               const float *__restrict__ coef, const float *__restrict__ g,
                                                               float *__restrict__ gpred) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * TPB + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * TPB) >> 6;
    for (long long row = wave; row < n; row += nwaves) {
        DistillRow d;
        distill_row(K, pred, soft, label, row, d);
        float ts = 0.f;
#pragma unroll
        for (int i = 0; i < MAXK / 64; ++i) ts += lane + 64 * i < K ? d.t[i] : 0.f;
        ts = wsum(ts);
        const float f = (d.y >= 0 && d.y < K) ? g[0] * d.ent * coef[d.y] : 0.f;  // (an ignored row: zero)
#pragma unroll
        for (int i = 0; i < MAXK / 64; ++i) {
            const int k = lane + 64 * i;
            if (k < K) gpred[row * K + k] = f * (expf(d.v[i] - d.lse) * ts - d.t[i]);
        }
    }
}

bool dims_ok(int K, int C) { return K >= 1 && K <= MAXK && C >= 4 && C <= MAXC && C % 4 == 0; }
int chunks_of(int max_rows) { return max_rows > 0 ? divup(max_rows, CHUNK) : 1; }
}  // namespace

extern "C" size_t cac_workspace_bytes(int b, int max_rows, int n, int k, int c) {
    if (b < 1 || max_rows < 0 || n < 0 || !dims_ok(k, c)) return 0;
    const size_t slabs = (size_t)b * chunks_of(max_rows);
    const size_t wsum = sizeof(float) * slabs * ((size_t)k * c + k);
    const size_t distill = sizeof(float) * ((size_t)divup(n > 0 ? n : 1, CHUNK) * 3 * k) + ptv2_align256(sizeof(float) * 3 * k);
    return ptv2_align256(wsum > distill ? wsum : distill) + 256;
}

extern "C" int cac_weighted_sum_forward_hip_launcher(int mode, int n, int b, int max_rows, int k, int c, const float *x,
                                                     const float *logits, const long long *label, const int *offset, float thr,
                                                     float eps, float *z, float *out, void *workspace, size_t workspace_bytes,
                                                     void *stream) {
    if ((mode != 0 && mode != 1) || n < 1 || b < 1 || max_rows < 1 || !dims_ok(k, c) || !x || !offset || !z || !out ||
        (mode == 0 && !logits) || (mode == 1 && !label))
        return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < cac_workspace_bytes(b, max_rows, n, k, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int J = chunks_of(max_rows);
    float *part = (float *)workspace;
    hipLaunchKernelGGL(wsum_partial_kernel, dim3(J, b), dim3(TPB), 0, st, mode, k, c, J, x, logits, label, offset, thr, part);
    const int nsets = mode == 0 ? b : 1, per = mode == 0 ? J : b * J;
    hipLaunchKernelGGL(wsum_finalize_kernel, dim3(divup((long long)nsets * k * (c + 1), TPB)), dim3(TPB), 0, st, k, c, nsets, per,
                       (const float *)part, eps, z, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int cac_weighted_sum_backward_hip_launcher(int mode, int n, int b, int max_rows, int k, int c, const float *x,
                                                      const float *logits, const long long *label, const int *offset, float thr,
                                                      float eps, const float *z, const float *out, const float *dout, float *gx,
                                                      float *glogits, void *stream) {
    if ((mode != 0 && mode != 1) || n < 1 || b < 1 || max_rows < 1 || !dims_ok(k, c) || !x || !offset || !z || !dout || !gx ||
        (mode == 0 && !logits) || (mode == 1 && (!label || glogits)) || (glogits && !out))
        return PTV2_ERR_ARG;
    hipLaunchKernelGGL(wsum_backward_kernel, dim3(chunks_of(max_rows), b), dim3(TPB), 0, (hipStream_t)stream, mode, k, c, x, logits,
                       label, offset, thr, eps, z, out, dout, gx, glogits);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int cac_cosine_forward_hip_launcher(int n, int b, int max_rows, int k, int c, const float *x, const float *q,
                                               int per_scene, const int *offset, float scale, float *out, void *stream) {
    if (n < 1 || b < 1 || max_rows < 1 || !dims_ok(k, c) || !x || !q || !offset || !out) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(cos_forward_kernel, dim3(chunks_of(max_rows), b), dim3(TPB), 0, (hipStream_t)stream, k, c, x, q, per_scene,
                       offset, scale, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int cac_cosine_backward_hip_launcher(int n, int b, int max_rows, int k, int c, const float *x, const float *q,
                                                int per_scene, const int *offset, float scale, const float *dout, float *gx,
                                                float *gq, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 1 || b < 1 || max_rows < 1 || !dims_ok(k, c) || !x || !q || !offset || !dout || !gx || !gq) return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < cac_workspace_bytes(b, max_rows, n, k, c)) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int J = chunks_of(max_rows);
    float *part = (float *)workspace;
    hipLaunchKernelGGL(cos_backward_kernel, dim3(J, b), dim3(TPB), 0, st, k, c, J, x, q, per_scene, offset, scale, dout, gx, part);
    hipLaunchKernelGGL(cos_proto_finalize_kernel, dim3(k, per_scene ? b : 1), dim3(64), 0, st, k, c, per_scene ? J : b * J,
                       (const float *)part, q, gq);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int cac_distill_forward_hip_launcher(int n, int k, const float *pred, const float *soft, const long long *label,
                                                float *loss, float *coef, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 1 || k < 1 || k > MAXK || !pred || !soft || !label || !loss || !coef) return PTV2_ERR_ARG;
    const int chunks = divup(n, CHUNK);
    const size_t part_bytes = sizeof(float) * (size_t)chunks * 3 * k;
    // the layout below: part at 0, sums (3 k floats) at the next 256-byte boundary
    if (!workspace || workspace_bytes < ptv2_align256(part_bytes) + sizeof(float) * 3 * k) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)workspace, *sums = (float *)((char *)workspace + ptv2_align256(part_bytes));
    hipLaunchKernelGGL(distill_partial_kernel, dim3(chunks), dim3(TPB), 0, st, n, k, pred, soft, label, part);
    hipLaunchKernelGGL(distill_class_kernel, dim3(k), dim3(64), 0, st, k, chunks, (const float *)part, sums);
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(64), 0, st, k, (const float *)sums, loss, coef);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int cac_distill_backward_hip_launcher(int n, int k, const float *pred, const float *soft, const long long *label,
                                                 const float *coef, const float *g, float *gpred, void *stream) {
    if (n < 1 || k < 1 || k > MAXK || !pred || !soft || !label || !coef || !g || !gpred) return PTV2_ERR_ARG;
    hipLaunchKernelGGL(distill_backward_kernel, dim3(std::min(divup(n, TPB / 64), 2048)), dim3(TPB), 0, (hipStream_t)stream, n, k,
                       pred, soft, label, coef, g, gpred);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
