// ao_amd/csrc/ptv1.hip -- Point Transformer V1's vector-attention layer (include/ptv2_ptv1_hip.h): forward and backward of
// everything between the q / k / v Linears and bn2, without a buffer of n * ns * C elements in either direction.
//
// Three training-mode BatchNorms sit in the chain, so the forward is four passes and the backward mirrors them; every pass
// recomputes what it needs of r, p_r, x_k[idx], x_v[idx] from x_*, coord and idx (gathers of a tensor that stays in cache):
//   forward   stats3 -> statsc -> u (+ its sums) -> out (BN_I, Lin, softmax, aggregation)
//   backward  logits (g of the BN_I output + sums, g w5) -> gu -> w2 (g w2, BN_C sums) -> rows (g x_q, g of the BN3 output,
//             g p3) -> gather (g x_k, g x_v over the inverse table) -> p0 (g p0)
// Sums across workgroups: each workgroup writes one record in a fixed order, a second launch adds the records in index order.
// The statistics and the BatchNorm-backward sums are accumulated in fp64; everything else is fp32.  No atomics.
// All matrix products run on the vector ALUs (the MFMA form of Lin(C -> I) is not built).
#include "common.h"
#include "../../include/ptv2_ptv1_hip.h"

#define PTV1_TPB 256
#define NSM PTV1_MAX_NS

namespace {

struct Ptv1Args {
    int n, ns, training;
    float eps;
    const float *xq, *xk, *xv, *coord;
    const int *idx;
    ptv1_params p;
    const float *mean3, *var3, *meanc, *varc, *meani, *vari;
};

// linear_p.0 and its norm, per thread (uniform values)
struct Ptv1P3 {
    float w[9], b[3], mean[3], rstd[3], g[3], be[3];
};

__device__ __forceinline__ float ptv1_rstd(float var, float eps) { return 1.0f / sqrtf(var + eps); }

// norm == false: the Linear alone (the pass that MAKES the statistics must not read them)
__device__ __forceinline__ Ptv1P3 ptv1_load_p3(const Ptv1Args &a, bool norm = true) {
    Ptv1P3 q;
    for (int k = 0; k < 9; ++k) q.w[k] = a.p.p0_w[k];
    for (int k = 0; k < 3; ++k) {
        q.b[k] = a.p.p0_b[k];
        q.mean[k] = norm ? a.mean3[k] : 0.0f;
        q.rstd[k] = norm ? ptv1_rstd(a.var3[k], a.eps) : 1.0f;
        q.g[k] = a.p.p1_g[k];
        q.be[k] = a.p.p1_b[k];
    }
    return q;
}

// rel of (point, neighbour j) and a = p0_w rel + p0_b
__device__ __forceinline__ void ptv1_rel_a(const Ptv1Args &a, const Ptv1P3 &q, int point, int j, float rel[3], float av[3]) {
    const bool valid = j >= 0;
    const int jj = valid ? j : point;
    for (int k = 0; k < 3; ++k) rel[k] = valid ? a.coord[(size_t)jj * 3 + k] - a.coord[(size_t)point * 3 + k] : 0.0f;
    for (int k = 0; k < 3; ++k)
        av[k] = fmaf(q.w[k * 3 + 2], rel[2], fmaf(q.w[k * 3 + 1], rel[1], fmaf(q.w[k * 3], rel[0], q.b[k])));
}
// xh = normalised a, y = the norm's output, h = ReLU(y)
__device__ __forceinline__ void ptv1_bn3(const Ptv1P3 &q, const float av[3], float xh[3], float y[3], float h[3]) {
    for (int k = 0; k < 3; ++k) {
        xh[k] = (av[k] - q.mean[k]) * q.rstd[k];
        y[k] = fmaf(xh[k], q.g[k], q.be[k]);
        h[k] = fmaxf(y[k], 0.0f);
    }
}

// the slots of one point, in LDS
struct Ptv1Point {
    int j[NSM];
    float rel[NSM][3], xh[NSM][3], y[NSM][3], h[NSM][3];
};
// threads 0 .. ns-1 fill it; the caller synchronises before and after
__device__ __forceinline__ void ptv1_point(const Ptv1Args &a, const Ptv1P3 &q, int point, Ptv1Point &pt) {
    const int s = threadIdx.x;
    if (s < a.ns) {
        const int j = a.idx[(size_t)point * a.ns + s];
        float rel[3], av[3], xh[3], y[3], h[3];
        ptv1_rel_a(a, q, point, j, rel, av);
        ptv1_bn3(q, av, xh, y, h);
        pt.j[s] = j;
        for (int k = 0; k < 3; ++k) { pt.rel[s][k] = rel[k]; pt.xh[s][k] = xh[k]; pt.y[s][k] = y[k]; pt.h[s][k] = h[k]; }
    }
}

// one channel's constants of linear_p.3 and BN_C
struct Ptv1Chan {
    float w1[3], b1, mean, rstd, g, be;
};
__device__ __forceinline__ Ptv1Chan ptv1_load_chan(const Ptv1Args &a, int c, bool norm = true) {
    Ptv1Chan ch;
    for (int k = 0; k < 3; ++k) ch.w1[k] = a.p.p3_w[c * 3 + k];
    ch.b1 = a.p.p3_b[c];
    ch.mean = norm ? a.meanc[c] : 0.0f;
    ch.rstd = norm ? ptv1_rstd(a.varc[c], a.eps) : 1.0f;
    ch.g = a.p.w0_g[c];
    ch.be = a.p.w0_b[c];
    return ch;
}
__device__ __forceinline__ float ptv1_pr(const Ptv1Chan &ch, const float h[3]) {
    return fmaf(ch.w1[2], h[2], fmaf(ch.w1[1], h[1], fmaf(ch.w1[0], h[0], ch.b1)));
}
// r of (point, neighbour j, channel c)
template <int C>
__device__ __forceinline__ float ptv1_r(const Ptv1Args &a, const Ptv1Chan &ch, int point, int j, int c, const float h[3]) {
    const float key = ptv2_ld_or_zero(a.xk + (size_t)(j >= 0 ? j : 0) * C + c, j >= 0);
    return key - a.xq[(size_t)point * C + c] + ptv1_pr(ch, h);
}

// the sum of v over the workgroup, in a fixed tree; `lds` has PTV1_TPB elements
template <class T>
__device__ __forceinline__ T ptv1_block_sum(T v, T *lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int o = PTV1_TPB / 2; o > 0; o >>= 1) {
        if (t < o) lds[t] += lds[t + o];
        __syncthreads();
    }
    const T r = lds[0];
    __syncthreads();
    return r;
}
// threads are laid out (group, lane) with `lanes` lanes; lane l < lanes of group 0 receives the sum over the groups, in
// group order.  Other threads receive their own value.
template <class T>
__device__ __forceinline__ T ptv1_group_sum(T v, T *lds, int lanes) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    if (t < lanes) {
        T s = lds[t];
        for (int g = 1; g < PTV1_TPB / lanes; ++g) s += lds[g * lanes + t];
        v = s;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- records

// out[j] = sum over the records b (in order) of part[b * stride + j], j < len
template <class T>
__global__ void ptv1_reduce_kernel(const T *__restrict__ part, int nblk, int stride, int len, float *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= len) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += (double)part[(size_t)b * stride + j];
    out[j] = (float)s;
}

// records of [len sums][len sums of squares] -> mean, biased variance, and the running buffers
__global__ void ptv1_stats_finalize_kernel(const double *__restrict__ part, int nblk, int len, double rows, float *mean,
                                           float *var, float *run_mean, float *run_var, long long *batches, float momentum) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= len) return;
    double s = 0.0, q = 0.0;
    for (int b = 0; b < nblk; ++b) {
        s += part[(size_t)b * 2 * len + j];
        q += part[(size_t)b * 2 * len + len + j];
    }
    const double m = s / rows;
    double v = q / rows - m * m;
    if (v < 0.0) v = 0.0;
    mean[j] = (float)m;
    var[j] = (float)v;
    if (run_mean) run_mean[j] = (float)((1.0 - (double)momentum) * (double)run_mean[j] + (double)momentum * m);
    if (run_var) run_var[j] = (float)((1.0 - (double)momentum) * (double)run_var[j] + (double)momentum * (v * rows / (rows - 1.0)));
    if (j == 0 && batches) *batches += 1;
}

__global__ void ptv1_transpose_kernel(const float *__restrict__ src, int rows, int cols, float *__restrict__ dst) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * cols) return;
    dst[(size_t)(e % cols) * rows + e / cols] = src[e];
}

// ---------------------------------------------------------------------------------------------------------------- forward

// pass 1: sums of a over the n * ns rows.  part[b][0..3) sums, [3..6) sums of squares
__global__ __launch_bounds__(PTV1_TPB) void ptv1_stats3_kernel(Ptv1Args a, double *__restrict__ part) {
    __shared__ double red[PTV1_TPB];
    Ptv1P3 q = ptv1_load_p3(a, false);
    double s[3] = {0, 0, 0}, sq[3] = {0, 0, 0};
    const long long rows = (long long)a.n * a.ns;
    for (long long r = (long long)blockIdx.x * PTV1_TPB + threadIdx.x; r < rows; r += (long long)gridDim.x * PTV1_TPB) {
        float rel[3], av[3];
        ptv1_rel_a(a, q, (int)(r / a.ns), a.idx[r], rel, av);
        for (int k = 0; k < 3; ++k) { s[k] += av[k]; sq[k] += (double)av[k] * av[k]; }
    }
    for (int k = 0; k < 3; ++k) {
        const double ts = ptv1_block_sum(s[k], red), tq = ptv1_block_sum(sq[k], red);
        if (threadIdx.x == 0) { part[blockIdx.x * 6 + k] = ts; part[blockIdx.x * 6 + 3 + k] = tq; }
    }
}

// the channel layout of the per-point kernels: CT lanes over the channels, NCH channels per thread, G groups over the slots
template <int C>
struct Ptv1Lay {
    static constexpr int I = C / PTV1_SHARE;
    static constexpr int CT = C < PTV1_TPB ? C : PTV1_TPB;
    static constexpr int NCH = C / CT;
    static constexpr int G = PTV1_TPB / CT;
};

// pass 2: sums of r per channel.  part[b][0..C) sums, [C..2C) sums of squares
template <int C>
__global__ __launch_bounds__(PTV1_TPB) void ptv1_statsc_kernel(Ptv1Args a, double *__restrict__ part) {
    using L = Ptv1Lay<C>;
    __shared__ Ptv1Point pt;
    __shared__ double red[PTV1_TPB];
    const int cl = threadIdx.x % L::CT, g = threadIdx.x / L::CT;
    const Ptv1P3 q = ptv1_load_p3(a);
    Ptv1Chan ch[L::NCH];
    double s[L::NCH], sq[L::NCH];
    for (int k = 0; k < L::NCH; ++k) { ch[k] = ptv1_load_chan(a, cl + k * L::CT, false); s[k] = 0; sq[k] = 0; }
    for (int point = blockIdx.x; point < a.n; point += gridDim.x) {
        __syncthreads();
        ptv1_point(a, q, point, pt);
        __syncthreads();
        for (int sl = g; sl < a.ns; sl += L::G)
            for (int k = 0; k < L::NCH; ++k) {
                const float r = ptv1_r<C>(a, ch[k], point, pt.j[sl], cl + k * L::CT, pt.h[sl]);
                s[k] += r;
                sq[k] += (double)r * r;
            }
    }
    for (int k = 0; k < L::NCH; ++k) {
        const double ts = ptv1_group_sum(s[k], red, L::CT), tq = ptv1_group_sum(sq[k], red, L::CT);
        if (g == 0) {
            part[(size_t)blockIdx.x * 2 * C + cl + k * L::CT] = ts;
            part[(size_t)blockIdx.x * 2 * C + C + cl + k * L::CT] = tq;
        }
    }
}

// pass 3: u = w2_w ReLU(BN_C(r)) + w2_b, and its sums.  w2t is w2_w transposed, (C, I).  part[b][0..I) sums, [I..2I) squares
template <int C>
__global__ __launch_bounds__(PTV1_TPB) void ptv1_u_kernel(Ptv1Args a, const float *__restrict__ w2t, float *__restrict__ u,
                                                           double *__restrict__ part) {
    using L = Ptv1Lay<C>;
    constexpr int I = L::I;
    __shared__ Ptv1Point pt;
    __shared__ float T[NSM][C + 1];
    __shared__ double red[PTV1_TPB];
    const int cl = threadIdx.x % L::CT, g = threadIdx.x / L::CT, i = threadIdx.x % I;
    const Ptv1P3 q = ptv1_load_p3(a);
    Ptv1Chan ch[L::NCH];
    for (int k = 0; k < L::NCH; ++k) ch[k] = ptv1_load_chan(a, cl + k * L::CT);
    const float b2 = a.p.w2_b[i];
    double s = 0, sq = 0;
    for (int point = blockIdx.x; point < a.n; point += gridDim.x) {
        __syncthreads();
        ptv1_point(a, q, point, pt);
        __syncthreads();
        for (int sl = g; sl < a.ns; sl += L::G)
            for (int k = 0; k < L::NCH; ++k) {
                const int c = cl + k * L::CT;
                const float r = ptv1_r<C>(a, ch[k], point, pt.j[sl], c, pt.h[sl]);
                T[sl][c] = fmaxf(fmaf((r - ch[k].mean) * ch[k].rstd, ch[k].g, ch[k].be), 0.0f);
            }
        __syncthreads();
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) {  // o = slot * I + i
            const int sl = o / I;
            float acc = b2;
            for (int c = 0; c < C; ++c) acc = fmaf(w2t[c * I + i], T[sl][c], acc);
            u[(size_t)point * a.ns * I + o] = acc;
            s += acc;
            sq += (double)acc * acc;
        }
    }
    const double ts = ptv1_group_sum(s, red, I), tq = ptv1_group_sum(sq, red, I);
    if (threadIdx.x < I) {
        part[(size_t)blockIdx.x * 2 * I + i] = ts;
        part[(size_t)blockIdx.x * 2 * I + I + i] = tq;
    }
}

// pass 4: z = w5_w ReLU(BN_I(u)) + w5_b, w = softmax over the slots, out = sum of (x_v[idx] + p_r) * w.  w3t is w5_w transposed
template <int C>
__global__ __launch_bounds__(PTV1_TPB) void ptv1_out_kernel(Ptv1Args a, const float *__restrict__ w3t, const float *__restrict__ u,
                                                             float *__restrict__ wsave, float *__restrict__ out) {
    using L = Ptv1Lay<C>;
    constexpr int I = L::I;
    __shared__ Ptv1Point pt;
    __shared__ float V[NSM][I], Z[NSM][I], W[NSM][I];
    __shared__ float red[PTV1_TPB];
    const int cl = threadIdx.x % L::CT, g = threadIdx.x / L::CT, i = threadIdx.x % I;
    const Ptv1P3 q = ptv1_load_p3(a);
    Ptv1Chan ch[L::NCH];
    for (int k = 0; k < L::NCH; ++k) ch[k] = ptv1_load_chan(a, cl + k * L::CT);
    const float mi = a.meani[i], ri = ptv1_rstd(a.vari[i], a.eps), gi = a.p.w3_g[i], bi = a.p.w3_b[i], b3 = a.p.w5_b[i];
    for (int point = blockIdx.x; point < a.n; point += gridDim.x) {
        const size_t base = (size_t)point * a.ns * I;
        __syncthreads();
        ptv1_point(a, q, point, pt);
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB)
            V[o / I][i] = fmaxf(fmaf((u[base + o] - mi) * ri, gi, bi), 0.0f);
        __syncthreads();
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) {
            const int sl = o / I;
            float acc = b3;
            for (int k = 0; k < I; ++k) acc = fmaf(w3t[k * I + i], V[sl][k], acc);
            Z[sl][i] = acc;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) {
            const int sl = o / I;
            float m = Z[0][i];
            for (int t = 1; t < a.ns; ++t) m = fmaxf(m, Z[t][i]);
            float den = 0.0f;
            for (int t = 0; t < a.ns; ++t) den += expf(Z[t][i] - m);
            const float w = expf(Z[sl][i] - m) / den;
            W[sl][i] = w;
            wsave[base + o] = w;
        }
        __syncthreads();
        float acc[L::NCH];
        for (int k = 0; k < L::NCH; ++k) acc[k] = 0.0f;
        for (int sl = g; sl < a.ns; sl += L::G) {
            const int j = pt.j[sl];
            for (int k = 0; k < L::NCH; ++k) {
                const int c = cl + k * L::CT;
                const float val = ptv2_ld_or_zero(a.xv + (size_t)(j >= 0 ? j : 0) * C + c, j >= 0) + ptv1_pr(ch[k], pt.h[sl]);
                acc[k] = fmaf(val, W[sl][c % I], acc[k]);
            }
        }
        for (int k = 0; k < L::NCH; ++k) {
            const float t = L::G > 1 ? ptv1_group_sum(acc[k], red, L::CT) : acc[k];
            if (g == 0) out[(size_t)point * C + cl + k * L::CT] = t;
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- backward

// pass 1: from g_out to gy = the gradient of the BN_I output, (n, ns, I).  partd[b]: [0..I) sum gy * xhat (g w3_g), [I..2I)
// sum gy (g w3_b), [2I..3I) sum gz (g w5_b); partw[b]: (I, I) sum gz[i] v[k] (g w5_w)
template <int C>
__global__ __launch_bounds__(PTV1_TPB) void ptv1_bwd_logits_kernel(Ptv1Args a, const float *__restrict__ u,
                                                                    const float *__restrict__ wsave, const float *__restrict__ gout,
                                                                    float *__restrict__ gy_out, double *__restrict__ partd,
                                                                    float *__restrict__ partw) {
    using L = Ptv1Lay<C>;
    constexpr int I = L::I;
    constexpr int MW = (I * I + PTV1_TPB - 1) / PTV1_TPB;
    __shared__ Ptv1Point pt;
    __shared__ float V[NSM][I], W[NSM][I], GW[NSM][I], GZ[NSM][I];
    __shared__ double red[PTV1_TPB];
    const int i = threadIdx.x % I;
    const Ptv1P3 q = ptv1_load_p3(a);
    const float mi = a.meani[i], ri = ptv1_rstd(a.vari[i], a.eps), gi = a.p.w3_g[i], bi = a.p.w3_b[i];
    float accw[MW];
    for (int m = 0; m < MW; ++m) accw[m] = 0.0f;
    double sg = 0, sb = 0, sb3 = 0;
    for (int point = blockIdx.x; point < a.n; point += gridDim.x) {
        const size_t base = (size_t)point * a.ns * I;
        __syncthreads();
        ptv1_point(a, q, point, pt);
        __syncthreads();
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) {
            const int sl = o / I, j = pt.j[sl];
            V[sl][i] = fmaxf(fmaf((u[base + o] - mi) * ri, gi, bi), 0.0f);
            W[sl][i] = wsave[base + o];
            float gw = 0.0f;
            for (int sh = 0; sh < PTV1_SHARE; ++sh) {
                const int c = sh * I + i;
                const Ptv1Chan ch = ptv1_load_chan(a, c, false);
                const float val = ptv2_ld_or_zero(a.xv + (size_t)(j >= 0 ? j : 0) * C + c, j >= 0) + ptv1_pr(ch, pt.h[sl]);
                gw = fmaf(gout[(size_t)point * C + c], val, gw);
            }
            GW[sl][i] = gw;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) {
            const int sl = o / I;
            float dot = 0.0f;
            for (int t = 0; t < a.ns; ++t) dot = fmaf(W[t][i], GW[t][i], dot);
            const float gz = W[sl][i] * (GW[sl][i] - dot);
            GZ[sl][i] = gz;
            sb3 += gz;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) {  // here i is the INPUT channel k of w5_w
            const int sl = o / I;
            float gv = 0.0f;
            for (int i2 = 0; i2 < I; ++i2) gv = fmaf(a.p.w5_w[i2 * I + i], GZ[sl][i2], gv);
            const float xh = (u[base + o] - mi) * ri;
            const float gy = fmaf(xh, gi, bi) > 0.0f ? gv : 0.0f;
            gy_out[base + o] = gy;
            sb += gy;
            sg += (double)gy * xh;
        }
        for (int m = 0; m < MW; ++m) {
            const int e = threadIdx.x + m * PTV1_TPB;
            if (e < I * I) {
                float acc = accw[m];
                for (int t = 0; t < a.ns; ++t) acc = fmaf(GZ[t][e / I], V[t][e % I], acc);
                accw[m] = acc;
            }
        }
    }
    for (int m = 0; m < MW; ++m) {
        const int e = threadIdx.x + m * PTV1_TPB;
        if (e < I * I) partw[(size_t)blockIdx.x * I * I + e] = accw[m];
    }
    const double tg = ptv1_group_sum(sg, red, I), tb = ptv1_group_sum(sb, red, I), t3 = ptv1_group_sum(sb3, red, I);
    if (threadIdx.x < I) {
        partd[(size_t)blockIdx.x * 3 * I + i] = tg;
        partd[(size_t)blockIdx.x * 3 * I + I + i] = tb;
        partd[(size_t)blockIdx.x * 3 * I + 2 * I + i] = t3;
    }
}

// gy -> gu = the gradient of u, in place; part[b][0..I) sum gu (g w2_b).  sum_g / sum_b: the reduced sums of pass 1
__global__ __launch_bounds__(PTV1_TPB) void ptv1_gu_kernel(Ptv1Args a, int I, const float *__restrict__ u, const float *__restrict__ sum_g,
                                                            const float *__restrict__ sum_b, float *__restrict__ g,
                                                            double *__restrict__ part) {
    __shared__ double red[PTV1_TPB];
    const int i = threadIdx.x % I;
    const float mi = a.meani[i], ri = ptv1_rstd(a.vari[i], a.eps), coef = a.p.w3_g[i] * ri;
    const double rows = (double)a.n * a.ns;
    const float m1 = a.training ? (float)(sum_b[i] / rows) : 0.0f, m2 = a.training ? (float)(sum_g[i] / rows) : 0.0f;
    const long long total = (long long)a.n * a.ns * I;
    double s = 0;
    for (long long e = (long long)blockIdx.x * PTV1_TPB + threadIdx.x; e < total; e += (long long)gridDim.x * PTV1_TPB) {
        const float xh = (u[e] - mi) * ri;
        const float gu = coef * (g[e] - m1 - xh * m2);
        g[e] = gu;
        s += gu;
    }
    const double ts = ptv1_group_sum(s, red, I);
    if (threadIdx.x < I) part[(size_t)blockIdx.x * I + i] = ts;
}

// pass 2, per (workgroup of points, chunk of CC channels): partw[b]: (I, C) sum gu[i] t[c] (g w2_w); partd[b]: [0..C) sum
// grh * rhat (g w0_g), [C..2C) sum grh (g w0_b), grh = the gradient of the BN_C output
template <int C>
__global__ __launch_bounds__(PTV1_TPB) void ptv1_bwd_w2_kernel(Ptv1Args a, const float *__restrict__ gu, float *__restrict__ partw,
                                                                double *__restrict__ partd) {
    constexpr int I = C / PTV1_SHARE;
    constexpr int CC = C < 64 ? C : 64, SG = PTV1_TPB / CC, KW = (I + SG - 1) / SG;
    __shared__ Ptv1Point pt;
    __shared__ float GU[NSM][I], T[NSM][CC + 1];
    __shared__ double red[PTV1_TPB];
    const int cl = threadIdx.x % CC, sg = threadIdx.x / CC, c = blockIdx.y * CC + cl;
    const Ptv1P3 q = ptv1_load_p3(a);
    const Ptv1Chan ch = ptv1_load_chan(a, c);
    float acc[KW];
    for (int k = 0; k < KW; ++k) acc[k] = 0.0f;
    double s1 = 0, s2 = 0;
    for (int point = blockIdx.x; point < a.n; point += gridDim.x) {
        const size_t base = (size_t)point * a.ns * I;
        __syncthreads();
        ptv1_point(a, q, point, pt);
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) GU[o / I][o % I] = gu[base + o];
        __syncthreads();
        for (int sl = sg; sl < a.ns; sl += SG) {
            const float r = ptv1_r<C>(a, ch, point, pt.j[sl], c, pt.h[sl]);
            const float rh = (r - ch.mean) * ch.rstd, y = fmaf(rh, ch.g, ch.be);
            T[sl][cl] = fmaxf(y, 0.0f);
            float gt = 0.0f;
            for (int i = 0; i < I; ++i) gt = fmaf(a.p.w2_w[i * C + c], GU[sl][i], gt);
            const float grh = y > 0.0f ? gt : 0.0f;
            s1 += grh;
            s2 += (double)grh * rh;
        }
        __syncthreads();
        for (int k = 0; k < KW; ++k) {
            const int i = sg + k * SG;
            if (i < I) {
                float t = acc[k];
                for (int sl = 0; sl < a.ns; ++sl) t = fmaf(GU[sl][i], T[sl][cl], t);
                acc[k] = t;
            }
        }
    }
    for (int k = 0; k < KW; ++k) {
        const int i = sg + k * SG;
        if (i < I) partw[((size_t)blockIdx.x * I + i) * C + c] = acc[k];
    }
    const double t2 = ptv1_group_sum(s2, red, CC), t1 = ptv1_group_sum(s1, red, CC);
    if (sg == 0) {
        partd[(size_t)blockIdx.x * 2 * C + c] = t2;
        partd[(size_t)blockIdx.x * 2 * C + C + c] = t1;
    }
}

// the gradient of r for one element: through ReLU, BN_C (sum_g / sum_b over rows: the reduced sums of pass 2)
struct Ptv1ChanB {
    float coef, m1, m2;
};
__device__ __forceinline__ Ptv1ChanB ptv1_load_chan_b(const Ptv1Args &a, const Ptv1Chan &ch, int c, const float *sum_g,
                                                       const float *sum_b) {
    const double rows = (double)a.n * a.ns;
    Ptv1ChanB b;
    b.coef = ch.g * ch.rstd;
    b.m1 = a.training ? (float)(sum_b[c] / rows) : 0.0f;
    b.m2 = a.training ? (float)(sum_g[c] / rows) : 0.0f;
    return b;
}
template <int C>
__device__ __forceinline__ float ptv1_gr(const Ptv1Args &a, const Ptv1Chan &ch, const Ptv1ChanB &cb, float r, int c,
                                         const float *gu_row) {
    constexpr int I = C / PTV1_SHARE;
    const float rh = (r - ch.mean) * ch.rstd, y = fmaf(rh, ch.g, ch.be);
    float gt = 0.0f;
    for (int i = 0; i < I; ++i) gt = fmaf(a.p.w2_w[i * C + c], gu_row[i], gt);
    const float grh = y > 0.0f ? gt : 0.0f;
    return cb.coef * (grh - cb.m1 - rh * cb.m2);
}

// pass 3 by query point: g x_q, ga = the gradient of the BN3 output (n, ns, 3); partw[b]: (C, 3) g p3_w then (C) g p3_b;
// partd[b]: [0..3) sum ga * xhat (g p1_g), [3..6) sum ga (g p1_b)
template <int C>
__global__ __launch_bounds__(PTV1_TPB) void ptv1_bwd_rows_kernel(Ptv1Args a, const float *__restrict__ gu, const float *__restrict__ wsave,
                                                                  const float *__restrict__ gout, const float *__restrict__ sum_g,
                                                                  const float *__restrict__ sum_b, float *__restrict__ gxq,
                                                                  float *__restrict__ ga_out, float *__restrict__ partw,
                                                                  double *__restrict__ partd) {
    using L = Ptv1Lay<C>;
    constexpr int I = L::I;
    __shared__ Ptv1Point pt;
    __shared__ float GU[NSM][I], W[NSM][I], GP[NSM][C];
    __shared__ float red[PTV1_TPB];
    __shared__ double red3[NSM][6];
    const int cl = threadIdx.x % L::CT, g = threadIdx.x / L::CT;
    const Ptv1P3 q = ptv1_load_p3(a);
    Ptv1Chan ch[L::NCH];
    Ptv1ChanB cb[L::NCH];
    float gw1[L::NCH][4];
    for (int k = 0; k < L::NCH; ++k) {
        ch[k] = ptv1_load_chan(a, cl + k * L::CT);
        cb[k] = ptv1_load_chan_b(a, ch[k], cl + k * L::CT, sum_g, sum_b);
        for (int m = 0; m < 4; ++m) gw1[k][m] = 0.0f;
    }
    const int hs = threadIdx.x / 16, hq = threadIdx.x % 16;  // the (slot, sub-lane) layout of the g h sums
    double s3[6] = {0, 0, 0, 0, 0, 0};
    for (int point = blockIdx.x; point < a.n; point += gridDim.x) {
        const size_t base = (size_t)point * a.ns * I;
        __syncthreads();
        ptv1_point(a, q, point, pt);
        for (int o = threadIdx.x; o < a.ns * I; o += PTV1_TPB) { GU[o / I][o % I] = gu[base + o]; W[o / I][o % I] = wsave[base + o]; }
        __syncthreads();
        float gq[L::NCH];
        for (int k = 0; k < L::NCH; ++k) gq[k] = 0.0f;
        for (int sl = g; sl < a.ns; sl += L::G)
            for (int k = 0; k < L::NCH; ++k) {
                const int c = cl + k * L::CT;
                const float r = ptv1_r<C>(a, ch[k], point, pt.j[sl], c, pt.h[sl]);
                const float gr = ptv1_gr<C>(a, ch[k], cb[k], r, c, GU[sl]);
                gq[k] -= gr;
                const float gp = fmaf(gout[(size_t)point * C + c], W[sl][c % I], gr);
                GP[sl][c] = gp;
                for (int m = 0; m < 3; ++m) gw1[k][m] = fmaf(gp, pt.h[sl][m], gw1[k][m]);
                gw1[k][3] += gp;
            }
        for (int k = 0; k < L::NCH; ++k) {
            const float t = L::G > 1 ? ptv1_group_sum(gq[k], red, L::CT) : gq[k];
            if (g == 0) gxq[(size_t)point * C + cl + k * L::CT] = t;
        }
        __syncthreads();
        float gh[3] = {0, 0, 0};
        if (hs < a.ns)
            for (int c = hq; c < C; c += 16) {
                const float gp = GP[hs][c];
                for (int m = 0; m < 3; ++m) gh[m] = fmaf(a.p.p3_w[c * 3 + m], gp, gh[m]);
            }
        for (int m = 0; m < 3; ++m)
            for (int o = 8; o > 0; o >>= 1) gh[m] += __shfl_xor(gh[m], o, 16);
        if (hs < a.ns && hq == 0)
            for (int m = 0; m < 3; ++m) {
                const float ga = pt.y[hs][m] > 0.0f ? gh[m] : 0.0f;
                ga_out[((size_t)point * a.ns + hs) * 3 + m] = ga;
                s3[m] += (double)ga * pt.xh[hs][m];
                s3[3 + m] += ga;
            }
    }
    for (int k = 0; k < L::NCH; ++k)
        for (int m = 0; m < 4; ++m) {
            const float t = L::G > 1 ? ptv1_group_sum(gw1[k][m], red, L::CT) : gw1[k][m];
            const int c = cl + k * L::CT;
            if (g == 0) partw[(size_t)blockIdx.x * 4 * C + (m < 3 ? c * 3 + m : 3 * C + c)] = t;
        }
    __syncthreads();
    if (hq == 0)
        for (int m = 0; m < 6; ++m) red3[hs][m] = s3[m];
    __syncthreads();
    if (threadIdx.x < 6) {
        double t = 0;
        for (int sl = 0; sl < NSM; ++sl) t += red3[sl][threadIdx.x];
        partd[(size_t)blockIdx.x * 6 + threadIdx.x] = t;
    }
}

// pass 3 by neighbour: g x_k[m] and g x_v[m] as sums over the slots that point at m, in the inverse table's order
template <int C>
__global__ __launch_bounds__(PTV1_TPB) void ptv1_bwd_gather_kernel(Ptv1Args a, const int *__restrict__ inv_ptr,
                                                                    const int *__restrict__ inv_rows, const float *__restrict__ gu,
                                                                    const float *__restrict__ wsave, const float *__restrict__ gout,
                                                                    const float *__restrict__ sum_g, const float *__restrict__ sum_b,
                                                                    float *__restrict__ gxk, float *__restrict__ gxv) {
    using L = Ptv1Lay<C>;
    constexpr int I = L::I;
    const int cl = threadIdx.x % L::CT, g = threadIdx.x / L::CT;
    const int m = blockIdx.x * L::G + g;
    if (m >= a.n) return;
    const Ptv1P3 q = ptv1_load_p3(a);
    Ptv1Chan ch[L::NCH];
    Ptv1ChanB cb[L::NCH];
    float ak[L::NCH], av[L::NCH];
    for (int k = 0; k < L::NCH; ++k) {
        ch[k] = ptv1_load_chan(a, cl + k * L::CT);
        cb[k] = ptv1_load_chan_b(a, ch[k], cl + k * L::CT, sum_g, sum_b);
        ak[k] = 0.0f;
        av[k] = 0.0f;
    }
    const long long rows = (long long)a.n * a.ns;
    for (int e = inv_ptr[m]; e < inv_ptr[m + 1]; ++e) {
        const int row = inv_rows[e];
        if (row < 0 || row >= rows) continue;  // never for a table built from idx
        const int point = row / a.ns;
        float rel[3], avv[3], xh[3], y[3], h[3];
        ptv1_rel_a(a, q, point, m, rel, avv);
        ptv1_bn3(q, avv, xh, y, h);
        for (int k = 0; k < L::NCH; ++k) {
            const int c = cl + k * L::CT;
            const float r = ptv1_r<C>(a, ch[k], point, m, c, h);
            ak[k] += ptv1_gr<C>(a, ch[k], cb[k], r, c, gu + (size_t)row * I);
            av[k] = fmaf(gout[(size_t)point * C + c], wsave[(size_t)row * I + c % I], av[k]);
        }
    }
    for (int k = 0; k < L::NCH; ++k) {
        gxk[(size_t)m * C + cl + k * L::CT] = ak[k];
        gxv[(size_t)m * C + cl + k * L::CT] = av[k];
    }
}

// pass 4: through BN3 to linear_p.0.  part[b]: [0..9) g p0_w, [9..12) g p0_b.  sum_g / sum_b: the reduced sums of pass 3
__global__ __launch_bounds__(PTV1_TPB) void ptv1_bwd_p0_kernel(Ptv1Args a, const float *__restrict__ ga, const float *__restrict__ sum_g,
                                                                const float *__restrict__ sum_b, double *__restrict__ part) {
    __shared__ double red[PTV1_TPB];
    const Ptv1P3 q = ptv1_load_p3(a);
    const double nrows = (double)a.n * a.ns;
    float m1[3], m2[3];
    for (int k = 0; k < 3; ++k) {
        m1[k] = a.training ? (float)(sum_b[k] / nrows) : 0.0f;
        m2[k] = a.training ? (float)(sum_g[k] / nrows) : 0.0f;
    }
    double acc[12];
    for (int k = 0; k < 12; ++k) acc[k] = 0;
    const long long rows = (long long)a.n * a.ns;
    for (long long r = (long long)blockIdx.x * PTV1_TPB + threadIdx.x; r < rows; r += (long long)gridDim.x * PTV1_TPB) {
        float rel[3], av[3];
        ptv1_rel_a(a, q, (int)(r / a.ns), a.idx[r], rel, av);
        for (int k = 0; k < 3; ++k) {
            const float xh = (av[k] - q.mean[k]) * q.rstd[k];
            const float g = q.g[k] * q.rstd[k] * (ga[r * 3 + k] - m1[k] - xh * m2[k]);
            for (int l = 0; l < 3; ++l) acc[k * 3 + l] += (double)g * rel[l];
            acc[9 + k] += g;
        }
    }
    for (int k = 0; k < 12; ++k) {
        const double t = ptv1_block_sum(acc[k], red);
        if (threadIdx.x == 0) part[blockIdx.x * 12 + k] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host

static int imin(long long a, long long b) { return (int)(a < b ? a : b); }
static int imax1(long long a) { return (int)(a < 1 ? 1 : a); }

// the grids: functions of the sizes alone, so that two calls add their records in the same order
struct Ptv1Plan {
    int n, ns, c, i;
    int nb_rows;    // stats3, p0: workgroups over the n * ns rows
    int nb_fwd;     // statsc, u, out: workgroups over the points
    int nb_logits;  // bwd_logits: a record holds (I, I) floats
    int nb_gu;      // gu: workgroups over the n * ns * I elements
    int nb_w2;      // bwd_w2: a record holds (I, C) floats
    int nb_prow;    // bwd_rows: a record holds 4 C floats
};
static Ptv1Plan ptv1_plan(long long n, int ns, int c) {
    Ptv1Plan p;
    p.n = (int)n; p.ns = ns; p.c = c; p.i = c / PTV1_SHARE;
    const long long budget = 2ll << 20;  // bytes of one family of fp32 records
    p.nb_rows = imax1(imin(divup(n * ns, PTV1_TPB), 1024));
    p.nb_fwd = imax1(imin(n, 1024));
    p.nb_logits = imax1(imin(imin(n, 1024), budget / (4ll * p.i * p.i)));
    p.nb_gu = imax1(imin(divup(n * ns * p.i, PTV1_TPB), 1024));
    p.nb_w2 = imax1(imin(imin(n, 1024), budget / (4ll * p.i * c)));
    p.nb_prow = imax1(imin(imin(n, 1024), budget / (16ll * c)));
    return p;
}

struct Ptv1Fwd {
    double *part3, *partc, *parti;
    float *w2t, *w3t;
};
static size_t ptv1_carve_fwd(const Ptv1Plan &p, char *base, Ptv1Fwd &w) {
    PtvCarver cv{base, 0};
    w.part3 = cv.take_n<double>((size_t)p.nb_rows * 6);
    w.partc = cv.take_n<double>((size_t)p.nb_fwd * 2 * p.c);
    w.parti = cv.take_n<double>((size_t)p.nb_fwd * 2 * p.i);
    w.w2t = cv.take_n<float>((size_t)p.c * p.i);
    w.w3t = cv.take_n<float>((size_t)p.i * p.i);
    return cv.off;
}
struct Ptv1Bwd {
    float *g, *ga, *partw3, *partw2, *partw1;
    double *partd1, *partgu, *partc, *part3, *part0;
};
static size_t ptv1_carve_bwd(const Ptv1Plan &p, char *base, Ptv1Bwd &w) {
    PtvCarver cv{base, 0};
    w.g = cv.take_n<float>((size_t)p.n * p.ns * p.i);
    w.ga = cv.take_n<float>((size_t)p.n * p.ns * 3);
    w.partw3 = cv.take_n<float>((size_t)p.nb_logits * p.i * p.i);
    w.partw2 = cv.take_n<float>((size_t)p.nb_w2 * p.i * p.c);
    w.partw1 = cv.take_n<float>((size_t)p.nb_prow * 4 * p.c);
    w.partd1 = cv.take_n<double>((size_t)p.nb_logits * 3 * p.i);
    w.partgu = cv.take_n<double>((size_t)p.nb_gu * p.i);
    w.partc = cv.take_n<double>((size_t)p.nb_w2 * 2 * p.c);
    w.part3 = cv.take_n<double>((size_t)p.nb_prow * 6);
    w.part0 = cv.take_n<double>((size_t)p.nb_rows * 12);
    return cv.off;
}

static bool ptv1_sizes_ok(long long n, int ns, int c) {
    if (n < 0 || n > 0x7fffffffll / (PTV1_MAX_NS * 64)) return false;  // n * ns * I and n * C stay below 2^31
    if (ns < 1 || ns > PTV1_MAX_NS) return false;
    return c == 32 || c == 64 || c == 128 || c == 256 || c == 512;
}

static Ptv1Args ptv1_args(int n, int ns, int training, float eps, const float *xq, const float *xk, const float *xv,
                          const float *coord, const int *idx, const ptv1_params *p, const ptv1_norms *s) {
    Ptv1Args a;
    a.n = n; a.ns = ns; a.training = training; a.eps = eps;
    a.xq = xq; a.xk = xk; a.xv = xv; a.coord = coord; a.idx = idx;
    a.p = *p;
    a.mean3 = s->mean3; a.var3 = s->var3; a.meanc = s->meanc; a.varc = s->varc; a.meani = s->meani; a.vari = s->vari;
    return a;
}
static bool ptv1_params_ok(const ptv1_params *p, const ptv1_norms *s) {
    if (!p || !s) return false;
    return p->p0_w && p->p0_b && p->p1_g && p->p1_b && p->p3_w && p->p3_b && p->w0_g && p->w0_b && p->w2_w && p->w2_b &&
           p->w3_g && p->w3_b && p->w5_w && p->w5_b && s->mean3 && s->var3 && s->meanc && s->varc && s->meani && s->vari;
}

template <class T>
static void ptv1_reduce(const T *part, int nblk, int stride, int len, float *out, hipStream_t st) {
    ptv1_reduce_kernel<T><<<divup(len, PTV1_TPB), PTV1_TPB, 0, st>>>(part, nblk, stride, len, out);
}

template <int C>
static int ptv1_forward(const Ptv1Plan &pl, Ptv1Args a, const ptv1_norms *s, float momentum, float *out, float *u, float *wsave,
                        const Ptv1Fwd &w, hipStream_t st) {
    constexpr int I = C / PTV1_SHARE;
    const double rows = (double)pl.n * pl.ns;
    ptv1_transpose_kernel<<<divup(I * C, PTV1_TPB), PTV1_TPB, 0, st>>>(a.p.w2_w, I, C, w.w2t);
    ptv1_transpose_kernel<<<divup(I * I, PTV1_TPB), PTV1_TPB, 0, st>>>(a.p.w5_w, I, I, w.w3t);
    if (a.training) {
        ptv1_stats3_kernel<<<pl.nb_rows, PTV1_TPB, 0, st>>>(a, w.part3);
        ptv1_stats_finalize_kernel<<<1, 64, 0, st>>>(w.part3, pl.nb_rows, 3, rows, s->mean3, s->var3, s->run_mean3, s->run_var3,
                                                      s->batches3, momentum);
        ptv1_statsc_kernel<C><<<pl.nb_fwd, PTV1_TPB, 0, st>>>(a, w.partc);
        ptv1_stats_finalize_kernel<<<divup(C, 64), 64, 0, st>>>(w.partc, pl.nb_fwd, C, rows, s->meanc, s->varc, s->run_meanc,
                                                                 s->run_varc, s->batchesc, momentum);
    }
    ptv1_u_kernel<C><<<pl.nb_fwd, PTV1_TPB, 0, st>>>(a, w.w2t, u, w.parti);
    if (a.training)
        ptv1_stats_finalize_kernel<<<1, 64, 0, st>>>(w.parti, pl.nb_fwd, I, rows, s->meani, s->vari, s->run_meani, s->run_vari,
                                                      s->batchesi, momentum);
    ptv1_out_kernel<C><<<pl.nb_fwd, PTV1_TPB, 0, st>>>(a, w.w3t, u, wsave, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

template <int C>
static int ptv1_backward(const Ptv1Plan &pl, Ptv1Args a, const int *inv_ptr, const int *inv_rows, const float *gout,
                         const float *u, const float *wsave, float *gxq, float *gxk, float *gxv, const ptv1_grads &g,
                         const Ptv1Bwd &w, hipStream_t st) {
    using L = Ptv1Lay<C>;
    constexpr int I = C / PTV1_SHARE;
    constexpr int CC = C < 64 ? C : 64;
    ptv1_bwd_logits_kernel<C><<<pl.nb_logits, PTV1_TPB, 0, st>>>(a, u, wsave, gout, w.g, w.partd1, w.partw3);
    ptv1_reduce(w.partd1, pl.nb_logits, 3 * I, I, g.w3_g, st);
    ptv1_reduce(w.partd1 + I, pl.nb_logits, 3 * I, I, g.w3_b, st);
    ptv1_reduce(w.partd1 + 2 * I, pl.nb_logits, 3 * I, I, g.w5_b, st);
    ptv1_reduce(w.partw3, pl.nb_logits, I * I, I * I, g.w5_w, st);
    ptv1_gu_kernel<<<pl.nb_gu, PTV1_TPB, 0, st>>>(a, I, u, g.w3_g, g.w3_b, w.g, w.partgu);
    ptv1_reduce(w.partgu, pl.nb_gu, I, I, g.w2_b, st);
    ptv1_bwd_w2_kernel<C><<<dim3(pl.nb_w2, C / CC), PTV1_TPB, 0, st>>>(a, w.g, w.partw2, w.partc);
    ptv1_reduce(w.partw2, pl.nb_w2, I * C, I * C, g.w2_w, st);
    ptv1_reduce(w.partc, pl.nb_w2, 2 * C, C, g.w0_g, st);
    ptv1_reduce(w.partc + C, pl.nb_w2, 2 * C, C, g.w0_b, st);
    ptv1_bwd_rows_kernel<C><<<pl.nb_prow, PTV1_TPB, 0, st>>>(a, w.g, wsave, gout, g.w0_g, g.w0_b, gxq, w.ga, w.partw1, w.part3);
    ptv1_reduce(w.partw1, pl.nb_prow, 4 * C, 3 * C, g.p3_w, st);
    ptv1_reduce(w.partw1 + 3 * C, pl.nb_prow, 4 * C, C, g.p3_b, st);
    ptv1_reduce(w.part3, pl.nb_prow, 6, 3, g.p1_g, st);
    ptv1_reduce(w.part3 + 3, pl.nb_prow, 6, 3, g.p1_b, st);
    ptv1_bwd_gather_kernel<C><<<divup(pl.n, L::G), PTV1_TPB, 0, st>>>(a, inv_ptr, inv_rows, w.g, wsave, gout, g.w0_g, g.w0_b,
                                                                       gxk, gxv);
    ptv1_bwd_p0_kernel<<<pl.nb_rows, PTV1_TPB, 0, st>>>(a, w.ga, g.p1_g, g.p1_b, w.part0);
    ptv1_reduce(w.part0, pl.nb_rows, 12, 9, g.p0_w, st);
    ptv1_reduce(w.part0 + 9, pl.nb_rows, 12, 3, g.p0_b, st);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

}  // namespace

extern "C" int ptv2_ptv1_abi_version(void) { return 1; }

extern "C" int ptv2_ptv1_struct_bytes(int which) {
    switch (which) {
        case 0: return (int)sizeof(ptv1_params);
        case 1: return (int)sizeof(ptv1_norms);
        case 2: return (int)sizeof(ptv1_grads);
    }
    return -1;
}

extern "C" long long ptv1_attention_workspace_bytes(long long n, int ns, int c) {
    if (!ptv1_sizes_ok(n, ns, c)) return -1;
    const Ptv1Plan pl = ptv1_plan(n, ns, c);
    Ptv1Fwd f;
    Ptv1Bwd b;
    const size_t fb = ptv1_carve_fwd(pl, nullptr, f), bb = ptv1_carve_bwd(pl, nullptr, b);
    return (long long)(fb > bb ? fb : bb);
}

extern "C" long long ptv1_attention_saved_bytes(long long n, int ns, int c) {
    if (!ptv1_sizes_ok(n, ns, c)) return -1;
    return 2 * (long long)ptv2_align256((size_t)n * ns * (c / PTV1_SHARE) * sizeof(float));
}

extern "C" int ptv1_attention_forward_hip_launcher(int n, int ns, int c, const float *x_q, const float *x_k, const float *x_v,
                                                   const float *coord, const int *idx, const ptv1_params *params,
                                                   const ptv1_norms *norms, int training, float eps, float momentum, float *out,
                                                   void *saved, long long saved_bytes, void *workspace, long long workspace_bytes,
                                                   void *stream) {
    if (!ptv1_sizes_ok(n, ns, c) || !ptv1_params_ok(params, norms)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (!x_q || !x_k || !x_v || !coord || !idx || !out || !saved || !workspace) return PTV2_ERR_ARG;
    if (training && (long long)n * ns < 2) return PTV2_ERR_ARG;
    const Ptv1Plan pl = ptv1_plan(n, ns, c);
    Ptv1Fwd w;
    if ((long long)ptv1_carve_fwd(pl, (char *)workspace, w) > workspace_bytes) return PTV2_ERR_WORKSPACE;
    if (ptv1_attention_saved_bytes(n, ns, c) > saved_bytes) return PTV2_ERR_WORKSPACE;
    float *u = (float *)saved, *wsave = (float *)((char *)saved + ptv1_attention_saved_bytes(n, ns, c) / 2);
    const Ptv1Args a = ptv1_args(n, ns, training != 0, eps, x_q, x_k, x_v, coord, idx, params, norms);
    hipStream_t st = (hipStream_t)stream;
    switch (c) {
        case 32: return ptv1_forward<32>(pl, a, norms, momentum, out, u, wsave, w, st);
        case 64: return ptv1_forward<64>(pl, a, norms, momentum, out, u, wsave, w, st);
        case 128: return ptv1_forward<128>(pl, a, norms, momentum, out, u, wsave, w, st);
        case 256: return ptv1_forward<256>(pl, a, norms, momentum, out, u, wsave, w, st);
        case 512: return ptv1_forward<512>(pl, a, norms, momentum, out, u, wsave, w, st);
    }
    return PTV2_ERR_ARG;
}

extern "C" int ptv1_attention_backward_hip_launcher(int n, int ns, int c, const float *x_q, const float *x_k, const float *x_v,
                                                    const float *coord, const int *idx, const int *inv_ptr, const int *inv_rows,
                                                    const ptv1_params *params, const ptv1_norms *norms, int training, float eps,
                                                    const float *g_out, const void *saved, long long saved_bytes, float *g_xq,
                                                    float *g_xk, float *g_xv, const ptv1_grads *grads, void *workspace,
                                                    long long workspace_bytes, void *stream) {
    if (!ptv1_sizes_ok(n, ns, c) || !ptv1_params_ok(params, norms) || !grads) return PTV2_ERR_ARG;
    const ptv1_grads &g = *grads;
    if (!g.p0_w || !g.p0_b || !g.p1_g || !g.p1_b || !g.p3_w || !g.p3_b || !g.w0_g || !g.w0_b || !g.w2_w || !g.w2_b || !g.w3_g ||
        !g.w3_b || !g.w5_w || !g.w5_b)
        return PTV2_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {  // the gradients of the parameters are still written
        const int i = c / PTV1_SHARE;
        float *arr[14] = {g.p0_w, g.p0_b, g.p1_g, g.p1_b, g.p3_w, g.p3_b, g.w0_g, g.w0_b, g.w2_w, g.w2_b, g.w3_g, g.w3_b, g.w5_w, g.w5_b};
        const int len[14] = {9, 3, 3, 3, 3 * c, c, c, c, i * c, i, i, i, i * i, i};
        for (int k = 0; k < 14; ++k) RUN(ptv2_zero_async(arr[k], sizeof(float) * len[k], st));
        return PTV2_OK;
    }
    if (!x_q || !x_k || !x_v || !coord || !idx || !inv_ptr || !inv_rows || !g_out || !saved || !g_xq || !g_xk || !g_xv || !workspace)
        return PTV2_ERR_ARG;
    const Ptv1Plan pl = ptv1_plan(n, ns, c);
    Ptv1Bwd w;
    if ((long long)ptv1_carve_bwd(pl, (char *)workspace, w) > workspace_bytes) return PTV2_ERR_WORKSPACE;
    if (ptv1_attention_saved_bytes(n, ns, c) > saved_bytes) return PTV2_ERR_WORKSPACE;
    const float *u = (const float *)saved, *wsave = (const float *)((const char *)saved + ptv1_attention_saved_bytes(n, ns, c) / 2);
    const Ptv1Args a = ptv1_args(n, ns, training != 0, eps, x_q, x_k, x_v, coord, idx, params, norms);
    switch (c) {
        case 32: return ptv1_backward<32>(pl, a, inv_ptr, inv_rows, g_out, u, wsave, g_xq, g_xk, g_xv, g, w, st);
        case 64: return ptv1_backward<64>(pl, a, inv_ptr, inv_rows, g_out, u, wsave, g_xq, g_xk, g_xv, g, w, st);
        case 128: return ptv1_backward<128>(pl, a, inv_ptr, inv_rows, g_out, u, wsave, g_xq, g_xk, g_xv, g, w, st);
        case 256: return ptv1_backward<256>(pl, a, inv_ptr, inv_rows, g_out, u, wsave, g_xq, g_xk, g_xv, g, w, st);
        case 512: return ptv1_backward<512>(pl, a, inv_ptr, inv_rows, g_out, u, wsave, g_xq, g_xk, g_xv, g, w, st);
    }
    return PTV2_ERR_ARG;
}
