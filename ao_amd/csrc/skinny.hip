// ao_amd/csrc/skinny.hip -- the narrow projection Linear(c, G), G <= 64, in front of the attention logits (kW = k Ww1^T,
// qW = q Ww1^T) on gfx950:
//   * forward, one tensor or the key / query pair per launch, optionally with BatchNorm + ReLU applied on the operand load;
//   * backward (input gradient), one tensor or the pair per launch, with the queued parameter-gradient sums riding along;
//   * the pair's backward fused with the reduce of the q / k BatchNorms behind it (skinny_bn_bwd_reduce_kernel, SkinnyBnArm).
// The forward and the fused backward + reduce each have two forms with the same bits in every output: operands staged in LDS
// (skinny_fwd_tile_kernel, skinny_bn_bwd_reduce_staged_kernel; the default) and one lane per output walking global memory
// (AO_AMD_SKINNY=lanes, and wherever the LDS image does not fit).
#include "dense_common.h"

namespace dense {

// ----------------------------------------------------------- skinny projection --
// y[n,o] = sum_i x[n,i] W[o,i] for cout <= 64 (the G-wide projections kW, qW of the attention logits); the
// BLAS kernel chosen for an N x 48 x 6 product runs 190 us (profiles/r01_fused_v5_*).  One lane per output,
// W in LDS, the x row is shared by the cout lanes of a point.
// xsc / xsh != NULL: the input row passes through ReLU(x * xsc + xsh) first (BatchNorm + ReLU of linear_q / linear_k
// fused into the projection that consumes them)
// blockIdx.y == 1 works on the second operand set (x2, xsc2, xsh2 -> y2; same W): the key and query projections
__global__ __launch_bounds__(TPB) void skinny_fwd_kernel(long long n, int cin, int cout, const float *x, const float *__restrict__ W,
                                                         const float *xsc, const float *xsh, float *y, const float *x2,
                                                         const float *xsc2, const float *xsh2, float *y2) {
    extern __shared__ float4 lds4[];
    if (blockIdx.y) { x = x2; xsc = xsc2; xsh = xsh2; y = y2; }
    float *sW = (float *)lds4;  // [cout][cin + 4], then [2][cin] scale / shift
    const int ldw = cin + 4, cq = cin >> 2;
    float *sSc = sW + (size_t)cout * ldw, *sSh = sSc + cin;
    for (int e = threadIdx.x; e < cout * cq; e += TPB) {
        const int r = e / cq, q = e - r * cq;
        *(float4 *)(sW + (size_t)r * ldw + 4 * q) = *(const float4 *)(W + (size_t)r * cin + 4 * q);
    }
    if (xsc)
        for (int e = threadIdx.x; e < cin; e += TPB) { sSc[e] = xsc[e]; sSh[e] = xsh[e]; }
    __syncthreads();
    const long long total = n * cout;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long long)gridDim.x * TPB) {
        const long long row = e / cout;
        const int o = (int)(e - row * cout);
        const float4 *xr = (const float4 *)(x + row * cin), *wr = (const float4 *)(sW + (size_t)o * ldw);
        float acc = 0.f;
        if (xsc) {
            int q = 0;
            for (; q + 4 <= cq; q += 4) {  // four row quads in flight per trip (cq is a multiple of 4 for C = 48 ... 512)
                float4 av[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) av[u] = xr[q + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float4 a = av[u];
                    const float4 w = wr[q + u], s4 = ((const float4 *)sSc)[q + u], h4 = ((const float4 *)sSh)[q + u];
                    a.x = fmaxf(__builtin_fmaf(a.x, s4.x, h4.x), 0.f); a.y = fmaxf(__builtin_fmaf(a.y, s4.y, h4.y), 0.f);
                    a.z = fmaxf(__builtin_fmaf(a.z, s4.z, h4.z), 0.f); a.w = fmaxf(__builtin_fmaf(a.w, s4.w, h4.w), 0.f);
                    acc = __builtin_fmaf(a.x, w.x, acc); acc = __builtin_fmaf(a.y, w.y, acc);
                    acc = __builtin_fmaf(a.z, w.z, acc); acc = __builtin_fmaf(a.w, w.w, acc);
                }
            }
            for (; q < cq; ++q) {
                float4 a = xr[q];
                const float4 w = wr[q], s4 = ((const float4 *)sSc)[q], h4 = ((const float4 *)sSh)[q];
                a.x = fmaxf(__builtin_fmaf(a.x, s4.x, h4.x), 0.f); a.y = fmaxf(__builtin_fmaf(a.y, s4.y, h4.y), 0.f);
                a.z = fmaxf(__builtin_fmaf(a.z, s4.z, h4.z), 0.f); a.w = fmaxf(__builtin_fmaf(a.w, s4.w, h4.w), 0.f);
                acc = __builtin_fmaf(a.x, w.x, acc); acc = __builtin_fmaf(a.y, w.y, acc);
                acc = __builtin_fmaf(a.z, w.z, acc); acc = __builtin_fmaf(a.w, w.w, acc);
            }
        } else {
            for (int q = 0; q < cq; ++q) {
                const float4 a = xr[q], w = wr[q];
                acc = __builtin_fmaf(a.x, w.x, acc); acc = __builtin_fmaf(a.y, w.y, acc);
                acc = __builtin_fmaf(a.z, w.z, acc); acc = __builtin_fmaf(a.w, w.w, acc);
            }
        }
        y[e] = acc;
    }
}

// Copies total float4 from global memory into LDS, element e to dst[(e / cq) * ld4 + e % cq], eight loads per lane in flight.
// nothing here is conditional -- a lane past the end repeats the last element, load and store (the same value
// to the same place); under a masked store the compiler sinks the load into the store's block and waits for each on the spot.
__device__ __forceinline__ void stage_rows4(float4 *dst, const float4 *__restrict__ src, int total, int cq, int ld4) {
    for (int b = 0; b < total; b += 8 * TPB) {
        float4 v[8];
        int e[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            e[u] = min(b + u * TPB + (int)threadIdx.x, total - 1);
            v[u] = src[e[u]];
        }
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise may pair each load with its store: one round trip each)
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[(e[u] / cq) * ld4 + e[u] % cq] = v[u];
    }
}

// The row-tile form of skinny_fwd_kernel: the same fmaf chain per output, its operands from LDS.  A workgroup walks tiles of
// R = skinny_tile_rows(cin) rows (at most SKINNY_TILE_LOADS float4 per lane): the tile's rows are loaded coalesced, all loads
// issued together and those of the NEXT tile before this tile's arithmetic; ReLU(x * xsc + xsh) is applied once per element
// on the way into LDS (the lane form evaluates it cout times); lane (row, o) then reads the row as a broadcast among the cout
// lanes of its point.  The lane form walks each row itself, cin / 16 dependent round trips per output with the cout lanes of
// a point issuing the same addresses.  Tail rows clamp to row n - 1 and are masked at the store.
constexpr int SKINNY_TILE_LOADS = 4;
static inline int skinny_tile_rows(int cin) { return SKINNY_TILE_LOADS * TPB / (cin >> 2); }

template <bool XF>
__global__ __launch_bounds__(TPB) void skinny_fwd_tile_kernel(int n, int cin, int cout, int R, int ntiles, const float *x,
                                                              const float *__restrict__ W, const float *xsc, const float *xsh,
                                                              float *y, const float *x2, const float *xsc2, const float *xsh2,
                                                              float *y2) {
    extern __shared__ float4 lds4[];
    if (blockIdx.y) { x = x2; xsc = xsc2; xsh = xsh2; y = y2; }
    const int cq = cin >> 2, ld4 = cq + 1, te = R * cq;
    float4 *sW = lds4, *sX = lds4 + (size_t)cout * ld4;  // [cout][cin + 4], [R][cin + 4]
    // the float4 of a tile this lane carries into LDS (clamped inside the tile: a lane past its end repeats the last one)
    int tr[SKINNY_TILE_LOADS], tq[SKINNY_TILE_LOADS];
    float4 xv[SKINNY_TILE_LOADS], s4[SKINNY_TILE_LOADS], h4[SKINNY_TILE_LOADS];
#pragma unroll
    for (int u = 0; u < SKINNY_TILE_LOADS; ++u) {
        const int e = min((int)threadIdx.x + u * TPB, te - 1);
        tr[u] = e / cq;
        tq[u] = e - tr[u] * cq;
    }
    long long tile = blockIdx.x;
#pragma unroll
    for (int u = 0; u < SKINNY_TILE_LOADS; ++u) {  // the first tile's rows are in flight while W is staged
        const long long row = min(tile * R + tr[u], (long long)n - 1);
        xv[u] = ((const float4 *)x)[row * cq + tq[u]];
        if (XF) { s4[u] = ((const float4 *)xsc)[tq[u]]; h4[u] = ((const float4 *)xsh)[tq[u]]; }
    }
    stage_rows4(sW, (const float4 *)W, cout * cq, cq, ld4);
    const int outs = R * cout;
    for (; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int u = 0; u < SKINNY_TILE_LOADS; ++u) {
            float4 a = xv[u];
            if (XF) {
                a.x = fmaxf(__builtin_fmaf(a.x, s4[u].x, h4[u].x), 0.f); a.y = fmaxf(__builtin_fmaf(a.y, s4[u].y, h4[u].y), 0.f);
                a.z = fmaxf(__builtin_fmaf(a.z, s4[u].z, h4[u].z), 0.f); a.w = fmaxf(__builtin_fmaf(a.w, s4[u].w, h4[u].w), 0.f);
            }
            sX[tr[u] * ld4 + tq[u]] = a;  // (a lane past the tile's end: the last element once more)
        }
        __syncthreads();
        const long long next = tile + gridDim.x;  // (past the last tile: every row clamps to n - 1, nothing is stored)
#pragma unroll
        for (int u = 0; u < SKINNY_TILE_LOADS; ++u) {
            const long long row = min(next * R + tr[u], (long long)n - 1);
            xv[u] = ((const float4 *)x)[row * cq + tq[u]];
        }
        for (int e = threadIdx.x; e < outs; e += TPB) {
            const int r = e / cout, o = e - r * cout;
            const float4 *xr = sX + r * ld4, *wr = sW + o * ld4;
            float acc = 0.f;
#pragma unroll 4
            for (int q = 0; q < cq; ++q) {
                const float4 a = xr[q], w = wr[q];
                acc = __builtin_fmaf(a.x, w.x, acc); acc = __builtin_fmaf(a.y, w.y, acc);
                acc = __builtin_fmaf(a.z, w.z, acc); acc = __builtin_fmaf(a.w, w.w, acc);
            }
            const long long row = tile * R + r;
            if (row < n) y[row * cout + o] = acc;
        }
        __syncthreads();
    }
}

// gx[n,i] = sum_o gy[n,o] W[o,i]; one lane per float4 of gx
__global__ __launch_bounds__(TPB) void skinny_bwd_kernel(long long n, int cin, int cout, const float *gy,
                                                         const float *__restrict__ W, float *gx, const float *gy2, float *gx2,
                                                         int main_blocks, gva::PtvRiders Rs) {
    if ((int)blockIdx.x >= main_blocks) {  // trailing workgroups: deferred parameter-gradient sums (gva_common.h, riders)
        if (blockIdx.y == 0) gva::rider_run(Rs, (int)blockIdx.x - main_blocks);
        return;
    }
    if (blockIdx.y) { gy = gy2; gx = gx2; }
    const int cq = cin >> 2;
    const long long total = n * cq;
    for (long long e = (long long)blockIdx.x * TPB + threadIdx.x; e < total; e += (long long)main_blocks * TPB) {
        const long long row = e / cq;
        const int q = (int)(e - row * cq);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        // six outputs per trip (G = 6, 12, 24, 48 ...): their twelve loads are in flight together -- one output per trip
        // waited for its own two loads every time, and the kernel sat parked on memory for 89 % of its wave cycles
        // (profiles/r02_final_sq_counters.jsonl)
        const float *g = gy + row * cout;
        const float *wc = W + 4 * q;
        int o = 0;
        for (; o + 6 <= cout; o += 6) {
            float sv[6];
            float4 wv[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) { sv[u] = g[o + u]; wv[u] = *(const float4 *)(wc + (size_t)(o + u) * cin); }
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                acc.x = __builtin_fmaf(sv[u], wv[u].x, acc.x); acc.y = __builtin_fmaf(sv[u], wv[u].y, acc.y);
                acc.z = __builtin_fmaf(sv[u], wv[u].z, acc.z); acc.w = __builtin_fmaf(sv[u], wv[u].w, acc.w);
            }
        }
        for (; o < cout; ++o) {
            const float s = g[o];
            const float4 w = *(const float4 *)(wc + (size_t)o * cin);
            acc.x = __builtin_fmaf(s, w.x, acc.x); acc.y = __builtin_fmaf(s, w.y, acc.y);
            acc.z = __builtin_fmaf(s, w.z, acc.z); acc.w = __builtin_fmaf(s, w.w, acc.w);
        }
        ((float4 *)gx)[e] = acc;
    }
}

// The same reduce with its gradient formed in place: gy[row, :] = sg[row, :] W (the input gradient of the skinny Linear(c, G) in
// front of the logits: kW = k Ww1^T, qW = q Ww1^T) is computed, stored (the apply pass reads it) and summed by the lane that owns
// the float4 -- skinny_bwd_kernel and the q / k BatchNorms' reduce were two launches over the same (n, c) rows in every Block's
// backward.  blockIdx.y: the tensor (k, q); trailing workgroups in x: the queued parameter-gradient sums (riders, as skinny_bwd).
struct SkinnyBn {
    const float *sg;   // (n, cout) gradient of the projection's output
    float *gy;         // (n, c) its input gradient = the BatchNorm's output gradient (written)
    const float *x, *mean, *rstd, *gamma, *beta;
};
__global__ __launch_bounds__(TPB) void skinny_bn_bwd_reduce_kernel(int n, int c, int cout, SkinnyBn A, SkinnyBn B,
                                                                   const float *__restrict__ W, int relu, float *__restrict__ part,
                                                                   int main_blocks, gva::PtvRiders Rs) {
    extern __shared__ float4 lds4[];
    if ((int)blockIdx.x >= main_blocks) {
        if (blockIdx.y == 0) gva::rider_run(Rs, (int)blockIdx.x - main_blocks);
        return;
    }
    const SkinnyBn &S = blockIdx.y ? B : A;
    const int cq = c >> 2;
    const int rl = TPB / cq;
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    if (r < rl) {
        const float4 m = ((const float4 *)S.mean)[q], rs = ((const float4 *)S.rstd)[q];
        const float4 g = ((const float4 *)S.gamma)[q], b = ((const float4 *)S.beta)[q];
        const float *wc = W + 4 * q;
        for (long long row = (long long)blockIdx.x * rl + r; row < n; row += (long long)main_blocks * rl) {
            const float4 v = ((const float4 *)S.x)[row * cq + q];
            const float *sg = S.sg + row * cout;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
            int o = 0;
            for (; o + 6 <= cout; o += 6) {  // (six outputs' loads in flight together, as skinny_bwd_kernel)
                float sv[6];
                float4 wv[6];
#pragma unroll
                for (int u = 0; u < 6; ++u) { sv[u] = sg[o + u]; wv[u] = *(const float4 *)(wc + (size_t)(o + u) * c); }
#pragma unroll
                for (int u = 0; u < 6; ++u) {
                    d.x = __builtin_fmaf(sv[u], wv[u].x, d.x); d.y = __builtin_fmaf(sv[u], wv[u].y, d.y);
                    d.z = __builtin_fmaf(sv[u], wv[u].z, d.z); d.w = __builtin_fmaf(sv[u], wv[u].w, d.w);
                }
            }
            for (; o < cout; ++o) {
                const float sv = sg[o];
                const float4 w = *(const float4 *)(wc + (size_t)o * c);
                d.x = __builtin_fmaf(sv, w.x, d.x); d.y = __builtin_fmaf(sv, w.y, d.y);
                d.z = __builtin_fmaf(sv, w.z, d.z); d.w = __builtin_fmaf(sv, w.w, d.w);
            }
            ((float4 *)S.gy)[row * cq + q] = d;
            const float4 h = bn_xhat(v, m, rs);
            if (relu) d = bn_relu_mask(d, h, g, b);
            bn_accumulate(s1, s2, d, h);
        }
    }
    column_sums_store(lds4, s1, s2, cq, rl, c, part + ((size_t)blockIdx.x * 2 + blockIdx.y) * 2 * c);  // record of a block: [set 0 | set 1]
}

// The staged form of skinny_bn_bwd_reduce_kernel: the same lanes own the same (row, float4) in the same order, so every gy
// element, every lane's s1 / s2 and the record of a block keep their bits; only where the chain's operands come from changes.
// W (cout x c) is staged into LDS once per workgroup.  The workgroup visits its rows SKINNY_BN_TRIP at a time: the sg rows of a
// trip go through LDS (rl * cout contiguous floats per visit), the x and sg loads of the NEXT trip are issued before this
// trip's arithmetic, and one W operand serves the chains of all the trip's rows (each row's chain still runs o = 0 ... cout - 1
// from zero).  The lane form reads cout rows of W and the sg scalars from global memory for every row, cout / 6 dependent
// trips each.  LDS: [W | sg of a trip]; column_sums_store's 2 * TPB float4 lie over it once the row loop is done.
constexpr int SKINNY_BN_TRIP = 4, SKINNY_BN_SG = 2;  // rows per lane and trip; sg floats a lane carries into LDS per trip
__global__ __launch_bounds__(TPB) void skinny_bn_bwd_reduce_staged_kernel(int n, int c, int cout, SkinnyBn A, SkinnyBn B,
                                                                          const float *__restrict__ W, int relu,
                                                                          float *__restrict__ part, int main_blocks, gva::PtvRiders Rs) {
    extern __shared__ float4 lds4[];
    if ((int)blockIdx.x >= main_blocks) {
        if (blockIdx.y == 0) gva::rider_run(Rs, (int)blockIdx.x - main_blocks);
        return;
    }
    const SkinnyBn &S = blockIdx.y ? B : A;
    const int cq = c >> 2;
    const int rl = TPB / cq;
    const int q = threadIdx.x % cq, r = threadIdx.x / cq;
    const int rg = rl * cout, ng = SKINNY_BN_TRIP * rg;  // sg floats of one visit (rows [b, b + rl)) and of a trip
    float *sG = (float *)(lds4 + (size_t)cout * cq);  // [SKINNY_BN_TRIP][rl * cout], behind W [cout][cq]
    const long long step = (long long)main_blocks * rl, last = (long long)n * cout - 1;
    const float4 m = ((const float4 *)S.mean)[q], rs = ((const float4 *)S.rstd)[q];
    const float4 g = ((const float4 *)S.gamma)[q], b = ((const float4 *)S.beta)[q];
    int ge[SKINNY_BN_SG], gu[SKINNY_BN_SG], gw[SKINNY_BN_SG];  // (a lane past the trip's end repeats its last float)
#pragma unroll
    for (int j = 0; j < SKINNY_BN_SG; ++j) {
        ge[j] = min((int)threadIdx.x + j * TPB, ng - 1);
        gu[j] = ge[j] / rg;
        gw[j] = ge[j] - gu[j] * rg;
    }
    float4 v[SKINNY_BN_TRIP], s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    float gs[SKINNY_BN_SG];
    long long b0 = (long long)blockIdx.x * rl;
    // every load unconditional: rows past n - 1 clamp to it and are masked where they would be kept
#define SKINNY_BN_LOADS(base)                                                                                          \
    _Pragma("unroll") for (int u = 0; u < SKINNY_BN_TRIP; ++u)                                                         \
        v[u] = ((const float4 *)S.x)[min((base) + u * step + r, (long long)n - 1) * cq + q];                           \
    _Pragma("unroll") for (int j = 0; j < SKINNY_BN_SG; ++j) gs[j] = S.sg[min(((base) + gu[j] * step) * cout + gw[j], last)];
    SKINNY_BN_LOADS(b0)
    if (b0 < n) stage_rows4(lds4, (const float4 *)W, cout * cq, cq, cq);  // (a block without rows leaves LDS to its record)
    const float *sg = sG + min(r, rl - 1) * cout;  // (lanes behind the last row lane compute along with it and keep nothing)
    const float4 *wq = lds4 + q;
    for (; b0 < n; b0 += SKINNY_BN_TRIP * step) {  // (uniform over the workgroup)
        float4 vc[SKINNY_BN_TRIP], d[SKINNY_BN_TRIP];
#pragma unroll
        for (int u = 0; u < SKINNY_BN_TRIP; ++u) { vc[u] = v[u]; d[u] = make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
        for (int j = 0; j < SKINNY_BN_SG; ++j) sG[ge[j]] = gs[j];
        __syncthreads();
        SKINNY_BN_LOADS(b0 + SKINNY_BN_TRIP * step)
#pragma unroll 12
        for (int o = 0; o < cout; ++o) {
            const float4 w = wq[(size_t)o * cq];
#pragma unroll
            for (int u = 0; u < SKINNY_BN_TRIP; ++u) {
                const float sv = sg[u * rg + o];
                d[u].x = __builtin_fmaf(sv, w.x, d[u].x); d[u].y = __builtin_fmaf(sv, w.y, d[u].y);
                d[u].z = __builtin_fmaf(sv, w.z, d[u].z); d[u].w = __builtin_fmaf(sv, w.w, d[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < SKINNY_BN_TRIP; ++u) {
            const long long row = b0 + u * step + r;
            if (r < rl && row < n) {
                ((float4 *)S.gy)[row * cq + q] = d[u];
                const float4 h = bn_xhat(vc[u], m, rs);
                if (relu) d[u] = bn_relu_mask(d[u], h, g, b);
                bn_accumulate(s1, s2, d[u], h);
            }
        }
        __syncthreads();
    }
#undef SKINNY_BN_LOADS
    column_sums_store(lds4, s1, s2, cq, rl, c, part + ((size_t)blockIdx.x * 2 + blockIdx.y) * 2 * c);  // record of a block: [set 0 | set 1]
}

}  // namespace dense

using namespace dense;

// AO_AMD_SKINNY=lanes (read on every call): the lane forms of the projection and of its backward + reduce everywhere
static inline bool skinny_lanes_only() { return ptv2_env_is("AO_AMD_SKINNY", 'l'); }

// The forward of `sets` (1 or 2) operand sets through the same W.  Which form runs is decided here, per (n, cin, cout):
// the row-tile kernel wherever its LDS image ([cout + R][cin + 4] floats) fits 160 KB, the lane kernel otherwise and under
// AO_AMD_SKINNY=lanes.  Measured per pair launch (MI355X), lanes / tiles: 120 000 x 48 14.7 / 13.8 us (12.8 on two other
// boxes: the smallest gain, below the lane form in every call), 18 905 x 96 10.2 / 9.2, 4 501 x 192 11.4 / 8.1, 1 074 x 384
// 20.9 / 10.0 -- no crossover at the sizes of a training step (profiles/HISTORY.md).
static int skinny_forward_run(int n, int cin, int cout, int sets, const float *const *x, const float *W, const float *const *xsc,
                              const float *const *xsh, float *const *y, hipStream_t st) {
    const int R = skinny_tile_rows(cin);
    const size_t tile_lds = sizeof(float) * (size_t)(cout + R) * (cin + 4);
    const bool tile = !skinny_lanes_only() && R >= 1 && tile_lds <= 160 * 1024;
    const float *x1 = sets > 1 ? x[1] : nullptr, *sc1 = sets > 1 ? xsc[1] : nullptr, *sh1 = sets > 1 ? xsh[1] : nullptr;
    float *y1 = sets > 1 ? y[1] : nullptr;
    PtvScopedTimer t(KID_SKINNY_FWD, st, 4.0 * sets * n * (cin + cout));
    if (tile) {
        // resident workgroups: 4 per CU by registers, fewer where the LDS image is large; each walks the same count of tiles
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, 160 * 1024 / tile_lds));
        const int ntiles = (n + R - 1) / R, cap = std::max(1, 256 * per_cu / sets);
        const int walk = (ntiles + cap - 1) / cap, nblk = (ntiles + walk - 1) / walk;
        auto kernel = xsc[0] ? skinny_fwd_tile_kernel<true> : skinny_fwd_tile_kernel<false>;
        RUN(ptv2_kernel_lds((const void *)kernel, tile_lds));
        hipLaunchKernelGGL(kernel, dim3(nblk, sets), dim3(TPB), tile_lds, st, n, cin, cout, R, ntiles, x[0], W, xsc[0], xsh[0], y[0],
                           x1, sc1, sh1, y1);
        return PTV2_OK;
    }
    const size_t lds = sizeof(float) * ((size_t)cout * (cin + 4) + 2 * (size_t)cin);
    if (lds > 160 * 1024) return PTV2_ERR_ARG;
    RUN(ptv2_kernel_lds((const void *)skinny_fwd_kernel, lds));
    const long long total = (long long)n * cout;
    const int nblk = (int)std::min<long long>((total + TPB - 1) / TPB, 256 * 8);
    hipLaunchKernelGGL(skinny_fwd_kernel, dim3(nblk, sets), dim3(TPB), lds, st, (long long)n, cin, cout, x[0], W, xsc[0], xsh[0], y[0],
                       x1, sc1, sh1, y1);
    return PTV2_OK;
}

extern "C" int skinny_linear_forward_xf_hip_launcher(int n, int cin, int cout, const float *x, const float *W,
                                                    const float *xsc, const float *xsh, float *y, void *stream) {
    if (n < 0 || cin < 4 || cin % 4 != 0 || cout < 1 || cout > 64 || (xsc == nullptr) != (xsh == nullptr)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (sizeof(float) * ((size_t)cout * (cin + 4) + 2 * (size_t)cin) > 160 * 1024) return PTV2_ERR_ARG;
    RUN(skinny_forward_run(n, cin, cout, 1, &x, W, &xsc, &xsh, &y, (hipStream_t)stream));
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// two projections through the same W in one launch (internal to the block runtime): y[i] = f(x[i]) W^T, i = 0, 1
int skinny_linear_forward_pair(int n, int cin, int cout, const float *const *x, const float *W, const float *const *xsc,
                               const float *const *xsh, float *const *y, void *stream) {
    if (n < 0 || cin < 4 || cin % 4 != 0 || cout < 1 || cout > 64) return PTV2_ERR_ARG;
    if ((xsc[0] == nullptr) != (xsc[1] == nullptr)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    if (sizeof(float) * ((size_t)cout * (cin + 4) + 2 * (size_t)cin) > 160 * 1024) return PTV2_ERR_ARG;
    RUN(skinny_forward_run(n, cin, cout, 2, x, W, xsc, xsh, y, (hipStream_t)stream));
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int skinny_linear_forward_hip_launcher(int n, int cin, int cout, const float *x, const float *W, float *y,
                                                 void *stream) {
    return skinny_linear_forward_xf_hip_launcher(n, cin, cout, x, W, nullptr, nullptr, y, stream);
}

extern "C" int skinny_linear_backward_hip_launcher(int n, int cin, int cout, const float *gy, const float *W, float *gx,
                                                  void *stream) {
    if (n < 0 || cin < 4 || cin % 4 != 0 || cout < 1) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    const long long total = (long long)n * (cin >> 2);
    const int nblk = apply_grid(total);
    {
        PtvScopedTimer t(KID_SKINNY_BWD, (hipStream_t)stream, 4.0 * n * (cin + cout));
        hipLaunchKernelGGL(skinny_bwd_kernel, dim3(nblk), dim3(TPB), 0, (hipStream_t)stream, (long long)n, cin, cout, gy, W, gx,
                           (const float *)nullptr, (float *)nullptr, nblk, gva::PtvRiders{});
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// gx[i] = gy[i] W for two gradient tensors in one launch (internal to the block runtime)
int skinny_linear_backward_pair(int n, int cin, int cout, const float *const *gy, const float *W, float *const *gx, void *stream) {
    if (n < 0 || cin < 4 || cin % 4 != 0 || cout < 1) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    const long long total = (long long)n * (cin >> 2);
    const int nblk = apply_grid(total);
    {
        PtvScopedTimer t(KID_SKINNY_BWD, (hipStream_t)stream, 8.0 * n * (cin + cout));
        // the parameter-gradient sums queued by the stages before (logits parameters, kW / qW weights) ride along: gx
        // depends on none of them
        const gva::PtvRiders Rs = gva::ptv2_rider_take();
        hipLaunchKernelGGL(skinny_bwd_kernel, dim3(nblk + gva::rider_blocks(Rs), 2), dim3(TPB), 0, (hipStream_t)stream, (long long)n,
                           cin, cout, gy[0], W, gx[0], gy[1], gx[1], nblk, Rs);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// ---- the q / k BatchNorms' reduce inside the launch that forms their output gradients (skinny_bn_bwd_reduce_kernel) ----
// block.hip arms this with the operands of the bn_backward_pair call that will follow its attention backward; gva_block.hip, at
// the skinny input-gradient launch, asks skinny_backward_pair_bn_reduce to run the fused kernel instead; the pair launcher finds
// `done` with matching operands and skips its reduce launch.  Thread-local: one Block backward per thread at a time.
struct SkinnyBnArm {
    bool armed = false, done = false;
    int n = 0, c = 0, nblk = 0, relu = 0;
    const float *x[2] = {}, *mean[2] = {}, *rstd[2] = {}, *gamma[2] = {}, *beta[2] = {};
    const float *gy[2] = {};
    float *part = nullptr;
};
static thread_local SkinnyBnArm t_skinny_bn;

void ptv2_skinny_bn_arm(int n, int c, const float *const *x, const float *const *gy, const float *const *mean, const float *const *rstd,
                        const float *const *gamma, const float *const *beta, int relu, void *workspace, size_t workspace_bytes) {
    SkinnyBnArm &K = t_skinny_bn;
    K = SkinnyBnArm{};
    static const bool off = ptv2_env_is("AO_AMD_SKINNY_BN", '0');  // A/B switch
    if (off || n < 1 || c < 4 || c % 4 != 0 || (c >> 2) > TPB || !workspace || workspace_bytes < dense_workspace_bytes(n, 2 * c, c)) return;
    K.armed = true;
    K.n = n; K.c = c; K.nblk = bn_grid(n, c); K.relu = relu;
    // (deep levels: two rows per lane up to 256 records -- 128 records of seven rows per lane left the launch at one workgroup per
    // CU waiting on its own loads: 21.6 us at 4 501 rows x 192 against 15.3)
    constexpr int cap = 256;
    if (n <= 16384) {
        const int rl = std::max(1, TPB / (c >> 2));
        K.nblk = (int)std::max<long long>(1, std::min<long long>(((long long)n + rl * 2 - 1) / (rl * 2), cap));
    }
    for (int i = 0; i < 2; ++i) { K.x[i] = x[i]; K.gy[i] = gy[i]; K.mean[i] = mean[i]; K.rstd[i] = rstd[i]; K.gamma[i] = gamma[i]; K.beta[i] = beta[i]; }
    K.part = (float *)workspace;
}
void ptv2_skinny_bn_disarm(void) { t_skinny_bn.armed = false; }

// internal (gva_block.hip): gx[i] = gy[i] W as skinny_linear_backward_pair -- and, when armed for exactly these outputs, the
// reduce records of the BatchNorm backward that consumes them, in the same launch
int skinny_backward_pair_bn_reduce(int n, int cin, int cout, const float *const *gy, const float *W, float *const *gx, void *stream) {
    SkinnyBnArm &K = t_skinny_bn;
    const bool fuse = K.armed && K.n == n && K.c == cin && K.gy[0] == gx[0] && K.gy[1] == gx[1] && n > 0;
    K.armed = false;
    if (!fuse) return skinny_linear_backward_pair(n, cin, cout, gy, W, gx, stream);
    hipStream_t st = (hipStream_t)stream;
    {
        PtvScopedTimer t(KID_SKINNY_BWD, st, 8.0 * n * (cin + cout) + 8.0 * n * cin);
        const gva::PtvRiders Rs = gva::ptv2_rider_take();
        const SkinnyBn A{gy[0], gx[0], K.x[0], K.mean[0], K.rstd[0], K.gamma[0], K.beta[0]};
        const SkinnyBn B{gy[1], gx[1], K.x[1], K.mean[1], K.rstd[1], K.gamma[1], K.beta[1]};
        // The form is chosen here: staged while a trip's sg rows fit the lanes that carry them and W's image leaves four
        // workgroups per CU (28 KB beside the riders' 12 KB of static LDS).  Measured per launch (pair, MI355X), lanes / staged:
        // 120 000 x 48 27.5 / 22.2 us, 18 905 x 96 16.6 / 12.2, 4 501 x 192 (20 KB) 14.8 / 11.3; 1 074 x 384 (75 KB: one
        // workgroup per CU, the 2 502 rider workgroups of that launch included) 21.4 / 23.7, and 28.0 with W left in global
        // memory -- the lane form stays there.  The same grid and records in both forms.
        const size_t rec_lds = sizeof(float4) * 2 * TPB;
        const size_t sg_lds = sizeof(float) * SKINNY_BN_TRIP * (TPB / (cin >> 2)) * cout, w_lds = sizeof(float) * (size_t)cout * cin;
        const bool staged = !skinny_lanes_only() && sg_lds <= sizeof(float) * SKINNY_BN_SG * TPB && w_lds + sg_lds <= 28 * 1024;
        hipLaunchKernelGGL(staged ? skinny_bn_bwd_reduce_staged_kernel : skinny_bn_bwd_reduce_kernel,
                           dim3(K.nblk + gva::rider_blocks(Rs), 2), dim3(TPB), staged ? std::max(rec_lds, w_lds + sg_lds) : rec_lds, st, n,
                           cin, cout, A, B, W, K.relu, K.part, K.nblk, Rs);
    }
    K.done = true;
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// bn.hip's pair launcher: the count of reduce records the launch above left for exactly these operands (0: none; it reduces)
int ptv2_skinny_bn_take_records(int n, int c, const float *part, const float *const *gy) {
    SkinnyBnArm &K = t_skinny_bn;
    const bool reduced = K.done && K.part == part && K.n == n && K.c == c && K.gy[0] == gy[0] && K.gy[1] == gy[1];
    K.done = false;
    return reduced ? K.nblk : 0;
}
