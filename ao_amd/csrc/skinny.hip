// ao_amd/csrc/skinny.hip -- the narrow projection Linear(c, G), G <= 64, in front of the attention logits (kW = k Ww1^T,
// qW = q Ww1^T) on gfx950:
//   * forward, one tensor or the key / query pair per launch, optionally with BatchNorm + ReLU applied on the operand load;
//   * backward (input gradient), one tensor or the pair per launch, with the queued parameter-gradient sums riding along;
//   * the pair's backward fused with the reduce of the q / k BatchNorms behind it (skinny_bn_bwd_reduce_kernel, SkinnyBnArm).
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

}  // namespace dense

using namespace dense;

extern "C" int skinny_linear_forward_xf_hip_launcher(int n, int cin, int cout, const float *x, const float *W,
                                                    const float *xsc, const float *xsh, float *y, void *stream) {
    if (n < 0 || cin < 4 || cin % 4 != 0 || cout < 1 || cout > 64 || (xsc == nullptr) != (xsh == nullptr)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    const size_t lds = sizeof(float) * ((size_t)cout * (cin + 4) + 2 * (size_t)cin);
    if (lds > 160 * 1024) return PTV2_ERR_ARG;
    if (lds > 32 * 1024)
        (void)hipFuncSetAttribute((const void *)skinny_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const long long total = (long long)n * cout;
    const int nblk = (int)std::min<long long>((total + TPB - 1) / TPB, 256 * 8);
    {
        PtvScopedTimer t(KID_SKINNY_FWD, (hipStream_t)stream, 4.0 * n * (cin + cout));
        hipLaunchKernelGGL(skinny_fwd_kernel, dim3(nblk), dim3(TPB), lds, (hipStream_t)stream, (long long)n, cin, cout, x, W, xsc,
                           xsh, y, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr, (float *)nullptr);
    }
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

// two projections through the same W in one launch (internal to the block runtime): y[i] = f(x[i]) W^T, i = 0, 1
int skinny_linear_forward_pair(int n, int cin, int cout, const float *const *x, const float *W, const float *const *xsc,
                               const float *const *xsh, float *const *y, void *stream) {
    if (n < 0 || cin < 4 || cin % 4 != 0 || cout < 1 || cout > 64) return PTV2_ERR_ARG;
    if ((xsc[0] == nullptr) != (xsc[1] == nullptr)) return PTV2_ERR_ARG;
    if (n == 0) return PTV2_OK;
    const size_t lds = sizeof(float) * ((size_t)cout * (cin + 4) + 2 * (size_t)cin);
    if (lds > 160 * 1024) return PTV2_ERR_ARG;
    if (lds > 32 * 1024)
        (void)hipFuncSetAttribute((const void *)skinny_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const long long total = (long long)n * cout;
    const int nblk = (int)std::min<long long>((total + TPB - 1) / TPB, 256 * 8);
    {
        PtvScopedTimer t(KID_SKINNY_FWD, (hipStream_t)stream, 8.0 * n * (cin + cout));
        hipLaunchKernelGGL(skinny_fwd_kernel, dim3(nblk, 2), dim3(TPB), lds, (hipStream_t)stream, (long long)n, cin, cout, x[0], W,
                           xsc[0], xsh[0], y[0], x[1], xsc[1], xsh[1], y[1]);
    }
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
        hipLaunchKernelGGL(skinny_bn_bwd_reduce_kernel, dim3(K.nblk + gva::rider_blocks(Rs), 2), dim3(TPB), sizeof(float4) * 2 * TPB, st,
                           n, cin, cout, A, B, W, K.relu, K.part, K.nblk, Rs);
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
