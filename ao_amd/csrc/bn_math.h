// ao_amd/csrc/bn_math.h -- the per-element arithmetic of BatchNorm1d, four columns (one float4) at a time: each formula is
// stated here once and used by every kernel of bn.hip and by skinny_bn_bwd_reduce_kernel (skinny.hip).  Plain C++ under the
// unit's default contraction: the callers' results depend on these exact statements (fused where written as fmaf).
#pragma once
#include <hip/hip_runtime.h>

namespace dense {

// xhat = (x - mean) * rstd
__device__ __forceinline__ float4 bn_xhat(const float4 v, const float4 m, const float4 rs) {
    return make_float4((v.x - m.x) * rs.x, (v.y - m.y) * rs.y, (v.z - m.z) * rs.z, (v.w - m.w) * rs.w);
}

// forward: BN(x) = xhat * gamma + beta
__device__ __forceinline__ float4 bn_affine(const float4 h, const float4 g, const float4 b) {
    return make_float4(__builtin_fmaf(h.x, g.x, b.x), __builtin_fmaf(h.y, g.y, b.y), __builtin_fmaf(h.z, g.z, b.z),
                       __builtin_fmaf(h.w, g.w, b.w));
}
__device__ __forceinline__ float4 bn_relu(const float4 o) {
    return make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
}
// the Block tail: ReLU(residual + rowscale * o)
__device__ __forceinline__ float4 bn_residual_relu(const float4 o, const float rsc, const float4 res) {
    return bn_relu(make_float4(__builtin_fmaf(rsc, o.x, res.x), __builtin_fmaf(rsc, o.y, res.y), __builtin_fmaf(rsc, o.z, res.z),
                               __builtin_fmaf(rsc, o.w, res.w)));
}

// backward through the fused ReLU: the gradient passes where the forward's pre-activation was positive
__device__ __forceinline__ float4 bn_relu_mask(float4 d, const float4 h, const float4 g, const float4 b) {
    const float4 pre = bn_affine(h, g, b);
    if (pre.x <= 0.f) d.x = 0.f;
    if (pre.y <= 0.f) d.y = 0.f;
    if (pre.z <= 0.f) d.z = 0.f;
    if (pre.w <= 0.f) d.w = 0.f;
    return d;
}
// backward through the Block tail: the gradient passes where the output y was positive.  Applied to gy it gives the residual's
// gradient; rowscale times that enters the BatchNorm.  (The apply kernels scale the masked gradient, the reduce kernel masks
// the scaled one: the same values, each in the order its sums were pinned with.)
__device__ __forceinline__ float4 bn_residual_mask(const float4 d, const float4 y) {
    return make_float4(y.x > 0.f ? d.x : 0.f, y.y > 0.f ? d.y : 0.f, y.z > 0.f ? d.z : 0.f, y.w > 0.f ? d.w : 0.f);
}
__device__ __forceinline__ float4 bn_scale(const float4 d, const float s) {
    return make_float4(d.x * s, d.y * s, d.z * s, d.w * s);
}

// the reduce step: s1 += d (dbeta), s2 += d * xhat (dgamma)
__device__ __forceinline__ void bn_accumulate(float4 &s1, float4 &s2, const float4 d, const float4 h) {
    s1.x += d.x; s1.y += d.y; s1.z += d.z; s1.w += d.w;
    s2.x = __builtin_fmaf(d.x, h.x, s2.x); s2.y = __builtin_fmaf(d.y, h.y, s2.y);
    s2.z = __builtin_fmaf(d.z, h.z, s2.z); s2.w = __builtin_fmaf(d.w, h.w, s2.w);
}

// gx = gamma * rstd * (d - dbeta/n - xhat * dgamma/n)   (training);   gamma * rstd * d   (eval)
__device__ __forceinline__ float4 bn_gx(const float4 g, const float4 rs, const float4 d, const float4 db, const float4 dg,
                                        const float4 h, const float inv_n, const int training) {
    float4 o;
    if (training) {
        o.x = g.x * rs.x * (d.x - db.x * inv_n - h.x * dg.x * inv_n);
        o.y = g.y * rs.y * (d.y - db.y * inv_n - h.y * dg.y * inv_n);
        o.z = g.z * rs.z * (d.z - db.z * inv_n - h.z * dg.z * inv_n);
        o.w = g.w * rs.w * (d.w - db.w * inv_n - h.w * dg.w * inv_n);
    } else {
        o.x = g.x * rs.x * d.x; o.y = g.y * rs.y * d.y; o.z = g.z * rs.z * d.z; o.w = g.w * rs.w * d.w;
    }
    return o;
}

}  // namespace dense
