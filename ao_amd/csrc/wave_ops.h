// ao_amd/csrc/wave_ops.h -- the wavefront idioms of the matrix-core kernels (the attention family, gemm.hip, wgrad.hip,
// spconv.hip), each stated once.  common.h includes it.  Everything here is __forceinline__ or constexpr: no symbol of its
// own, and a kernel's instructions do not depend on which unit spells the idiom (tools/isa_diff.py is the check).
#pragma once

typedef float v4f __attribute__((ext_vector_type(4)));  // accumulator tile of the fp32 16x16x4 matrix instruction

// V_MFMA_F32_16X16X4_F32: c (16 x 16, 4 values per lane) += a (16 x 4, one value per lane) b (4 x 16, one value per lane)
__device__ __forceinline__ v4f mfma4(float a, float b, v4f c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// all-reduce over the 16 lanes of a DPP row (lanes that share lane >> 4)
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    return v;
}
// all-reduce over the 8 lanes that share lane >> 3: the first three steps of row16_sum
__device__ __forceinline__ float row8_sum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    return v;
}

// v + the same lane of the other three lane quarters (lane ^ 16, then lane ^ 32), fixed order.  Two forms, because they are
// different instructions and both are in use -- a kernel keeps the one it was measured with:
//   quarter_sum_shfl  two __shfl_xor (gva_mul.hip)
//   quarter_sum_swap  without the LDS crossbar: gfx950 swaps rows / halves (v_permlane16_swap, v_permlane32_swap; gva_bwd_tile.hip)
__device__ __forceinline__ float quarter_sum_shfl(float v) {
    v += __shfl_xor(v, 16, WAVE);
    v += __shfl_xor(v, 32, WAVE);
    return v;
}
__device__ __forceinline__ float quarter_sum_swap(float v) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float h = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(h), __float_as_uint(h), false, false);
    return __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
}

// LDS hand-off inside a wavefront (a wave-private tile or record written in one lane layout and read in another), two forms:
//   wave_lds_sync    the wavefront's LDS operations complete in order once counted down; the compiler must not move LDS
//                    accesses across.  The form to use.
//   wave_fence_sync  a wavefront-scope fence.  It also waits for the wavefront's GLOBAL stores -- vmcnt(0): ~2 us per point
//                    behind the gW1 stores of gva_bwd_tile.hip's tail, which is why the tile kernels left it.  gva_fwd_point.hip,
//                    gva_bwd_point.hip and gva_bwd_logits.hip still use it: replacing it changes their instructions and nobody
//                    has measured that yet -- a candidate for a later, measured change, one kernel at a time.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void wave_fence_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// LDS pitch: the smallest p >= x, reached from x in steps of `step`, with p = 4 mod `mod`
__host__ __device__ constexpr int lds_pitch(int x, int mod, int step) {
    int p = x;
    while (p % mod != 4) p += step;
    return p;
}
// rows of x floats read one float per lane: = 4 mod 16 puts the 4 lane quarters on disjoint LDS banks
__host__ __device__ constexpr int pitch16(int x) { return lds_pitch(x, 16, 1); }
// records of x floats (x % 4 == 0) read with ds_read_b128: = 4 mod 64 puts the 16 records of a read on 16 distinct 16-byte slots
__host__ __device__ constexpr int pitch64(int x) { return lds_pitch(x, 64, 4); }
// the values in use: a Cfg that moves one of these changes an LDS image
static_assert(pitch16(6) == 20 && pitch16(12) == 20 && pitch16(24) == 36 && pitch16(48) == 52 && pitch16(64) == 68, "pitch16");
static_assert(pitch64(48) == 68 && pitch64(80) == 132 && pitch64(96) == 132 && pitch64(160) == 196 && pitch64(192) == 196 &&
              pitch64(240) == 260 && pitch64(320) == 324 && pitch64(384) == 388 && pitch64(480) == 516 && pitch64(512) == 516 &&
              pitch64(960) == 964, "pitch64");
