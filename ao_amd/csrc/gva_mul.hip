// ao_amd/csrc/gva_mul.hip -- the logits stage of PT-v2m1's grouped vector attention: GroupedLinear as the first layer of
// weight_encoding and the position multiplier linear_p_multiplier (include/ptv2_v2m1_hip.h states the formulas).
//
// Reference op: GroupedVectorAttention.forward, point_transformer_v2m1_origin.py:141-159 with pe_multiplier = pe_bias = True:
//   relation_qk = (key[idx] - query) * linear_p_multiplier(pos) + linear_p_bias(pos);  W1 = GroupedLinear(relation_qk)
// The multiplier pem = Pm Wm2^T + bm2 is a dense (N K, C) x (C, C) product that the factorisation kW[idx] - qW of the
// PT-v2m2 kernels does not survive; the bias part still folds into P M + cW (gva.py), so it is left to the logits kernels
// that exist (called from the launchers below with kW = qW = 0) and this unit adds the multiplier term
//   W1[r, j] += sum_{ch in j} w[ch] (key[idx_r, ch] mask_r - query[n_r, ch]) pem[r, ch]          r = n K + s, 8 channels per group
// and everything that differentiates it.  The unit of work is a TILE OF 16 SLOTS r (consecutive rows of the (N K) axis) of
// one wavefront:
//   Pm tile  (16 x C) = ReLU(pos a_m^T + b_m) is built in LDS (pitch = 4 mod 64: the 16 rows of a ds_read_b128 on 16 banks)
//   pem tile (16 x 16 channels) = Pm tile x Wm2[16 channels, :]^T on v_mfma_f32_16x16x4_f32, Wm2 streamed from L2 in chunks of
//            16 columns (a float4 per lane and chunk; never staged whole: it is 1 MB at C = 512)
//   epilogue lane = (channel, 4 slots): the gathered key rows, the 8-channel group sums on DPP
// forward:   one pass over the tiles; W1 read-modify-write, the column sums T1 / T2 as per-workgroup records
// backward:  rows pass (tiles again; NW wavefronts of a workgroup side by side): pem again, then g_w, g_bm2, g_query, the
//            tile of g_pem = gWt w rel into LDS, g_Pm = g_pem Wm2 -> (g_a_m, g_b_m) through the ReLU, and
//            g_Wm2 += g_pem^T Pm over the workgroup's NW tiles into the workgroup's own (C x C) record;
//            key pass (a wavefront per point j): the slots of j's inverse list in tiles of 16, pem again, the column sum of
//            gWt w pem over the list in list order -> g_key[j]
// No float atomics; every sum has a fixed order (records are summed by finalize_kernel of gva_common.h).
#include <algorithm>

#include "gva_common.h"
#include "../../include/ptv2_v2m1_hip.h"

namespace gva {
namespace mul {

constexpr size_t PART_BUDGET = (size_t)16 << 20;  // floats of rows-pass records at most
constexpr int ROWS_MAX_BLOCKS = 1024;

template <int C>
struct Cfg {
    static constexpr int G = C / 8, CT = C / 16, CK = C / 16, GT = (G + 15) / 16, G16 = GT * 16, GP = G + 1, PITCH = pitch64(C);
    static constexpr int NW_FWD = C <= 192 ? 4 : 2;              // wavefronts per workgroup: forward and key pass
    static constexpr int NW_ROWS = C <= 192 ? 4 : (C <= 384 ? 2 : 1);  // rows pass (two tiles per wavefront in LDS)
    static constexpr size_t REC = (size_t)C * C + 6 * (size_t)C;  // rows-pass record: g_Wm2 | g_w | g_bm2 | g_a_m xyz | g_b_m
    static constexpr size_t fwd_wave_floats = 16 * (size_t)PITCH + 16 * GP;
    static constexpr size_t key_wave_floats = 16 * (size_t)PITCH + 16 * GP + (size_t)C + 16;
    static constexpr size_t rows_wave_floats = 2 * 16 * (size_t)PITCH + 16 * GP + 64 + 7 * (size_t)C;
    static constexpr size_t shared_floats = 4 * (size_t)C + 2 * G16;
    static_assert(C % 16 == 0 && G * 8 == C, "8 channels per group, whole 16-channel tiles");
};
inline int rows_blocks_cap(size_t rec) { return (int)std::max<size_t>(1, std::min<size_t>(ROWS_MAX_BLOCKS, PART_BUDGET / rec)); }

// D (slot 4 q + r, channel 16 ct + l15) = sum_c' T[slot][c'] Wm2[16 ct + l15][c']: the tile T (16 x C, pitch PITCH) in LDS is
// the A operand, Wm2 streamed in chunks of 16 columns the B operand; two accumulator chains
template <int C>
__device__ __forceinline__ v4f tile_times_rows(const float *tile, const float *__restrict__ Wm2, int ct, int l15, int q) {
    using K = Cfg<C>;
    const float *wrow = Wm2 + (size_t)(16 * ct + l15) * C + 4 * q;
    const float *arow = tile + l15 * K::PITCH + 4 * q;
    v4f d0 = (v4f){0.f, 0.f, 0.f, 0.f}, d1 = (v4f){0.f, 0.f, 0.f, 0.f};
    auto step = [&](int ck, v4f d) -> v4f {
        const float4 wv = *(const float4 *)(wrow + 16 * ck);
        const float4 av = *(const float4 *)(arow + 16 * ck);
        d = mfma4(av.x, wv.x, d);
        d = mfma4(av.y, wv.y, d);
        d = mfma4(av.z, wv.z, d);
        d = mfma4(av.w, wv.w, d);
        return d;
    };
#pragma unroll 2
    for (int ck = 0; ck + 1 < K::CK; ck += 2) {
        d0 = step(ck, d0);
        d1 = step(ck + 1, d1);
    }
    if (K::CK & 1) d0 = step(K::CK - 1, d0);
    return d0 + d1;
}

// what a lane knows of its tile: slot l15 (the rows of the LDS tiles) and slots 4 q + r (the rows of a product's result)
struct TileRows {
    float px, py, pz;    // masked relative position of slot l15
    int src[4];          // neighbour of slot 4 q + r, -1: masked or beyond the end
    long long pt[4];     // point of slot 4 q + r (clamped: always a valid row of query)
    bool ok[4];          // slot 4 q + r exists
};
__device__ __forceinline__ TileRows tile_rows(long long r0, long long rows, int lk, int n, const float *__restrict__ coord,
                                              const int *__restrict__ idx, bool live, int l15, int q) {
    TileRows T;
    const long long row = r0 + l15, rowc = row < rows ? row : rows - 1;
    int s = idx[rowc];
    if (!(live && row < rows && s >= 0 && s < n)) s = -1;
    const long long ps = s >= 0 ? s : 0, pp = rowc >> lk;
    const float sx = coord[3 * ps], sy = coord[3 * ps + 1], sz = coord[3 * ps + 2];
    const float qx = coord[3 * pp], qy = coord[3 * pp + 1], qz = coord[3 * pp + 2];
    T.px = s >= 0 ? sx - qx : 0.f;
    T.py = s >= 0 ? sy - qy : 0.f;
    T.pz = s >= 0 ? sz - qz : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long rr = r0 + 4 * q + r;
        T.src[r] = __shfl(s, 4 * q + r, WAVE);
        T.ok[r] = live && rr < rows;
        T.pt[r] = (rr < rows ? rr : rows - 1) >> lk;
    }
    return T;
}
// row l15 of the Pm tile: channels q, q + 4, ...
template <int C>
__device__ __forceinline__ void build_pm(float *sPm, const float4 *sABm, float px, float py, float pz, int l15, int q) {
    for (int cc = q; cc < C; cc += 4) {
        const float4 ab = sABm[cc];
        sPm[l15 * Cfg<C>::PITCH + cc] = pe_act(ab.x, ab.y, ab.z, ab.w, px, py, pz);
    }
}

// ================================================================================================== forward ==
// W1 holds P M + cW on entry.  part[blockIdx.x][2 G] = column sums of W1 and of W1^2 over the workgroup's tiles
template <int C, int NW>
__global__ __launch_bounds__(64 * NW) void mul_logits_fwd_kernel(long long rows, int lk, int n, const float *__restrict__ key,
                                                                 const float *__restrict__ query, const float *__restrict__ w,
                                                                 const float *__restrict__ a_m, const float *__restrict__ b_m,
                                                                 const float *__restrict__ Wm2, const float *__restrict__ bm2,
                                                                 const float *__restrict__ coord, const int *__restrict__ idx,
                                                                 float *__restrict__ W1, float *__restrict__ part) {
    using K = Cfg<C>;
    constexpr int G = K::G, GT = K::GT, G16 = K::G16, GP = K::GP;
    extern __shared__ float4 lds4[];
    float4 *sABm = lds4;                               // [C]  (a_m.xyz, b_m)
    float *sRed = (float *)(sABm + C);                 // [NW][2 G16]
    float *wave0 = sRed + NW * 2 * G16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, q = lane >> 4;
    float *sPm = wave0 + (size_t)wid * K::fwd_wave_floats;  // [16][PITCH]
    float *sW = sPm + 16 * K::PITCH;                        // [16][GP]  the multiplier term of W1 (slot, group)
    for (int ch = tid; ch < C; ch += 64 * NW) sABm[ch] = make_float4(a_m[3 * ch], a_m[3 * ch + 1], a_m[3 * ch + 2], b_m[ch]);
    __syncthreads();

    float t1[GT], t2[GT];
#pragma unroll
    for (int t = 0; t < GT; ++t) t1[t] = t2[t] = 0.f;
    const long long ntiles = (rows + 15) / 16;
    for (long long tile = (long long)blockIdx.x * NW + wid; tile < ntiles; tile += (long long)gridDim.x * NW) {
        const long long r0 = tile * 16;
        const TileRows T = tile_rows(r0, rows, lk, n, coord, idx, true, l15, q);
        build_pm<C>(sPm, sABm, T.px, T.py, T.pz, l15, q);
        wave_lds_sync();
#pragma unroll 1
        for (int ct = 0; ct < K::CT; ++ct) {
            const int c = 16 * ct + l15;
            float kv[4], qv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // (requested in front of the product)
                kv[r] = ptv2_ld_or_zero(key + (long long)T.src[r] * C + c, T.src[r] >= 0);
                qv[r] = query[T.pt[r] * C + c];
            }
            const float wc = w[c], bm = bm2[c];
            const v4f D = tile_times_rows<C>(sPm, Wm2, ct, l15, q);
            float val[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) val[r] = row8_sum((kv[r] - qv[r]) * (D[r] + bm) * wc);
            if ((l15 & 7) == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sW[(4 * q + r) * GP + 2 * ct + (l15 >> 3)] = val[r];
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < GT; ++t) {
            const int g = 16 * t + l15, gc = g < G ? g : G - 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long rr = r0 + 4 * q + r;
                const bool ok = rr < rows && g < G;
                float *dst = W1 + (rr < rows ? rr : rows - 1) * G + gc;
                const float v = *dst + sW[(4 * q + r) * GP + gc];
                if (ok) *dst = v;
                t1[t] += ok ? v : 0.f;
                t2[t] = ok ? __builtin_fmaf(v, v, t2[t]) : t2[t];
            }
        }
        wave_lds_sync();  // sW and the Pm tile are rewritten by the next trip
    }
#pragma unroll
    for (int t = 0; t < GT; ++t) {
        t1[t] = quarter_sum_shfl(t1[t]);
        t2[t] = quarter_sum_shfl(t2[t]);
        if (q == 0) { sRed[wid * 2 * G16 + 16 * t + l15] = t1[t]; sRed[wid * 2 * G16 + G16 + 16 * t + l15] = t2[t]; }
    }
    __syncthreads();
    if (tid < 2 * G) {
        const int col = tid < G ? tid : G16 + (tid - G);
        float v = 0.f;
        for (int wv = 0; wv < NW; ++wv) v += sRed[wv * 2 * G16 + col];
        part[(size_t)blockIdx.x * 2 * G + tid] = v;
    }
}

// ============================================================================================ backward: rows ==
// gWt tile (16 x G) of the slots r0 .. r0 + 15 into LDS; rows beyond the end (or of a wavefront without a tile) are zero
template <int C>
__device__ __forceinline__ void build_gwt(float *sG, const float *sC1, const float *sC2, long long r0, long long rows, bool live,
                                          const float *__restrict__ W1, const float *__restrict__ gW1, int lane) {
    constexpr int G = Cfg<C>::G, GP = Cfg<C>::GP;
    for (int e = lane; e < 16 * G; e += 64) {
        const int rr = e / G, gg = e - rr * G;
        const bool ok = live && r0 + rr < rows;
        const float wv = ptv2_ld_or_zero(W1 + r0 * G + e, ok), gv = ptv2_ld_or_zero(gW1 + r0 * G + e, ok);
        sG[rr * GP + gg] = ok ? __builtin_fmaf(wv, sC2[gg], gv + sC1[gg]) : 0.f;
    }
}

// wpart[blockIdx.x][REC]
template <int C, int NW>
__global__ __launch_bounds__(64 * NW) void mul_logits_bwd_rows_kernel(
    long long rows, int lk, int n, const float *__restrict__ key, const float *__restrict__ query, const float *__restrict__ w,
    const float *__restrict__ a_m, const float *__restrict__ b_m, const float *__restrict__ Wm2, const float *__restrict__ bm2,
    const float *__restrict__ coord, const int *__restrict__ idx, const float *__restrict__ W1, const float *__restrict__ gW1,
    const double *__restrict__ gT1, const double *__restrict__ gT2, float *__restrict__ g_query, float *__restrict__ wpart) {
    using K = Cfg<C>;
    constexpr int G = K::G, G16 = K::G16, GP = K::GP, PITCH = K::PITCH, CT = K::CT, CK = K::CK;
    extern __shared__ float4 lds4[];
    float4 *sABm = lds4;                              // [C]
    float *sC1 = (float *)(sABm + C);                 // [G16]  gT1
    float *sC2 = sC1 + G16;                           // [G16]  2 gT2
    float *wave0 = sC2 + G16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, q = lane >> 4;
    auto wave_base = [&](int wv) { return wave0 + (size_t)wv * K::rows_wave_floats; };
    float *sPm = wave_base(wid);                      // [16][PITCH]
    float *sGp = sPm + 16 * PITCH;                    // [16][PITCH]  g_pem = gWt w rel
    float4 *sPos = (float4 *)(sGp + 16 * PITCH);      // [16]
    float *sG = (float *)(sPos + 16);                 // [16][GP]     gWt
    float *sQ = sG + 16 * GP;                         // [C]          g_query of a point with more than 16 slots
    float *sVec = sQ + C;                             // [6][C]       g_w | g_bm2 | g_a_m x, y, z | g_b_m of this wavefront
    for (int ch = tid; ch < C; ch += 64 * NW) sABm[ch] = make_float4(a_m[3 * ch], a_m[3 * ch + 1], a_m[3 * ch + 2], b_m[ch]);
    for (int j = tid; j < G16; j += 64 * NW) {
        sC1[j] = j < G ? (float)gT1[j] : 0.f;
        sC2[j] = j < G ? 2.f * (float)gT2[j] : 0.f;
    }
    for (int e = lane; e < 7 * C; e += 64) sQ[e] = 0.f;  // (sQ and sVec are adjacent)
    __syncthreads();

    const int k = 1 << lk, SUB = k > 16 ? k / 16 : 1;
    const long long ntiles = (rows + 15) / 16, units = (ntiles + SUB - 1) / SUB;
    float *rec = wpart + (size_t)blockIdx.x * K::REC;
    bool first = true;
    for (long long ub = (long long)blockIdx.x * NW; ub < units; ub += (long long)gridDim.x * NW) {
        const long long unit = ub + wid;
        const bool live = unit < units;
        for (int sub = 0; sub < SUB; ++sub) {  // (uniform over the workgroup: it meets at the barriers below)
            const long long tile = live ? unit * SUB + sub : 0, r0 = tile * 16;
            const TileRows T = tile_rows(r0, rows, lk, n, coord, idx, live, l15, q);
            sPos[l15] = make_float4(T.px, T.py, T.pz, 0.f);
            build_gwt<C>(sG, sC1, sC2, r0, rows, live, W1, gW1, lane);
            build_pm<C>(sPm, sABm, T.px, T.py, T.pz, l15, q);
            wave_lds_sync();
            // ---- pem again; g_w, g_bm2, g_query; the g_pem tile
#pragma unroll 1
            for (int ct = 0; ct < CT; ++ct) {
                const int c = 16 * ct + l15;
                float kv[4], qv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    kv[r] = ptv2_ld_or_zero(key + (long long)T.src[r] * C + c, T.src[r] >= 0);
                    qv[r] = query[T.pt[r] * C + c];
                }
                const float wc = w[c], bm = bm2[c];
                const v4f D = tile_times_rows<C>(sPm, Wm2, ct, l15, q);
                float aw = 0.f, abm = 0.f, gq[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gw = sG[(4 * q + r) * GP + (c >> 3)];  // (zero for a slot that does not exist)
                    const float rel = kv[r] - qv[r], pem = D[r] + bm, u = gw * wc;
                    aw = __builtin_fmaf(gw * rel, pem, aw);
                    const float gp = u * rel;
                    abm += gp;
                    gq[r] = u * pem;
                    sGp[(4 * q + r) * PITCH + c] = gp;
                }
                aw = quarter_sum_shfl(aw);
                abm = quarter_sum_shfl(abm);
                if (q == 0) { sVec[c] += aw; sVec[C + c] += abm; }
                // g_query[point] = - sum over the point's k slots (slot 4 q + r of the tile)
                const float s01 = gq[0] + gq[1], s23 = gq[2] + gq[3];
                float s = s01 + s23;
                if (k == 2) {
                    if (T.ok[0]) g_query[T.pt[0] * C + c] = -s01;
                    if (T.ok[2]) g_query[T.pt[2] * C + c] = -s23;
                } else if (k == 4) {
                    if (T.ok[0]) g_query[T.pt[0] * C + c] = -s;
                } else if (k == 8) {
                    s += __shfl_xor(s, 16, WAVE);
                    if (!(q & 1) && T.ok[0]) g_query[T.pt[0] * C + c] = -s;
                } else {
                    s = quarter_sum_shfl(s);
                    if (q == 0) {
                        if (SUB > 1) {
                            const float acc = sub ? sQ[c] + s : s;
                            sQ[c] = acc;
                            s = acc;
                        }
                        if (sub == SUB - 1 && T.ok[0]) g_query[T.pt[0] * C + c] = -s;
                    }
                }
            }
            wave_lds_sync();
            // ---- g_Pm (slot, c') = sum_ch g_pem[slot][ch] Wm2[ch][c'] -> through the ReLU of Pm -> g_a_m, g_b_m
#pragma unroll 1
            for (int ctp = 0; ctp < CT; ++ctp) {
                const int cp = 16 * ctp + l15;
                const float *arow = sGp + l15 * PITCH + 4 * q;
                const float *bcol = Wm2 + (size_t)(4 * q) * C + cp;
                v4f d0 = (v4f){0.f, 0.f, 0.f, 0.f}, d1 = (v4f){0.f, 0.f, 0.f, 0.f};
                auto step = [&](int ck, v4f d) -> v4f {
                    const float4 av = *(const float4 *)(arow + 16 * ck);
                    const float *bp = bcol + (size_t)(16 * ck) * C;
                    const float b0 = bp[0], b1 = bp[C], b2 = bp[2 * C], b3 = bp[3 * C];
                    d = mfma4(av.x, b0, d);
                    d = mfma4(av.y, b1, d);
                    d = mfma4(av.z, b2, d);
                    d = mfma4(av.w, b3, d);
                    return d;
                };
#pragma unroll 2
                for (int ck = 0; ck + 1 < CK; ck += 2) {
                    d0 = step(ck, d0);
                    d1 = step(ck + 1, d1);
                }
                if (CK & 1) d0 = step(CK - 1, d0);
                const v4f D3 = d0 + d1;
                float ax = 0.f, ay = 0.f, az = 0.f, ab = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pm = sPm[(4 * q + r) * PITCH + cp];
                    const float gpre = pm > 0.f ? D3[r] : 0.f;
                    const float4 p4 = sPos[4 * q + r];
                    ax = __builtin_fmaf(gpre, p4.x, ax);
                    ay = __builtin_fmaf(gpre, p4.y, ay);
                    az = __builtin_fmaf(gpre, p4.z, az);
                    ab += gpre;
                }
                ax = quarter_sum_shfl(ax); ay = quarter_sum_shfl(ay); az = quarter_sum_shfl(az); ab = quarter_sum_shfl(ab);
                if (q == 0) { sVec[2 * C + cp] += ax; sVec[3 * C + cp] += ay; sVec[4 * C + cp] += az; sVec[5 * C + cp] += ab; }
            }
            // ---- g_Wm2 (ch, c') += sum over the NW tiles' slots g_pem[slot][ch] Pm[slot][c']: the output tiles dealt to the wavefronts
            __syncthreads();
#pragma unroll 1
            for (int o = wid; o < CT * CT; o += NW) {
                const int i = o / CT, j = o - i * CT;
                float *dst = rec + (size_t)(16 * i + 4 * q) * C + 16 * j + l15;
                v4f acc = (v4f){0.f, 0.f, 0.f, 0.f};
                if (!first) { acc[0] = dst[0]; acc[1] = dst[C]; acc[2] = dst[2 * C]; acc[3] = dst[3 * C]; }
#pragma unroll
                for (int wv = 0; wv < NW; ++wv) {
                    const float *tp = wave_base(wv), *tg = tp + 16 * PITCH;
#pragma unroll
                    for (int st = 0; st < 4; ++st)
                        acc = mfma4(tg[(4 * st + q) * PITCH + 16 * i + l15], tp[(4 * st + q) * PITCH + 16 * j + l15], acc);
                }
                dst[0] = acc[0]; dst[C] = acc[1]; dst[2 * C] = acc[2]; dst[3 * C] = acc[3];
            }
            first = false;
            __syncthreads();  // the tiles are rewritten by the next trip
        }
    }
    // the wavefronts' vectors, added in wavefront order
    for (int e = tid; e < 6 * C; e += 64 * NW) {
        float v = 0.f;
        for (int wv = 0; wv < NW; ++wv) v += (wave_base(wv) + 2 * 16 * PITCH + 64 + 16 * GP + C)[e];
        rec[(size_t)C * C + e] = v;
    }
}

struct MapMulParams {  // record columns -> g_Wm2 (c,c), g_w, g_bm2, g_a_m (c,3), g_b_m
    float *gWm2, *gw, *gbm2, *gam, *gbm;
    int c;
    __device__ void operator()(int e, double v) const {
        const int cc = c * c;
        if (e < cc) { gWm2[e] = (float)v; return; }
        const int f = e - cc, which = f / c, ch = f - which * c;
        if (which == 0) gw[ch] = (float)v;
        else if (which == 1) gbm2[ch] = (float)v;
        else if (which < 5) gam[ch * 3 + (which - 2)] = (float)v;
        else gbm[ch] = (float)v;
    }
};

// ============================================================================================= backward: key ==
// g_key[j] = sum over the slots r of j's inverse list (list order) of gWt[r, group] w pem[r]; every slot of the list names j,
// so its position is coord[j] - coord[point of r]
template <int C, int NW>
__global__ __launch_bounds__(64 * NW) void mul_logits_bwd_key_kernel(
    long long rows, int lk, int n, const float *__restrict__ w, const float *__restrict__ a_m, const float *__restrict__ b_m,
    const float *__restrict__ Wm2, const float *__restrict__ bm2, const float *__restrict__ coord, const float *__restrict__ W1,
    const float *__restrict__ gW1, const double *__restrict__ gT1, const double *__restrict__ gT2, const int *__restrict__ inv_ptr,
    const int *__restrict__ inv_rows, float *__restrict__ g_key) {
    using K = Cfg<C>;
    constexpr int G = K::G, G16 = K::G16, GP = K::GP, PITCH = K::PITCH;
    extern __shared__ float4 lds4[];
    float4 *sABm = lds4;
    float *sC1 = (float *)(sABm + C);
    float *sC2 = sC1 + G16;
    float *wave0 = sC2 + G16;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, q = lane >> 4;
    float *sPm = wave0 + (size_t)wid * K::key_wave_floats;  // [16][PITCH]
    float *sG = sPm + 16 * PITCH;                           // [16][GP]
    float *sK = sG + 16 * GP;                               // [C]
    int *sRow = (int *)(sK + C);                            // [16]  slot of list entry l15, -1 beyond the list
    for (int ch = tid; ch < C; ch += 64 * NW) sABm[ch] = make_float4(a_m[3 * ch], a_m[3 * ch + 1], a_m[3 * ch + 2], b_m[ch]);
    for (int j = tid; j < G16; j += 64 * NW) {
        sC1[j] = j < G ? (float)gT1[j] : 0.f;
        sC2[j] = j < G ? 2.f * (float)gT2[j] : 0.f;
    }
    __syncthreads();
    for (long long j = (long long)blockIdx.x * NW + wid; j < n; j += (long long)gridDim.x * NW) {
        long long beg = inv_ptr[j], end = inv_ptr[j + 1];
        beg = beg < 0 ? 0 : (beg > rows ? rows : beg);
        end = end > rows ? rows : end;
        for (int c = lane; c < C; c += 64) sK[c] = 0.f;
        const float jx = coord[3 * j], jy = coord[3 * j + 1], jz = coord[3 * j + 2];
        for (long long base = beg; base < end; base += 16) {
            const bool ok = base + l15 < end;
            long long r = inv_rows[ok ? base + l15 : beg];
            r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
            const long long pp = r >> lk;
            const float px = ok ? jx - coord[3 * pp] : 0.f, py = ok ? jy - coord[3 * pp + 1] : 0.f, pz = ok ? jz - coord[3 * pp + 2] : 0.f;
            if (q == 0) sRow[l15] = ok ? (int)r : -1;
            build_pm<C>(sPm, sABm, px, py, pz, l15, q);
            wave_lds_sync();
            for (int e = lane; e < 16 * G; e += 64) {
                const int rr = e / G, gg = e - rr * G;
                const int row = sRow[rr];
                const size_t o = (size_t)(row >= 0 ? row : 0) * G + gg;
                const float wv = W1[o], gv = gW1[o];
                sG[rr * GP + gg] = row >= 0 ? __builtin_fmaf(wv, sC2[gg], gv + sC1[gg]) : 0.f;
            }
            wave_lds_sync();
#pragma unroll 1
            for (int ct = 0; ct < K::CT; ++ct) {
                const int c = 16 * ct + l15;
                const float wc = w[c], bm = bm2[c];
                const v4f D = tile_times_rows<C>(sPm, Wm2, ct, l15, q);
                float s = 0.f;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) s = __builtin_fmaf(sG[(4 * q + r4) * GP + (c >> 3)] * wc, D[r4] + bm, s);
                s = quarter_sum_shfl(s);
                if (q == 0) sK[c] += s;
            }
            wave_lds_sync();
        }
        wave_lds_sync();
        for (int c = lane; c < C; c += 64) g_key[j * C + c] = sK[c];
        wave_lds_sync();
    }
}

template <int C>
static int launch_fwd(int n, int k, int lk, const float *key, const float *query, const float *w, const float *a_m, const float *b_m,
                      const float *Wm2, const float *bm2, const float *coord, const int *idx, float *W1, double *T1, double *T2,
                      float *part, hipStream_t st) {
    using K = Cfg<C>;
    constexpr int NW = K::NW_FWD;
    const size_t lds = sizeof(float) * (K::shared_floats + (size_t)NW * 2 * K::G16 + (size_t)NW * K::fwd_wave_floats);
    auto kern = mul_logits_fwd_kernel<C, NW>;
    RUN(ptv2_kernel_lds((const void *)kern, lds));
    const long long rows = (long long)n * k, ntiles = (rows + 15) / 16;
    const int nblk = (int)std::max<long long>(1, std::min<long long>((ntiles + NW - 1) / NW, MAX_BLOCKS));
    hipLaunchKernelGGL(kern, dim3(nblk), dim3(64 * NW), lds, st, rows, lk, n, key, query, w, a_m, b_m, Wm2, bm2, coord, idx, W1, part);
    launch_finalize(st, (const float *)part, nblk, 2 * K::G, MapSplit2<double>{T1, T2, K::G});
    return PTV2_OK;
}

template <int C>
static int launch_bwd(int n, int k, int lk, const float *key, const float *query, const float *w, const float *a_m, const float *b_m,
                      const float *Wm2, const float *bm2, const float *coord, const int *idx, const float *W1, const float *gW1,
                      const double *gT1, const double *gT2, const int *inv_ptr, const int *inv_rows, float *g_key, float *g_query,
                      float *g_w, float *g_Wm2, float *g_bm2, float *g_a_m, float *g_b_m, float *wpart, hipStream_t st) {
    using K = Cfg<C>;
    const long long rows = (long long)n * k, ntiles = (rows + 15) / 16;
    {
        constexpr int NW = K::NW_ROWS;
        const size_t lds = sizeof(float) * (K::shared_floats + (size_t)NW * K::rows_wave_floats);
        auto kern = mul_logits_bwd_rows_kernel<C, NW>;
        RUN(ptv2_kernel_lds((const void *)kern, lds));
        const int sub = k > 16 ? k / 16 : 1;
        const long long units = (ntiles + sub - 1) / sub;
        const int nblk = (int)std::max<long long>(1, std::min<long long>((units + NW - 1) / NW, rows_blocks_cap(K::REC)));
        hipLaunchKernelGGL(kern, dim3(nblk), dim3(64 * NW), lds, st, rows, lk, n, key, query, w, a_m, b_m, Wm2, bm2, coord, idx, W1, gW1,
                           gT1, gT2, g_query, wpart);
        launch_finalize(st, (const float *)wpart, nblk, (int)K::REC, MapMulParams{g_Wm2, g_w, g_bm2, g_a_m, g_b_m, C});
    }
    {
        constexpr int NW = K::NW_FWD;
        const size_t lds = sizeof(float) * (K::shared_floats + (size_t)NW * K::key_wave_floats);
        auto kern = mul_logits_bwd_key_kernel<C, NW>;
        RUN(ptv2_kernel_lds((const void *)kern, lds));
        const int nblk = (int)std::max<long long>(1, std::min<long long>(((long long)n + NW - 1) / NW, MAX_BLOCKS));
        hipLaunchKernelGGL(kern, dim3(nblk), dim3(64 * NW), lds, st, rows, lk, n, w, a_m, b_m, Wm2, bm2, coord, W1, gW1, gT1, gT2, inv_ptr,
                           inv_rows, g_key);
    }
    return PTV2_OK;
}

static bool shape_ok(int n, int k, int c, int g) {
    if (n < 1 || k < 2 || k > 64 || (k & (k - 1)) != 0 || (long long)n * k >= (1ll << 31)) return false;
    return (c == 48 && g == 6) || (c == 96 && g == 12) || (c == 192 && g == 24) || (c == 384 && g == 48) || (c == 512 && g == 64);
}
static int log2i(int k) { int l = 0; while ((1 << l) < k) ++l; return l; }

// workspace: [the logits kernels' own workspace][zeros / scratch (2 n g)][records]
struct Carve { char *inner; size_t inner_bytes; float *ng; float *part; size_t total; };
static Carve carve(void *ws, int n, int k, int c, int g) {
    PtvCarver cv{(char *)ws, 0};
    Carve o;
    o.inner_bytes = gva_workspace_bytes(n, k, c, g);
    o.inner = cv.take(o.inner_bytes);
    o.ng = cv.take_n<float>(2 * (size_t)n * g);
    const size_t rec = (size_t)c * c + 6 * (size_t)c;
    o.part = cv.take_n<float>(std::max((size_t)rows_blocks_cap(rec) * rec, (size_t)MAX_BLOCKS * 2 * g));
    o.total = cv.off;
    return o;
}

}  // namespace mul
}  // namespace gva

extern "C" int ptv2_v2m1_abi_version(void) { return 1; }

extern "C" size_t gva_mul_workspace_bytes(int n, int k, int c, int g) {
    if (!gva::mul::shape_ok(n, k, c, g)) return 0;
    return gva::mul::carve(nullptr, n, k, c, g).total;
}

#define GVA_MUL_DISPATCH_C(c, CALL) \
    switch (c) {                    \
        case 48: rc = CALL(48); break;   \
        case 96: rc = CALL(96); break;   \
        case 192: rc = CALL(192); break; \
        case 384: rc = CALL(384); break; \
        default: rc = CALL(512); break;  \
    }

extern "C" int gva_mul_logits_forward_hip_launcher(int n, int k, int c, int g, const float *key, const float *query, const float *w,
                                                   const float *a_m, const float *b_m, const float *Wm2, const float *bm2,
                                                   const float *a, const float *b, const float *M, const float *cW,
                                                   const float *coord, const int *idx, float *W1, double *T1, double *T2,
                                                   void *workspace, size_t workspace_bytes, void *stream) {
    using namespace gva::mul;
    if (!key || !query || !w || !a_m || !b_m || !Wm2 || !bm2 || !a || !b || !M || !cW || !coord || !idx || !W1 || !T1 || !T2 || !workspace)
        return PTV2_ERR_ARG;
    if (!shape_ok(n, k, c, g)) return PTV2_ERR_ARG;
    const Carve cv = carve(workspace, n, k, c, g);
    if (workspace_bytes < cv.total) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // the bias part P M + cW of every slot: the logits stage that exists, with kW = qW = 0
    if (hipMemsetAsync(cv.ng, 0, sizeof(float) * (size_t)n * g, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    RUN(gva_logits_forward_hip_launcher(n, k, c, g, cv.ng, cv.ng, a, b, M, cW, coord, idx, W1, T1, T2, cv.inner, cv.inner_bytes, stream));
    const int lk = log2i(k);
    int rc;
#define CALL(CC) launch_fwd<CC>(n, k, lk, key, query, w, a_m, b_m, Wm2, bm2, coord, idx, W1, T1, T2, cv.part, st)
    GVA_MUL_DISPATCH_C(c, CALL)
#undef CALL
    if (rc != PTV2_OK) return rc;
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int gva_mul_logits_backward_hip_launcher(int n, int k, int c, int g, const float *key, const float *query, const float *w,
                                                    const float *a_m, const float *b_m, const float *Wm2, const float *bm2,
                                                    const float *a, const float *b, const float *M, const float *coord,
                                                    const int *idx, const float *W1, const float *gW1, const double *gT1,
                                                    const double *gT2, const int *inv_ptr, const int *inv_rows, float *g_key,
                                                    float *g_query, float *g_w, float *g_Wm2, float *g_bm2, float *g_a_m,
                                                    float *g_b_m, float *g_a, float *g_b, float *g_M, float *g_cW, void *workspace,
                                                    size_t workspace_bytes, void *stream) {
    using namespace gva::mul;
    if (!key || !query || !w || !a_m || !b_m || !Wm2 || !bm2 || !a || !b || !M || !coord || !idx || !W1 || !gW1 || !gT1 || !gT2 ||
        !inv_ptr || !inv_rows || !g_key || !g_query || !g_w || !g_Wm2 || !g_bm2 || !g_a_m || !g_b_m || !g_a || !g_b || !g_M || !g_cW ||
        !workspace)
        return PTV2_ERR_ARG;
    if (!shape_ok(n, k, c, g)) return PTV2_ERR_ARG;
    const Carve cv = carve(workspace, n, k, c, g);
    if (workspace_bytes < cv.total) return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // the bias part: g_a, g_b, g_M, g_cW depend on gWt and P alone (its gkW / gqW go to scratch)
    RUN(gva_logits_backward_hip_launcher(n, k, c, g, a, b, M, coord, idx, W1, gW1, gT1, gT2, inv_ptr, inv_rows, cv.ng,
                                         cv.ng + (size_t)n * g, g_a, g_b, g_M, g_cW, cv.inner, cv.inner_bytes, stream));
    const int lk = log2i(k);
    int rc;
#define CALL(CC) launch_bwd<CC>(n, k, lk, key, query, w, a_m, b_m, Wm2, bm2, coord, idx, W1, gW1, gT1, gT2, inv_ptr, inv_rows, g_key, \
                                g_query, g_w, g_Wm2, g_bm2, g_a_m, g_b_m, cv.part, st)
    GVA_MUL_DISPATCH_C(c, CALL)
#undef CALL
    if (rc != PTV2_OK) return rc;
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
