// ao_amd/csrc/lovasz.hip -- multiclass Lovasz-softmax loss (pointcept/models/losses/lovasz.py:211-253, mode="multiclass",
// per_image=False: the LovaszLoss entry of configs/scannet/semseg-pt-v2m2-3-lovasz.py and its ScanNet200 / SemanticKITTI
// siblings) for (N, C <= 1024) fp32 logits, without a host synchronisation and with a launch count that does not depend on
// the number of classes present.
//
// Contract.  p = softmax(logits) per row (fp32: m = max, s = sum_j expf(x_j - m) in column order, p_c = expf(x_c - m) / s).
// Rows used: label != ignore_index (every row when there is no ignore_index).  Classes: those present among the used rows,
// ascending, limited to class_seen when a mask is given; each takes a SLOT (0 .. nseg-1, ascending class).  For a class:
// e = |fg - p_c| over the used rows, sorted descending; ties keep ascending row order (a stable sort; the reference's
// torch.sort leaves it open, and the gradient depends on it).  g = _lovasz_grad(fg_sorted) (:22-33) evaluated with the
// reference's fp32 formula: I_k = gts - cumfg_k, U_k = gts + (k + 1 - cumfg_k), J_k = 1 - I_k / U_k, g_0 = J_0,
// g_k = J_k - J_{k-1}; J_{k-1} is the same formula at (k - 1, cumfg_k - fg_k), so one exclusive scan of fg gives g bit for
// bit.  loss = weight * mean over slots of dot(e_sorted, g) (the dot products and the mean are summed in double).
// Backward: the sort permutation is a constant, dL/dp[i,c] = -sign(fg - p) * g_rank(i) / nseg (sign(0) = 0, torch's abs),
// then through the softmax Jacobian; unused rows get 0.
// Edge cases: no slot (no used row, or no present class in class_seen) -> loss 0 and a zero gradient; a label that is
// neither ignore_index nor in [0, c) -> that row is not used and the loss is NaN (bad_labels counts them, as the
// cross-entropy of loss.hip); n >= 2^24 rows -> PTV2_ERR_ARG (fp32 counts stop being exact there).  C == 1 is refused by
// the Python layer (ValueError, lovasz.py:135-137).
//
// Launches (forward 18, backward 1):
//   memset   the per-call counters
//   count    per 1024-row block: used rows (-> the rank scan), rows per class (LDS histogram, then integer atomics)
//   plan     one workgroup: exclusive scan of the block counts, class -> slot table, nseg
//   rows     softmax per used row; its rank among the used rows; one (key, value) per (row, slot) at slot * nlab + rank,
//            key = 0x3F800000 - bits(e) (ascending key = descending e, 30 bits), value = rank | fg << 31
//   sort     stable LSD radix sort of every slot's segment by key, 8-bit digits, 4 passes of (hist, scan, scatter).
//            Segments are sorted side by side: a workgroup owns one 4096-element chunk of one segment, the digit counts are
//            kept per (segment, digit, chunk) and scanned per segment, and the scatter ranks a chunk's elements in order
//            (wave ballots + per-wave counts in LDS), so equal keys keep their order.  Grids are sized for
//            min(C, n) segments of n elements; workgroups beyond nseg / nlab (device values) return at once.
//   fgcount  fg per sorted chunk
//   final    exclusive scan of fg per segment -> g per element, e * g summed per chunk, -sign * g written to gs[slot, rank]
//            for the backward; the last workgroup to arrive sums the chunks in a fixed order -> loss (bitwise reproducible)
//   backward one lane per row: gp_j = gs[slot(j), rank] for present classes, g_logits = p * (gp - <gp, p>) * scale
#include "gva_common.h"

namespace {

constexpr int LV_TPB = 256;
constexpr int LV_ROWS = 4 * LV_TPB;         // rows per workgroup of count / rows
constexpr int LV_CHUNK = 4096;              // sorted elements per workgroup of hist / scatter / fgcount / final
constexpr int LV_PER = LV_CHUNK / LV_TPB;   // elements per thread in final
constexpr int LV_SCAN_TPB = 1024;
constexpr int LV_MAX_C = 1024;
constexpr unsigned LV_ONE = 0x3F800000u;
enum { M_NSEG = 0, M_NLAB = 1, M_BAD = 2, M_WORDS = 16 };

struct SavedLayout {  // per call, kept for the backward
    size_t meta, cls_cnt, slot_of, cls_of_slot, rank_of, rowstat, gs, total;
    SavedLayout(int n, int c) {
        const size_t segs = (size_t)std::min(n, c);
        meta = 0;
        cls_cnt = meta + sizeof(int) * M_WORDS;
        slot_of = ptv2_align256(cls_cnt + sizeof(int) * c);
        cls_of_slot = slot_of + ptv2_align256(sizeof(int) * c);
        rank_of = cls_of_slot + ptv2_align256(sizeof(int) * c);
        rowstat = rank_of + ptv2_align256(sizeof(int) * n);
        gs = rowstat + ptv2_align256(sizeof(float) * 2 * n);
        total = gs + ptv2_align256(sizeof(float) * segs * n);
    }
};

struct WsLayout {  // scratch of one forward call
    size_t blkcnt, keys0, vals0, keys1, vals1, cnt, chunkfg, part, total;
    int cps;  // chunks per segment (host bound)
    WsLayout(int n, int c) {
        const size_t segs = (size_t)std::min(n, c), elems = segs * n;
        const int nblk = (n + LV_ROWS - 1) / LV_ROWS;
        cps = (n + LV_CHUNK - 1) / LV_CHUNK;
        blkcnt = 0;
        keys0 = ptv2_align256(sizeof(int) * nblk);
        vals0 = keys0 + ptv2_align256(4 * elems);
        keys1 = vals0 + ptv2_align256(4 * elems);
        vals1 = keys1 + ptv2_align256(4 * elems);
        cnt = vals1 + ptv2_align256(4 * elems);
        chunkfg = cnt + ptv2_align256(sizeof(int) * segs * 256 * cps);
        part = chunkfg + ptv2_align256(sizeof(int) * segs * cps);
        total = part + ptv2_align256(sizeof(double) * segs * cps);
    }
};

__device__ __forceinline__ bool lv_used(long long y, int ignore_index, int has_ignore) {
    return !has_ignore || y != (long long)ignore_index;
}

// exclusive scan of one int per thread over the workgroup (blockDim.x == LV_TPB); returns the exclusive prefix, *total
__device__ __forceinline__ int lv_block_excl(int v, int *s_wave, int *total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < LV_TPB / 64; ++w) {
        const int s = s_wave[w];
        before += w < wid ? s : 0;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(LV_TPB) void lv_count_kernel(int n, int c, const long long *__restrict__ label, int ignore_index,
                                                          int has_ignore, int *__restrict__ meta, int *__restrict__ cls_cnt,
                                                          int *__restrict__ blkcnt) {
    __shared__ int s_hist[LV_MAX_C];
    __shared__ int s_wave[LV_TPB / 64];
    for (int j = threadIdx.x; j < c; j += LV_TPB) s_hist[j] = 0;
    __syncthreads();
    int used = 0, bad = 0;
    for (int i = 0; i < LV_ROWS / LV_TPB; ++i) {
        const long long r = (long long)blockIdx.x * LV_ROWS + i * LV_TPB + threadIdx.x;
        if (r >= n) break;
        const long long y = label[r];
        if (!lv_used(y, ignore_index, has_ignore)) continue;
        if (y >= 0 && y < c) { ++used; atomicAdd(&s_hist[y], 1); }
        else ++bad;
    }
    int total;
    lv_block_excl(used, s_wave, &total);
    const int bad_total = (int)gva::wave_sum((float)bad);  // (exact: at most 64 * 4)
    if ((threadIdx.x & 63) == 0 && bad_total > 0) atomicAdd(meta + M_BAD, bad_total);
    if (threadIdx.x == 0) blkcnt[blockIdx.x] = total;
    __syncthreads();
    for (int j = threadIdx.x; j < c; j += LV_TPB)
        if (s_hist[j]) atomicAdd(cls_cnt + j, s_hist[j]);
}

// one workgroup of LV_SCAN_TPB threads
__global__ __launch_bounds__(LV_SCAN_TPB) void lv_plan_kernel(int nblk, int c, const int *__restrict__ seen,
                                                              int *__restrict__ meta, const int *__restrict__ cls_cnt,
                                                              int *__restrict__ slot_of, int *__restrict__ cls_of_slot,
                                                              int *__restrict__ blkcnt) {
    __shared__ int s_wave[LV_SCAN_TPB / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    auto scan = [&](int v, int *total) {  // workgroup exclusive scan
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        __syncthreads();
        if (lane == 63) s_wave[wid] = incl;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < LV_SCAN_TPB / 64; ++w) {
            const int s = s_wave[w];
            before += w < wid ? s : 0;
            all += s;
        }
        *total = all;
        return before + incl - v;
    };
    int carry = 0, total;
    for (int b0 = 0; b0 < nblk; b0 += LV_SCAN_TPB) {
        const int b = b0 + threadIdx.x;
        const int v = b < nblk ? blkcnt[b] : 0;
        const int ex = scan(v, &total);
        if (b < nblk) blkcnt[b] = carry + ex;
        carry += total;
    }
    // c <= LV_MAX_C == LV_SCAN_TPB: one tile
    const int j = threadIdx.x;
    const bool present = j < c && cls_cnt[j] > 0 && (!seen || seen[j] != 0);
    const int slot = scan(present ? 1 : 0, &total);
    if (j < c) slot_of[j] = present ? slot : -1;
    if (present) cls_of_slot[slot] = j;
    if (threadIdx.x == 0) {
        meta[M_NSEG] = total;
        meta[M_NLAB] = carry;
    }
}

__global__ __launch_bounds__(LV_TPB) void lv_rows_kernel(int n, int c, const float *__restrict__ logits,
                                                         const long long *__restrict__ label, int ignore_index, int has_ignore,
                                                         const int *__restrict__ meta, const int *__restrict__ cls_of_slot,
                                                         const int *__restrict__ blkoff, int *__restrict__ rank_of,
                                                         float2 *__restrict__ rowstat, unsigned *__restrict__ keys,
                                                         unsigned *__restrict__ vals) {
    __shared__ int s_cls[LV_MAX_C];
    __shared__ int s_wave[LV_TPB / 64];
    const int nseg = meta[M_NSEG], nlab = meta[M_NLAB];
    for (int s = threadIdx.x; s < nseg; s += LV_TPB) s_cls[s] = cls_of_slot[s];
    int base = blkoff[blockIdx.x];
    for (int i = 0; i < LV_ROWS / LV_TPB; ++i) {
        const long long r = (long long)blockIdx.x * LV_ROWS + i * LV_TPB + threadIdx.x;
        long long y = -1;
        bool on = false;
        if (r < n) {
            y = label[r];
            on = lv_used(y, ignore_index, has_ignore) && y >= 0 && y < c;
        }
        int total;
        const int rank = base + lv_block_excl(on ? 1 : 0, s_wave, &total);  // (its barriers also publish s_cls)
        base += total;
        if (r < n) rank_of[r] = on ? rank : -1;
        if (!on) continue;
        const float *row = logits + r * c;
        float mx = row[0];
        for (int j = 1; j < c; ++j) mx = fmaxf(mx, row[j]);
        float se = 0.f;
        for (int j = 0; j < c; ++j) se += expf(row[j] - mx);
        rowstat[r] = make_float2(mx, se);
        for (int s = 0; s < nseg; ++s) {
            const int cls = s_cls[s];
            const float p = expf(row[cls] - mx) / se;
            const unsigned fg = cls == (int)y ? 1u : 0u;
            const float e = fabsf((float)fg - p);
            const size_t at = (size_t)s * nlab + rank;
            keys[at] = LV_ONE - __float_as_uint(e);
            vals[at] = (unsigned)rank | (fg << 31);
        }
    }
}

// digit counts of one chunk: cnt[(seg * 256 + digit) * cps + chunk]
__global__ __launch_bounds__(LV_TPB) void lv_hist_kernel(const int *__restrict__ meta, int cps, int shift,
                                                         const unsigned *__restrict__ keys, int *__restrict__ cnt) {
    __shared__ int s_hist[256];
    const int seg = blockIdx.y, ch = blockIdx.x, nseg = meta[M_NSEG], nlab = meta[M_NLAB];
    if (seg >= nseg || ch * LV_CHUNK >= nlab) return;
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned *k = keys + (size_t)seg * nlab;
    const int e1 = min(nlab, (ch + 1) * LV_CHUNK);
    for (int e = ch * LV_CHUNK + threadIdx.x; e < e1; e += LV_TPB) atomicAdd(&s_hist[(k[e] >> shift) & 255], 1);
    __syncthreads();
    cnt[((size_t)seg * 256 + threadIdx.x) * cps + ch] = s_hist[threadIdx.x];
}

// per segment, in place: exclusive scan of the counts in (digit, chunk) order over the chunks that exist
__global__ __launch_bounds__(LV_SCAN_TPB) void lv_scan_kernel(const int *__restrict__ meta, int cps, int *__restrict__ cnt) {
    __shared__ int s_wave[LV_SCAN_TPB / 64];
    const int seg = blockIdx.x, nseg = meta[M_NSEG], nlab = meta[M_NLAB];
    if (seg >= nseg || nlab == 0) return;
    const int nch = (nlab + LV_CHUNK - 1) / LV_CHUNK, total_e = 256 * nch;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int *base = cnt + (size_t)seg * 256 * cps;
    int carry = 0;
    for (int e0 = 0; e0 < total_e; e0 += 4 * LV_SCAN_TPB) {
        int v[4], at[4], tsum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + threadIdx.x * 4 + u;
            at[u] = e < total_e ? (e / nch) * cps + e % nch : -1;
            v[u] = at[u] >= 0 ? base[at[u]] : 0;
            tsum += v[u];
        }
        int incl = tsum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        __syncthreads();
        if (lane == 63) s_wave[wid] = incl;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < LV_SCAN_TPB / 64; ++w) {
            const int s = s_wave[w];
            before += w < wid ? s : 0;
            all += s;
        }
        int run = carry + before + incl - tsum;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (at[u] >= 0) base[at[u]] = run;
            run += v[u];
        }
        carry += all;
    }
}

// stable scatter of one chunk by the digit at `shift`: rounds of 256 elements in order; inside a round, a wave ranks its
// lanes by ballots, the waves' counts per digit are combined in wave order through LDS
__global__ __launch_bounds__(LV_TPB) void lv_scatter_kernel(const int *__restrict__ meta, int cps, int shift,
                                                            const unsigned *__restrict__ kin, const unsigned *__restrict__ vin,
                                                            unsigned *__restrict__ kout, unsigned *__restrict__ vout,
                                                            const int *__restrict__ cnt) {
    __shared__ int s_run[256];
    __shared__ int s_wcnt[LV_TPB / 64][256];
    const int seg = blockIdx.y, ch = blockIdx.x, nseg = meta[M_NSEG], nlab = meta[M_NLAB];
    if (seg >= nseg || ch * LV_CHUNK >= nlab) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    s_run[tid] = cnt[((size_t)seg * 256 + tid) * cps + ch];
#pragma unroll
    for (int w = 0; w < LV_TPB / 64; ++w) s_wcnt[w][tid] = 0;
    const size_t sbase = (size_t)seg * nlab;
    const int e1 = min(nlab, (ch + 1) * LV_CHUNK);
    const unsigned long long below = (1ull << lane) - 1ull;
    __syncthreads();
    for (int e0 = ch * LV_CHUNK; e0 < e1; e0 += LV_TPB) {
        const int e = e0 + tid;
        const bool ok = e < e1;
        unsigned key = 0, val = 0;
        if (ok) { key = kin[sbase + e]; val = vin[sbase + e]; }
        const unsigned d = (key >> shift) & 255u;
        unsigned long long m = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bb = __ballot((d >> b) & 1u);
            m &= ((d >> b) & 1u) ? bb : ~bb;
        }
        const int rank = __popcll(m & below);
        if (ok && rank == 0) s_wcnt[wid][d] = __popcll(m);
        __syncthreads();
        if (ok) {
            int pos = s_run[d] + rank;
            for (int w = 0; w < wid; ++w) pos += s_wcnt[w][d];
            kout[sbase + pos] = key;
            vout[sbase + pos] = val;
        }
        __syncthreads();
        int add = 0;
#pragma unroll
        for (int w = 0; w < LV_TPB / 64; ++w) { add += s_wcnt[w][tid]; s_wcnt[w][tid] = 0; }
        s_run[tid] += add;
        __syncthreads();
    }
}

__global__ __launch_bounds__(LV_TPB) void lv_fgcount_kernel(const int *__restrict__ meta, int cps,
                                                            const unsigned *__restrict__ vals, int *__restrict__ chunkfg) {
    __shared__ int s_wave[LV_TPB / 64];
    const int seg = blockIdx.y, ch = blockIdx.x, nseg = meta[M_NSEG], nlab = meta[M_NLAB];
    if (seg >= nseg || ch * LV_CHUNK >= nlab) return;
    const unsigned *v = vals + (size_t)seg * nlab;
    const int e1 = min(nlab, (ch + 1) * LV_CHUNK);
    int f = 0;
    for (int e = ch * LV_CHUNK + threadIdx.x; e < e1; e += LV_TPB) f += (int)(v[e] >> 31);
    int total;
    lv_block_excl(f, s_wave, &total);
    if (threadIdx.x == 0) chunkfg[(size_t)seg * cps + ch] = total;
}

__global__ __launch_bounds__(LV_TPB) void lv_final_kernel(const int *__restrict__ meta, int cps,
                                                          const int *__restrict__ cls_cnt, const int *__restrict__ cls_of_slot,
                                                          const unsigned *__restrict__ keys, const unsigned *__restrict__ vals,
                                                          const int *__restrict__ chunkfg, double *part, unsigned *counter,
                                                          float weight, float *__restrict__ gs, float *__restrict__ out) {
    __shared__ int s_wave[LV_TPB / 64];
    __shared__ double s_acc[LV_TPB];
    const int seg = blockIdx.y, ch = blockIdx.x, nseg = meta[M_NSEG], nlab = meta[M_NLAB];
    const int tid = threadIdx.x;
    if (seg < nseg && ch * LV_CHUNK < nlab) {
        int before = 0;  // fg of the segment's earlier chunks
        for (int k = tid; k < ch; k += LV_TPB) before += chunkfg[(size_t)seg * cps + k];
        int fg_chunk0;
        lv_block_excl(before, s_wave, &fg_chunk0);
        const float gts = (float)cls_cnt[cls_of_slot[seg]];
        const size_t sbase = (size_t)seg * nlab;
        const int k0 = ch * LV_CHUNK + tid * LV_PER;
        unsigned v[LV_PER];
        int mine = 0;
#pragma unroll
        for (int u = 0; u < LV_PER; ++u) {
            v[u] = k0 + u < nlab ? vals[sbase + k0 + u] : 0u;
            mine += (int)(v[u] >> 31);
        }
        int tot;
        int cum = fg_chunk0 + lv_block_excl(mine, s_wave, &tot);  // fg before element k0 (exclusive)
        double dot = 0.0;
#pragma unroll
        for (int u = 0; u < LV_PER; ++u) {
            const int k = k0 + u;
            if (k >= nlab) break;
            const unsigned fg = v[u] >> 31;
            const float e = __uint_as_float(LV_ONE - keys[sbase + k]);
            cum += (int)fg;  // inclusive cumsum of fg at k
            // _lovasz_grad in fp32 (lovasz.py:22-33): intersection = gts - cumsum(fg), union = gts + cumsum(1 - fg)
            const float inter = gts - (float)cum, uni = gts + (float)(k + 1 - cum);
            float g = 1.0f - inter / uni;
            if (k > 0) {
                const int cp = cum - (int)fg;
                const float ip = gts - (float)cp, up = gts + (float)(k - cp);
                g = g - (1.0f - ip / up);
            }
            dot += (double)e * (double)g;
            const float sg = e > 0.f ? (fg ? 1.f : -1.f) : 0.f;  // sign(fg - p)
            gs[sbase + (v[u] & 0x7fffffffu)] = -sg * g;
        }
        s_acc[tid] = dot;
        __syncthreads();
        for (int s = LV_TPB / 2; s > 0; s >>= 1) {
            if (tid < s) s_acc[tid] += s_acc[tid + s];
            __syncthreads();
        }
        if (tid == 0) __hip_atomic_store(part + (size_t)seg * cps + ch, s_acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (gva::last_block_arrives(counter)) {
        const int nch = (nlab + LV_CHUNK - 1) / LV_CHUNK, total_e = nseg * nch;
        double a = 0.0;
        for (int i = tid; i < total_e; i += LV_TPB) a += part[(size_t)(i / nch) * cps + i % nch];
        __syncthreads();
        s_acc[tid] = a;
        __syncthreads();
        for (int s = LV_TPB / 2; s > 0; s >>= 1) {
            if (tid < s) s_acc[tid] += s_acc[tid + s];
            __syncthreads();
        }
        if (tid == 0) {
            const int bad = meta[M_BAD];
            const float mean = nseg > 0 ? (float)(s_acc[0] / (double)nseg) : 0.f;
            out[0] = bad > 0 ? __builtin_nanf("") : mean * weight;
            out[1] = (float)nseg;
            out[2] = (float)bad;
            out[3] = (float)nlab;
        }
    }
}

__global__ __launch_bounds__(LV_TPB) void lv_backward_kernel(int n, int c, const float *__restrict__ logits,
                                                             const int *__restrict__ meta, const int *__restrict__ slot_of,
                                                             const int *__restrict__ rank_of, const float2 *__restrict__ rowstat,
                                                             const float *__restrict__ gs, float weight,
                                                             const float *__restrict__ g_loss, float *__restrict__ g_logits) {
    __shared__ int s_slot[LV_MAX_C];
    for (int j = threadIdx.x; j < c; j += LV_TPB) s_slot[j] = slot_of[j];
    __syncthreads();
    const int nseg = meta[M_NSEG], nlab = meta[M_NLAB];
    const float scale = nseg > 0 ? *g_loss * weight / (float)nseg : 0.f;
    for (long long r = (long long)blockIdx.x * LV_TPB + threadIdx.x; r < n; r += (long long)gridDim.x * LV_TPB) {
        float *o = g_logits + r * c;
        const int rank = rank_of[r];
        if (rank < 0) {
            for (int j = 0; j < c; ++j) o[j] = 0.f;
            continue;
        }
        const float *row = logits + r * c;
        const float2 st = rowstat[r];
        float dot = 0.f;
        for (int j = 0; j < c; ++j) {
            const int s = s_slot[j];
            if (s >= 0) dot += gs[(size_t)s * nlab + rank] * (expf(row[j] - st.x) / st.y);
        }
        for (int j = 0; j < c; ++j) {
            const int s = s_slot[j];
            const float gp = s >= 0 ? gs[(size_t)s * nlab + rank] : 0.f;
            const float p = expf(row[j] - st.x) / st.y;
            o[j] = p * (gp - dot) * scale;
        }
    }
}

}  // namespace

extern "C" size_t lovasz_softmax_workspace_bytes(int n, int c) {
    if (n < 1 || c < 1) return 0;
    return WsLayout(n, c).total;
}

extern "C" size_t lovasz_softmax_saved_bytes(int n, int c) {
    if (n < 1 || c < 1) return 0;
    return SavedLayout(n, c).total;
}

extern "C" int lovasz_softmax_forward_hip_launcher(int n, int c, const float *logits, const long long *label, int ignore_index,
                                                   int has_ignore, const int *class_seen, float weight, float *out, void *saved,
                                                   size_t saved_bytes, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 1 || n >= (1 << 24) || c < 2 || c > LV_MAX_C || !logits || !label || !out || !saved) return PTV2_ERR_ARG;
    if (!workspace || workspace_bytes < lovasz_softmax_workspace_bytes(n, c) || saved_bytes < lovasz_softmax_saved_bytes(n, c))
        return PTV2_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned *counters = ptv2_stream_counters(st);
    if (!counters) return PTV2_ERR_LAUNCH;
    const SavedLayout S(n, c);
    const WsLayout W(n, c);
    char *sv = (char *)saved, *ws = (char *)workspace;
    int *meta = (int *)(sv + S.meta), *cls_cnt = (int *)(sv + S.cls_cnt), *slot_of = (int *)(sv + S.slot_of);
    int *cls_of_slot = (int *)(sv + S.cls_of_slot), *rank_of = (int *)(sv + S.rank_of);
    float2 *rowstat = (float2 *)(sv + S.rowstat);
    float *gs = (float *)(sv + S.gs);
    int *blkcnt = (int *)(ws + W.blkcnt), *cnt = (int *)(ws + W.cnt), *chunkfg = (int *)(ws + W.chunkfg);
    unsigned *k0 = (unsigned *)(ws + W.keys0), *v0 = (unsigned *)(ws + W.vals0);
    unsigned *k1 = (unsigned *)(ws + W.keys1), *v1 = (unsigned *)(ws + W.vals1);
    double *part = (double *)(ws + W.part);
    const int nblk = (n + LV_ROWS - 1) / LV_ROWS, segs = std::min(n, c), cps = W.cps;

    if (hipMemsetAsync(meta, 0, S.slot_of - S.meta, st) != hipSuccess) return PTV2_ERR_LAUNCH;
    hipLaunchKernelGGL(lv_count_kernel, dim3(nblk), dim3(LV_TPB), 0, st, n, c, label, ignore_index, has_ignore, meta, cls_cnt,
                       blkcnt);
    PTV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(lv_plan_kernel, dim3(1), dim3(LV_SCAN_TPB), 0, st, nblk, c, class_seen, meta, cls_cnt, slot_of,
                       cls_of_slot, blkcnt);
    PTV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(lv_rows_kernel, dim3(nblk), dim3(LV_TPB), 0, st, n, c, logits, label, ignore_index, has_ignore, meta,
                       cls_of_slot, blkcnt, rank_of, rowstat, k0, v0);
    PTV2_CHECK_LAUNCH();
    const dim3 grid(cps, segs);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 8 * pass;
        hipLaunchKernelGGL(lv_hist_kernel, grid, dim3(LV_TPB), 0, st, meta, cps, shift, k0, cnt);
        PTV2_CHECK_LAUNCH();
        hipLaunchKernelGGL(lv_scan_kernel, dim3(segs), dim3(LV_SCAN_TPB), 0, st, meta, cps, cnt);
        PTV2_CHECK_LAUNCH();
        hipLaunchKernelGGL(lv_scatter_kernel, grid, dim3(LV_TPB), 0, st, meta, cps, shift, k0, v0, k1, v1, cnt);
        PTV2_CHECK_LAUNCH();
        std::swap(k0, k1);
        std::swap(v0, v1);
    }
    hipLaunchKernelGGL(lv_fgcount_kernel, grid, dim3(LV_TPB), 0, st, meta, cps, v0, chunkfg);
    PTV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(lv_final_kernel, grid, dim3(LV_TPB), 0, st, meta, cps, cls_cnt, cls_of_slot, k0, v0, chunkfg, part,
                       counters + CNT_LOVASZ, weight, gs, out);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}

extern "C" int lovasz_softmax_backward_hip_launcher(int n, int c, const float *logits, const void *saved, float weight,
                                                    const float *g_loss, float *g_logits, void *stream) {
    if (n < 1 || n >= (1 << 24) || c < 2 || c > LV_MAX_C || !logits || !saved || !g_loss || !g_logits) return PTV2_ERR_ARG;
    const SavedLayout S(n, c);
    const char *sv = (const char *)saved;
    const int nblk = (int)std::min<long long>(((long long)n + LV_TPB - 1) / LV_TPB, 4096);
    hipLaunchKernelGGL(lv_backward_kernel, dim3(nblk), dim3(LV_TPB), 0, (hipStream_t)stream, n, c, logits,
                       (const int *)(sv + S.meta), (const int *)(sv + S.slot_of), (const int *)(sv + S.rank_of),
                       (const float2 *)(sv + S.rowstat), (const float *)(sv + S.gs), weight, g_loss, g_logits);
    PTV2_CHECK_LAUNCH();
    return PTV2_OK;
}
