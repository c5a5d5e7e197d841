// Device helpers shared by decode.hip and ctc_grad.hip: the sortable float key, the in-LDS bitonic sort, the
// per-query sigmoid sum and the CTC alpha recursion's frame (one code path, so the CTC forward and backward see bit-identical sums,
// reading orders and alphas).
#pragma once
#include "gfx950_prims.h"      // dpp_f / dpp_i

namespace dtlr {

// monotone map float -> uint32 (ascending)
__device__ __forceinline__ uint32_t f32_sortable(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// in-LDS bitonic sort of n = power of two 64-bit keys, ascending.  A thread owns compare-exchange PAIRS (pair t of stage j is
// i = the index with bit j cleared, i | j), four at a time, and reads all eight keys before it writes any: one LDS round trip
// per stage instead of one per element (the element-wise form serialised 8 dependent read->write trips per stage at n = 8192
// and made the two selection kernels ~100 us each).
__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* keys, int n) {
    const int half = n >> 1;
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t0 = threadIdx.x; t0 < half; t0 += 4 * blockDim.x) {
                unsigned long long a[4], b[4];
                int ia[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = t0 + u * blockDim.x;
                    ia[u] = t < half ? (((t & ~(j - 1)) << 1) | (t & (j - 1))) : -1;
                    if (ia[u] >= 0) { a[u] = keys[ia[u]]; b[u] = keys[ia[u] | j]; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (ia[u] < 0) continue;
                    const bool up = (ia[u] & k) == 0;
                    if ((a[u] > b[u]) == up) { keys[ia[u]] = b[u]; keys[ia[u] | j] = a[u]; }
                }
            }
        }
    }
    __syncthreads();
}

// sum over classes of sigmoid(logit) for every query: 16 lanes per query, 256 threads = 16 queries per workgroup (DPP reductions)
__device__ __forceinline__ void query_sum_rows(const float* __restrict__ logits, float* __restrict__ sums, long nrows, int C)
{
    const int l16 = threadIdx.x & 15;
    const long q = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = q < nrows;
    const float* lr = logits + (live ? q : 0) * C;
    float sum = 0.f;
    for (int c0 = 0; c0 < C; c0 += 64) {
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int c = c0 + 16 * u + l16; x[u] = (live && c < C) ? lr[c] : -INFINITY; }
#pragma unroll
        for (int u = 0; u < 4; ++u) sum += 1.f / (1.f + expf(-x[u]));
    }
    sum += dpp_f<0xB1, true>(sum); sum += dpp_f<0x4E, true>(sum); sum += dpp_f<0x141, true>(sum); sum += dpp_f<0x140, true>(sum);
    if (live && l16 == 0) sums[q] = sum;
}

// ---- the CTC alpha recursion of SetCriterion.loss_CTC, one thread per state s of the blank-extended label sequence.  The forward
// (decode.hip) and the backward (ctc_grad.hip) both call these three, so the per-line NLL of the two is the same float sequence by
// construction.

// log of the blank-augmented probability of this state's channel (lab = 0: the blank) at a query with logit x and class sum `sum`
__device__ __forceinline__ float ctc_log_prob(int lab, float x, float sum, float thr, float one_m_eps, float eps)
{
    float p;
    if (sum < thr) p = lab == 0 ? 1.f - sum : 1.f / (1.f + expf(-x));
    else p = lab == 0 ? eps : one_m_eps * (1.f / (1.f + expf(-x))) / sum;
    return logf(p);
}

// one frame: cur[s] = lse(prev[s], prev[s-1], skip ? prev[s-2]) + lp with torch's CTCLoss update (max shift, -inf handling); prev
// carries two -inf guard slots in front.  Ends with the workgroup barrier; returns the new alpha (-inf for a dead thread).
__device__ __forceinline__ float ctc_alpha_step(const float* prev, float* cur, int s, bool live, bool skip, float lp)
{
    float v = -INFINITY;
    if (live) {
        const float la1 = prev[s], la2 = prev[s - 1], la3 = skip ? prev[s - 2] : -INFINITY;
        float m = fmaxf(la1, fmaxf(la2, la3));
        if (m == -INFINITY) m = 0.f;
        v = logf(expf(la1 - m) + expf(la2 - m) + expf(la3 - m)) + m + lp;
        cur[s] = v;
    }
    __syncthreads();
    return v;
}

// -log P of a line from the alphas after the last frame (S = 2 L + 1 states)
__device__ __forceinline__ float ctc_final_nll(const float* a, int S, int L)
{
    const float l1 = a[S - 1], l2 = L > 0 ? a[S - 2] : -INFINITY;
    float m = fmaxf(l1, l2);
    if (m == -INFINITY) m = 0.f;
    return -(logf(expf(l1 - m) + expf(l2 - m)) + m);
}

}  // namespace dtlr
