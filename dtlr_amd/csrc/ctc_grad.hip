// Gradient of the CTC loss of SetCriterion.loss_CTC (models/dino/dino.py:457-551) with respect to the class logits: what the class
// head needs to be adapted to a new charset on the device (dtlr_amd/adapt.py).
//   dtlr_ctc_loss_interleaved_backward   per-line NLL (bit-identical to dtlr_ctc_loss_interleaved: both call decode_common.h's
//                                        ctc_log_prob / ctc_alpha_step / ctc_final_nll in the same order) and
//                                        dlogits [B, nq, C] of  mean_b( nll_b / max(L_b, 1) ), zero_infinity
// Where the two differ, on inputs the forward leaves undefined: a target length outside 0..max_target_length is clamped here; a NaN
// NLL (NaN logits) and a line holding a label outside 1..C give loss 0 and an all-zero gradient here, like an infeasible line.
// Three launches:
//   1. query sums, chip-wide (decode_common.h: the forward's own code);
//   2. one workgroup per line, one thread per state of the blank-extended label sequence: reading-order sort, the forward's alpha
//      recursion with the alphas of the even frames (t = 2 r = the query of rank r) stored to the caller's workspace, then the beta
//      recursion backwards over the same 2 nq frames (filler frames are constants but take part), turning every stored alpha into
//      the posterior occupancy of its state   occ_r(s) = alpha_r(s) beta_r(s) / (y_r(s) P);
//   3. one workgroup per (line, rank), chip-wide: merges the occupancies per channel -- omega(0) = sum over the blank states, omega(c) =
//      sum over the states of label c, a repeated label's states chained in sequence order -- and writes the row
//          s < 1 - eps :  d nll / d x_c = (1 - p_c) (p_c omega(0) / (1 - s) - omega(c))
//          else        :  d nll / d x_c = (1 - p_c) (p_c sum_c' omega(c') / s  - omega(c))          p = sigmoid(x), s = sum_c p_c
//      scaled by 1 / (B max(L_b, 1)).  Every sum runs in a fixed order: two runs give the same bits.
#include "dtlr_common.h"
#include "decode_common.h"

namespace dtlr {

constexpr int CTCB_PF = 8;

__global__ __launch_bounds__(256) void ctcb_query_sum_kernel(const float* __restrict__ logits, float* __restrict__ sums, long nrows, int C)
{
    query_sum_rows(logits, sums, nrows, C);
}

// workspace of one call, in 4-byte words: sums [B nq] | order [B nq] int | lscale [B] | chain [B][2 Lc] int (next, first) | occ [B nq SW]
struct CtcbWs { float* sums; int* order; float* lscale; int* chain; float* occ; };
static inline CtcbWs ctcb_ws(float* ws, long B, long nq, long Lc)
{
    CtcbWs w;
    w.sums = ws;
    w.order = reinterpret_cast<int*>(ws + B * nq);
    w.lscale = ws + 2 * B * nq;
    w.chain = reinterpret_cast<int*>(ws + 2 * B * nq + B);
    w.occ = ws + 2 * B * nq + B + 2 * B * Lc;
    return w;
}

__global__ __launch_bounds__(1024) void ctc_interleaved_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                                   const float* __restrict__ sums, const int* __restrict__ targets,
                                                                   const int* __restrict__ target_lengths, float* __restrict__ nll,
                                                                   int* __restrict__ order, float* __restrict__ lscale,
                                                                   int* __restrict__ chain, float* __restrict__ occ,
                                                                   int B, int nq, int C, int Lmax, int Lcap, int Lc, int SW,
                                                                   float eps, float filler, int npow2)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];      // [npow2] | float ssum[npow2] | float alpha[2][blockDim + 2]
    float* ssum = reinterpret_cast<float*>(keys + npow2);
    float* alpha = ssum + npow2;
    __shared__ float s_nll;
    const int b = blockIdx.x, s = threadIdx.x, AP = blockDim.x + 2;
    const int L = min(max(target_lengths[b], 0), Lcap), S = 2 * L + 1;       // Lcap = the host's max_target_length: S <= blockDim, S <= SW
    for (int i = threadIdx.x; i < npow2; i += blockDim.x)
        keys[i] = i < nq ? (((unsigned long long)f32_sortable(boxes[((long)b * nq + i) * 4])) << 32) | (unsigned)i : ~0ull;
    bitonic_sort_u64(keys, npow2);                                             // ascending cx, ties: lower index first
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        const int q = (int)(keys[i] & 0xffffffffull);
        ssum[i] = sums[(long)b * nq + q];
        order[(long)b * nq + i] = q;
    }
    const bool live = s < S;
    const int lab = (live && (s & 1)) ? targets[(long)b * Lmax + (s >> 1)] : 0;
    const bool skip = live && (s & 1) && s >= 3 && lab != targets[(long)b * Lmax + (s >> 1) - 1];
    // the beta recursion's skip s -> s + 2: state s + 2 is a label state whose label differs from this one's
    const bool skipn = live && (s & 1) && s + 2 < S && lab != targets[(long)b * Lmax + (s >> 1) + 1];
    if (live && (s & 1)) {                                                      // the chain of a repeated label's states, in sequence order
        const int j = s >> 1;
        int nxt = -1, first = 1;
        for (int k = j + 1; k < L; ++k) if (targets[(long)b * Lmax + k] == lab) { nxt = k; break; }
        for (int k = 0; k < j; ++k) if (targets[(long)b * Lmax + k] == lab) { first = 0; break; }
        chain[((long)b * Lc + j) * 2] = nxt;
        chain[((long)b * Lc + j) * 2 + 1] = first;
    }
    const float one_m_eps = (float)(1.0 - (double)eps), thr = one_m_eps;
    const float lfill = lab == 0 ? 0.f : logf(filler);
    const float* lrow = logits + (long)b * nq * C + (lab > 0 ? lab - 1 : 0);
    float* orow = occ + (long)b * nq * SW + s;
    // a label outside 1..C would address another query's logits: the line is dropped like an infeasible one (block-uniform)
    if (__syncthreads_or(live && (s & 1) && (lab < 1 || lab > C))) {
        if (threadIdx.x == 0) { nll[b] = 0.f; lscale[b] = 0.f; }
        return;
    }
    float* a0 = alpha + 2;
    float* a1 = alpha + AP + 2;
    if (threadIdx.x < 2) { alpha[threadIdx.x] = -INFINITY; alpha[AP + threadIdx.x] = -INFINITY; }

    float pf[CTCB_PF];
#pragma unroll
    for (int u = 0; u < CTCB_PF; ++u) pf[u] = (lab > 0 && u < nq) ? lrow[(long)(int)(keys[u] & 0xffffffffull) * C] : 0.f;

    auto logp = [&](float x, float sum) -> float { return ctc_log_prob(lab, x, sum, thr, one_m_eps, eps); };
    auto step = [&](const float* prev, float* cur, float lp) -> float { return ctc_alpha_step(prev, cur, s, live, skip, lp); };
    // ---- forward: dtlr_ctc_loss_interleaved's recursion (decode.hip: the same decode_common.h calls), plus one store per even frame
    for (int i0 = 0; i0 < nq; i0 += CTCB_PF) {
        float nx[CTCB_PF];
#pragma unroll
        for (int u = 0; u < CTCB_PF; ++u) {
            const int i = i0 + CTCB_PF + u;
            nx[u] = (lab > 0 && i < nq) ? lrow[(long)(int)(keys[i] & 0xffffffffull) * C] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CTCB_PF; ++u) {
            const int i = i0 + u;
            if (i < nq) {                                                       // block-uniform
                const float lp = logp(pf[u], ssum[i]);
                float v;
                if (i == 0) {                                                   // t = 0: only states 0 and 1 are reachable
                    v = s < 2 ? lp : -INFINITY;
                    if (live) a0[s] = v;
                    __syncthreads();
                } else v = step(a1, a0, lp);                                    // t = 2 i   : a1 -> a0
                if (live) orow[(long)i * SW] = v;
                step(a0, a1, lfill);                                            // t = 2 i + 1: a0 -> a1
            }
        }
#pragma unroll
        for (int u = 0; u < CTCB_PF; ++u) pf[u] = nx[u];
    }
    if (threadIdx.x == 0) {                                                     // after t = T - 1 the alphas are in a1
        const float v = ctc_final_nll(a1, S, L);
        const bool inf = isinf(v) || isnan(v);
        nll[b] = inf ? 0.f : v;                                                 // zero_infinity=True
        lscale[b] = inf ? 0.f : 1.f / ((float)B * (float)(L > 1 ? L : 1));       // 0: the line contributes no gradient
        s_nll = inf ? INFINITY : v;
    }
    __syncthreads();
    const float lnll = s_nll;
    if (lnll == INFINITY) return;                                               // block-uniform
    // ---- backward: beta_t(s) = lse(beta_{t+1}(s), beta_{t+1}(s+1), skip ? beta_{t+1}(s+2)) + log y_t(s); the buffers get -inf
    // everywhere first, so the two slots past the last state (and every dead thread's slot) read as -inf
    for (int i = threadIdx.x; i < 2 * AP; i += blockDim.x) alpha[i] = -INFINITY;
    float* b0 = alpha;                                                          // even frames
    float* b1 = alpha + AP;                                                     // odd (filler) frames
    __syncthreads();
    auto bstep = [&](const float* nxt, float* cur, float lp) -> float {
        float v = -INFINITY;
        if (live) {
            const float lb1 = nxt[s], lb2 = nxt[s + 1], lb3 = skipn ? nxt[s + 2] : -INFINITY;
            float m = fmaxf(lb1, fmaxf(lb2, lb3));
            if (m == -INFINITY) m = 0.f;
            v = logf(expf(lb1 - m) + expf(lb2 - m) + expf(lb3 - m)) + m + lp;
            cur[s] = v;
        }
        __syncthreads();
        return v;
    };
    const int top = ((nq - 1) / CTCB_PF) * CTCB_PF;
    float al[CTCB_PF];
#pragma unroll
    for (int u = 0; u < CTCB_PF; ++u) {
        const int i = top + u;
        pf[u] = (lab > 0 && i < nq) ? lrow[(long)(int)(keys[i] & 0xffffffffull) * C] : 0.f;
        al[u] = (live && i < nq) ? orow[(long)i * SW] : 0.f;
    }
    for (int i0 = top; i0 >= 0; i0 -= CTCB_PF) {
        float nx[CTCB_PF], na[CTCB_PF];
#pragma unroll
        for (int u = 0; u < CTCB_PF; ++u) {
            const int i = i0 - CTCB_PF + u;
            nx[u] = (lab > 0 && i >= 0) ? lrow[(long)(int)(keys[i] & 0xffffffffull) * C] : 0.f;
            na[u] = (live && i >= 0) ? orow[(long)i * SW] : 0.f;
        }
#pragma unroll
        for (int u = CTCB_PF - 1; u >= 0; --u) {
            const int i = i0 + u;
            if (i < nq) {                                                       // block-uniform
                if (i == nq - 1) {                                              // t = T - 1: only the last two states may end the path
                    if (live) b1[s] = (s == S - 1 || s == S - 2) ? lfill : -INFINITY;
                    __syncthreads();
                } else bstep(b0, b1, lfill);                                    // t = 2 i + 1: b0 -> b1
                const float lp = logp(pf[u], ssum[i]);
                const float lb = bstep(b1, b0, lp);                             // t = 2 i    : b1 -> b0
                if (live) {
                    const float e = al[u] + lb - lp + lnll;                     // log of alpha beta / (y P)
                    orow[(long)i * SW] = (al[u] == -INFINITY || lb == -INFINITY) ? 0.f : expf(e);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < CTCB_PF; ++u) { pf[u] = nx[u]; al[u] = na[u]; }
    }
}

// one workgroup per (line, rank): the row of dlogits of the query at that rank
__global__ __launch_bounds__(256) void ctc_dlogits_kernel(const float* __restrict__ logits, const float* __restrict__ sums,
                                                          const int* __restrict__ order, const float* __restrict__ lscale,
                                                          const int* __restrict__ chain, const float* __restrict__ occ,
                                                          const int* __restrict__ targets, const int* __restrict__ target_lengths,
                                                          float* __restrict__ dlogits, int nq, int C, int Lmax, int Lcap, int Lc, int SW, float eps)
{
    extern __shared__ __attribute__((aligned(16))) float wl[];                  // [C]: omega(c) of this row
    __shared__ float red[2][4];
    const long row = blockIdx.x;
    const int b = (int)(row / nq);
    const int q = order[row];
    const float scale = lscale[b];
    float* out = dlogits + ((long)b * nq + q) * C;
    if (scale == 0.f) {                                                         // infeasible line (zero_infinity): exactly 0
        for (int c = threadIdx.x; c < C; c += blockDim.x) out[c] = 0.f;
        return;
    }
    const int L = min(max(target_lengths[b], 0), Lcap);
    const float* orow = occ + row * SW;
    for (int c = threadIdx.x; c < C; c += blockDim.x) wl[c] = 0.f;
    float w0 = 0.f, wc = 0.f;                                                   // blank states 0, 2, .., 2 L ; label states
    for (int j = threadIdx.x; j <= L; j += blockDim.x) w0 += orow[2 * j];
    for (int j = threadIdx.x; j < L; j += blockDim.x) wc += orow[2 * j + 1];
    w0 = wave_sum(w0);
    wc = wave_sum(wc);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = w0; red[1][threadIdx.x >> 6] = wc; }
    __syncthreads();
    w0 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    wc = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        const int* ch = chain + ((long)b * Lc + j) * 2;
        if (ch[1]) {                                                            // first occurrence of its label: owns the merged sum
            float a = 0.f;
            for (int k = j; k >= 0; k = chain[((long)b * Lc + k) * 2]) a += orow[2 * k + 1];
            const int t = targets[(long)b * Lmax + j];
            if (t >= 1 && t <= C) wl[t - 1] = a;
        }
    }
    __syncthreads();
    const float sum = sums[(long)b * nq + q];
    const float thr = (float)(1.0 - (double)eps);
    const float coef = sum < thr ? w0 / (1.f - sum) : wc / sum;
    const float* lr = logits + ((long)b * nq + q) * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float p = 1.f / (1.f + expf(-lr[c]));
        out[c] = scale * ((1.f - p) * (p * coef - wl[c]));
    }
}

}  // namespace dtlr

using namespace dtlr;

static inline int ctcb_next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }

extern "C" long dtlr_ctc_loss_interleaved_backward_workspace_bytes(int B, int nq, int Lmax)
{
    if (B <= 0 || nq <= 0 || Lmax < 0) return 0;
    const long Lc = Lmax > 0 ? Lmax : 1, SW = 2l * Lmax + 1;
    return 4 * (2l * B * nq + B + 2l * B * Lc + (long)B * nq * SW);
}

extern "C" int dtlr_ctc_loss_interleaved_backward(const float* logits, const float* boxes, const int* targets, const int* target_lengths,
                                                  float* nll, float* dlogits, float* workspace, int B, int nq, int C, int Lmax,
                                                  int max_target_length, float eps, float filler, void* stream)
{
    clear_stale_error();
    if (!logits || !boxes || !target_lengths || !nll || !dlogits || !workspace) return DTLR_EINVAL;
    if (B <= 0 || nq <= 0 || C <= 0 || Lmax < 0 || max_target_length < 0 || max_target_length > Lmax) return DTLR_EINVAL;
    if (Lmax > 0 && !targets) return DTLR_EINVAL;
    const int S = 2 * max_target_length + 1;
    if (S > 1024) return DTLR_ESHAPE;                          // one thread per state
    const int threads = S <= 64 ? 64 : ((S + 63) / 64) * 64;
    const int np = ctcb_next_pow2(nq);
    const size_t lds = (size_t)np * 12 + (size_t)2 * (threads + 2) * 4;
    if (lds > 150 * 1024) return DTLR_ESHAPE;
    if ((size_t)C * 4 > 60 * 1024) return DTLR_ESHAPE;         // the per-row channel table of the elementwise kernel lives in LDS
    const long nrows = (long)B * nq;
    if (nrows > 0x7fffffffl) return DTLR_ESHAPE;
    const int Lc = Lmax > 0 ? Lmax : 1, SW = 2 * Lmax + 1;
    const CtcbWs w = ctcb_ws(workspace, B, nq, Lc);
    if (int rc = launch<ctcb_query_sum_kernel>(dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, (hipStream_t)stream, logits, w.sums, nrows, C)) return rc;
    if (int rc = launch<ctc_interleaved_bwd_kernel>(dim3(B), dim3(threads), lds, (hipStream_t)stream, logits, boxes, w.sums, targets,
                                                    target_lengths, nll, w.order, w.lscale, w.chain, w.occ, B, nq, C, Lmax, max_target_length, Lc, SW, eps, filler, np)) return rc;
    return launch<ctc_dlogits_kernel>(dim3((unsigned)nrows), dim3(256), (size_t)C * 4, (hipStream_t)stream, logits, w.sums, w.order,
                                      w.lscale, w.chain, w.occ, targets, target_lengths, dlogits, nq, C, Lmax, max_target_length, Lc, SW, eps);
}
