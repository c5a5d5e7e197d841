// What the two CTC prefix beam searches share (ngram_beam.hip, word_beam.hip): fp64 log-add, the order-preserving key image, the walk
// of the packed back-off trie (dtlr_ngram_lm), and the exact radix top-K over keys in LDS.  Included inside each kernel file's own
// anonymous namespace after `using namespace dtlr;`, which declares THREADS (256) first.  `Fixed` is the file's LDS struct: the select
// uses its hist[256], s_total, s_digit, s_above and s_cnt.
#pragma once
#include "dtlr_common.h"
#include <math.h>

typedef unsigned long long u64;

#define DTLR_NEG_INF (-__builtin_huge_val())

__device__ __forceinline__ double log_add(double a, double b) {
    if (a < b) { const double t = a; a = b; b = t; }
    if (b == DTLR_NEG_INF) return a;
    return a + log1p(exp(b - a));
}

// order-preserving image of a double; 0 = "no candidate" (-inf)
__device__ __forceinline__ u64 ukey(double x) {
    if (x == DTLR_NEG_INF) return 0;
    const long long b = __double_as_longlong(x + 0.0);
    return b < 0 ? ~(u64)b : ((u64)b | 0x8000000000000000ull);
}

__device__ __forceinline__ double log_prob(float e) { return log(fmax((double)e, 1e-30)); }

// log10 P(c | state s) with back-off (ArpaLM.score), and the state after c
__device__ double lm_walk(const dtlr_ngram_lm& L, int s, int c, int* new_state) {
    double acc = 0.0;
    int ns = -1;
    const int n = L.n_nodes;
    for (int hop = 0; hop < 8; ++hop) {
        s = min(max(s, 0), n - 1);
        int lo = min(max(L.child_lo[s], 0), n), hi = min(max(L.child_hi[s], 0), n);
        int found = -1;
        for (int it = 0; it < 32 && lo < hi; ++it) {
            const int mid = (lo + hi) >> 1, tk = L.tok[mid];
            if (tk == c) { found = mid; break; }
            if (tk < c) lo = mid + 1; else hi = mid;
        }
        if (found >= 0) {
            if (ns < 0) ns = L.ctx[found];
            const double p = L.logp[found];
            if (p <= 0.0) { *new_state = ns; return acc + p; }       // logp > 0 marks a node that is only a prefix of longer n-grams
        }
        if (s == 0) break;
        acc += L.bo[s];
        s = L.suffix[s];
    }
    *new_state = ns < 0 ? 0 : ns;
    return acc + L.unk;
}

struct Sel { u64 prefix; int shift, tie, none; };

// Threshold of the `want` largest of key(0..M) (u64, 0 = absent).  Uniform result in every thread.  All threads must call.
template <class Fixed, class KeyFn>
__device__ Sel radix_select(Fixed& F, KeyFn key, int M, int want) {
    const int tid = threadIdx.x;
    Sel r; r.prefix = 0; r.shift = 56; r.tie = -1; r.none = 0;
    int need = want;
    for (int pass = 7; pass >= 0; --pass) {
        F.hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < M; i += THREADS) {
            const u64 u = key(i);
            if (u != 0 && (pass == 7 || (u >> (8 * (pass + 1))) == r.prefix)) atomicAdd(&F.hist[(unsigned)(u >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {                                          // digits in descending order: lane l owns 255 - 4l .. 252 - 4l
            int c[4], s = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { c[k] = (int)F.hist[255 - (4 * tid + k)]; s += c[k]; }
            int inc = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (tid >= o) inc += v; }
            const int total = __shfl(inc, 63, 64);
            const int nd = min(need, total);
            if (tid == 0) F.s_total = total;
            int a = inc - s;
            if (nd > 0 && a < nd && nd <= inc) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (a < nd && a + c[k] >= nd) { F.s_digit = 255 - (4 * tid + k); F.s_above = a; F.s_cnt = c[k]; }
                    a += c[k];
                }
            }
        }
        __syncthreads();
        need = min(need, F.s_total);
        if (need <= 0) { r.none = 1; break; }
        need -= F.s_above;
        r.prefix = (r.prefix << 8) | (u64)F.s_digit;
        r.shift = 8 * pass;
        if (F.s_cnt == need) break;                              // the whole bucket is taken
        if (pass == 0) r.tie = need;                             // equal keys straddle the cut: the lowest indices are taken
    }
    __syncthreads();
    return r;
}

template <class KeyFn>
__device__ __forceinline__ bool is_winner(const Sel& r, KeyFn key, u64 u, int i) {
    if (u == 0 || r.none) return false;
    const u64 hi = u >> r.shift;
    if (hi != r.prefix) return hi > r.prefix;
    if (r.tie < 0) return true;
    int rank = 0;
    for (int j = 0; j < i; ++j) rank += key(j) == u;
    return rank < r.tie;
}
