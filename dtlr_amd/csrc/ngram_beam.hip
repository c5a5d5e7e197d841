// Character n-gram CTC prefix beam search on the device (include/dtlr_hip.h: dtlr_ngram_beam).  gfx950 only.
//
// One workgroup of 256 threads per span, every span of a batch in one launch.  The beam (<= 64 hypotheses) lives in LDS, one lane
// of wave 0 per hypothesis for the per-hypothesis work; the K x N extension candidates of a frame are spread over all four waves.
// Per frame:
//   1. token list: all V - 1 non-blank channels, or the N largest E[t, c] (radix select over (value, -index) keys read from the row,
//      ordered compaction: ascending channel), with their fp64 log-probabilities, in LDS;
//   2. lane h: tot = pb (+) pnb, the stay terms, and the live hypothesis whose sequence is h's sequence minus its last label
//      (64-bit sequence hashes, confirmed on the back-pointer chain), whose extension by last(h) is the same label sequence as h;
//   3. that extension is merged into h's pnb' and its candidate slot is killed;
//   4. candidate keys (pb' (+) pnb') + lm, fp64, written to LDS once (the LM search is the expensive part of a key);
//   5. exact top-K: 8-bit radix select over the order-preserving 64-bit image of the keys (stops at the first digit where the
//      bucket holds exactly what is still needed), winners gathered, ranked by (key, candidate index) in wave 0;
//   6. the new beam is written in rank order; an extension appends its back-pointer node (parent, token) at arena slot t * K + rank.
// Scores are fp64 throughout.  Exact ties are ordered by candidate index (stay entries in beam order first, then extensions by
// (parent's beam slot, channel)): the same records on every run.
//
// The language model is a read-only sorted trie in global memory (dtlr_ngram_lm, packed by dtlr_amd.ngram.pack_lm): a hypothesis carries
// the node of the longest suffix of its context that the trie knows; a score is one binary search among the node's children per back-off hop.
#include "dtlr_common.h"
#include <math.h>

namespace {
using namespace dtlr;

constexpr int KMAX = 64;            // beam: one lane per hypothesis
constexpr int NTOK_MAX = 1024;      // tokens per frame that can be extended
constexpr int THREADS = 256;
constexpr size_t LDS_MAX = 150 * 1024;
typedef unsigned long long u64;

#define DTLR_NEG_INF (-__builtin_huge_val())

struct BeamFixed {
    double pb[2][KMAX], pnb[2][KMAX], lmv[2][KMAX];
    u64 hs[2][KMAX], phs[2][KMAX];               // hash of the label sequence / of the sequence without its last label
    double tot[KMAX], npb[KMAX], npnb[KMAX];
    u64 wkey[KMAX];
    int node[2][KMAX], pnode[2][KMAX], last[2][KMAX], lms[2][KMAX], len[2][KMAX];
    int dead[KMAX], widx[KMAX];
    unsigned hist[256];
    int wcnt[THREADS / 64];
    int s_total, s_digit, s_above, s_cnt, s_nw, s_pad;
};

struct BeamArgs {
    const float* em; const int* spans; int B, T, V, n;
    dtlr_ngram_lm lm; int has_lm; double wln10;
    int K, N, all_tokens, bos, eos, Tmax, Lmax;
    int* labels; int* lens; double* scores; int2* arena;
};

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
template <class KeyFn>
__device__ Sel radix_select(BeamFixed& F, KeyFn key, int M, int want) {
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

__global__ __launch_bounds__(THREADS) void ngram_beam_kernel(BeamArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    BeamFixed& F = *reinterpret_cast<BeamFixed*>(smem_raw);
    const int K = A.K, N = A.N, V = A.V;
    double* keys = reinterpret_cast<double*>(smem_raw + sizeof(BeamFixed));      // [KMAX stay | K x N extensions]
    double* lpt = keys + KMAX + (size_t)K * N;                                   // [N]
    int* toks = reinterpret_cast<int*>(lpt + N);                                  // [N]
    const int tid = threadIdx.x, sp = blockIdx.x;

    // the span table is device data nobody has checked: clamp it
    const int line = min(max(A.spans[3 * sp], 0), A.B - 1);
    const int t0 = min(max(A.spans[3 * sp + 1], 0), A.T);
    const int t1 = min(max(A.spans[3 * sp + 2], t0), A.T);
    const int nT = min(t1 - t0, A.Tmax);
    const float* em = A.em + ((size_t)line * A.T + t0) * V;
    int2* arena = A.arena + (size_t)sp * A.Tmax * K;
    int* labels = A.labels + (size_t)sp * A.Lmax;

    for (int i = tid; i < A.Lmax; i += THREADS) labels[i] = -1;
    int cur = 0, nlive = 1;
    if (tid < KMAX) {
        F.pb[0][tid] = tid == 0 ? 0.0 : DTLR_NEG_INF; F.pnb[0][tid] = DTLR_NEG_INF; F.lmv[0][tid] = 0.0;
        F.hs[0][tid] = 0x243F6A8885A308D3ull; F.phs[0][tid] = 0;
        F.node[0][tid] = -1; F.pnode[0][tid] = -1; F.last[0][tid] = 0; F.len[0][tid] = 0;
        F.lms[0][tid] = (A.has_lm && A.bos) ? A.lm.bos_state : 0;
    }
    if (A.all_tokens) for (int j = tid; j < N; j += THREADS) toks[j] = j + 1;
    __syncthreads();

    for (int t = 0; t < nT; ++t) {
        const float* row = em + (size_t)t * V;
        // ---- 1. tokens of this frame
        if (!A.all_tokens) {
            auto tkey = [&](int i) -> u64 {
                const unsigned b = __float_as_uint(row[i + 1]);
                const unsigned ub = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
                return ((u64)ub << 32) | (u64)(0xFFFFFFFFu - (unsigned)(i + 1));
            };
            const Sel r = radix_select(F, tkey, V - 1, N);
            int base = 0;
            for (int i0 = 0; i0 < V - 1; i0 += THREADS) {        // ordered compaction: ascending channel
                const int i = i0 + tid;
                const bool w = i < V - 1 && is_winner(r, tkey, tkey(i), i);
                const u64 bal = __ballot(w);
                if ((tid & 63) == 0) F.wcnt[tid >> 6] = __popcll(bal);
                __syncthreads();
                int off = base;
                for (int q = 0; q < (tid >> 6); ++q) off += F.wcnt[q];
                off += __popcll(bal & ((1ull << (tid & 63)) - 1ull));
                if (w && off < N) toks[off] = i + 1;
                for (int q = 0; q < THREADS / 64; ++q) base += F.wcnt[q];
                __syncthreads();
            }
        }
        for (int j = tid; j < N; j += THREADS) lpt[j] = log_prob(row[min(max(toks[j], 1), V - 1)]);
        // ---- 2. per hypothesis: stay terms, and the live parent sequence
        if (tid < KMAX) { F.dead[tid] = -1; keys[tid] = DTLR_NEG_INF; }
        int par = -1;
        if (tid < nlive) {
            const int h = tid;
            const double pb = F.pb[cur][h], pnb = F.pnb[cur][h];
            const double tot = log_add(pb, pnb);
            F.tot[h] = tot;
            F.npb[h] = tot + log_prob(row[0]);
            const int ln = F.len[cur][h];
            F.npnb[h] = ln > 0 ? pnb + log_prob(row[min(max(F.last[cur][h], 0), V - 1)]) : DTLR_NEG_INF;
            if (ln > 0) {
                const u64 ph = F.phs[cur][h];
                for (int g = 0; g < nlive && par < 0; ++g) {
                    if (F.len[cur][g] + 1 != ln || F.hs[cur][g] != ph) continue;
                    int a = F.node[cur][g], b = F.pnode[cur][h];
                    bool same = true;
                    for (int it = 0; it < ln && a != b; ++it) {  // equal hashes, different nodes: compare the chains
                        if (a < 0 || b < 0) { same = false; break; }
                        const int2 na = arena[a], nb = arena[b];
                        if (na.y != nb.y) { same = false; break; }
                        a = na.x; b = nb.x;
                    }
                    if (same && a == b) par = g;
                }
            }
        }
        __syncthreads();
        // ---- 3. the parent's extension by last(h) is h itself: merge it, kill its slot
        if (tid < nlive && par >= 0) {
            const int c = F.last[cur][tid];
            int j = -1;
            if (A.all_tokens) j = c - 1;
            else {
                int lo = 0, hi = N;
                for (int it = 0; it < 16 && lo < hi; ++it) {
                    const int mid = (lo + hi) >> 1, tk = toks[mid];
                    if (tk == c) { j = mid; break; }
                    if (tk < c) lo = mid + 1; else hi = mid;
                }
            }
            if (j >= 0 && j < N) {
                const double base = (c == F.last[cur][par] && F.len[cur][par] > 0) ? F.pb[cur][par] : F.tot[par];
                if (base != DTLR_NEG_INF) F.npnb[tid] = log_add(F.npnb[tid], base + lpt[j]);
                F.dead[tid] = par * N + j;
            }
        }
        __syncthreads();
        // ---- 4. candidate keys
        if (tid < nlive) keys[tid] = log_add(F.npb[tid], F.npnb[tid]) + F.lmv[cur][tid];
        for (int e = tid; e < nlive * N; e += THREADS) {
            const int h = e / N, j = e - h * N, c = toks[j];
            const double base = (c == F.last[cur][h] && F.len[cur][h] > 0) ? F.pb[cur][h] : F.tot[h];
            double k = DTLR_NEG_INF;
            if (base != DTLR_NEG_INF) {
                k = base + lpt[j] + F.lmv[cur][h];
                if (A.has_lm) { int ns; k += A.wln10 * lm_walk(A.lm, F.lms[cur][h], c, &ns); }
            }
            keys[KMAX + e] = k;
        }
        __syncthreads();
        if (tid < nlive && F.dead[tid] >= 0) keys[KMAX + F.dead[tid]] = DTLR_NEG_INF;
        if (tid == 0) F.s_nw = 0;
        __syncthreads();
        // ---- 5. the K best
        const int M = KMAX + nlive * N;
        auto bkey = [&](int i) -> u64 { return ukey(keys[i]); };
        const Sel r = radix_select(F, bkey, M, K);
        for (int i = tid; i < M; i += THREADS) {
            const u64 u = bkey(i);
            if (is_winner(r, bkey, u, i)) {
                const int slot = atomicAdd(&F.s_nw, 1);
                if (slot < KMAX) { F.widx[slot] = i; F.wkey[slot] = u; }
            }
        }
        __syncthreads();
        const int nw = min(F.s_nw, K);
        // ---- 6. the new beam, in rank order
        const int nxt = cur ^ 1;
        if (tid < nw) {
            const u64 u = F.wkey[tid];
            const int i = F.widx[tid];
            int rank = 0;
            for (int m = 0; m < nw; ++m) rank += (F.wkey[m] > u) || (F.wkey[m] == u && F.widx[m] < i);
            if (i < KMAX) {
                const int h = i;
                F.pb[nxt][rank] = F.npb[h]; F.pnb[nxt][rank] = F.npnb[h]; F.lmv[nxt][rank] = F.lmv[cur][h];
                F.hs[nxt][rank] = F.hs[cur][h]; F.phs[nxt][rank] = F.phs[cur][h];
                F.node[nxt][rank] = F.node[cur][h]; F.pnode[nxt][rank] = F.pnode[cur][h];
                F.last[nxt][rank] = F.last[cur][h]; F.lms[nxt][rank] = F.lms[cur][h]; F.len[nxt][rank] = F.len[cur][h];
            } else {
                const int e = i - KMAX, h = e / N, j = e - h * N, c = toks[j];
                const double base = (c == F.last[cur][h] && F.len[cur][h] > 0) ? F.pb[cur][h] : F.tot[h];
                double lmv = F.lmv[cur][h];
                int ns = 0;
                if (A.has_lm) lmv += A.wln10 * lm_walk(A.lm, F.lms[cur][h], c, &ns);
                const int nd = t * K + rank;
                arena[nd] = make_int2(F.node[cur][h], c);
                F.pb[nxt][rank] = DTLR_NEG_INF; F.pnb[nxt][rank] = base + lpt[j]; F.lmv[nxt][rank] = lmv;
                F.hs[nxt][rank] = F.hs[cur][h] * 0x9E3779B97F4A7C15ull + (u64)(c + 1); F.phs[nxt][rank] = F.hs[cur][h];
                F.node[nxt][rank] = nd; F.pnode[nxt][rank] = F.node[cur][h];
                F.last[nxt][rank] = c; F.lms[nxt][rank] = ns; F.len[nxt][rank] = F.len[cur][h] + 1;
            }
        }
        nlive = nw;
        cur = nxt;
        __syncthreads();
    }

    // ---- the best hypothesis (with the end-of-sentence term) and its labels
    if (tid < nlive) {
        double s = log_add(F.pb[cur][tid], F.pnb[cur][tid]) + F.lmv[cur][tid];
        if (A.has_lm && A.eos) { int ns; s += A.wln10 * lm_walk(A.lm, F.lms[cur][tid], A.lm.eos_tok, &ns); }
        F.tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        for (int h = 1; h < nlive; ++h) if (F.tot[h] > F.tot[best]) best = h;
        const int ln = F.len[cur][best];
        int nd = F.node[cur][best];
        for (int p = ln - 1; p >= 0 && nd >= 0; --p) {
            const int2 v = arena[nd];
            if (p < A.Lmax) labels[p] = v.y;
            nd = v.x;
        }
        A.lens[sp] = min(ln, A.Lmax);
        A.scores[sp] = F.tot[best];
    }
}

}  // namespace

extern "C" long dtlr_ngram_beam_workspace_bytes(int n, int Tmax, int K)
{
    if (n <= 0 || Tmax <= 0 || K <= 0) return 16;
    return (long)n * Tmax * K * (long)sizeof(int2) + 16;
}

extern "C" int dtlr_ngram_beam(const float* emissions, int B, int T, int V, const int* spans, int n, int Tmax,
                               const dtlr_ngram_lm* lm, double lm_weight, int K, int N, int bos, int eos,
                               int* labels_out, int Lmax, int* len_out, double* score_out, void* workspace, void* stream)
{
    clear_stale_error();
    if (n == 0) return DTLR_OK;
    if (!emissions || !spans || !labels_out || !len_out || !score_out || !workspace) return DTLR_EINVAL;
    if (B <= 0 || T <= 0 || V < 2 || n < 0 || Tmax < 0 || Lmax <= 0) return DTLR_EINVAL;
    if (K < 1 || K > KMAX || V > 65536 || Lmax < Tmax) return DTLR_ESHAPE;
    if (N <= 0 || N > V - 1) N = V - 1;
    if (N > NTOK_MAX) return DTLR_ESHAPE;
    if (lm && (!lm->tok || !lm->child_lo || !lm->child_hi || !lm->suffix || !lm->ctx || !lm->logp || !lm->bo || lm->n_nodes < 1 ||
               lm->bos_state < 0 || lm->bos_state >= lm->n_nodes)) return DTLR_EINVAL;
    const size_t lds = sizeof(BeamFixed) + ((size_t)KMAX + (size_t)K * N + N) * 8 + (size_t)N * 4;
    if (lds > LDS_MAX) return DTLR_ESHAPE;
    BeamArgs A;
    A.em = emissions; A.spans = spans; A.B = B; A.T = T; A.V = V; A.n = n;
    A.has_lm = lm != nullptr;
    if (lm) A.lm = *lm; else A.lm = dtlr_ngram_lm{};
    A.wln10 = lm_weight * 2.302585092994046;
    A.K = K; A.N = N; A.all_tokens = N == V - 1; A.bos = bos != 0; A.eos = eos != 0 && lm;
    A.Tmax = Tmax; A.Lmax = Lmax;                               // Tmax = 0: no span runs a frame, the arena is not touched
    A.labels = labels_out; A.lens = len_out; A.scores = score_out;
    A.arena = reinterpret_cast<int2*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    return launch<ngram_beam_kernel>(dim3((unsigned)n), dim3(THREADS), lds, (hipStream_t)stream, A);
}
