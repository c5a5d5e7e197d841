// Word beam search on the device (include/dtlr_wordbeam.h: dtlr_word_beam; semantics: DESIGN.md section 17).  gfx950 only.
//
// The CTC prefix beam search of ngram_beam.hip over WHOLE LINES, with two changes: a hypothesis may only be extended inside a dictionary
// (a trie of the words' channels: a word character must be a child of the hypothesis' trie node, a separator needs the root or a node
// where a word ends), and the language model is a WORD n-gram whose term is added when a word completes (a separator after a word, or
// the end of the span).  One workgroup of 256 threads per span, every span of a batch in one launch; the beam (<= 64 hypotheses) in
// LDS, one lane of wave 0 per hypothesis; the K x N candidates of a frame over all four waves.  The frame loop is ngram_beam.hip's,
// step by step (tokens, stay terms and the live parent, the merge, keys, exact radix top-K, the new beam in rank order); what differs:
//   * a hypothesis also carries dn, its dictionary node (0 = the root: the sequence is empty or ends in a separator), and its LM state
//     is the word LM's (the node of the packed back-off trie after its completed words);
//   * a candidate's key looks its channel up among dn's children (binary search in the node's sorted child range) or, for a separator,
//     walks the word LM once; a character extension never touches the LM;
//   * the key that is RANKED adds w ln10 ahead[dn'] (the best unigram of any word at or below the node: a hypothesis inside a word has
//     not paid for it yet); the score that is kept does not;
//   * at the end only complete hypotheses (root, or a node where a word ends) compete; none: length -1, score -inf.
// Every table is device data nobody has checked: nodes, child ranges, word ids and classes are clamped where they are read.
#include "dtlr_common.h"
#include "../../include/dtlr_wordbeam.h"
#include <math.h>

namespace {
using namespace dtlr;

constexpr int KMAX = 64;            // beam: one lane per hypothesis
constexpr int NTOK_MAX = 1024;      // tokens per frame that can be extended
constexpr int THREADS = 256;
constexpr int DEPTH_MAX = 64;       // characters of a dictionary word
constexpr size_t LDS_MAX = 150 * 1024;

#include "beam_common.h"

struct WordFixed {
    double pb[2][KMAX], pnb[2][KMAX], lmv[2][KMAX];
    u64 hs[2][KMAX], phs[2][KMAX];               // hash of the label sequence / of the sequence without its last label
    double tot[KMAX], npb[KMAX], npnb[KMAX];
    u64 wkey[KMAX];
    int node[2][KMAX], pnode[2][KMAX], last[2][KMAX], lms[2][KMAX], len[2][KMAX];
    int dn[2][KMAX];                             // dictionary node of the trailing run of word characters
    int dead[KMAX], widx[KMAX];
    unsigned hist[256];
    int wcnt[THREADS / 64];
    int s_total, s_digit, s_above, s_cnt, s_nw, s_pad;
};

struct WordArgs {
    const float* em; const int* spans; int B, T, V, n;
    const int *child_lo, *child_hi, *chan, *word, *cls; const double* ahead; int n_nodes, W;
    dtlr_ngram_lm lm; int has_lm, look; double wln10;
    int K, N, all_tokens, bos, eos, Tmax, Lmax;
    int* labels; int* lens; double* scores; int2* arena;
};

// w ln10 ahead[node]: part of the ranked key only
__device__ __forceinline__ double look(const WordArgs& A, int dn) {
    return A.look ? A.wln10 * A.ahead[min(max(dn, 0), A.n_nodes - 1)] : 0.0;
}

// The extension of (dictionary node dn, LM state s) by channel c: false when the dictionary forbids it; else the node and state after
// it and the LM term it adds (0 unless a word completes).
__device__ bool word_step(const WordArgs& A, int dn, int s, int c, int* dn2, int* s2, double* term) {
    const int n = A.n_nodes;
    dn = min(max(dn, 0), n - 1);
    const int k = A.cls[min(max(c, 0), A.V - 1)];
    *s2 = s; *term = 0.0; *dn2 = 0;
    if (k == 1) {
        int lo = min(max(A.child_lo[dn], 0), n), hi = min(max(A.child_hi[dn], 0), n);
        for (int it = 0; it < 32 && lo < hi; ++it) {
            const int mid = (lo + hi) >> 1, ch = A.chan[mid];
            if (ch == c) { *dn2 = mid; return true; }
            if (ch < c) lo = mid + 1; else hi = mid;
        }
        return false;
    }
    if (k != 2) return false;
    if (dn == 0) return true;
    const int wd = min(max(A.word[dn], -1), A.W - 1);
    if (wd < 0) return false;
    if (A.has_lm) *term = A.wln10 * lm_walk(A.lm, s, wd + 1, s2);
    return true;
}

__global__ __launch_bounds__(THREADS) void word_beam_kernel(WordArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WordFixed& F = *reinterpret_cast<WordFixed*>(smem_raw);
    const int K = A.K, N = A.N, V = A.V;
    double* keys = reinterpret_cast<double*>(smem_raw + sizeof(WordFixed));      // [KMAX stay | K x N extensions]
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
        F.dn[0][tid] = 0;
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
        if (tid < nlive) keys[tid] = (log_add(F.npb[tid], F.npnb[tid]) + F.lmv[cur][tid]) + look(A, F.dn[cur][tid]);
        for (int e = tid; e < nlive * N; e += THREADS) {
            const int h = e / N, j = e - h * N, c = toks[j];
            const double base = (c == F.last[cur][h] && F.len[cur][h] > 0) ? F.pb[cur][h] : F.tot[h];
            double k = DTLR_NEG_INF;
            if (base != DTLR_NEG_INF) {
                int dn2, ns;
                double term;
                if (word_step(A, F.dn[cur][h], F.lms[cur][h], c, &dn2, &ns, &term)) k = ((base + lpt[j]) + (F.lmv[cur][h] + term)) + look(A, dn2);
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
                F.dn[nxt][rank] = F.dn[cur][h];
            } else {
                const int e = i - KMAX, h = e / N, j = e - h * N, c = toks[j];
                const double base = (c == F.last[cur][h] && F.len[cur][h] > 0) ? F.pb[cur][h] : F.tot[h];
                int dn2 = 0, ns = 0;
                double term = 0.0;
                word_step(A, F.dn[cur][h], F.lms[cur][h], c, &dn2, &ns, &term);     // a winner was allowed: the same walk as its key's
                const double lmv = F.lmv[cur][h] + term;
                const int nd = t * K + rank;
                arena[nd] = make_int2(F.node[cur][h], c);
                F.pb[nxt][rank] = DTLR_NEG_INF; F.pnb[nxt][rank] = base + lpt[j]; F.lmv[nxt][rank] = lmv;
                F.hs[nxt][rank] = F.hs[cur][h] * 0x9E3779B97F4A7C15ull + (u64)(c + 1); F.phs[nxt][rank] = F.hs[cur][h];
                F.node[nxt][rank] = nd; F.pnode[nxt][rank] = F.node[cur][h];
                F.last[nxt][rank] = c; F.lms[nxt][rank] = ns; F.len[nxt][rank] = F.len[cur][h] + 1;
                F.dn[nxt][rank] = dn2;
            }
        }
        nlive = nw;
        cur = nxt;
        __syncthreads();
    }

    // ---- the best COMPLETE hypothesis (its pending word's term, then the end-of-sentence term) and its labels
    if (tid < KMAX) F.dead[tid] = 0;                         // reused after the last frame: 1 = the hypothesis is complete
    __syncthreads();
    if (tid < nlive) {
        const int dn = min(max(F.dn[cur][tid], 0), A.n_nodes - 1);
        const int wd = dn == 0 ? -1 : min(max(A.word[dn], -1), A.W - 1);
        double s = log_add(F.pb[cur][tid], F.pnb[cur][tid]) + F.lmv[cur][tid];
        int st = F.lms[cur][tid];
        if (dn == 0 || wd >= 0) {
            if (A.has_lm && wd >= 0) s += A.wln10 * lm_walk(A.lm, st, wd + 1, &st);
            if (A.has_lm && A.eos) { int ns; s += A.wln10 * lm_walk(A.lm, st, A.lm.eos_tok, &ns); }
            F.dead[tid] = 1;
        }
        F.tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int best = -1;
        for (int h = 0; h < nlive; ++h) if (F.dead[h] && (best < 0 || F.tot[h] > F.tot[best])) best = h;
        if (best < 0) {                                          // no complete hypothesis: the labels are all -1 already
            A.lens[sp] = -1;
            A.scores[sp] = DTLR_NEG_INF;
        } else {
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
}

}  // namespace

extern "C" long dtlr_word_beam_workspace_bytes(int n, int Tmax, int K)
{
    if (n <= 0 || Tmax <= 0 || K <= 0) return 16;
    return (long)n * Tmax * K * (long)sizeof(int2) + 16;
}

extern "C" int dtlr_word_beam(const float* emissions, int B, int T, int V, const int* spans, int n, int Tmax,
                              const int* child_lo, const int* child_hi, const int* chan, const int* node_word, const double* ahead,
                              int n_nodes, int max_depth, int W, const int* cls,
                              const dtlr_ngram_lm* lm, double lm_weight, int K, int N, int bos, int eos, int lookahead,
                              int* labels_out, int Lmax, int* len_out, double* score_out, void* workspace, void* stream)
{
    clear_stale_error();
    if (n == 0) return DTLR_OK;
    if (!emissions || !spans || !labels_out || !len_out || !score_out || !workspace) return DTLR_EINVAL;
    if (!child_lo || !child_hi || !chan || !node_word || !ahead || !cls) return DTLR_EINVAL;
    if (B <= 0 || T <= 0 || V < 2 || n < 0 || Tmax < 0 || Lmax <= 0 || n_nodes < 1 || W < 0 || max_depth < 0) return DTLR_EINVAL;
    if (K < 1 || K > KMAX || V > 65536 || Lmax < Tmax || max_depth > DEPTH_MAX) return DTLR_ESHAPE;
    if (N <= 0 || N > V - 1) N = V - 1;
    if (N > NTOK_MAX) return DTLR_ESHAPE;
    if (lm && (!lm->tok || !lm->child_lo || !lm->child_hi || !lm->suffix || !lm->ctx || !lm->logp || !lm->bo || lm->n_nodes < 1 ||
               lm->bos_state < 0 || lm->bos_state >= lm->n_nodes)) return DTLR_EINVAL;
    const size_t lds = sizeof(WordFixed) + ((size_t)KMAX + (size_t)K * N + N) * 8 + (size_t)N * 4;
    if (lds > LDS_MAX) return DTLR_ESHAPE;
    WordArgs A;
    A.em = emissions; A.spans = spans; A.B = B; A.T = T; A.V = V; A.n = n;
    A.child_lo = child_lo; A.child_hi = child_hi; A.chan = chan; A.word = node_word; A.cls = cls; A.ahead = ahead;
    A.n_nodes = n_nodes; A.W = W;
    A.has_lm = lm != nullptr;
    if (lm) A.lm = *lm; else A.lm = dtlr_ngram_lm{};
    A.wln10 = lm_weight * 2.302585092994046;
    A.look = lm != nullptr && lookahead != 0;
    A.K = K; A.N = N; A.all_tokens = N == V - 1; A.bos = bos != 0; A.eos = eos != 0 && lm;
    A.Tmax = Tmax; A.Lmax = Lmax;                               // Tmax = 0: no span runs a frame, the arena is not touched
    A.labels = labels_out; A.lens = len_out; A.scores = score_out;
    A.arena = reinterpret_cast<int2*>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15);
    return launch<word_beam_kernel>(dim3((unsigned)n), dim3(THREADS), lds, (hipStream_t)stream, A);
}
