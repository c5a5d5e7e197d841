// Regular-expression decoding and spotting over the CTC lattice: a deterministic automaton (the host compiles
// it, dtlr_amd/pattern.py) run against the emissions of a batch.  The word trie of lexicon.hip and the single keyword of ctc_spot.hip
// are special cases of it.
//   pattern_decode_kernel  one workgroup per span, a bounded grid: workgroup g takes spans g, g + G, ...  The best string of the
//                          language over the span's frames, with its traceback.
//   pattern_search_kernel  one workgroup per line: every occurrence of the language, free start and end, and in the same launch the
//                          greedy selection of up to H hits that do not overlap.
// Both run the same frame step.  A value (d, n[, e]) lives on every arc (nb: the frame emits the arc's channel) and on every state (b:
// a blank after arriving there), double-buffered in the workgroup's slice of the caller's workspace: item i < A is arc i, item A + q
// state q.  A frame is two phases with a barrier between them:
//   reduce   per state q, over the arcs into q (a contiguous range: the arcs are sorted by destination), two records: the best arc by
//            key (lowest id on ties) and the best arc whose channel differs from the first's.  They stand for the ordered maximum over
//            "the arcs into src whose channel is not mine" of every arc that leaves q.  A state with up to PAT_LIGHT incoming arcs is
//            one thread's; the others (`.+` at V = 7357 has thousands) are listed once per workgroup in LDS and reduced by a wave each.
//   update   per item, the new value from the old values and the records.
// The workgroup is sized by the automaton (64 threads for a date pattern: its barriers cost nothing), and the frame's fp64 logs are
// staged in LDS as lexicon.hip stages them (two rows when they fit, so that the fill of frame t + 1 hides behind frame t).
// Nothing here synchronises with the host.  The tables are device data: sources are clamped to [0, S), channels to [0, V), arc ranges
// to [0, A] and made non-decreasing, spans as dtlr_ctc_align clamps them, and every back-pointer that is followed; the traceback walks
// at most F frames.  A bad table gives a wrong record, never a fault.  No 16-bit type is involved: both builds export the same code.
#include "dtlr_common.h"
#include "../../include/dtlr_pattern.h"

// key = d + bonus * n is a product, then a sum: a fused multiply-add would round once and could order two candidates differently
#pragma clang fp contract(off)

namespace dtlr {

constexpr int PAT_GRID = 2048;                       // workgroups at the most
constexpr int PAT_SMAX = 4096;                       // states
constexpr int PAT_AMAX = 1 << 20;                    // arcs
constexpr int PAT_HMAX = 16;
constexpr int PAT_VMAX = 15360;                      // 8 V bytes of LDS: 120 KB
constexpr int PAT_MAX_THREADS = 1024;
constexpr int PAT_MAX_WAVES = PAT_MAX_THREADS / 64;
constexpr int PAT_LIGHT = 32;                        // incoming arcs one thread reduces alone
constexpr size_t PAT_LDS_ROWS = 120 * 1024;          // dynamic LDS: the rows of logs; the static arrays (below) take 17 KB of the rest

struct PatBest {                                     // a candidate of an arg-max: id < 0 is none
    double key;
    int id;
};
struct PatRec {                                      // the two records of a state while they are reduced
    double k1, k2;
    int r1, c1, r2;
};
struct PatTables {
    const int* arc_src;
    const int* arc_chan;
    const int* dst_start;
    const int* accept;
    int S, A, V;
};

static_assert(PAT_LDS_ROWS + PAT_SMAX * sizeof(int) + 2 * PAT_MAX_WAVES * (sizeof(float) + sizeof(PatBest)) + 256 <= 160 * 1024,
              "the rows of logs and the static arrays share 160 KB of LDS");
static_assert((size_t)PAT_VMAX * 8 <= PAT_LDS_ROWS, "one row of logs of the widest vocabulary fits");

__device__ __forceinline__ double pat_key(double d, int n, double bonus)
{
    const double p = __dmul_rn(bonus, (double)n);
    return __dadd_rn(d, p);
}
// whether (ka, ia) comes before (kb, ib): the larger key, the lower id on equal keys
__device__ __forceinline__ bool pat_before(double ka, int ia, double kb, int ib)
{
    if (ia < 0) return false;
    if (ib < 0) return true;
    return ka > kb || (ka == kb && ia < ib);
}
__device__ __forceinline__ void pat_take(PatBest& best, double key, int id)
{
    if (pat_before(key, id, best.key, best.id)) { best.key = key; best.id = id; }
}
__device__ __forceinline__ PatBest pat_wave_best(PatBest v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const double k = __shfl_xor(v.key, off);
        const int i = __shfl_xor(v.id, off);
        pat_take(v, k, i);
    }
    return v;
}
__device__ __forceinline__ int pat_chan(const PatTables& tb, int a) { return min(max(tb.arc_chan[a], 0), tb.V - 1); }
__device__ __forceinline__ void pat_range(const PatTables& tb, int q, int& lo, int& hi)
{
    lo = min(max(tb.dst_start[q], 0), tb.A);
    hi = min(max(tb.dst_start[q + 1], lo), tb.A);
}

// one more arc, in ascending id, into the records of its state
__device__ __forceinline__ void pat_rec_add(PatRec& r, double k, int x, int c)
{
    if (k > r.k1) {
        if (r.r1 >= 0 && c != r.c1) { r.r2 = r.r1; r.k2 = r.k1; }       // the old best is the best of another channel than x's
        r.r1 = x; r.k1 = k; r.c1 = c;
    } else if (c != r.c1 && k > r.k2) {
        r.r2 = x; r.k2 = k;
    }
}
// the records of two disjoint sets of arcs -> those of their union
__device__ __forceinline__ PatRec pat_rec_merge(const PatRec& a, const PatRec& b)
{
    PatRec o;
    const bool bf = pat_before(b.k1, b.r1, a.k1, a.r1);
    o.k1 = bf ? b.k1 : a.k1; o.r1 = bf ? b.r1 : a.r1; o.c1 = bf ? b.c1 : a.c1;
    const bool a1 = a.r1 >= 0 && a.c1 != o.c1, b1 = b.r1 >= 0 && b.c1 != o.c1;   // each set's best arc of a channel other than c1
    const double ka = a1 ? a.k1 : a.k2, kb = b1 ? b.k1 : b.k2;
    const int ia = a1 ? a.r1 : a.r2, ib = b1 ? b.r1 : b.r2;
    const bool b2 = pat_before(kb, ib, ka, ia);
    o.k2 = b2 ? kb : ka; o.r2 = b2 ? ib : ia;
    return o;
}

// the states with more than PAT_LIGHT incoming arcs, once per workgroup (their order does not matter)
__device__ void pat_list_heavy(const PatTables& tb, int* heavy, int* nheavy)
{
    if (threadIdx.x == 0) *nheavy = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < tb.S; q += blockDim.x) {
        int lo, hi;
        pat_range(tb, q, lo, hi);
        if (hi - lo > PAT_LIGHT) heavy[atomicAdd(nheavy, 1)] = q;
    }
    __syncthreads();
}

// phase 1: rec[q] = (best arc into q, best arc into q of another channel), -1 = none, from the values pd / pn.  ENDS: `ends` also takes
// the best arc into an accepting state (the thread's share: pat_wave_best and the waves' slots make it the workgroup's).
template <bool ENDS>
__device__ __forceinline__ void pat_reduce(const PatTables& tb, const double* pd, const int* pn, double bonus, int2* rec,
                                           const int* heavy, int nheavy, PatBest& ends)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    for (int q = tid; q < tb.S; q += blockDim.x) {
        int lo, hi;
        pat_range(tb, q, lo, hi);
        if (hi - lo > PAT_LIGHT) continue;
        PatRec r;
        r.k1 = r.k2 = -INFINITY; r.r1 = r.r2 = r.c1 = -1;
        for (int x = lo; x < hi; ++x) pat_rec_add(r, pat_key(pd[x], pn[x], bonus), x, pat_chan(tb, x));
        rec[q] = make_int2(r.r1, r.r2);
        if (ENDS && tb.accept[q]) pat_take(ends, r.k1, r.r1);
    }
    for (int h = wave; h < nheavy; h += nw) {                                   // wave-uniform
        const int q = min(max(heavy[h], 0), tb.S - 1);
        int lo, hi;
        pat_range(tb, q, lo, hi);
        PatRec r;
        r.k1 = r.k2 = -INFINITY; r.r1 = r.r2 = r.c1 = -1;
        for (int x = lo + lane; x < hi; x += 64) pat_rec_add(r, pat_key(pd[x], pn[x], bonus), x, pat_chan(tb, x));
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            PatRec o;
            o.k1 = __shfl_xor(r.k1, off); o.k2 = __shfl_xor(r.k2, off);
            o.r1 = __shfl_xor(r.r1, off); o.c1 = __shfl_xor(r.c1, off); o.r2 = __shfl_xor(r.r2, off);
            r = pat_rec_merge(r, o);
        }
        if (lane == 0) {
            rec[q] = make_int2(r.r1, r.r2);
            if (ENDS && tb.accept[q]) pat_take(ends, r.k1, r.r1);
        }
    }
}

// phase 2: the values of frame t (cd / cn / ce) from those of frame t - 1 and the records.  lp: the frame's logs in LDS; sub: what is
// taken off each (0 in decode, ln of the frame's maximum in search).  bp (decode): one byte per item, which candidate won.
template <bool SEARCH>
__device__ __forceinline__ void pat_update(const PatTables& tb, const double* pd, const int* pn, const int* pe, double* cd, int* cn,
                                           int* ce, const int2* rec, const double* lp, double sub, double bonus, int t,
                                           unsigned char* bp)
{
    const int A = tb.A, N = tb.A + tb.S;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        double dw = pd[i];                                                      // stay
        int nw = pn[i], ew = SEARCH ? pe[i] : 0, code = 0, ch = 0;
        double kw = pat_key(dw, nw, bonus);
        if (i < A) {
            const int src = min(max(tb.arc_src[i], 0), tb.S - 1);
            ch = pat_chan(tb, i);
            {                                                                   // b(src)
                const double d = pd[A + src];
                const int n = pn[A + src];
                const double k = pat_key(d, n, bonus);
                if (k > kw) { kw = k; dw = d; nw = n; if (SEARCH) ew = pe[A + src]; code = 1; }
            }
            const int2 rc = rec[src];                                           // the arcs into src of another channel
            int x = -1, cx = 0;
            if (rc.x >= 0) {
                const int r1 = min(rc.x, A - 1);
                if (pat_chan(tb, r1) != ch) { x = r1; cx = 2; }
                else if (rc.y >= 0) { x = min(rc.y, A - 1); cx = 3; }
            }
            if (x >= 0) {
                const double d = pd[x];
                const int n = pn[x];
                const double k = pat_key(d, n, bonus);
                if (k > kw) { kw = k; dw = d; nw = n; if (SEARCH) ew = pe[x]; code = cx; }
            }
            if (SEARCH && src == 0 && 0.0 > kw) { dw = 0.0; nw = 0; ew = t; code = 4; }     // the fresh entry (0, 0, t): key 0
            nw += code ? 1 : 0;
        } else {
            const int r1 = rec[i - A].x;                                        // the arcs into q: the best of them
            if (r1 >= 0) {
                const int x = min(r1, A - 1);
                const double d = pd[x];
                const int n = pn[x];
                const double k = pat_key(d, n, bonus);
                if (k > kw) { kw = k; dw = d; nw = n; if (SEARCH) ew = pe[x]; code = 1; }
            }
        }
        cd[i] = dw + (lp[ch] - sub);
        cn[i] = nw;
        if (SEARCH) ce[i] = ew;
        else bp[i] = (unsigned char)code;
    }
}

// frame t's logs into `lp` and every wave's fp32 maximum of its channels into wmax
__device__ __forceinline__ void pat_fill(const float* e, int V, double* lp, float* wmax)
{
    float m = -INFINITY;
    for (int c = threadIdx.x; c < V; c += blockDim.x) {
        const float v = e[c];
        lp[c] = log(fmax((double)v, 1e-30));
        m = fmaxf(m, v);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
}
__device__ __forceinline__ double pat_lnmax(const float* wmax)
{
    float m = wmax[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, wmax[w]);
    return log(fmax((double)m, 1e-30));
}

static inline long pat_round16(long v) { return (v + 15) / 16 * 16; }
static inline long pat_groups(int n) { return n < PAT_GRID ? n : PAT_GRID; }
static inline long pat_decode_group_bytes(int S, int A, int Tmax)
{
    const long N = (long)A + S;
    return pat_round16(24 * N + 8 * ((long)Tmax + 1) * S + (long)Tmax * N);
}
static inline long pat_search_group_bytes(int S, int A, int T) { return pat_round16(32 * ((long)A + S) + 8 * (long)S + 24 * (long)T); }
// the workgroup: one thread per item up to 1024, whole waves
static inline int pat_threads(int S, int A)
{
    const long N = (long)A + S;
    const long t = (N + 63) / 64 * 64;
    return (int)(t < 64 ? 64 : t > PAT_MAX_THREADS ? PAT_MAX_THREADS : t);
}

__global__ __launch_bounds__(PAT_MAX_THREADS) void pattern_decode_kernel(
    const float* __restrict__ E, const int* __restrict__ spans, PatTables tb, double bonus, int* __restrict__ labels,
    int* __restrict__ length, double* __restrict__ score, double* __restrict__ base, unsigned char* ws, long group_bytes, int B, int T,
    int n, int Tmax, int Lcap, int two_rows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pat_smem[];        // double lp[two_rows ? 2 : 1][V]
    __shared__ int s_heavy[PAT_SMAX];
    __shared__ int s_nheavy;
    __shared__ float s_wmax[2][PAT_MAX_WAVES];
    __shared__ PatBest s_arc[PAT_MAX_WAVES], s_blank[PAT_MAX_WAVES];
    double* lpbuf = reinterpret_cast<double*>(pat_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int S = tb.S, A = tb.A, V = tb.V, N = A + S;

    unsigned char* mine = ws + (size_t)blockIdx.x * group_bytes;
    double* d0 = reinterpret_cast<double*>(mine);
    double* d1 = d0 + N;
    int2* recs = reinterpret_cast<int2*>(d1 + N);                                    // [Tmax + 1][S]
    int* n0 = reinterpret_cast<int*>(recs + ((size_t)Tmax + 1) * S);
    int* n1 = n0 + N;
    unsigned char* bps = reinterpret_cast<unsigned char*>(n1 + N);                   // [Tmax][N]

    pat_list_heavy(tb, s_heavy, &s_nheavy);
    const int nheavy = s_nheavy;

    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int b = min(max(spans[3 * k], 0), B - 1);
        const int t0 = min(max(spans[3 * k + 1], 0), T);
        const int t1 = min(max(spans[3 * k + 2], t0), T);
        const int F = min(t1 - t0, Tmax);                                           // block-uniform
        const float* eline = E + ((long)b * T + t0) * V;

        double *pd = d0, *cd = d1;
        int *pn = n0, *cn = n1;
        for (int i = tid; i < N; i += blockDim.x) { pd[i] = i == A ? 0.0 : -INFINITY; pn[i] = 0; }   // b(0) = (0, 0)
        for (int i = tid; i < Lcap; i += blockDim.x) labels[(long)k * Lcap + i] = -1;
        if (F > 0) pat_fill(eline, V, lpbuf, s_wmax[0]);
        __syncthreads();
        double bsum = 0.0;                                                          // thread 0's: the sum of ln mx in frame order
        PatBest none;
        none.key = -INFINITY; none.id = -1;
        for (int t = 0; t < F; ++t) {
            const int r = two_rows ? (t & 1) : 0;
            if (two_rows && t + 1 < F) pat_fill(eline + (long)(t + 1) * V, V, lpbuf + (size_t)(r ^ 1) * V, s_wmax[r ^ 1]);
            if (tid == 0) bsum += pat_lnmax(s_wmax[r]);
            int2* rec = recs + (size_t)t * S;
            PatBest unused = none;
            pat_reduce<false>(tb, pd, pn, bonus, rec, s_heavy, nheavy, unused);
            __syncthreads();
            pat_update<false>(tb, pd, pn, nullptr, cd, cn, nullptr, rec, lpbuf + (size_t)r * V, 0.0, bonus, t, bps + (size_t)t * N);
            __syncthreads();
            if (!two_rows && t + 1 < F) {
                pat_fill(eline + (long)(t + 1) * V, V, lpbuf, s_wmax[0]);
                __syncthreads();
            }
            double* sd = pd; pd = cd; cd = sd;
            int* sn = pn; pn = cn; cn = sn;
        }

        // the end: the arcs into accepting states by ascending id, then b(q) of accepting q ascending
        PatBest arc = none, blank = none;
        pat_reduce<true>(tb, pd, pn, bonus, recs + (size_t)F * S, s_heavy, nheavy, arc);
        for (int q = tid; q < S; q += blockDim.x)
            if (tb.accept[q]) {
                const double kq = pat_key(pd[A + q], pn[A + q], bonus);
                if (kq > -INFINITY) pat_take(blank, kq, q);
            }
        arc = pat_wave_best(arc);
        blank = pat_wave_best(blank);
        if (lane == 0) { s_arc[wave] = arc; s_blank[wave] = blank; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 0; w < nw; ++w) { pat_take(arc, s_arc[w].key, s_arc[w].id); pat_take(blank, s_blank[w].key, s_blank[w].id); }
            int kind = -1, idx = 0;                                                 // 0: on an arc, 1: on a state's blank
            if (arc.id >= 0) { kind = 0; idx = min(arc.id, A - 1); }
            if (blank.id >= 0 && (kind < 0 || blank.key > arc.key)) { kind = 1; idx = min(blank.id, S - 1); }
            const int item = kind == 0 ? idx : A + idx;
            const int len = kind < 0 ? -1 : pn[item];
            length[k] = len;
            score[k] = kind < 0 ? -INFINITY : pd[item];
            base[k] = bsum;
            int* out = labels + (long)k * Lcap;
            int pos = len - 1;
            for (int t = F - 1; t >= 0 && kind >= 0; --t) {                         // at most F frames, every pointer clamped
                const unsigned char* bp = bps + (size_t)t * N;
                const int2* rec = recs + (size_t)t * S;
                if (kind == 0) {
                    const int code = bp[idx];
                    if (code == 0) continue;                                        // the character goes on
                    if (pos >= 0 && pos < Lcap) out[pos] = pat_chan(tb, idx);
                    --pos;
                    const int src = min(max(tb.arc_src[idx], 0), S - 1);
                    if (code == 1) { kind = 1; idx = src; continue; }
                    const int x = code == 2 ? rec[src].x : rec[src].y;
                    if (x < 0) break;
                    idx = min(x, A - 1);
                } else {
                    if (bp[A + idx] == 0) continue;
                    const int x = rec[idx].x;
                    if (x < 0) break;
                    kind = 0;
                    idx = min(x, A - 1);
                }
            }
        }
        __syncthreads();                                                            // the slots and the workspace go to the next span
    }
}

__global__ __launch_bounds__(PAT_MAX_THREADS) void pattern_search_kernel(
    const float* __restrict__ E, PatTables tb, double bonus, double ln_min_conf, int* __restrict__ count, int* __restrict__ start,
    int* __restrict__ end, double* __restrict__ ratio, int* __restrict__ nchar, unsigned char* ws, long group_bytes, int B, int T, int H,
    int two_rows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pat_smem[];
    __shared__ int s_heavy[PAT_SMAX];
    __shared__ int s_nheavy;
    __shared__ float s_wmax[2][PAT_MAX_WAVES];
    __shared__ PatBest s_arc[PAT_MAX_WAVES];
    __shared__ PatBest s_pick;
    __shared__ int s_pick_start;
    __shared__ double s_lnm;
    double* lpbuf = reinterpret_cast<double*>(pat_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int S = tb.S, A = tb.A, V = tb.V, N = A + S;

    unsigned char* mine = ws + (size_t)blockIdx.x * group_bytes;
    double* d0 = reinterpret_cast<double*>(mine);
    double* d1 = d0 + N;
    double* rd = d1 + N;                                                            // r[t]: d, and its key (-inf: no candidate)
    double* rk = rd + T;
    int2* rec = reinterpret_cast<int2*>(rk + T);
    int* n0 = reinterpret_cast<int*>(rec + S);
    int* n1 = n0 + N;
    int* e0 = n1 + N;
    int* e1 = e0 + N;
    int* rn = e1 + N;
    int* rs = rn + T;

    pat_list_heavy(tb, s_heavy, &s_nheavy);
    const int nheavy = s_nheavy;
    PatBest none;
    none.key = -INFINITY; none.id = -1;

    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const float* eline = E + (long)b * T * V;
        double *pd = d0, *cd = d1;
        int *pn = n0, *cn = n1, *pe = e0, *ce = e1;
        for (int i = tid; i < N; i += blockDim.x) { pd[i] = -INFINITY; pn[i] = 0; pe[i] = -1; }
        pat_fill(eline, V, lpbuf, s_wmax[0]);
        __syncthreads();
        for (int t = 0; t <= T; ++t) {                                              // the reduce of step t also closes frame t - 1
            const int r = two_rows ? (t & 1) : 0;
            if (t < T) {
                if (two_rows && t + 1 < T) pat_fill(eline + (long)(t + 1) * V, V, lpbuf + (size_t)(r ^ 1) * V, s_wmax[r ^ 1]);
                if (tid == 0) s_lnm = pat_lnmax(s_wmax[r]);
            }
            PatBest arc = none;
            pat_reduce<true>(tb, pd, pn, bonus, rec, s_heavy, nheavy, arc);
            if (t > 0) {
                arc = pat_wave_best(arc);
                if (lane == 0) s_arc[wave] = arc;
            }
            __syncthreads();
            if (t > 0 && tid == 0) {                                                // r[t - 1]: the best arc into an accepting state
                for (int w = 0; w < nw; ++w) pat_take(arc, s_arc[w].key, s_arc[w].id);
                double d = -INFINITY, key = -INFINITY;
                int nc = 0, st = -1;
                if (arc.id >= 0) {
                    const int x = min(arc.id, A - 1);
                    d = pd[x]; nc = pn[x]; st = pe[x];
                    if (d > -INFINITY && d < INFINITY && d >= (double)nc * ln_min_conf) key = pat_key(d, nc, bonus);
                }
                rd[t - 1] = d; rk[t - 1] = key; rn[t - 1] = nc; rs[t - 1] = st;
            }
            if (t == T) break;
            pat_update<true>(tb, pd, pn, pe, cd, cn, ce, rec, lpbuf + (size_t)r * V, s_lnm, bonus, t, nullptr);
            __syncthreads();
            if (!two_rows && t + 1 < T) {
                pat_fill(eline + (long)(t + 1) * V, V, lpbuf, s_wmax[0]);
                __syncthreads();
            }
            double* sd = pd; pd = cd; cd = sd;
            int* sn = pn; pn = cn; cn = sn;
            int* se = pe; pe = ce; ce = se;
        }
        __syncthreads();                                                            // thread 0's r, before every thread reads its frames

        // the selection: from here a thread reads and writes rk only at its own frames (t = tid mod the workgroup)
        int found = 0;
        for (int h = 0; h < H; ++h) {
            PatBest best = none;
            for (int t = tid; t < T; t += blockDim.x) {
                const double v = rk[t];
                if (v > -INFINITY) pat_take(best, v, t);
            }
            best = pat_wave_best(best);
            if (lane == 0) s_arc[wave] = best;
            __syncthreads();
            if (tid == 0) {
                for (int w = 0; w < nw; ++w) pat_take(best, s_arc[w].key, s_arc[w].id);
                s_pick = best;
                s_pick_start = best.id >= 0 ? rs[best.id] : -1;
            }
            __syncthreads();
            const int bt = s_pick.id, ps = s_pick_start;
            if (bt < 0) break;                                                      // block-uniform
            if (tid == 0) {
                const long o = (long)b * H + h;
                start[o] = ps; end[o] = bt; ratio[o] = rd[bt]; nchar[o] = rn[bt];
            }
            ++found;
            for (int t = tid; t < T; t += blockDim.x)
                if (t >= ps && rs[t] <= bt) rk[t] = -INFINITY;                      // [start[t], t] overlaps [ps, bt]; the pick itself too
            __syncthreads();                                                        // s_arc and s_pick go to the next round
        }
        if (tid == 0) {
            count[b] = found;
            for (int h = found; h < H; ++h) {
                const long o = (long)b * H + h;
                start[o] = -1; end[o] = -1; ratio[o] = 0.0; nchar[o] = -1;
            }
        }
        __syncthreads();
    }
}

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_pattern_decode_workspace_bytes(int n, int n_states, int n_arcs, int Tmax)
{
    if (n <= 0 || n_states <= 0 || n_arcs < 0 || Tmax < 0) return 0;
    return pat_groups(n) * pat_decode_group_bytes(n_states, n_arcs, Tmax);
}

extern "C" long dtlr_pattern_search_workspace_bytes(int B, int n_states, int n_arcs, int T)
{
    if (B <= 0 || n_states <= 0 || n_arcs < 0 || T <= 0) return 0;
    return pat_groups(B) * pat_search_group_bytes(n_states, n_arcs, T);
}

extern "C" int dtlr_pattern_decode(const float* emissions, int B, int T, int V, const int* spans, int n, int Tmax, const int* arc_src,
                                   const int* arc_chan, const int* dst_start, const int* accept, int n_states, int n_arcs, double bonus,
                                   int* labels, int Lcap, int* length, double* score, double* base, void* workspace, void* stream)
{
    clear_stale_error();
    if (n < 0 || Tmax < 0 || n_arcs < 0) return DTLR_EINVAL;
    if (n_states > PAT_SMAX || n_arcs > PAT_AMAX || Lcap < Tmax) return DTLR_ESHAPE;
    if (n == 0) return DTLR_OK;
    if (B <= 0 || T <= 0 || V <= 0 || n_states < 1) return DTLR_EINVAL;
    if (V > PAT_VMAX) return DTLR_ESHAPE;
    if (Tmax > (1 << 29) || (long)B * T * V < 0 || (long)n * (Lcap > 0 ? Lcap : 1) < 0) return DTLR_ESHAPE;
    if (!emissions || !spans || !arc_src || !arc_chan || !dst_start || !accept || !length || !score || !base || !workspace) return DTLR_EINVAL;
    if (Lcap > 0 && !labels) return DTLR_EINVAL;
    if (!(bonus == bonus) || bonus == INFINITY || bonus == -INFINITY) return DTLR_EINVAL;
    const int two_rows = (size_t)V * 16 <= PAT_LDS_ROWS ? 1 : 0;
    const size_t lds = (size_t)V * 8 * (two_rows ? 2 : 1);
    PatTables tb;
    tb.arc_src = arc_src; tb.arc_chan = arc_chan; tb.dst_start = dst_start; tb.accept = accept; tb.S = n_states; tb.A = n_arcs; tb.V = V;
    return launch<pattern_decode_kernel>(dim3((unsigned)pat_groups(n)), dim3(pat_threads(n_states, n_arcs)), lds, (hipStream_t)stream,
                                         emissions, spans, tb, bonus, labels, length, score, base,
                                         reinterpret_cast<unsigned char*>(workspace), pat_decode_group_bytes(n_states, n_arcs, Tmax), B, T,
                                         n, Tmax, Lcap, two_rows);
}

extern "C" int dtlr_pattern_search(const float* emissions, int B, int T, int V, const int* arc_src, const int* arc_chan,
                                   const int* dst_start, const int* accept, int n_states, int n_arcs, double bonus, double ln_min_conf,
                                   int H, int* count, int* start, int* end, double* ratio, int* nchar, void* workspace, void* stream)
{
    clear_stale_error();
    if (B < 0 || n_arcs < 0) return DTLR_EINVAL;
    if (n_states > PAT_SMAX || n_arcs > PAT_AMAX || H < 1 || H > PAT_HMAX) return DTLR_ESHAPE;
    if (B == 0) return DTLR_OK;
    if (T <= 0 || V <= 0 || n_states < 1) return DTLR_EINVAL;
    if (V > PAT_VMAX) return DTLR_ESHAPE;
    if (T > (1 << 29) || (long)B * T * V < 0 || (long)B * H > 0x7fffffffL) return DTLR_ESHAPE;
    if (!emissions || !arc_src || !arc_chan || !dst_start || !accept || !count || !start || !end || !ratio || !nchar || !workspace) return DTLR_EINVAL;
    if (!(bonus == bonus) || bonus == INFINITY || bonus == -INFINITY || ln_min_conf != ln_min_conf) return DTLR_EINVAL;
    const int two_rows = (size_t)V * 16 <= PAT_LDS_ROWS ? 1 : 0;
    const size_t lds = (size_t)V * 8 * (two_rows ? 2 : 1);
    PatTables tb;
    tb.arc_src = arc_src; tb.arc_chan = arc_chan; tb.dst_start = dst_start; tb.accept = accept; tb.S = n_states; tb.A = n_arcs; tb.V = V;
    return launch<pattern_search_kernel>(dim3((unsigned)pat_groups(B)), dim3(pat_threads(n_states, n_arcs)), lds, (hipStream_t)stream,
                                         emissions, tb, bonus, ln_min_conf, count, start, end, ratio, nchar,
                                         reinterpret_cast<unsigned char*>(workspace), pat_search_group_bytes(n_states, n_arcs, T), B, T, H,
                                         two_rows);
}
