// Lexicon decoding over the CTC lattice: the best words of a dictionary for every word span of a batch.  The
// lexicon is a trie in breadth-first order; one max-product pass over the trie scores all its words at once, exactly (no pruning).
//   lexicon_decode_kernel  one workgroup per span, a fixed grid: workgroup g takes spans g, g + G, ...  Per frame the workgroup puts
//                          ln(max(E[t, :], 1e-30)) as fp64 into LDS (double-buffered when two rows fit, so that a frame costs one
//                          barrier), and every wave its channels' fp32 maximum, from which thread 0 sums the span's `base` in frame
//                          order.  The threads then sweep the nodes: a node's (nb, b) pair is 16 bytes of the workgroup's own slice
//                          of the caller's workspace, double-buffered, and a node reads last frame's pair of itself and of its parent
//                          only, so a sweep has no ordering hazard.  At frame t only nodes of depth <= t + 1 can be finite and nodes
//                          deeper than the span never matter: the breadth-first order makes both a prefix of the node array, and
//                          nothing outside it is read or written (a node that enters the prefix starts from -inf without a load).
//                          Selection: H rounds of a workgroup arg-max over the terminal nodes by (key, lower word id), each round
//                          taking the best record strictly behind the previous one, so nothing is marked or rewritten.
// Nothing here synchronises with the host.  The trie and the span table are device data: parents are clamped to [0, n), channels to
// [0, V), word ids to [-1, W), prefix ends to [1, n_nodes] and spans as dtlr_ctc_align clamps them, so a bad table gives a wrong
// record, never a fault.  No 16-bit type is involved: both builds export the same code.
#include "dtlr_common.h"
#include "../../include/dtlr_lexicon.h"

namespace dtlr {

constexpr int LEXD_THREADS = 1024;
constexpr int LEXD_WAVES = LEXD_THREADS / 64;
constexpr int LEXD_GRID = 2048;                      // workgroups at the most
constexpr int LEXD_HMAX = 8;
constexpr int LEXD_DMAX = 64;                        // the longest word
constexpr int LEXD_VMAX = 15360;                     // 8 V bytes of LDS: 120 KB
constexpr size_t LEXD_LDS_BUDGET = 150 * 1024;       // dynamic LDS of the 160 KB; the static arrays take part of the rest (below)

struct LexdPick {                                    // one candidate of the selection
    double key, score;
    int word;
};
// the kernel's static LDS (every wave's maximum of two frames, the waves' picks and the workgroup's pick) has to fit beside the rows
constexpr size_t LEXD_STATIC_LDS = 2 * LEXD_WAVES * sizeof(float) + (LEXD_WAVES + 1) * sizeof(LexdPick);
static_assert(LEXD_LDS_BUDGET + LEXD_STATIC_LDS + 64 <= 160 * 1024, "the rows of logs and the static arrays share 160 KB of LDS");
static_assert((size_t)LEXD_VMAX * 8 <= LEXD_LDS_BUDGET, "one row of logs of the widest vocabulary fits the budget");

// whether a comes before b: the larger key, on equal keys the lower word id; word < 0 is no candidate
__device__ __forceinline__ bool lexd_before(const LexdPick& a, const LexdPick& b)
{
    if (a.word < 0) return false;
    if (b.word < 0) return true;
    return a.key > b.key || (a.key == b.key && a.word < b.word);
}

__global__ __launch_bounds__(LEXD_THREADS) void lexicon_decode_kernel(
    const float* __restrict__ E, const int* __restrict__ spans, const int* __restrict__ parent, const int* __restrict__ chan,
    const int* __restrict__ node_word, const int* __restrict__ depth_start, const double* __restrict__ prior, int* __restrict__ count,
    int* __restrict__ word, double* __restrict__ score, double* __restrict__ base, double2* ws, int B, int T, int V, int n, int Tmax,
    int n_nodes, int max_depth, int W, int H, int two_rows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lexd_smem[];       // double lp[two_rows ? 2 : 1][V]
    __shared__ float s_wmax[2][LEXD_WAVES];                                         // every wave's maximum of a frame's channels
    __shared__ LexdPick s_pick[LEXD_WAVES];
    __shared__ LexdPick s_best;
    double* lpbuf = reinterpret_cast<double*>(lexd_smem);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double2* st0 = ws + (size_t)blockIdx.x * 2 * n_nodes;                            // this workgroup's two state arrays
    double2* st1 = st0 + n_nodes;

    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int b = min(max(spans[3 * k], 0), B - 1);
        const int t0 = min(max(spans[3 * k + 1], 0), T);
        const int t1 = min(max(spans[3 * k + 2], t0), T);
        const int F = min(t1 - t0, Tmax);                                           // block-uniform
        const float* eline = E + ((long)b * T + t0) * V;
        const int dcap = min(F, max_depth);                                         // nodes deeper than this never matter

        // frame t: lp[t, :] and the waves' maxima into row `r`
        auto fill = [&](int t, int r) {
            const float* e = eline + (long)t * V;
            double* lp = lpbuf + (size_t)r * V;
            float m = -INFINITY;
            for (int c = tid; c < V; c += LEXD_THREADS) {
                const float v = e[c];
                lp[c] = log(fmax((double)v, 1e-30));
                m = fmaxf(m, v);
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            if (lane == 0) s_wmax[r][wave] = m;
        };

        double bsum = 0.0;                                                          // thread 0's: sum of ln mx in frame order
        double2* prev = st0;
        double2* cur = st1;
        int nprev = 0;                                                              // nodes that hold a value of the last frame
        if (F > 0) fill(0, 0);
        __syncthreads();
        for (int t = 0; t < F; ++t) {
            const int r = two_rows ? (t & 1) : 0;
            if (two_rows && t + 1 < F) fill(t + 1, r ^ 1);
            const double* lp = lpbuf + (size_t)r * V;
            if (tid == 0) {
                float m = s_wmax[r][0];
#pragma unroll
                for (int w = 1; w < LEXD_WAVES; ++w) m = fmaxf(m, s_wmax[r][w]);
                bsum += log(fmax((double)m, 1e-30));
            }
            const int nact = max(nprev, min(max(depth_start[min(t + 2, dcap + 1)], 1), n_nodes));
            const double lp0 = lp[0];
            for (int i = tid; i < nact; i += LEXD_THREADS) {
                double2 me = make_double2(-INFINITY, -INFINITY);                    // (nb, b) of the last frame
                if (i < nprev) me = prev[i];
                double2 nx;
                if (i == 0) {                                                       // the root: b(root) = 0 before frame 0, never a character
                    nx.x = -INFINITY;
                    nx.y = (t == 0 ? 0.0 : me.y) + lp0;
                } else {
                    const int p = min(max(parent[i], 0), i - 1);
                    const int c = min(max(chan[i], 0), V - 1);
                    double2 pa = make_double2(-INFINITY, -INFINITY);
                    if (p < nprev) pa = prev[p];
                    if (p == 0) pa = make_double2(-INFINITY, t == 0 ? 0.0 : pa.y);
                    else if (min(max(chan[p], 0), V - 1) == c) pa.x = -INFINITY;    // a repeated character needs the blank between
                    nx.x = fmax(fmax(me.x, pa.y), pa.x) + lp[c];
                    nx.y = fmax(me.y, me.x) + lp0;
                }
                cur[i] = nx;
            }
            nprev = nact;
            __syncthreads();
            if (!two_rows && t + 1 < F) {
                fill(t + 1, 0);
                __syncthreads();
            }
            double2* sw = prev; prev = cur; cur = sw;
        }

        // selection: after the last frame the values are in prev[0, nprev)
        LexdPick last;
        last.key = INFINITY; last.score = 0.0; last.word = -1;
        int found = 0;
        for (int h = 0; h < H; ++h) {
            LexdPick best;
            best.key = -INFINITY; best.score = 0.0; best.word = -1;
            if (h == found) {                                                       // block-uniform: a round that found nothing ends the search
                for (int i = tid; i < nprev; i += LEXD_THREADS) {
                    const int w = min(max(node_word[i], -1), W - 1);
                    if (w < 0) continue;
                    const double2 v = prev[i];
                    LexdPick c;
                    c.score = fmax(v.x, v.y);
                    if (!(c.score > -INFINITY)) continue;
                    c.key = c.score + (prior ? prior[w] : 0.0);
                    if (c.key != c.key) c.key = -INFINITY;
                    c.word = w;
                    const bool behind = h == 0 || c.key < last.key || (c.key == last.key && w > last.word);
                    if (behind && lexd_before(c, best)) best = c;
                }
#pragma unroll
                for (int off = 32; off; off >>= 1) {
                    LexdPick o;
                    o.key = __shfl_xor(best.key, off);
                    o.score = __shfl_xor(best.score, off);
                    o.word = __shfl_xor(best.word, off);
                    if (lexd_before(o, best)) best = o;
                }
                if (lane == 0) s_pick[wave] = best;
                __syncthreads();
                if (tid == 0) {
                    LexdPick m = s_pick[0];
                    for (int w = 1; w < LEXD_WAVES; ++w)
                        if (lexd_before(s_pick[w], m)) m = s_pick[w];
                    s_best = m;
                }
                __syncthreads();
                best = s_best;
                if (best.word >= 0) { last = best; ++found; }
            }
            if (tid == 0) {
                word[(long)k * H + h] = best.word;
                score[(long)k * H + h] = best.word >= 0 ? best.score : 0.0;
            }
        }
        if (tid == 0) {
            count[k] = found;
            base[k] = bsum;
        }
        __syncthreads();                                                            // s_wmax, s_best and the state arrays go to the next span
    }
}

// the same arithmetic sizes the launch and answers the workspace query
static inline long lexd_groups(int n) { return n < LEXD_GRID ? n : LEXD_GRID; }

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_lexicon_decode_workspace_bytes(int n, int n_nodes, int Tmax)
{
    if (n <= 0 || n_nodes <= 0 || Tmax <= 0) return 0;
    return lexd_groups(n) * (long)n_nodes * 2 * (long)sizeof(double2);              // per workgroup: two arrays of (nb, b)
}

extern "C" int dtlr_lexicon_decode(const float* emissions, int B, int T, int V, const int* spans, int n, int Tmax, const int* parent,
                                   const int* chan, const int* node_word, const int* depth_start, int n_nodes, int max_depth, int W,
                                   const double* prior, int H, int* count, int* word, double* score, double* base, void* workspace,
                                   void* stream)
{
    clear_stale_error();
    if (n < 0 || Tmax < 0) return DTLR_EINVAL;
    if (H < 1 || H > LEXD_HMAX) return DTLR_ESHAPE;
    if (n == 0) return DTLR_OK;
    if (B <= 0 || T <= 0 || V <= 0 || n_nodes < 1 || W < 0) return DTLR_EINVAL;
    if (V > LEXD_VMAX || max_depth < 0 || max_depth > LEXD_DMAX) return DTLR_ESHAPE;
    if (Tmax > (1 << 29) || (long)B * T * V < 0 || (long)n * H > 0x7fffffffL) return DTLR_ESHAPE;
    if (!emissions || !spans || !parent || !chan || !node_word || !depth_start || !count || !word || !score || !base) return DTLR_EINVAL;
    if (Tmax > 0 && !workspace) return DTLR_EINVAL;
    const int two_rows = (size_t)V * 16 <= LEXD_LDS_BUDGET ? 1 : 0;
    const size_t lds = (size_t)V * 8 * (two_rows ? 2 : 1);
    return launch<lexicon_decode_kernel>(dim3((unsigned)lexd_groups(n)), dim3(LEXD_THREADS), lds, (hipStream_t)stream, emissions, spans,
                                         parent, chan, node_word, depth_start, prior, count, word, score, base,
                                         reinterpret_cast<double2*>(workspace), B, T, V, n, Tmax, n_nodes, max_depth, W, H, two_rows);
}
