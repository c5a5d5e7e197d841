// N-gram language model training on the device (include/dtlr_lm.h; the model: DESIGN.md section 18): interpolated modified Kneser-Ney
// from a token stream, over one sort of 64-bit keys (lm_sort.h).  gfx950 only.
//   lm_keys_kernel       position i -> the key of the `order` tokens from i on, first token in the most significant bits in use, pad
//                        (0) behind the line's </s>.
//   (dtlr_sort_u64)      the keys in ascending order: the n-grams of EVERY order are then contiguous, an n-gram being the first n
//                        tokens of a key whose n-th token is not pad; pad sorts first, so inside a group of equal (n - 1)-prefixes the
//                        keys that are too short for order n come before all others.
//   lm_heads_kernel      per tile of SORT_TILE positions and per order, the number of group heads: positions whose key is long enough
//                        and differs from its predecessor inside the first n tokens (common prefix = clz(xor) / bits).  One integer
//                        add per workgroup and order gives the totals (dtlr_lm_count); the [order][tile] table, scanned as one row,
//                        gives every head its row in the tables of all orders at once (dtlr_lm_compact).
//   lm_compact_kernel    a thread walks 16 consecutive positions; a head writes its n-gram and subtracts its position from the row's
//                        count, the first position of the next group adds its own: c_n = end - start, two integer atomics a row.
//   estimate             adjusted counts (each (n + 1)-gram finds its tail among the n-grams by binary search and adds 1), the counts of
//                        counts t_1..t_4 (a reduction per workgroup, one integer add each), the discounts (one thread), then order by
//                        order: a thread per context finds its children (contiguous: a binary search), sums den and N_1..N_3, writes the
//                        context's back-off and every child's probability; p_{n-1} of the child's tail is again a binary search.
// All sums over n-grams are integer; every fp64 value is computed by one thread from integers and from fp64 values of the order below,
// in a fixed order of operations: two runs give the same bits.  No float atomics.  Nothing here synchronises with the host.
#include "lm_sort.h"

namespace dtlr {

constexpr int LM_THREADS = 256;
constexpr int LM_PER_THREAD = 16;                                   // positions a thread walks in lm_heads / lm_compact
static_assert(LM_THREADS * LM_PER_THREAD == SORT_TILE, "the tiles of the compaction are the sort's");

__device__ __forceinline__ u64 low_mask(int b) { return b >= 64 ? ~0ull : (1ull << b) - 1ull; }

// tokens of `key` that are not pad (pad is trailing only)
__device__ __forceinline__ int key_len(u64 key, int order, int bits)
{
    int len = order;
    while (len > 0 && ((key >> ((order - len) * bits)) & low_mask(bits)) == 0) --len;
    return len;
}

// leading tokens that two keys share
__device__ __forceinline__ int common_prefix(u64 a, u64 b, int order, int bits)
{
    const u64 x = a ^ b;
    if (x == 0) return order;
    return (__clzll((long long)x) - (64 - order * bits)) / bits;
}

__global__ __launch_bounds__(LM_THREADS) void lm_keys_kernel(const int* __restrict__ tokens, long n, int order, int bits,
                                                             u64* __restrict__ keys)
{
    const long i = (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 mask = low_mask(bits);
    u64 key = 0;
    bool open = true;
    for (int j = 0; j < order; ++j) {
        u64 t = 0;
        if (open && i + j < n) t = (u64)(unsigned)tokens[i + j] & mask;
        if (t == 0) open = false;
        key = (key << bits) | t;
        if (t == DTLR_LM_EOS) open = false;
    }
    keys[i] = key;
}

__global__ __launch_bounds__(LM_THREADS) void lm_fill_kernel(long* __restrict__ p, long count, long value)
{
    const long i = (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i < count) p[i] = value;
}

// (len, common prefix with the key before) of position i in 0..n ; position n is the end: no key, a boundary of every order
__device__ __forceinline__ void position_of(const u64* __restrict__ keys, long n, long i, int order, int bits, u64* key, int* len, int* cpl)
{
    *key = 0; *len = 0; *cpl = 0;
    if (i >= n) return;
    *key = keys[i];
    *len = key_len(*key, order, bits);
    if (i > 0) *cpl = common_prefix(*key, keys[i - 1], order, bits);
}

__global__ __launch_bounds__(LM_THREADS) void lm_heads_kernel(const u64* __restrict__ keys, long n, int order, int bits,
                                                              unsigned* __restrict__ table, int tiles, unsigned long long* __restrict__ totals)
{
    __shared__ unsigned sum[DTLR_LM_MAX_ORDER];
    if (threadIdx.x < DTLR_LM_MAX_ORDER) sum[threadIdx.x] = 0;
    __syncthreads();
    unsigned mine[DTLR_LM_MAX_ORDER] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long first = (long)blockIdx.x * SORT_TILE + (long)threadIdx.x * LM_PER_THREAD;
    for (int j = 0; j < LM_PER_THREAD; ++j) {
        u64 key; int len, cpl;
        position_of(keys, n, first + j, order, bits, &key, &len, &cpl);
#pragma unroll
        for (int k = 1; k <= DTLR_LM_MAX_ORDER; ++k) mine[k - 1] += (k <= len && cpl < k) ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < DTLR_LM_MAX_ORDER; ++k) {
        const unsigned w = (unsigned)wave_sum_i((int)mine[k]);
        if ((threadIdx.x & (kWave - 1)) == 0 && w) atomicAdd(&sum[k], w);
    }
    __syncthreads();
    if ((int)threadIdx.x < order) {
        if (table) table[(size_t)threadIdx.x * tiles + blockIdx.x] = sum[threadIdx.x];
        if (totals && sum[threadIdx.x]) atomicAdd(&totals[threadIdx.x], (unsigned long long)sum[threadIdx.x]);
    }
}

__global__ __launch_bounds__(LM_THREADS) void lm_compact_kernel(const u64* __restrict__ keys, long n, int order, int bits,
                                                                const unsigned* __restrict__ table, const unsigned* __restrict__ sums,
                                                                int tiles, long total, u64* __restrict__ grams,
                                                                unsigned long long* __restrict__ cnt)
{
    __shared__ unsigned part[SORT_WAVES + 1];
    const long first = (long)blockIdx.x * SORT_TILE + (long)threadIdx.x * LM_PER_THREAD;
    u64 key[LM_PER_THREAD];
    unsigned char len[LM_PER_THREAD], cpl[LM_PER_THREAD];
    int len_before = 0;                                             // of the key in front of this thread's first position
    if (first > 0 && first - 1 < n) len_before = key_len(keys[first - 1], order, bits);
#pragma unroll
    for (int j = 0; j < LM_PER_THREAD; ++j) {
        int l, c;
        position_of(keys, n, first + j, order, bits, &key[j], &l, &c);
        len[j] = (unsigned char)l;
        cpl[j] = (unsigned char)c;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && 2 < total) {         // the <unk> row of order 1
        grams[2] = DTLR_LM_UNK;
        cnt[2] = 0;
    }
    for (int k = 1; k <= order; ++k) {
        unsigned mine = 0;
#pragma unroll
        for (int j = 0; j < LM_PER_THREAD; ++j) mine += (k <= len[j] && cpl[j] < k) ? 1u : 0u;
        unsigned all;
        const size_t at = (size_t)(k - 1) * tiles + blockIdx.x;
        // the row of the first head of this thread: heads of lower orders and of earlier tiles, then of earlier threads
        long row = (long)table[at] + sums[at / SCAN_CHUNK] + block_scan_excl(mine, part, &all);
        const long row0 = k == 1 ? 0 : 1;                           // orders above 1 lie behind the <unk> row ; order 1 steps over it
        int prev = len_before;
#pragma unroll
        for (int j = 0; j < LM_PER_THREAD; ++j) {
            const long i = first + j;
            if (i <= n && cpl[j] < k) {                             // a boundary of order k
                if (i > 0 && prev >= k) {                           // it ends the group of the key before: row - 1
                    long r = row - 1 + row0;
                    if (k == 1 && r >= 2) ++r;
                    if (r >= 0 && r < total) atomicAdd(&cnt[r], (unsigned long long)i);
                }
                if (k <= len[j]) {                                  // and begins one
                    long r = row + row0;
                    if (k == 1 && r >= 2) ++r;
                    if (r >= 0 && r < total) {
                        grams[r] = key[j] >> ((order - k) * bits);
                        atomicAdd(&cnt[r], (unsigned long long)(-i));
                    }
                    ++row;
                }
            }
            prev = len[j];
        }
    }
}

// ---- the estimator -------------------------------------------------------------------------------------------------------------
// the workspace: per order 64 bytes, then 64 bytes of the unigram context
struct LmOrderStats { long long t[4]; double D[3]; long long fallback; };
struct LmUnigram { long long den, nk[3]; double b; long long pad[3]; };
static_assert(sizeof(LmOrderStats) == 64 && sizeof(LmUnigram) == 64, "dtlr_lm_estimate_workspace_bytes");

// the row (inside its order) of `g` among grams[lo, hi), or -1
__device__ __forceinline__ long find_gram(const u64* __restrict__ grams, long lo, long hi, u64 g)
{
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        const u64 v = grams[mid];
        if (v == g) return mid;
        if (v < g) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// the first row of grams[lo, hi) that is >= g
__device__ __forceinline__ long lower_bound(const u64* __restrict__ grams, long lo, long hi, u64 g)
{
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (grams[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// which order row i belongs to (1-based) ; 0 for a row outside the tables
__device__ __forceinline__ int order_of(const long* __restrict__ offs, int order, long i)
{
    for (int k = 1; k <= order; ++k)
        if (i < offs[k]) return i >= offs[0] ? k : 0;
    return 0;
}

// a_n before the left extensions are counted: c_n for the highest order and for an n-gram that begins with <s>, else 0 ; the
// unigram <s> is never predicted: 0.  Also clears the statistics.
__global__ __launch_bounds__(LM_THREADS) void lm_adjust_init_kernel(const u64* __restrict__ grams, const long* __restrict__ cnt,
                                                                    const long* __restrict__ offs, int order, int bits, long total,
                                                                    long* __restrict__ adj, int* __restrict__ flags, long long* __restrict__ ws)
{
    const long i = (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i < 8 * ((long)order + 1)) ws[i] = 0;
    if (i < 2) flags[i] = 0;
    if (i >= total) return;
    const int k = order_of(offs, order, i);
    if (k == 0) { adj[i] = 0; return; }
    const u64 first = (grams[i] >> ((k - 1) * bits)) & low_mask(bits);
    long a = 0;
    if (k == order || first == DTLR_LM_BOS) a = cnt[i];
    if (k == 1 && first == DTLR_LM_BOS) a = 0;
    adj[i] = a;
}

// every (k + 1)-gram adds 1 to its tail, the k-gram without its first word, unless the tail begins with <s> (it never does)
__global__ __launch_bounds__(LM_THREADS) void lm_extend_kernel(const u64* __restrict__ grams, const long* __restrict__ offs, int order,
                                                               int bits, long total, unsigned long long* __restrict__ adj,
                                                               int* __restrict__ flags)
{
    const long i = (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i >= total) return;
    const int k1 = order_of(offs, order, i);                        // this row's order, k + 1
    if (k1 < 2) return;
    const int k = k1 - 1;
    const u64 tail = grams[i] & low_mask(k * bits);
    const long at = find_gram(grams, offs[k - 1], offs[k], tail);
    if (at < 0) { atomicOr(&flags[1], 1); return; }
    if (k < order && ((tail >> ((k - 1) * bits)) & low_mask(bits)) != DTLR_LM_BOS) atomicAdd(&adj[at], 1ull);
}

// t_1..t_4 of every order
__global__ __launch_bounds__(LM_THREADS) void lm_count_of_counts_kernel(const long* __restrict__ adj, const long* __restrict__ offs,
                                                                        int order, long total, LmOrderStats* __restrict__ stats)
{
    __shared__ unsigned sum[DTLR_LM_MAX_ORDER][4];
    if (threadIdx.x < DTLR_LM_MAX_ORDER * 4) (&sum[0][0])[threadIdx.x] = 0;
    __syncthreads();
    const long i = (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i < total) {
        const int k = order_of(offs, order, i);
        const long a = adj[i];
        if (k > 0 && a >= 1 && a <= 4) atomicAdd(&sum[k - 1][a - 1], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < order * 4 && (&sum[0][0])[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(&stats[threadIdx.x >> 2].t[threadIdx.x & 3]),
                  (unsigned long long)(&sum[0][0])[threadIdx.x]);
}

__global__ void lm_discounts_kernel(int order, LmOrderStats* __restrict__ stats, int* __restrict__ flags)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int mask = 0;
    for (int k = 0; k < order; ++k) {
        const double t1 = (double)stats[k].t[0], t2 = (double)stats[k].t[1], t3 = (double)stats[k].t[2], t4 = (double)stats[k].t[3];
        bool ok = stats[k].t[0] > 0 && stats[k].t[1] > 0 && stats[k].t[2] > 0 && stats[k].t[3] > 0;
        double D[3] = {0.5, 1.0, 1.5};
        if (ok) {
            const double Y = t1 / (t1 + 2.0 * t2);
            D[0] = 1.0 - 2.0 * Y * t2 / t1;
            D[1] = 2.0 - 3.0 * Y * t3 / t2;
            D[2] = 3.0 - 4.0 * Y * t4 / t3;
            for (int j = 0; j < 3; ++j) ok = ok && D[j] >= 0.0 && D[j] <= (double)(j + 1);
            if (!ok) { D[0] = 0.5; D[1] = 1.0; D[2] = 1.5; }
        }
        stats[k].D[0] = D[0]; stats[k].D[1] = D[1]; stats[k].D[2] = D[2];
        stats[k].fallback = ok ? 0 : 1;
        if (!ok) mask |= 1 << k;
    }
    flags[0] = mask;
}

__device__ __forceinline__ double backoff_mass(const double* D, long long n1, long long n2, long long n3, long long den)
{
    return (D[0] * (double)n1 + D[1] * (double)n2 + D[2] * (double)n3) / (double)den;
}

__device__ __forceinline__ double discounted(const double* D, long a)
{
    return a <= 0 ? 0.0 : (double)a - D[(a < 3 ? a : 3) - 1];
}

// the one context of order 1: den_1, N_1..N_3 over all unigrams (one workgroup, integer sums), its back-off mass
__global__ __launch_bounds__(LM_THREADS) void lm_unigram_context_kernel(const long* __restrict__ adj, const long* __restrict__ offs,
                                                                        const LmOrderStats* __restrict__ stats, LmUnigram* __restrict__ uni)
{
    __shared__ unsigned long long sum[4];
    if (threadIdx.x < 4) sum[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long mine[4] = {0, 0, 0, 0};
    for (long i = offs[0] + threadIdx.x; i < offs[1]; i += LM_THREADS) {
        const long a = adj[i];
        if (a > 0) {
            mine[0] += (unsigned long long)a;
            mine[a < 3 ? a : 3] += 1;
        }
    }
    for (int j = 0; j < 4; ++j) if (mine[j]) atomicAdd(&sum[j], mine[j]);
    __syncthreads();
    if (threadIdx.x == 0) {
        uni->den = (long long)sum[0];
        uni->nk[0] = (long long)sum[1]; uni->nk[1] = (long long)sum[2]; uni->nk[2] = (long long)sum[3];
        uni->b = sum[0] ? backoff_mass(stats[0].D, (long long)sum[1], (long long)sum[2], (long long)sum[3], (long long)sum[0]) : 0.0;
    }
}

// p_1(w) = (a - D(a)) / den + b / |V| for every unigram but <s> (p = 0 here, -99 in the table) ; |V| = the rows without <s>
__global__ __launch_bounds__(LM_THREADS) void lm_unigram_kernel(const u64* __restrict__ grams, const long* __restrict__ adj,
                                                                const long* __restrict__ offs, const LmOrderStats* __restrict__ stats,
                                                                const LmUnigram* __restrict__ uni, double* __restrict__ p)
{
    const long i = offs[0] + (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i >= offs[1]) return;
    const double V = (double)(offs[1] - offs[0] - 1);
    if (grams[i] == DTLR_LM_BOS || uni->den <= 0) { p[i] = 0.0; return; }
    p[i] = discounted(stats[0].D, adj[i]) / (double)uni->den + uni->b / V;
}

// order k >= 2: a thread per (k - 1)-gram, the context.  Its children are the k-grams that begin with it: contiguous.
__global__ __launch_bounds__(LM_THREADS) void lm_order_kernel(const u64* __restrict__ grams, const long* __restrict__ adj,
                                                              const long* __restrict__ offs, int k, int bits,
                                                              const LmOrderStats* __restrict__ stats, double* __restrict__ p,
                                                              double* __restrict__ bo, int* __restrict__ flags)
{
    const long c = offs[k - 2] + (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (c >= offs[k - 1]) return;
    const u64 ctx = grams[c];
    const long lo = lower_bound(grams, offs[k - 1], offs[k], ctx << bits);
    const long hi = lower_bound(grams, lo, offs[k], (ctx << bits) | low_mask(bits));      // a last word of all ones is no id: < suffices
    long end = hi;
    if (end < offs[k] && grams[end] == ((ctx << bits) | low_mask(bits))) ++end;
    long long den = 0, nk[3] = {0, 0, 0};
    for (long i = lo; i < end; ++i) {
        const long a = adj[i];
        if (a > 0) {
            den += a;
            nk[(a < 3 ? a : 3) - 1] += 1;
        }
    }
    if (den <= 0) { bo[c] = 0.0; for (long i = lo; i < end; ++i) p[i] = 0.0; return; }
    const double* D = stats[k - 1].D;
    const double b = backoff_mass(D, nk[0], nk[1], nk[2], den);
    bo[c] = log10(b);
    const u64 tail_mask = low_mask((k - 1) * bits);
    for (long i = lo; i < end; ++i) {
        const long at = find_gram(grams, offs[k - 2], offs[k - 1], grams[i] & tail_mask);
        double lower = 0.0;
        if (at < 0) atomicOr(&flags[1], 1); else lower = p[at];
        p[i] = discounted(D, adj[i]) / (double)den + b * lower;
    }
}

// p -> log10 p (-99 for the unigram <s>), the back-off of the highest order (0), the ids
__global__ __launch_bounds__(LM_THREADS) void lm_finish_kernel(const u64* __restrict__ grams, const long* __restrict__ offs, int order,
                                                               int bits, long total, int* __restrict__ ids, double* __restrict__ p,
                                                               double* __restrict__ bo)
{
    const long i = (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (i >= total) return;
    const int k = order_of(offs, order, i);
    if (k == 0) return;
    long at = 0;                                                    // where order k's ids begin
    for (int j = 1; j < k; ++j) at += (offs[j] - offs[j - 1]) * j;
    at += (i - offs[k - 1]) * k;
    const u64 g = grams[i];
    for (int j = 0; j < k; ++j) ids[at + j] = (int)((g >> ((k - 1 - j) * bits)) & low_mask(bits));
    if (k == order) bo[i] = 0.0;
    p[i] = (k == 1 && g == DTLR_LM_BOS) ? -99.0 : log10(p[i]);
}

static inline bool lm_shape_ok(int order, int bits)
{
    return order >= 1 && order <= DTLR_LM_MAX_ORDER && bits >= 2 && bits <= 32 && order * bits <= 64;
}

static inline unsigned blocks_for(long n) { return (unsigned)((n + LM_THREADS - 1) / LM_THREADS); }
constexpr long LM_MAX_ROWS = (1L << 31) - 1;

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_sort_u64_workspace_bytes(long n) { return sort_workspace_bytes(n); }

extern "C" int dtlr_sort_u64(const void* keys_in, void* keys_out, long n, int key_bits, void* workspace, long workspace_bytes, void* stream)
{
    clear_stale_error();
    if (n < 0) return DTLR_EINVAL;
    if (key_bits < 1 || key_bits > 64 || n > LM_MAX_ROWS) return DTLR_ESHAPE;
    if (workspace_bytes < sort_workspace_bytes(n)) return DTLR_ESHAPE;
    if (n == 0) return DTLR_OK;
    if (!keys_in || !keys_out || !workspace || keys_in == keys_out) return DTLR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (int)sort_tiles(n);
    const long m = 256L * tiles;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    u64* other = reinterpret_cast<u64*>(ws);
    unsigned* table = reinterpret_cast<unsigned*>(ws + round_up(8 * n, 256));
    unsigned* sums = table + m;
    const int passes = (key_bits + 7) / 8;
    const u64* src = reinterpret_cast<const u64*>(keys_in);
    u64* out = reinterpret_cast<u64*>(keys_out);
    for (int pass = 0; pass < passes; ++pass) {
        u64* dst = ((passes - pass) & 1) ? out : other;             // the last pass writes keys_out
        int rc = launch<sort_hist_kernel>(dim3((unsigned)tiles), dim3(SORT_THREADS), 0, st, src, n, 8 * pass, table, tiles);
        if (rc != DTLR_OK) return rc;
        rc = scan_table(table, m, sums, st);
        if (rc != DTLR_OK) return rc;
        rc = launch<sort_scatter_kernel>(dim3((unsigned)tiles), dim3(SORT_THREADS), 0, st, src, dst, n, 8 * pass,
                                         (const unsigned*)table, (const unsigned*)sums, tiles);
        if (rc != DTLR_OK) return rc;
        src = dst;
    }
    return DTLR_OK;
}

extern "C" int dtlr_lm_keys(const int* tokens, long n, int order, int bits, void* keys, void* stream)
{
    clear_stale_error();
    if (n < 0) return DTLR_EINVAL;
    if (!lm_shape_ok(order, bits) || n > LM_MAX_ROWS) return DTLR_ESHAPE;
    if (n == 0) return DTLR_OK;
    if (!tokens || !keys) return DTLR_EINVAL;
    return launch<lm_keys_kernel>(dim3(blocks_for(n)), dim3(LM_THREADS), 0, (hipStream_t)stream, tokens, n, order, bits,
                                  reinterpret_cast<u64*>(keys));
}

extern "C" int dtlr_lm_count(const void* keys, long n, int order, int bits, long* counts, void* stream)
{
    clear_stale_error();
    if (n < 0) return DTLR_EINVAL;
    if (!lm_shape_ok(order, bits) || n > LM_MAX_ROWS) return DTLR_ESHAPE;
    if (!counts || (n > 0 && !keys)) return DTLR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch<lm_fill_kernel>(dim3(1), dim3(LM_THREADS), 0, st, counts, (long)order, 0L);
    if (rc != DTLR_OK || n == 0) return rc;
    const int tiles = (int)sort_tiles(n + 1);
    return launch<lm_heads_kernel>(dim3((unsigned)tiles), dim3(LM_THREADS), 0, st, reinterpret_cast<const u64*>(keys), n, order, bits,
                                   (unsigned*)nullptr, tiles, reinterpret_cast<unsigned long long*>(counts));
}

extern "C" long dtlr_lm_compact_workspace_bytes(long n, int order)
{
    if (n < 0 || order < 1) return 0;
    const long t = sort_tiles(n + 1);
    return round_up(4 * order * t, 256) + round_up(4 * scan_chunks(order * t), 256);
}

extern "C" int dtlr_lm_compact(const void* keys, long n, int order, int bits, long total, void* grams, long* cnt, void* workspace,
                               long workspace_bytes, void* stream)
{
    clear_stale_error();
    if (n < 0 || total < 0) return DTLR_EINVAL;
    if (!lm_shape_ok(order, bits) || n > LM_MAX_ROWS || total > LM_MAX_ROWS) return DTLR_ESHAPE;      // rows are counted in 32 bits
    if (workspace_bytes < dtlr_lm_compact_workspace_bytes(n, order)) return DTLR_ESHAPE;
    if (total == 0) return DTLR_OK;
    if (!grams || !cnt || !workspace || (n > 0 && !keys)) return DTLR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (int)sort_tiles(n + 1);
    const long m = (long)order * tiles;
    unsigned* table = reinterpret_cast<unsigned*>(workspace);
    unsigned* sums = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(workspace) + round_up(4 * m, 256));
    const u64* k = reinterpret_cast<const u64*>(keys);
    int rc = launch<lm_fill_kernel>(dim3(blocks_for(total)), dim3(LM_THREADS), 0, st, cnt, total, 0L);
    if (rc != DTLR_OK) return rc;
    rc = launch<lm_heads_kernel>(dim3((unsigned)tiles), dim3(LM_THREADS), 0, st, k, n, order, bits, table, tiles,
                                 (unsigned long long*)nullptr);
    if (rc != DTLR_OK) return rc;
    rc = scan_table(table, m, sums, st);
    if (rc != DTLR_OK) return rc;
    return launch<lm_compact_kernel>(dim3((unsigned)tiles), dim3(LM_THREADS), 0, st, k, n, order, bits, (const unsigned*)table,
                                     (const unsigned*)sums, tiles, total, reinterpret_cast<u64*>(grams),
                                     reinterpret_cast<unsigned long long*>(cnt));
}

extern "C" long dtlr_lm_estimate_workspace_bytes(int order)
{
    return order < 1 ? 0 : 64L * (order + 1);
}

extern "C" int dtlr_lm_estimate(const void* grams, const long* cnt, const long* offs, int order, int bits, long total, long* adj,
                                int* ids, double* logp, double* bo, int* flags, void* workspace, long workspace_bytes, void* stream)
{
    clear_stale_error();
    if (total < 0) return DTLR_EINVAL;
    if (!lm_shape_ok(order, bits) || total > LM_MAX_ROWS) return DTLR_ESHAPE;
    if (workspace_bytes < dtlr_lm_estimate_workspace_bytes(order)) return DTLR_ESHAPE;
    if (!grams || !cnt || !offs || !adj || !ids || !logp || !bo || !flags || !workspace) return DTLR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const u64* g = reinterpret_cast<const u64*>(grams);
    LmOrderStats* stats = reinterpret_cast<LmOrderStats*>(workspace);
    LmUnigram* uni = reinterpret_cast<LmUnigram*>(stats + order);
    const dim3 grid(blocks_for(total > 128 ? total : 128)), block(LM_THREADS);      // at least the threads that clear the statistics
    int rc = launch<lm_adjust_init_kernel>(grid, block, 0, st, g, cnt, offs, order, bits, total, adj, flags,
                                           reinterpret_cast<long long*>(workspace));
    if (rc != DTLR_OK) return rc;
    rc = launch<lm_extend_kernel>(grid, block, 0, st, g, offs, order, bits, total, reinterpret_cast<unsigned long long*>(adj), flags);
    if (rc != DTLR_OK) return rc;
    rc = launch<lm_count_of_counts_kernel>(grid, block, 0, st, (const long*)adj, offs, order, total, stats);
    if (rc != DTLR_OK) return rc;
    rc = launch<lm_discounts_kernel>(dim3(1), dim3(kWave), 0, st, order, stats, flags);
    if (rc != DTLR_OK) return rc;
    rc = launch<lm_unigram_context_kernel>(dim3(1), block, 0, st, (const long*)adj, offs, (const LmOrderStats*)stats, uni);
    if (rc != DTLR_OK) return rc;
    rc = launch<lm_unigram_kernel>(grid, block, 0, st, g, (const long*)adj, offs, (const LmOrderStats*)stats, (const LmUnigram*)uni, logp);
    if (rc != DTLR_OK) return rc;
    for (int k = 2; k <= order; ++k) {
        rc = launch<lm_order_kernel>(grid, block, 0, st, g, (const long*)adj, offs, k, bits, (const LmOrderStats*)stats, logp, bo, flags);
        if (rc != DTLR_OK) return rc;
    }
    return launch<lm_finish_kernel>(grid, block, 0, st, g, offs, order, bits, total, ids, logp, bo);
}
