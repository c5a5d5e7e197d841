// Device-wide radix sort of 64-bit keys (include/dtlr_lm.h: dtlr_sort_u64).  gfx950 only: wave = 64 lanes.
// Least significant digit first, 8 bits a pass, over the digits in use.  A pass is four launches:
//   sort_hist_kernel     one workgroup per tile of SORT_TILE keys: the tile's digit histogram, counted in LDS (integer atomics), stored
//                        as column `tile` of the [256][tiles] table.
//   scan_chunks_kernel   the table as one row of 256 * tiles counters, in chunks of SCAN_CHUNK: every counter becomes the sum of the
//                        counters before it in its chunk, the chunk's total goes to sums[chunk].
//   scan_sums_kernel     one workgroup: sums[] becomes its exclusive scan.  table[d][t] + sums[chunk of (d, t)] is then where the first
//                        key of tile t with digit d lands.
//   sort_scatter_kernel  one workgroup (4 waves) per tile.  Wave w owns keys [w * 64 * SORT_KPT, (w + 1) * 64 * SORT_KPT) of the tile and
//                        takes them 64 at a time, a key a lane.  The lanes that hold the same digit find each other by eight ballots
//                        (one per bit of the digit); a key's rank among them is the number of lower lanes.  The lowest of them adds their
//                        number to the wave's own counter of that digit in LDS and hands the old value round: the rank of a key inside
//                        its wave's keys is old value + rank among the lanes, in key order, so the pass is stable.  Then thread d turns
//                        the four wave counters of digit d into bases (table + sums + the waves before), and every key goes to
//                        base[wave][digit] + rank.  The counters are private to a wave and the table is filled by plain stores: no
//                        result depends on the order in which workgroups or waves run.
// Nothing here synchronises with the host.
#pragma once
#include "dtlr_common.h"
#include "../../include/dtlr_lm.h"

namespace dtlr {

constexpr int SORT_THREADS = 256;
constexpr int SORT_WAVES = SORT_THREADS / kWave;
constexpr int SORT_KPT = 16;                                       // keys a lane
constexpr int SORT_TILE = SORT_THREADS * SORT_KPT;
constexpr int SCAN_CHUNK = 4096;                                   // counters one workgroup scans: 16 a thread
static_assert(SORT_TILE == DTLR_SORT_TILE, "the header states the tile");
static_assert(SCAN_CHUNK == SORT_THREADS * 16, "scan_chunks_kernel: 16 counters a thread");

typedef unsigned long long u64;

static inline long round_up(long v, long a) { return (v + a - 1) / a * a; }

// exclusive scan of one value a thread over the 256 threads of a workgroup ; *total: the sum.  `part` holds SORT_WAVES + 1 words of
// LDS.  Ends with a barrier in front of the read of part[], begins with one behind the last read: it can be called in a loop.
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned* part, unsigned* total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += up;
    }
    __syncthreads();                                               // part[] of the call before has been read
    if (lane == kWave - 1) part[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
        const unsigned p = part[w];
        if (w < wave) before += p;
        all += p;
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(const u64* __restrict__ keys, long n, int shift,
                                                                 unsigned* __restrict__ table, int tiles)
{
    __shared__ unsigned hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const long base = (long)blockIdx.x * SORT_TILE;
#pragma unroll 4
    for (int r = 0; r < SORT_KPT; ++r) {
        const long i = base + r * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&hist[(unsigned)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(SORT_THREADS) void scan_chunks_kernel(unsigned* __restrict__ table, long m, unsigned* __restrict__ sums)
{
    __shared__ unsigned part[SORT_WAVES + 1];
    const long first = (long)blockIdx.x * SCAN_CHUNK + threadIdx.x * 16;
    unsigned v[16], mine = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        v[j] = first + j < m ? table[first + j] : 0u;
        mine += v[j];
    }
    unsigned total;
    unsigned run = block_scan_excl(mine, part, &total);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (first + j < m) table[first + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(SORT_THREADS) void scan_sums_kernel(unsigned* __restrict__ sums, int chunks)
{
    __shared__ unsigned part[SORT_WAVES + 1];
    unsigned carry = 0;
    for (int c0 = 0; c0 < chunks; c0 += SORT_THREADS) {
        const int c = c0 + threadIdx.x;
        const unsigned v = c < chunks ? sums[c] : 0u;
        unsigned total;
        const unsigned ex = block_scan_excl(v, part, &total);
        if (c < chunks) sums[c] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(const u64* __restrict__ in, u64* __restrict__ out, long n, int shift,
                                                                    const unsigned* __restrict__ table,
                                                                    const unsigned* __restrict__ sums, int tiles)
{
    __shared__ unsigned cnt[SORT_WAVES][256];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) cnt[w][threadIdx.x] = 0;
    __syncthreads();

    const long base = (long)blockIdx.x * SORT_TILE + (long)wave * (kWave * SORT_KPT);
    const u64 below = (1ull << lane) - 1ull;                        // the lanes before this one
    u64 key[SORT_KPT];
    unsigned rank[SORT_KPT];
#pragma unroll
    for (int r = 0; r < SORT_KPT; ++r) {
        const long i = base + r * kWave + lane;
        const bool valid = i < n;
        key[r] = valid ? in[i] : 0ull;
        const unsigned d = (unsigned)(key[r] >> shift) & 255u;
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 has = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? has : ~has;
        }
        unsigned old = 0;
        const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
        if (valid && lane == leader) old = atomicAdd(&cnt[wave][d], (unsigned)__popcll(peers));
        old = __shfl(old, leader, kWave);
        rank[r] = old + (unsigned)__popcll(peers & below);
    }
    __syncthreads();
    {                                                               // thread d: the four counters of digit d become bases
        const size_t at = (size_t)threadIdx.x * tiles + blockIdx.x;
        unsigned run = table[at] + sums[at / SCAN_CHUNK];
#pragma unroll
        for (int w = 0; w < SORT_WAVES; ++w) {
            const unsigned c = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_KPT; ++r) {
        const long i = base + r * kWave + lane;
        if (i < n) {
            const unsigned d = (unsigned)(key[r] >> shift) & 255u;
            const long to = (long)cnt[wave][d] + rank[r];
            if (to < n) out[to] = key[r];                           // holds by construction ; a guard costs nothing here
        }
    }
}

static inline long sort_tiles(long n) { return (n + SORT_TILE - 1) / SORT_TILE; }
static inline long scan_chunks(long m) { return (m + SCAN_CHUNK - 1) / SCAN_CHUNK; }

static inline long sort_workspace_bytes(long n)
{
    if (n <= 0) return 0;
    const long t = sort_tiles(n);
    return round_up(8 * n, 256) + 1024 * t + round_up(4 * scan_chunks(256 * t), 256);
}

// the scan of a table of m counters in place, as the two launches above ; sums: scan_chunks(m) words
static inline int scan_table(unsigned* table, long m, unsigned* sums, hipStream_t st)
{
    const int chunks = (int)scan_chunks(m);
    int rc = launch<scan_chunks_kernel>(dim3((unsigned)chunks), dim3(SORT_THREADS), 0, st, table, m, sums);
    if (rc != DTLR_OK) return rc;
    return launch<scan_sums_kernel>(dim3(1), dim3(SORT_THREADS), 0, st, sums, chunks);
}

}  // namespace dtlr
