// Edit distance and alignment of n pairs of int32 sequences: the Levenshtein distance, the (insertions,
// deletions, substitutions) of the alignment the reference's walk back picks, and that alignment step by step.
//   edit_align_kernel  one wavefront (a workgroup of 64 threads) per pair, a fixed grid: workgroup g takes pairs g, g + G, ...  The
//                      rows of the lattice belong to a, the columns to b.  The rows go in bands of 64, one row a lane; inside a band
//                      the lanes sweep the anti-diagonals: at step t lane l fills column t - l + 1 of its row.  A cell is one 32-bit
//                      word, (D << 16) | deletions: the deletions of the walk back from that cell travel with the distance, the
//                      insertions follow from them (ins - del = j - i on every path to (i, j)) and the substitutions from the
//                      distance, so `dist` and `counts` need no stored lattice.  A lane's left neighbour is its own last cell, its
//                      upper neighbour arrives from lane l - 1 by one shuffle a step and becomes the diagonal neighbour of the next
//                      step.  Lane 0's upper row is the last row of the band before: two rows of max_b + 1 words in LDS, one read
//                      while the other is written, a barrier between two bands.
//                      With want_ops every lane also packs the 2-bit move of its cells (0 equal, 1 substitution, 2 deletion,
//                      3 insertion), sixteen columns a word, and stores the word into the pair's slot of the workspace: a row of the
//                      lattice is ceil(lb / 16) words that one lane alone writes.  After the fill (a device-scope fence, a barrier)
//                      lane 0 walks the moves back from (la, lb), reading a word again only when the row or the word changes, and
//                      writes the steps from slot n_ops - 1 downwards: n_ops = lb + deletions is known from the fill, so the
//                      steps land in forward order.  What is left at the border (i == 0 or j == 0) is written by all lanes.
// Nothing here synchronises with the host.  No 16-bit type is involved: both builds export the same code.
#include "dtlr_common.h"
#include "../../include/dtlr_metrics.h"

namespace dtlr {

constexpr int EDIT_LANES = 64;
constexpr int EDIT_GRID = 1 << 16;                   // workgroups at the most
constexpr int EDIT_MAX = DTLR_EDIT_MAX_LEN;
static_assert(EDIT_MAX < (1 << 15), "a distance and a deletion count share one 32-bit word");
static_assert(2 * (size_t)(EDIT_MAX + 1) * sizeof(unsigned) <= 64 * 1024, "the two boundary rows fit the LDS of one workgroup");

// bytes of one pair's slot of moves: max_a rows of ceil(max_b / 16) words, rounded up to 128 bytes
static inline long edit_slot_bytes(int max_a, int max_b)
{
    const long bytes = (long)max_a * ((max_b + 15) / 16) * 4;
    return (bytes + 127) / 128 * 128;
}

__global__ __launch_bounds__(EDIT_LANES) void edit_align_kernel(
    const int* __restrict__ a, const long* __restrict__ a_off, const int* __restrict__ b, const long* __restrict__ b_off,
    int* __restrict__ dist, int* __restrict__ counts, int* __restrict__ n_ops, int* __restrict__ ops, unsigned* ws, long slot_words,
    int n, int max_a, int max_b, int want_ops)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char edit_smem[];        // unsigned row[2][max_b + 1]
    unsigned* rows = reinterpret_cast<unsigned*>(edit_smem);
    const int lane = threadIdx.x;

    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        const long a0 = a_off[p], b0 = b_off[p];
        const int la = (int)min(max(a_off[p + 1] - a0, 0L), (long)max_a);
        const int lb = (int)min(max(b_off[p + 1] - b0, 0L), (long)max_b);
        const int* ap = a + a0;
        const int* bp = b + b0;
        const int pitch = (lb + 15) >> 4;                                            // words of moves in a row
        unsigned* codes = ws + (size_t)p * slot_words;

        unsigned* rin = rows;                                                        // the row above the band: cell (64 r, j) at [j]
        unsigned* rout = rows + (max_b + 1);
        for (int j = lane; j <= lb; j += EDIT_LANES) rin[j] = (unsigned)j << 16;     // row 0: D = j, no deletion
        __syncthreads();

        unsigned last = (unsigned)lb << 16;                                          // cell (la, lb); la == 0: the end of row 0
        for (int r0 = 0; r0 < la; r0 += EDIT_LANES) {
            const int nrows = min(EDIT_LANES, la - r0);
            const int i = r0 + lane + 1;                                             // this lane's row, 1-based
            const bool mine = lane < nrows;
            const int ai = mine ? ap[i - 1] : 0;
            unsigned left = ((unsigned)i << 16) | (unsigned)i;                       // cell (i, 0): D = i, all deletions
            unsigned diag = ((unsigned)(i - 1) << 16) | (unsigned)(i - 1);           // cell (i - 1, 0)
            unsigned acc = 0;
            if (lane == nrows - 1) rout[0] = left;
            const int steps = lb + nrows - 1;
            for (int t = 0; t < steps; ++t) {
                const int j = t - lane + 1;                                          // this lane's column, 1-based
                const bool valid = mine && j >= 1 && j <= lb;
                unsigned up = __shfl_up(left, 1);                                    // cell (i - 1, j): lane l - 1 filled it last step
                if (lane == 0) up = rin[min(max(j, 0), lb)];
                if (valid) {
                    unsigned cur, code;
                    if (ai == bp[j - 1]) {
                        cur = diag;
                        code = 0;
                    } else {
                        const unsigned dd = diag >> 16, du = up >> 16, dl = left >> 16;
                        if (dd <= du && dd <= dl) {
                            cur = diag + (1u << 16);
                            code = 1;
                        } else if (du <= dl) {
                            cur = up + (1u << 16) + 1u;
                            code = 2;
                        } else {
                            cur = left + (1u << 16);
                            code = 3;
                        }
                    }
                    left = cur;
                    if (lane == nrows - 1) rout[j] = cur;
                    if (want_ops) {
                        acc |= code << (((j - 1) & 15) << 1);
                        if (((j - 1) & 15) == 15 || j == lb) {
                            codes[(size_t)(i - 1) * pitch + ((j - 1) >> 4)] = acc;
                            acc = 0;
                        }
                    }
                }
                diag = up;
            }
            last = __shfl(left, nrows - 1);                                          // cell (r0 + nrows, lb)
            __syncthreads();                                                         // rout is whole; rin has been read
            unsigned* sw = rin; rin = rout; rout = sw;
        }

        const int d = (int)(last >> 16), dele = (int)(last & 0xffffu);
        const int ins = dele + lb - la, steps = lb + dele;
        if (lane == 0) {
            dist[p] = d;
            counts[3 * (long)p] = ins;
            counts[3 * (long)p + 1] = dele;
            counts[3 * (long)p + 2] = d - ins - dele;
        }
        if (want_ops) {
            __threadfence();                                                         // the moves of all lanes, before lane 0 reads them
            __syncthreads();
            int2* out = reinterpret_cast<int2*>(ops) + (a0 + b0);
            int i = la, j = lb, k = steps - 1;
            if (lane == 0) {
                n_ops[p] = steps;
                long at = -1;
                unsigned w = 0;
                while (i > 0 && j > 0 && k >= 0) {                                   // k >= 0 holds by itself: the moves are the fill's
                    const long want = (long)(i - 1) * pitch + ((j - 1) >> 4);
                    if (want != at) {
                        at = want;
                        w = __hip_atomic_load(codes + want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    const unsigned code = (w >> (((j - 1) & 15) << 1)) & 3u;
                    if (code <= 1) {
                        out[k] = make_int2(i - 1, j - 1);
                        --i; --j;
                    } else if (code == 2) {
                        out[k] = make_int2(i - 1, -1);
                        --i;
                    } else {
                        out[k] = make_int2(-1, j - 1);
                        --j;
                    }
                    --k;
                }
            }
            i = __shfl(i, 0);                                                        // the border: one of the two is 0, the other k + 1
            j = __shfl(j, 0);
            k = __shfl(k, 0);
            for (int q = lane; q < min(j, k + 1); q += EDIT_LANES) out[q] = make_int2(-1, q);
            for (int q = lane; q < min(i, k + 1); q += EDIT_LANES) out[q] = make_int2(q, -1);
        }
        __syncthreads();                                                             // the rows go to the next pair
    }
}

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_edit_align_workspace_bytes(int n, int max_a, int max_b)
{
    if (n <= 0 || max_a <= 0 || max_b <= 0) return 0;
    return (long)n * edit_slot_bytes(max_a, max_b);
}

extern "C" int dtlr_edit_align(const int* a, const long* a_off, const int* b, const long* b_off, int n, int max_a, int max_b,
                               int want_ops, int* dist, int* counts, int* n_ops, int* ops, void* workspace, long workspace_bytes,
                               void* stream)
{
    clear_stale_error();
    if (n < 0 || max_a < 0 || max_b < 0) return DTLR_EINVAL;
    if (max_a > EDIT_MAX || max_b > EDIT_MAX) return DTLR_ESHAPE;
    const long need = want_ops ? dtlr_edit_align_workspace_bytes(n, max_a, max_b) : 0;
    if (want_ops && workspace_bytes < need) return DTLR_ESHAPE;
    if (n == 0) return DTLR_OK;
    if (!a_off || !b_off || !dist || !counts) return DTLR_EINVAL;
    if ((max_a > 0 && !a) || (max_b > 0 && !b)) return DTLR_EINVAL;
    if (want_ops && (!n_ops || (max_a + max_b > 0 && !ops) || (need > 0 && !workspace))) return DTLR_EINVAL;
    const size_t lds = 2 * (size_t)(max_b + 1) * sizeof(unsigned);
    return launch<edit_align_kernel>(dim3((unsigned)(n < EDIT_GRID ? n : EDIT_GRID)), dim3(EDIT_LANES), lds, (hipStream_t)stream, a,
                                     a_off, b, b_off, dist, counts, n_ops, ops, reinterpret_cast<unsigned*>(workspace),
                                     edit_slot_bytes(max_a, max_b) / 4, n, max_a, max_b, want_ops);
}
