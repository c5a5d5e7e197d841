// CTC forced alignment: the best path of a KNOWN transcript through a span of emissions, and from it the
// frames of every character.  The max-product twin of the alpha recursion of dtlr_ctc_loss_interleaved, with a back-trace.
//   dtlr_ctc_align        every span of a table in one launch, one workgroup per span, one thread per state of the blank-extended
//                         target (2 L + 1 <= 1024).  Scores are fp64, double-buffered in LDS.  A thread's channel never changes, so it
//                         loads its own emissions CTCA_PF frames ahead and takes their logs in a block, outside the chain of dependent
//                         steps; filler frames read nothing.  Back-pointers are 2 bits per (frame, state), stored as two wave ballots
//                         (16 bytes per wave and frame): in LDS when the span's frames fit beside the scores, else in the caller's
//                         workspace, from which the back-trace stages them through LDS a chunk of frames at a time.  One lane walks the
//                         back-trace and leaves every character's first and last lattice frame in LDS; L lanes then find the peaks and
//                         write the records.
//   dtlr_reading_order    rank -> query of every line by the decoders' key (ascending cx, equal cx: lower query first).
// Nothing here synchronises with the host.  The span table and the targets are device data: lines, frames and channels are clamped,
// so a bad table gives a wrong or infeasible record, never a fault.
#include "dtlr_common.h"
#include "decode_common.h"

namespace dtlr {

constexpr int CTCA_PF = 8;                           // real frames fetched ahead
constexpr size_t CTCA_LDS_BUDGET = 150 * 1024;       // of the 160 KB

// how one call lays a span out: the same arithmetic sizes the launch and answers the workspace query
struct CtcaPlan {
    int threads, nw, Lc, J, rows;     // nw waves; J lattice frames at most; rows of back-pointers held in LDS
    size_t lds;
    bool use_ws;
    long ws_span;                     // 8-byte words of workspace per span
};

static inline CtcaPlan ctca_plan(int Tmax, int Lcap, int interleaved)
{
    CtcaPlan p;
    const int S = 2 * Lcap + 1;
    p.threads = S <= 64 ? 64 : ((S + 63) / 64) * 64;
    p.nw = p.threads / 64;
    p.Lc = Lcap > 0 ? Lcap : 1;
    p.J = interleaved ? 2 * Tmax : Tmax;
    const size_t fixed = (size_t)2 * (p.threads + 2) * 8 + (size_t)2 * p.Lc * 4, row = (size_t)p.nw * 16;
    const long cap = (long)((CTCA_LDS_BUDGET - fixed) / row);
    const int need = p.J > 1 ? p.J - 1 : 1;           // frame 0 has no back-pointer
    p.use_ws = need > cap;
    p.rows = p.use_ws ? (int)cap : need;
    p.lds = fixed + (size_t)p.rows * row;
    p.ws_span = p.use_ws ? (long)need * p.nw * 2 : 0;
    return p;
}

__global__ __launch_bounds__(1024) void ctc_align_kernel(const float* __restrict__ E, const int* __restrict__ spans,
                                                         const int* __restrict__ targets, const int* __restrict__ target_lengths,
                                                         double* __restrict__ score, int* __restrict__ first, int* __restrict__ last,
                                                         int* __restrict__ peak, float* __restrict__ prob, int* __restrict__ length,
                                                         unsigned long long* __restrict__ ws, int B, int T, int V, int Lmax, int Lcap,
                                                         int Tmax, int interleaved, float filler, int rows, int use_ws, long ws_span)
{
    // double d[2][blockDim + 2] (two -inf guard slots in front) | u64 bp[rows][nw][2] | int segF[Lc] | int segL[Lc]
    extern __shared__ __attribute__((aligned(16))) unsigned char ctca_smem[];
    __shared__ int s_end;
    const int AP = blockDim.x + 2, nw = blockDim.x >> 6;
    double* dbuf = reinterpret_cast<double*>(ctca_smem);
    unsigned long long* bpl = reinterpret_cast<unsigned long long*>(dbuf + 2 * AP);
    int* segF = reinterpret_cast<int*>(bpl + (size_t)rows * nw * 2);
    int* segL = segF + (Lcap > 0 ? Lcap : 1);
    const int k = blockIdx.x, s = threadIdx.x, wave = s >> 6, lane = s & 63;
    const int b = min(max(spans[3 * k], 0), B - 1);
    const int t0 = min(max(spans[3 * k + 1], 0), T);
    const int t1 = min(max(spans[3 * k + 2], t0), T);
    const int F = min(t1 - t0, Tmax);                                          // real frames
    const int J = interleaved ? 2 * F : F;                                     // lattice frames
    const int L = min(max(target_lengths[k], 0), Lcap), S = 2 * L + 1;
    const int* z = targets + (long)k * Lmax;
    const bool live = s < S, odd = live && (s & 1);
    int ch = 0;                                                                 // this state's channel: 0 = the blank
    bool skip = false;
    if (odd) {
        ch = min(max(z[s >> 1], 0), V - 1);
        skip = s >= 3 && ch != min(max(z[(s >> 1) - 1], 0), V - 1);
    }
    const float* eline = E + ((long)b * T + t0) * V;                            // frame t0 of the line
    const float* erow = eline + ch;
    const double lfill = odd ? log((double)filler) : 0.0;
    unsigned long long* wsk = ws + (long)k * ws_span;

    double* prev = dbuf + 2;
    double* cur = dbuf + AP + 2;
    if (s < 2) { dbuf[s] = -INFINITY; dbuf[AP + s] = -INFINITY; }

    // lattice frame j >= 1: prev -> cur.  Equal candidates take the smallest shift.
    auto step = [&](int j, double lp) {
        int bp = 0;
        if (live) {
            const double c1 = prev[s - 1], c2 = skip ? prev[s - 2] : -INFINITY;
            double m = prev[s];
            if (c1 > m) { m = c1; bp = 1; }
            if (c2 > m) { m = c2; bp = 2; }
            cur[s] = m + lp;
        }
        const unsigned long long m0 = __builtin_amdgcn_ballot_w64((bp & 1) != 0), m1 = __builtin_amdgcn_ballot_w64((bp & 2) != 0);
        if (lane == 0) {
            unsigned long long* row = (use_ws ? wsk : bpl) + ((long)(j - 1) * nw + wave) * 2;
            row[0] = m0;
            row[1] = m1;
        }
        __syncthreads();
        double* t = prev; prev = cur; cur = t;
    };

    float pf[CTCA_PF];
#pragma unroll
    for (int u = 0; u < CTCA_PF; ++u) pf[u] = (live && u < F) ? erow[(long)u * V] : 1.f;
    for (int i0 = 0; i0 < F; i0 += CTCA_PF) {
        float nx[CTCA_PF];
        double lpv[CTCA_PF];
#pragma unroll
        for (int u = 0; u < CTCA_PF; ++u) {
            const int i = i0 + CTCA_PF + u;
            nx[u] = (live && i < F) ? erow[(long)i * V] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < CTCA_PF; ++u) lpv[u] = log(fmax((double)pf[u], 1e-30));
#pragma unroll
        for (int u = 0; u < CTCA_PF; ++u) {
            const int i = i0 + u;
            if (i < F) {                                                        // block-uniform
                if (i == 0) {                                                   // frame 0: only states 0 and 1 can start a path
                    if (live) prev[s] = s < 2 ? lpv[u] : -INFINITY;
                    __syncthreads();
                } else step(interleaved ? 2 * i : i, lpv[u]);
                if (interleaved) step(2 * i + 1, lfill);
            }
        }
#pragma unroll
        for (int u = 0; u < CTCA_PF; ++u) pf[u] = nx[u];
    }

    if (s == 0) {                                                               // after the last frame the scores are in prev
        int e = -1;
        double sc = -INFINITY;
        if (F == 0) { if (L == 0) { sc = 0.0; e = 0; } }
        else if (L == 0) { sc = prev[0]; e = 0; }
        else {
            const double a = prev[2 * L - 1], c = prev[2 * L];
            if (a >= c) { sc = a; e = 2 * L - 1; } else { sc = c; e = 2 * L; }
        }
        if (!(sc > -INFINITY)) { sc = -INFINITY; e = -1; }
        score[k] = sc;
        length[k] = e >= 0 ? L : -1;
        s_end = e;
    }
    __syncthreads();
    const int e = s_end;
    if (e >= 0 && L > 0) {                                                      // block-uniform; F > 0 here
        int st = e, pst = -1;                                                   // thread 0's walk
        auto visit = [&](int j) {
            if (st & 1) {
                if (st != pst) segL[st >> 1] = j;
                segF[st >> 1] = j;
            }
            pst = st;
        };
        for (int jhi = J - 1; jhi >= 1; jhi -= rows) {
            const int jlo = max(jhi - rows + 1, 1);
            if (use_ws) {                                                       // stage rows jlo..jhi
                const long nwords = (long)(jhi - jlo + 1) * nw * 2;
                const unsigned long long* src = wsk + (long)(jlo - 1) * nw * 2;
                for (long w = s; w < nwords; w += blockDim.x) bpl[w] = src[w];
                __syncthreads();
            }
            if (s == 0) {
                for (int j = jhi; j >= jlo; --j) {
                    visit(j);
                    const unsigned long long* row = bpl + ((long)(j - jlo) * nw + (st >> 6)) * 2;
                    const int l = st & 63;
                    st -= (int)((row[0] >> l) & 1ull) + 2 * (int)((row[1] >> l) & 1ull);
                }
            }
            if (use_ws) __syncthreads();
        }
        if (s == 0) visit(0);
        __syncthreads();
    }
    for (int i = s; i < Lmax; i += blockDim.x) {
        int f = -1, l = -1, pk = -1;
        float pr = 0.f;
        if (e >= 0 && i < L) {
            const int c = min(max(z[i], 0), V - 1), jF = min(max(segF[i], 0), J - 1), jL = min(max(segL[i], 0), J - 1);
            double bv = 0.0;
            int bj = -1;
            for (int j = jF; j <= jL; ++j) {                                    // log is strictly monotone: compare its argument
                float ev;
                double v;
                if (interleaved && (j & 1)) { ev = filler; v = (double)filler; }
                else { ev = eline[(long)(interleaved ? j >> 1 : j) * V + c]; v = fmax((double)ev, 1e-30); }
                if (bj < 0 || v > bv) { bv = v; bj = j; pr = ev; }
            }
            f = t0 + (interleaved ? jF >> 1 : jF);
            l = t0 + (interleaved ? jL >> 1 : jL);
            pk = t0 + (interleaved ? bj >> 1 : bj);
        }
        const long o = (long)k * Lmax + i;
        first[o] = f;
        last[o] = l;
        peak[o] = pk;
        prob[o] = pr;
    }
}

// one workgroup per line: order[b, r] = the query at rank r
__global__ __launch_bounds__(1024) void ctca_reading_order_kernel(const float* __restrict__ boxes, int* __restrict__ order, int nq, int npow2)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long ro_keys[];
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < npow2; i += blockDim.x)
        ro_keys[i] = i < nq ? (((unsigned long long)f32_sortable(boxes[((long)b * nq + i) * 4])) << 32) | (unsigned)i : ~0ull;
    bitonic_sort_u64(ro_keys, npow2);                                           // ascending cx, ties: lower index first
    for (int i = threadIdx.x; i < nq; i += blockDim.x) order[(long)b * nq + i] = (int)(ro_keys[i] & 0xffffffffull);
}

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_ctc_align_workspace_bytes(int n, int Tmax, int max_target_length, int interleaved)
{
    if (n <= 0 || Tmax < 0 || max_target_length < 0 || 2 * (long)max_target_length + 1 > 1024) return 0;
    return (long)n * ctca_plan(Tmax, max_target_length, interleaved != 0).ws_span * 8;
}

extern "C" int dtlr_ctc_align(const float* emissions, int B, int T, int V, const int* spans, const int* targets, const int* target_lengths,
                              int n, int Lmax, int max_target_length, int Tmax, int interleaved, float filler,
                              double* score, int* first, int* last, int* peak, float* prob, int* length, void* workspace, void* stream)
{
    clear_stale_error();
    if (n < 0 || Lmax < 0 || max_target_length < 0 || max_target_length > Lmax || Tmax < 0) return DTLR_EINVAL;
    if (n == 0) return DTLR_OK;
    if (!emissions || !spans || !target_lengths || !score || !length || B <= 0 || T <= 0 || V <= 0) return DTLR_EINVAL;
    if (Lmax > 0 && (!targets || !first || !last || !peak || !prob)) return DTLR_EINVAL;
    if (2 * (long)max_target_length + 1 > 1024) return DTLR_ESHAPE;            // one thread per state
    if (Tmax > (1 << 29) || (long)B * T * V < 0) return DTLR_ESHAPE;
    const CtcaPlan p = ctca_plan(Tmax, max_target_length, interleaved != 0);
    if (p.rows < 1) return DTLR_ESHAPE;
    if (p.use_ws && !workspace) return DTLR_EINVAL;
    return launch<ctc_align_kernel>(dim3(n), dim3(p.threads), p.lds, (hipStream_t)stream, emissions, spans, targets, target_lengths,
                                    score, first, last, peak, prob, length, reinterpret_cast<unsigned long long*>(workspace), B, T, V, Lmax,
                                    max_target_length, Tmax, interleaved != 0 ? 1 : 0, filler, p.rows, p.use_ws ? 1 : 0, p.ws_span);
}

extern "C" int dtlr_reading_order(const float* boxes, int* order, int B, int nq, void* stream)
{
    clear_stale_error();
    if (!boxes || !order || B <= 0 || nq <= 0) return DTLR_EINVAL;
    int np = 1;
    while (np < nq) np <<= 1;
    if ((size_t)np * 8 > CTCA_LDS_BUDGET) return DTLR_ESHAPE;
    const size_t lds = (size_t)np * 8;
    const int threads = np / 2 >= 1024 ? 1024 : (np / 2 <= 64 ? 64 : np / 2);
    return launch<ctca_reading_order_kernel>(dim3(B), dim3(threads), lds, (hipStream_t)stream, boxes, order, nq, np);
}
