// Keyword spotting over the CTC lattice: does a GIVEN word occur in a line, where, and how confidently.  Every
// (line, keyword) pair is one dynamic program with a free start and a free end over all T frames of the plain lattice; its score is the
// log-likelihood ratio of the keyword's best path against the frame-wise argmax path over the same frames (<= 0, 0 = the argmax spells it).
//   ctcs_rowmax_kernel    mx[b,t] = the fp32 maximum of a frame's V channels and ln mx as fp64, one wave per frame.
//   ctc_spot_kernel       one WAVE per (line, keyword), lane s = state s of the keyword WITHOUT outer blanks (2 L - 1 <= 63 states, hence
//                         L <= 32).  A workgroup is up to CTCS_WAVES waves on keywords of one line; they share nothing and the kernel has no
//                         workgroup barrier.  The neighbours' fp64 score and entry frame arrive by cross-lane moves (ds_bpermute: no LDS
//                         memory).  A lane's channel never changes, so it loads its own emissions CTCS_PF frames ahead and takes their fp64
//                         gains in a block, outside the chain of dependent steps (as ctc_align.hip does).  The last state leaves r[t] and
//                         start[t] in the wave's own slice of LDS (12 bytes a frame); the same wave then takes up to H hits greedily: a wave
//                         arg-max by (r, then the smaller t), after which every lane kills the candidates of its frames that overlap the pick.
// Nothing here synchronises with the host.  Keywords, lengths and thresholds are device data: lengths are clamped to [1, min(32, Lmax)] and
// channels to [0, V), so a bad table gives a wrong record, never a fault.
#include "dtlr_common.h"
#include "decode_common.h"

namespace dtlr {

constexpr int CTCS_PF = 8;                           // frames fetched ahead
constexpr int CTCS_WAVES = 4;                        // waves (keywords) per workgroup at most
constexpr int CTCS_LMAX = 32;                        // 2 L - 1 <= 63 lanes
constexpr int CTCS_HMAX = 16;
constexpr size_t CTCS_LDS_BUDGET = 150 * 1024;       // of the 160 KB

// bytes of LDS one wave needs for T frames: double r[T] | int start[T], rounded up to 8
static inline size_t ctcs_wave_bytes(int T) { return (((size_t)T * 12 + 7) / 8) * 8; }
// the largest T one wave per workgroup can hold: 150 KB / 12 B = 12800 frames
static inline int ctcs_waves_for(int T)
{
    const size_t per = ctcs_wave_bytes(T);
    const size_t fit = CTCS_LDS_BUDGET / per;
    return fit >= (size_t)CTCS_WAVES ? CTCS_WAVES : (int)fit;
}

__global__ __launch_bounds__(256) void ctcs_rowmax_kernel(const float* __restrict__ E, float* __restrict__ mx, double* __restrict__ lnmx,
                                                          long rows, int V)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                                    // wave-uniform
    const float* e = E + row * V;
    float m = -INFINITY;
    for (int c = lane; c < V; c += 64) m = fmaxf(m, e[c]);
#pragma unroll
    for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) {
        mx[row] = m;
        lnmx[row] = log(fmax((double)m, 1e-30));
    }
}

__global__ __launch_bounds__(64 * CTCS_WAVES) void ctc_spot_kernel(const float* __restrict__ E, const float* __restrict__ mx,
                                                                   const double* __restrict__ lnmx, const int* __restrict__ keywords,
                                                                   const int* __restrict__ keyword_lengths,
                                                                   const double* __restrict__ min_ratio, int* __restrict__ count,
                                                                   int* __restrict__ start, int* __restrict__ end,
                                                                   double* __restrict__ ratio, int B, int T, int V, int Q, int Lmax, int H,
                                                                   int nqb, int wave_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ctcs_smem[];
    const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x / nqb, q = (blockIdx.x % nqb) * nw + wave;
    if (b >= B || q >= Q) return;                                               // wave-uniform; no workgroup barrier follows
    double* r = reinterpret_cast<double*>(ctcs_smem + (size_t)wave * wave_bytes);
    int* st = reinterpret_cast<int*>(r + T);

    const int L = min(max(keyword_lengths[q], 1), min(CTCS_LMAX, Lmax)), S = 2 * L - 1;
    const int* z = keywords + (long)q * Lmax;
    const int s = lane;
    const bool live = s < S, chr = live && !(s & 1);
    int ch = 0;                                                                 // this state's channel: 0 = the blank
    bool skip = false;
    if (chr) {
        ch = min(max(z[s >> 1], 0), V - 1);
        skip = s >= 2 && ch != min(max(z[(s >> 1) - 1], 0), V - 1);
    }
    const float* erow = E + (long)b * T * V + ch;
    const float* mrow = mx + (long)b * T;
    const double* lrow = lnmx + (long)b * T;

    double d = -INFINITY;                                                       // this state's score and the frame its path entered state 0
    int a = -1;
    float pf[CTCS_PF];
#pragma unroll
    for (int u = 0; u < CTCS_PF; ++u) pf[u] = u < T ? erow[(long)u * V] : 1.f;
    for (int i0 = 0; i0 < T; i0 += CTCS_PF) {
        float nx[CTCS_PF];
        double gv[CTCS_PF];
#pragma unroll
        for (int u = 0; u < CTCS_PF; ++u) {
            const int i = i0 + CTCS_PF + u;
            nx[u] = i < T ? erow[(long)i * V] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < CTCS_PF; ++u) {                                     // the gains: 0 where the fp32 inputs are equal, else fp64 logs
            const int i = min(i0 + u, T - 1);
            gv[u] = pf[u] == mrow[i] ? 0.0 : log(fmax((double)pf[u], 1e-30)) - lrow[i];
        }
#pragma unroll
        for (int u = 0; u < CTCS_PF; ++u) {
            const int t = i0 + u;
            if (t < T) {                                                        // wave-uniform
                double c1 = __shfl_up(d, 1), c2 = __shfl_up(d, 2);
                int a1 = __shfl_up(a, 1);
                const int a2 = __shfl_up(a, 2);
                if (s == 0) { c1 = 0.0; a1 = t; }                               // a fresh entry
                if (!skip) c2 = -INFINITY;
                double m = d;                                                   // stay, then s - 1, then s - 2: the earlier on equality
                int am = a;
                if (c1 > m) { m = c1; am = a1; }
                if (c2 > m) { m = c2; am = a2; }
                d = live ? m + gv[u] : -INFINITY;
                a = am;
                if (s == S - 1) { r[t] = d; st[t] = a; }
            }
        }
#pragma unroll
        for (int u = 0; u < CTCS_PF; ++u) pf[u] = nx[u];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                      // the last state's r / start, before every lane reads them
    __builtin_amdgcn_wave_barrier();

    // candidates: finite r >= the threshold.  From here a lane reads and writes r only at its own frames (t = lane mod 64).
    const double thr = min_ratio[q];
    for (int t = lane; t < T; t += 64) {
        const double v = r[t];
        if (!(v >= thr && v > -INFINITY)) r[t] = -INFINITY;
    }
    int n = 0, ms = -1, me = -1;
    double mr = 0.0;
    for (int h = 0; h < H; ++h) {
        double br = -INFINITY;
        int bt = 0x7fffffff;
        for (int t = lane; t < T; t += 64) {                                    // ascending t: the smaller t stays on equality
            const double v = r[t];
            if (v > br) { br = v; bt = t; }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const double o_r = __shfl_xor(br, off);
            const int o_t = __shfl_xor(bt, off);
            if (o_r > br || (o_r == br && o_t < bt)) { br = o_r; bt = o_t; }
        }
        if (!(br > -INFINITY)) break;                                           // wave-uniform
        const int ps = st[bt];
        if (lane == h) { ms = ps; me = bt; mr = br; }
        ++n;
        for (int t = lane; t < T; t += 64)
            if (t >= ps && st[t] <= bt) r[t] = -INFINITY;                       // [start[t], t] overlaps [ps, bt]; the pick itself included
    }
    const long o = (long)b * Q + q;
    if (lane == 0) count[o] = n;
    if (lane < H) {
        start[o * H + lane] = ms;
        end[o * H + lane] = me;
        ratio[o * H + lane] = mr;
    }
}

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_ctc_spot_workspace_bytes(int B, int T)
{
    if (B <= 0 || T <= 0) return 0;
    return (long)B * T * 12;                                                    // double ln mx [B,T] | float mx [B,T]
}

extern "C" int dtlr_ctc_spot(const float* emissions, int B, int T, int V, const int* keywords, const int* keyword_lengths,
                             const double* min_ratio, int Q, int Lmax, int H, int* count, int* start, int* end, double* ratio,
                             void* workspace, void* stream)
{
    clear_stale_error();
    if (B < 0 || Q < 0) return DTLR_EINVAL;
    if (B == 0 || Q == 0) return DTLR_OK;
    if (T <= 0 || V <= 0 || Lmax < 1) return DTLR_EINVAL;
    if (Lmax > CTCS_LMAX || H < 1 || H > CTCS_HMAX) return DTLR_ESHAPE;          // one lane per state; the hit records of a wave
    const int nw = ctcs_waves_for(T);
    if (nw < 1) return DTLR_ESHAPE;                                              // T > 12800: a wave's r / start do not fit LDS
    if (!emissions || !keywords || !keyword_lengths || !min_ratio || !count || !start || !end || !ratio || !workspace) return DTLR_EINVAL;
    const long rows = (long)B * T, nqb = ((long)Q + nw - 1) / nw;
    if ((rows + 3) / 4 > 0x7fffffffL || (long)B * nqb > 0x7fffffffL || (long)B * Q * H > 0x7fffffffL) return DTLR_ESHAPE;
    double* lnmx = reinterpret_cast<double*>(workspace);
    float* mx = reinterpret_cast<float*>(lnmx + rows);
    if (int rc = launch<ctcs_rowmax_kernel>(dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, emissions, mx, lnmx, rows, V)) return rc;
    const int wave_bytes = (int)ctcs_wave_bytes(T);
    const size_t lds = (size_t)nw * wave_bytes;
    return launch<ctc_spot_kernel>(dim3((unsigned)(B * nqb)), dim3(64 * nw), lds, (hipStream_t)stream, emissions, mx, lnmx, keywords,
                                   keyword_lengths, min_ratio, count, start, end, ratio, B, T, V, Q, Lmax, H, (int)nqb, wave_bytes);
}
