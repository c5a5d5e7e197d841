// The set criterion of a DETR-style detector on the device (include/dtlr_setloss.h):
//   dtlr_set_cost    the matching cost of every query against its own line's targets, [P, Tmax, nq] target-major
//   dtlr_hungarian   the minimum-cost assignment of each block: shortest augmenting paths with duals, one workgroup a problem
//   dtlr_set_loss    focal / L1 / GIoU losses and their gradients given the assignment
//
// dtlr_set_cost: a thread owns one query of one problem and walks the line's targets.  The class term needs logits[q, label_t], a gather
// that strides C floats between queries; it is read once per distinct label of the line (the first target with a label is its leader,
// found in LDS), left in the leader's row of the block, and the rows are then finished from the last target to the first, so a row
// reads its leader's class term before the leader's own row is overwritten -- by the same thread, no barrier involved.
//
// dtlr_hungarian: scipy's rectangular_lsap restated for a workgroup.  The state (duals u, v, the shortest path costs, the predecessor,
// both assignments, the visited flags) lives in LDS; a scan step is one strided pass of the workgroup over the unvisited columns (the
// cost row is contiguous: target-major) and a (cost, unassigned first, index) min-reduction through the waves' shuffles and one LDS
// exchange.  The next row, the minimum and the sink travel through LDS, so every loop that holds a barrier runs the same trip count in
// every thread, and each carries a hard bound.
//
// dtlr_set_loss: one pass over the logits (a wave a query row) gives the focal sum, dlogits, the row's argmax and zeroes the row of
// dboxes; a finishing workgroup an output adds the partial sums in a fixed order and does the matched pairs.
#include "dtlr_common.h"
#include "../../include/dtlr_setloss.h"
#include <math.h>

namespace dtlr {

constexpr int SL_TMAX = 2048;             // set_cost: targets a line (24 bytes of LDS each)
constexpr int SL_QB = 32;                 // set_loss: query rows a workgroup (8 a wave)
constexpr long SL_HUNG_LDS = 150 * 1024;  // hungarian: the most LDS a problem may take

struct SlTargets { int t0, T; };
__device__ __forceinline__ SlTargets sl_targets(const int* __restrict__ offsets, int b, int Tmax, int n_targets)
{
    int t0 = offsets[b], t1 = offsets[b + 1];
    t0 = min(max(t0, 0), n_targets);
    t1 = min(max(t1, t0), n_targets);
    SlTargets r;
    r.t0 = t0;
    r.T = min(t1 - t0, Tmax);
    return r;
}

// GIoU of two (cx, cy, w, h) boxes through their xyxy forms, with the reference's 1e-6 in both denominators (util/box_ops.py:
// I / (U + 1e-6) - (Ac - U) / (Ac + 1e-6)) ; grad (or nullptr): d GIoU / d (cx, cy, w, h) of the first
__device__ __forceinline__ double sl_giou(const double* s, const double* g, double* grad)
{
    const double x0 = s[0] - 0.5 * s[2], y0 = s[1] - 0.5 * s[3], x1 = s[0] + 0.5 * s[2], y1 = s[1] + 0.5 * s[3];
    const double gx0 = g[0] - 0.5 * g[2], gy0 = g[1] - 0.5 * g[3], gx1 = g[0] + 0.5 * g[2], gy1 = g[1] + 0.5 * g[3];
    const double a1 = (x1 - x0) * (y1 - y0), a2 = (gx1 - gx0) * (gy1 - gy0);
    const double iwr = fmin(x1, gx1) - fmax(x0, gx0), ihr = fmin(y1, gy1) - fmax(y0, gy0);
    const double iw = fmax(iwr, 0.0), ih = fmax(ihr, 0.0), inter = iw * ih, uni = a1 + a2 - inter;
    const double cwr = fmax(x1, gx1) - fmin(x0, gx0), chr = fmax(y1, gy1) - fmin(y0, gy0);
    const double cw = fmax(cwr, 0.0), ch = fmax(chr, 0.0), ac = cw * ch, ue = uni + 1e-6, ae = ac + 1e-6;
    if (grad) {
        // d GIoU = kI dI + kA dA1 + kC dAc  (U = A1 + A2 - I, dU = dA1 - dI)
        const double kI = 1.0 / ue + inter / (ue * ue) - 1.0 / ae, kA = 1.0 / ae - inter / (ue * ue), kC = -ue / (ae * ae);
        const double miw = iwr >= 0.0 ? ih : 0.0, mih = ihr >= 0.0 ? iw : 0.0, mcw = cwr >= 0.0 ? ch : 0.0, mch = chr >= 0.0 ? cw : 0.0;
        const double dx1 = kI * (x1 < gx1 ? miw : 0.0) + kA * (y1 - y0) + kC * (x1 > gx1 ? mcw : 0.0);
        const double dx0 = -(kI * (x0 > gx0 ? miw : 0.0) + kA * (y1 - y0) + kC * (x0 < gx0 ? mcw : 0.0));
        const double dy1 = kI * (y1 < gy1 ? mih : 0.0) + kA * (x1 - x0) + kC * (y1 > gy1 ? mch : 0.0);
        const double dy0 = -(kI * (y0 > gy0 ? mih : 0.0) + kA * (x1 - x0) + kC * (y0 < gy0 ? mch : 0.0));
        grad[0] = dx0 + dx1;
        grad[1] = dy0 + dy1;
        grad[2] = 0.5 * (dx1 - dx0);
        grad[3] = 0.5 * (dy1 - dy0);
    }
    return inter / ue - (ac - uni) / ae;
}

// ------------------------------------------------------------------------------------------------------------------ the matching cost
// grid (ceil(nq / 256), P) ; dynamic LDS: Tmax x (box 16, label 4, leader 4)
__global__ __launch_bounds__(256) void set_cost_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                       const int* __restrict__ labels, const int* __restrict__ offsets,
                                                       const float* __restrict__ tboxes, int n_targets, int B, int nq, int C, int Tmax,
                                                       double wc, double wb, double wg, double alpha, float* cost)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sl_smem[];
    float* tb = reinterpret_cast<float*>(sl_smem);
    int* lab = reinterpret_cast<int*>(tb + 4l * Tmax);
    int* lead = lab + Tmax;
    const int p = blockIdx.y, b = p % B;
    const SlTargets tg = sl_targets(offsets, b, Tmax, n_targets);
    for (int t = threadIdx.x; t < tg.T; t += 256) {
        lab[t] = min(max(labels[tg.t0 + t], 0), C - 1);
        for (int i = 0; i < 4; ++i) tb[4 * t + i] = tboxes[4l * (tg.t0 + t) + i];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tg.T; t += 256) {
        const int l = lab[t];
        int k = t;
        for (int j = 0; j < t; ++j)
            if (lab[j] == l) { k = j; break; }
        lead[t] = k;
    }
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    float* cp = cost + (long)p * Tmax * nq + q;
    const float* lrow = logits + ((long)p * nq + q) * C;
    for (int t = 0; t < tg.T; ++t) {
        if (lead[t] != t) continue;
        const double x = (double)lrow[lab[t]];
        const double s = 1.0 / (1.0 + exp(-x));
        const double pos = alpha * ((1.0 - s) * (1.0 - s)) * -log(s + 1e-8);
        const double neg = (1.0 - alpha) * (s * s) * -log(1.0 - s + 1e-8);
        cp[(long)t * nq] = (float)(pos - neg);
    }
    const float4 bq = *reinterpret_cast<const float4*>(boxes + ((long)p * nq + q) * 4);
    const double sb[4] = {(double)bq.x, (double)bq.y, (double)bq.z, (double)bq.w};
    for (int t = tg.T - 1; t >= 0; --t) {
        const double cls = (double)cp[(long)lead[t] * nq];
        const double g[4] = {(double)tb[4 * t], (double)tb[4 * t + 1], (double)tb[4 * t + 2], (double)tb[4 * t + 3]};
        const double l1 = (fabs(sb[0] - g[0]) + fabs(sb[1] - g[1])) + (fabs(sb[2] - g[2]) + fabs(sb[3] - g[3]));
        const double giou = sl_giou(sb, g, nullptr);
        cp[(long)t * nq] = (float)(wb * l1 + wc * cls - wg * giou);
    }
    for (int t = tg.T; t < Tmax; ++t) cp[(long)t * nq] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ the assignment
// grid P, NT threads ; dynamic LDS: see dtlr_hungarian below.  nr rows (the smaller side) are assigned to nc columns.
template <int NT>
__global__ __launch_bounds__(NT) void hungarian_kernel(const float* __restrict__ cost, const int* __restrict__ sizes, int Rmax, int ncols,
                                                       int* __restrict__ match, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sl_smem[];
    constexpr int NW = NT / 64;
    __shared__ double red_v[NW];
    __shared__ int red_j[NW], red_f[NW];
    __shared__ double s_min;
    __shared__ int s_row, s_sink, s_fail;
    const int NR = min(Rmax, ncols), NC = max(Rmax, ncols);
    double* u = reinterpret_cast<double*>(sl_smem);
    double* v = u + NR;
    double* sh = v + NC;
    int* path = reinterpret_cast<int*>(sh + NC);
    int* row4col = path + NC;
    int* col4row = row4col + NC;
    unsigned char* SC = reinterpret_cast<unsigned char*>(col4row + NR);
    unsigned char* SR = SC + NC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int T = min(max(sizes[p], 0), Rmax);
    const bool tr = T > ncols;                                   // the columns of the block are the smaller side: assign them
    const int nr = tr ? ncols : T, nc = tr ? T : ncols;
    const float* cp = cost + (long)p * Rmax * ncols;
    int* mp = match + (long)p * Rmax;
    const double INF = __builtin_huge_val();
    for (int t = tid; t < Rmax; t += NT) mp[t] = -1;
    int bad = 0;
    for (long e = tid; e < (long)T * ncols; e += NT) bad |= !isfinite(cp[e]);
    bad = __syncthreads_or(bad);
    if (bad) {                                                   // uniform: every thread holds the workgroup's OR
        if (tid == 0) status[p] = -1;
        return;
    }
    if (nr == 0) {
        if (tid == 0) status[p] = 0;
        return;
    }
    for (int i = tid; i < nr; i += NT) { u[i] = 0.0; col4row[i] = -1; }
    for (int j = tid; j < nc; j += NT) { v[j] = 0.0; row4col[j] = -1; }
    for (int cur = 0; cur < nr; ++cur) {                         // at most min(rows, columns) augmentations
        for (int j = tid; j < nc; j += NT) { sh[j] = INF; SC[j] = 0; path[j] = -1; }
        for (int i = tid; i < nr; i += NT) SR[i] = 0;
        if (tid == 0) { s_row = cur; s_min = 0.0; s_sink = -1; s_fail = 0; }
        __syncthreads();
        int sink = -1;
        for (int step = 0; step <= nr; ++step) {                 // at most min(rows, columns) + 1 scan steps
            const int i = s_row;
            const double minv = s_min, ui = u[i];
            if (tid == 0) SR[i] = 1;
            double bv = INF;
            int bj = -1, bf = 0;
            const float* crow = tr ? cp + i : cp + (long)i * ncols;
            const long cstride = tr ? ncols : 1;
            for (int j = tid; j < nc; j += NT) {
                if (SC[j]) continue;
                const double r = minv + (double)crow[j * cstride] - ui - v[j];
                double s = sh[j];
                if (r < s) { s = r; sh[j] = r; path[j] = i; }
                const int f = row4col[j] < 0;
                if (s < bv || (s == bv && f > bf)) { bv = s; bj = j; bf = f; }       // j ascends: the lowest index of equals stays
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oj = __shfl_xor(bj, o, 64), of = __shfl_xor(bf, o, 64);
                if (ov < bv || (ov == bv && (of > bf || (of == bf && (unsigned)oj < (unsigned)bj)))) { bv = ov; bj = oj; bf = of; }
            }
            if (lane == 0) { red_v[wave] = bv; red_j[wave] = bj; red_f[wave] = bf; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < NW; ++w) {
                    const double ov = red_v[w];
                    const int oj = red_j[w], of = red_f[w];
                    if (ov < bv || (ov == bv && (of > bf || (of == bf && (unsigned)oj < (unsigned)bj)))) { bv = ov; bj = oj; bf = of; }
                }
                if (bj < 0 || bj >= nc || !(bv < INF)) {
                    s_fail = 1;
                } else {
                    s_min = bv;
                    SC[bj] = 1;
                    const int r = row4col[bj];
                    if (r < 0) s_sink = bj;
                    else s_row = r;
                }
            }
            __syncthreads();
            sink = s_sink;
            if (s_fail || sink >= 0) break;                      // read after the barrier: the same in every thread
        }
        if (sink < 0) {                                          // uniform
            for (int t = tid; t < Rmax; t += NT) mp[t] = -1;
            if (tid == 0) status[p] = -2;
            return;
        }
        const double minv = s_min;
        for (int i = tid; i < nr; i += NT) {
            const int c = col4row[i];
            if (SR[i] && i != cur && c >= 0) u[i] += minv - sh[c];
        }
        if (tid == 0) u[cur] += minv;
        for (int j = tid; j < nc; j += NT)
            if (SC[j]) v[j] -= minv - sh[j];
        __syncthreads();
        if (tid == 0) {                                          // augment along the predecessors: at most nr links
            int j = sink, k = 0;
            for (; k <= nr; ++k) {
                const int i = path[j];
                if (i < 0 || i >= nr) break;
                row4col[j] = i;
                const int old = col4row[i];
                col4row[i] = j;
                j = old;
                if (i == cur) { k = -1; break; }
                if (j < 0 || j >= nc) break;
            }
            if (k != -1) s_fail = 1;
        }
        __syncthreads();
        if (s_fail) {                                            // uniform
            for (int t = tid; t < Rmax; t += NT) mp[t] = -1;
            if (tid == 0) status[p] = -2;
            return;
        }
    }
    for (int t = tid; t < T; t += NT) mp[t] = tr ? row4col[t] : col4row[t];
    if (tid == 0) status[p] = 0;
}

// ------------------------------------------------------------------------------------------------------------------ losses, gradients
// grid (ceil(nq / SL_QB), P), 256 threads: a wave a query row.  part[p][chunk] the focal sum ; cnt[p][chunk] = (rows whose argmax is
// not the last class, matched rows whose argmax is their label)
__global__ __launch_bounds__(256) void set_focal_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                        const int* __restrict__ offsets, int n_targets, const int* __restrict__ match,
                                                        const float* __restrict__ weights, const int* __restrict__ dl_slot,
                                                        float* __restrict__ dlogits, float* __restrict__ dboxes, double* __restrict__ part,
                                                        int* __restrict__ cnt, int B, int nq, int C, int Tmax, float alpha, float inv_nb)
{
    __shared__ int tq[SL_QB];
    __shared__ double wsum[4];
    __shared__ int wcard[4], wcorr[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.y, l = p / B, b = p - l * B, q0 = blockIdx.x * SL_QB;
    if (tid < SL_QB) tq[tid] = -1;
    __syncthreads();
    const SlTargets tg = sl_targets(offsets, b, Tmax, n_targets);
    for (int t = tid; t < tg.T; t += 256) {
        const int q = match[(long)p * Tmax + t];
        if (q >= q0 && q < q0 + SL_QB && q < nq) tq[q - q0] = t;
    }
    __syncthreads();
    const int slot = dl_slot[l];
    float* dl = (slot >= 0 && dlogits) ? dlogits + ((long)slot * B + b) * nq * C : nullptr;
    const float gs = weights[3 * l] * inv_nb;
    const float wa = alpha >= 0.f ? alpha : 1.f, wn = alpha >= 0.f ? 1.f - alpha : 1.f;
    double acc = 0.0;
    int card = 0, corr = 0;
    for (int r = wave; r < SL_QB; r += 4) {
        const int q = q0 + r;
        if (q >= nq) break;                                      // uniform over the wave ; no barrier below
        const int t = tq[r];
        const int tc = t >= 0 ? min(max(labels[tg.t0 + t], 0), C - 1) : -1;
        const float* row = logits + ((long)p * nq + q) * C;
        float s = 0.f, bestv = -__builtin_huge_valf();
        int bestc = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const float x = row[c];
            if (x > bestv) { bestv = x; bestc = c; }
            const float e = expf(-fabsf(x)), d = 1.f / (1.f + e);
            const float pr = x >= 0.f ? d : e * d, np = x >= 0.f ? e * d : d;          // sigmoid(x), 1 - sigmoid(x)
            const float sp = log1pf(e);
            float loss, g;
            if (c == tc) {
                const float ce = fmaxf(-x, 0.f) + sp;                                     // -log p
                loss = wa * ce * (np * np);
                g = -wa * (np * np) * (np + 2.f * pr * ce);
            } else {
                const float ce = fmaxf(x, 0.f) + sp;                                      // -log(1 - p)
                loss = wn * ce * (pr * pr);
                g = wn * (pr * pr) * (pr + 2.f * np * ce);
            }
            s += loss;
            if (dl) dl[(long)q * C + c] = g * gs;
        }
        double sd = (double)s;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sd += __shfl_xor(sd, o, 64);
            const float ov = __shfl_xor(bestv, o, 64);
            const int oc = __shfl_xor(bestc, o, 64);
            if (ov > bestv || (ov == bestv && oc < bestc)) { bestv = ov; bestc = oc; }
        }
        acc += sd;
        card += bestc != C - 1;
        corr += (t >= 0 && bestc == tc);
        if (lane < 4) dboxes[((long)p * nq + q) * 4 + lane] = 0.f;
    }
    if (lane == 0) { wsum[wave] = acc; wcard[wave] = card; wcorr[wave] = corr; }
    __syncthreads();
    if (tid == 0) {
        const long o = (long)p * gridDim.x + blockIdx.x;
        part[o] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        cnt[2 * o] = (wcard[0] + wcard[1]) + (wcard[2] + wcard[3]);
        cnt[2 * o + 1] = (wcorr[0] + wcorr[1]) + (wcorr[2] + wcorr[3]);
    }
}

// the sum of v over the workgroup's 256 threads, in a fixed order, in every thread
__device__ __forceinline__ double sl_block_sum(double v, double* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid L, 256 threads: the matched pairs of output l, and the sums of its partials
__global__ __launch_bounds__(256) void set_pairs_kernel(const float* __restrict__ boxes, const int* __restrict__ offsets,
                                                        const float* __restrict__ tboxes, int n_targets, const int* __restrict__ match,
                                                        const float* __restrict__ weights, const double* __restrict__ part,
                                                        const int* __restrict__ cnt, float* __restrict__ dboxes, float* __restrict__ losses,
                                                        int B, int nq, int Tmax, int nch, double inv_nb)
{
    __shared__ double red[4];
    const int l = blockIdx.x, tid = threadIdx.x;
    const double wb = (double)weights[3 * l + 1] * inv_nb, wg = (double)weights[3 * l + 2] * inv_nb;
    double a_xy = 0.0, a_hw = 0.0, a_g = 0.0, a_ce = 0.0, a_n = 0.0, a_card = 0.0, a_corr = 0.0;
    for (long e = tid; e < (long)B * Tmax; e += 256) {
        const int b = (int)(e / Tmax), t = (int)(e - (long)b * Tmax);
        const SlTargets tg = sl_targets(offsets, b, Tmax, n_targets);
        if (t >= tg.T) continue;
        const long p = (long)l * B + b;
        const int q = match[p * Tmax + t];
        if (q < 0 || q >= nq) continue;
        const float4 sq = *reinterpret_cast<const float4*>(boxes + (p * nq + q) * 4);
        const float* gt = tboxes + 4l * (tg.t0 + t);
        const double s[4] = {(double)sq.x, (double)sq.y, (double)sq.z, (double)sq.w};
        const double g[4] = {(double)gt[0], (double)gt[1], (double)gt[2], (double)gt[3]};
        double dg[4], d[4];
        const double giou = sl_giou(s, g, dg);
        for (int i = 0; i < 4; ++i) {
            const double df = s[i] - g[i];
            d[i] = wb * (df > 0.0 ? 1.0 : (df < 0.0 ? -1.0 : 0.0)) - wg * dg[i];
        }
        a_xy += fabs(s[0] - g[0]) + fabs(s[1] - g[1]);
        a_hw += fabs(s[2] - g[2]) + fabs(s[3] - g[3]);
        a_g += 1.0 - giou;
        a_n += 1.0;
        *reinterpret_cast<float4*>(dboxes + (p * nq + q) * 4) = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
    }
    for (long e = tid; e < (long)B * nch; e += 256) a_ce += part[(long)l * B * nch + e];
    for (int b = tid; b < B; b += 256) {
        long c = 0, k = 0;
        for (int h = 0; h < nch; ++h) {
            c += cnt[2 * (((long)l * B + b) * nch + h)];
            k += cnt[2 * (((long)l * B + b) * nch + h) + 1];
        }
        const int t0 = min(max(offsets[b], 0), n_targets), t1 = min(max(offsets[b + 1], t0), n_targets);
        a_card += fabs((double)c - (double)(t1 - t0));
        a_corr += (double)k;
    }
    a_xy = sl_block_sum(a_xy, red);
    a_hw = sl_block_sum(a_hw, red);
    a_g = sl_block_sum(a_g, red);
    a_ce = sl_block_sum(a_ce, red);
    a_n = sl_block_sum(a_n, red);
    a_card = sl_block_sum(a_card, red);
    a_corr = sl_block_sum(a_corr, red);
    if (tid == 0) {
        float* o = losses + 8l * l;
        o[0] = (float)(a_ce * inv_nb);
        o[1] = (float)((a_xy + a_hw) * inv_nb);
        o[2] = (float)(a_g * inv_nb);
        o[3] = (float)(a_xy * inv_nb);
        o[4] = (float)(a_hw * inv_nb);
        o[5] = (float)(a_card / (double)B);
        o[6] = (float)(a_n > 0.0 ? 100.0 - 100.0 * a_corr / a_n : 100.0);
        o[7] = (float)a_n;
    }
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_set_cost(const float* logits, const float* boxes, const int* labels, const int* offsets, const float* tboxes, int n_targets,
                             int L, int B, int nq, int C, int Tmax, float cost_class, float cost_bbox, float cost_giou, float alpha,
                             float* cost, void* stream)
{
    clear_stale_error();
    if (!logits || !boxes || !offsets || !cost || n_targets < 0 || (n_targets > 0 && (!labels || !tboxes))) return DTLR_EINVAL;
    if (L <= 0 || B <= 0 || nq <= 0 || C <= 0 || Tmax <= 0) return DTLR_EINVAL;
    if ((long)L * B > 65535 || Tmax > SL_TMAX) return DTLR_ESHAPE;
    if (reinterpret_cast<uintptr_t>(boxes) & 15) return DTLR_EINVAL;
    return launch<set_cost_kernel>(dim3((unsigned)((nq + 255) / 256), (unsigned)(L * B)), dim3(256), (size_t)24 * Tmax, (hipStream_t)stream,
                                   logits, boxes, labels, offsets, tboxes, n_targets, B, nq, C, Tmax, (double)cost_class, (double)cost_bbox,
                                   (double)cost_giou, (double)alpha, cost);
}

extern "C" int dtlr_hungarian(const float* cost, const int* sizes, int P, int Rmax, int ncols, int threads, int* match, int* status, void* stream)
{
    clear_stale_error();
    if (!cost || !sizes || !match || !status || P <= 0 || Rmax <= 0 || ncols <= 0) return DTLR_EINVAL;
    if (threads != 0 && threads != 256 && threads != 1024) return DTLR_EINVAL;
    const long NR = Rmax < ncols ? Rmax : ncols, NC = Rmax < ncols ? ncols : Rmax;
    const long lds = ((13 * NR + 25 * NC) + 15) / 16 * 16;
    if (lds > SL_HUNG_LDS) return DTLR_ESHAPE;
    if (threads != 256)
        return launch<hungarian_kernel<1024>>(dim3((unsigned)P), dim3(1024), (size_t)lds, (hipStream_t)stream, cost, sizes, Rmax, ncols, match, status);
    return launch<hungarian_kernel<256>>(dim3((unsigned)P), dim3(256), (size_t)lds, (hipStream_t)stream, cost, sizes, Rmax, ncols, match, status);
}

extern "C" long dtlr_set_loss_workspace_bytes(int L, int B, int nq)
{
    if (L <= 0 || B <= 0 || nq <= 0) return 0;
    const long nch = (nq + SL_QB - 1) / SL_QB;
    return (long)L * B * nch * 16;                                // a double and two ints a (problem, chunk)
}

extern "C" int dtlr_set_loss(const float* logits, const float* boxes, const int* labels, const int* offsets, const float* tboxes, int n_targets,
                             const int* match_q, int L, int B, int nq, int C, int Tmax, float alpha, float num_boxes, const float* weights,
                             const int* dl_slot, float* dlogits, float* dboxes, float* losses, void* workspace, void* stream)
{
    clear_stale_error();
    if (!logits || !boxes || !offsets || !match_q || !weights || !dl_slot || !dboxes || !losses || !workspace) return DTLR_EINVAL;
    if (n_targets < 0 || (n_targets > 0 && (!labels || !tboxes))) return DTLR_EINVAL;
    if (L <= 0 || B <= 0 || nq <= 0 || C <= 0 || Tmax <= 0 || !(num_boxes > 0.f)) return DTLR_EINVAL;
    if ((long)L * B > 65535) return DTLR_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(dboxes)) & 15) return DTLR_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return DTLR_EINVAL;
    const int nch = (nq + SL_QB - 1) / SL_QB;
    double* part = reinterpret_cast<double*>(workspace);
    int* cnt = reinterpret_cast<int*>(part + (long)L * B * nch);
    const double inv_nb = 1.0 / (double)num_boxes;
    if (int rc = launch<set_focal_kernel>(dim3((unsigned)nch, (unsigned)(L * B)), dim3(256), 0, (hipStream_t)stream, logits, labels, offsets,
                                          n_targets, match_q, weights, dl_slot, dlogits, dboxes, part, cnt, B, nq, C, Tmax, alpha,
                                          (float)inv_nb)) return rc;
    return launch<set_pairs_kernel>(dim3((unsigned)L), dim3(256), 0, (hipStream_t)stream, boxes, offsets, tboxes, n_targets, match_q, weights,
                                    part, cnt, dboxes, losses, B, nq, Tmax, nch, inv_nb);
}
