// The d^T x tile routine shared by dtlr_head_grad (head_grad.hip) and dtlr_box_mlp_grad (box_grad.hip):
//   dW[C, D] = G^T[C, M] . X[M, D],  db[C] = sum_m G[m, :]       over rows m0 .. m1 - 1 of one split, one 64 x 64 tile of dW a workgroup.
// Both operands are stored M-major and M is the reduction dimension: a stage of 32 rows of G (64 channels) and of X (64 features) goes
// to LDS as it lies in memory and every thread forms the 4 x 4 outer products of its channels and features.  Products and sums are plain
// fp32 FMAs; a stage's 32 terms are summed in an fp32 accumulator, the stages in an fp64 one.  The split's partial tile (fp32; the bias
// partial fp64) goes to the caller's workspace; hg_reduce adds the splits in split order -- no float atomics.
// live: nullptr, or one int a stage of 32 rows (rows 32 s .. 32 s + 31, splits are whole stages): a stage whose entry is 0 is skipped
// -- its rows are never read, so they need not be initialised.  A skipped stage adds nothing, exactly what a stage of zero rows of G adds.
#pragma once
#include "dtlr_common.h"

namespace dtlr {

constexpr int HG_TC = 64, HG_TD = 64, HG_MK = 32, HG_MAX_SPLITS = 64;

struct HgPlan { int tiles_c, tiles_d, splits; long chunk; };
static inline HgPlan hg_plan(long M, int C, int D)
{
    HgPlan p;
    p.tiles_c = (C + HG_TC - 1) / HG_TC;
    p.tiles_d = D / HG_TD;
    long want = 1024 / ((long)p.tiles_c * p.tiles_d);
    if (want < 1) want = 1;
    if (want > HG_MAX_SPLITS) want = HG_MAX_SPLITS;
    long chunk = (M + want - 1) / want;
    chunk = ((chunk + HG_MK - 1) / HG_MK) * HG_MK;
    p.chunk = chunk;
    p.splits = (int)((M + chunk - 1) / chunk);
    return p;
}

// workgroup (tile, split) of 256 threads: part[split][C][D] and partb[split][C].  Gs / Xs: the caller's LDS stages.
__device__ __forceinline__ void hg_partial_tile(float (&Gs)[HG_MK][HG_TC], float (&Xs)[HG_MK][HG_TD], const float* __restrict__ G,
                                                const float* __restrict__ X, float* __restrict__ part, double* __restrict__ partb,
                                                const int* __restrict__ live, long M, int C, int D, int tiles_d, long chunk, int tile, int split)
{
    const int tc = tile / tiles_d, td = tile - tc * tiles_d;
    const int cbase = tc * HG_TC, dbase = td * HG_TD;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;                     // features 4 tx .. 4 tx + 3, channels 4 ty .. 4 ty + 3
    const long m0 = (long)split * chunk;
    const long m1 = m0 + chunk < M ? m0 + chunk : M;
    double acc[4][4], accb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { accb[i] = 0.0; for (int j = 0; j < 4; ++j) acc[i][j] = 0.0; }
    for (long ms = m0; ms < m1; ms += HG_MK) {
        if (live && !live[ms / HG_MK]) continue;                                // workgroup-uniform
        __syncthreads();
#pragma unroll
        for (int u = 0; u < HG_MK * HG_TC / 256; ++u) {                         // G: scalar loads (rows of C floats have no alignment)
            const int e = u * 256 + threadIdx.x, r = e >> 6, c = e & 63;
            const long m = ms + r;
            Gs[r][c] = (m < m1 && cbase + c < C) ? G[m * C + cbase + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < HG_MK * HG_TD / 4 / 256; ++u) {                     // X: rows of D floats, D % 64 == 0
            const int e = u * 256 + threadIdx.x, r = e >> 4, d4 = e & 15;
            const long m = ms + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < m1) v = *reinterpret_cast<const float4*>(X + m * D + dbase + 4 * d4);
            *reinterpret_cast<float4*>(&Xs[r][4 * d4]) = v;
        }
        __syncthreads();
        float a[4][4], ab[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { ab[i] = 0.f; for (int j = 0; j < 4; ++j) a[i][j] = 0.f; }
#pragma unroll 8
        for (int r = 0; r < HG_MK; ++r) {
            const float4 g = *reinterpret_cast<const float4*>(&Gs[r][4 * ty]);
            const float4 x = *reinterpret_cast<const float4*>(&Xs[r][4 * tx]);
            const float gv[4] = {g.x, g.y, g.z, g.w}, xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ab[i] += gv[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) a[i][j] = fmaf(gv[i], xv[j], a[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { accb[i] += (double)ab[i]; for (int j = 0; j < 4; ++j) acc[i][j] += (double)a[i][j]; }
    }
    float* po = part + (long)split * C * D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cbase + 4 * ty + i;
        if (c < C) {
            *reinterpret_cast<float4*>(po + (long)c * D + dbase + 4 * tx) = make_float4((float)acc[i][0], (float)acc[i][1], (float)acc[i][2], (float)acc[i][3]);
            if (td == 0 && tx == 0) partb[(long)split * C + c] = accb[i];
        }
    }
}

// element i of [dW (nW = C D) | db (C)] = the partials added in split order
__device__ __forceinline__ void hg_reduce(const float* __restrict__ part, const double* __restrict__ partb, float* __restrict__ dW,
                                          float* __restrict__ db, long nW, int C, int splits, long i)
{
    if (i < nW) {
        double a = 0.0;
        for (int s = 0; s < splits; ++s) a += (double)part[(long)s * nW + i];
        dW[i] = (float)a;
    } else if (i < nW + C) {
        const long c = i - nW;
        double a = 0.0;
        for (int s = 0; s < splits; ++s) a += partb[(long)s * C + c];
        db[c] = (float)a;
    }
}

}  // namespace dtlr
