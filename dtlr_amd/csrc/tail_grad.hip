// Gradient of the decoder's tail with the trunk frozen (dtlr_amd/adapt.py train=("tail", ..), DESIGN.md section 22;
// include/dtlr_tailgrad.h states the entry points):
//     u --FFN(linear1, ReLU, linear2)--> + u --norm3--> t --decoder.norm--> h --class_embed / bbox_embed--> outputs
//   dtlr_head_dx        dh (+)= dlogits W                               the class head's input gradient
//   dtlr_box_mlp_dx     dh[rows] += the box MLP's input gradient        on the matched rows (the matcher's list)
//   dtlr_ln_backward    dx, dgamma, dbeta of a LayerNorm over 256       decoder.norm, then norm3
//   dtlr_ffn_recompute  h = relu(W1 u + b1), y = u + W2 h + b2          fp32, from the master weights
//   dtlr_ffn_grad       [dW1 | db1 | dW2 | db2]
// Two routines carry all of it.
//   * tg_rows_gemm_kernel: out[M, N] = epilogue(A[M, K] Wt[K, N]), one workgroup a tile of 32 rows x 256 columns, thread n one column for
//     the 32 rows.  A goes to LDS 32 k at a time, transposed ([k][row]), and is broadcast from there; the weight is read k-major,
//     coalesced over n (W of the class head, W2 of the FFN and W0 / W1 of the box MLP ARE k-major for their input gradients; the
//     forward products read transposes made in the workspace by grad_rows.h's gr_transpose, the kernel the cross-attention and
//     self-attention gradients use too).  32 terms in an fp32 accumulator, those stages in an fp64 one.
//     The products are plain fp32 FMAs: exact fp32 products, the reason DESIGN section 11 gives.
//   * hg_partial_tile / hg_reduce (head_grad_tile.h) for the two d^T x products of the FFN, whose reduction runs over M.
// The LayerNorm backward is one wavefront a row; its column sums are taken 32 rows at a time in fp32 by each wavefront, then in fp64,
// and the workgroups' partials are added in workgroup order by a second kernel.  No float atomics anywhere.
#include "dtlr_common.h"
#include "grad_rows.h"
#include "head_grad_tile.h"
#include "../../include/dtlr_tailgrad.h"

namespace dtlr {

static_assert(GR_D == DTLR_TAIL_HIDDEN && GR_TR == HG_MK, "one thread a column, one stage 32 rows");

// out[m][n] = epi(sum_k A[m][k] Wt[k][n] + bias[n] + res[m][n]) ; epi: ReLU (relu), zero where mask[m][n] <= 0 (mask, pitch ldo), added
// to what out holds (accumulate).  A [M, K] pitch K (a_h16: 16-bit), res [M, N] pitch N (res_h16).  grid (ceil(M / 32), ceil(N / 256)).
__global__ __launch_bounds__(256) void tg_rows_gemm_kernel(const void* __restrict__ A, int a_h16, long M, int K, const float* __restrict__ Wt,
                                                           long ldw, int N, const float* __restrict__ bias, const void* __restrict__ res,
                                                           int res_h16, const float* __restrict__ mask, float* out, long ldo, int relu,
                                                           int accumulate)
{
    __shared__ __attribute__((aligned(16))) float As[32 * GR_LD];
    const long m0 = (long)blockIdx.x * GR_TR;
    const int n = (int)blockIdx.y * 256 + threadIdx.x;
    const bool nvalid = n < N;
    const int sr = threadIdx.x >> 3, sk = (threadIdx.x & 7) * 4;                 // staging: row sr, columns sk .. sk + 3 of the chunk
    const long sm = m0 + sr;
    double acc[GR_TR];
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) acc[r] = 0.0;
    for (int kc = 0; kc < K; kc += 32) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kc + sk + j;
            As[(sk + j) * GR_LD + sr] = (sm < M && k < K) ? gr_load(A, a_h16, sm * K + k) : 0.f;
        }
        __syncthreads();
        gr_mac<double, true, long>(Wt + (long)kc * ldw, ldw, n, nvalid, As, 32, K - kc, acc);
    }
    if (!nvalid) return;
    const double bn = bias ? (double)bias[n] : 0.0;
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) {                               // fully unrolled: acc stays in registers
        const long m = m0 + r;
        if (m >= M) continue;
        double v = acc[r] + bn;
        if (res) v += (double)gr_load(res, res_h16, m * N + n);
        float f = (float)v;
        if (relu && !(f > 0.f)) f = 0.f;
        if (mask && !(mask[m * ldo + n] > 0.f)) f = 0.f;
        if (accumulate) f += out[m * ldo + n];
        out[m * ldo + n] = f;
    }
}

__global__ __launch_bounds__(256) void tg_cast_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = bf16_to_f32(src[i]);
}

// ------------------------------------------------------------------------------------------------------------ the box MLP's dx
struct TgApps { const void* x[DTLR_TAIL_MAX_APPS]; const float* dz[DTLR_TAIL_MAX_APPS]; float* dh[DTLR_TAIL_MAX_APPS]; };

// grid: one workgroup a tile of 32 list entries of one application ; dynamic LDS 2 x [256][GR_LD] floats
__global__ __launch_bounds__(256) void tg_box_dx_kernel(TgApps apps, const int* __restrict__ rows, long M, long R, long Rpad, int x_h16,
                                                        const float* __restrict__ W0T, const float* __restrict__ b0,
                                                        const float* __restrict__ W1T, const float* __restrict__ b1,
                                                        const float* __restrict__ W0, const float* __restrict__ W1, const float* __restrict__ W2)
{
    extern __shared__ __attribute__((aligned(16))) float tg_lds[];
    float* bufA = tg_lds;
    float* bufB = tg_lds + GR_D * GR_LD;
    __shared__ __attribute__((aligned(16))) float dzs[GR_TR][4];
    __shared__ long ridx[GR_TR];
    const long tile = blockIdx.x, tiles_app = Rpad / GR_TR;
    const int a = (int)(tile / tiles_app), n = threadIdx.x;
    const long k0 = (tile - (long)a * tiles_app) * GR_TR;
    int nz = 0;
    if (n < GR_TR) {
        const long k = k0 + n;
        long idx = -1;
        if (k < R) idx = rows ? (long)rows[(long)a * R + k] : k;
        if (idx < 0 || idx >= M) idx = -1;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx >= 0) d = *reinterpret_cast<const float4*>(apps.dz[a] + idx * 4);
        nz = d.x != 0.f || d.y != 0.f || d.z != 0.f || d.w != 0.f;
        ridx[n] = nz ? idx : -1;                                    // a row without a gradient is neither read nor written
        *reinterpret_cast<float4*>(dzs[n]) = d;
    }
    if (!__syncthreads_or(nz)) return;                              // workgroup-uniform
#pragma unroll 4
    for (int r = 0; r < GR_TR; ++r) {
        const long idx = ridx[r];
        bufA[n * GR_LD + r] = idx >= 0 ? gr_load(apps.x[a], x_h16, idx * GR_D + n) : 0.f;
    }
    __syncthreads();
    double acc[GR_TR];
    unsigned m0 = 0;
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) acc[r] = 0.0;
    gr_mac<double, true, long>(W0T, GR_D, n, true, bufA, GR_D, GR_D, acc);
    {
        const double bn = (double)b0[n];
#pragma unroll
        for (int r = 0; r < GR_TR; ++r) {
            float v = (float)(acc[r] + bn);
            if (v > 0.f) m0 |= 1u << r; else v = 0.f;
            bufB[n * GR_LD + r] = v;
            acc[r] = 0.0;
        }
    }
    __syncthreads();
    gr_mac<double, true, long>(W1T, GR_D, n, true, bufB, GR_D, GR_D, acc);
    {
        const double bn = (double)b1[n];
        const float w20 = W2[n], w21 = W2[GR_D + n], w22 = W2[2 * GR_D + n], w23 = W2[3 * GR_D + n];
#pragma unroll
        for (int r = 0; r < GR_TR; ++r) {
            const bool pos = (float)(acc[r] + bn) > 0.f;
            const float4 d = *reinterpret_cast<const float4*>(dzs[r]);
            const float dh1 = fmaf(d.w, w23, fmaf(d.z, w22, fmaf(d.y, w21, d.x * w20)));
            bufA[n * GR_LD + r] = pos ? dh1 : 0.f;                  // bufA's x was last read before the barrier above
            acc[r] = 0.0;
        }
    }
    __syncthreads();
    gr_mac<double, true, long>(W1, GR_D, n, true, bufA, GR_D, GR_D, acc);               // dh0[r][n] = sum_m W1[m][n] da1[r][m]
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) {
        bufB[n * GR_LD + r] = ((m0 >> r) & 1u) ? (float)acc[r] : 0.f;     // bufB's h0 was last read before the barrier above
        acc[r] = 0.0;
    }
    __syncthreads();
    gr_mac<double, true, long>(W0, GR_D, n, true, bufB, GR_D, GR_D, acc);               // dx[r][n] = sum_m W0[m][n] da0[r][m]
    float* dh = apps.dh[a];
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) {
        const long idx = ridx[r];
        if (idx >= 0) dh[idx * GR_D + n] += (float)acc[r];
    }
}

// ------------------------------------------------------------------------------------------------------------ LayerNorm backward
constexpr int LN_ROUND = 128, LN_MAX_WGS = 1024;                   // a round: 4 wavefronts x 32 rows

template <int H16>
__device__ __forceinline__ void ln_load4(const void* x, long row, int lane, float (&v)[4])
{
    if (H16) {
        const uint2 t = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(x) + row * GR_D + 4 * lane);
        v[0] = h16_lo(t.x); v[1] = h16_hi(t.x); v[2] = h16_lo(t.y); v[3] = h16_hi(t.y);
    } else {
        const float4 t = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + row * GR_D + 4 * lane);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
}

// workgroup b: rows b rows_wg .. (b + 1) rows_wg - 1 (rows_wg % 128 == 0), wavefront w the rows 32 w .. 32 w + 31 of every round ;
// part[b][0..255] = the workgroup's sum of g xhat, part[b][256..511] = of g (fp64)
template <int H16>
__global__ __launch_bounds__(256) void tg_ln_bwd_kernel(const void* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ g,
                                                        float* __restrict__ dx, long dx_row0, long M, float eps, long rows_wg,
                                                        double* __restrict__ part)
{
    __shared__ double red[4][2 * GR_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float gav[4] = {gamma[4 * lane], gamma[4 * lane + 1], gamma[4 * lane + 2], gamma[4 * lane + 3]};      // gamma may be a view of a flat buffer: no alignment
    double dsg[4] = {0.0, 0.0, 0.0, 0.0}, dsb[4] = {0.0, 0.0, 0.0, 0.0};
    const long base = (long)blockIdx.x * rows_wg;
    for (long rd = 0; rd < rows_wg; rd += LN_ROUND) {
        const long r0 = base + rd + 32 * wave;
        if (r0 >= M) break;                                         // wavefront-uniform
        float sg[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < 32; ++i) {
            const long row = r0 + i;
            if (row >= M) break;
            float v[4];
            ln_load4<H16>(x, row, lane, v);
            const float4 gt = *reinterpret_cast<const float4*>(g + row * GR_D + 4 * lane);
            const float gv[4] = {gt.x, gt.y, gt.z, gt.w};
            const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / GR_D);
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] -= mean; q += v[j] * v[j]; }
            const float rstd = rsqrtf(wave_sum(q) * (1.0f / GR_D) + eps);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] *= rstd; sg[j] = fmaf(gv[j], v[j], sg[j]); sb[j] += gv[j]; }
            if (dx && row >= dx_row0) {
                float qv[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) { qv[j] = gav[j] * gv[j]; s1 += qv[j]; s2 = fmaf(qv[j], v[j], s2); }
                const float m1 = wave_sum(s1) * (1.0f / GR_D), m2 = wave_sum(s2) * (1.0f / GR_D);
                *reinterpret_cast<float4*>(dx + (row - dx_row0) * GR_D + 4 * lane) =
                    make_float4(rstd * (qv[0] - m1 - v[0] * m2), rstd * (qv[1] - m1 - v[1] * m2), rstd * (qv[2] - m1 - v[2] * m2),
                                rstd * (qv[3] - m1 - v[3] * m2));
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { dsg[j] += (double)sg[j]; dsb[j] += (double)sb[j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[wave][4 * lane + j] = dsg[j]; red[wave][GR_D + 4 * lane + j] = dsb[j]; }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * GR_D; c += 256)
        part[(long)blockIdx.x * 2 * GR_D + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

__global__ __launch_bounds__(256) void tg_ln_reduce_kernel(const double* __restrict__ part, int nwg, float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    const int c = blockIdx.x * 256 + threadIdx.x;                   // grid 2: c < 512
    double a = 0.0;
    for (int b = 0; b < nwg; ++b) a += part[(long)b * 2 * GR_D + c];
    if (c < GR_D) dgamma[c] = (float)a; else dbeta[c - GR_D] = (float)a;
}

struct LnPlan { long rows_wg; int nwg; };
static inline LnPlan ln_plan(long M)
{
    LnPlan p;
    const long rounds = (M + LN_ROUND - 1) / LN_ROUND;
    const long per = (rounds + LN_MAX_WGS - 1) / LN_MAX_WGS;
    p.rows_wg = per * LN_ROUND;
    p.nwg = (int)((rounds + per - 1) / per);
    return p;
}

// ------------------------------------------------------------------------------------------------------------ the FFN's gradient
struct TgProb { const float* G; const float* X; float* part; double* partb; int C, D; };

// grid (tiles, splits, 2): dW1 = da^T u (C = F, D = 256) and dW2 = dy^T h (C = 256, D = F): both 4 F / 64 tiles
__global__ __launch_bounds__(256) void tg_ffn_partial_kernel(TgProb p0, TgProb p1, long M, long chunk)
{
    __shared__ __attribute__((aligned(16))) float Gs[HG_MK][HG_TC];
    __shared__ __attribute__((aligned(16))) float Xs[HG_MK][HG_TD];
    const TgProb p = blockIdx.z == 0 ? p0 : p1;
    hg_partial_tile(Gs, Xs, p.G, p.X, p.part, p.partb, nullptr, M, p.C, p.D, p.D / HG_TD, chunk, (int)blockIdx.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(256) void tg_ffn_reduce_kernel(TgProb p0, TgProb p1, float* __restrict__ grad, int splits)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n0 = (long)p0.C * p0.D + p0.C, n1 = (long)p1.C * p1.D + p1.C;
    if (i >= n0 + n1) return;
    const TgProb p = i < n0 ? p0 : p1;
    const long off = i < n0 ? 0 : n0, nW = (long)p.C * p.D;
    hg_reduce(p.part, p.partb, grad + off, grad + off + nW, nW, p.C, splits, i - off);
}

static inline bool tg_ffn_ok(long M, int F) { return M > 0 && M <= 0x7fffffffl && F >= 64 && F <= DTLR_TAIL_MAX_FFN && F % 64 == 0; }

// the workspace of dtlr_ffn_grad
struct FgWs { float *da, *u32, *part0, *part1; double *pb0, *pb1; long bytes; };
static inline FgWs fg_ws(float* ws, long M, int F, bool cast, int splits)
{
    FgWs w;
    float* p = ws;
    w.da = p; p += M * F;                                        // FIRST: include/dtlr_tailgrad.h promises da at the workspace's head
    w.u32 = p; p += cast ? (M * GR_D + 3) / 4 * 4 : 0;
    w.part0 = p; p += (long)splits * F * GR_D;
    w.part1 = p; p += (long)splits * F * GR_D;                    // every count above is a multiple of 4 floats: p stays 16-byte aligned
    double* q = reinterpret_cast<double*>(p);
    w.pb0 = q; q += (long)splits * F;
    w.pb1 = q; q += (long)splits * GR_D;
    w.bytes = (long)(reinterpret_cast<char*>(q) - reinterpret_cast<char*>(ws));
    return w;
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_head_dx(const float* G, const float* W, float* dh, long M, int C, int accumulate, void* stream)
{
    clear_stale_error();
    if (!G || !W || !dh || M <= 0 || C <= 0) return DTLR_EINVAL;
    if (C > DTLR_TAIL_MAX_CLASSES || M > 0x7fffffffl) return DTLR_ESHAPE;
    return launch<tg_rows_gemm_kernel>(dim3(gr_tiles(M), 1), dim3(256), 0, (hipStream_t)stream, (const void*)G, 0, M, C, W, (long)GR_D, GR_D,
                                       (const float*)nullptr, (const void*)nullptr, 0, (const float*)nullptr, dh, (long)GR_D, 0, accumulate != 0);
}

static inline long tg_box_rpad(int A, long M, int R)
{
    if (A < 1 || A > DTLR_TAIL_MAX_APPS || M <= 0 || M > 0x7fffffffl) return 0;
    const long r = R > 0 ? (long)R : M;
    const long rpad = (r + GR_TR - 1) / GR_TR * GR_TR;
    return (long)A * rpad > 0x7fffffffl ? 0 : rpad;
}

extern "C" long dtlr_box_mlp_dx_workspace_bytes(int A, long M, int R)
{
    return tg_box_rpad(A, M, R) ? 2l * GR_D * GR_D * (long)sizeof(float) : 0;
}

extern "C" int dtlr_box_mlp_dx(const void* x_ptrs, const void* dz_ptrs, const void* dh_ptrs, const int* rows, int A, long M, int R, int x_dtype,
                               const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, void* workspace, void* stream)
{
    clear_stale_error();
    if (!x_ptrs || !dz_ptrs || !dh_ptrs || !W0 || !b0 || !W1 || !b1 || !W2 || !workspace) return DTLR_EINVAL;
    if (A < 1 || M <= 0 || (rows && R <= 0)) return DTLR_EINVAL;
    if (!is_f32_or_h16(x_dtype)) return DTLR_EDTYPE;
    const long rpad = tg_box_rpad(A, M, rows ? R : 0);
    if (!rpad) return DTLR_ESHAPE;
    if (misaligned(workspace, 15)) return DTLR_EINVAL;
    TgApps apps{};
    for (int a = 0; a < A; ++a) {
        apps.x[a] = static_cast<const void* const*>(x_ptrs)[a];
        apps.dz[a] = static_cast<const float* const*>(dz_ptrs)[a];
        apps.dh[a] = static_cast<float* const*>(dh_ptrs)[a];
        if (!apps.x[a] || !apps.dz[a] || !apps.dh[a] || misaligned(apps.dz[a], 15) || misaligned(apps.dh[a], 3)) return DTLR_EINVAL;
        if (misaligned(apps.x[a], x_dtype == DTLR_F32 ? 3 : 1)) return DTLR_EINVAL;
    }
    float* W0T = static_cast<float*>(workspace);
    float* W1T = W0T + GR_D * GR_D;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = gr_transpose(W0, W0T, GR_D, GR_D, st)) return rc;
    if (int rc = gr_transpose(W1, W1T, GR_D, GR_D, st)) return rc;
    const size_t lds = (size_t)2 * GR_D * GR_LD * sizeof(float);
    return launch<tg_box_dx_kernel>(dim3((unsigned)((long)A * rpad / GR_TR)), dim3(256), lds, st, apps, rows, M, rows ? (long)R : M, rpad,
                                    (int)(x_dtype != DTLR_F32), (const float*)W0T, b0, (const float*)W1T, b1, W0, W1, W2);
}

extern "C" long dtlr_ln_backward_workspace_bytes(long M)
{
    if (M <= 0 || M > (1l << 40)) return 0;
    return (long)ln_plan(M).nwg * 2 * GR_D * (long)sizeof(double);
}

extern "C" int dtlr_ln_backward(const void* x, int x_dtype, const float* gamma, const float* g, float* dx, long dx_row0, float* dgamma,
                                float* dbeta, long M, float eps, void* workspace, void* stream)
{
    clear_stale_error();
    if (!x || !gamma || !g || !dgamma || !dbeta || !workspace || M <= 0 || dx_row0 < 0) return DTLR_EINVAL;
    if (!is_f32_or_h16(x_dtype)) return DTLR_EDTYPE;
    if (M > (1l << 40)) return DTLR_ESHAPE;
    if (misaligned(x, x_dtype == DTLR_F32 ? 15 : 7) || misaligned(gamma, 3) || misaligned(g, 15) || misaligned(dx, 15) || misaligned(workspace, 15)) return DTLR_EINVAL;
    const LnPlan p = ln_plan(M);
    const hipStream_t st = (hipStream_t)stream;
    int rc;
    if (x_dtype == DTLR_F32)
        rc = launch<tg_ln_bwd_kernel<0>>(dim3((unsigned)p.nwg), dim3(256), 0, st, x, gamma, g, dx, dx_row0, M, eps, p.rows_wg, (double*)workspace);
    else
        rc = launch<tg_ln_bwd_kernel<1>>(dim3((unsigned)p.nwg), dim3(256), 0, st, x, gamma, g, dx, dx_row0, M, eps, p.rows_wg, (double*)workspace);
    if (rc) return rc;
    return launch<tg_ln_reduce_kernel>(dim3(2), dim3(256), 0, st, (const double*)workspace, p.nwg, dgamma, dbeta);
}

extern "C" long dtlr_ffn_recompute_workspace_bytes(long M, int F)
{
    return tg_ffn_ok(M, F) ? 2l * F * GR_D * (long)sizeof(float) : 0;
}

extern "C" int dtlr_ffn_recompute(const void* u, int u_dtype, const float* W1, const float* b1, const float* W2, const float* b2, float* h,
                                  float* y, long M, int F, void* workspace, void* stream)
{
    clear_stale_error();
    if (!u || !W1 || !b1 || !W2 || !b2 || !h || !y || !workspace || M <= 0 || F <= 0) return DTLR_EINVAL;
    if (!is_f32_or_h16(u_dtype)) return DTLR_EDTYPE;
    if (!tg_ffn_ok(M, F)) return DTLR_ESHAPE;
    if (misaligned(u, u_dtype == DTLR_F32 ? 3 : 1) || misaligned(h, 3) || misaligned(y, 3) || misaligned(workspace, 15)) return DTLR_EINVAL;
    float* W1T = static_cast<float*>(workspace);                   // [256][F]
    float* W2T = W1T + (long)F * GR_D;                              // [F][256]
    const hipStream_t st = (hipStream_t)stream;
    const int h16 = u_dtype != DTLR_F32;
    if (int rc = gr_transpose(W1, W1T, F, GR_D, st)) return rc;
    if (int rc = gr_transpose(W2, W2T, GR_D, F, st)) return rc;
    if (int rc = launch<tg_rows_gemm_kernel>(dim3(gr_tiles(M), (unsigned)((F + 255) / 256)), dim3(256), 0, st, u, h16, M, GR_D, (const float*)W1T,
                                             (long)F, F, b1, (const void*)nullptr, 0, (const float*)nullptr, h, (long)F, 1, 0)) return rc;
    return launch<tg_rows_gemm_kernel>(dim3(gr_tiles(M), 1), dim3(256), 0, st, (const void*)h, 0, M, F, (const float*)W2T, (long)GR_D, GR_D, b2,
                                       u, h16, (const float*)nullptr, y, (long)GR_D, 0, 0);
}

extern "C" long dtlr_ffn_grad_workspace_bytes(long M, int F, int u_dtype)
{
    if (!tg_ffn_ok(M, F) || !is_f32_or_h16(u_dtype)) return 0;
    return fg_ws(nullptr, M, F, u_dtype != DTLR_F32, hg_plan(M, F, GR_D).splits).bytes;
}

extern "C" int dtlr_ffn_grad(const void* u, int u_dtype, const float* h, const float* dy, const float* W2, float* grad, long M, int F,
                             void* workspace, void* stream)
{
    clear_stale_error();
    if (!u || !h || !dy || !W2 || !grad || !workspace || M <= 0 || F <= 0) return DTLR_EINVAL;
    if (!is_f32_or_h16(u_dtype)) return DTLR_EDTYPE;
    if (!tg_ffn_ok(M, F)) return DTLR_ESHAPE;
    if (misaligned(u, u_dtype == DTLR_F32 ? 15 : 1) || misaligned(h, 15) || misaligned(dy, 15) || misaligned(grad, 3) || misaligned(workspace, 15)) return DTLR_EINVAL;
    const bool cast = u_dtype != DTLR_F32;
    const HgPlan hp = hg_plan(M, F, GR_D);                          // tiles_c tiles_d = 4 F / 64 for both products: one plan
    const FgWs w = fg_ws(static_cast<float*>(workspace), M, F, cast, hp.splits);
    const hipStream_t st = (hipStream_t)stream;
    // da = [h > 0] (dy W2): W2 [256][F] is k-major for this product
    if (int rc = launch<tg_rows_gemm_kernel>(dim3(gr_tiles(M), (unsigned)((F + 255) / 256)), dim3(256), 0, st, (const void*)dy, 0, M, GR_D, W2, (long)F,
                                             F, (const float*)nullptr, (const void*)nullptr, 0, h, w.da, (long)F, 0, 0)) return rc;
    const float* u32 = static_cast<const float*>(u);
    if (cast) {
        const long n = M * GR_D;
        if (int rc = launch<tg_cast_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const uint16_t*>(u), w.u32, n)) return rc;
        u32 = w.u32;
    }
    const TgProb p0{w.da, u32, w.part0, w.pb0, F, GR_D}, p1{dy, h, w.part1, w.pb1, GR_D, F};
    const unsigned tiles = (unsigned)(4 * (F / 64));
    if (int rc = launch<tg_ffn_partial_kernel>(dim3(tiles, (unsigned)hp.splits, 2), dim3(256), 0, st, p0, p1, M, hp.chunk)) return rc;
    const long total = 2l * F * GR_D + F + GR_D;
    return launch<tg_ffn_reduce_kernel>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p0, p1, grad, hp.splits);
}
