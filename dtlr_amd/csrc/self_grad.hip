// Gradient of the last decoder layer's self-attention with everything below it frozen (dtlr_amd/adapt.py train=(.., "cross", "self"),
// DESIGN.md section 24; include/dtlr_selfgrad.h states the entry points):
//     t, p --in_proj--> Q, K (of t + p), V (of t) --softmax(Q K^T / sqrt(32)) V per head--> a --out_proj--> + t --norm2--> s --> the cross block
//   dtlr_self_recompute    x, qkv, a, x0, s in fp32 from the master weights (the attention core is dtlr_mha_forward's exact-fp32 kernel)
//   dtlr_mha_grad          dQ, dK, dV from the gradient at a: the backward of the attention core
// The backward is three kernels on v_mfma_f32_16x16x4_f32, each wavefront owning a 16-row tile of one (batch, head) and walking the
// other side in 16-row tiles, the operands read from global memory (a head's K and V are 115 KB each at L = 900 and stay in L2):
//   sg_mha_stats_kernel    per query: the row maximum m (in log2 units), 1 / sum and Delta = sum_j P_ij dP_ij     (S, dP recomputed)
//   sg_mha_dq_kernel       per 16-query tile over all key tiles:   dQ^T += K^T dS^T                                (S, dP recomputed)
//   sg_mha_dkv_kernel      per 16-key tile over all query tiles:   dV^T += dO^T P,  dK^T += Q^T dS                 (S, dP recomputed)
// As in mha_fwd_f32_kernel a lane feeds ONE float per MFMA (A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15]) and the lane's 8
// contiguous channels are spread over 8 MFMAs.  The accumulator layout D[row = 4 g + r][col = n] of the first product is the B-operand
// layout of the second, so the probabilities go from one to the other in registers; the other operand of the second product is read
// transposed (a lane reads one float, 16 lanes a 64-byte piece of a row).  S and dP are formed by the same MFMA chain in all three
// kernels, so that P = exp2(S c - m) never exceeds 1 and, at L = 1, dS is exactly zero.  No LDS, no atomics; every sum in a fixed order.
// The two row products are grad_rows.h's 32-row tile product (exact fp32 FMAs, 32 terms in fp32, the stages in fp64).
#include "gfx950_prims.h"
#include "grad_rows.h"
#include "../../include/dtlr_selfgrad.h"

namespace dtlr {

static_assert(GR_D == DTLR_SELF_HIDDEN && DTLR_SELF_HEADS * DTLR_SELF_HEAD_DIM == DTLR_SELF_HIDDEN, "8 heads x 32 channels");
constexpr int SG_QKV = 3 * GR_D;                                    // [Q | K | V]

// ------------------------------------------------------------------------------------------------------------ the row products
// out[m][n] = sum_k (A[m][k] + A2[m][k]) Wt[k][n] + bias[n] + res[m][n], K = 256 ; A, A2 (optional), res (optional) in fp32 or the 16-bit
// format ; out has row pitch ldo, out2 (optional, row pitch ldo2) receives the same values ; xsum (optional): receives A + A2 in fp32.
// grid (ceil(M / 32), ceil(N / 256)).
__global__ __launch_bounds__(256) void sg_rows_gemm_kernel(const void* __restrict__ A, const void* __restrict__ A2, int a_h16, long M,
                                                           const float* __restrict__ Wt, int ldw, int N, const float* __restrict__ bias,
                                                           const void* __restrict__ res, int res_h16, float* __restrict__ out, int ldo,
                                                           float* __restrict__ out2, int ldo2, float* __restrict__ xsum)
{
    __shared__ __attribute__((aligned(16))) float As[32 * GR_LD];
    const long m0 = (long)blockIdx.x * GR_TR;
    const int n = (int)blockIdx.y * 256 + threadIdx.x;
    const bool nvalid = n < N;
    const int sr = threadIdx.x >> 3, sk = (threadIdx.x & 7) * 4;
    const long sm = m0 + sr;
    double acc[GR_TR];
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) acc[r] = 0.0;
    for (int kc = 0; kc < GR_D; kc += 32) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kc + sk + j;
            float v = 0.f;
            if (sm < M) {
                v = gr_load(A, a_h16, sm * GR_D + k);
                if (A2) v += gr_load(A2, a_h16, sm * GR_D + k);
                if (xsum && blockIdx.y == 0) xsum[sm * GR_D + k] = v;
            }
            As[(sk + j) * GR_LD + sr] = v;
        }
        __syncthreads();
        gr_mac<double, true, int>(Wt + (long)kc * ldw, ldw, n, nvalid, As, 32, GR_D - kc, acc);
    }
    if (!nvalid) return;
    const double bn = (double)bias[n];
#pragma unroll
    for (int r = 0; r < GR_TR; ++r) {
        const long m = m0 + r;
        if (m >= M) continue;
        double v = acc[r] + bn;
        if (res) v += (double)gr_load(res, res_h16, m * N + n);
        out[m * ldo + n] = (float)v;
        if (out2) out2[m * ldo2 + n] = (float)v;
    }
}

// dst[c][r] = src[r][c], src [R, C]
__global__ __launch_bounds__(256) void sg_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C)
{
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) t[j][tx] = src[(long)(r0 + j) * C + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) dst[(long)(c0 + j) * R + r0 + tx] = t[tx][j];
}

// s = LayerNorm(x) over rows of 256: one wavefront a row, statistics fp32 two-pass (as dtlr_ln_backward takes them)
__global__ __launch_bounds__(256) void sg_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float* __restrict__ s, long M, float eps)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;                                           // wavefront-uniform
    const float4 t = *reinterpret_cast<const float4*>(x + row * GR_D + 4 * lane);
    float v[4] = {t.x, t.y, t.z, t.w};
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / GR_D);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] -= mean; q += v[j] * v[j]; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / GR_D) + eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] * rstd * gamma[4 * lane + j] + beta[4 * lane + j];      // views of a flat buffer: no alignment
    *reinterpret_cast<float4*>(s + row * GR_D + 4 * lane) = make_float4(v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------------------------------------------------ the attention core's backward
// 8 contiguous floats of a row
__device__ __forceinline__ void sg_row8(const float* __restrict__ p, float (&f)[8])
{
    const float4 a = reinterpret_cast<const float4*>(p)[0], c = reinterpret_cast<const float4*>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = c.x; f[5] = c.y; f[6] = c.z; f[7] = c.w;
}
// D[i][j] = sum_d A[i][d] B[j][d], d < 32: lane (g, n) supplies A[n][8 g + e] and B[n][8 g + e], e = 0..7, and receives D[4 g + r][n].
// The one chain every kernel forms S and dP with: the bits of an element do not depend on the kernel.
__device__ __forceinline__ f32x4_t sg_dot32(const float (&a)[8], const float (&b)[8])
{
    f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 8; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], s, 0, 0, 0);
    return s;
}
// the sum over a query's four lane groups (lanes n, n + 16, n + 32, n + 48), in a fixed order
__device__ __forceinline__ float sg_sum_g(float v) { v += __shfl_xor(v, 16, 64); return v + __shfl_xor(v, 32, 64); }
__device__ __forceinline__ float sg_max_g(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); return fmaxf(v, __shfl_xor(v, 32, 64)); }

// stats [3][B H Lp]: m (row maximum of S c, c = log2(e) / sqrt(32)), 1 / sum_j exp2(S_ij c - m_i), Delta_i ; rows L .. Lp - 1: zeros.
// grid (ceil(L / 64), H, B): a wavefront per 16 queries.
__global__ __launch_bounds__(256) void sg_mha_stats_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           long ld, const float* __restrict__ go, int L, int Lp, int H, float c,
                                                           float* __restrict__ stats, long plane)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z, C = H * 32;
    const int q0 = blockIdx.x * 64 + wave * 16;
    if (q0 >= L) return;                                            // wavefront-uniform ; no barrier below
    const long row0 = (long)b * L;
    const int qi = min(q0 + n, L - 1);
    float qf[8], gf[8];
    sg_row8(q + (row0 + qi) * ld + h * 32 + 8 * g, qf);
    sg_row8(go + (row0 + qi) * C + h * 32 + 8 * g, gf);
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int kb = 0; kb < L; kb += 16) {
        const int key = min(kb + n, L - 1);
        float kf[8], vf[8];
        sg_row8(k + (row0 + key) * ld + h * 32 + 8 * g, kf);
        sg_row8(v + (row0 + key) * ld + h * 32 + 8 * g, vf);
        const f32x4_t s = sg_dot32(kf, qf), dp = sg_dot32(vf, gf);      // [key 4 g + r][query n]
        float t[4], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            t[r] = kb + 4 * g + r < L ? __fmul_rn(s[r], c) : -INFINITY;
            mx = fmaxf(mx, t[r]);
        }
        const float m_new = fmaxf(m, sg_max_g(mx));                  // finite: every tile holds a key < L
        const float alpha = exp2f(m - m_new);
        float ps = 0.f, pa = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = exp2f(t[r] - m_new);
            ps += p;
            pa = fmaf(p, dp[r], pa);
        }
        l = fmaf(l, alpha, ps);
        acc = fmaf(acc, alpha, pa);
        m = m_new;
    }
    l = sg_sum_g(l);
    acc = sg_sum_g(acc);
    if (g == 0) {
        const bool valid = q0 + n < L;                              // q0 + n < Lp always
        const float inv = 1.0f / l;
        const long i = ((long)b * H + h) * Lp + q0 + n;
        stats[i] = valid ? m : 0.f;
        stats[plane + i] = valid ? inv : 0.f;
        stats[2 * plane + i] = valid ? acc * inv : 0.f;
    }
}

// dq[query][d] = sum_key dS[query][key] K[key][d] / sqrt(32).  grid (ceil(L / 64), H, B): a wavefront per 16 queries.
__global__ __launch_bounds__(256) void sg_mha_dq_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                        long ld, const float* __restrict__ go, int L, int Lp, int H, float c, float scale,
                                                        const float* __restrict__ stats, long plane, float* __restrict__ dq)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z, C = H * 32;
    const int q0 = blockIdx.x * 64 + wave * 16;
    if (q0 >= L) return;
    const long row0 = (long)b * L;
    const int qi = min(q0 + n, L - 1);
    float qf[8], gf[8];
    sg_row8(q + (row0 + qi) * ld + h * 32 + 8 * g, qf);
    sg_row8(go + (row0 + qi) * C + h * 32 + 8 * g, gf);
    const long si = ((long)b * H + h) * Lp + q0 + n;
    const float m = stats[si], inv = stats[plane + si], delta = stats[2 * plane + si];
    f32x4_t o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int kb = 0; kb < L; kb += 16) {
        const int key = min(kb + n, L - 1);
        float kf[8], vf[8];
        sg_row8(k + (row0 + key) * ld + h * 32 + 8 * g, kf);
        sg_row8(v + (row0 + key) * ld + h * 32 + 8 * g, vf);
        float kt[2][4];                                             // K^T[d = 16 dt + n][key 4 g + r]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* kr = k + (row0 + min(kb + 4 * g + r, L - 1)) * ld + h * 32 + n;
            kt[0][r] = kr[0];
            kt[1][r] = kr[16];
        }
        const f32x4_t s = sg_dot32(kf, qf), dp = sg_dot32(vf, gf);      // [key 4 g + r][query n]
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = kb + 4 * g + r < L ? exp2f(__fmul_rn(s[r], c) - m) * inv : 0.f;
            ds[r] = p * (dp[r] - delta);
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt[dt][r], ds[r], o[dt], 0, 0, 0);
    }
    if (q0 + n < L) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)                              // [d = 16 dt + 4 g + r][query n]
            *reinterpret_cast<float4*>(dq + (row0 + q0 + n) * C + h * 32 + dt * 16 + 4 * g) =
                make_float4(o[dt][0] * scale, o[dt][1] * scale, o[dt][2] * scale, o[dt][3] * scale);
    }
}

// dv[key][d] = sum_query P[query][key] dO[query][d] ;  dk[key][d] = sum_query dS[query][key] Q[query][d] / sqrt(32).
// grid (ceil(L / 64), H, B): a wavefront per 16 keys.
__global__ __launch_bounds__(256) void sg_mha_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                         long ld, const float* __restrict__ go, int L, int Lp, int H, float c, float scale,
                                                         const float* __restrict__ stats, long plane, float* __restrict__ dk,
                                                         float* __restrict__ dv)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z, C = H * 32;
    const int k0 = blockIdx.x * 64 + wave * 16;
    if (k0 >= L) return;
    const long row0 = (long)b * L;
    const int ki = min(k0 + n, L - 1);
    const bool kvalid = k0 + n < L;
    float kf[8], vf[8];
    sg_row8(k + (row0 + ki) * ld + h * 32 + 8 * g, kf);
    sg_row8(v + (row0 + ki) * ld + h * 32 + 8 * g, vf);
    const float* st = stats + ((long)b * H + h) * Lp;
    f32x4_t ok[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, ov[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int qb = 0; qb < L; qb += 16) {
        const int qi = min(qb + n, L - 1);
        float qf[8], gf[8];
        sg_row8(q + (row0 + qi) * ld + h * 32 + 8 * g, qf);
        sg_row8(go + (row0 + qi) * C + h * 32 + 8 * g, gf);
        float qt[2][4], gt[2][4];                                   // Q^T, dO^T [d = 16 dt + n][query 4 g + r]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = row0 + min(qb + 4 * g + r, L - 1);
            const float* qr = q + row * ld + h * 32 + n;
            const float* gr = go + row * C + h * 32 + n;
            qt[0][r] = qr[0]; qt[1][r] = qr[16];
            gt[0][r] = gr[0]; gt[1][r] = gr[16];
        }
        const float4 m4 = *reinterpret_cast<const float4*>(st + qb + 4 * g);               // qb + 4 g + 3 < Lp
        const float4 i4 = *reinterpret_cast<const float4*>(st + plane + qb + 4 * g);
        const float4 d4 = *reinterpret_cast<const float4*>(st + 2 * plane + qb + 4 * g);
        const float mr[4] = {m4.x, m4.y, m4.z, m4.w}, ir[4] = {i4.x, i4.y, i4.z, i4.w}, dr[4] = {d4.x, d4.y, d4.z, d4.w};
        const f32x4_t s = sg_dot32(qf, kf), dp = sg_dot32(gf, vf);      // [query 4 g + r][key n]
        float p[4], ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = (kvalid && qb + 4 * g + r < L) ? exp2f(__fmul_rn(s[r], c) - mr[r]) * ir[r] : 0.f;
            ds[r] = p[r] * (dp[r] - dr[r]);
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ov[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gt[dt][r], p[r], ov[dt], 0, 0, 0);
                ok[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qt[dt][r], ds[r], ok[dt], 0, 0, 0);
            }
    }
    if (kvalid) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {                            // [d = 16 dt + 4 g + r][key n]
            const long i = (row0 + k0 + n) * C + h * 32 + dt * 16 + 4 * g;
            *reinterpret_cast<float4*>(dv + i) = make_float4(ov[dt][0], ov[dt][1], ov[dt][2], ov[dt][3]);
            *reinterpret_cast<float4*>(dk + i) = make_float4(ok[dt][0] * scale, ok[dt][1] * scale, ok[dt][2] * scale, ok[dt][3] * scale);
        }
    }
}

static inline bool sg_mis(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
static inline long sg_lp(long L) { return (L + 15) / 16 * 16; }

}  // namespace dtlr

using namespace dtlr;

extern "C" long dtlr_mha_grad_workspace_bytes(long B, long L, long H)
{
    if (B <= 0 || L <= 0 || H <= 0 || B > 65535 || H > 65535 || B * L * H * 32 >= (1l << 31)) return 0;
    return 3 * B * H * sg_lp(L) * (long)sizeof(float);
}

extern "C" int dtlr_mha_grad(const float* q, const float* k, const float* v, int row_stride, const float* grad_out, int B, int L, int H,
                             int head_dim, float* dq, float* dk, float* dv, void* workspace, void* stream)
{
    clear_stale_error();
    if (!q || !k || !v || !grad_out || !dq || !dk || !dv || !workspace) return DTLR_EINVAL;
    if (B <= 0 || L <= 0 || H <= 0 || head_dim <= 0) return DTLR_EINVAL;
    if (head_dim != DTLR_SELF_HEAD_DIM) return DTLR_ESHAPE;
    if (!dtlr_mha_grad_workspace_bytes(B, L, H)) return DTLR_ESHAPE;
    const int C = H * 32;
    const long ld = row_stride > 0 ? row_stride : C;
    if (ld < C || (ld & 3) || (long)B * L * ld >= (1l << 33)) return DTLR_ESHAPE;
    if (sg_mis(q, 15) || sg_mis(k, 15) || sg_mis(v, 15) || sg_mis(grad_out, 15) || sg_mis(dq, 15) || sg_mis(dk, 15) || sg_mis(dv, 15) ||
        sg_mis(workspace, 15)) return DTLR_EINVAL;
    const int Lp = (int)sg_lp(L);
    const long plane = (long)B * H * Lp;
    float* stats = static_cast<float*>(workspace);
    const float scale = 1.0f / sqrtf((float)head_dim), c = 1.4426950408889634f * scale;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((L + 63) / 64), (unsigned)H, (unsigned)B);
    if (int rc = launch<sg_mha_stats_kernel>(grid, dim3(256), 0, st, q, k, v, ld, grad_out, L, Lp, H, c, stats, plane)) return rc;
    if (int rc = launch<sg_mha_dq_kernel>(grid, dim3(256), 0, st, q, k, v, ld, grad_out, L, Lp, H, c, scale, (const float*)stats, plane, dq)) return rc;
    return launch<sg_mha_dkv_kernel>(grid, dim3(256), 0, st, q, k, v, ld, grad_out, L, Lp, H, c, scale, (const float*)stats, plane, dk, dv);
}

extern "C" long dtlr_self_recompute_workspace_bytes(long B, long L)
{
    if (B <= 0 || L <= 0 || B > 65535 || B * L * SG_QKV >= (1l << 31)) return 0;
    const long M = B * L;
    return ((long)GR_D * SG_QKV + (long)GR_D * GR_D + M * SG_QKV) * (long)sizeof(float) + dtlr_mha_workspace_bytes((int)B, (int)L, DTLR_SELF_HEADS, DTLR_SELF_HEAD_DIM);
}

extern "C" int dtlr_self_recompute(const void* t, const void* p, int x_dtype, int B, int L, const float* Win, const float* bin, const float* Wo,
                                   const float* bo, const float* gamma2, const float* beta2, float eps, float* x, float* qkv, float* a,
                                   float* x0, float* s, void* workspace, void* stream)
{
    clear_stale_error();
    if (!t || !p || !Win || !bin || !Wo || !bo || !gamma2 || !beta2 || !x || !qkv || !a || !x0 || !s || !workspace) return DTLR_EINVAL;
    if (B <= 0 || L <= 0) return DTLR_EINVAL;
    if (x_dtype != DTLR_F32 && x_dtype != DTLR_H16) return DTLR_EDTYPE;
    if (!dtlr_self_recompute_workspace_bytes(B, L)) return DTLR_ESHAPE;
    const long M = (long)B * L;
    if (sg_mis(t, x_dtype == DTLR_F32 ? 3 : 1) || sg_mis(p, x_dtype == DTLR_F32 ? 3 : 1) || sg_mis(x, 15) || sg_mis(qkv, 15) || sg_mis(a, 15) ||
        sg_mis(x0, 15) || sg_mis(s, 15) || sg_mis(workspace, 15)) return DTLR_EINVAL;
    float* WinT = static_cast<float*>(workspace);                   // [256][768]
    float* WoT = WinT + (long)GR_D * SG_QKV;                         // [256][256]
    float* qk = WoT + (long)GR_D * GR_D;                             // [M][512]: the image dtlr_mha_forward reads
    float* vv = qk + M * 2 * GR_D;                                   // [M][256]
    float* vt = vv + M * GR_D;                                       // dtlr_mha_forward's workspace
    const hipStream_t st = (hipStream_t)stream;
    const int h16 = x_dtype != DTLR_F32;
    const unsigned tiles = (unsigned)((M + GR_TR - 1) / GR_TR);
    if (int rc = launch<sg_transpose_kernel>(dim3(GR_D / 32, SG_QKV / 32), dim3(256), 0, st, Win, WinT, SG_QKV, GR_D)) return rc;
    if (int rc = launch<sg_transpose_kernel>(dim3(GR_D / 32, GR_D / 32), dim3(256), 0, st, Wo, WoT, GR_D, GR_D)) return rc;
    if (int rc = launch<sg_rows_gemm_kernel>(dim3(tiles, 2), dim3(256), 0, st, t, p, h16, M, (const float*)WinT, SG_QKV, 2 * GR_D, bin,
                                             (const void*)nullptr, 0, qkv, SG_QKV, qk, 2 * GR_D, x)) return rc;
    if (int rc = launch<sg_rows_gemm_kernel>(dim3(tiles, 1), dim3(256), 0, st, t, (const void*)nullptr, h16, M, (const float*)(WinT + 2 * GR_D), SG_QKV,
                                             GR_D, bin + 2 * GR_D, (const void*)nullptr, 0, qkv + 2 * GR_D, SG_QKV, vv, GR_D, (float*)nullptr)) return rc;
    if (int rc = dtlr_mha_forward(qk, vv, vt, a, B, L, DTLR_SELF_HEADS, DTLR_SELF_HEAD_DIM, DTLR_F32, stream)) return rc;
    if (int rc = launch<sg_rows_gemm_kernel>(dim3(tiles, 1), dim3(256), 0, st, (const void*)a, (const void*)nullptr, 0, M, (const float*)WoT, GR_D, GR_D,
                                             bo, t, h16, x0, GR_D, (float*)nullptr, 0, (float*)nullptr)) return rc;
    return launch<sg_ln_kernel>(dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (const float*)x0, gamma2, beta2, s, M, eps);
}
