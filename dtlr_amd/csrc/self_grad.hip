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
// The weight transposes, the three row products and norm2 are grad_rows.h's launches (gr_transpose, gr_rows_gemm256, gr_layernorm256: the
// kernels cross_grad.hip runs too).
#include "gfx950_prims.h"
#include "grad_rows.h"
#include "../../include/dtlr_selfgrad.h"

namespace dtlr {

static_assert(GR_D == DTLR_SELF_HIDDEN && DTLR_SELF_HEADS * DTLR_SELF_HEAD_DIM == DTLR_SELF_HIDDEN, "8 heads x 32 channels");
constexpr int SG_QKV = 3 * GR_D;                                    // [Q | K | V]

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
    if (misaligned(q, 15) || misaligned(k, 15) || misaligned(v, 15) || misaligned(grad_out, 15) || misaligned(dq, 15) || misaligned(dk, 15) || misaligned(dv, 15) ||
        misaligned(workspace, 15)) return DTLR_EINVAL;
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
    if (!is_f32_or_h16(x_dtype)) return DTLR_EDTYPE;
    if (!dtlr_self_recompute_workspace_bytes(B, L)) return DTLR_ESHAPE;
    const long M = (long)B * L;
    if (misaligned(t, x_dtype == DTLR_F32 ? 3 : 1) || misaligned(p, x_dtype == DTLR_F32 ? 3 : 1) || misaligned(x, 15) || misaligned(qkv, 15) || misaligned(a, 15) ||
        misaligned(x0, 15) || misaligned(s, 15) || misaligned(workspace, 15)) return DTLR_EINVAL;
    float* WinT = static_cast<float*>(workspace);                   // [256][768]
    float* WoT = WinT + (long)GR_D * SG_QKV;                         // [256][256]
    float* qk = WoT + (long)GR_D * GR_D;                             // [M][512]: the image dtlr_mha_forward reads
    float* vv = qk + M * 2 * GR_D;                                   // [M][256]
    float* vt = vv + M * GR_D;                                       // dtlr_mha_forward's workspace
    const hipStream_t st = (hipStream_t)stream;
    const int h16 = x_dtype != DTLR_F32;
    if (int rc = gr_transpose(Win, WinT, SG_QKV, GR_D, st)) return rc;
    if (int rc = gr_transpose(Wo, WoT, GR_D, GR_D, st)) return rc;
    // [Q | K] of t + p, then V of t: both into qkv and into the images dtlr_mha_forward reads
    if (int rc = gr_rows_gemm256({.A = t, .A2 = p, .a_h16 = h16, .M = M, .Wt = WinT, .ldw = SG_QKV, .N = 2 * GR_D, .bias = bin, .out = qkv,
                                  .ldo = SG_QKV, .out2 = qk, .ldo2 = 2 * GR_D, .xsum = x}, st)) return rc;
    if (int rc = gr_rows_gemm256({.A = t, .a_h16 = h16, .M = M, .Wt = WinT + 2 * GR_D, .ldw = SG_QKV, .N = GR_D, .bias = bin + 2 * GR_D,
                                  .out = qkv + 2 * GR_D, .ldo = SG_QKV, .out2 = vv, .ldo2 = GR_D}, st)) return rc;
    if (int rc = dtlr_mha_forward(qk, vv, vt, a, B, L, DTLR_SELF_HEADS, DTLR_SELF_HEAD_DIM, DTLR_F32, stream)) return rc;
    if (int rc = gr_rows_gemm256({.A = a, .M = M, .Wt = WoT, .ldw = GR_D, .N = GR_D, .bias = bo, .res = t, .res_h16 = h16, .out = x0, .ldo = GR_D}, st))
        return rc;
    return gr_layernorm256(x0, gamma2, beta2, s, M, eps, st);
}
