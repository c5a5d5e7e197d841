// Gradient of the last decoder layer's deformable cross-attention with everything below it frozen (dtlr_amd/adapt.py
// train=(.., "tail", "cross"); include/dtlr_crossgrad.h states the entry points):
//     s, p --[sampling_offsets ; attention_weights]--> off, A --> loc --sampling of V--> o --output_proj--> + s --norm1--> u --> the tail
//   dtlr_cross_recompute   qin, A, loc, o, x1, u in fp32 from the master weights
//   dtlr_msda_query_grad   grad_loc, grad_attn from the gradient at o: the two gathers of the deformable attention's backward
//   dtlr_cross_dow         the softmax's and the offsets' backward: the gradient at the projection's output
// The sampling kernels keep msda.hip's forward mapping: a head's 32 channels lie in adjacent lanes (8 lanes x 4 fp32 channels, or 4
// lanes x 8 16-bit channels), so every corner is one 16-byte load and a head's lanes read one contiguous pixel row.  The loads are
// branch-free: an address is clamped into the map and an invalid corner gets a zero weight (msda.hip gives the measurements behind
// that).  The gradient kernel forms, per lane, the partial dot products of its channels with the four corners, combines them into the
// three outputs of a point, and folds the 48 values of a head over its lanes by a transposing butterfly of fixed order: after
// log2(lanes) exchange steps lane j holds the finished sums 48 / lanes * j .., and stores them.  No atomics, no LDS.
// The weight transposes, the two row products and norm1 are grad_rows.h's launches (gr_transpose, gr_rows_gemm256, gr_layernorm256: the
// kernels self_grad.hip runs too) ; the level table, the point and its corners are msda_grad_geo.h's, shared with msda_value_grad.hip.
#include "gfx950_prims.h"
#include "grad_rows.h"
#include "msda_grad_geo.h"
#include "../../include/dtlr_crossgrad.h"

namespace dtlr {

static_assert(GR_D == DTLR_CROSS_HIDDEN && DTLR_CROSS_HEADS * DTLR_CROSS_HEAD_DIM == DTLR_CROSS_HIDDEN, "8 heads x 32 channels");
constexpr int CG_OW = 384;                                          // [offsets 8 x 4 x 4 x 2 | logits 8 x 16]

// VEC channels of one corner: one 16-byte load
template <typename T> struct CgVec;
template <> struct CgVec<float> {
    static constexpr int VEC = 4;
    using raw_t = float4;
    static __device__ __forceinline__ raw_t ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ void unpack(const raw_t& t, float (&v)[4]) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
};
template <> struct CgVec<uint16_t> {
    static constexpr int VEC = 8;
    using raw_t = uint4;
    static __device__ __forceinline__ raw_t ld(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }
    static __device__ __forceinline__ void unpack(const raw_t& t, float (&v)[8]) { unpack8_h16(t, v); }
};

// ------------------------------------------------------------------------------------------------------------ the forward, fp32 out
// thread: VEC channels of one (row, head).  ow [M,384] fp32 ; R [M,16] ; A [M,8,16], loc [M,8,32] (written by the head's first lane),
// o [M,256].  total = M * 8 * (32 / VEC): a head is never split.
template <typename T>
__global__ __launch_bounds__(256) void cg_attend_kernel(const T* __restrict__ value, const long* __restrict__ shapes, const long* __restrict__ lsi,
                                                        const float* __restrict__ ow, const float* __restrict__ R, int S, int Lq, int vstride,
                                                        float* __restrict__ A, float* __restrict__ loc, float* __restrict__ o, long total)
{
    using V = CgVec<T>;
    constexpr int VEC = V::VEC, LPH = 32 / VEC;
    const long tid = (long)blockIdx.x * 256 + threadIdx.x;
    if (tid >= total) return;
    const int sub = (int)(tid % LPH);
    const long si = tid / LPH;                                      // row * 8 + head
    const int m = (int)(si & 7);
    const long bq = si >> 3, b = bq / Lq;
    const GeoLevels lv = geo_levels(shapes, lsi, S);
    const float* row = ow + bq * CG_OW;
    float off[32], lg[16], rf[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float4 t = reinterpret_cast<const float4*>(row + m * 32)[i];
        off[4 * i] = t.x; off[4 * i + 1] = t.y; off[4 * i + 2] = t.z; off[4 * i + 3] = t.w; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float4 t = reinterpret_cast<const float4*>(row + 256 + m * 16)[i];
        lg[4 * i] = t.x; lg[4 * i + 1] = t.y; lg[4 * i + 2] = t.z; lg[4 * i + 3] = t.w; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float4 t = reinterpret_cast<const float4*>(R + bq * 16)[i];
        rf[4 * i] = t.x; rf[4 * i + 1] = t.y; rf[4 * i + 2] = t.z; rf[4 * i + 3] = t.w; }
    float mx = lg[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, lg[i]);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { lg[i] = expf(lg[i] - mx); sum += lg[i]; }
#pragma unroll
    for (int i = 0; i < 16; ++i) lg[i] = lg[i] / sum;
    float lc[32];
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            // the reference's operation order (ms_deform_attn.py:112-114), each step rounded on its own: / 4 and * 0.5 are exact, the
            // product with the box size and the final sum are written with the non-contracting intrinsics
            lc[(l * 4 + p) * 2] = __fadd_rn(rf[4 * l], __fmul_rn(__fmul_rn(off[(l * 4 + p) * 2] * 0.25f, rf[4 * l + 2]), 0.5f));
            lc[(l * 4 + p) * 2 + 1] = __fadd_rn(rf[4 * l + 1], __fmul_rn(__fmul_rn(off[(l * 4 + p) * 2 + 1] * 0.25f, rf[4 * l + 3]), 0.5f));
        }
    if (sub == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) reinterpret_cast<float4*>(A + si * 16)[i] = make_float4(lg[4 * i], lg[4 * i + 1], lg[4 * i + 2], lg[4 * i + 3]);
#pragma unroll
        for (int i = 0; i < 8; ++i) reinterpret_cast<float4*>(loc + si * 32)[i] = make_float4(lc[4 * i], lc[4 * i + 1], lc[4 * i + 2], lc[4 * i + 3]);
    }
    const T* vb = value + b * (long)S * vstride + m * 32 + sub * VEC;
    float col[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) col[i] = 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        typename V::raw_t d[4][4];
        float wgt[4][4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const GeoCorners g = geo_corners(geo_point(lc[(l * 4 + p) * 2], lc[(l * 4 + p) * 2 + 1], lv.H[l], lv.W[l]), lv.H[l], lv.W[l], lv.st[l], S, vstride);
#pragma unroll
            for (int c = 0; c < 4; ++c) d[p][c] = V::ld(vb + g.o[c]);
            wgt[p][0] = g.wy0 * g.wx0; wgt[p][1] = g.wy0 * g.wx1; wgt[p][2] = g.wy1 * g.wx0; wgt[p][3] = g.wy1 * g.wx1;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
            V::unpack(d[p][0], v0); V::unpack(d[p][1], v1); V::unpack(d[p][2], v2); V::unpack(d[p][3], v3);
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                col[i] += (wgt[p][0] * v0[i] + wgt[p][1] * v1[i] + wgt[p][2] * v2[i] + wgt[p][3] * v3[i]) * lg[l * 4 + p];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < VEC; i += 4) *reinterpret_cast<float4*>(o + si * 32 + sub * VEC + i) = make_float4(col[i], col[i + 1], col[i + 2], col[i + 3]);
}

// ------------------------------------------------------------------------------------------------------------ the two query gradients
// one exchange step of the transposing butterfly: the N live values of v become N / 2, each the sum of this lane's and of lane ^ MASK's
template <int N, int MASK>
__device__ __forceinline__ void cg_fold(float (&v)[48], int sub)
{
    const bool up = (sub & MASK) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const float keep = up ? v[i + N / 2] : v[i];
        const float send = up ? v[i] : v[i + N / 2];
        v[i] = keep + __shfl_xor(send, MASK, 64);
    }
}

// thread: VEC channels of one (row, head) ; v[0..31]: grad_loc of the head's 16 points (x, y), v[32..47]: grad_attn
template <typename T>
__global__ __launch_bounds__(256) void cg_query_grad_kernel(const T* __restrict__ value, const long* __restrict__ shapes, const long* __restrict__ lsi,
                                                            const float* __restrict__ loc, const float* __restrict__ attn,
                                                            const float* __restrict__ go, int S, int Lq, int vstride,
                                                            float* __restrict__ gloc, float* __restrict__ gattn, long total)
{
    using V = CgVec<T>;
    constexpr int VEC = V::VEC, LPH = 32 / VEC, NOUT = 48 / LPH;
    const long tid0 = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = tid0 < total;                                 // a head's lanes are live together (total % LPH == 0) ; the others follow the
    const long tid = live ? tid0 : total - 1;                       // last thread through the exchanges and store nothing
    const int sub = (int)(tid % LPH);
    const long si = tid / LPH;
    const int m = (int)(si & 7);
    const long b = (si >> 3) / Lq;
    const GeoLevels lv = geo_levels(shapes, lsi, S);
    float4 lq[8], aq[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) lq[i] = reinterpret_cast<const float4*>(loc + si * 32)[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) aq[i] = reinterpret_cast<const float4*>(attn + si * 16)[i];
    float g[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i += 4) { const float4 t = *reinterpret_cast<const float4*>(go + si * 32 + sub * VEC + i);
        g[i] = t.x; g[i + 1] = t.y; g[i + 2] = t.z; g[i + 3] = t.w; }
    const T* vb = value + b * (long)S * vstride + m * 32 + sub * VEC;
    float v[48];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const float a[4] = {aq[l].x, aq[l].y, aq[l].z, aq[l].w};
        const float lx[4] = {lq[2 * l].x, lq[2 * l].z, lq[2 * l + 1].x, lq[2 * l + 1].z};
        const float ly[4] = {lq[2 * l].y, lq[2 * l].w, lq[2 * l + 1].y, lq[2 * l + 1].w};
        typename V::raw_t d[4][4];
        GeoCorners geo[4];
        GeoPoint pt[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            pt[p] = geo_point(lx[p], ly[p], lv.H[l], lv.W[l]);
            geo[p] = geo_corners(pt[p], lv.H[l], lv.W[l], lv.st[l], S, vstride);
#pragma unroll
            for (int c = 0; c < 4; ++c) d[p][c] = V::ld(vb + geo[p].o[c]);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float dot[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float t[VEC];
                V::unpack(d[p][c], t);
                float s = g[0] * t[0];
#pragma unroll
                for (int i = 1; i < VEC; ++i) s = fmaf(g[i], t[i], s);
                dot[c] = s;
            }
            const GeoCorners& q = geo[p];
            const float da = q.wy0 * (q.wx0 * dot[0] + q.wx1 * dot[1]) + q.wy1 * (q.wx0 * dot[2] + q.wx1 * dot[3]);
            const float dx = q.wy0 * (q.mx1 * dot[1] - q.mx0 * dot[0]) + q.wy1 * (q.mx1 * dot[3] - q.mx0 * dot[2]);
            const float dy = q.wx0 * (q.my1 * dot[2] - q.my0 * dot[0]) + q.wx1 * (q.my1 * dot[3] - q.my0 * dot[1]);
            v[(l * 4 + p) * 2] = pt[p].inside ? a[p] * (float)lv.W[l] * dx : 0.f;
            v[(l * 4 + p) * 2 + 1] = pt[p].inside ? a[p] * (float)lv.H[l] * dy : 0.f;
            v[32 + l * 4 + p] = pt[p].inside ? da : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (LPH == 8) { cg_fold<48, 4>(v, sub); cg_fold<24, 2>(v, sub); cg_fold<12, 1>(v, sub); }
    else { cg_fold<48, 2>(v, sub); cg_fold<24, 1>(v, sub); }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
        const int idx = NOUT * sub + i;
        if (idx < 32) gloc[si * 32 + idx] = v[i]; else gattn[si * 16 + idx - 32] = v[i];
    }
}

// ------------------------------------------------------------------------------------------------------------ softmax / offsets backward
// thread: one (row, head)
__global__ __launch_bounds__(256) void cg_dow_kernel(const float* __restrict__ A, const float* __restrict__ dA, const float* __restrict__ dloc,
                                                     const float* __restrict__ R, float* __restrict__ doff, float* __restrict__ dlogit, long total)
{
    const long si = (long)blockIdx.x * 256 + threadIdx.x;
    if (si >= total) return;
    const long row = si >> 3;
    const int h = (int)(si & 7);
    float a[16], da[16], rf[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 t = reinterpret_cast<const float4*>(A + si * 16)[i], u = reinterpret_cast<const float4*>(dA + si * 16)[i];
        const float4 r = reinterpret_cast<const float4*>(R + row * 16)[i];
        a[4 * i] = t.x; a[4 * i + 1] = t.y; a[4 * i + 2] = t.z; a[4 * i + 3] = t.w;
        da[4 * i] = u.x; da[4 * i + 1] = u.y; da[4 * i + 2] = u.z; da[4 * i + 3] = u.w;
        rf[4 * i] = r.x; rf[4 * i + 1] = r.y; rf[4 * i + 2] = r.z; rf[4 * i + 3] = r.w;
    }
    float dotp = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) dotp = fmaf(a[i], da[i], dotp);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        reinterpret_cast<float4*>(dlogit + row * 128 + h * 16)[i] = make_float4(a[4 * i] * (da[4 * i] - dotp), a[4 * i + 1] * (da[4 * i + 1] - dotp),
                                                                                a[4 * i + 2] * (da[4 * i + 2] - dotp), a[4 * i + 3] * (da[4 * i + 3] - dotp));
#pragma unroll
    for (int i = 0; i < 8; ++i) {                                    // float4 i: points 2 i, 2 i + 1 of level i / 2
        const float4 t = reinterpret_cast<const float4*>(dloc + si * 32)[i];
        const float sx = rf[4 * (i >> 1) + 2] * 0.5f / 4.0f, sy = rf[4 * (i >> 1) + 3] * 0.5f / 4.0f;
        reinterpret_cast<float4*>(doff + row * 256 + h * 32)[i] = make_float4(t.x * sx, t.y * sy, t.z * sx, t.w * sy);
    }
}

// the value map's row stride in elements, or 0 where the shape is not the supported one
static inline int cg_vstride(int value_row_stride, long N, long S, long Lq)
{
    const int vs = value_row_stride > 0 ? value_row_stride : GR_D;
    if (vs < GR_D || (vs & 7) || S * (long)vs >= (1l << 31) || N * Lq > (1l << 31)) return 0;
    return vs;
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_msda_query_grad(const void* value, int value_dtype, int value_row_stride, const long* shapes, const long* lsi,
                                    const float* loc, const float* attn, const float* grad_out, int N, int S, int M, int D, int L, int Lq,
                                    int P, float* grad_loc, float* grad_attn, void* stream)
{
    clear_stale_error();
    if (!value || !shapes || !lsi || !loc || !attn || !grad_out || !grad_loc || !grad_attn) return DTLR_EINVAL;
    if (N <= 0 || S <= 0 || M <= 0 || D <= 0 || L <= 0 || Lq <= 0 || P <= 0) return DTLR_EINVAL;
    if (!is_f32_or_h16(value_dtype)) return DTLR_EDTYPE;
    if (M != DTLR_CROSS_HEADS || D != DTLR_CROSS_HEAD_DIM || L != DTLR_CROSS_LEVELS || P != DTLR_CROSS_POINTS) return DTLR_ESHAPE;
    const int vs = cg_vstride(value_row_stride, N, S, Lq);
    if (!vs) return DTLR_ESHAPE;
    if (misaligned(value, 15) || misaligned(loc, 15) || misaligned(attn, 15) || misaligned(grad_out, 15) || misaligned(grad_loc, 15) || misaligned(grad_attn, 15)) return DTLR_EINVAL;
    const int lph = value_dtype == DTLR_F32 ? 8 : 4;
    const long total = (long)N * Lq * 8 * lph;
    const unsigned grid = (unsigned)((total + 255) / 256);
    const hipStream_t st = (hipStream_t)stream;
    if (value_dtype == DTLR_F32)
        return launch<cg_query_grad_kernel<float>>(dim3(grid), dim3(256), 0, st, (const float*)value, shapes, lsi, loc, attn, grad_out, S, Lq, vs,
                                                   grad_loc, grad_attn, total);
    return launch<cg_query_grad_kernel<uint16_t>>(dim3(grid), dim3(256), 0, st, (const uint16_t*)value, shapes, lsi, loc, attn, grad_out, S, Lq, vs,
                                                  grad_loc, grad_attn, total);
}

extern "C" long dtlr_cross_recompute_workspace_bytes(long M)
{
    if (M <= 0 || M > (1l << 31)) return 0;
    return ((long)GR_D * CG_OW + (long)GR_D * GR_D + M * CG_OW) * (long)sizeof(float);
}

extern "C" int dtlr_cross_recompute(const void* s, const void* p, int x_dtype, const float* R, const void* value, int value_dtype,
                                    int value_row_stride, const long* shapes, const long* lsi, int N, int S, int Lq, const float* Wow,
                                    const float* bow, const float* Wo, const float* bo, const float* gamma1, const float* beta1, float eps,
                                    float* qin, float* A, float* loc, float* o, float* x1, float* u, void* workspace, void* stream)
{
    clear_stale_error();
    if (!s || !p || !R || !value || !shapes || !lsi || !Wow || !bow || !Wo || !bo || !gamma1 || !beta1 || !qin || !A || !loc || !o || !x1 || !u ||
        !workspace) return DTLR_EINVAL;
    if (N <= 0 || S <= 0 || Lq <= 0) return DTLR_EINVAL;
    if (!is_f32_or_h16(x_dtype) || !is_f32_or_h16(value_dtype)) return DTLR_EDTYPE;
    const int vs = cg_vstride(value_row_stride, N, S, Lq);
    if (!vs) return DTLR_ESHAPE;
    const long M = (long)N * Lq;
    if (misaligned(s, x_dtype == DTLR_F32 ? 3 : 1) || misaligned(p, x_dtype == DTLR_F32 ? 3 : 1) || misaligned(R, 15) || misaligned(value, 15) || misaligned(qin, 15) ||
        misaligned(A, 15) || misaligned(loc, 15) || misaligned(o, 15) || misaligned(x1, 15) || misaligned(u, 15) || misaligned(workspace, 15)) return DTLR_EINVAL;
    float* WowT = static_cast<float*>(workspace);                  // [256][384]
    float* WoT = WowT + (long)GR_D * CG_OW;                         // [256][256]
    float* ow = WoT + (long)GR_D * GR_D;                            // [M][384]
    const hipStream_t st = (hipStream_t)stream;
    const int h16 = x_dtype != DTLR_F32;
    if (int rc = gr_transpose(Wow, WowT, CG_OW, GR_D, st)) return rc;
    if (int rc = gr_transpose(Wo, WoT, GR_D, GR_D, st)) return rc;
    if (int rc = gr_rows_gemm256({.A = s, .A2 = p, .a_h16 = h16, .M = M, .Wt = WowT, .ldw = CG_OW, .N = CG_OW, .bias = bow, .out = ow, .ldo = CG_OW,
                                  .xsum = qin}, st)) return rc;
    const int lph = value_dtype == DTLR_F32 ? 8 : 4;
    const long total = M * 8 * lph;
    const unsigned grid = (unsigned)((total + 255) / 256);
    int rc;
    if (value_dtype == DTLR_F32)
        rc = launch<cg_attend_kernel<float>>(dim3(grid), dim3(256), 0, st, (const float*)value, shapes, lsi, (const float*)ow, R, S, Lq, vs, A, loc, o, total);
    else
        rc = launch<cg_attend_kernel<uint16_t>>(dim3(grid), dim3(256), 0, st, (const uint16_t*)value, shapes, lsi, (const float*)ow, R, S, Lq, vs, A, loc,
                                                o, total);
    if (rc) return rc;
    if (int rc2 = gr_rows_gemm256({.A = o, .M = M, .Wt = WoT, .ldw = GR_D, .N = GR_D, .bias = bo, .res = s, .res_h16 = h16, .out = x1, .ldo = GR_D}, st))
        return rc2;
    return gr_layernorm256(x1, gamma1, beta1, u, M, eps, st);
}

extern "C" int dtlr_cross_dow(const float* A, const float* dA, const float* dloc, const float* R, float* doff, float* dlogit, long M, void* stream)
{
    clear_stale_error();
    if (!A || !dA || !dloc || !R || !doff || !dlogit || M <= 0) return DTLR_EINVAL;
    if (M > (1l << 31)) return DTLR_ESHAPE;
    if (misaligned(A, 15) || misaligned(dA, 15) || misaligned(dloc, 15) || misaligned(R, 15) || misaligned(doff, 15) || misaligned(dlogit, 15)) return DTLR_EINVAL;
    const long total = M * 8;
    return launch<cg_dow_kernel>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, dA, dloc, R, doff, dlogit, total);
}
