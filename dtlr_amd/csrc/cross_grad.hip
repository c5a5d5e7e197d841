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
// The two row products are grad_rows.h's 32-row tile product (exact fp32 FMAs, 32 terms in fp32, the stages in fp64).
#include "gfx950_prims.h"
#include "grad_rows.h"
#include "../../include/dtlr_crossgrad.h"

namespace dtlr {

static_assert(GR_D == DTLR_CROSS_HIDDEN && DTLR_CROSS_HEADS * DTLR_CROSS_HEAD_DIM == DTLR_CROSS_HIDDEN, "8 heads x 32 channels");
constexpr int CG_OW = 384;                                          // [offsets 8 x 4 x 4 x 2 | logits 8 x 16]

// ------------------------------------------------------------------------------------------------------------ the row products
// out[m][n] = sum_k (A[m][k] + A2[m][k]) Wt[k][n] + bias[n] + res[m][n], K = 256 ; A, A2 (optional), res (optional) in fp32 or the 16-bit
// format ; qin (optional): receives A + A2 in fp32.  grid (ceil(M / 32), ceil(N / 256)).
__global__ __launch_bounds__(256) void cg_rows_gemm_kernel(const void* __restrict__ A, const void* __restrict__ A2, int a_h16, long M,
                                                           const float* __restrict__ Wt, int ldw, int N, const float* __restrict__ bias,
                                                           const void* __restrict__ res, int res_h16, float* __restrict__ out,
                                                           float* __restrict__ qin)
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
                if (qin && blockIdx.y == 0) qin[sm * GR_D + k] = v;
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
        out[m * N + n] = (float)v;
    }
}

// dst[c][r] = src[r][c], src [R, C]
__global__ __launch_bounds__(256) void cg_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C)
{
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) t[j][tx] = src[(long)(r0 + j) * C + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) dst[(long)(c0 + j) * R + r0 + tx] = t[tx][j];
}

// u = LayerNorm(x) over rows of 256: one wavefront a row, statistics fp32 two-pass (as dtlr_ln_backward takes them)
__global__ __launch_bounds__(256) void cg_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float* __restrict__ u, long M, float eps)
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
    *reinterpret_cast<float4*>(u + row * GR_D + 4 * lane) = make_float4(v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------------------------------------------------ the sampling geometry
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

// the level table of a launch, read from the device and made safe: 1 <= H, W <= 2^15 and 0 <= start <= S - 1
struct CgLevels { int H[4], W[4], st[4]; };
__device__ __forceinline__ long cg_clamp(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ CgLevels cg_levels(const long* __restrict__ shapes, const long* __restrict__ lsi, int S)
{
    CgLevels lv;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        lv.H[l] = (int)cg_clamp(shapes[2 * l], 1, 32768);
        lv.W[l] = (int)cg_clamp(shapes[2 * l + 1], 1, 32768);
        lv.st[l] = (int)cg_clamp(lsi[l], 0, (long)S - 1);
    }
    return lv;
}

// One sampling point.  px = loc_x W - 0.5, py = loc_y H - 0.5 ; the coordinate is clamped to [-1, size] first (msda.hip: identical
// inside the map, every weight zero outside it), each separable factor depends on one unsigned compare.  o[c]: element offset of corner c
// (00, 01, 10, 11 = (y0,x0), (y0,x1), (y1,x0), (y1,x1)) from the image's base, the pixel clamped into [0, S) ; wy / wx: the bilinear
// factors, zero for a row / column outside the map ; my / mx: 1 where that row / column is inside (the factors' derivatives up to sign) ;
// inside: the reference's test on the unclamped point (a NaN coordinate fails it).
struct CgGeo { int o[4]; float wy0, wy1, wx0, wx1, my0, my1, mx0, mx1; bool inside; };
__device__ __forceinline__ CgGeo cg_geo(float lx, float ly, int H, int W, int st, int S, int vstride)
{
    CgGeo g;
    const float fh = ly * (float)H - 0.5f, fw = lx * (float)W - 0.5f;
    g.inside = fh > -1.f && fw > -1.f && fh < (float)H && fw < (float)W;
    const float h_im = __builtin_amdgcn_fmed3f(fh, -1.f, (float)H), w_im = __builtin_amdgcn_fmed3f(fw, -1.f, (float)W);      // NaN -> -1
    const float hf = floorf(h_im), wf = floorf(w_im);
    const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
    const int h_low = (int)hf, w_low = (int)wf;
    const int h_high = h_low + 1, w_high = w_low + 1;
    const bool y0 = (unsigned)h_low < (unsigned)H, y1 = (unsigned)h_high < (unsigned)H;
    const bool x0 = (unsigned)w_low < (unsigned)W, x1 = (unsigned)w_high < (unsigned)W;
    g.wy0 = y0 ? hh : 0.f; g.wy1 = y1 ? lh : 0.f; g.wx0 = x0 ? hw : 0.f; g.wx1 = x1 ? lw : 0.f;
    g.my0 = y0 ? 1.f : 0.f; g.my1 = y1 ? 1.f : 0.f; g.mx0 = x0 ? 1.f : 0.f; g.mx1 = x1 ? 1.f : 0.f;
    // clamp BOTH ways: h_low ranges over [-1, H], h_high over [0, H + 1]: data unused there, the address must stay in the map
    const int h0 = min(max(h_low, 0), H - 1), h1 = max(min(h_high, H - 1), 0), w0 = min(max(w_low, 0), W - 1), w1 = max(min(w_high, W - 1), 0);
    const int r0 = st + h0 * W, r1 = st + h1 * W, last = S - 1;
    g.o[0] = min(r0 + w0, last) * vstride; g.o[1] = min(r0 + w1, last) * vstride;
    g.o[2] = min(r1 + w0, last) * vstride; g.o[3] = min(r1 + w1, last) * vstride;
    return g;
}

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
    const CgLevels lv = cg_levels(shapes, lsi, S);
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
            const CgGeo g = cg_geo(lc[(l * 4 + p) * 2], lc[(l * 4 + p) * 2 + 1], lv.H[l], lv.W[l], lv.st[l], S, vstride);
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
    const CgLevels lv = cg_levels(shapes, lsi, S);
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
        CgGeo geo[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            geo[p] = cg_geo(lx[p], ly[p], lv.H[l], lv.W[l], lv.st[l], S, vstride);
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
            const CgGeo& q = geo[p];
            const float da = q.wy0 * (q.wx0 * dot[0] + q.wx1 * dot[1]) + q.wy1 * (q.wx0 * dot[2] + q.wx1 * dot[3]);
            const float dx = q.wy0 * (q.mx1 * dot[1] - q.mx0 * dot[0]) + q.wy1 * (q.mx1 * dot[3] - q.mx0 * dot[2]);
            const float dy = q.wx0 * (q.my1 * dot[2] - q.my0 * dot[0]) + q.wx1 * (q.my1 * dot[3] - q.my0 * dot[1]);
            v[(l * 4 + p) * 2] = q.inside ? a[p] * (float)lv.W[l] * dx : 0.f;
            v[(l * 4 + p) * 2 + 1] = q.inside ? a[p] * (float)lv.H[l] * dy : 0.f;
            v[32 + l * 4 + p] = q.inside ? da : 0.f;
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

static inline bool cg_mis(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
static inline bool cg_dtype_ok(int dt) { return dt == DTLR_F32 || dt == DTLR_H16; }
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
    if (!cg_dtype_ok(value_dtype)) return DTLR_EDTYPE;
    if (M != DTLR_CROSS_HEADS || D != DTLR_CROSS_HEAD_DIM || L != DTLR_CROSS_LEVELS || P != DTLR_CROSS_POINTS) return DTLR_ESHAPE;
    const int vs = cg_vstride(value_row_stride, N, S, Lq);
    if (!vs) return DTLR_ESHAPE;
    if (cg_mis(value, 15) || cg_mis(loc, 15) || cg_mis(attn, 15) || cg_mis(grad_out, 15) || cg_mis(grad_loc, 15) || cg_mis(grad_attn, 15)) return DTLR_EINVAL;
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
    if (!cg_dtype_ok(x_dtype) || !cg_dtype_ok(value_dtype)) return DTLR_EDTYPE;
    const int vs = cg_vstride(value_row_stride, N, S, Lq);
    if (!vs) return DTLR_ESHAPE;
    const long M = (long)N * Lq;
    if (cg_mis(s, x_dtype == DTLR_F32 ? 3 : 1) || cg_mis(p, x_dtype == DTLR_F32 ? 3 : 1) || cg_mis(R, 15) || cg_mis(value, 15) || cg_mis(qin, 15) ||
        cg_mis(A, 15) || cg_mis(loc, 15) || cg_mis(o, 15) || cg_mis(x1, 15) || cg_mis(u, 15) || cg_mis(workspace, 15)) return DTLR_EINVAL;
    float* WowT = static_cast<float*>(workspace);                  // [256][384]
    float* WoT = WowT + (long)GR_D * CG_OW;                         // [256][256]
    float* ow = WoT + (long)GR_D * GR_D;                            // [M][384]
    const hipStream_t st = (hipStream_t)stream;
    const int h16 = x_dtype != DTLR_F32;
    const unsigned tiles = (unsigned)((M + GR_TR - 1) / GR_TR);
    if (int rc = launch<cg_transpose_kernel>(dim3(GR_D / 32, CG_OW / 32), dim3(256), 0, st, Wow, WowT, CG_OW, GR_D)) return rc;
    if (int rc = launch<cg_transpose_kernel>(dim3(GR_D / 32, GR_D / 32), dim3(256), 0, st, Wo, WoT, GR_D, GR_D)) return rc;
    if (int rc = launch<cg_rows_gemm_kernel>(dim3(tiles, 2), dim3(256), 0, st, s, p, h16, M, (const float*)WowT, CG_OW, CG_OW, bow,
                                             (const void*)nullptr, 0, ow, qin)) return rc;
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
    if (int rc2 = launch<cg_rows_gemm_kernel>(dim3(tiles, 1), dim3(256), 0, st, (const void*)o, (const void*)nullptr, 0, M, (const float*)WoT, GR_D, GR_D,
                                              bo, s, h16, x1, (float*)nullptr)) return rc2;
    return launch<cg_ln_kernel>(dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (const float*)x1, gamma1, beta1, u, M, eps);
}

extern "C" int dtlr_cross_dow(const float* A, const float* dA, const float* dloc, const float* R, float* doff, float* dlogit, long M, void* stream)
{
    clear_stale_error();
    if (!A || !dA || !dloc || !R || !doff || !dlogit || M <= 0) return DTLR_EINVAL;
    if (M > (1l << 31)) return DTLR_ESHAPE;
    if (cg_mis(A, 15) || cg_mis(dA, 15) || cg_mis(dloc, 15) || cg_mis(R, 15) || cg_mis(doff, 15) || cg_mis(dlogit, 15)) return DTLR_EINVAL;
    const long total = M * 8;
    return launch<cg_dow_kernel>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, dA, dloc, R, doff, dlogit, total);
}
