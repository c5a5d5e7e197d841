// Decoder self-attention over the 900 queries (nn.MultiheadAttention(256, 8), q = k = tgt + query_pos,
// v = tgt, no masks in eval: models/dino/deformable_transformer.py:847,904-907) as one fused
// flash-style kernel on the bf16 matrix cores: scores, softmax and P.V never touch HBM
// (the unfused form writes/reads a [B,8,900,900] fp32 score tensor, 829 MB per layer at B=32).
//
// One wavefront owns 32 queries of one (batch, head) and walks the keys in blocks of 32; no LDS, no
// barriers: every MFMA operand fragment is a plain 16-/8-byte global load (K/V of one (b,h) are
// 115 KB and L2-resident), and the orientation is chosen so that the accumulator layout of the first
// MFMA IS the operand layout of the second:
//     S^T[key, query] = K[key, :] . Q[query, :]^T        mfma_16x16x32 (A = K rows, B = Q rows)
//        C layout: lane (g = l>>4, n = l&15) holds keys 4g..4g+3 of query n  -> softmax statistics of
//        query n live in the four lanes {n, n+16, n+32, n+48}: two xor-shuffles per reduction
//     O^T[d, query]  += V^T[d, key] . P^T[key, query]     mfma_16x16x32 (A = V^T rows, B = P^T)
//        B operand of lane (g,n) = its own 8 probabilities (two key tiles x 4 regs): zero data movement;
//        the MFMA k-index <-> key permutation this implies is applied identically to the V^T fragment.
// V^T ([B, H, 32, Lpad], Lpad = 32-multiple, zero padded) is produced by the V projection.
#include "gfx950_prims.h"

namespace dtlr {

__device__ __forceinline__ uint32_t pack2(float a, float b) { return pack_bf16x2(a, b); }

// qk [B, L, 2*C]: q in columns [0, C), k in [C, 2C);  vt [B, H, 32, Lpad];  out [B, L, C];  C = H*32.
__global__ __launch_bounds__(256) void mha_fwd_bf16_kernel(const uint16_t* __restrict__ qk, const uint16_t* __restrict__ vt,
                                                           uint16_t* __restrict__ out, int L, int Lpad, int H,
                                                           float scale_log2e)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z;
    const int C = H * 32;
    const int q0 = blockIdx.x * 128 + wave * 32;
    if (q0 >= L) return;                                   // whole wave: no block-level sync is used
    const uint16_t* qkb = qk + (long)b * L * (2 * C);
    h16x8_t qf[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = min(q0 + qt * 16 + n, L - 1);
        qf[qt] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(qkb + (long)q * (2 * C) + h * 32 + 8 * g));
    }
    const uint16_t* vtb = vt + ((long)(b * H + h) * 32) * Lpad;
    f32x4_t o[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) o[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.f, 0.f};

    for (int kb = 0; kb < Lpad; kb += 32) {
        h16x8_t kf[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int key = min(kb + kt * 16 + n, L - 1);
            kf[kt] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(qkb + (long)key * (2 * C) + C + h * 32 + 8 * g));
        }
        h16x8_t vf[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            const uint16_t* vr = vtb + (long)(dt * 16 + n) * Lpad + kb + 4 * g;
            const uint2 lo = *reinterpret_cast<const uint2*>(vr), hi = *reinterpret_cast<const uint2*>(vr + 16);
            vf[dt] = __builtin_bit_cast(h16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            f32x4_t s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
                s[kt] = DTLR_MFMA_16x16x32_H16(kf[kt], qf[qt], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kb + kt * 16 + 4 * g + r;
                    const float v = key < L ? s[kt][r] * scale_log2e : -INFINITY;
                    s[kt][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m[qt], mx);              // finite: every 32-key block has >= 1 valid key
            const float alpha = __builtin_amdgcn_exp2f(m[qt] - m_new);
            m[qt] = m_new;
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - m_new); ps += s[kt][r]; }
            lsum[qt] = lsum[qt] * alpha + ps;
            const h16x8_t pf = __builtin_bit_cast(h16x8_t, make_uint4(pack2(s[0][0], s[0][1]), pack2(s[0][2], s[0][3]),
                                                                    pack2(s[1][0], s[1][1]), pack2(s[1][2], s[1][3])));
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                o[qt][dt] *= alpha;
                o[qt][dt] = DTLR_MFMA_16x16x32_H16(vf[dt], pf, o[qt][dt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        float l = lsum[qt];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
        const int q = q0 + qt * 16 + n;
        if (q < L) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const f32x4_t v = o[qt][dt] * inv;
                *reinterpret_cast<uint2*>(out + ((long)b * L + q) * C + h * 32 + dt * 16 + 4 * g) =
                    make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
            }
        }
    }
}

// ---- LDS-staged variant (the default when K and V^T of one (batch, head) fit the 160 KB LDS: L <= 1184) ----------
// The kernel above re-reads K and V^T of its (b, h) from global memory in every wave: 29 query blocks x 115 KB = 3.3 MB
// per (b, h), 855 MB per call at B = 32 -- it was L1/TA-bound at 112 us.  Here ONE workgroup (8 waves) owns a (b, h):
// it stages K and V^T once, in MFMA-fragment order (a fragment = one linear 1 KB block, lane l at 16 l: conflict-free),
// and its waves walk the query blocks (wave w takes blocks w, w+16) reading operands with ds_read_b128.
//   K image : key tile t (16 keys)           at t * 1024       : lane (g, n) <- K[16 t + n][8 g .. 8 g + 7]
//   V^T image: key block j (32 keys), d tile  at (2 j + dt) * 1024: lane (g, n) <- V^T[16 dt + n][32 j + 4 g .. +3 | 32 j + 16 + 4 g .. +3]
//              (gathered from the untransposed v while staging)
// Same operand values as mha_fwd_bf16_kernel; the softmax scale is applied by FMA here (results agree to fp32 rounding).
// reductions over the four lanes {n, n+16, n+32, n+48} of a query with the gfx950 row/half swaps (VALU, no LDS round trip):
// permlane16_swap(x, x) = ([x0,x0,x2,x2], [x1,x1,x3,x3]) by 16-lane rows, permlane32_swap(y, y) = ([lo,lo], [hi,hi])
__device__ __forceinline__ float g4_max(float x) {
    const unsigned u = __float_as_uint(x);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float y = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned v = __float_as_uint(y);
    const auto c = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return fmaxf(__uint_as_float(c[0]), __uint_as_float(c[1]));
}
__device__ __forceinline__ float g4_sum(float x) {
    const unsigned u = __float_as_uint(x);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const float y = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const unsigned v = __float_as_uint(y);
    const auto c = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return __uint_as_float(c[0]) + __uint_as_float(c[1]);
}

__global__ __launch_bounds__(1024) void mha_fwd_bf16_lds_kernel(const uint16_t* __restrict__ qk, const uint16_t* __restrict__ v,
                                                               uint16_t* __restrict__ out, int L, int Lpad, int H,
                                                               float scale_log2e)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_att[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.x, b = blockIdx.y;
    const int C = H * 32;
    const uint16_t* qkb = qk + (long)b * L * (2 * C);
    const uint16_t* vb = v + (long)b * L * C;
    const int nkb = Lpad / 32;                               // key blocks
    unsigned char* kimg = smem_att;                          // nkb * 2 KB
    unsigned char* vimg = smem_att + (long)nkb * 2048;       // nkb * 2 KB
    // ---- stage: fragment f of the K image = (tile t = f), of the V^T image = (j, dt); 16 waves-worth per pass ----
    for (int f = wave; f < 2 * nkb; f += 16) {
        const int key = min(f * 16 + n, L - 1);
        const uint4 kd = *reinterpret_cast<const uint4*>(qkb + (long)key * (2 * C) + C + h * 32 + 8 * g);
        *reinterpret_cast<uint4*>(kimg + f * 1024 + lane * 16) = kd;
        // V^T fragment (j, dt) gathered straight from v [B, L, C] (the transpose happens here, once per workgroup: no separate
        // transpose pass): lane (g, n) <- V[32 j + 4 g + r][16 dt + n] (r = 0..3) | V[32 j + 16 + 4 g + r][16 dt + n]; keys >= L -> 0
        const int j = f >> 1, dt = f & 1;
        const uint16_t* vc = vb + h * 32 + dt * 16 + n;
        uint32_t e[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int key = j * 32 + (r >> 2) * 16 + 4 * g + (r & 3);
            e[r] = key < L ? (uint32_t)vc[(long)key * C] : 0u;
        }
        *reinterpret_cast<uint4*>(vimg + f * 1024 + lane * 16) =
            make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    }
    __syncthreads();
    const int nqb = (L + 31) / 32;                           // query blocks of 32
    for (int qb = wave; qb < nqb; qb += 16) {
        const int q0 = qb * 32;
        h16x8_t qf[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int q = min(q0 + qt * 16 + n, L - 1);
            qf[qt] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(qkb + (long)q * (2 * C) + h * 32 + 8 * g));
        }
        f32x4_t o[2][2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        float m[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.f, 0.f};
        // one 32-key block; MASKED only for the last one (keys >= L are padding).  The softmax scale is folded into one FMA per
        // score (exp2(s*c - m)) and the running maximum is kept in scaled units: 149 -> ~110 VALU instructions per block, and
        // this kernel is bound by exactly that work.
#define MHA_KEY_BLOCK(J, MASKED)                                                                   \
        {                                                                                          \
            const int kb = (J) * 32;                                                               \
            h16x8_t kf[2], vf[2];                                                                   \
            _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                        \
                kf[t] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(kimg + (2 * (J) + t) * 1024 + lane * 16)); \
                vf[t] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(vimg + (2 * (J) + t) * 1024 + lane * 16)); \
            }                                                                                      \
            _Pragma("unroll") for (int qt = 0; qt < 2; ++qt) {                                     \
                f32x4_t sc[2];                                                                       \
                _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                                   \
                    sc[kt] = DTLR_MFMA_16x16x32_H16(kf[kt], qf[qt], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0); \
                if (MASKED) {                                                                      \
                    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                               \
                        _Pragma("unroll") for (int r = 0; r < 4; ++r)                              \
                            if (kb + kt * 16 + 4 * g + r >= L) sc[kt][r] = -INFINITY;              \
                }                                                                                  \
                float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),      \
                                 fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));     \
                mx = g4_max(mx) * scale_log2e;                                                     \
                const float m_new = fmaxf(m[qt], mx);       /* finite: every key block has >= 1 valid key */ \
                const float alpha = __builtin_amdgcn_exp2f(m[qt] - m_new);                         \
                m[qt] = m_new;                                                                     \
                float ps = 0.f;                                                                    \
                _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                                   \
                    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                \
                        sc[kt][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kt][r], scale_log2e, -m_new)); \
                        ps += sc[kt][r];                                                           \
                    }                                                                              \
                lsum[qt] = lsum[qt] * alpha + ps;                                                  \
                const h16x8_t pf = __builtin_bit_cast(h16x8_t, make_uint4(pack2(sc[0][0], sc[0][1]), pack2(sc[0][2], sc[0][3]), \
                                                                        pack2(sc[1][0], sc[1][1]), pack2(sc[1][2], sc[1][3]))); \
                _Pragma("unroll") for (int dt = 0; dt < 2; ++dt) {                                 \
                    o[qt][dt] *= alpha;                                                            \
                    o[qt][dt] = DTLR_MFMA_16x16x32_H16(vf[dt], pf, o[qt][dt], 0, 0, 0); \
                }                                                                                  \
            }                                                                                      \
        }
        for (int j = 0; j + 1 < nkb; ++j) MHA_KEY_BLOCK(j, false)
        MHA_KEY_BLOCK(nkb - 1, true)
#undef MHA_KEY_BLOCK
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float l = lsum[qt];
            l = g4_sum(l);
            const float inv = 1.0f / l;
            const int q = q0 + qt * 16 + n;
            if (q < L) {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const f32x4_t v = o[qt][dt] * inv;
                    *reinterpret_cast<uint2*>(out + ((long)b * L + q) * C + h * 32 + dt * 16 + 4 * g) =
                        make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
                }
            }
        }
    }
}

// ---- the same kernel with a TWO-PASS softmax (round 4: the DEFAULT 16-bit form; same-box A/B 9.24 -> 9.14 ms per step) ----------------
// The LDS-staged kernel is bound by the softmax's VALU work (tools/isa_mix.py: 125 VALU instructions against 8 MFMAs per 32-key block,
// the matrix pipe idles ~80%), and a good third of that work exists only because the row maximum is not known in advance: the per-block
// cross-lane max reduction, exp2 of the correction, the rescaling of the 16 accumulator registers and of the running sum.  Pass 1
// recomputes Q K^T (4 MFMAs per block, on the idle pipe) and keeps only the row maximum; pass 2 is exp2(s c - m) with the FINAL
// maximum and (V^T | 1) P -- the row sums come out of the matrix pipe as a third output tile: the softmax the reference computes (one
// subtraction of the global maximum), with fewer roundings than the online form.  Staging and operand layouts are those of mha_fwd_bf16_lds_kernel (kept as a separate copy so that the default
// kernel's instruction stream does not change: tools/isa_diff.py).
__global__ __launch_bounds__(1024) void mha_fwd_bf16_lds2_kernel(const uint16_t* __restrict__ qk, const uint16_t* __restrict__ v,
                                                               uint16_t* __restrict__ out, int L, int Lpad, int H,
                                                               float scale_log2e)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_att[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.x, b = blockIdx.y;
    const int C = H * 32;
    const uint16_t* qkb = qk + (long)b * L * (2 * C);
    const uint16_t* vb = v + (long)b * L * C;
    const int nkb = Lpad / 32;                               // key blocks
    unsigned char* kimg = smem_att;                          // nkb * 2 KB
    unsigned char* vimg = smem_att + (long)nkb * 2048;       // nkb * 2 KB
    // ---- stage: fragment f of the K image = (tile t = f), of the V^T image = (j, dt); 16 waves-worth per pass ----
    for (int f = wave; f < 2 * nkb; f += 16) {
        const int key = min(f * 16 + n, L - 1);
        const uint4 kd = *reinterpret_cast<const uint4*>(qkb + (long)key * (2 * C) + C + h * 32 + 8 * g);
        *reinterpret_cast<uint4*>(kimg + f * 1024 + lane * 16) = kd;
        // V^T fragment (j, dt) gathered straight from v [B, L, C] (the transpose happens here, once per workgroup: no separate
        // transpose pass): lane (g, n) <- V[32 j + 4 g + r][16 dt + n] (r = 0..3) | V[32 j + 16 + 4 g + r][16 dt + n]; keys >= L -> 0
        const int j = f >> 1, dt = f & 1;
        const uint16_t* vc = vb + h * 32 + dt * 16 + n;
        uint32_t e[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int key = j * 32 + (r >> 2) * 16 + 4 * g + (r & 3);
            e[r] = key < L ? (uint32_t)vc[(long)key * C] : 0u;
        }
        *reinterpret_cast<uint4*>(vimg + f * 1024 + lane * 16) =
            make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    }
    __syncthreads();
    const int nqb = (L + 31) / 32;                           // query blocks of 32
    // a third "d tile" of V^T whose row 0 is all ones: (V^T | 1) P yields the row sums of the ROUNDED probabilities -- the very values the
    // numerator multiplies -- from the idle matrix pipe instead of 16 v_add_f32 per key block
    const uint32_t one2 = n == 0 ? ((uint32_t)H16_ONE | ((uint32_t)H16_ONE << 16)) : 0u;
    const h16x8_t ones_f = __builtin_bit_cast(h16x8_t, make_uint4(one2, one2, one2, one2));
    // query blocks: wave w of workgroup z takes blocks w + 16 z, + 16 gridDim.z, ...  (gridDim.z = 1: the whole head in one workgroup; 2 for
    // small batches (round 5): at ONE line the 8 (head) workgroups each walked two query blocks per wave after staging K / V^T -- 58 us on 8
    // CUs; two workgroups per head stage the images twice and finish in one block per wave)
    for (int qb = wave + 16 * (int)blockIdx.z; qb < nqb; qb += 16 * (int)gridDim.z) {
        const int q0 = qb * 32;
        h16x8_t qf[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int q = min(q0 + qt * 16 + n, L - 1);
            qf[qt] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(qkb + (long)q * (2 * C) + h * 32 + 8 * g));
        }
        f32x4_t o[2][2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        float m[2];
        f32x4_t osum[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};    // row 0 = the row sums of P (see ones_f)
        // ---- pass 1: row maxima (raw scores; the scale is positive, so it commutes with the maximum) ----
        float mraw[2] = {-INFINITY, -INFINITY};
#define MHA_MAX_BLOCK(J, MASKED)                                                                   \
        {                                                                                      \
            const int kb = (J) * 32;                                                           \
            h16x8_t kf[2];                                                                      \
            _Pragma("unroll") for (int t = 0; t < 2; ++t)                                      \
                kf[t] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(kimg + (2 * (J) + t) * 1024 + lane * 16)); \
            _Pragma("unroll") for (int qt = 0; qt < 2; ++qt) {                                 \
                f32x4_t sc[2];                                                                   \
                _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                               \
                    sc[kt] = DTLR_MFMA_16x16x32_H16(kf[kt], qf[qt], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0); \
                if (MASKED) {                                                                  \
                    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                           \
                        _Pragma("unroll") for (int r = 0; r < 4; ++r)                          \
                            if (kb + kt * 16 + 4 * g + r >= L) sc[kt][r] = -INFINITY;          \
                }                                                                              \
                mraw[qt] = fmaxf(fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])), \
                                       fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3]))), mraw[qt]); \
            }                                                                                  \
        }
        for (int j = 0; j + 1 < nkb; ++j) MHA_MAX_BLOCK(j, false)
        MHA_MAX_BLOCK(nkb - 1, true)
#undef MHA_MAX_BLOCK
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) m[qt] = g4_max(mraw[qt]) * scale_log2e;      // finite: every row has >= 1 valid key
        // ---- pass 2: p = exp2(s c - m), row sums, O^T += V^T P ----
#define MHA_PV_BLOCK(J, MASKED)                                                                    \
        {                                                                                      \
            const int kb = (J) * 32;                                                           \
            h16x8_t kf[2], vf[2];                                                               \
            _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                    \
                kf[t] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(kimg + (2 * (J) + t) * 1024 + lane * 16)); \
                vf[t] = __builtin_bit_cast(h16x8_t, *reinterpret_cast<const uint4*>(vimg + (2 * (J) + t) * 1024 + lane * 16)); \
            }                                                                                  \
            _Pragma("unroll") for (int qt = 0; qt < 2; ++qt) {                                 \
                f32x4_t sc[2];                                                                   \
                _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                               \
                    sc[kt] = DTLR_MFMA_16x16x32_H16(kf[kt], qf[qt], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0); \
                if (MASKED) {                                                                  \
                    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                           \
                        _Pragma("unroll") for (int r = 0; r < 4; ++r)                          \
                            if (kb + kt * 16 + 4 * g + r >= L) sc[kt][r] = -INFINITY;          \
                }                                                                              \
                _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                               \
                    _Pragma("unroll") for (int r = 0; r < 4; ++r)                              \
                        sc[kt][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kt][r], scale_log2e, -m[qt])); \
                const h16x8_t pf = __builtin_bit_cast(h16x8_t, make_uint4(pack2(sc[0][0], sc[0][1]), pack2(sc[0][2], sc[0][3]), \
                                                                        pack2(sc[1][0], sc[1][1]), pack2(sc[1][2], sc[1][3]))); \
                _Pragma("unroll") for (int dt = 0; dt < 2; ++dt)                               \
                    o[qt][dt] = DTLR_MFMA_16x16x32_H16(vf[dt], pf, o[qt][dt], 0, 0, 0);        \
                osum[qt] = DTLR_MFMA_16x16x32_H16(ones_f, pf, osum[qt], 0, 0, 0);              \
            }                                                                                  \
        }
        for (int j = 0; j + 1 < nkb; ++j) MHA_PV_BLOCK(j, false)
        MHA_PV_BLOCK(nkb - 1, true)
#undef MHA_PV_BLOCK
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const float l = __shfl(osum[qt][0], n, 64);       // row 0 of the sum tile lives in lanes (g = 0, n): query n's denominator
            const float inv = 1.0f / l;
            const int q = q0 + qt * 16 + n;
            if (q < L) {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const f32x4_t v = o[qt][dt] * inv;
                    *reinterpret_cast<uint2*>(out + ((long)b * L + q) * C + h * 32 + dt * 16 + 4 * g) =
                        make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
                }
            }
        }
    }
}

// v [B, L, C] -> vt [B, H, 32, Lpad] (zero padded): the transposed image the attention kernel reads.
__global__ __launch_bounds__(256) void v_transpose_kernel(const uint16_t* __restrict__ v, uint16_t* __restrict__ vt,
                                                          int L, int Lpad, int H)
{
    // one block per (32-key tile, b): tile [32 keys][C] -> LDS -> [C][32 keys]
    extern __shared__ __attribute__((aligned(16))) uint16_t tile[];
    const int C = H * 32;
    const int k0 = blockIdx.x * 32, b = blockIdx.y;
    for (int i = threadIdx.x; i < 32 * C / 2; i += blockDim.x) {      // bf16 pairs, coalesced rows
        const int key = i / (C / 2), c2 = i % (C / 2);
        uint32_t w = 0;
        if (k0 + key < L) w = *reinterpret_cast<const uint32_t*>(v + ((long)b * L + k0 + key) * C + 2 * c2);
        tile[(2 * c2) * 33 + key] = (uint16_t)(w & 0xffffu);          // [c][key] padded to 33
        tile[(2 * c2 + 1) * 33 + key] = (uint16_t)(w >> 16);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 32; i += blockDim.x) {
        const int c = i / 32, key = i % 32;
        const int hh = c / 32, d = c % 32;
        vt[((long)(b * H + hh) * 32 + d) * Lpad + k0 + key] = tile[c * 33 + key];
    }
}


// ---- fp32 variant (parity path): same orientation trick on the exact-fp32 matrix core v_mfma_f32_16x16x4_f32.
// A lane feeds ONE float per MFMA (A[row = l&15][k = l>>4]); the lane's 8 contiguous d (or 4 contiguous keys)
// are spread over 8 (or 4) MFMAs -- a permutation of the contraction index applied to both operands alike.
//   S^T tile (16 keys x 16 queries): 8 MFMAs, lane (g,n) supplies K[key n][8g+j] and Q[query n][8g+j], j = 0..7
//   O^T tile (16 d x 16 queries) per 16-key tile: 4 MFMAs, lane supplies V^T[d n][4g+r] and its own P[key 4g+r]
__global__ __launch_bounds__(256) void mha_fwd_f32_kernel(const float* __restrict__ qk, const float* __restrict__ vt,
                                                          float* __restrict__ out, int L, int Lpad, int H, float scale_log2e)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.y, b = blockIdx.z;
    const int C = H * 32;
    const int q0 = blockIdx.x * 128 + wave * 32;
    if (q0 >= L) return;
    const float* qkb = qk + (long)b * L * (2 * C);
    float qf[2][8];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = min(q0 + qt * 16 + n, L - 1);
        const float4* p = reinterpret_cast<const float4*>(qkb + (long)q * (2 * C) + h * 32 + 8 * g);
        const float4 a = p[0], c = p[1];
        qf[qt][0] = a.x; qf[qt][1] = a.y; qf[qt][2] = a.z; qf[qt][3] = a.w; qf[qt][4] = c.x; qf[qt][5] = c.y; qf[qt][6] = c.z; qf[qt][7] = c.w;
    }
    const float* vtb = vt + ((long)(b * H + h) * 32) * Lpad;
    f32x4_t o[2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) o[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.f, 0.f};

    for (int kb = 0; kb < Lpad; kb += 32) {
        float kf[2][8];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const int key = min(kb + kt * 16 + n, L - 1);
            const float4* p = reinterpret_cast<const float4*>(qkb + (long)key * (2 * C) + C + h * 32 + 8 * g);
            const float4 a = p[0], c = p[1];
            kf[kt][0] = a.x; kf[kt][1] = a.y; kf[kt][2] = a.z; kf[kt][3] = a.w; kf[kt][4] = c.x; kf[kt][5] = c.y; kf[kt][6] = c.z; kf[kt][7] = c.w;
        }
        float vf[2][2][4];                                  // [d tile][key tile][r]
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const float4 t = *reinterpret_cast<const float4*>(vtb + (long)(dt * 16 + n) * Lpad + kb + kt * 16 + 4 * g);
                vf[dt][kt][0] = t.x; vf[dt][kt][1] = t.y; vf[dt][kt][2] = t.z; vf[dt][kt][3] = t.w;
            }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            f32x4_t s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                s[kt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 8; ++j) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt][j], qf[qt][j], s[kt], 0, 0, 0);
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kb + kt * 16 + 4 * g + r;
                    const float v = key < L ? s[kt][r] * scale_log2e : -INFINITY;
                    s[kt][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m[qt], mx);
            const float alpha = exp2f(m[qt] - m_new);
            m[qt] = m_new;
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { s[kt][r] = exp2f(s[kt][r] - m_new); ps += s[kt][r]; }
            lsum[qt] = lsum[qt] * alpha + ps;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                o[qt][dt] *= alpha;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        o[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[dt][kt][r], s[kt][r], o[qt][dt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        float l = lsum[qt];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
        const int q = q0 + qt * 16 + n;
        if (q < L) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const f32x4_t v = o[qt][dt] * inv;
                *reinterpret_cast<float4*>(out + ((long)b * L + q) * C + h * 32 + dt * 16 + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

// ---- split-fp32 variant (round 4; dtype DTLR_F32S): fp32 q / k / v / out, every product as three fp16 MFMAs on hi + lo halves ------
// The exact-fp32 kernel above (v_mfma_f32_16x16x4_f32, operands re-read from global memory by every wave) took 393 us per call at
// B = 32 -- 2.4 of the split engine's 35 ms.  Here a workgroup owns a (batch, head) like the LDS-staged 16-bit kernel, with K and V^T
// staged as FOUR fragment images (K_hi, K_lo, V^T_hi, V^T_lo; hi = fp16(x), lo = fp16(x - hi), split while staging: the fp32 values are
// read once per chunk from L2).  Four images of 900 keys are 232 KB, more than the LDS: the keys are walked in CHUNKS of `kc` 32-key
// blocks (kc x 8 KB <= 152 KB), each staged between two barriers; the online softmax carries (m, l, O) across chunks in registers.
//     S^T = K_hi Q_lo + K_lo Q_hi + K_hi Q_hi                     (Q split once per query block)
//     O^T += V^T_hi P_lo + V^T_lo P_hi + V^T_hi P_hi              (P = exp2(s c - m) in fp32, split in registers: the accumulator
//                                                                  layout of S^T is still the B-operand layout of the second product)
// Row sums are taken of the fp32 probabilities (hi + lo reproduces them to 2^-22).  Waves take query blocks w, w + 16, ...; a group of
// 16 query blocks re-stages the chunks (2 groups at L = 900: 464 KB of L2 reads per (batch, head)).
__device__ __forceinline__ void split8(const float (&x)[8], uint4& hi, uint4& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split2_f16(x[2 * i], x[2 * i + 1], h[i], l[i]);
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}

__global__ __launch_bounds__(1024) void mha_fwd_f32s_kernel(const float* __restrict__ qk, const float* __restrict__ v,
                                                            float* __restrict__ out, int L, int Lpad, int H, int kc, float scale_log2e)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_att[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int h = blockIdx.x, b = blockIdx.y;
    const int C = H * 32;
    const float* qkb = qk + (long)b * L * (2 * C);
    const float* vb = v + (long)b * L * C;
    const int nkb = Lpad / 32;                               // key blocks of 32
    unsigned char* k_hi = smem_att;                          // each image: kc * 2 KB (2 fragments of 1 KB per key block)
    unsigned char* k_lo = smem_att + (long)kc * 2048;
    unsigned char* v_hi = smem_att + (long)kc * 4096;
    unsigned char* v_lo = smem_att + (long)kc * 6144;
    const int nqb = (L + 31) / 32;                           // query blocks of 32
    for (int grp = 0; grp * 16 < nqb; ++grp) {
        const int qb = grp * 16 + wave;
        const bool active = qb < nqb;
        const int q0 = qb * 32;
        uint4 qh[2], ql[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int q = min(q0 + qt * 16 + n, L - 1);
            const float4* pq = reinterpret_cast<const float4*>(qkb + (long)q * (2 * C) + h * 32 + 8 * g);
            const float4 a = pq[0], c = pq[1];
            const float x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
            split8(x, qh[qt], ql[qt]);
        }
        f32x4_t o[2][2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[qt][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        float m[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.f, 0.f};

        for (int c0 = 0; c0 < nkb; c0 += kc) {
            const int cn = min(kc, nkb - c0);                // key blocks of this chunk
            __syncthreads();                                 // the previous chunk (or group) has been consumed by every wave
            for (int f = wave; f < 2 * cn; f += 16) {
                // K fragment f = key tile (16 keys): lane (g, n) <- K[16 (2 c0 + f) + n][8 g .. 8 g + 7]
                const int key = min((2 * c0 + f) * 16 + n, L - 1);
                const float4* pk = reinterpret_cast<const float4*>(qkb + (long)key * (2 * C) + C + h * 32 + 8 * g);
                const float4 a = pk[0], c = pk[1];
                const float kx[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
                uint4 hi, lo;
                split8(kx, hi, lo);
                *reinterpret_cast<uint4*>(k_hi + f * 1024 + lane * 16) = hi;
                *reinterpret_cast<uint4*>(k_lo + f * 1024 + lane * 16) = lo;
                // V^T fragment (j, dt): lane (g, n) <- V[32 j + 4 g + r][16 dt + n] (r = 0..3) | V[32 j + 16 + 4 g + r][16 dt + n]; keys >= L -> 0
                const int j = c0 + (f >> 1), dt = f & 1;
                const float* vc = vb + h * 32 + dt * 16 + n;
                float vx[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int kk = j * 32 + (r >> 2) * 16 + 4 * g + (r & 3);
                    vx[r] = kk < L ? vc[(long)kk * C] : 0.f;
                }
                split8(vx, hi, lo);
                *reinterpret_cast<uint4*>(v_hi + f * 1024 + lane * 16) = hi;
                *reinterpret_cast<uint4*>(v_lo + f * 1024 + lane * 16) = lo;
            }
            __syncthreads();
            if (!active) continue;
#define MHA_S_KEY_BLOCK(JL, MASKED)                                                                \
            {                                                                                      \
                const int kb = (c0 + (JL)) * 32;                                                   \
                uint4 kh[2], kl[2], vh[2], vl[2];                                                  \
                _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                    \
                    kh[t] = *reinterpret_cast<const uint4*>(k_hi + (2 * (JL) + t) * 1024 + lane * 16); \
                    kl[t] = *reinterpret_cast<const uint4*>(k_lo + (2 * (JL) + t) * 1024 + lane * 16); \
                    vh[t] = *reinterpret_cast<const uint4*>(v_hi + (2 * (JL) + t) * 1024 + lane * 16); \
                    vl[t] = *reinterpret_cast<const uint4*>(v_lo + (2 * (JL) + t) * 1024 + lane * 16); \
                }                                                                                  \
                _Pragma("unroll") for (int qt = 0; qt < 2; ++qt) {                                 \
                    f32x4_t sc[2];                                                                   \
                    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) sc[kt] = mma16_f16(kh[kt], ql[qt], f32x4_t{0.f, 0.f, 0.f, 0.f}); \
                    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) sc[kt] = mma16_f16(kl[kt], qh[qt], sc[kt]); \
                    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) sc[kt] = mma16_f16(kh[kt], qh[qt], sc[kt]); \
                    if (MASKED) {                                                                  \
                        _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                           \
                            _Pragma("unroll") for (int r = 0; r < 4; ++r)                          \
                                if (kb + kt * 16 + 4 * g + r >= L) sc[kt][r] = -INFINITY;          \
                    }                                                                              \
                    float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),  \
                                     fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3]))); \
                    mx = g4_max(mx) * scale_log2e;                                                 \
                    const float m_new = fmaxf(m[qt], mx);   /* finite: every key block has >= 1 valid key */ \
                    const float alpha = __builtin_amdgcn_exp2f(m[qt] - m_new);                     \
                    m[qt] = m_new;                                                                 \
                    float ps = 0.f, pv[8];                                                         \
                    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                               \
                        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                            \
                            pv[4 * kt + r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kt][r], scale_log2e, -m_new)); \
                            ps += pv[4 * kt + r];                                                  \
                        }                                                                          \
                    lsum[qt] = lsum[qt] * alpha + ps;                                              \
                    uint4 ph, pl;                                                                  \
                    split8(pv, ph, pl);                                                            \
                    _Pragma("unroll") for (int dt = 0; dt < 2; ++dt) o[qt][dt] *= alpha;           \
                    _Pragma("unroll") for (int dt = 0; dt < 2; ++dt) o[qt][dt] = mma16_f16(vh[dt], pl, o[qt][dt]); \
                    _Pragma("unroll") for (int dt = 0; dt < 2; ++dt) o[qt][dt] = mma16_f16(vl[dt], ph, o[qt][dt]); \
                    _Pragma("unroll") for (int dt = 0; dt < 2; ++dt) o[qt][dt] = mma16_f16(vh[dt], ph, o[qt][dt]); \
                }                                                                                  \
            }
            const bool last_chunk = c0 + cn == nkb;
            for (int jl = 0; jl + (last_chunk ? 1 : 0) < cn; ++jl) MHA_S_KEY_BLOCK(jl, false)
            if (last_chunk) MHA_S_KEY_BLOCK(cn - 1, true)
#undef MHA_S_KEY_BLOCK
        }
        if (active) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const float l = g4_sum(lsum[qt]);
                const float inv = 1.0f / l;
                const int q = q0 + qt * 16 + n;
                if (q < L) {
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const f32x4_t r = o[qt][dt] * inv;
                        *reinterpret_cast<float4*>(out + ((long)b * L + q) * C + h * 32 + dt * 16 + 4 * g) = make_float4(r[0], r[1], r[2], r[3]);
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void v_transpose_f32_kernel(const float* __restrict__ v, float* __restrict__ vt, int L, int Lpad, int H)
{
    extern __shared__ __attribute__((aligned(16))) float tilef[];      // [C][33]
    const int C = H * 32;
    const int k0 = blockIdx.x * 32, b = blockIdx.y;
    for (int i = threadIdx.x; i < 32 * C; i += blockDim.x) {
        const int key = i / C, c = i % C;
        tilef[c * 33 + key] = (k0 + key < L) ? v[((long)b * L + k0 + key) * C + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 32; i += blockDim.x) {
        const int c = i / 32, key = i % 32;
        vt[((long)(b * H + c / 32) * 32 + c % 32) * Lpad + k0 + key] = tilef[c * 33 + key];
    }
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_mha_forward(const void* qk, const void* v, void* vt_workspace, void* out,
                                int B, int L, int H, int head_dim, int dtype, void* stream)
{
    clear_stale_error();
    if (!qk || !v || !vt_workspace || !out) return DTLR_EINVAL;
    if (B <= 0 || L <= 0 || H <= 0) return DTLR_EINVAL;
    if (head_dim != 32) return DTLR_ESHAPE;
    if (dtype != DTLR_H16 && dtype != DTLR_F32 && dtype != DTLR_F32S) return DTLR_EDTYPE;
    hipStream_t st = (hipStream_t)stream;
    const int Lpad = (L + 31) / 32 * 32;
    const int C = H * 32;
    if (dtype == DTLR_F32S) {
        // key blocks per staged chunk: the fewest chunks whose four images (8 KB per key block) fit 152 KB, evenly sized
        const int nkb = Lpad / 32, cap = 19;
        const int nchunks = (nkb + cap - 1) / cap, kc = (nkb + nchunks - 1) / nchunks;
        const size_t lds = (size_t)kc * 8192;
        return launch<mha_fwd_f32s_kernel>(dim3(H, B), dim3(1024), lds, st, (const float*)qk, (const float*)v, (float*)out, L, Lpad, H, kc,
                                           1.4426950408889634f / sqrtf((float)head_dim));
    }
    if (dtype == DTLR_F32) {
        if (int rc = launch<v_transpose_f32_kernel>(dim3(Lpad / 32, B), dim3(256), (size_t)C * 33 * sizeof(float), st,
                                                    (const float*)v, (float*)vt_workspace, L, Lpad, H)) return rc;
        return launch<mha_fwd_f32_kernel>(dim3((L + 127) / 128, H, B), dim3(256), 0, st,
                                          (const float*)qk, (const float*)vt_workspace, (float*)out, L, Lpad, H,
                                          1.4426950408889634f / sqrtf((float)head_dim));
    }
    const float scale_log2e = 1.4426950408889634f / sqrtf((float)head_dim);
    const size_t lds = (size_t)(Lpad / 32) * 4096;               // K image + V^T image
    if (lds <= 152 * 1024) {                                     // transposes V while staging: no separate pass, no workspace
        // the two-pass softmax form is the default since round 4 (same-box A/B of the step: 9.24 -> 9.14 ms; its tests ran green on hardware);
        // the online-softmax form stays reachable in experiment builds only (DTLR_MHA_V=0)
        static const bool two_pass = exp_env_int("DTLR_MHA_V", 1) != 0;
        if (two_pass) {
            const int nz = (B * H <= 64 && (L + 31) / 32 > 16) ? 2 : 1;        // few (batch, head) pairs: split the query blocks over two workgroups
            return launch<mha_fwd_bf16_lds2_kernel>(dim3(H, B, nz), dim3(1024), lds, st,
                                                    (const uint16_t*)qk, (const uint16_t*)v, (uint16_t*)out, L, Lpad, H, scale_log2e);
        }
        return launch<mha_fwd_bf16_lds_kernel>(dim3(H, B), dim3(1024), lds, st,
                                               (const uint16_t*)qk, (const uint16_t*)v, (uint16_t*)out, L, Lpad, H, scale_log2e);
    }
    if (int rc = launch<v_transpose_kernel>(dim3(Lpad / 32, B), dim3(256), (size_t)C * 33 * sizeof(uint16_t), st,
                                            (const uint16_t*)v, (uint16_t*)vt_workspace, L, Lpad, H)) return rc;
    return launch<mha_fwd_bf16_kernel>(dim3((L + 127) / 128, H, B), dim3(256), 0, st,
                                       (const uint16_t*)qk, (const uint16_t*)vt_workspace, (uint16_t*)out, L, Lpad, H, scale_log2e);
}

extern "C" long dtlr_mha_workspace_bytes(int B, int L, int H, int head_dim)
{
    const long Lpad = (L + 31) / 32 * 32;
    return (long)B * H * head_dim * Lpad * 4;        // sized for fp32; bf16 uses half
}
