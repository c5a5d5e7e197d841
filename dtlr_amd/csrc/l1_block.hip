// One torchvision `Bottleneck` of ResNet-50's layer1 as ONE launch, 16-bit NHWC (models/dino/backbone.py:62-72,97-106; FrozenBN folded):
//
//     t1   = relu(x W1^T + b1)                              64 channels, rounded to 16 bit
//     t2   = relu(conv3x3(t1, W2, pad 1) + b2)              64 channels, rounded to 16 bit
//     out  = relu(t2 W3^T + b3 + x)                         identity form (x: 256 channels)
//     out  = relu([t2 | x0] [W3 | Wd]^T + (b3 + bd))        first-block form (x0: 64 channels; the 1x1 shortcut as K columns 64..127)
//     next = relu(out Wn^T + bn)                            optional (identity form): the NEXT bottleneck's first 1x1 convolution
//
// The separate launches (gemm.hip / gemm_kres.hip 1x1, conv3x3.hip, gemm_kres_chain tail) write t1 and t2 to HBM and read them back:
// 4 x 67 MB per block at 32 lines of 128 x 2048.  Here they never leave the CU:
//   * a workgroup of 8 waves owns (image, segment of 64 columns) and walks the image's rows top to bottom;
//   * per row step r: the x row segment + one halo pixel per side (72 pixel slots; DMA'd one step ahead through a 3-stage ring with the
//     sibling kernels' XOR chunk swizzle) -> t1 row r into a rolling LDS ring of three t1 rows -> t2 row r - 1 from the ring (the nine taps
//     are pixel offsets into the ring rows, as in conv3x3_patch_kernel) -> out row r - 1 from t2 and the x row still in its stage -> next
//     from the rounded out tile, which overwrites that x row in place (the lane that reads a residual chunk writes the result chunk);
//   * every weight is resident in registers as MFMA A-fragments, sliced by output channel across the waves (the images are the ones the
//     separate launches take: dtlr_gemm_kres_pack_weights for the 1x1 convolutions, the raw [64][3][3][64] weight for the 3x3);
//   * zero padding applies to t1: a ring row above / below the image and a pixel left / right of it are 0, not relu(b1).  The x loads
//     are clamped into the image row, so nothing is read across a row, image or buffer boundary.
// Every sum is the one the separate launches form: 16x16x32 MFMAs with the weight as the A operand, k-steps of 32 in ascending order (the
// 3x3: taps major, two k-steps per tap) from a zero accumulator, then + bias (+ residual), ReLU, one rounding -- so t1, t2, out and next
// are bit-identical to them.
#include "gfx950_prims.h"

namespace dtlr {

constexpr int LB_S = 64;                       // columns per segment
constexpr int LB_PX = 72;                      // pixel slots of a staged row: slot p = column xs - 1 + p; 0 and 65 are the halo, 66..71 unused
constexpr int LB_T1 = LB_PX * 128;             // one t1 ring row
constexpr int LB_T2 = LB_S * 128;              // the t2 tile
constexpr int LB_NSX = 3;                      // x stages

__device__ __forceinline__ void lb_sync() { DTLR_WAITCNT_LGKM(0); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); }

// CATF: first-block form (X = x0 [B, H, W, 64]; W3p = the [W3 | Wd] image, K = 128); otherwise X [B, H, W, 256], W3p K = 64.
// NQ2 = N2 / 64 of `next` (0: none; identity form only).  grid = B * nseg workgroups of 512 threads.
template <bool CATF, int NQ2>
__global__ __launch_bounds__(512, 1) void l1_bottleneck_kernel(
    const uint16_t* __restrict__ X, const uint16_t* __restrict__ W1p, const float* __restrict__ b1, const uint16_t* __restrict__ W2,
    const float* __restrict__ b2, const uint16_t* __restrict__ W3p, const float* __restrict__ b3, uint16_t* __restrict__ OUT,
    const uint16_t* __restrict__ Wnp, const float* __restrict__ bn, uint16_t* __restrict__ NEXT, int H, int W, int nseg)
{
    static_assert(!CATF || NQ2 == 0, "the out tile of the first-block form has no 256-channel stage to live in");
    extern __shared__ __attribute__((aligned(16))) unsigned char lb_smem[];
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lb_smem;
    constexpr int XG = CATF ? 1 : 4, CX = 64 * XG, KS1 = 2 * XG, KS3 = CATF ? 4 : 2, N2 = 64 * NQ2;
    constexpr int XST = 9 * XG * 1024;                                      // one x stage: 9 groups of 8 pixel slots x XG k blocks x 128 B
    constexpr int T1O = LB_NSX * XST, T2O = T1O + 3 * LB_T1, BO = T2O + LB_T2;   // BO: fp32 biases b1 [64] b2 [64] b3 [256] bn [128]
    constexpr int NDMA = 9 * XG, NJ = (NDMA + 7) / 8;                       // DMA instructions per row, per wave (at most)
    constexpr int NST = 4 + (NQ2 == 2 ? 4 : NQ2 == 1 ? 2 : 0);              // global stores per wave and row step
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    // workgroup b runs on XCD b % 8; logical ids are contiguous inside an XCD, so the segments of an image share an L2 (the halo re-read)
    const int nwg = (int)gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = (int)blockIdx.x & 7;
    const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + ((int)blockIdx.x >> 3);
    const int img = logical / nseg, xs = (logical - img * nseg) * LB_S;
    const bool full = xs + LB_S <= W;                                       // every store of the segment has all its lanes
    float* const bl = reinterpret_cast<float*>(lb_smem + BO);

    // staged x pixel slot p, k block kb, 16-byte chunk c (XG = 1: p * 128 + ..., the layout of a t1 ring row as well)
    auto xoff = [&](int p, int kb, int c) -> unsigned {
        return (unsigned)((p >> 3) * (XG * 1024) + kb * 1024 + (p & 7) * 128 + ((c ^ (p & 7)) * 16));
    };
    auto toff = [&](int p, int c) -> unsigned { return (unsigned)(p * 128 + ((c ^ (p & 7)) * 16)); };

    // DMA of row r: instruction i = (group of 8 slots, k block); slots past the halo and columns outside the row re-read an inside pixel
    const int dr = lane >> 3, dc = (lane & 7) ^ dr;
    auto issue = [&](int r, int st) {
        const uint16_t* rowp = X + ((long)img * H + r) * (long)W * CX;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = wave + 8 * j;
            if (i < NDMA) {
                const int grp = i / XG, kb = i - grp * XG;
                const int col = min(max(xs - 1 + min(8 * grp + dr, LB_S + 1), 0), W - 1);
                glds16(rowp + (long)col * CX + kb * 64 + dc * 8, lds_base + (unsigned)(st * XST + i * 1024));
            }
        }
    };
    issue(0, 0);
    // the ring row above the image, and the biases
    for (int o = tid * 16; o < LB_T1; o += 512 * 16) *reinterpret_cast<uint4*>(lb_smem + T1O + 2 * LB_T1 + o) = make_uint4(0u, 0u, 0u, 0u);
    if (tid < 64) { bl[tid] = b1[tid]; bl[64 + tid] = b2[tid]; }
    if (tid < 256) bl[128 + tid] = b3[tid];
    if constexpr (NQ2 > 0) { if (tid < N2) bl[384 + tid] = bn[tid]; }

    // ---- the resident operands -----------------------------------------------------------------------------------------------------
    // c1: wave w -> channel tile (q1, e1) = channels 32 q1 + 8 (m >> 2) + 4 e1 + (m & 3), pixel tiles {0, 1, halo} (w < 4) or {2, 3}
    const int q1 = (wave >> 1) & 1, e1 = wave & 1, tg = wave >> 2;
    uint4 w1f[KS1];
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) w1f[ks] = load16(W1p + ((long)((q1 * 2 + e1) * KS1 + ks)) * 512 + lane * 8);
    // c2: wave w -> channels 16 (w & 3) + m, pixel tiles 2 (w >> 2) + {0, 1}; A-fragment of (tap, kq): row m = n, k = 64 tap + 32 kq + 8 g ..
    const int c2i = wave & 3;
    uint4 w2f[9][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int kq = 0; kq < 2; ++kq) w2f[tap][kq] = load16(W2 + (long)(16 * c2i + n) * 576 + tap * 64 + kq * 32 + 8 * g);
    // c3: wave w -> channels 32 w .. 32 w + 31 (tiles e = 0, 1), every pixel tile
    uint4 w3f[2][KS3];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int ks = 0; ks < KS3; ++ks) w3f[e][ks] = load16(W3p + ((long)((wave * 2 + e) * KS3 + ks)) * 512 + lane * 8);
    // next: N2 = 128: wave w -> channel tile (w >> 1, w & 1), every pixel tile; N2 = 64: (w & 1, (w >> 1) & 1), pixel tiles 2 (w >> 2) + {0, 1}
    const int qn = NQ2 == 2 ? (wave >> 1) : (wave & 1), en = NQ2 == 2 ? (wave & 1) : ((wave >> 1) & 1);
    uint4 wnf[NQ2 > 0 ? 8 : 1];
    if constexpr (NQ2 > 0) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) wnf[ks] = load16(Wnp + ((long)((qn * 2 + en) * 8 + ks)) * 512 + lane * 8);
    }
    wait_vm<0>();

    for (int r = 0; r <= H; ++r) {
        lb_sync();                                   // row r staged by every wave; step r - 1 read out; (r = 0: the zero row and biases)
        const bool dma = r + 1 < H;
        if (dma) issue(r + 1, (r + 1) % 3);          // into the stage of row r - 2
        unsigned char* const t1w = lb_smem + T1O + (r % 3) * LB_T1;

        // ---- t1 row r = relu(x W1^T + b1), 0 outside the image ----------------------------------------------------------------------
        if (r < H) {
            const unsigned char* xr = lb_smem + (r % 3) * XST;
            const float4 bv = *reinterpret_cast<const float4*>(bl + 32 * q1 + 8 * g + 4 * e1);
            auto c1_store = [&](const f32x4_t& a, int p, bool mine) {
                const int col = xs - 1 + p;
                const bool ok = col >= 0 && col < W;
                const float v0 = ok ? fmaxf(a[0] + bv.x, 0.f) : 0.f, v1 = ok ? fmaxf(a[1] + bv.y, 0.f) : 0.f;
                const float v2 = ok ? fmaxf(a[2] + bv.z, 0.f) : 0.f, v3 = ok ? fmaxf(a[3] + bv.w, 0.f) : 0.f;
                if (mine) *reinterpret_cast<uint2*>(t1w + toff(p, 4 * q1 + g) + 8 * e1) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
            };
            {
                const int p0 = 32 * tg + n, p1 = p0 + 16;
                f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    const uint4 f0 = *reinterpret_cast<const uint4*>(xr + xoff(p0, ks >> 1, 4 * (ks & 1) + g));
                    const uint4 f1 = *reinterpret_cast<const uint4*>(xr + xoff(p1, ks >> 1, 4 * (ks & 1) + g));
                    a0 = mma16(w1f[ks], f0, a0);
                    a1 = mma16(w1f[ks], f1, a1);
                }
                c1_store(a0, p0, true);
                c1_store(a1, p1, true);
            }
            if (tg == 0) {                           // slots 64, 65 as lanes 8, 9 of the tile of slots 56..71
                const int p = 56 + n;
                f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks)
                    a = mma16(w1f[ks], *reinterpret_cast<const uint4*>(xr + xoff(p, ks >> 1, 4 * (ks & 1) + g)), a);
                c1_store(a, p, p >= LB_S && p <= LB_S + 1);
            }
        } else {
            for (int o = tid * 16; o < LB_T1; o += 512 * 16) *reinterpret_cast<uint4*>(t1w + o) = make_uint4(0u, 0u, 0u, 0u);
        }
        lb_sync();                                   // t1 row r published
        if (r >= 1) {
            const int y = r - 1;
            const unsigned char* xy = lb_smem + (y % 3) * XST;
            // ---- t2 row y = relu(conv3x3(t1) + b2): ring rows y - 1, y, y + 1 ------------------------------------------------------
            {
                const int s0 = (y + 2) % 3;
                f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
                const int j0 = 32 * tg + n;          // this lane's pixel of the first tile (the second: + 16)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int dy = tap / 3, dx = tap - 3 * dy;
                    const int sl = s0 + dy >= 3 ? s0 + dy - 3 : s0 + dy;
                    const unsigned char* tr = lb_smem + T1O + sl * LB_T1;
#pragma unroll
                    for (int kq = 0; kq < 2; ++kq) {
                        const uint4 f0 = *reinterpret_cast<const uint4*>(tr + toff(j0 + dx, kq * 4 + g));
                        const uint4 f1 = *reinterpret_cast<const uint4*>(tr + toff(j0 + 16 + dx, kq * 4 + g));
                        a0 = mma16(w2f[tap][kq], f0, a0);
                        a1 = mma16(w2f[tap][kq], f1, a1);
                    }
                }
                const float4 bv = *reinterpret_cast<const float4*>(bl + 64 + 16 * c2i + 4 * g);
                auto c2_store = [&](const f32x4_t& a, int j) {
                    const uint2 pk = make_uint2(pack_bf16x2(fmaxf(a[0] + bv.x, 0.f), fmaxf(a[1] + bv.y, 0.f)),
                                                pack_bf16x2(fmaxf(a[2] + bv.z, 0.f), fmaxf(a[3] + bv.w, 0.f)));
                    *reinterpret_cast<uint2*>(lb_smem + T2O + toff(j, 2 * c2i + (g >> 1)) + 8 * (g & 1)) = pk;
                };
                c2_store(a0, j0);
                c2_store(a1, j0 + 16);
            }
            lb_sync();                               // t2 row y published
            // ---- out row y = relu(t2 W3^T + b3 + x)  /  relu([t2 | x0] [W3 | Wd]^T + b) ---------------------------------------------
            {
                float bs[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) bs[e] = bl[128 + 32 * wave + 8 * g + e];
                uint16_t* orow = OUT + ((long)img * H + y) * (long)W * 256 + 32 * wave + 8 * g;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int j = 16 * tt + n, p = j + 1;
                    f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS3; ++ks) {
                        const uint4 f = ks < 2 ? *reinterpret_cast<const uint4*>(lb_smem + T2O + toff(j, 4 * (ks & 1) + g))
                                               : *reinterpret_cast<const uint4*>(xy + xoff(p, 0, 4 * (ks & 1) + g));
                        a0 = mma16(w3f[0][ks], f, a0);
                        a1 = mma16(w3f[1][ks], f, a1);
                    }
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (e < 4 ? a0[e & 3] : a1[e & 3]) + bs[e];
                    unsigned char* const rp = const_cast<unsigned char*>(xy) + xoff(p, CATF ? 0 : (wave >> 1), 4 * (wave & 1) + g);
                    if constexpr (!CATF) {
                        const uint4 rr = *reinterpret_cast<const uint4*>(rp);
                        const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += (e & 1) ? h16_hi(rw[e >> 1]) : h16_lo(rw[e >> 1]);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
                    const uint4 pk = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
                    if (xs + j < W) *reinterpret_cast<uint4*>(orow + (long)(xs + j) * 256) = pk;
                    if constexpr (NQ2 > 0) *reinterpret_cast<uint4*>(rp) = pk;
                }
            }
            if constexpr (NQ2 > 0) {
                // ---- next row y = relu(out Wn^T + bn), from the rounded out tile now in the x stage ---------------------------------
                lb_sync();
                const float4 bv = *reinterpret_cast<const float4*>(bl + 384 + 32 * qn + 8 * g + 4 * en);
                uint16_t* nrow = NEXT + ((long)img * H + y) * (long)W * N2 + 32 * qn + 8 * g + 4 * en;
                constexpr int NTT = NQ2 == 2 ? 4 : 2;
                const int tt0 = NQ2 == 2 ? 0 : 2 * tg;
#pragma unroll
                for (int u = 0; u < NTT; u += 2) {
                    const int j0 = 16 * (tt0 + u) + n, j1 = j0 + 16;
                    f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) {
                        const uint4 f0 = *reinterpret_cast<const uint4*>(xy + xoff(j0 + 1, ks >> 1, 4 * (ks & 1) + g));
                        const uint4 f1 = *reinterpret_cast<const uint4*>(xy + xoff(j1 + 1, ks >> 1, 4 * (ks & 1) + g));
                        a0 = mma16(wnf[ks], f0, a0);
                        a1 = mma16(wnf[ks], f1, a1);
                    }
                    if (xs + j0 < W)
                        *reinterpret_cast<uint2*>(nrow + (long)(xs + j0) * N2) = make_uint2(pack_bf16x2(fmaxf(a0[0] + bv.x, 0.f), fmaxf(a0[1] + bv.y, 0.f)),
                                                                                            pack_bf16x2(fmaxf(a0[2] + bv.z, 0.f), fmaxf(a0[3] + bv.w, 0.f)));
                    if (xs + j1 < W)
                        *reinterpret_cast<uint2*>(nrow + (long)(xs + j1) * N2) = make_uint2(pack_bf16x2(fmaxf(a1[0] + bv.x, 0.f), fmaxf(a1[1] + bv.y, 0.f)),
                                                                                            pack_bf16x2(fmaxf(a1[2] + bv.z, 0.f), fmaxf(a1[3] + bv.w, 0.f)));
                }
            }
        }
        // my pieces of row r + 1 must have landed before the next barrier.  Issued after them: this step's NST stores -- when the segment is
        // whole and the step has an output row (a ragged segment's waves may skip a store whose lanes are all past the row: vmcnt(0) then)
        if (dma) {
            if (full && r >= 1) wait_vm<NST>();
            else wait_vm<0>();
        }
    }
}

// One layer1 bottleneck.  X [B, H, W, cin] 16-bit NHWC, cin = 256 (identity form) or 64 (first-block form); W1p / W3p / Wnp: device copies of
// dtlr_gemm_kres_pack_weights of W1 [64, cin], of W3 [256, 64] (identity) or [W3 | Wd] [256, 128] (first block), of Wn [n2, 256];
// W2 [64, 3, 3, 64]; biases fp32 ([64], [64], [256], [n2]); OUT [B, H, W, 256]; NEXT [B, H, W, n2], n2 = 0 (none: Wnp, bn, NEXT unused),
// 64 or 128 (identity form only).
extern "C" int dtlr_l1_bottleneck(const void* X, int cin, const void* W1p, const float* b1, const void* W2, const float* b2, const void* W3p,
                                  const float* b3, void* OUT, const void* Wnp, const float* bn, void* NEXT, int n2, int B, int H, int W,
                                  void* stream)
{
    clear_stale_error();
    if (!X || !W1p || !b1 || !W2 || !b2 || !W3p || !b3 || !OUT || B <= 0 || H <= 0 || W <= 0) return DTLR_EINVAL;
    if ((cin != 64 && cin != 256) || (n2 != 0 && n2 != 64 && n2 != 128) || (cin == 64 && n2 != 0)) return DTLR_ESHAPE;
    if (n2 != 0 && (!Wnp || !bn || !NEXT)) return DTLR_EINVAL;
    const int nseg = (W + LB_S - 1) / LB_S;
    if ((long)B * nseg >= (1L << 31)) return DTLR_ESHAPE;
    const unsigned grid = (unsigned)(B * nseg);
    hipStream_t st = (hipStream_t)stream;
#define LB_LAUNCH(CATF_, NQ2_)                                                                     \
    {                                                                                              \
        constexpr int lds_ = LB_NSX * 9 * (CATF_ ? 1 : 4) * 1024 + 3 * LB_T1 + LB_T2 + 512 * 4;    \
        return launch<l1_bottleneck_kernel<CATF_, NQ2_>>(dim3(grid), dim3(512), lds_, st, (const uint16_t*)X, (const uint16_t*)W1p, b1, \
                                                         (const uint16_t*)W2, b2, (const uint16_t*)W3p, b3, (uint16_t*)OUT, (const uint16_t*)Wnp, bn, (uint16_t*)NEXT, H, W, nseg); \
    }
    if (cin == 64) LB_LAUNCH(true, 0)
    else if (n2 == 0) LB_LAUNCH(false, 0)
    else if (n2 == 64) LB_LAUNCH(false, 1)
    else LB_LAUNCH(false, 2)
#undef LB_LAUNCH
}

}  // namespace dtlr
