// ConvNeXt backbone operators for gfx950 (include/dtlr_convnext.h; models/dino/convnext.py of the reference).
//
//   dtlr_cnx_dwconv_ln     Block.dwconv (depthwise 7x7, zero padding 3) + Block.norm (LayerNorm over C, eps 1e-6) in one launch
//   dtlr_cnx_ln_gather2x2  downsample_layers[i]: per-pixel LayerNorm + the 2x2 / stride-2 regrouping; the convolution itself is a GEMM
//   dtlr_cnx_stem          downsample_layers[0]: 4x4 / stride-4 convolution (floor sizes) + LayerNorm
//
// No MFMA here: the depthwise convolution is 49 FMAs per output against one load and one store, VALU- and bandwidth-bound.
// All offsets are 64-bit (the stage-0 map of a 32-line xlarge batch has 1.3e8 elements).
#include "dtlr_common.h"
#include "../../include/dtlr_convnext.h"

using namespace dtlr;

namespace {

template <typename T> __device__ __forceinline__ float4 load4(const T* p) {
    if constexpr (sizeof(T) == 2) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        return make_float4(h16_lo(t.x), h16_hi(t.x), h16_lo(t.y), h16_hi(t.y));
    } else {
        return *reinterpret_cast<const float4*>(p);
    }
}
template <typename T> __device__ __forceinline__ void store4(T* p, float a, float b, float c, float d) {
    if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
    else *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

// ---------------------------------------------------------------------------------------------------- depthwise 7x7 + LayerNorm
// Workgroup (256 threads) = ALL C channels of PX neighbouring columns, walking down `rows` output rows.  A thread owns 4 channels of
// one column: its 49 x 4 taps stay in registers for the whole walk, and seven running sums -- the output rows y-3 .. y+3 that input
// row y feeds -- form a register ring: every input row is loaded once per column (7 loads of 4 channels, lanes along channels:
// 8-byte (16-bit) / 16-byte (fp32) accesses), multiplied into all seven sums, and the oldest sum leaves as a finished output row.
// Finished rows wait in LDS ([rows][PX][C] fp32) until the walk ends; then one wavefront per (row, column) takes mean and variance
// over C (two passes over LDS: no cancellation) and writes the normalised row.  C > 1024 (more than 256 x 4 channels): the walk is
// repeated per 1024-channel pass with that pass's taps, PX = 1.
template <typename T>
__global__ __launch_bounds__(256) void cnx_dwconv_ln_kernel(const T* __restrict__ x, const float* __restrict__ k,
                                                            const float* __restrict__ bias, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ y,
                                                            int H, int W, int C, int PX, int rows, float eps)
{
    extern __shared__ __attribute__((aligned(16))) float cnx_stash[];           // [rows][PX][C]
    const int b = blockIdx.z, r0 = blockIdx.y * rows, x0 = blockIdx.x * PX;
    const int cgb = min(C >> 2, 256);                     // channel groups (of 4) a pass covers
    const int cg = threadIdx.x % cgb, px = threadIdx.x / cgb;
    const int col = x0 + px;
    const int nrow = min(rows, H - r0);
    const T* xb = x + (long)b * H * W * C;
    if (px < PX) {
        for (int c = 4 * cg; c < C; c += DTLR_CNX_PASS_CHANNELS) {
            float4 kw[49];
#pragma unroll
            for (int t = 0; t < 49; ++t) kw[t] = *reinterpret_cast<const float4*>(k + (long)t * C + c);
            const float4 bs = *reinterpret_cast<const float4*>(bias + c);
            float4 acc[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int iy = 0; iy < nrow + 6; ++iy) {
                const int yy = r0 - 3 + iy;                               // input row; it feeds output rows yy-3 .. yy+3 = acc[0] .. acc[6]
                if (yy >= 0 && yy < H) {
                    const T* xr = xb + (long)yy * W * C + c;
#pragma unroll
                    for (int dx = 0; dx < 7; ++dx) {
                        const int xx = col + dx - 3;
                        if (xx >= 0 && xx < W) {
                            const float4 v = load4(xr + (long)xx * C);
#pragma unroll
                            for (int j = 0; j < 7; ++j) {                 // output row yy-3+j: tap row (yy - out) + 3 = 6 - j
                                const float4 kk = kw[(6 - j) * 7 + dx];
                                acc[j].x = fmaf(v.x, kk.x, acc[j].x); acc[j].y = fmaf(v.y, kk.y, acc[j].y);
                                acc[j].z = fmaf(v.z, kk.z, acc[j].z); acc[j].w = fmaf(v.w, kk.w, acc[j].w);
                            }
                        }
                    }
                }
                const int orow = iy - 6;                                  // output row yy-3 is complete, as row r0 + orow of the tile
                if (orow >= 0)
                    *reinterpret_cast<float4*>(cnx_stash + ((long)orow * PX + px) * C + c) =
                        make_float4(acc[0].x + bs.x, acc[0].y + bs.y, acc[0].z + bs.z, acc[0].w + bs.w);
#pragma unroll
                for (int j = 0; j < 6; ++j) acc[j] = acc[j + 1];
                acc[6] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int npx = min(PX, W - x0);
    const float invC = 1.0f / (float)C;
    for (int e = wv; e < nrow * npx; e += 4) {
        const int r = e / npx, p = e % npx;
        const float* s = cnx_stash + ((long)r * PX + p) * C;
        float sum = 0.f;
        for (int c = 4 * lane; c < C; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(s + c);
            sum += (v.x + v.y) + (v.z + v.w);
        }
        const float mean = wave_sum(sum) * invC;
        float q = 0.f;
        for (int c = 4 * lane; c < C; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(s + c);
            const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
        const float rstd = rsqrtf(wave_sum(q) * invC + eps);
        T* yr = y + (((long)b * H + r0 + r) * W + x0 + p) * C;
        for (int c = 4 * lane; c < C; c += 256) {
            const float4 v = *reinterpret_cast<const float4*>(s + c);
            const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
            store4(yr + c, (v.x - mean) * rstd * ga.x + be.x, (v.y - mean) * rstd * ga.y + be.y,
                   (v.z - mean) * rstd * ga.z + be.z, (v.w - mean) * rstd * ga.w + be.w);
        }
    }
}

// ------------------------------------------------------------------------------------------------- LayerNorm + 2x2 regrouping
// One wavefront per INPUT pixel (y < 2 H2, x < 2 W2): lane l holds channels 4l + 256g, g < 8 (C <= 2048); the normalised row goes to
// part (y & 1) * 2 + (x & 1) of output pixel (y / 2, x / 2).
template <typename T>
__global__ __launch_bounds__(256) void cnx_ln_gather_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ y,
                                                            int H, int W, int C, int H2, int W2, long rows, float eps)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int We = 2 * W2, He = 2 * H2;
    const int xx = (int)(row % We), yy = (int)((row / We) % He);
    const long b = row / ((long)We * He);
    const T* p = x + ((b * H + yy) * W + xx) * (long)C;
    float4 v[8];
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int c = g * 256 + 4 * lane;
        v[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            v[g] = load4(p + c);
            s += (v[g].x + v[g].y) + (v[g].z + v[g].w);
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g)
        if (g * 256 + 4 * lane < C) {
            const float d0 = v[g].x - mean, d1 = v[g].y - mean, d2 = v[g].z - mean, d3 = v[g].w - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    T* yr = y + (((b * H2 + (yy >> 1)) * W2 + (xx >> 1)) * 4 + ((yy & 1) * 2 + (xx & 1))) * (long)C;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int c = g * 256 + 4 * lane;
        if (c < C) {
            const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
            store4(yr + c, (v[g].x - mean) * rstd * ga.x + be.x, (v[g].y - mean) * rstd * ga.y + be.y,
                   (v[g].z - mean) * rstd * ga.z + be.z, (v[g].w - mean) * rstd * ga.w + be.w);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- stem
// One wavefront per 4 output pixels of a row (a workgroup: 16); lane l accumulates channels l + 64 j, j < 8 (E <= 512), of its four
// pixels from the 4 x 48 patch values in LDS; weights [48][E] are read along E (coalesced, cache resident).  LayerNorm by wave sums.
template <typename OT>
__global__ __launch_bounds__(256) void cnx_stem_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, OT* __restrict__ out,
                                                       int H, int W, int Hp, int Wp, int E, float eps)
{
    __shared__ float patch[16][48];
    const int b = blockIdx.z, i = blockIdx.y, j0 = blockIdx.x * 16;
    for (int t = threadIdx.x; t < 16 * 48; t += 256) {
        const int px = t / 48, kk = t % 48;
        const int c = kk >> 4, dy = (kk >> 2) & 3, dx = kk & 3;
        patch[px][kk] = (j0 + px < Wp) ? x[(((long)b * 3 + c) * H + 4 * i + dy) * W + 4 * (j0 + px) + dx] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc[4][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float bv = (lane + 64 * j < E) ? bias[lane + 64 * j] : 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[p][j] = bv;
    }
    for (int kk = 0; kk < 48; ++kk) {
        float pv[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) pv[p] = patch[4 * wv + p][kk];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = lane + 64 * j;
            if (e < E) {
                const float wk = w[(long)kk * E + e];
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p][j] = fmaf(pv[p], wk, acc[p][j]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (lane + 64 * j < E) s += acc[p][j];
        const float mean = wave_sum(s) / (float)E;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (lane + 64 * j < E) { const float d = acc[p][j] - mean; q += d * d; }
        const float rstd = rsqrtf(wave_sum(q) / (float)E + eps);
        const int jx = j0 + 4 * wv + p;
        if (jx < Wp) {
            OT* o = out + (((long)b * Hp + i) * Wp + jx) * E;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = lane + 64 * j;
                if (e < E) {
                    const float r = (acc[p][j] - mean) * rstd * gamma[e] + beta[e];
                    if constexpr (sizeof(OT) == 2) o[e] = f32_to_bf16(r);
                    else o[e] = r;
                }
            }
        }
    }
}

bool cnx_sizes_ok(int B, int H, int W, int C, int maxC)
{
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 31) || C > maxC) return false;
    const long hw = (long)H * W;                                   // < 2^62
    if (hw > DTLR_CNX_MAX_ELEMS / C) return false;
    return hw * C <= DTLR_CNX_MAX_ELEMS / B;
}

}  // namespace

extern "C" int dtlr_cnx_dwconv_ln(const void* x, const float* k, const float* bias, const float* ln_w, const float* ln_b, void* y,
                                  int B, int H, int W, int C, float eps, int dtype, void* stream)
{
    clear_stale_error();
    if (!x || !k || !bias || !ln_w || !ln_b || !y) return DTLR_EINVAL;
    if (!cnx_sizes_ok(B, H, W, C, DTLR_CNX_MAX_C) || B > 65535) return DTLR_EINVAL;
    if (dtype != DTLR_H16 && dtype != DTLR_F32) return DTLR_EINVAL;
    const int PX = C >= DTLR_CNX_PASS_CHANNELS ? 1 : DTLR_CNX_PASS_CHANNELS / C;             // C = 96: 10 columns, 240 threads at work
    const int rows = C <= DTLR_CNX_PASS_CHANNELS ? DTLR_CNX_TILE_ROWS : DTLR_CNX_TILE_ROWS_WIDE;
    const long gy = ((long)H + rows - 1) / rows;
    if (gy > 65535) return DTLR_EINVAL;
    const dim3 grid((unsigned)(((long)W + PX - 1) / PX), (unsigned)gy, (unsigned)B);
    const size_t lds = (size_t)rows * PX * C * sizeof(float);                                // <= 16 x 4 KB, or 8 x 16 KB at C = 4096
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DTLR_H16)
        return launch<cnx_dwconv_ln_kernel<uint16_t>>(grid, dim3(256), lds, st, (const uint16_t*)x, k, bias, ln_w, ln_b, (uint16_t*)y, H, W, C, PX, rows, eps);
    return launch<cnx_dwconv_ln_kernel<float>>(grid, dim3(256), lds, st, (const float*)x, k, bias, ln_w, ln_b, (float*)y, H, W, C, PX, rows, eps);
}

extern "C" int dtlr_cnx_ln_gather2x2(const void* x, const float* ln_w, const float* ln_b, void* y,
                                     int B, int H, int W, int C, float eps, int dtype, void* stream)
{
    clear_stale_error();
    if (!x || !ln_w || !ln_b || !y) return DTLR_EINVAL;
    if (!cnx_sizes_ok(B, H, W, C, DTLR_CNX_GATHER_MAX_C) || H < 2 || W < 2) return DTLR_EINVAL;
    if (dtype != DTLR_H16 && dtype != DTLR_F32) return DTLR_EINVAL;
    const int H2 = H / 2, W2 = W / 2;
    const long rows = (long)B * H2 * W2 * 4;
    const long grid = (rows + 3) / 4;
    if (grid > 0x7fffffffL) return DTLR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DTLR_H16)
        return launch<cnx_ln_gather_kernel<uint16_t>>(dim3((unsigned)grid), dim3(256), 0, st, (const uint16_t*)x, ln_w, ln_b, (uint16_t*)y, H, W, C, H2, W2, rows, eps);
    return launch<cnx_ln_gather_kernel<float>>(dim3((unsigned)grid), dim3(256), 0, st, (const float*)x, ln_w, ln_b, (float*)y, H, W, C, H2, W2, rows, eps);
}

extern "C" int dtlr_cnx_stem(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, void* out,
                             int B, int H, int W, int E, float eps, int out_dtype, void* stream)
{
    clear_stale_error();
    if (!x || !w || !bias || !ln_w || !ln_b || !out) return DTLR_EINVAL;
    if (B <= 0 || B > 65535 || H < 4 || W < 4 || E <= 0 || (E & 31) || E > DTLR_CNX_STEM_MAX_E) return DTLR_EINVAL;
    if (out_dtype != DTLR_H16 && out_dtype != DTLR_F32) return DTLR_EINVAL;
    const int Hp = H / 4, Wp = W / 4;
    if (Hp > 65535) return DTLR_EINVAL;
    const dim3 grid((unsigned)((Wp + 15) / 16), (unsigned)Hp, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == DTLR_H16)
        return launch<cnx_stem_kernel<uint16_t>>(grid, dim3(256), 0, st, x, w, bias, ln_w, ln_b, (uint16_t*)out, H, W, Hp, Wp, E, eps);
    return launch<cnx_stem_kernel<float>>(grid, dim3(256), 0, st, x, w, bias, ln_w, ln_b, (float*)out, H, W, Hp, Wp, E, eps);
}
