// Synthetic text lines rendered on the device (include/dtlr_synth.h): what the reference does with Pillow on the
// host (datasets/synthetic_lines_general.py + datasets/generate_canva.py: text layer -> GaussianBlur -> paste over a background crop with
// patterns -> blur -> grey) as ONE launch over a batch of lines, written straight into a pool of uint8 HWC images.  The host draws and
// lays out (dtlr_amd/synthlines.py); everything that touches a pixel is here, and all of it is integer arithmetic, so the bytes are a
// function of the tables alone and tests/synth_lines_ref.py restates them in numpy for equality.
//
// A workgroup renders one strip of DTLR_SYNTH_STRIP columns of one line (blockIdx.x, blockIdx.y): line and strip are the same for every
// lane, so the parameter row, the taps, the placement / stain / glyph tables are read through uniform addresses.  Phases, a barrier
// between two:
//   1  coverage M (uint8) of the strip + 1 + R columns each side, by GATHER: a thread owns pixels and loops over the candidate
//      placements -- the smallest contiguous range of the line's (x-sorted) table that holds every glyph meeting the strip
//   2  horizontal blur pass  H = sum t_j M      (uint32, unrounded)       strip + 1 each side
//   3  vertical pass         K = (sum t_j H + 2^23) >> 24                 rows outside the line are zero coverage
//   4  background + stains + ink + compose C (3 x uint8, in phase 2's LDS)
//   5  final 3 x 3 blur with clamped edges, grey, store: every byte of the strip once
// No atomics, no inline assembly, no scratch; LDS is static (the figures are in section 27).  Whatever the tables hold, nothing outside
// the atlas, the pool and the line's own bytes is touched: out-of-range entries are skipped, never followed (the header says which).
#include "dtlr_common.h"
#include "../../include/dtlr_synth.h"

namespace dtlr {

constexpr int SY_SW = DTLR_SYNTH_STRIP, SY_MR = DTLR_SYNTH_MAX_R, SY_MH = DTLR_SYNTH_MAX_H, SY_LW = DTLR_SYNTH_LINE_WORDS;
constexpr int SY_CW = SY_SW + 2;                  // columns that are composed: the strip and the final blur's neighbours
constexpr int SY_MW = SY_CW + 2 * SY_MR;          // columns that carry coverage: those and the text blur's reach
constexpr int SY_GLYPH_SIDE = 4096;               // a mask is at most this high and wide (keeps h * w in 32 bits)
constexpr int SY_BG_SIDE = 65536;                 // a background image likewise

// the 32-bit mixer of the procedural background ("lowbias32" with a golden-ratio offset so that 0 does not map to 0)
__device__ __forceinline__ unsigned sy_mix(unsigned a) {
    a += 0x9E3779B9u; a ^= a >> 16; a *= 0x7FEB352Du; a ^= a >> 15; a *= 0x846CA68Bu; a ^= a >> 16;
    return a;
}
__device__ __forceinline__ unsigned sy_hash(unsigned seed, int x, int y) { return sy_mix(sy_mix(sy_mix(seed) ^ (unsigned)x) ^ (unsigned)y); }

__device__ __forceinline__ int sy_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// what the procedural background adds to the base colour at (x, y) >= 0: a 16-px lattice of hashed bytes, bilinear in integer weights,
// centred and scaled by amp_l / 128, plus the sum of the four bytes of one hash, centred and scaled by amp_g / 512
__device__ __forceinline__ int sy_noise(unsigned seed, int x, int y, int amp_l, int amp_g) {
    const int cx = x >> 4, cy = y >> 4, fx = x & 15, fy = y & 15;
    const int v00 = (int)(sy_hash(seed, cx, cy) & 255u), v10 = (int)(sy_hash(seed, cx + 1, cy) & 255u);
    const int v01 = (int)(sy_hash(seed, cx, cy + 1) & 255u), v11 = (int)(sy_hash(seed, cx + 1, cy + 1) & 255u);
    const int top = v00 * (16 - fx) + v10 * fx, bot = v01 * (16 - fx) + v11 * fx;
    const int n = top * (16 - fy) + bot * fy;                                  // 0 .. 255 * 256
    const int lf = ((n - 32768) * amp_l + 16384) >> 15;                        // arithmetic shift: floor
    const unsigned g = sy_hash(seed ^ 0xA511E9B3u, x, y);
    const int s = (int)(g & 255u) + (int)((g >> 8) & 255u) + (int)((g >> 16) & 255u) + (int)(g >> 24);
    return lf + (((s - 510) * amp_g + 256) >> 9);
}

// glyph `id` of the atlas, or false when the id or the mask's extent is outside it (an empty mask is false too: nothing to draw)
__device__ __forceinline__ bool sy_glyph(const int* __restrict__ glyphs, int G, long atlas_bytes, int id, int& off, int& gh, int& gw) {
    if (id < 0 || id >= G) return false;
    off = glyphs[4 * id]; gh = glyphs[4 * id + 1]; gw = glyphs[4 * id + 2];
    if (off < 0 || gh <= 0 || gw <= 0 || gh > SY_GLYPH_SIDE || gw > SY_GLYPH_SIDE) return false;
    return (long)off + (long)(gh * gw) <= atlas_bytes;
}

__global__ __launch_bounds__(256) void synth_lines_kernel(const unsigned char* __restrict__ atlas, long atlas_bytes, const int* __restrict__ glyphs, int G,
                                                          const int* __restrict__ lines, const int* __restrict__ taps,
                                                          const int* __restrict__ placements, int P, const int* __restrict__ stains, int S,
                                                          const unsigned char* __restrict__ bg_pool, long bg_bytes, const long* __restrict__ bg_off,
                                                          const int* __restrict__ bg_hw, int K,
                                                          const long* __restrict__ dst_off, unsigned char* __restrict__ dst, long dst_bytes, int max_w)
{
    __shared__ unsigned char sM[SY_MH * SY_MW];
    __shared__ unsigned sH[SY_MH * SY_CW];                       // phase 4 reuses it for the composite, 3 bytes a pixel
    __shared__ unsigned char sK[SY_MH * SY_CW];
    const int b = blockIdx.y, sx0 = blockIdx.x * SY_SW, tid = threadIdx.x;
    const int* ln = lines + (long)b * SY_LW;                     // uniform: scalar loads
    const int h = ln[0], w = ln[1], R = ln[6];
    if (h < 1 || h > SY_MH || w < 1 || w > max_w || R < 0 || R > SY_MR || sx0 >= w) return;
    const long o = dst_off[b], nbytes = (long)h * w * 3;
    if (o < 0 || o > dst_bytes - nbytes) return;
    int p0 = ln[2], np = ln[3], s0 = ln[4], ns = ln[5];
    if (p0 < 0 || np < 0 || np > DTLR_SYNTH_MAX_GLYPHS || (long)p0 + np > P) np = 0;
    if (s0 < 0 || ns < 0 || ns > DTLR_SYNTH_MAX_STAINS || (long)s0 + ns > S) ns = 0;
    const int sw = w - sx0 < SY_SW ? w - sx0 : SY_SW, cw = sw + 2, mw = cw + 2 * R;
    const int mx0 = sx0 - 1 - R;                                 // the image column of coverage column 0
    const int* tp = taps + (long)b * (2 * SY_MR + 1) + SY_MR;

    // ---- 1: coverage.  The candidates first (uniform), then the gather
    int lo = np, hi = 0;
    for (int p = 0; p < np; ++p) {
        const int* pl = placements + 4L * (p0 + p);
        int off, gh, gw;
        if (!sy_glyph(glyphs, G, atlas_bytes, pl[0], off, gh, gw)) continue;
        const long x = pl[1];
        if (x + gw > mx0 && x < (long)mx0 + mw) { lo = p < lo ? p : lo; hi = p + 1; }
    }
    for (int i = tid; i < h * mw; i += 256) {
        const int y = i / mw, m = i - y * mw, x = mx0 + m;
        unsigned M = 0;
        if (x >= 0 && x < w) {
            for (int p = lo; p < hi; ++p) {
                const int* pl = placements + 4L * (p0 + p);
                int off, gh, gw;
                if (!sy_glyph(glyphs, G, atlas_bytes, pl[0], off, gh, gw)) continue;
                const unsigned gx = (unsigned)x - (unsigned)pl[1], gy = (unsigned)y - (unsigned)pl[2];
                if (gx < (unsigned)gw && gy < (unsigned)gh) {
                    const unsigned g = atlas[(long)off + (long)(gy * (unsigned)gw + gx)];
                    M += ((255u - M) * g + 127u) / 255u;
                }
            }
        }
        sM[y * SY_MW + m] = (unsigned char)M;
    }
    __syncthreads();

    // ---- 2: horizontal pass, unrounded (at most 4096 * 255)
    for (int i = tid; i < h * cw; i += 256) {
        const int y = i / cw, c = i - y * cw;
        unsigned a = 0;
        for (int j = -R; j <= R; ++j) a += (unsigned)tp[j] * sM[y * SY_MW + c + R + j];
        sH[y * SY_CW + c] = a;
    }
    __syncthreads();

    // ---- 3: vertical pass: at most 2^24 * 255 + 2^23 < 2^32
    for (int i = tid; i < h * cw; i += 256) {
        const int y = i / cw, c = i - y * cw;
        unsigned a = 1u << 23;
        for (int j = -R; j <= R; ++j)
            if (y + j >= 0 && y + j < h) a += (unsigned)tp[j] * sH[(y + j) * SY_CW + c];
        a >>= 24;
        sK[y * SY_CW + c] = (unsigned char)(a > 255u ? 255u : a);
    }
    __syncthreads();

    // ---- 4: background, stains, ink, compose
    unsigned char* sC = reinterpret_cast<unsigned char*>(sH);
    const int cr = sy_clamp(ln[7], 0, 255), cg = sy_clamp(ln[8], 0, 255), cb = sy_clamp(ln[9], 0, 255), op = sy_clamp(ln[10], 0, 255);
    const int base_r = sy_clamp(ln[16], 0, 255), base_g = sy_clamp(ln[17], 0, 255), base_b = sy_clamp(ln[18], 0, 255);
    const int amp_l = sy_clamp(ln[19], 0, 255), amp_g = sy_clamp(ln[20], 0, 255), flip = ln[15];
    const unsigned seed = (unsigned)ln[21];
    bool pool = false;
    int bh = 0, bw = 0, bx0 = 0, by0 = 0;
    long boff = 0;
    if (ln[11] == 1 && ln[12] >= 0 && ln[12] < K) {
        const int k = ln[12];
        bh = bg_hw[2 * k]; bw = bg_hw[2 * k + 1]; boff = bg_off[k];
        pool = bh >= 1 && bw >= 1 && bh <= SY_BG_SIDE && bw <= SY_BG_SIDE && boff >= 0 && boff <= bg_bytes - (long)bh * bw * 3;
        if (pool) {                                              // the crop's corner reduced into one mirror period, once
            long u = (long)ln[13] % (2L * bw), v = (long)ln[14] % (2L * bh);
            bx0 = (int)(u < 0 ? u + 2L * bw : u); by0 = (int)(v < 0 ? v + 2L * bh : v);
        }
    }
    for (int i = tid; i < h * cw; i += 256) {
        const int y = i / cw, c = i - y * cw, x = sx0 - 1 + c;
        if (x < 0 || x >= w) continue;
        int r0, g0, b0;
        if (pool) {
            int u = (bx0 + x) % (2 * bw), v = (by0 + y) % (2 * bh);
            if (u >= bw) u = 2 * bw - 1 - u;
            if (v >= bh) v = 2 * bh - 1 - v;
            if (flip) u = bw - 1 - u;
            const unsigned char* q = bg_pool + boff + ((long)v * bw + u) * 3;
            r0 = q[0]; g0 = q[1]; b0 = q[2];
        } else {
            const int n = sy_noise(seed, x, y, amp_l, amp_g);
            r0 = sy_clamp(base_r + n, 0, 255); g0 = sy_clamp(base_g + n, 0, 255); b0 = sy_clamp(base_b + n, 0, 255);
        }
        for (int s = 0; s < ns; ++s) {
            const int* st = stains + 8L * (s0 + s);
            int off, gh, gw;
            if (!sy_glyph(glyphs, G, atlas_bytes, st[0], off, gh, gw)) continue;
            const unsigned gx = (unsigned)x - (unsigned)st[1], gy = (unsigned)y - (unsigned)st[2];
            if (gx < (unsigned)gw && gy < (unsigned)gh) {
                const int g = atlas[(long)off + (long)(gy * (unsigned)gw + gx)];
                const int a = (sy_clamp(st[6], 0, 255) * g + 127) / 255;
                r0 = (r0 * (255 - a) + sy_clamp(st[3], 0, 255) * a + 127) / 255;
                g0 = (g0 * (255 - a) + sy_clamp(st[4], 0, 255) * a + 127) / 255;
                b0 = (b0 * (255 - a) + sy_clamp(st[5], 0, 255) * a + 127) / 255;
            }
        }
        const int k = sK[y * SY_CW + c], A = (op * k + 127) / 255;
        const int ir = (cr * k + 255 * (255 - k) + 127) / 255, ig = (cg * k + 255 * (255 - k) + 127) / 255, ib = (cb * k + 255 * (255 - k) + 127) / 255;
        unsigned char* q = sC + (y * SY_CW + c) * 3;
        q[0] = (unsigned char)((r0 * (255 - A) + ir * A + 127) / 255);
        q[1] = (unsigned char)((g0 * (255 - A) + ig * A + 127) / 255);
        q[2] = (unsigned char)((b0 * (255 - A) + ib * A + 127) / 255);
    }
    __syncthreads();

    // ---- 5: final blur (t1, 4096 - 2 t1, t1) both ways, edges clamped; grey; store
    const unsigned t1 = (unsigned)sy_clamp(ln[22], 0, 2048), t0 = 4096u - 2u * t1;
    const int grey = ln[23];
    unsigned char* out = dst + o;
    for (int i = tid; i < h * sw; i += 256) {
        const int y = i / sw, xs = i - y * sw, x = sx0 + xs;
        const int cl = (x > 0 ? x - 1 : 0) - sx0 + 1, cc = xs + 1, cn = (x < w - 1 ? x + 1 : w - 1) - sx0 + 1;
        const int yu = y > 0 ? y - 1 : 0, yd = y < h - 1 ? y + 1 : h - 1;
        unsigned f[3];
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned hu = t1 * sC[(yu * SY_CW + cl) * 3 + ch] + t0 * sC[(yu * SY_CW + cc) * 3 + ch] + t1 * sC[(yu * SY_CW + cn) * 3 + ch];
            const unsigned hc = t1 * sC[(y * SY_CW + cl) * 3 + ch] + t0 * sC[(y * SY_CW + cc) * 3 + ch] + t1 * sC[(y * SY_CW + cn) * 3 + ch];
            const unsigned hd = t1 * sC[(yd * SY_CW + cl) * 3 + ch] + t0 * sC[(yd * SY_CW + cc) * 3 + ch] + t1 * sC[(yd * SY_CW + cn) * 3 + ch];
            f[ch] = (t1 * hu + t0 * hc + t1 * hd + (1u << 23)) >> 24;
        }
        if (grey) f[0] = f[1] = f[2] = (19595u * f[0] + 38470u * f[1] + 7471u * f[2] + 32768u) >> 16;      // Pillow's convert("L")
        unsigned char* q = out + ((long)y * w + x) * 3;
        q[0] = (unsigned char)f[0]; q[1] = (unsigned char)f[1]; q[2] = (unsigned char)f[2];
    }
}

}  // namespace dtlr

using namespace dtlr;

extern "C" int dtlr_synth_lines(const unsigned char* atlas, long atlas_bytes, const int* glyphs, int G, const int* lines, const int* taps,
                                const int* placements, int P, const int* stains, int S, const unsigned char* bg_pool, long bg_bytes,
                                const long* bg_off, const int* bg_hw, int K, const long* dst_off, unsigned char* dst, long dst_bytes, int B,
                                int max_w, void* stream)
{
    clear_stale_error();
    if (!atlas || !glyphs || !lines || !taps || !dst_off || !dst) return DTLR_EINVAL;
    if ((P > 0 && !placements) || (S > 0 && !stains) || (K > 0 && (!bg_pool || !bg_off || !bg_hw))) return DTLR_EINVAL;
    if (B <= 0 || B > 65535 || max_w <= 0 || max_w > DTLR_SYNTH_MAX_W || G < 0 || P < 0 || S < 0 || K < 0) return DTLR_ESHAPE;
    if (atlas_bytes < 0 || atlas_bytes > 0x7FFFFFFFL || bg_bytes < 0 || dst_bytes <= 0) return DTLR_ESHAPE;
    const dim3 grid((max_w + SY_SW - 1) / SY_SW, B);
    return launch<synth_lines_kernel>(grid, dim3(256), 0, (hipStream_t)stream, atlas, atlas_bytes, glyphs, G, lines, taps, placements, P, stains,
                                      S, bg_pool, bg_bytes, bg_off, bg_hw, K, dst_off, dst, dst_bytes, max_w);
}
