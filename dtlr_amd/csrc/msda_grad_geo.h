// The sampling-point geometry of the deformable attention as its gradient kernels take it (cross_grad.hip: the recomputed forward and
// the two query gradients ; msda_value_grad.hip: the value gradient): the level table made safe, then a point, then its four corners.
// msda.hip's forward kernels keep their own statement.  The expressions are written as they were in the kernels they came from: HIP
// contracts a * b + c, so reshaping one may change a bit.  Device code only, no launches.
#pragma once
#include "dtlr_common.h"

namespace dtlr {

// the level table of a launch, read from the device and made safe: 1 <= H, W <= 2^15 and 0 <= start <= S - 1
struct GeoLevels { int H[4], W[4], st[4]; };
__device__ __forceinline__ long geo_clamp(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ GeoLevels geo_levels(const long* __restrict__ shapes, const long* __restrict__ lsi, int S)
{
    GeoLevels lv;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        lv.H[l] = (int)geo_clamp(shapes[2 * l], 1, 32768);
        lv.W[l] = (int)geo_clamp(shapes[2 * l + 1], 1, 32768);
        lv.st[l] = (int)geo_clamp(lsi[l], 0, (long)S - 1);
    }
    return lv;
}

// One sampling point.  px = loc_x W - 0.5, py = loc_y H - 0.5 ; the coordinate is clamped to [-1, size] first (msda.hip: identical
// inside the map, every weight zero outside it ; a NaN becomes -1).  y0 / x0: the pixel of corner 00, in [-1, size] ; lh / lw: the
// point's fraction below / right of it, hh / hw: 1 minus them ; inside: the reference's test on the unclamped point (a NaN coordinate
// fails it).
struct GeoPoint { int y0, x0; float lh, lw, hh, hw; bool inside; };
__device__ __forceinline__ GeoPoint geo_point(float lx, float ly, int H, int W)
{
    GeoPoint p;
    const float fh = ly * (float)H - 0.5f, fw = lx * (float)W - 0.5f;
    p.inside = fh > -1.f && fw > -1.f && fh < (float)H && fw < (float)W;
    const float h_im = __builtin_amdgcn_fmed3f(fh, -1.f, (float)H), w_im = __builtin_amdgcn_fmed3f(fw, -1.f, (float)W);      // NaN -> -1
    const float hf = floorf(h_im), wf = floorf(w_im);
    p.lh = h_im - hf; p.lw = w_im - wf; p.hh = 1.f - p.lh; p.hw = 1.f - p.lw;
    p.y0 = (int)hf; p.x0 = (int)wf;
    return p;
}

// The four corners of a point, each separable factor depending on one unsigned compare.  o[c]: element offset of corner c (00, 01, 10,
// 11 = (y0,x0), (y0,x1), (y1,x0), (y1,x1)) from the image's base, the pixel clamped into [0, S) ; wy / wx: the bilinear factors, zero
// for a row / column outside the map ; my / mx: 1 where that row / column is inside (the factors' derivatives up to sign).
struct GeoCorners { int o[4]; float wy0, wy1, wx0, wx1, my0, my1, mx0, mx1; };
__device__ __forceinline__ GeoCorners geo_corners(const GeoPoint& p, int H, int W, int st, int S, int vstride)
{
    GeoCorners g;
    const float lh = p.lh, lw = p.lw, hh = p.hh, hw = p.hw;
    const int h_low = p.y0, w_low = p.x0;
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

}  // namespace dtlr
