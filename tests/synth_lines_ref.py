"""The yardstick of the synthetic line renderer (include/dtlr_synth.h): the section's integer arithmetic restated in
numpy int64 over whole images -- no strips, no halos, no LDS -- so that the kernel's bytes can be compared for equality.  Written from
the section, not from the kernel.  Also the hand-made tables and seeded atlases the tests share."""
import numpy as np

MAX_R = 8
LINE_WORDS = 32
TAP_ONE = 4096
GLYPH_SIDE = 4096
BG_SIDE = 65536
U32 = np.uint64(0xFFFFFFFF)


def mix(a):
    """section 27's 32-bit mixer on uint64 arrays holding 32-bit values"""
    a = (np.asarray(a, dtype=np.uint64) + np.uint64(0x9E3779B9)) & U32
    a ^= a >> np.uint64(16)
    a = (a * np.uint64(0x7FEB352D)) & U32
    a ^= a >> np.uint64(15)
    a = (a * np.uint64(0x846CA68B)) & U32
    a ^= a >> np.uint64(16)
    return a


def hash3(seed, x, y):
    x = np.asarray(x, dtype=np.int64).astype(np.uint64) & U32
    y = np.asarray(y, dtype=np.int64).astype(np.uint64) & U32
    return mix(mix(mix(np.uint64(int(seed) & 0xFFFFFFFF)) ^ x) ^ y)


def noise(seed, h, w, amp_l, amp_g):
    """what the procedural background adds to the base colour: int64 [h, w]"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    cx, cy, fx, fy = x >> 4, y >> 4, x & 15, y & 15
    v = lambda i, j: (hash3(seed, i, j) & np.uint64(255)).astype(np.int64)
    top = v(cx, cy) * (16 - fx) + v(cx + 1, cy) * fx
    bot = v(cx, cy + 1) * (16 - fx) + v(cx + 1, cy + 1) * fx
    n = top * (16 - fy) + bot * fy
    lf = ((n - 32768) * amp_l + 16384) >> 15
    g = hash3((int(seed) & 0xFFFFFFFF) ^ 0xA511E9B3, x, y)
    s = sum(((g >> np.uint64(k)) & np.uint64(255)).astype(np.int64) for k in (0, 8, 16, 24))
    return lf + (((s - 510) * amp_g + 256) >> 9)


def glyph_of(atlas, glyphs, gid):
    """the mask of glyph `gid` as int64 [gh, gw], or None where the kernel skips it"""
    if gid < 0 or gid >= len(glyphs):
        return None
    off, gh, gw = (int(v) for v in glyphs[gid][:3])
    if off < 0 or gh <= 0 or gw <= 0 or gh > GLYPH_SIDE or gw > GLYPH_SIDE or off + gh * gw > len(atlas):
        return None
    return atlas[off: off + gh * gw].reshape(gh, gw).astype(np.int64)


def overlap(h, w, x, y, gh, gw):
    """(image slices, glyph slices) of a gh x gw mask whose corner is at (x, y), or None when it misses the image"""
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + gw, w), min(y + gh, h)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 - y, y1 - y), slice(x0 - x, x1 - x))


def coverage(h, w, placements, atlas, glyphs):
    M = np.zeros((h, w), dtype=np.int64)
    for gid, x, y in placements:
        g = glyph_of(atlas, glyphs, int(gid))
        ov = g is not None and overlap(h, w, int(x), int(y), *g.shape)
        if ov:
            M[ov[0]] += ((255 - M[ov[0]]) * g[ov[1]] + 127) // 255
    return M


def text_blur(M, taps, R):
    """horizontal then vertical, zero coverage outside: K = (sum t_j (sum t_i M) + 2^23) >> 24"""
    h, w = M.shape
    t = [int(taps[MAX_R + j]) for j in range(-R, R + 1)]
    P = np.pad(M, ((0, 0), (R, R)))
    H = sum(t[j + R] * P[:, R + j: R + j + w] for j in range(-R, R + 1))
    P = np.pad(H, ((R, R), (0, 0)))
    return (sum(t[j + R] * P[R + j: R + j + h, :] for j in range(-R, R + 1)) + (1 << 23)) >> 24


def background(row, h, w, bg):
    mode, k, x0, y0, flip = (int(v) for v in row[11:16])
    if mode == 1 and bg is not None and 0 <= k < len(bg[1]):
        pool, offs, hw = bg
        bh, bw, off = int(hw[k][0]), int(hw[k][1]), int(offs[k])
        if 1 <= bh <= BG_SIDE and 1 <= bw <= BG_SIDE and off >= 0 and off + bh * bw * 3 <= len(pool):
            img = pool[off: off + bh * bw * 3].reshape(bh, bw, 3).astype(np.int64)
            u, v = (x0 + np.arange(w, dtype=np.int64)) % (2 * bw), (y0 + np.arange(h, dtype=np.int64)) % (2 * bh)
            u, v = np.where(u >= bw, 2 * bw - 1 - u, u), np.where(v >= bh, 2 * bh - 1 - v, v)
            if flip:
                u = bw - 1 - u
            return img[v][:, u]
    base = np.clip(np.asarray(row[16:19], dtype=np.int64), 0, 255)
    n = noise(int(row[21]), h, w, int(np.clip(row[19], 0, 255)), int(np.clip(row[20], 0, 255)))
    return np.clip(base[None, None, :] + n[:, :, None], 0, 255)


def render_line(t, b, atlas, glyphs, bg=None):
    """line b of the tables `t` (lines, taps, placements, stains): uint8 [h, w, 3]"""
    row = t["lines"][b]
    h, w, p0, n_p, s0, n_s, R = (int(v) for v in row[:7])
    pl = t["placements"][p0: p0 + n_p] if n_p else np.zeros((0, 4), dtype=np.int64)
    K = text_blur(coverage(h, w, [r[:3] for r in pl], atlas, glyphs), t["taps"][b], R)
    B = background(row, h, w, bg)
    for st in (t["stains"][s0: s0 + n_s] if n_s else []):
        g = glyph_of(atlas, glyphs, int(st[0]))
        ov = g is not None and overlap(h, w, int(st[1]), int(st[2]), *g.shape)
        if ov:
            a = (int(np.clip(st[6], 0, 255)) * g[ov[1]] + 127) // 255
            col = np.clip(np.asarray(st[3:6], dtype=np.int64), 0, 255)
            B[ov[0]] = (B[ov[0]] * (255 - a)[:, :, None] + col[None, None, :] * a[:, :, None] + 127) // 255
    c = np.clip(np.asarray(row[7:10], dtype=np.int64), 0, 255)
    op = int(np.clip(row[10], 0, 255))
    ink = (c[None, None, :] * K[:, :, None] + 255 * (255 - K)[:, :, None] + 127) // 255
    A = ((op * K + 127) // 255)[:, :, None]
    C = (B * (255 - A) + ink * A + 127) // 255
    t1 = int(np.clip(row[22], 0, 2048))
    t0 = TAP_ONE - 2 * t1
    P = np.pad(C, ((0, 0), (1, 1), (0, 0)), mode="edge")
    Fh = t1 * P[:, :-2] + t0 * P[:, 1:-1] + t1 * P[:, 2:]
    P = np.pad(Fh, ((1, 1), (0, 0), (0, 0)), mode="edge")
    F = (t1 * P[:-2] + t0 * P[1:-1] + t1 * P[2:] + (1 << 23)) >> 24
    if int(row[23]):
        L = (19595 * F[:, :, 0] + 38470 * F[:, :, 1] + 7471 * F[:, :, 2] + 32768) >> 16
        F = np.stack([L, L, L], axis=2)
    assert F.min() >= 0 and F.max() <= 255
    return F.astype(np.uint8)


def render(t, atlas, glyphs, bg=None):
    return [render_line(t, b, atlas, glyphs, bg) for b in range(len(t["lines"]))]


# ------------------------------------------------------------------------------------------------------------ what the tests share
def taps_of(sigma, R):
    """round(4096 * gaussian) on -R..R, the centre adjusted to a sum of exactly 4096; tap j at MAX_R + j"""
    j = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(j * j) / (2.0 * sigma * sigma))
    t = np.round(TAP_ONE * g / g.sum()).astype(np.int64)
    t[R] += TAP_ONE - int(t.sum())
    out = np.zeros((2 * MAX_R + 1,), dtype=np.int32)
    out[MAX_R - R: MAX_R + R + 1] = t
    return out


def tables(specs):
    """hand-made tables: one dict a line with h, w and optionally placements [(glyph, x, y)], stains [(glyph, x, y, r, g, b, opacity)],
    R, sigma, colour, opacity, bg = (k, x0, y0, flip) for a pool image, base, amp = (lattice, grain), seed, t1, grey"""
    lines = np.zeros((len(specs), LINE_WORDS), dtype=np.int32)
    taps = np.zeros((len(specs), 2 * MAX_R + 1), dtype=np.int32)
    pl, st = [], []
    for b, s in enumerate(specs):
        p, q, R = list(s.get("placements", [])), list(s.get("stains", [])), int(s.get("R", 0))
        lines[b, :7] = (s["h"], s["w"], len(pl), len(p), len(st), len(q), R)
        lines[b, 7:10] = s.get("colour", (0, 0, 0))
        lines[b, 10] = s.get("opacity", 255)
        if "bg" in s:
            lines[b, 11:16] = (1,) + tuple(s["bg"])
        lines[b, 16:19] = s.get("base", (255, 255, 255))
        lines[b, 19:21] = s.get("amp", (0, 0))
        lines[b, 21] = s.get("seed", 0)
        lines[b, 22] = s.get("t1", 0)
        lines[b, 23] = s.get("grey", 0)
        taps[b] = taps_of(s.get("sigma", max(R, 1) / 3.0 + 0.2), R)
        pl += [tuple(r) + (0,) for r in p]
        st += [tuple(r) + (0,) for r in q]
    return {"lines": lines, "taps": taps, "placements": np.array(pl, dtype=np.int32).reshape(-1, 4), "stains": np.array(st, dtype=np.int32).reshape(-1, 8),
            "hw": [(int(s["h"]), int(s["w"])) for s in specs]}


def random_masks(seed, sizes):
    """seeded uint8 masks of the given (h, w): smooth-ish coverage with full, empty and partial pixels"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for h, w in sizes:
        m = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
        m[rng.random((h, w)) < 0.25] = 255
        m[rng.random((h, w)) < 0.15] = 0
        out.append(m)
    return out
