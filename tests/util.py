"""Shared helpers for the tests (test infrastructure; may import the oracle)."""
import ctypes

import numpy as np
import torch


def msda_inputs(N, M, D, Lq, P, shapes, seed, lo=0.0, hi=1.0, value_scale=1.0, dtype=np.float32):
    """Same generator as tests/golden/make_golden.py::msda_inputs (numpy PCG64)."""
    r = np.random.Generator(np.random.PCG64(seed))
    S = sum(h * w for h, w in shapes)
    L = len(shapes)
    value = (r.random((N, S, M, D), dtype=np.float32) * 2 - 1) * value_scale
    loc = r.uniform(lo, hi, (N, Lq, M, L, P, 2)).astype(np.float32)
    aw = r.random((N, Lq, M, L, P), dtype=np.float32) + 1e-5
    aw = (aw / aw.sum((-1, -2), keepdims=True)).astype(np.float32)
    shp = torch.as_tensor(shapes, dtype=torch.long)
    lsi = torch.cat((shp.new_zeros((1,)), shp.prod(1).cumsum(0)[:-1]))
    return (torch.from_numpy(value.astype(dtype)), shp, lsi, torch.from_numpy(loc.astype(dtype)), torch.from_numpy(aw.astype(dtype)))


def c_oracle_msda(clib, value, shapes, lsi, loc, attn):
    """Run oracle/msda_ref.c on CPU tensors."""
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    out = torch.empty((N, Lq, M * D), dtype=value.dtype)
    fn = clib.msda_ref_forward_f64 if value.dtype == torch.float64 else clib.msda_ref_forward_f32
    fn.restype = ctypes.c_int
    vp = ctypes.c_void_p
    rc = fn(vp(value.contiguous().data_ptr()), vp(shapes.contiguous().data_ptr()), vp(lsi.contiguous().data_ptr()),
            vp(loc.contiguous().data_ptr()), vp(attn.contiguous().data_ptr()),
            N, S, M, D, L, Lq, P, vp(out.data_ptr()))
    assert rc == 0
    return out


def selection_is_valid(idx, scores, k, tol):
    """Tie-aware check of a top-k selection `idx` [B,k] against fp32 `scores` [B,S]: every selected
    score >= (k-th largest - tol), every unselected <= (k-th largest + tol), order descending within tol."""
    for b in range(scores.shape[0]):
        s = scores[b]
        kth = torch.topk(s, k)[0][-1]
        sel = s[idx[b].long()]
        if not bool((sel >= kth - tol).all()):
            return False
        m = torch.ones_like(s, dtype=torch.bool)
        m[idx[b].long()] = False
        if m.any() and not bool((s[m] <= kth + tol).all()):
            return False
        if not bool((sel[:-1] >= sel[1:] - tol).all()):
            return False
        if len(set(idx[b].tolist())) != k:
            return False
    return True


def preproc_image(h, w, seed):
    """Seeded uint8 RGB test image [h, w, 3] shared by tests/golden/make_golden_preproc.py and the preprocessing tests:
    uniform noise, or (odd seeds) stroke-like light paper with dark runs."""
    g = np.random.Generator(np.random.PCG64(seed))
    base = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if seed % 2:
        base = np.where(g.random((h, w, 1)) < 0.15, base // 4, 200 + base // 5).astype(np.uint8)
    return base


def ctc_case(seed, B, nq, C, bias, lmax):
    """Seeded head outputs + label sequences for the CTC-loss tests (shared with tests/golden/make_golden_ctc.py):
    logits ~ N(bias, 1) with a few confident queries per line, boxes uniform, ragged label sequences incl. an empty one and
    repeated characters."""
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    logits = (g.standard_normal((B, nq, C)) + bias).astype(np.float32)
    for b in range(B):
        hot = g.choice(nq, size=max(2, nq // 6), replace=False)
        logits[b, hot, g.integers(0, C, hot.shape[0])] += 9.0
    boxes = g.uniform(0.02, 0.98, (B, nq, 4)).astype(np.float32)
    labels = []
    for b in range(B):
        L = int(g.integers(1, min(lmax, nq) + 1))
        seq = g.integers(0, C, L).tolist()
        if L > 3:
            seq[2] = seq[1]                                        # a repeated character: needs the blank between them
        labels.append(seq)
    if B > 2:
        labels[-1] = []                                            # an empty transcription
    return {"pred_logits": torch.from_numpy(logits), "pred_boxes": torch.from_numpy(boxes)}, labels


# ---- margin-aware comparison of decoded outputs: moved to oracle/compare.py (checker code shared with bench.py's parity leg) -------
from oracle.compare import compare_decoded, query_decisions, safe_reading, tie_aware_compare  # noqa: E402,F401


# ---- n-gram re-scoring fixtures (shared by tests/golden/make_golden_ngram.py and the tests) -------------------------------------
def ngram_case(seed):
    """Seeded head outputs of ONE line whose argmax sequence looks like text: words of letters / digits / dashes separated by
    spaces and punctuation, blanks in between.  charset = the model's (label c <-> emission channel c + 1); ngram_charset = the
    n-gram side's table indexed by emission channel (index 0 = the CTC token)."""
    g = np.random.Generator(np.random.PCG64(4000 + seed))
    charset = list("abcdefgHIJ 0123-.,")
    ngram_charset = ["<ctc>"] + charset
    ignore = [ngram_charset.index(c) for c in " .,"]
    nq, C = 40, len(charset)
    logits = np.full((1, nq, C), -9.0, dtype=np.float32)
    cx = np.sort(g.uniform(0.02, 0.98, nq)).astype(np.float32)
    for q in range(nq):
        r = g.random()
        if r < 0.25:
            continue                                               # blank query
        c = int(g.integers(0, C)) if r < 0.9 else charset.index(" ")
        logits[0, q, c] = float(g.uniform(2.0, 8.0))
        if g.random() < 0.2:
            logits[0, q, int(g.integers(0, C))] = float(g.uniform(-1.0, 1.5))
    boxes = np.stack([cx, np.full(nq, 0.5, np.float32), np.full(nq, 0.02, np.float32), np.full(nq, 0.8, np.float32)], -1)[None]
    perm = g.permutation(nq)                                      # queries are not in reading order in the head output
    return ({"pred_logits": torch.from_numpy(logits[:, perm]), "pred_boxes": torch.from_numpy(boxes[:, perm].copy())},
            charset, ngram_charset, ignore)


def fake_ctc_decoder(ngram_charset):
    """A deterministic stand-in with torchaudio's ctc_decoder interface: greedy CTC collapse of the emissions, upper-cased, returned
    as hypothesis.words (a list of strings) -- enough to show WHICH spans were sent to the decoder and where its output lands."""
    class _H:
        def __init__(self, words):
            self.words = words

    def dec(em):
        lab = em[0].argmax(-1).tolist()
        out, prev = [], None
        for v in lab:
            if v != prev and v != 0:
                out.append(ngram_charset[v].upper())
            prev = v
        return [[_H(out)]]
    return dec


# ---- deformable-sampler plans and sampling patterns (shared by tests/test_host_logic.py and tests/test_gpu_msda_plans.py) -----------
def canvas_level_hw(H, W, levels=4, s0=3):
    """Encoder level shapes of an H x W canvas: every stride-2 stage maps n to ceil(n / 2), level l has stride 2^(s0 + l)."""
    return [(-(-H // (1 << (s0 + l))), -(-W // (1 << (s0 + l)))) for l in range(levels)]


def msda_enc_plan(level_hw, elem, halo):
    """Python restatement of make_plan (dtlr_amd/csrc/msda_enc.hip): the LDS window plan dtlr_msda_encoder_forward launches for these
    level shapes, element size of the value (4 = fp32, 2 = 16-bit) and halo.  Level-0 tiles of TW0 columns; level l stages
    wmax[l] = ceil(TW0 W_l / W_0) + 2 halo + 1 columns of every row (at most W_l: "clamped"), plus a token table of one int per
    query.  The widest TW0 of {64, 32, 16} within 80 KB (two workgroups per CU) wins, then the widest of {64, ..., 4} within 160 KB.
    -> dict(TW0, cap, wmax, clamped, lds), or None when no plan fits."""
    Hs, Ws = [int(h) for h, _ in level_hw], [int(w) for _, w in level_hw]
    if len(Hs) != 4 or min(Hs + Ws) <= 0:
        return None
    W0 = Ws[0]
    for cap, tws in ((80 * 1024, (64, 32, 16)), (160 * 1024, (64, 32, 16, 8, 4))):
        for tw in tws:
            span = [(tw * w + W0 - 1) // W0 for w in Ws]
            full = [s + 2 * halo + 1 for s in span]
            wmax = [min(f, w) for f, w in zip(full, Ws)]
            pix = sum(h * wm for h, wm in zip(Hs, wmax))
            nqmax = sum(h * (s + 1) for h, s in zip(Hs, span))
            lds = ((pix * 32 * elem + 15) & ~15) + nqmax * 4
            if lds <= cap:
                return dict(TW0=tw, cap=cap, wmax=wmax, clamped=[f > w for f, w in zip(full, Ws)], lds=lds)
    return None


MSDA_HALOS = (0, 8, 16, 24)          # the halos the engine's calibration picks from (8, 16, 24) and the window-only plan (0)


def msda_offsets(N, Lq, M, level_hw, seed, halo_max=max(MSDA_HALOS), P=4):
    """Deterministic sampling offsets [N, Lq, M, L, P, 2] (x, y in pixels of the SAMPLED level) in three regimes, one per group of heads:
    heads 0..M/2-1 a dense sweep -- x on a 1/8-px grid across +-(halo_max + 3) columns, y on a 1/8-px grid across +-(H_l + 1) rows, so
    samples cross every staged-window edge of every halo up to halo_max, the global path and both map borders (with power-of-two level
    sizes, h_im / w_im land exactly on -1 and on H / W); the next quarter Gaussian with sigma = 8 px (a trained checkpoint); the rest
    Gaussian with sigma = 40 px (far samples: mostly the global path or outside the map)."""
    g = np.random.Generator(np.random.PCG64(seed))
    L = len(level_hw)
    off = np.empty((N, Lq, M, L, P, 2), dtype=np.float32)
    ms, mg = M // 2, M // 2 + M // 4
    kx = 8 * (halo_max + 3)
    for l, (h, _) in enumerate(level_hw):
        ky = 8 * (int(h) + 1)
        off[:, :, :ms, l, :, 0] = g.integers(-kx, kx + 1, (N, Lq, ms, P)) / 8.0
        off[:, :, :ms, l, :, 1] = g.integers(-ky, ky + 1, (N, Lq, ms, P)) / 8.0
    off[:, :, ms:mg] = g.standard_normal((N, Lq, mg - ms, L, P, 2)) * 8.0
    off[:, :, mg:] = g.standard_normal((N, Lq, M - mg, L, P, 2)) * 40.0
    return torch.from_numpy(off)


def msda_row(off, seed):
    """The raw [offsets | attention logits] projection row [N, Lq, M * L * P * 3] fp32 the samplers read, for offsets [N, Lq, M, L, P, 2]."""
    N, Lq, M, L, P, _ = off.shape
    g = np.random.Generator(np.random.PCG64(seed))
    logits = torch.from_numpy((g.standard_normal((N, Lq, M * L * P)) * 1.5).astype(np.float32))
    return torch.cat([off.reshape(N, Lq, M * L * P * 2), logits], -1).contiguous()


def msda_oracle_from_row(O, value, shapes, row, ref):
    """The oracle the sampler tests compare with: locations in fp32 from the row's offsets (as the kernels compute them), the bilinear
    gather with the value and the softmaxed attention weights promoted to fp64.  -> [N, Lq, M * D] fp64.
    h_im = loc * H - 0.5 is rounded once, as the kernels' fused multiply-add does (O.ms_deform_attn_core(fma_im=True)): at a level
    wider than 256 columns the oracle's separate rounding of the product moves lh by up to half an fp32 ulp of h_im (2^-16), and the
    result by up to 6.9e-6 on the Chinese 128x2560 case of tests/test_gpu_msda_plans.py -- more than the fp32 bound of 5e-6.  The
    older sampler tests use levels at most 256 columns wide, where the product is exact or small, and never met the difference."""
    N, Lq, _ = row.shape
    M, L = value.shape[2], shapes.shape[0]
    P = row.shape[-1] // (M * L * 3)
    r = row.float()
    off = r[..., : M * L * P * 2].reshape(N, Lq, M, L, P, 2)
    aw = torch.softmax(r[..., M * L * P * 2:].reshape(N, Lq, M, L * P).double(), -1).view(N, Lq, M, L, P)
    loc = O.msda_sampling_locations(ref, off, shapes, P)
    return O.ms_deform_attn_core(value.double(), shapes, loc, aw, fma_im=True)


def per_line_geometry(sizes, level_hw, s0=3, device="cuda:0"):
    """Encoder reference points enc_ref [B, S, 4, 2], valid_ratios [B, 4, 2] and the padding mask mask_flat [B, S] of a per-line canvas
    of lines with image extents `sizes` [(h, w)], from ops.geometry_ext (on the device): each line's ratios differ by level
    (ceil(h / 2^s) / H_l), unlike a padded batch's uniform ones."""
    from dtlr_amd import ops
    ext = torch.tensor(sizes, dtype=torch.int32, device=device)
    le = torch.zeros((4, 256), dtype=torch.float32, device=device)
    g = ops.geometry_ext(ext, s0, level_hw, le, 10000.0, 10000.0, torch.float32)
    return {k: g[k].cpu() for k in ("enc_ref", "valid_ratios", "mask_flat")}


# Canvases the encoder-sampler plan tests run (tests/test_gpu_msda_plans.py): (name, H, W, per-line image extents or None).  Every case
# runs at every halo of MSDA_HALOS whose plan fits; tests/test_host_logic.py checks that together they reach all 16 (value element size,
# TW0, LDS cap) plans make_plan can choose.
MSDA_PLAN_CASES = [
    ("latin_128x2048", 128, 2048, None),
    ("chinese_128x2560", 128, 2560, None),
    ("eval_83x1328", 83, 1328, None),
    ("iam_96x1333", 96, 1333, None),
    ("tall_184x2048", 184, 2048, None),
    ("tall_200x2048", 200, 2048, None),
    ("tall_200x300", 200, 300, None),
    ("short_8x1040", 8, 1040, None),
    ("mid_48x1040", 48, 1040, None),
    ("per_line_128x1333", 128, 1333, [(96, 1333), (83, 1330), (70, 1100), (128, 1024)]),
]


def msda_plan_coverage(cases=MSDA_PLAN_CASES, halos=MSDA_HALOS):
    """{(elem, TW0, cap): [(case, halo)]} over the cases' canvases, both value element sizes and every halo that fits."""
    cov = {}
    for name, H, W, _ in cases:
        lhw = canvas_level_hw(H, W)
        for elem in (2, 4):
            for halo in halos:
                p = msda_enc_plan(lhw, elem, halo)
                if p is not None:
                    cov.setdefault((elem, p["TW0"], p["cap"]), []).append((name, halo))
    return cov
