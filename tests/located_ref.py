"""CPU restatement of the located decoders ("Located transcripts"), written against the stated semantics in plain
fp32 / fp64 numpy, and the seeded "planted" head outputs the located tests share.  Test infrastructure: nothing here is imported
by the package.

blank_located / nms_located return, per line, a dict of numpy arrays:
    labels, query (, rank) int32 ; score fp32 ; score64 fp64 (the same formula with every operation in fp64) ; box [n,4] fp32 ; length
Every discrete decision (blank or not, argmax, kept or suppressed, above the threshold or not, the order) is taken in fp32, as the
device takes it; the planted lines keep each of them far from its threshold (margins(), checked by tests/test_located_host.py), so
the two cannot disagree through the last bit of an exponential.
Tie rules: reading order by ascending cx, equal cx -> the lower query first; flat top-k by descending logit, equal logits -> the
lower flat index first; NMS in that order; survivors by ascending cx' = (x0 + x1) / 2, equal cx' -> the entry earlier in the
descending-score order first.  (-0.0 and +0.0 are one value here; the blank decoders' sort key tells them apart -- a cx is a sigmoid's
output and never -0.0.)
"""
import numpy as np
import torch

F32 = np.float32


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _sigmoid(x):
    """1 / (1 + exp(-x)) in x's precision"""
    one = x.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-x))


def xyxy(boxes):
    """cxcywh -> xyxy in fp32, every product / sum / difference rounded on its own (numpy never contracts)"""
    b = _np(boxes).astype(F32)
    hw, hh = F32(0.5) * b[..., 2], F32(0.5) * b[..., 3]
    return np.stack([b[..., 0] - hw, b[..., 1] - hh, b[..., 0] + hw, b[..., 1] + hh], -1).astype(F32)


def _scale(box, hw):
    h, w = (F32(1), F32(1)) if hw is None else (F32(hw[0]), F32(hw[1]))
    return (box * np.array([w, h, w, h], dtype=F32)).astype(F32)


def _query_step(lg, eps, dt):
    """per query: (label or -1 = blank, top) with the blank construction, all in precision dt"""
    p = _sigmoid(lg.astype(dt))
    s = p.sum(-1)
    best, arg = p.max(-1), p.argmax(-1)                          # argmax: the first maximum
    e = dt(F32(eps))
    low = s < dt(1) - e
    blank = np.where(low, dt(1) - s, e)
    top = np.where(low, best, (dt(1) - e) * best / s)
    return np.where(blank >= top, -1, arg).astype(np.int32), top, s, blank


def blank_located(logits, boxes, eps, src_hw=None):
    lg, bx = _np(logits).astype(F32), _np(boxes).astype(F32)
    hw = None if src_hw is None else _np(src_hw).astype(F32)
    out = []
    for b in range(lg.shape[0]):
        nq = lg.shape[1]
        if not np.isfinite(lg[b]).all():
            out.append(dict(labels=np.zeros(0, np.int32), query=np.zeros(0, np.int32), rank=np.zeros(0, np.int32), score=np.zeros(0, F32),
                            score64=np.zeros(0), box=np.zeros((0, 4), F32), length=-1))
            continue
        lab, top, _, _ = _query_step(lg[b], eps, F32)
        _, top64, _, _ = _query_step(lg[b], eps, np.float64)
        order = np.lexsort((np.arange(nq), bx[b, :, 0]))         # ascending cx, then the lower query
        keep = lab[order] >= 0
        q = order[keep].astype(np.int32)
        out.append(dict(labels=lab[q], query=q, rank=np.nonzero(keep)[0].astype(np.int32), score=top[q].astype(F32), score64=top64[q],
                        box=_scale(xyxy(bx[b])[q], None if hw is None else hw[b]), length=int(keep.sum())))
    return out


def _iou(a, c):
    """fp32 IoU of box a against boxes c, the expression of torchvision's nms"""
    area_a, area_c = (a[2] - a[0]) * (a[3] - a[1]), (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
    iw = np.maximum(np.minimum(a[2], c[:, 2]) - np.maximum(a[0], c[:, 0]), F32(0))
    ih = np.maximum(np.minimum(a[3], c[:, 3]) - np.maximum(a[1], c[:, 1]), F32(0))
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area_a + area_c - inter)


def flat_topk(lg_row, k):
    """positions of the k largest logits of a [nq, C] row, descending, equal logits: the lower flat index first"""
    flat = lg_row.reshape(-1)
    return np.argsort(-flat.astype(np.float64), kind="stable")[:k]


def nms_located(logits, boxes, TH, NM, src_hw=None):
    lg, bx = _np(logits).astype(F32), _np(boxes).astype(F32)
    hw = None if src_hw is None else _np(src_hw).astype(F32)
    B, nq, C = lg.shape
    k = min(900, nq)
    out = []
    for b in range(B):
        idx = flat_topk(lg[b], k)
        val = lg[b].reshape(-1)[idx]
        sc, sc64 = _sigmoid(val), _sigmoid(val.astype(np.float64))
        pos = np.argsort(-sc.astype(np.float64), kind="stable")  # descending score, equal scores: the lower position first
        nb = xyxy(bx[b])[idx[pos] // C]                          # normalised boxes in sorted order
        removed = np.zeros(k, bool)
        kept = []
        for i in range(k):
            if removed[i]:
                continue
            kept.append(i)
            removed[i + 1:] |= _iou(nb[i], nb[i + 1:]) > F32(NM)
        kept = np.array([i for i in kept if sc[pos[i]] > F32(TH)], dtype=np.int64)
        cx = ((nb[kept, 0] + nb[kept, 2]) * F32(0.5)).astype(F32)
        kept = kept[np.argsort(cx.astype(np.float64), kind="stable")]
        src = pos[kept]
        out.append(dict(labels=(idx[src] % C).astype(np.int32), query=(idx[src] // C).astype(np.int32), score=sc[src].astype(F32),
                        score64=sc64[src], box=_scale(nb[kept], None if hw is None else hw[b]), length=len(kept)))
    return out


def words(labels, scores, boxes, space_label):
    """[(i0, i1, box, score)]: maximal runs [i0, i1) of characters that are not the space; box = (min x0, min y0, max x1, max y1),
    score = the minimum.  space_label None: the whole (non-empty) line is one word."""
    labels = [int(v) for v in labels]
    runs, start = [], None
    for i, v in enumerate(labels + [space_label if space_label is not None else -12345]):
        sep = i == len(labels) or (space_label is not None and v == space_label)
        if not sep and start is None:
            start = i
        if sep and start is not None:
            runs.append((start, i))
            start = None
    out = []
    for i0, i1 in runs:
        bb = np.asarray(boxes, dtype=F32)[i0:i1]
        out.append((i0, i1, (float(bb[:, 0].min()), float(bb[:, 1].min()), float(bb[:, 2].max()), float(bb[:, 3].max())),
                    float(np.min(np.asarray(scores, dtype=F32)[i0:i1]))))
    return out


# ------------------------------------------------------------------------------------------------------- planted head outputs
HI, LO = 4.0, -6.0            # a character's class logit, and every other logit


def planted(seed, B, nq, C, m=None, duplicates=False):
    """Head outputs whose decode is known by construction.  Per line, m character queries (default about nq / 3) carry one class logit
    at HI, everything else is at LO; the cx of the nq queries sit on a grid of pitch 1 / nq with +-0.1 pitch of jitter, boxes are
    half a pitch wide, and the queries are shuffled.  duplicates (the NMS tests): every character gets a second query on the same box
    moved by 8 % of its width (IoU 0.85) with the same class at logit 3, and the line's first character also a second class at
    logit 3 on its own query.  -> {"pred_logits" [B,nq,C], "pred_boxes" [B,nq,4]} fp32 CPU tensors."""
    g = np.random.Generator(np.random.PCG64(7000 + seed))
    lg = np.full((B, nq, C), LO, dtype=F32)
    bx = np.empty((B, nq, 4), dtype=F32)
    for b in range(B):
        mm = max(1, nq // 3) if m is None else m
        cx = (np.arange(nq) + 0.5 + g.uniform(-0.1, 0.1, nq)) / nq
        perm = g.permutation(nq)
        bx[b, perm, 0] = cx
        bx[b, :, 1] = g.uniform(0.45, 0.55, nq)
        bx[b, :, 2] = 0.5 / nq
        bx[b, :, 3] = g.uniform(0.5, 0.7, nq)
        slots = np.sort(g.choice(nq // 2 if duplicates else nq, size=min(mm, nq // 2 if duplicates else nq), replace=False))
        chars = perm[2 * slots] if duplicates else perm[slots]
        cls = g.integers(0, C, len(chars))
        lg[b, chars, cls] = HI
        if duplicates:
            twins = perm[2 * slots + 1]
            bx[b, twins] = bx[b, chars]
            bx[b, twins, 0] += F32(0.081) * bx[b, chars, 2]
            lg[b, twins, cls] = 3.0
            if C > 1:
                lg[b, chars[0], (cls[0] + 1) % C] = 3.0
    return {"pred_logits": torch.from_numpy(lg), "pred_boxes": torch.from_numpy(bx)}


def margins(outputs, eps, TH=None, NM=None):
    """How far the planted lines keep the discrete decisions from their thresholds, in fp64:
    branch  min |s - (1 - eps)|                       (which form the blank construction takes)
    blank   min |blank - top| / max(blank, top)       (blank or character)
    second  min over queries of (best - second best class probability) / best, queries whose maximum is an exact tie left out
    and with TH / NM: score = min |sigmoid(logit) - TH| over the flat top-k, iou = min |IoU - NM| over pairs of entries above TH."""
    lg, bx = _np(outputs["pred_logits"]).astype(np.float64), _np(outputs["pred_boxes"])
    p = _sigmoid(lg)
    s = p.sum(-1)
    e = float(F32(eps))
    low = s < 1 - e
    best = p.max(-1)
    blank = np.where(low, 1 - s, e)
    top = np.where(low, best, (1 - e) * best / s)
    res = dict(branch=float(np.abs(s - (1 - e)).min()), blank=float((np.abs(blank - top) / np.maximum(blank, top)).min()))
    if lg.shape[-1] > 1:
        part = np.partition(lg, -2, axis=-1)
        gap = np.where(part[..., -1] == part[..., -2], np.inf, (best - _sigmoid(part[..., -2])) / best)
        res["second"] = float(gap.min())
    if TH is not None:
        B, nq, C = lg.shape
        sc_gap, iou_gap = np.inf, np.inf
        for b in range(B):
            idx = flat_topk(_np(outputs["pred_logits"])[b], min(900, nq))
            sc = _sigmoid(lg[b].reshape(-1)[idx])
            sc_gap = min(sc_gap, float(np.abs(sc - TH).min()))
            nb = xyxy(bx[b])[idx[sc > TH] // C].astype(np.float64)
            for i in range(len(nb) - 1):
                iou = _iou(nb[i], nb[i + 1:])
                iou_gap = min(iou_gap, float(np.abs(iou - NM).min()))
        res.update(score=sc_gap, iou=iou_gap)
    return res
