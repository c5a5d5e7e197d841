"""Decoders and metrics of the reference's inference harness, batched on the GPU.

  convert_output_to_pred, NMS branch      <- evaluation.py:94-115   (scripts: --NMS 0.5 --TH 0.3)
  convert_output_to_pred, blank branch    <- evaluation.py:116-158  == SetCriterion.loss_CTC's
                                             blank construction (models/dino/dino.py:466-502)
                                             + engine.convert_output_to_pred (engine.py:511-530)
  CER / cumulative CER / normalisation    <- evaluation.py:296-334,430-450,517-529 ; engine.py:594-633
  WER, word splitting, gt normalisation   <- evaluation.py:358-428 ; engine.py:487-494,543-593
  per-character impact, WA, CR            <- evaluation.py:162-290
  the evaluation loop / CLI               <- evaluation.py:460-659  (dtlr_amd/eval_harness.py; `python -m dtlr_amd.evaluation`)

The reference decodes batch index 0 only (evaluation.py:154-155, batch size 1) with one `.item()`
device sync per character; here the whole batch is decoded on the device and ONE fixed-width record
per line (labels[nq] int32, length int32) crosses to the host -- the same record the data-parallel
driver all-gathers (dtlr_amd/dist.py).
"""
from __future__ import annotations

import dataclasses
import re
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from .dino import PostProcess, box_xyxy_to_cxcywh


def load_model(model, weights, device="cuda", new_class_embedding: bool = False, charset_size: Optional[int] = None,
               new_label_enc: bool = False, fix_enc_out_class: bool = False):
    """Checkpoint ingestion of the evaluation harness (evaluation.py:51-88), returning the model in eval mode on `device`.

    weights: path of a `checkpoint.pth` ({"model": state_dict}) or a state dict.  Without `new_class_embedding` the
    checkpoint is loaded as is (:54-59).  With it (HWDB / READ / cipher scripts) the class heads are first rebuilt to the
    dataset's charset size (:60-83): one Linear shared by the six decoder layers under `model.class_embed`, a separate
    bare Linear under `model.transformer.decoder.class_embed`, the two-stage head `enc_out_class_embed` unless
    `fix_enc_out_class`, and with `new_label_enc` the denoising label embedding (:84-85, unused at inference).
    charset_size None = take it from the checkpoint's `class_embed.0.weight` (what a matching charset has to equal)."""
    from . import weights as W
    sd = W.load_checkpoint_state_dict(weights) if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") else weights
    if new_class_embedding:
        features_dim = model.class_embed[0].weight.data.shape[1]
        n = int(charset_size) if charset_size is not None else W.num_classes_of(sd)
        new_class_embed = nn.Linear(features_dim, n)
        if not model.dec_pred_class_embed_share:
            raise NotImplementedError("load_model: the reference's head-resize flow only exists for dec_pred_class_embed_share "
                                      "(evaluation.py:75-79 leaves class_embed_layerlist undefined otherwise)")
        model.class_embed = nn.ModuleList([new_class_embed for _ in range(model.transformer.num_decoder_layers)])
        model.transformer.decoder.class_embed = nn.Linear(features_dim, n)
        if not fix_enc_out_class:
            model.transformer.enc_out_class_embed = nn.Linear(features_dim, n)
        if new_label_enc:
            model.label_enc = nn.Embedding(n + 1, features_dim)
    model.load_state_dict(sd)
    model.eval()
    return model.to(device)


@torch.no_grad()
def blank_probabilities(outputs: Dict[str, torch.Tensor], eps: float, scale: float = 1.0) -> torch.Tensor:
    """[B, nq, C+1] probabilities with the blank channel at index 0, queries sorted by box cx (HIP kernels: dtlr_blank_emissions)."""
    from . import ops
    return ops.blank_emissions(outputs["pred_logits"], outputs["pred_boxes"], eps, scale)


@torch.no_grad()
def decode_blank_records(outputs, eps: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device-side blank/argmax decode (HIP kernel, one workgroup per line) -> (labels [B,nq] int32
    left-packed, -1 padded; lengths [B] int32).  No repeat collapse (engine.py:511-530, duplicate=False)."""
    from . import ops
    C = outputs["pred_logits"].shape[-1]
    return ops.decode_blank(outputs["pred_logits"], outputs["pred_boxes"], 0.03 / C if eps is None else eps)


def _ctc_targets(logits, target_labels, what: str):
    """label lists -> (targets [B, max(Lmax, 1)] int32 = label + 1, lengths [B] int32, Lmax) on the logits' device"""
    B = logits.shape[0]
    if len(target_labels) != B:
        raise ValueError(f"{what}: {len(target_labels)} label sequences for a batch of {B}")
    lens = [len(t) for t in target_labels]
    Lmax = max(lens) if lens else 0
    tt = torch.zeros((B, max(Lmax, 1)), dtype=torch.int32)
    for i, t in enumerate(target_labels):
        if len(t):
            tt[i, : len(t)] = torch.as_tensor([int(v) for v in t], dtype=torch.int32) + 1
    tl = torch.tensor(lens, dtype=torch.int32)
    return tt.to(logits.device), tl.to(logits.device), Lmax


def loss_ctc(outputs, target_labels: Sequence[Sequence[int]], eps: float = 0.003, filler: float = 1e-5) -> torch.Tensor:
    """Forward value of `SetCriterion.loss_CTC` (models/dino/dino.py:457-551) as engine.evaluate_CTC logs it
    (engine.py:381): HIP kernels (per-query sigmoid sums chip-wide, then one workgroup per line for the reading-order sort
    and the CTC alpha recursion over the 2 nq interleaved steps); the 'mean' reduction of nn.CTCLoss -- per-line NLL over
    max(target length, 1), averaged over the batch -- is applied here.  target_labels: per line, the label indices
    (charset positions, WITHOUT the +1 blank shift).  Returns a 0-d fp32 CUDA tensor."""
    from . import ops
    logits = outputs["pred_logits"]
    tt, tl, Lmax = _ctc_targets(logits, target_labels, "loss_ctc")
    nll = ops.ctc_loss_interleaved(logits, outputs["pred_boxes"], tt, tl, Lmax, eps, filler)
    return (nll / tl.clamp(min=1).float()).mean()


def loss_ctc_backward(outputs, target_labels: Sequence[Sequence[int]], eps: float = 0.003, filler: float = 1e-5):
    """`loss_ctc` and its gradient with respect to outputs["pred_logits"], as engine.train_one_epoch_CTC's
    `criterion.loss_CTC(outputs, targets, None, None)` + backward produce them (engine.py:200-212): HIP kernels
    (dtlr_ctc_loss_interleaved_backward: the forward's alpha recursion, a beta recursion over the same 2 nq frames, then the
    blank construction's chain rule chip-wide).  A line whose transcription does not fit 2 nq frames contributes loss 0 and gradient 0
    (zero_infinity).  A label outside 0..C-1 raises ValueError (the labels are host lists: the check costs no synchronisation).
    Returns (loss: 0-d fp32 CUDA tensor with loss_ctc's bits, dlogits [B,nq,C] fp32)."""
    from . import ops
    logits = outputs["pred_logits"]
    C = logits.shape[-1]
    for i, t in enumerate(target_labels):
        if any(not 0 <= int(v) < C for v in t):
            raise ValueError(f"loss_ctc_backward: line {i} has a label outside 0..{C - 1}")
    tt, tl, Lmax = _ctc_targets(logits, target_labels, "loss_ctc_backward")
    nll, dlogits = ops.ctc_loss_interleaved_backward(logits, outputs["pred_boxes"], tt, tl, Lmax, eps, filler)
    return (nll / tl.clamp(min=1).float()).mean(), dlogits


def evaluate_ctc_step(outputs, target_labels: Sequence[Sequence[int]]) -> Dict[str, float]:
    """One batch of engine.evaluate_CTC (engine.py:371-411): the CTC loss value and the summed per-line character error rate
    of the argmax decode that shares the loss's blank construction (eps = 0.003; engine.py:511-530, 544-568, 594-633).
    Returns {"loss_CTC", "cer_sum", "n"}: the caller accumulates cer_sum / n over the loader like engine.py:413-420."""
    loss = loss_ctc(outputs, target_labels)
    labels, lengths = decode_blank_records(outputs, eps=0.003)
    preds = records_to_lists(labels, lengths)
    cer = sum(character_error_rate(p, [int(v) for v in t]) for p, t in zip(preds, target_labels))
    return {"loss_CTC": float(loss.item()), "cer_sum": float(cer), "n": len(preds)}


def records_to_lists(labels: torch.Tensor, lengths: torch.Tensor) -> List[List[int]]:
    """decode records -> label lists.  A length of -1 marks a line whose logits were not finite (dtlr_decode_blank flags it on the device):
    on the float16 / split engines that is an activation beyond fp16's range (65504) -- raise instead of returning garbage."""
    lab, ln = labels.cpu().tolist(), lengths.cpu().tolist()
    bad = [i for i, n in enumerate(ln) if n < 0]
    if bad:
        from ._lib import DTLRError
        raise DTLRError(f"non-finite logits in line(s) {bad[:8]}{'...' if len(bad) > 8 else ''}: on the float16 / f32s engines an activation left fp16's "
                        "range (65504) -- run this checkpoint on the bfloat16 or the exact float32 engine")
    return [row[:n] for row, n in zip(lab, ln)]


def decode_blank(outputs, eps: Optional[float] = None) -> List[List[int]]:
    return records_to_lists(*decode_blank_records(outputs, eps))


@torch.no_grad()
def decode_nms(outputs, postprocessor: Optional[PostProcess] = None, TH: float = 0.3, NM: float = 0.5) -> List[List[int]]:
    """evaluation.py:94-115 for every line of the batch: PostProcess with num_select = #queries (900), NMS IoU NM on a (1,1)
    canvas, keep score > TH, order by box cx.  Top-k and the per-line filtering are batched device ops, the NMS one HIP launch
    for the whole batch (dtlr_nms); the only host transfers are the NMS counts and the final label lists."""
    pp = postprocessor or PostProcess()
    B, nq, _ = outputs["pred_logits"].shape
    pp.num_select, pp.nms_iou_threshold = min(900, nq) if nq < 900 else 900, NM
    dev = outputs["pred_logits"].device
    res = []
    for o in pp(outputs, torch.ones((B, 2), device=dev)):
        boxes = box_xyxy_to_cxcywh(o["boxes"])
        sel = o["scores"] > TH
        order = torch.sort(boxes[sel][:, 0], descending=False)[1]
        res.append(o["labels"].long()[sel][order])
    return [[int(i) for i in r.cpu().tolist()] for r in res]


# ------------------------------------------------------------------------------- located transcripts ("Located transcripts")
Box = Tuple[float, float, float, float]


@dataclasses.dataclass
class LocatedChar:
    """One decoded character: its label, the score the decoder gave it, its xyxy box, the query it came from and (blank decoder) its
    rank = the query's position in the line's reading order = its frame in the n-gram emissions.  A character placed by the forced
    alignment also carries `first` / `last`, the frames of the first and the last lattice frame its state holds (rank = the peak)."""
    label: int
    score: float
    box: Box
    query: int
    rank: Optional[int] = None
    first: Optional[int] = None
    last: Optional[int] = None


@dataclasses.dataclass
class LocatedWord:
    """A word of a located line: `labels`, the union `box` and the minimum `score` of its characters, `chars` = (i0, i1), the range
    of the line's `chars` it covers (None when it covers none), and `source`: "kept" = the detection decoder's own characters,
    "ngram" = a span the n-gram beam re-scored (its labels are the beam's; `same` tells whether they equal the detections').
    `aligned`: the characters of a word the beam rewrote, placed by the forced alignment of its labels over its own frames
    (ngram.rescored_located_batch(align_rewritten=True)); None otherwise, [] when the labels do not fit the frames."""
    labels: List[int]
    box: Box
    score: float
    chars: Optional[Tuple[int, int]]
    source: str = "kept"
    same: bool = True
    aligned: Optional[List[LocatedChar]] = None


@dataclasses.dataclass
class LocatedLine:
    labels: List[int]
    chars: List[LocatedChar]
    words: List[LocatedWord]
    decoder: str = "blank"
    logp: Optional[float] = None        # decoder "align": ln p of the best path of `labels`; -inf: they do not fit the line

    def text(self, charset: Sequence) -> str:
        return labels_to_string(self.labels, charset)


def union_box(boxes: Sequence[Box]) -> Box:
    return (min(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), max(b[3] for b in boxes))


def located_words(chars: Sequence[LocatedChar], space_label: Optional[int]) -> List[LocatedWord]:
    """A word is a maximal run of characters whose label is not `space_label`; its box is the union of theirs, its score their
    minimum.  space_label None (scripts without a word separator): the line is one word.  An empty line has no words."""
    words: List[LocatedWord] = []
    start = None
    for i in range(len(chars) + 1):
        sep = i == len(chars) or (space_label is not None and chars[i].label == space_label)
        if not sep and start is None:
            start = i
        if sep and start is not None:
            run = chars[start:i]
            words.append(LocatedWord([c.label for c in run], union_box([c.box for c in run]), min(c.score for c in run), (start, i)))
            start = None
    return words


def space_label_of(charset: Optional[Sequence]) -> Optional[int]:
    """the charset's ' ' index, or None"""
    cs = list(charset) if charset is not None else []
    return cs.index(" ") if " " in cs else None


@torch.no_grad()
def decode_blank_located_records(outputs, eps: Optional[float] = None, src_hw=None) -> Dict[str, torch.Tensor]:
    """decode_blank_records with every character's record (dtlr_decode_blank_located): device tensors labels, query, rank [B,nq] int32,
    score [B,nq] fp32, box [B,nq,4] fp32 xyxy, lengths [B] int32.  src_hw: [B,2] (h, w) of the source images -> boxes in their pixels;
    None: normalised boxes."""
    from . import ops
    C = outputs["pred_logits"].shape[-1]
    return ops.decode_blank_located(outputs["pred_logits"], outputs["pred_boxes"], 0.03 / C if eps is None else eps, src_hw)


@torch.no_grad()
def decode_nms_located_records(outputs, TH: float = 0.3, NM: float = 0.5, src_hw=None) -> Dict[str, torch.Tensor]:
    """The NMS decoder (evaluation.py:94-115) of the whole batch as one device path (dtlr_topk_flat + dtlr_decode_nms_located, no host
    round trip): device tensors labels, query [B,k] int32, score [B,k] fp32, box [B,k,4] fp32 xyxy, lengths [B] int32, k = min(900, nq)."""
    from . import ops
    return ops.decode_nms_located(outputs["pred_logits"], outputs["pred_boxes"], TH, NM, src_hw)


def located_records_to_lines(rec: Dict[str, torch.Tensor], space_label: Optional[int] = None, decoder: str = "blank") -> List[LocatedLine]:
    """located records (device or host) -> LocatedLine per line: one copy per tensor, then host lists.  A length of -1 raises like
    records_to_lists."""
    host = {k: v.cpu() for k, v in rec.items()}
    ln = host["lengths"].tolist()
    records_to_lists(host["labels"], host["lengths"])                       # raises on a line with non-finite logits
    lab, qry, sc, bx = host["labels"].tolist(), host["query"].tolist(), host["score"].tolist(), host["box"].tolist()
    rk = host["rank"].tolist() if "rank" in host else None
    lines = []
    for b, n in enumerate(ln):
        chars = [LocatedChar(lab[b][i], sc[b][i], tuple(bx[b][i]), qry[b][i], rk[b][i] if rk is not None else None) for i in range(n)]
        lines.append(LocatedLine(lab[b][:n], chars, located_words(chars, space_label), decoder))
    return lines


def decode_blank_located(outputs, eps: Optional[float] = None, src_hw=None, space_label: Optional[int] = None) -> List[LocatedLine]:
    return located_records_to_lines(decode_blank_located_records(outputs, eps, src_hw), space_label, "blank")


def decode_nms_located(outputs, TH: float = 0.3, NM: float = 0.5, src_hw=None, space_label: Optional[int] = None) -> List[LocatedLine]:
    return located_records_to_lines(decode_nms_located_records(outputs, TH, NM, src_hw), space_label, "nms")


def located_line_to_json(line: LocatedLine, charset: Sequence, line_id: str) -> Dict:
    """The object `--layout-out` writes for one line image.  A word that carries aligned characters adds them as "aligned"."""
    cs = list(charset)
    char = lambda c: {"c": str(cs[c.label]), "label": c.label, "score": c.score, "box": list(c.box), "query": c.query}     # noqa: E731
    return {"id": line_id, "decoder": line.decoder, "text": line.text(cs),
            "chars": [char(c) for c in line.chars],
            "words": [{"text": labels_to_string(w.labels, cs), "box": list(w.box), "score": w.score,
                       "chars": list(w.chars) if w.chars is not None else None, **({"source": w.source} if line.decoder == "ngram" else {}),
                       **({"aligned": [dict(char(c), rank=c.rank, first=c.first, last=c.last) for c in w.aligned]}
                          if w.aligned is not None else {})}
                      for w in line.words]}


def aligned_line_to_json(line: LocatedLine, charset: Sequence, line_id: str) -> Dict:
    """The object `--align-out` writes for one line image: the located JSON of the transcript's characters (each with the frames it
    holds), plus the best path's "logp" (null when there is none) and "feasible"."""
    obj = located_line_to_json(line, charset, line_id)
    for d, c in zip(obj["chars"], line.chars):
        d.update(rank=c.rank, first=c.first, last=c.last)
    feasible = line.logp is not None and line.logp > float("-inf")
    obj.update(logp=line.logp if feasible else None, feasible=feasible)
    return obj


# ------------------------------------------------------------------------------- forced alignment
ALIGN_EMISSION_BYTES = 256 << 20        # the emissions of one chunk of lines stay under this (C = 7356: 900 x 7357 x 4 = 26 MB a line)


def query_boxes_xyxy(boxes: torch.Tensor, src_hw=None) -> torch.Tensor:
    """[B,nq,4] xyxy boxes of every query with PostProcess's arithmetic (box_cxcywh_to_xyxy, then the (W, H, W, H) scale as an
    element-wise product of its own): the bits of the located decoders' boxes."""
    from . import ops
    from .dino import box_cxcywh_to_xyxy
    boxes = boxes.float()
    out = box_cxcywh_to_xyxy(boxes)
    hw = ops._src_hw(src_hw, boxes.shape[0], boxes.device)
    if hw is not None:
        out = out * torch.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], dim=1)[:, None, :]
    return out


def gather_aligned(peak: torch.Tensor, order: torch.Tensor, allbox: torch.Tensor, line: Optional[torch.Tensor] = None):
    """peak [n,L] int32 frames (-1 padded) of spans on lines `line` [n] (None: span k is line k) -> (query [n,L] int32, -1 padded;
    box [n,L,4] fp32, 0 padded): query = order[line, peak], box = allbox[line, query]."""
    n, L = peak.shape
    valid = peak >= 0
    idx = peak.clamp(min=0).long()
    rows = (torch.arange(n, device=peak.device) if line is None else line.long().to(peak.device))[:, None].expand(n, L)
    query = order[rows, idx]
    box = torch.where(valid[:, :, None], allbox[rows, query.long()], allbox.new_zeros(()))
    return torch.where(valid, query, torch.full_like(query, -1)), box


@torch.no_grad()
def align_ctc_records(outputs, target_labels: Sequence[Sequence[int]], eps: float = 0.003, src_hw=None,
                      interleaved: bool = True) -> Dict[str, torch.Tensor]:
    """CTC forced alignment of every line against its KNOWN transcript (dtlr_ctc_align over the emissions of dtlr_blank_emissions, each
    line one span): where each character of target_labels[b] (label indices, no blank shift) sits.  Device tensors, left-packed, padded
    with -1 / 0: labels, query, rank (the peak frame), first, last [B,Lmax] int32, score [B,Lmax] fp32 (the emission at the peak),
    box [B,Lmax,4] fp32 xyxy (that query's box, bit for bit the located decoders'), lengths [B] int32 (-1: the transcript does not fit
    the line; all its rows are padding), logp [B] fp64 (ln p of the best path, -inf then).  interleaved: loss_CTC's lattice (a filler
    frame after every query) or the plain frames.  A label outside 0..C-1 raises ValueError."""
    from . import ops
    logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
    B, nq, C = logits.shape
    if len(target_labels) != B:
        raise ValueError(f"align_ctc_records: {len(target_labels)} label sequences for a batch of {B}")
    lens = [len(t) for t in target_labels]
    Lmax = max(lens) if lens else 0
    tt = torch.zeros((B, Lmax), dtype=torch.int64)
    for i, t in enumerate(target_labels):
        if len(t):
            tt[i, : len(t)] = torch.as_tensor([int(v) for v in t], dtype=torch.int64) + 1
    dev = logits.device
    chunk = max(1, ALIGN_EMISSION_BYTES // (nq * (C + 1) * 4))
    parts = []
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        em = ops.blank_emissions(logits[b0:b1], boxes[b0:b1], eps)
        parts.append(ops.ctc_align(em, [(i, 0, nq) for i in range(b1 - b0)], tt[b0:b1], lens[b0:b1], interleaved))
        del em
    rec = {k: torch.cat([p[k] for p in parts]) for k in parts[0]} if parts else ops.ctc_align(logits.new_zeros((1, 1, 2)), [], [], [])
    order = ops.reading_order(boxes)
    query, box = gather_aligned(rec["peak"], order, query_boxes_xyxy(boxes, src_hw))
    labels = torch.where(rec["peak"] >= 0, (tt - 1).to(torch.int32).to(dev), torch.full((B, Lmax), -1, dtype=torch.int32, device=dev))
    return dict(labels=labels, query=query, rank=rec["peak"], first=rec["first"], last=rec["last"], score=rec["prob"], box=box,
                lengths=rec["length"], logp=rec["score"])


def aligned_chars(labels, query, rank, first, last, score, box, n: int) -> List[LocatedChar]:
    """host rows of an alignment record -> its first n characters"""
    return [LocatedChar(int(labels[i]), float(score[i]), tuple(box[i]), int(query[i]), int(rank[i]), int(first[i]), int(last[i]))
            for i in range(n)]


def align_ctc(outputs, target_labels: Sequence[Sequence[int]], eps: float = 0.003, src_hw=None, interleaved: bool = True,
              space_label: Optional[int] = None) -> List[LocatedLine]:
    """align_ctc_records as LocatedLines with decoder "align": `labels` are the transcript's, `chars` its characters where the best
    path puts them, words cut by located_words, `logp` the path's log-probability.  A transcript that does not fit its line gives a
    line without chars or words and logp = -inf."""
    host = {k: v.cpu().tolist() for k, v in align_ctc_records(outputs, target_labels, eps, src_hw, interleaved).items()}
    lines = []
    for b, n in enumerate(host["lengths"]):
        chars = aligned_chars(*(host[k][b] for k in ("labels", "query", "rank", "first", "last", "score", "box")), max(n, 0))
        lines.append(LocatedLine([int(v) for v in target_labels[b]], chars, located_words(chars, space_label), "align",
                                 float(host["logp"][b]) if n >= 0 else float("-inf")))
    return lines


# ------------------------------------------------------------------------------- keyword spotting
@dataclasses.dataclass
class KeywordHit:
    """One occurrence of a keyword in a line: `keyword` = its index in the list that was searched, `line` = the line's index in the
    batch, `start` / `end` = the first and the last frame (rank in reading order) of the hit, `ratio` = the log-likelihood ratio of its
    best path against the frame-wise argmax path over the same frames (<= 0), `conf` = exp(ratio / L), the geometric mean per character
    in (0, 1], `box` = the union of its characters' boxes, `chars` = its characters where the forced alignment of the hit's frames puts
    them."""
    keyword: int
    line: int
    start: int
    end: int
    ratio: float
    conf: float
    box: Box
    chars: List[LocatedChar]
    pattern: Optional[int] = None          # a hit of spot_patterns: the expression's index in the list (then `keyword` holds it too)


def _spot_tables(keywords: Sequence[Sequence[int]], C: int, min_conf: float):
    """keywords as label indices -> (emission channels = label + 1, min_ratio [Q] fp64 = L ln(min_conf))"""
    import math
    if not 0.0 <= float(min_conf) <= 1.0:
        raise ValueError(f"spot: min_conf {min_conf} outside 0..1")
    chans = []
    for i, z in enumerate(keywords):
        z = [int(v) for v in z]
        if any(not 0 <= v < C for v in z):
            raise ValueError(f"spot: keyword {i} has a label outside 0..{C - 1}")
        chans.append([v + 1 for v in z])
    ln = math.log(min_conf) if min_conf > 0 else float("-inf")
    return chans, torch.tensor([len(z) * ln if len(z) else ln for z in chans], dtype=torch.float64)


@torch.no_grad()
def spot_records(outputs, keywords: Sequence[Sequence[int]], min_conf: float = 0.5, max_hits: int = 4, eps: float = 0.003, src_hw=None,
                 with_chars: bool = False) -> Dict[str, torch.Tensor]:
    """Query-by-string keyword spotting of every keyword (label indices, no blank shift) in every line of the batch (dtlr_ctc_spot over
    the emissions of dtlr_blank_emissions, chunked under ALIGN_EMISSION_BYTES).  Device tensors: count [B,Q] int32, start / end [B,Q,H]
    int32 (frames = ranks in reading order, -1 padded), ratio [B,Q,H] fp64 and conf [B,Q,H] fp64 = exp(ratio / L) (0 padded), hits best
    first; a hit needs conf >= min_conf (min_conf 0: every keyword's best hit is returned wherever the keyword fits the line).
    with_chars: every hit of the batch is aligned by dtlr_ctc_align over its own frames [start, end + 1) of the plain lattice, and the
    record gains hit [n,3] int64 (line, keyword, h), query / rank / first / last [n,Lmax] int32, score [n,Lmax] fp32, box [n,Lmax,4]
    fp32 xyxy and logp [n] fp64 (the alignment's score), rows in (line, keyword, h) order: one host round trip for the span table.
    ValueError for a label outside 0..C-1, an empty or too long keyword, max_hits outside 1..16."""
    from . import ops
    logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
    B, nq, C = logits.shape
    chans, min_ratio = _spot_tables(keywords, C, min_conf)
    kw, kl = ops.ctc_spot_tables(chans, C + 1, max_hits)
    Q, Lmax, H, dev = len(chans), int(kw.shape[1]), int(max_hits), logits.device
    chunk = max(1, ALIGN_EMISSION_BYTES // (nq * (C + 1) * 4))
    parts, hits, aligned = [], [], []
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        em = ops.blank_emissions(logits[b0:b1], boxes[b0:b1], eps)
        rec = ops.ctc_spot(em, chans, min_ratio, H)
        parts.append(rec)
        if with_chars and Q:
            cnt, st, en = rec["count"].cpu(), rec["start"].cpu(), rec["end"].cpu()
            idx = [(b, q, h) for b in range(b1 - b0) for q in range(Q) for h in range(int(cnt[b, q]))]
            if idx:
                spans = [(b, int(st[b, q, h]), int(en[b, q, h]) + 1) for b, q, h in idx]
                aligned.append(ops.ctc_align(em, spans, kw[[q for _, q, _ in idx]], kl[[q for _, q, _ in idx]], False))
                hits += [(b0 + b, q, h) for b, q, h in idx]
        del em
    if parts:
        out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    else:
        out = dict(count=torch.empty((0, Q), dtype=torch.int32, device=dev), start=torch.empty((0, Q, H), dtype=torch.int32, device=dev),
                   end=torch.empty((0, Q, H), dtype=torch.int32, device=dev), ratio=torch.empty((0, Q, H), dtype=torch.float64, device=dev))
    taken = torch.arange(H, device=dev)[None, None, :] < out["count"][:, :, None]
    lens = kl.to(dev).double().clamp(min=1)[None, :, None]
    out["conf"] = torch.where(taken, torch.exp(out["ratio"] / lens), torch.zeros((), dtype=torch.float64, device=dev))
    if with_chars:
        n = len(hits)
        hit = torch.tensor(hits, dtype=torch.int64).reshape(n, 3).to(dev)
        if aligned:
            al = {k: torch.cat([p[k] for p in aligned]) for k in aligned[0]}
            order = ops.reading_order(boxes)
            query, box = gather_aligned(al["peak"], order, query_boxes_xyxy(boxes, src_hw), hit[:, 0])
        else:
            i32 = lambda: torch.empty((0, Lmax), dtype=torch.int32, device=dev)                         # noqa: E731
            al = dict(peak=i32(), first=i32(), last=i32(), prob=torch.empty((0, Lmax), dtype=torch.float32, device=dev),
                      score=torch.empty((0,), dtype=torch.float64, device=dev))
            query, box = i32(), torch.empty((0, Lmax, 4), dtype=torch.float32, device=dev)
        out.update(hit=hit, query=query, rank=al["peak"], first=al["first"], last=al["last"], score=al["prob"], box=box, logp=al["score"])
    return out


def spot_keywords(outputs, keywords: Sequence[Sequence[int]], min_conf: float = 0.5, max_hits: int = 4, eps: float = 0.003,
                  src_hw=None) -> List[List[KeywordHit]]:
    """spot_records(with_chars=True) as KeywordHits, one list per line, in (keyword, best hit first) order."""
    rec = spot_records(outputs, keywords, min_conf, max_hits, eps, src_hw, with_chars=True)
    host = {k: v.cpu().tolist() for k, v in rec.items()}
    lines: List[List[KeywordHit]] = [[] for _ in range(outputs["pred_logits"].shape[0])]
    for k, (b, q, h) in enumerate(host["hit"]):
        z = [int(v) for v in keywords[q]]
        chars = aligned_chars(z, *(host[key][k] for key in ("query", "rank", "first", "last", "score", "box")), len(z))
        lines[b].append(KeywordHit(q, b, host["start"][b][q][h], host["end"][b][q][h], host["ratio"][b][q][h], host["conf"][b][q][h],
                                   union_box([c.box for c in chars]), chars))
    return lines


def keyword_hit_to_json(hit: KeywordHit, charset: Sequence, line_id: str, regex: Optional[str] = None) -> Dict:
    """The object `--spot-out` writes for one hit: the line's id, the word, its confidence and ratio, the first and the last rank
    (frame in reading order) it covers, its box and its characters (each as in `--align-out`).  A hit of an expression
    (hit.pattern is set) also carries "pattern" and, when handed in, the expression's text as "regex"; a word hit's object has
    neither."""
    cs = list(charset)
    obj = {"id": line_id, "word": "".join(str(cs[c.label]) for c in hit.chars), "keyword": hit.keyword, "line": hit.line,
           "conf": hit.conf, "ratio": hit.ratio, "start": hit.start, "end": hit.end, "box": list(hit.box),
           "chars": [{"c": str(cs[c.label]), "label": c.label, "score": c.score, "box": list(c.box), "query": c.query, "rank": c.rank,
                      "first": c.first, "last": c.last} for c in hit.chars]}
    if hit.pattern is not None:
        obj["pattern"] = hit.pattern
        if regex is not None:
            obj["regex"] = regex
    return obj


def keyword_hit_from_json(obj: Dict) -> KeywordHit:
    """the KeywordHit a `--spot-out` object was written from"""
    chars = [LocatedChar(c["label"], c["score"], tuple(c["box"]), c["query"], c["rank"], c["first"], c["last"]) for c in obj["chars"]]
    return KeywordHit(obj["keyword"], obj["line"], obj["start"], obj["end"], obj["ratio"], obj["conf"], tuple(obj["box"]), chars,
                      obj.get("pattern"))


# ------------------------------------------------------------------- regular expressions over the lattice
@dataclasses.dataclass
class PatternRead:
    """The best string of an expression's language over a line or span: `labels` = its label indices (None when no string of the
    language fits the frames), `logp` = ln p of its best path (-inf then), `conf` = exp((logp - base) / max(len, 1)): the geometric
    mean per character of the likelihood ratio against the frame-wise argmax path, in (0, 1] (0 when nothing fits)."""
    labels: Optional[List[int]]
    logp: float
    conf: float


def _automaton(pattern, charset):
    from . import pattern as P
    return pattern if isinstance(pattern, P.Automaton) else P.compile_pattern(pattern, charset)


@torch.no_grad()
def decode_pattern(outputs, pattern, charset: Sequence[str], eps: float = 0.003, spans=None, bonus: float = 0.0) -> List[PatternRead]:
    """The best string of an expression's language for every line of the batch, or for every span (line, first rank, one past the
    last) when `spans` is given (dtlr_pattern_decode over the emissions of dtlr_blank_emissions, chunked under ALIGN_EMISSION_BYTES).
    pattern: the expression's text in the dialect of dtlr_amd/pattern.py, compiled against `charset`, or a compiled Automaton.  bonus:
    what every character adds to the key candidates are compared by (logp is without it)."""
    import math
    from . import ops
    from . import pattern as P
    logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
    B, nq, C = logits.shape
    sp = [(b, 0, nq) for b in range(B)] if spans is None else [(int(b), int(lo), int(hi)) for b, lo, hi in spans]
    if any(not (0 <= b < B and 0 <= lo <= hi <= nq) for b, lo, hi in sp):
        raise ValueError(f"decode_pattern: a span outside the batch of {B} lines of {nq} queries")
    tables = P.pattern_upload(_automaton(pattern, charset), C + 1, logits.device)
    chunk = max(1, ALIGN_EMISSION_BYTES // (nq * (C + 1) * 4))
    out: List[Optional[PatternRead]] = [None] * len(sp)
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        mine = [k for k, (b, _, _) in enumerate(sp) if b0 <= b < b1]
        if not mine:
            continue
        em = ops.blank_emissions(logits[b0:b1], boxes[b0:b1], eps)
        rec = {k: v.cpu().tolist() for k, v in ops.pattern_decode(em, [(sp[k][0] - b0, sp[k][1], sp[k][2]) for k in mine], tables, bonus).items()}
        del em
        for i, k in enumerate(mine):
            n = rec["length"][i]
            if n < 0:
                out[k] = PatternRead(None, float("-inf"), 0.0)
            else:
                out[k] = PatternRead([c - 1 for c in rec["labels"][i][:n]], rec["score"][i], math.exp((rec["score"][i] - rec["base"][i]) / max(n, 1)))
    return out


@torch.no_grad()
def spot_patterns(outputs, patterns: Sequence, charset: Sequence[str], min_conf: float = 0.5, max_hits: int = 4,
                  bonus: Optional[float] = None, eps: float = 0.003, src_hw=None) -> List[List[KeywordHit]]:
    """Every occurrence of every expression in every line of the batch, one list of KeywordHits per line in (expression, best hit
    first) order (dtlr_pattern_search over the emissions of dtlr_blank_emissions).  patterns: texts in the dialect of
    dtlr_amd/pattern.py, compiled against `charset`, or compiled Automata; one that accepts the empty string raises ValueError.  A hit
    needs conf = exp(ratio / characters) >= min_conf.  bonus: what every character adds to the key hits grow and are ranked by; None =
    -ln(min_conf), 0 when min_conf is 0: a hit then grows over a character exactly when that character alone clears the bar.  A
    hit's string is dtlr_pattern_decode's over its frames [start, end + 1) with the same bonus; its characters and boxes come from
    dtlr_ctc_align of that string over the same frames of the plain lattice, as spot_records(with_chars=True) takes a word's.  In a
    hit, `keyword` and `pattern` both hold the expression's index."""
    import math
    from . import ops
    from . import pattern as P
    logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
    B, nq, C = logits.shape
    if not 0.0 <= float(min_conf) <= 1.0:
        raise ValueError(f"spot: min_conf {min_conf} outside 0..1")
    if not 1 <= int(max_hits) <= 16:
        raise ValueError(f"spot: max_hits {max_hits} outside 1..16")
    bonus = P.default_bonus(float(min_conf)) if bonus is None else float(bonus)
    tables = [P.pattern_upload(_automaton(p, charset), C + 1, logits.device) for p in patterns]
    for tb in tables:
        if tb["accepts_empty"]:
            raise ValueError(f"spot: the pattern {tb['regex']!r} accepts the empty string: it is found everywhere")
    lines: List[List[KeywordHit]] = [[] for _ in range(B)]
    if not tables or B == 0:
        return lines
    order = ops.reading_order(boxes)
    allbox = query_boxes_xyxy(boxes, src_hw)
    chunk = max(1, ALIGN_EMISSION_BYTES // (nq * (C + 1) * 4))
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        em = ops.blank_emissions(logits[b0:b1], boxes[b0:b1], eps)
        for p, tb in enumerate(tables):
            rec = {k: v.cpu().tolist() for k, v in ops.pattern_search(em, tb, min_conf, max_hits, bonus).items()}
            idx = [(b, h) for b in range(b1 - b0) for h in range(rec["count"][b])]
            if not idx:
                continue
            spans = [(b, rec["start"][b][h], rec["end"][b][h] + 1) for b, h in idx]
            dec = ops.pattern_decode(em, spans, tb, bonus)
            lens = dec["length"].cpu().clamp(min=0)
            Lmax = max(int(lens.max()), 1)
            al = ops.ctc_align(em, spans, dec["labels"][:, :Lmax].clamp(min=1).long().cpu(), lens, False)
            line = torch.tensor([b0 + b for b, _ in idx], dtype=torch.int64)
            query, box = gather_aligned(al["peak"], order, allbox, line)
            host = {k: v.cpu().tolist() for k, v in dict(labels=dec["labels"], query=query, rank=al["peak"], first=al["first"],
                                                         last=al["last"], score=al["prob"], box=box).items()}
            for k, (b, h) in enumerate(idx):
                n = int(lens[k])
                z = [c - 1 for c in host["labels"][k][:n]]
                chars = aligned_chars(z, *(host[key][k] for key in ("query", "rank", "first", "last", "score", "box")), n)
                ratio = rec["ratio"][b][h]
                lines[b0 + b].append(KeywordHit(p, b0 + b, rec["start"][b][h], rec["end"][b][h], ratio,
                                                math.exp(ratio / max(rec["nchar"][b][h], 1)), union_box([c.box for c in chars]), chars, p))
        del em
    return lines


def labels_to_string(labels: Sequence[int], charset: Sequence[str]) -> str:
    return "".join(charset[int(i)] for i in labels)


# ----------------------------------------------------------------------------------- metrics (host)
def levenshtein(s1, s2) -> int:
    """== editdistance.eval (evaluation.py:519,524); row-by-row DP."""
    if len(s1) < len(s2):
        s1, s2 = s2, s1
    if len(s2) == 0:
        return len(s1)
    prev = list(range(len(s2) + 1))
    for i, c1 in enumerate(s1):
        cur = [i + 1] + [0] * len(s2)
        for j, c2 in enumerate(s2):
            a, b, c = prev[j + 1] + 1, cur[j] + 1, prev[j] + (c1 != c2)
            cur[j + 1] = a if a < b and a < c else (b if b < c else c)
        prev = cur
    return prev[-1]


def character_error_rate(pred, gt) -> float:
    """engine.py:594-633: distance / max(len(gt),1); 1 if either side is empty."""
    if len(gt) == 0 or len(pred) == 0:
        return 1
    return levenshtein(pred, gt) / max(len(gt), 1)


def process_pred_string(s: str) -> str:
    """evaluation.py:430-450 (string normalisation before CER on IAM/RIMES/READ)."""
    for a, b in (("B B C", "BBC"), ("I T V", "ITV"), ("  ", " "), (" -", "-"), ("- ", "-"), (" .", "."), (" ,", ",")):
        s = s.replace(a, b)
    s = re.sub(r"(\d), (\d)", r"\1,\2", s)
    s = s.replace(" '", "'").replace("' ", "'")
    s = re.sub(r"(?<=\S)€(?=\S)", " € ", s)
    s = re.sub(r"(?<!\.)\.\.(?!\.)", ".", s)
    return s.replace(",,", ",")


def cumulative_cer(gt_strings: Sequence[str], pred_strings: Sequence[str], normalise: bool = True):
    """evaluation.py:517-529,547,653-656: running sum(dist)/sum(len); the reported number is the mean
    of that running series (reference quirk kept).  Returns (reported, series)."""
    dist, length, series = 0, 0, []
    for g, p in zip(gt_strings, pred_strings):
        if normalise:
            g, p = process_pred_string(g), process_pred_string(p)
        dist += levenshtein(g, p)
        length += len(g)
        series.append(dist / length)
    return (sum(series) / len(series) if series else 0.0), series


def word_error_rate(predicted_words, gt_words) -> float:
    """evaluation.py:358-396: word-level edit distance / max(#gt words, 1).  The reference's loop passes (gt_split, pred_split)
    (evaluation.py:533-535, 546-549), so the figure it reports is normalised by the number of PREDICTED words; the harness
    here calls it the same way."""
    return levenshtein(predicted_words, gt_words) / max(len(gt_words), 1)


def split_labels_into_words(labels: Sequence[int], charset: Sequence[str]) -> List[List[int]]:
    """evaluation.py:400-412: cut a label sequence at the charset's space; no empty words."""
    space = list(charset).index(" ")
    words: List[List[int]] = [[]]
    for lab in labels:
        if lab == space:
            if words[-1]:
                words.append([])
        else:
            words[-1].append(lab)
    return words if words[-1] else words[:-1]


_GT_RULES = (("B B C", "BBC"), ("I T V", "ITV"), (" -", "-"), ("- ", "-"), (" -", "-"), ("- ", "-"), (" .", "."), (" ,", ","),
             (" '", "'"), ("' ", "'"))


def process_gt_string(s: str) -> str:
    """evaluation.py:414-428 (ground-truth normalisation; unlike process_pred_string it does not collapse double blanks or
    repeated punctuation)."""
    for a, b in _GT_RULES:
        s = s.replace(a, b)
    s = re.sub(r"(\d), (\d)", r"\1,\2", s)
    return re.sub(r"(?<=\S)€(?=\S)", " € ", s)


def character_error_rate_with_impact(pred: Sequence[int], gt: Sequence[int], impact: Dict[int, int]):
    """evaluation.py:162-210 -> (cer, impact, div).  `impact[c]` grows, for every predicted character c, by the number of
    ground-truth characters that differ from it (what the reference's bookkeeping inside its DP loop amounts to); written to
    dict_char.json by the harness.  An empty ground truth raises (the reference fails on it too)."""
    if len(gt) == 0:
        raise ValueError("character_error_rate_with_impact: empty ground truth")
    counts: Dict[int, int] = {}
    for g_ in gt:
        counts[int(g_)] = counts.get(int(g_), 0) + 1
    for p_ in pred:
        n = len(gt) - counts.get(int(p_), 0)
        if n:
            impact[int(p_)] = impact.get(int(p_), 0) + n
    return levenshtein(pred, gt) / len(gt), impact, len(gt)


def character_impact(pred: Sequence[int], gt: Sequence[int], impact: Dict[int, int]) -> Dict[int, int]:
    """the `impact` bookkeeping of character_error_rate_with_impact alone, for a caller that has the distance already"""
    counts: Dict[int, int] = {}
    for g_ in gt:
        counts[int(g_)] = counts.get(int(g_), 0) + 1
    for p_ in pred:
        n = len(gt) - counts.get(int(p_), 0)
        if n:
            impact[int(p_)] = impact.get(int(p_), 0) + n
    return impact


def compute_wa(gt: Sequence[int], pred: Sequence[int]) -> float:
    """evaluation.py:212-238 (cipher "word accuracy"): matching positions over max(len(gt), 1)."""
    return sum(1 for a, b in zip(gt, pred) if a == b) / max(len(gt), 1)


def compute_edit_operations(s1: Sequence, s2: Sequence) -> Tuple[int, int, int]:
    """evaluation.py:239-281 -> (insertions, deletions, substitutions) of the alignment the reference's backtrace picks
    (substitution before deletion before insertion)."""
    m, n = len(s1), len(s2)
    rows = [list(range(n + 1))]
    for i in range(1, m + 1):
        prev, cur = rows[-1], [i] + [0] * n
        for j in range(1, n + 1):
            cur[j] = prev[j - 1] if s1[i - 1] == s2[j - 1] else 1 + min(prev[j], cur[j - 1], prev[j - 1])
        rows.append(cur)
    i, j, ins, dele, sub = m, n, 0, 0, 0
    while i and j:
        here = rows[i][j]
        if s1[i - 1] == s2[j - 1]:
            i, j = i - 1, j - 1
        elif here == rows[i - 1][j - 1] + 1:
            sub, i, j = sub + 1, i - 1, j - 1
        elif here == rows[i - 1][j] + 1:
            dele, i = dele + 1, i - 1
        else:
            ins, j = ins + 1, j - 1
    return ins + j, dele + i, sub


def compute_cr(gt: Sequence[int], pred: Sequence[int]) -> float:
    """evaluation.py:283-290 (Chinese correct rate): (len(gt) - deletions - substitutions) / len(gt)."""
    _, dele, sub = compute_edit_operations(gt, pred)
    return (len(gt) - dele - sub) / len(gt)


# ----------------------------------------------------------------------- edit distance and alignment on the device
def compute_edit_alignment(s1: Sequence, s2: Sequence) -> List[Tuple[int, int]]:
    """The alignment compute_edit_operations counts, step by step in forward order: (i, j) = s1[i] stands against s2[j] (a match when
    they are equal, a substitution otherwise), (i, -1) = s1[i] is deleted, (-1, j) = s2[j] is inserted.  The host statement of what
    dtlr_edit_align writes as `ops`."""
    m, n = len(s1), len(s2)
    rows = [list(range(n + 1))]
    for i in range(1, m + 1):
        prev, cur = rows[-1], [i] + [0] * n
        for j in range(1, n + 1):
            cur[j] = prev[j - 1] if s1[i - 1] == s2[j - 1] else 1 + min(prev[j], cur[j - 1], prev[j - 1])
        rows.append(cur)
    i, j, steps = m, n, []
    while i and j:
        here = rows[i][j]
        if s1[i - 1] == s2[j - 1] or here == rows[i - 1][j - 1] + 1:
            steps.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        elif here == rows[i - 1][j] + 1:
            steps.append((i - 1, -1))
            i -= 1
        else:
            steps.append((-1, j - 1))
            j -= 1
    return [(-1, k) for k in range(j)] + [(k, -1) for k in range(i)] + steps[::-1]


def _device_pairs(a_seqs, b_seqs):
    """the pairs the device can score (both sides at most EDIT_MAX_LEN elements that are ints inside int32, or str): their indices"""
    from .metrics import EDIT_MAX_LEN

    def fits(s):
        if len(s) > EDIT_MAX_LEN:
            return False
        return isinstance(s, str) or all(isinstance(v, int) and -(1 << 31) <= v < (1 << 31) for v in s)

    return [k for k, (x, y) in enumerate(zip(a_seqs, b_seqs)) if fits(x) and fits(y)]


def edit_align_batch(a_seqs, b_seqs, device="cuda", want_ops: bool = False):
    """Every pair (a_seqs[p], b_seqs[p]) scored in one pass on `device` (ops.edit_align: the pairs of the whole call in as few launches as
    the workspace limit allows).  Sequences of ints or str (a str is packed as its code points).  -> (dist: list of int, counts: list
    of (ins, del, sub), alignments: per pair its list of (i, j) steps, or None without want_ops): levenshtein(a, b),
    compute_edit_operations(a, b) and compute_edit_alignment(a, b) of every pair.  A pair the device cannot take (a side above
    ops.EDIT_MAX_LEN, elements that are no int32) is scored by those host functions instead, not refused."""
    from . import ops
    a_seqs, b_seqs = list(a_seqs), list(b_seqs)
    if len(a_seqs) != len(b_seqs):
        raise ValueError(f"edit_align_batch: {len(a_seqs)} sequences against {len(b_seqs)}")
    n = len(a_seqs)
    dist, counts, aligns = [None] * n, [None] * n, [None] * n if want_ops else None
    on = _device_pairs(a_seqs, b_seqs)
    taken = set(on)
    for k in range(n):
        if k not in taken:
            dist[k] = levenshtein(a_seqs[k], b_seqs[k])
            counts[k] = compute_edit_operations(a_seqs[k], b_seqs[k])
            if want_ops:
                aligns[k] = compute_edit_alignment(a_seqs[k], b_seqs[k])
    if on:
        a, a_off, b, b_off = ops.edit_align_tables([a_seqs[k] for k in on], [b_seqs[k] for k in on])
        d, c, n_ops, steps = ops.edit_align(a.to(device), a_off, b.to(device), b_off, want_ops)
        d, c = d.cpu().tolist(), c.cpu().tolist()
        if want_ops:
            n_ops, steps, start = n_ops.cpu().tolist(), steps.cpu().numpy(), (a_off + b_off).tolist()
        for q, k in enumerate(on):
            dist[k], counts[k] = d[q], tuple(c[q])
            if want_ops:
                aligns[k] = [tuple(r) for r in steps[start[q]: start[q] + n_ops[q]].tolist()]
    return dist, counts, aligns


def edit_distances(a_seqs, b_seqs, device="cuda") -> List[int]:
    """levenshtein(a, b) of every pair, on the device (edit_align_batch)"""
    return edit_align_batch(a_seqs, b_seqs, device)[0]


def edit_operations(a_seqs, b_seqs, device="cuda") -> List[Tuple[int, int, int]]:
    """compute_edit_operations(a, b) = (insertions, deletions, substitutions) of every pair, on the device (edit_align_batch)"""
    return edit_align_batch(a_seqs, b_seqs, device)[1]


def edit_alignments(a_seqs, b_seqs, device="cuda") -> List[List[Tuple[int, int]]]:
    """compute_edit_alignment(a, b) of every pair, on the device (edit_align_batch)"""
    return edit_align_batch(a_seqs, b_seqs, device, True)[2]


class ConfusionReport:
    """Which characters a recogniser confuses, drops and invents: accumulated from alignments of (gt, pred) with a = gt, the way
    compute_cr calls compute_edit_operations.  sub[(g, p)]: g was read as p; dele[g]: g has no partner; ins[p]: p has no partner;
    n[g]: occurrences of g in the ground truth; correct[g]: those that stand against an equal character.  The keys are the sequences'
    elements (label indices in the harness)."""

    def __init__(self):
        self.sub: Dict[Tuple[int, int], int] = {}
        self.dele: Dict[int, int] = {}
        self.ins: Dict[int, int] = {}
        self.n: Dict[int, int] = {}
        self.correct: Dict[int, int] = {}
        self.lines = 0

    def add_counted(self, rows, lines: int = 0) -> "ConfusionReport":
        """rows of (g, p, count): a step of the alignments and how often it occurred; g None = an insertion of p, p None = a deletion of g"""
        for g, p, c in rows:
            c = int(c)
            if g is None:
                self.ins[int(p)] = self.ins.get(int(p), 0) + c
                continue
            g = int(g)
            self.n[g] = self.n.get(g, 0) + c
            if p is None:
                self.dele[g] = self.dele.get(g, 0) + c
            elif int(p) == g:
                self.correct[g] = self.correct.get(g, 0) + c
            else:
                self.sub[(g, int(p))] = self.sub.get((g, int(p)), 0) + c
        self.lines += int(lines)
        return self

    def add_alignment(self, gt: Sequence[int], pred: Sequence[int], steps: Sequence[Tuple[int, int]]) -> "ConfusionReport":
        """one line's alignment (compute_edit_alignment(gt, pred), or edit_alignments's) on the host"""
        return self.add_counted(((None if i < 0 else gt[i], None if j < 0 else pred[j], 1) for i, j in steps), 1)

    def add_device(self, a, a_off, b, b_off, n_ops, ops) -> "ConfusionReport":
        """The alignments of a whole ops.edit_align call (a = the ground truths; a_off, b_off the HOST offsets, everything else on the
        device): the gather through `ops` and the counting run on the device, only the counted table of distinct (g, p) comes back."""
        dev = a.device
        ao, bo = a_off.to(dev), b_off.to(dev)
        start = ao[:-1] + bo[:-1]                                                  # first slot of every pair
        S = int(a_off[-1]) + int(b_off[-1])
        n = int(n_ops.numel())
        if S and n:
            slot = torch.arange(S, device=dev)
            pair = (torch.searchsorted(start.contiguous(), slot, right=True) - 1).clamp(min=0)
            # equal starts (pairs without slots) resolve to the last of them: only a pair that owns slots is ever looked at
            keep = (slot - start[pair]) < n_ops[pair].long()
            pair, st = pair[keep], ops[keep].long()
            none = -(1 << 40)                                                      # no int32: the partner of an insertion / a deletion
            ax = torch.cat([a.long(), torch.full((1,), none, dtype=torch.int64, device=dev)])      # [-1] = none
            bx = torch.cat([b.long(), torch.full((1,), none, dtype=torch.int64, device=dev)])
            g = ax[torch.where(st[:, 0] >= 0, ao[pair] + st[:, 0], -1)]
            p = bx[torch.where(st[:, 1] >= 0, bo[pair] + st[:, 1], -1)]
            keys, cnt = torch.unique(torch.stack([g, p], dim=1), dim=0, return_counts=True)
            table = torch.cat([keys, cnt[:, None]], dim=1).cpu().tolist()
            self.add_counted((None if g_ == none else g_, None if p_ == none else p_, c) for g_, p_, c in table)
        self.lines += n
        return self

    def recall(self, g: int) -> float:
        return self.correct.get(g, 0) / self.n[g]

    def totals(self) -> Dict[str, int]:
        """ins / del / sub: the sums over the lines of compute_edit_operations(gt, pred); n: ground-truth characters; correct: n - del - sub"""
        return {"lines": self.lines, "n": sum(self.n.values()), "correct": sum(self.correct.values()), "ins": sum(self.ins.values()),
                "del": sum(self.dele.values()), "sub": sum(self.sub.values())}

    def __eq__(self, other):
        return isinstance(other, ConfusionReport) and all(getattr(self, k) == getattr(other, k) for k in ("sub", "dele", "ins", "n", "correct", "lines"))

    def to_json(self, charset: Optional[Sequence] = None, top: int = 50) -> Dict:
        """The object `--confusion-out` writes.  Every list is sorted by count descending, then by (gt, pred) label ascending, and cut to
        its first `top` entries; charset given: entries also carry the characters."""
        cs = list(charset) if charset is not None else None
        name = lambda v: {} if cs is None else {"c": str(cs[v])}                                         # noqa: E731

        def ranked(d):
            return sorted(d.items(), key=lambda kv: (-kv[1], kv[0]))[: int(top)]

        return {"totals": self.totals(),
                "substitutions": [{"gt": g, "pred": p, "count": c, **({} if cs is None else {"gt_c": str(cs[g]), "pred_c": str(cs[p])})}
                                  for (g, p), c in ranked(self.sub)],
                "deletions": [{"gt": g, "count": c, **name(g)} for g, c in ranked(self.dele)],
                "insertions": [{"pred": p, "count": c, **name(p)} for p, c in ranked(self.ins)],
                "characters": [{"gt": g, "n": c, "correct": self.correct.get(g, 0), "recall": self.recall(g), **name(g)}
                               for g, c in ranked(self.n)]}


_WER_PUNCT = re.compile(r"""([\[\]{}/\()"'&+*=<>?.;:,!\-—_€#%°])""")


def format_string_for_wer(s: str) -> List[str]:
    """engine.py:487-494: every punctuation mark is a word of its own; blanks and line breaks collapse."""
    s = _WER_PUNCT.sub(r" \1 ", s)
    return re.sub(r"[ \n]+", " ", s).strip().split(" ")


def compute_wer(pred_labels: Sequence[Sequence[int]], target_labels: Sequence[Sequence[int]], charset: Sequence,
                mode_chr: bool = True) -> Tuple[float, float]:
    """engine.py:543-593 on decoded label sequences (its duplicate=False path): (sum of per-line WER, sum of per-line CER),
    WER = word edit distance of the formatted strings / number of ground-truth words, '¬' removed."""
    wer = cer = 0.0
    for pred, tgt in zip(pred_labels, target_labels):
        tgt = [int(t) for t in tgt]
        cer += character_error_rate(list(pred), tgt)
        conv = (lambda c: c) if mode_chr else (lambda c: chr(int(c)))
        gt_words = format_string_for_wer("".join(conv(charset[t]) for t in tgt).replace("¬", ""))
        pr_words = format_string_for_wer("".join(conv(charset[int(p)]) for p in pred).replace("¬", ""))
        wer += levenshtein(gt_words, pr_words) / len(gt_words)
    return wer, cer


if __name__ == "__main__":
    from .eval_harness import main
    main()
