"""The evaluation loop of the reference's harness (evaluation.py:460-659) on the MI355X engine:

    python -m dtlr_amd.evaluation --config latin --weights checkpoint.pth --images DIR --labels labels.pkl --mode test \
           --dataset IAM --NMS 0.5 --TH 0.3                       # scripts/evaluating/IAM.sh
    python -m torch.distributed.run --nproc-per-node 8 -m dtlr_amd.evaluation ...      # data-parallel over the node

checkpoint + folder of line images + labels  ->  preprocess (device) -> forward -> decode -> CER / WER / AR / CR / WA, and the
reference's output files under <out>/<dataset>/: cer_list.npy, dict_char.json, list_preds.txt, list_gt.txt,
cer_TH_{TH}_NMS_{NM}.txt (the character-impact histogram PNG is visualisation and is not produced).

What differs from the reference loop, and why the numbers do not:
  * the reference forwards ONE image at a time (`model(image[None])`, evaluation.py:499).  Here lines whose resized size is
    identical are batched together WITHOUT padding (`--batching exact`, default): the per-line arithmetic is exactly the
    bs = 1 arithmetic, only the launch is shared.  `--batching padded` pads mixed sizes into one canvas (faster, but a padded
    line is not bit-identical to the same line alone: the backbone sees the canvas's zero padding instead of its own border);
    `--batching ragged` pads mixed sizes the same way but runs the forward per line (each line's result is its bs = 1 result up to
    rounding and the order of near-tied queries; DESIGN.md, per-line batching);
  * lines are sharded over the ranks of a torch.distributed job (contiguous shards of the size-sorted list), decoded records
    are all-gathered, rank 0 computes the metrics in dataset order -- the running CER series (the figure the reference reports
    is the MEAN of the running sum(dist)/sum(len) series, evaluation.py:521-529,547) is order dependent;
  * a line whose forward raises is skipped by the reference (evaluation.py:498-504: message, `continue`, the line enters no
    metric).  Same here: a failing batch is retried line by line, a line that still fails (or whose image file cannot be read)
    is reported on stderr and left out of every list -- one bad image does not end a 2915-line run, and does not take its
    batch neighbours with it;
  * every rank reads only the image HEADERS of the whole set (sizes, for the batch plan) and decodes only the lines of its own
    shard -- not N copies of the dataset in host memory.
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dist as ddist
from . import evaluation as E
from .config import DTLRConfig
from .transforms import EVAL_MAX_SIZE, EVAL_SIZE, EvalTransform, get_size_with_aspect_ratio

HERE = os.path.dirname(os.path.abspath(__file__))
CER_DATASETS = ("IAM", "RIMES", "READ")          # evaluation.py:510,521: string-level cumulative CER + WER


def load_charset(path: Optional[str]) -> List:
    """A JSON list (datasets/default_charset.json layout) or a pickle of a list (data/HWDB_v1/charset_full.pkl layout)."""
    path = path or os.path.join(HERE, "data", "default_charset.json")
    if path.endswith(".json"):
        with open(path, encoding="utf-8") as f:
            return list(json.load(f))
    with open(path, "rb") as f:
        return list(pickle.load(f))


def load_labels(path: str, mode: str) -> List[Tuple[str, str]]:
    """-> [(image id / file name, text)] in dataset order.  Accepts the reference's labels.pkl ({"ground_truth": {split: [{"id",
    "text"}, ...]}}, datasets/IAM.py:57-60,77-80; mode "val" means "valid"), a JSON object {name: text} or list of [name, text],
    or a TSV file `name<TAB>text`."""
    if path.endswith(".pkl"):
        with open(path, "rb") as f:
            data = pickle.load(f)             # the reference's own pickle of plain dicts/lists/strings
        split = "valid" if mode == "val" else mode
        return [(str(ex["id"]), ex["text"]) for ex in data["ground_truth"][split]]
    if path.endswith(".json"):
        with open(path, encoding="utf-8") as f:
            data = json.load(f)
        return [(str(k), v) for k, v in (data.items() if isinstance(data, dict) else data)]
    rows = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\n")
            if line:
                name, _, text = line.partition("\t")
                rows.append((name, text))
    return rows


def find_image(folder: str, name: str) -> str:
    for cand in (name, name + ".jpg", name + ".png", name + ".jpeg"):
        p = os.path.join(folder, cand)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"{name}[.jpg|.png] not found under {folder}")


def read_rgb(path: str) -> np.ndarray:
    from PIL import Image                     # decoding the image FILE is host I/O; resize / normalise run on the device
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))  # datasets/IAM.py:87-89


def plan_batches(sizes: Sequence[Tuple[int, int]], batch: int, exact: bool, size: int, max_size: int) -> List[List[int]]:
    """Index batches.  exact: only lines with the same resized (h, w) share a batch (no padding); padded: neighbours in the
    width-sorted order share a batch."""
    resized = [get_size_with_aspect_ratio((w, h), size, max_size) for (h, w) in sizes]
    order = sorted(range(len(sizes)), key=lambda i: (resized[i][1], resized[i][0], i))
    batches: List[List[int]] = []
    for i in order:
        if batches and len(batches[-1]) < batch and (not exact or resized[batches[-1][0]] == resized[i]):
            batches[-1].append(i)
        else:
            batches.append([i])
    return batches


def image_size(path: str) -> Tuple[int, int]:
    """(h, w) from the file header (no pixel decode)."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return int(h), int(w)


@torch.no_grad()
def predict_labels(model, images, batch: int = 32, exact: bool = True, TH: Optional[float] = None,
                   NM: Optional[float] = None, postprocessor=None, device="cuda", size: int = EVAL_SIZE,
                   max_size: int = EVAL_MAX_SIZE, rank: int = 0, world: int = 1, sizes: Optional[Sequence[Tuple[int, int]]] = None,
                   skip_errors: bool = True, per_line: bool = False, ngram: Optional[Dict] = None,
                   spot: Optional[Dict] = None) -> List[Optional[List[int]]]:
    """convert_output_to_pred (evaluation.py:94-158) for a list of RGB uint8 images -> one label list per image, dataset
    order.  TH / NM given: the NMS decoder; otherwise the blank/argmax decoder with eps = 0.03 / C.
    `images`: a sequence of [h, w, 3] uint8 arrays, or (with `sizes` = the (h, w) of every line) a callable i -> array that is
    invoked only for the lines of this rank's shard.  skip_errors (the reference's behaviour, evaluation.py:498-504): a line whose
    load / forward / decode raises is reported and returned as None; KeyboardInterrupt always propagates.
    per_line (`--batching ragged`): mixed sizes share a padded batch as with exact=False, and the forward runs per line
    (DINO.forward(per_line=True)): every line gets the result it gets alone.
    ngram (`--ngram-arpa`): the bundle of ngram_bundle(); the batch's lines are then re-scored by the device n-gram beam decoder
    (ngram.rescored_labels_batch: one launch over every word span of the batch) instead of decoded by the blank / NMS decoder.
    A bundle of word_beam_bundle() (`--word-beam-lexicon`) sends the batch's whole lines to the device word beam search instead
    (ngram.word_beam_labels_batch).
    spot (`--spot-words`): the bundle of spot_bundle(); every batch's output is also searched for its keywords (spot_batch)."""
    lazy = callable(images)
    if lazy and sizes is None:
        raise ValueError("predict_labels: a loader callable needs `sizes`")
    sizes = list(sizes) if sizes is not None else [im.shape[:2] for im in images]
    n = len(sizes)
    load = images if lazy else (lambda i: images[i])
    batches = plan_batches(sizes, batch, exact and not per_line, size, max_size)
    lo, hi = ddist.shard_bounds(len(batches), rank, world)
    tf = EvalTransform(size, max_size)
    nq = model.num_queries
    rec = torch.full((n, nq + 2), -1, dtype=torch.int32)          # labels[nq] | length | status (-1 not mine, 0 decoded, 1 skipped)

    def run(idx):
        samples = tf([load(i) for i in idx], device=device)
        out = model(samples, per_line=True) if per_line else model(samples)
        if spot is not None:
            spot_batch(spot, out, samples, idx)
        if ngram is not None:
            from . import ngram as NG
            preds = NG.word_beam_labels_batch(out, ngram) if ngram.get("word_beam") else NG.rescored_labels_batch(out, ngram)
        else:
            preds = E.decode_nms(out, postprocessor, TH, NM) if (TH is not None and NM is not None) else E.decode_blank(out)
        for i, p in zip(idx, preds):
            rec[i, : len(p)] = torch.tensor(p, dtype=torch.int32)
            rec[i, nq], rec[i, nq + 1] = len(p), 0

    for b in batches[lo:hi]:
        try:
            run(b)
        except KeyboardInterrupt:
            raise
        except Exception as e:
            if not skip_errors:
                raise
            for i in b:                                          # retry alone: only the offending line is lost
                try:
                    run([i])
                except KeyboardInterrupt:
                    raise
                except Exception as e1:
                    print(f"An error occurred affecting the metrics computation (line {i}: {type(e1).__name__}: {e1})", file=sys.stderr)
                    rec[i, :nq] = -1
                    rec[i, nq], rec[i, nq + 1] = 0, 1
                    if spot is not None:
                        spot["hits"].pop(i, None)
            del e
    if world > 1:                               # every line is owned by exactly one rank: element-wise max merges the shards
        import torch.distributed as dist
        t = rec.to(device) if dist.get_backend() == "nccl" else rec
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        rec = t.cpu()
    return [None if int(rec[i, nq + 1]) == 1 else rec[i, : int(rec[i, nq])].tolist() for i in range(n)]


# ------------------------------------------------------------------------------------------ located transcripts
# One located line as ONE int32 row, floats as their bit patterns:
#   [n chars | n words | n word labels | labels K | query K | rank K | score K | box 4K]
#   and, for the n-gram decoder, [words K x 10 = (first char, end char, source, same, score, box x 4, n labels) | word labels 2K]
# A rank fills the rows of other ranks' lines with ZEROS and the shards are merged with all_reduce(SUM): exactly one rank owns a line
# and adding zeros is exact for every bit pattern (the -1 fill + MAX merge of predict_labels is not: a negative coordinate, or
# -0.0, is a large negative int32).  The status column travels apart, with predict_labels's -1 fill and MAX.
#   and, with aligned words (align_rewritten), [per word: 0 = none, else 1 + its aligned characters, K | aligned characters 2K x 10 =
#   (label, query, rank, first, last, score, box x 4)]
# A line of the forced alignment (decoder "align") is the first form plus [first K | last K | logp as the two halves of its fp64 |
# feasible]; its transcript is the caller's and does not travel.
_LOC_HEAD = 3
_LOC_WORD = 10                 # first char, end char (-1, -1: no characters), source (1 = ngram), same, score, box x 4, n labels
_LOC_ALIGNED = 10              # label, query, rank, first, last, score, box x 4


def located_row_width(K: int, with_words: bool, with_aligned: bool = False) -> int:
    return _LOC_HEAD + 8 * K + ((_LOC_WORD + 2) * K if with_words else 0) + ((1 + 2 * _LOC_ALIGNED) * K if with_aligned else 0)


def aligned_row_width(K: int) -> int:
    return located_row_width(K, False) + 2 * K + 3


def _f2i(values) -> np.ndarray:
    return np.asarray(values, dtype=np.float32).reshape(-1).view(np.int32)


def _i2f(values) -> np.ndarray:
    return np.ascontiguousarray(values, dtype=np.int32).view(np.float32)


def _pack_aligned_char(c: "E.LocatedChar") -> np.ndarray:
    ints = np.array([c.label, c.query, -1 if c.rank is None else c.rank, -1 if c.first is None else c.first,
                     -1 if c.last is None else c.last], dtype=np.int32)
    return np.concatenate([ints, _f2i([c.score]), _f2i(c.box)])


def _unpack_aligned_char(v) -> "E.LocatedChar":
    opt = lambda x: None if x < 0 else int(x)                              # noqa: E731
    return E.LocatedChar(int(v[0]), float(_i2f(v[5:6])[0]), tuple(_i2f(v[6:10]).tolist()), int(v[1]), opt(v[2]), opt(v[3]), opt(v[4]))


def pack_located(line: "E.LocatedLine", K: int, with_words: bool, with_aligned: bool = False) -> np.ndarray:
    """LocatedLine -> int32 row of located_row_width(K, with_words, with_aligned).  Without the word table the words are rebuilt from
    the characters on the other side (unpack_located(space_label=...))."""
    row = np.zeros(located_row_width(K, with_words, with_aligned), dtype=np.int32)
    n = len(line.chars)
    if n > K:
        raise ValueError(f"pack_located: {n} characters for {K} slots")
    row[0] = n
    o = _LOC_HEAD
    row[o: o + n] = [c.label for c in line.chars]
    row[o + K: o + K + n] = [c.query for c in line.chars]
    row[o + 2 * K: o + 2 * K + n] = [-1 if c.rank is None else c.rank for c in line.chars]
    row[o + 3 * K: o + 3 * K + n] = _f2i([c.score for c in line.chars])
    row[o + 4 * K: o + 4 * K + 4 * n] = _f2i([c.box for c in line.chars])
    if with_words:
        wl = [v for w in line.words for v in w.labels]
        if len(line.words) > K or len(wl) > 2 * K:
            raise ValueError(f"pack_located: {len(line.words)} words / {len(wl)} word labels for {K} slots")
        row[1], row[2] = len(line.words), len(wl)
        o = _LOC_HEAD + 8 * K
        for k, w in enumerate(line.words):
            c0, c1 = w.chars if w.chars is not None else (-1, -1)
            row[o + _LOC_WORD * k: o + _LOC_WORD * (k + 1)] = np.concatenate(
                [np.array([c0, c1, int(w.source == "ngram"), int(w.same)], dtype=np.int32), _f2i([w.score]), _f2i(w.box),
                 np.array([len(w.labels)], dtype=np.int32)])
        row[o + _LOC_WORD * K: o + _LOC_WORD * K + len(wl)] = wl
        if with_aligned:
            o = located_row_width(K, True)
            at = o + K
            if sum(len(w.aligned or ()) for w in line.words) > 2 * K:
                raise ValueError(f"pack_located: more than {2 * K} aligned characters")
            for k, w in enumerate(line.words):
                if w.aligned is not None:
                    row[o + k] = 1 + len(w.aligned)
                    for c in w.aligned:
                        row[at: at + _LOC_ALIGNED] = _pack_aligned_char(c)
                        at += _LOC_ALIGNED
    return row


def pack_aligned(line: "E.LocatedLine", K: int) -> np.ndarray:
    """A line of the forced alignment -> int32 row of aligned_row_width(K)"""
    row = np.zeros(aligned_row_width(K), dtype=np.int32)
    o = located_row_width(K, False)
    row[:o] = pack_located(line, K, False)
    n = len(line.chars)
    row[o: o + n] = [c.first for c in line.chars]
    row[o + K: o + K + n] = [c.last for c in line.chars]
    feasible = line.logp is not None and line.logp > float("-inf")
    row[o + 2 * K: o + 2 * K + 2] = np.array([line.logp if feasible else 0.0], dtype=np.float64).view(np.int32)
    row[o + 2 * K + 2] = int(feasible)
    return row


def unpack_aligned(row, K: int, labels: Sequence[int], space_label: Optional[int] = None) -> "E.LocatedLine":
    """pack_aligned's row and the line's transcript -> the LocatedLine of E.align_ctc"""
    row = np.asarray(row, dtype=np.int32)
    o = located_row_width(K, False)
    base = unpack_located(row[:o], K, False, "align", space_label)
    for i, c in enumerate(base.chars):
        c.first, c.last = int(row[o + i]), int(row[o + K + i])
    logp = float(np.ascontiguousarray(row[o + 2 * K: o + 2 * K + 2]).view(np.float64)[0]) if row[o + 2 * K + 2] else float("-inf")
    return E.LocatedLine([int(v) for v in labels], base.chars, E.located_words(base.chars, space_label), "align", logp)


def unpack_located(row, K: int, with_words: bool, decoder: str, space_label: Optional[int] = None,
                   with_aligned: bool = False) -> "E.LocatedLine":
    row = np.asarray(row, dtype=np.int32)
    n, o = int(row[0]), _LOC_HEAD
    lab, qry, rk = row[o: o + n].tolist(), row[o + K: o + K + n].tolist(), row[o + 2 * K: o + 2 * K + n].tolist()
    sc = _i2f(row[o + 3 * K: o + 3 * K + n]).tolist()
    bx = _i2f(row[o + 4 * K: o + 4 * K + 4 * n]).reshape(n, 4).tolist()
    chars = [E.LocatedChar(lab[i], sc[i], tuple(bx[i]), qry[i], None if rk[i] < 0 else rk[i]) for i in range(n)]
    if not with_words:
        return E.LocatedLine(lab, chars, E.located_words(chars, space_label), decoder)
    nw, o = int(row[1]), _LOC_HEAD + 8 * K
    words, at = [], o + _LOC_WORD * K
    for k in range(nw):
        w = row[o + _LOC_WORD * k: o + _LOC_WORD * (k + 1)]
        nl = int(w[9])
        words.append(E.LocatedWord(row[at: at + nl].tolist(), tuple(_i2f(w[5:9]).tolist()), float(_i2f(w[4:5])[0]),
                                   None if w[0] < 0 else (int(w[0]), int(w[1])), "ngram" if w[2] else "kept", bool(w[3])))
        at += nl
    if with_aligned:
        o = located_row_width(K, True)
        at = o + K
        for k, w in enumerate(words):
            if row[o + k]:
                w.aligned = [_unpack_aligned_char(row[at + _LOC_ALIGNED * i: at + _LOC_ALIGNED * (i + 1)]) for i in range(int(row[o + k]) - 1)]
                at += _LOC_ALIGNED * len(w.aligned)
    return E.LocatedLine([v for w in words for v in w.labels], chars, words, decoder)


def merge_located(rows: torch.Tensor, status: torch.Tensor, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge the shards of a torch.distributed job: `rows` [n, width] int32 (zeros in the rows of other ranks' lines) by SUM,
    `status` [n] int32 (-1 not mine, 0 decoded, 1 skipped) by MAX.  -> host tensors."""
    import torch.distributed as dist
    on = device if (device is not None and dist.get_backend() == "nccl") else None
    r, st = (rows.to(on), status.to(on)) if on is not None else (rows, status)
    dist.all_reduce(r, op=dist.ReduceOp.SUM)
    dist.all_reduce(st, op=dist.ReduceOp.MAX)
    return r.cpu(), st.cpu()


@torch.no_grad()
def predict_located(model, images, batch: int = 32, exact: bool = True, TH: Optional[float] = None, NM: Optional[float] = None,
                    device="cuda", size: int = EVAL_SIZE, max_size: int = EVAL_MAX_SIZE, rank: int = 0, world: int = 1,
                    sizes: Optional[Sequence[Tuple[int, int]]] = None, skip_errors: bool = True, per_line: bool = False,
                    ngram: Optional[Dict] = None, decoder: str = "blank", space_label: Optional[int] = None,
                    targets: Optional[Sequence[Optional[Sequence[int]]]] = None,
                    align_rewritten: bool = False, spot: Optional[Dict] = None) -> List[Optional["E.LocatedLine"]]:
    """predict_labels with every character located: one LocatedLine per image (None for a skipped line), dataset order, boxes in
    the SOURCE image's pixels.  decoder: "blank" (eps = 0.03 / C), "nms" (TH / NM, default 0.3 / 0.5) or "ngram" (`ngram` = the bundle
    of ngram_bundle(); words re-scored by the device beam, boxes at word level).  Batching (`exact`, padded, `per_line`), sharding and
    error handling are predict_labels's.  pred_boxes are normalised to each line's own extent, so the source (w, h) is the whole
    scale, for padded and ragged batches alike.  space_label: the charset's ' ' index (words are cut there), or None.
    decoder "align": the forced alignment of `targets` (per image its transcript as label indices; None: the line is skipped) against
    the model's output (E.align_ctc, eps = 0.003, loss_CTC's lattice).  align_rewritten (decoder "ngram"): words the beam rewrote
    carry their aligned characters.  spot: as in predict_labels (single process only)."""
    if decoder not in ("blank", "nms", "ngram", "align"):
        raise ValueError(f"predict_located: unknown decoder {decoder!r}")
    if decoder == "ngram" and ngram is None:
        raise ValueError("predict_located: decoder 'ngram' needs the `ngram` bundle")
    if decoder == "align" and targets is None:
        raise ValueError("predict_located: decoder 'align' needs `targets`")
    lazy = callable(images)
    if lazy and sizes is None:
        raise ValueError("predict_located: a loader callable needs `sizes`")
    sizes = list(sizes) if sizes is not None else [im.shape[:2] for im in images]
    n = len(sizes)
    load = images if lazy else (lambda i: images[i])
    batches = plan_batches(sizes, batch, exact and not per_line, size, max_size)
    lo, hi = ddist.shard_bounds(len(batches), rank, world)
    tf = EvalTransform(size, max_size)
    K, with_words = model.num_queries, decoder == "ngram"
    with_aligned = with_words and align_rewritten
    if decoder == "align":
        if len(targets) != n:
            raise ValueError(f"predict_located: {len(targets)} transcripts for {n} images")
        K = max([1] + [len(t) for t in targets if t is not None])
    rows = torch.zeros((n, aligned_row_width(K) if decoder == "align" else located_row_width(K, with_words, with_aligned)), dtype=torch.int32)
    status = torch.full((n,), -1, dtype=torch.int32)

    def run(idx):
        samples = tf([load(i) for i in idx], device=device)
        out = model(samples, per_line=True) if per_line else model(samples)
        hw = torch.tensor(samples.orig_sizes, dtype=torch.float32)
        if spot is not None:
            spot_batch(spot, out, samples, idx)
        if decoder == "align":
            if any(targets[i] is None for i in idx):
                raise ValueError("a transcript holds a character outside the charset")
            lines = E.align_ctc(out, [targets[i] for i in idx], 0.003, hw, True, space_label)
        elif decoder == "ngram":
            from . import ngram as NG
            lines = NG.rescored_located_batch(out, ngram, hw, space_label, align_rewritten)
        elif decoder == "nms":
            lines = E.decode_nms_located(out, 0.3 if TH is None else TH, 0.5 if NM is None else NM, hw, space_label)
        else:
            lines = E.decode_blank_located(out, None, hw, space_label)
        for i, line in zip(idx, lines):
            rows[i] = torch.from_numpy(pack_aligned(line, K) if decoder == "align" else pack_located(line, K, with_words, with_aligned))
            status[i] = 0

    for b in batches[lo:hi]:
        try:
            run(b)
        except KeyboardInterrupt:
            raise
        except Exception:
            if not skip_errors:
                raise
            for i in b:                                          # retry alone: only the offending line is lost
                try:
                    run([i])
                except KeyboardInterrupt:
                    raise
                except Exception as e1:
                    print(f"An error occurred affecting the metrics computation (line {i}: {type(e1).__name__}: {e1})", file=sys.stderr)
                    rows[i] = 0
                    status[i] = 1
                    if spot is not None:
                        spot["hits"].pop(i, None)
    if world > 1:
        rows, status = merge_located(rows, status, device)
    rows_np = rows.numpy()
    if decoder == "align":
        return [None if int(status[i]) == 1 else unpack_aligned(rows_np[i], K, targets[i], space_label) for i in range(n)]
    return [None if int(status[i]) == 1 else unpack_located(rows_np[i], K, with_words, decoder, space_label, with_aligned) for i in range(n)]


def write_layout(path: str, ids: Sequence[str], lines: Sequence[Optional["E.LocatedLine"]], charset: Sequence[str]) -> int:
    """`--layout-out`: one JSON object per located line image (a skipped line writes none), in dataset order.  -> lines written."""
    k = 0
    with open(path, "w", encoding="utf-8") as f:
        for line_id, line in zip(ids, lines):
            if line is None:
                continue
            f.write(json.dumps(E.located_line_to_json(line, charset, line_id), ensure_ascii=False) + "\n")
            k += 1
    return k


def write_aligned(path: str, ids: Sequence[str], lines: Sequence[Optional["E.LocatedLine"]], charset: Sequence[str]) -> int:
    """`--align-out`: one JSON object per aligned line image (a skipped line writes none), in dataset order.  -> lines written."""
    k = 0
    with open(path, "w", encoding="utf-8") as f:
        for line_id, line in zip(ids, lines):
            if line is None:
                continue
            f.write(json.dumps(E.aligned_line_to_json(line, charset, line_id), ensure_ascii=False) + "\n")
            k += 1
    return k


def spot_bundle(words: Sequence[str], charset: Sequence[str], min_conf: float = 0.5, max_hits: int = 4,
                patterns: Sequence[str] = (), bonus: Optional[float] = None) -> Dict:
    """What predict_labels / predict_located take as `spot`: the words that can be searched (1..32 characters, all in the charset) as
    label lists, and `hits`: image index -> its KeywordHits, filled batch by batch.  A word that cannot be searched is named on stderr
    and skipped.  patterns (`--spot-patterns`): expressions in the dialect of dtlr_amd/pattern.py, compiled here against the charset;
    one that does not compile, or that accepts the empty string, is named on stderr and skipped.  bonus (`--spot-length-bonus`): the
    expressions' length bonus, None = -ln(min_conf)."""
    if not 1 <= int(max_hits) <= 16:
        raise ValueError(f"--spot-max-hits {max_hits} outside 1..16")
    if not 0.0 <= float(min_conf) <= 1.0:
        raise ValueError(f"--spot-min-conf {min_conf} outside 0..1")
    kept, keywords = [], []
    for w, z in zip(words, transcript_labels(words, charset)):
        if z is None:
            print(f"--spot-words: {w!r} holds a character outside the charset: skipped", file=sys.stderr)
        elif not 1 <= len(z) <= 32:
            print(f"--spot-words: {w!r} has {len(z)} characters, the limits are 1..32: skipped", file=sys.stderr)
        else:
            kept.append(w)
            keywords.append(z)
    regexes, automata = [], []
    if patterns:
        from .pattern import compile_pattern
        for rx in patterns:
            try:
                auto = compile_pattern(rx, list(charset))
            except ValueError as e:
                print(f"--spot-patterns: {e}: skipped", file=sys.stderr)
                continue
            if auto.accepts_empty:
                print(f"--spot-patterns: pattern {rx!r} accepts the empty string: skipped", file=sys.stderr)
                continue
            regexes.append(rx)
            automata.append(auto)
    return dict(words=kept, keywords=keywords, min_conf=float(min_conf), max_hits=int(max_hits), hits={}, patterns=regexes,
                automata=automata, bonus=None if bonus is None else float(bonus), charset=list(charset))


def load_spot_patterns(path: str) -> List[str]:
    """`--spot-patterns`: one expression per line, UTF-8; empty lines are dropped, a repeated expression is searched once"""
    with open(path, encoding="utf-8") as f:
        lines = [ln.rstrip("\r\n") for ln in f]
    return list(dict.fromkeys(ln for ln in lines if ln))


def load_spot_words(path: str) -> List[str]:
    """`--spot-words`: one word per line, UTF-8; empty lines are dropped, a repeated word is searched once"""
    with open(path, encoding="utf-8") as f:
        words = [ln.rstrip("\r\n") for ln in f]
    return list(dict.fromkeys(w for w in words if w))


@torch.no_grad()
def spot_batch(spot: Dict, out, samples, idx: Sequence[int]) -> None:
    """search the batch's output for the bundle's keywords (E.spot_keywords, eps = 0.003, boxes in the source images' pixels) and
    then for its expressions (E.spot_patterns): a line's word hits come first"""
    if not spot["keywords"] and not spot.get("automata"):
        return
    hw = torch.tensor(samples.orig_sizes, dtype=torch.float32)
    if spot["keywords"]:
        for i, hits in zip(idx, E.spot_keywords(out, spot["keywords"], spot["min_conf"], spot["max_hits"], 0.003, hw)):
            spot["hits"][i] = hits
    if spot.get("automata"):
        found = E.spot_patterns(out, spot["automata"], spot["charset"], spot["min_conf"], spot["max_hits"], spot["bonus"], 0.003, hw)
        for i, hits in zip(idx, found):
            spot["hits"][i] = spot["hits"].get(i, []) + hits if spot["keywords"] else hits


def write_spotted(path: str, ids: Sequence[str], spot: Dict, charset: Sequence[str]) -> int:
    """`--spot-out`: one JSON object per hit, in dataset order, then the word list's (and after the words the expressions'), then
    best first.  -> hits written."""
    k = 0
    regexes = spot.get("patterns") or []
    with open(path, "w", encoding="utf-8") as f:
        for i, line_id in enumerate(ids):
            for hit in spot["hits"].get(i, ()):
                regex = regexes[hit.pattern] if hit.pattern is not None else None
                f.write(json.dumps(E.keyword_hit_to_json(hit, charset, line_id, regex), ensure_ascii=False) + "\n")
                k += 1
    return k


def transcript_labels(texts: Sequence[str], charset: Sequence[str]) -> List[Optional[List[int]]]:
    """per transcript its label indices, or None when it holds a character the charset lacks"""
    index = {c: i for i, c in enumerate(charset)}
    return [[index[ch] for ch in t] if all(ch in index for ch in t) else None for t in texts]


_NAN = float("nan")                # the one NaN of an empty list's mean: two result dicts then compare equal with ==


def _mean_ci(v):
    return (float(np.mean(v)), float(np.std(v) * 1.96 / np.sqrt(len(v)))) if len(v) else (_NAN, _NAN)


def _evaluate_predictions_device(pred_labels, gt_texts, cs: List, dataset: str, metrics: str, unicode_charset: bool, device,
                                 confusion: Optional["E.ConfusionReport"]) -> Dict:
    """evaluate_predictions with every dynamic program of the pass on the device: the label pairs (CER, CR's operations, the
    confusion report's alignment) in one E.edit_align call, the normalised strings and the word-id sequences in a second, then the
    host path's bookkeeping on the integers that come back."""
    from . import ops
    conv =(lambda c: chr(c)) if unicode_charset else (lambda c: c)
    index: Dict = {}
    for i, c in enumerate(cs):                                                     # cs.index: the first position of a repeated entry
        index.setdefault(c, i)
    string_cer, lines = dataset in CER_DATASETS, []
    jobs_a, jobs_b, word_ids = [], [], {}
    for pred, text in zip(pred_labels, gt_texts):
        if pred is None:
            continue
        pred = [int(v) for v in pred]
        gt = []
        for c in text:
            key = ord(c) if unicode_charset else c
            if key not in index:
                cs.index(key)                                                      # the host path's ValueError
            gt.append(index[key])
        if len(pred) > 0 and len(gt) == 0:
            raise ValueError("character_error_rate_with_impact: empty ground truth")
        line = dict(pred=pred, gt=gt, ps="".join(conv(cs[i]) for i in pred), gs="".join(conv(cs[i]) for i in gt))
        if string_cer:
            line["string"] = len(jobs_a)
            jobs_a.append(E.process_pred_string(line["gs"]))
            jobs_b.append(E.process_pred_string(line["ps"]))
        if metrics == "default":
            gw, pw = ([word_ids.setdefault(tuple(w), len(word_ids)) for w in E.split_labels_into_words(z, cs)] for z in (gt, pred))
            line["words"], line["n_pred_words"] = len(jobs_a), len(pw)
            jobs_a.append(gw)
            jobs_b.append(pw)
        lines.append(line)
    gts, preds = [ln["gt"] for ln in lines], [ln["pred"] for ln in lines]
    if confusion is not None:                                                      # the alignments stay on the device: only the table returns
        on = set(E._device_pairs(gts, preds))
        dev_lines = [k for k in range(len(lines)) if k in on]
        a, a_off, b, b_off = ops.edit_align_tables([gts[k] for k in dev_lines], [preds[k] for k in dev_lines])
        a, b = a.to(device), b.to(device)
        d, c, n_ops, steps = ops.edit_align(a, a_off, b, b_off, True)
        confusion.add_device(a, a_off, b, b_off, n_ops, steps)
        lab_d, lab_c = [None] * len(lines), [None] * len(lines)
        for k, dk, ck in zip(dev_lines, d.cpu().tolist(), c.cpu().tolist()):
            lab_d[k], lab_c[k] = dk, tuple(ck)
        for k in range(len(lines)):
            if k not in on:                                                        # a line above the device's length limit
                lab_d[k], lab_c[k] = E.levenshtein(preds[k], gts[k]), E.compute_edit_operations(gts[k], preds[k])
                confusion.add_alignment(gts[k], preds[k], E.compute_edit_alignment(gts[k], preds[k]))
    else:
        lab_d, lab_c, _ = E.edit_align_batch(gts, preds, device)
    job_d = E.edit_align_batch(jobs_a, jobs_b, device)[0] if jobs_a else []

    CER_list, WER_list, AR_list, CR_list, WA_list = [], [], [], [], []
    dict_char: Dict[int, int] = {}
    preds_str, gts_str, dist_sum, len_sum = [], [], 0, 0
    for k, line in enumerate(lines):
        pred, gt = line["pred"], line["gt"]
        if len(pred) > 0:
            E.character_impact(pred, gt, dict_char)
            cer_it = lab_d[k] / len(gt)
        else:
            cer_it = 1
        preds_str.append(line["ps"])
        gts_str.append(line["gs"])
        if string_cer:
            dist_sum += job_d[line["string"]]
            len_sum += len(jobs_a[line["string"]])
            cer_it = dist_sum / len_sum
        if metrics == "default":
            CER_list.append(cer_it)
            WER_list.append(job_d[line["words"]] / max(line["n_pred_words"], 1))
        elif metrics == "CER_only":
            CER_list.append(cer_it)
        elif metrics == "chinese":
            CER_list.append(cer_it)
            AR_list.append(1 - cer_it)
            CR_list.append((len(gt) - lab_c[k][1] - lab_c[k][2]) / len(gt))
        elif metrics == "cipher":
            CER_list.append(cer_it)
            WA_list.append(E.compute_wa(gt, pred))
        else:
            raise ValueError(f"unknown --metrics {metrics}")
    return dict(CER_list=CER_list, WER_list=WER_list, AR_list=AR_list, CR_list=CR_list, WA_list=WA_list, dict_char=dict_char,
                list_preds_str=preds_str, list_gt_str=gts_str, cer=_mean_ci(CER_list), wer=_mean_ci(WER_list), ar=_mean_ci(AR_list),
                cr=_mean_ci(CR_list), wa=_mean_ci(WA_list))


def evaluate_predictions(pred_labels: Sequence[Sequence[int]], gt_texts: Sequence[str], charset: Sequence, dataset: str = "IAM",
                         metrics: str = "default", unicode_charset: bool = False, device=None,
                         confusion: Optional["E.ConfusionReport"] = None) -> Dict:
    """The per-sample metric bookkeeping of evaluation.py:495-581 on already decoded predictions.
    device (`--device-metrics`): every edit-distance lattice of the pass -- label CER, the normalised strings' distance, the word-level
    WER, CR's operations -- runs on that device in a few launches for the whole pass instead of line by line in
    Python; the returned dict equals the host path's with ==, every ratio being formed here from the same integers.
    confusion: an E.ConfusionReport that takes the label-level alignment (a = ground truth) of every scored line; with a device the
    alignments are gathered and counted there."""
    cs = list(charset)
    if device is not None:
        return _evaluate_predictions_device(pred_labels, gt_texts, cs, dataset, metrics, unicode_charset, device, confusion)
    CER_list, WER_list, AR_list, CR_list, WA_list = [], [], [], [], []
    dict_char: Dict[int, int] = {}
    preds_str, gts_str, dists, lens = [], [], [], []
    conv = (lambda c: chr(c)) if unicode_charset else (lambda c: c)
    for pred, text in zip(pred_labels, gt_texts):
        if pred is None:                                                           # skipped line (evaluation.py:501-504: `continue`)
            continue
        gt = [cs.index(ord(c) if unicode_charset else c) for c in text]            # datasets/IAM.py:66-72
        if len(pred) > 0:                                                          # evaluation.py:340-352
            cer_it, dict_char, _ = E.character_error_rate_with_impact(list(pred), gt, dict_char)
        else:
            cer_it = 1
        preds_str.append("".join(conv(cs[int(i)]) for i in pred))
        gts_str.append("".join(conv(cs[int(i)]) for i in gt))
        wer_it = None
        if dataset in CER_DATASETS:                                                # :521-535 running string-level CER
            pg, pp = E.process_pred_string(gts_str[-1]), E.process_pred_string(preds_str[-1])
            dists.append(E.levenshtein(pg, pp))
            lens.append(len(pg))
            cer_it = sum(dists) / sum(lens)
        if metrics == "default":                                                   # :544-549 (argument order as the reference calls it)
            wer_it = E.word_error_rate(E.split_labels_into_words(gt, cs), E.split_labels_into_words(list(pred), cs))
            CER_list.append(cer_it)
            WER_list.append(wer_it)
        elif metrics == "CER_only":
            CER_list.append(cer_it)
        elif metrics == "chinese":                                                 # :560-565
            CER_list.append(cer_it)
            AR_list.append(1 - cer_it)
            CR_list.append(E.compute_cr(gt, list(pred)))
        elif metrics == "cipher":                                                  # :572-575
            CER_list.append(cer_it)
            WA_list.append(E.compute_wa(gt, list(pred)))
        else:
            raise ValueError(f"unknown --metrics {metrics}")
        if confusion is not None:
            confusion.add_alignment(gt, list(pred), E.compute_edit_alignment(gt, list(pred)))

    return dict(CER_list=CER_list, WER_list=WER_list, AR_list=AR_list, CR_list=CR_list, WA_list=WA_list, dict_char=dict_char,
                list_preds_str=preds_str, list_gt_str=gts_str, cer=_mean_ci(CER_list), wer=_mean_ci(WER_list), ar=_mean_ci(AR_list),
                cr=_mean_ci(CR_list), wa=_mean_ci(WA_list))


def write_outputs(res: Dict, out_dir: str, dataset: str, TH, NM) -> str:
    """The files evaluation.py:584-656 writes (except the PNG)."""
    stats_dir = os.path.join(out_dir, dataset)
    os.makedirs(stats_dir, exist_ok=True)
    np.save(os.path.join(stats_dir, "cer_list.npy"), res["CER_list"])
    with open(os.path.join(stats_dir, "dict_char.json"), "w") as f:
        json.dump(res["dict_char"], f)
    with open(os.path.join(stats_dir, "list_preds.txt"), "w", encoding="utf-8") as fp, \
            open(os.path.join(stats_dir, "list_gt.txt"), "w", encoding="utf-8") as fg:
        for p, g in zip(res["list_preds_str"], res["list_gt_str"]):
            fp.write(f"{p}\n")
            fg.write(f"{g}\n")
    with open(os.path.join(stats_dir, f"cer_TH_{TH}_NMS_{NM}.txt"), "w") as f:
        f.write(f"CER (TH={TH}) (NMS={NM}): {res['cer'][0]:.4f} +- {res['cer'][1]:.4f}")
    return stats_dir


def default_ngram_tokens(charset: Sequence) -> List[str]:
    """The token table of the n-gram side, indexed by emission channel: the CTC token, then the charset with " " spelled <space>
    (the layout ngram/preprocessing/get_char_training_text.py:95-100 writes)."""
    return ["<ctc>"] + ["<space>" if c == " " else str(c) for c in charset]


def default_ngram_ignore(charset: Sequence) -> List[int]:
    """Channels that are never re-scored: the charset's non-alphanumeric characters except the apostrophe (the RIMES / READ rule of
    ngram/clean_gen_ngram_preds.py:288-311)."""
    return [i + 1 for i, c in enumerate(charset) if not str(c).isalnum() and str(c) != "'"]


def _ngram_tokens_ignore(args, charset: Sequence):
    """(tokens, ngram_charset, ignore) of the re-scoring path from --ngram-tokens / --ngram-ignore"""
    if args.ngram_tokens:
        with open(args.ngram_tokens, encoding="utf-8") as f:
            tokens = [line.rstrip("\n") for line in f if line.rstrip("\n")]
    else:
        tokens = default_ngram_tokens(charset)
    if len(tokens) != len(charset) + 1:
        raise SystemExit(f"--ngram-tokens: {len(tokens)} tokens for {len(charset)} characters + the CTC token")
    if len(set(tokens)) != len(tokens):
        dup = sorted({t for t in tokens if tokens.count(t) > 1})
        raise SystemExit(f"--ngram-tokens: repeated token(s) {dup}: a token must name one emission channel")
    ngram_charset = ["<ctc>"] + [str(c) for c in charset]
    if args.ngram_ignore is None:
        ignore = default_ngram_ignore(charset)
    else:
        missing = [c for c in args.ngram_ignore if c not in ngram_charset[1:]]
        if missing:
            raise SystemExit(f"--ngram-ignore: {missing} not in the charset")
        ignore = [ngram_charset.index(c, 1) for c in args.ngram_ignore]
    return tokens, ngram_charset, ignore


def ngram_bundle(args, charset: Sequence, device) -> Optional[Dict]:
    """What predict_labels(ngram=...) takes, from the command line; None without --ngram-arpa / --ngram-train-text."""
    if not args.ngram_arpa and not args.ngram_train_text:
        return None
    from . import ngram as NG
    tokens, ngram_charset, ignore = _ngram_tokens_ignore(args, charset)
    if args.ngram_train_text:
        from . import lmtrain
        with open(args.ngram_train_text, encoding="utf-8") as f:
            lines = lmtrain.char_lines(f, keep=[str(c) for c in charset])
        lm = lmtrain.train_ngram(lines, args.ngram_order, device=device).to_arpa_lm()
    else:
        lm = NG.ArpaLM(args.ngram_arpa)
    dec = NG.DeviceNgramDecoder(tokens, lm, args.ngram_weight, args.ngram_beam, args.ngram_beam_token,
                                blank_token=tokens[0], device=device)
    return dict(decoder=dec, ignore=ignore, ngram_charset=ngram_charset, no_uppercase_words=args.no_uppercase_words,
                no_digits=args.no_digits, no_dash=args.no_dash, multiply_pred_logits_by=args.multiply_pred_logits_by)


def load_lexicon(path: str):
    """`--lexicon`: UTF-8, one word per line, optionally `word<TAB>count`; empty lines are dropped.  -> (words, counts or None: counts
    only when every line carries one)"""
    words, counts = [], []
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\r\n")
            if not line:
                continue
            w, tab, c = line.partition("\t")
            words.append(w)
            if tab:
                try:
                    counts.append(float(c))
                except ValueError:
                    raise SystemExit(f"--lexicon: {line!r}: the count after the tab is no number")
    if counts and len(counts) != len(words):
        raise SystemExit("--lexicon: either every line carries `word<TAB>count` or none does")
    return words, counts or None


def check_lexicon_args(args) -> None:
    """the refusals of the --lexicon flags, before any work (main calls it first); without --lexicon the other three are not read"""
    if not args.lexicon:
        return
    if args.ngram_arpa or args.ngram_train_text:
        raise SystemExit("--lexicon and --ngram-arpa are two decoders for the same word spans: give one")
    if not 1 <= args.lexicon_nbest <= 8:
        raise SystemExit(f"--lexicon-nbest {args.lexicon_nbest} outside 1..8")
    if not 0.0 <= args.lexicon_min_conf <= 1.0:
        raise SystemExit(f"--lexicon-min-conf {args.lexicon_min_conf} outside 0..1")


def lexicon_bundle(args, charset: Sequence, device) -> Optional[Dict]:
    """What predict_labels(ngram=...) takes when the word spans go to the device lexicon decoder (`--lexicon`): the dict shape of
    ngram_bundle, tokens and ignore flags included; None without --lexicon.  A word that cannot be packed (a character that is no
    token, more than 64 characters) is named on stderr and skipped."""
    if not args.lexicon:
        return None
    from . import ngram as NG
    tokens, ngram_charset, ignore = _ngram_tokens_ignore(args, charset)
    words, counts = load_lexicon(args.lexicon)
    good, good_counts = [], []
    chan_of = {t: c for c, t in enumerate(tokens) if c > 0}
    for i, w in enumerate(words):
        try:
            NG.spell_word(w, chan_of)
        except ValueError as e:
            print(f"--lexicon: {e}: skipped", file=sys.stderr)
            continue
        if counts is not None and not counts[i] > 0:
            print(f"--lexicon: {w!r} has the count {counts[i]}: skipped", file=sys.stderr)
            continue
        good.append(w)
        good_counts.append(counts[i] if counts is not None else 1.0)
    if not good:
        raise SystemExit(f"--lexicon: {args.lexicon} holds no word that can be spelled with the tokens")
    dec = NG.DeviceLexiconDecoder(tokens, good, good_counts if counts is not None else None, args.lexicon_prior_weight,
                                  args.lexicon_min_conf, args.lexicon_nbest, device=device, blank_token=tokens[0])
    return dict(decoder=dec, ignore=ignore, ngram_charset=ngram_charset, no_uppercase_words=args.no_uppercase_words,
                no_digits=args.no_digits, no_dash=args.no_dash, multiply_pred_logits_by=args.multiply_pred_logits_by)


def check_word_beam_args(args) -> None:
    """the refusals of the --word-beam flags, before any work (main calls it first); without --word-beam-lexicon the others are not read"""
    if not args.word_beam_lexicon:
        if args.word_beam_arpa:
            raise SystemExit("--word-beam-arpa needs --word-beam-lexicon: the word n-gram scores the dictionary's words")
        return
    if args.ngram_arpa or args.ngram_train_text or args.lexicon:
        raise SystemExit("--word-beam-lexicon decodes whole lines, --ngram-arpa and --lexicon the word spans of the argmax: give one")
    if args.layout_out or args.layout_align:
        raise SystemExit("--word-beam-lexicon has no located output: not together with --layout-out / --layout-align")
    if not 1 <= args.word_beam_beam <= 64:
        raise SystemExit(f"--word-beam-beam {args.word_beam_beam} outside 1..64")
    if args.word_beam_beam_token is not None and args.word_beam_beam_token < 0:
        raise SystemExit(f"--word-beam-beam-token {args.word_beam_beam_token} is negative")


def word_beam_bundle(args, charset: Sequence, device) -> Optional[Dict]:
    """What predict_labels(ngram=...) takes when whole lines go to the device word beam search (`--word-beam-lexicon`); None without
    it.  A word that cannot be packed (a character that is no token, more than 64 characters) is named on stderr and skipped; counts in
    the file are not used.  Separators: every channel no dictionary word uses."""
    if not args.word_beam_lexicon:
        return None
    from . import ngram as NG
    tokens, _, _ = _ngram_tokens_ignore(args, charset)
    words, _ = load_lexicon(args.word_beam_lexicon)
    good = []
    chan_of = {t: c for c, t in enumerate(tokens) if c > 0}
    for w in words:
        try:
            NG.spell_word(w, chan_of, "--word-beam-lexicon")
        except ValueError as e:
            print(f"{e}: skipped", file=sys.stderr)
            continue
        good.append(w)
    if not good:
        raise SystemExit(f"--word-beam-lexicon: {args.word_beam_lexicon} holds no word that can be spelled with the tokens")
    lm = NG.ArpaLM(args.word_beam_arpa) if args.word_beam_arpa else None
    dec = NG.DeviceWordBeamDecoder(tokens, good, lm, args.word_beam_weight if lm is not None else 0.0, args.word_beam_beam,
                                   args.word_beam_beam_token, lookahead=not args.word_beam_no_lookahead, blank_token=tokens[0], device=device)
    return dict(decoder=dec, word_beam=True, multiply_pred_logits_by=args.multiply_pred_logits_by)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m dtlr_amd.evaluation", description=__doc__.split("\n\n")[0])
    # the reference's flags (evaluation.py:15-27)
    ap.add_argument("--dataset", default="IAM")
    ap.add_argument("--mode", default="val")
    ap.add_argument("--new_class_embedding", action="store_true")
    ap.add_argument("--new_label_enc", action="store_true")
    ap.add_argument("--NMS_inference", action="store_true")
    ap.add_argument("--metrics", default="default", choices=["default", "CER_only", "chinese", "cipher"])
    ap.add_argument("--unicode", action="store_true")
    ap.add_argument("--weights", default="checkpoint.pth")
    ap.add_argument("--config", default="latin", help="a reference config file (config/*.py) or a preset: latin | chinese | tiny")
    ap.add_argument("--fix_enc_out_class", action="store_true")
    ap.add_argument("--TH", type=float, default=None)
    ap.add_argument("--NMS", type=float, default=None)
    # what the reference takes from its dataset registry (datasets/config.json + build_dataset)
    ap.add_argument("--images", required=True, help="folder with the line images (<id>.jpg / .png)")
    ap.add_argument("--labels", required=True, help="labels.pkl (reference layout), .json or .tsv")
    ap.add_argument("--charset", default=None, help="charset file (.json list / .pkl list); default datasets/default_charset.json")
    ap.add_argument("--out", default="stats_dect")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batching", default="exact", choices=["exact", "padded", "ragged"],
                    help="exact: same-size lines only (bs = 1 results); padded: mixed sizes in one canvas (the reference's padded-batch "
                         "results); ragged: mixed sizes in one canvas, each line with its bs = 1 result")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32s", "f32"],
                    help="bf16 / f16: the 16-bit engines; f32s: fp32 activations, split fp16 products (parity-grade, ~1/3 of the 16-bit rate); f32: exact-fp32 MFMA")
    ap.add_argument("--limit", type=int, default=0, help="evaluate only the first N lines")
    ap.add_argument("--size", type=int, default=EVAL_SIZE, help="eval resize: short side (config/coco_transformer.py:1)")
    ap.add_argument("--max_size", type=int, default=EVAL_MAX_SIZE, help="eval resize: long-side cap (config/coco_transformer.py:2)")
    # n-gram re-scoring (the reference's ngram/ path; ngram/IAM.yaml: 6-gram character model, weight 0.25, per word)
    lm_source = ap.add_mutually_exclusive_group()               # one character n-gram: read, or trained here
    lm_source.add_argument("--ngram-arpa", default=None, help="character n-gram in ARPA text: switches re-scoring by the device beam decoder on")
    lm_source.add_argument("--ngram-train-text", default=None, metavar="FILE",
                           help="instead of --ngram-arpa: train the character n-gram on the device from this UTF-8 text (dtlr_amd.lmtrain, "
                                "level char-word: every word a line of its characters, characters outside the charset dropped)")
    ap.add_argument("--ngram-order", type=int, default=5, help="order of the model --ngram-train-text trains, 1..8")
    ap.add_argument("--ngram-weight", type=float, default=0.25)
    ap.add_argument("--ngram-beam", type=int, default=50, help="beam size, 1..64")
    ap.add_argument("--ngram-beam-token", type=int, default=None, help="tokens extended per frame (default: all)")
    ap.add_argument("--ngram-tokens", default=None, help="token table, one per line, channel order (default: <ctc> + the charset, ' ' as <space>)")
    ap.add_argument("--ngram-ignore", default=None, help="characters never re-scored (default: the charset's non-alphanumerics except ')")
    ap.add_argument("--lexicon", default=None, metavar="FILE",
                    help="closed-vocabulary decoding of the word spans on the device: UTF-8, one word per line, optionally word<TAB>count; "
                         "uses --ngram-tokens / --ngram-ignore and the no_* flags; not together with --ngram-arpa")
    ap.add_argument("--lexicon-min-conf", type=float, default=0.5,
                    help="a span takes its best word when exp((score - base) / characters) >= this, else it keeps its argmax")
    ap.add_argument("--lexicon-prior-weight", type=float, default=0.0, help="weight of ln(count / sum of counts) in a word's key")
    ap.add_argument("--lexicon-nbest", type=int, default=1, help="words returned per span, 1..8")
    ap.add_argument("--word-beam-lexicon", default=None, metavar="FILE",
                    help="word beam search of the WHOLE line on the device: only the words of FILE (the format of --lexicon), with "
                         "separators between them; uses --ngram-tokens; not together with --ngram-arpa, --lexicon, --layout-out, --layout-align")
    ap.add_argument("--word-beam-arpa", default=None, metavar="FILE", help="word-level n-gram in ARPA text that scores the word sequence")
    ap.add_argument("--word-beam-weight", type=float, default=0.5, help="weight of the word n-gram")
    ap.add_argument("--word-beam-beam", type=int, default=50, help="beam size, 1..64")
    ap.add_argument("--word-beam-beam-token", type=int, default=None, help="tokens extended per frame (default: all)")
    ap.add_argument("--word-beam-no-lookahead", action="store_true",
                    help="rank a hypothesis inside a word without the best unigram of the words it can still become")
    ap.add_argument("--multiply_pred_logits_by", type=float, default=1.0)
    ap.add_argument("--no_uppercase_words", action="store_true")
    ap.add_argument("--no_digits", action="store_true")
    ap.add_argument("--no_dash", action="store_true")
    ap.add_argument("--layout-out", default=None, metavar="FILE.jsonl",
                    help="also write every line's located transcript (characters and words with boxes in source-image pixels), one JSON "
                         "object per line image; needs a single decoder setting")
    ap.add_argument("--layout-align", action="store_true",
                    help="with --layout-out and an n-gram: a word the beam rewrote also gets \"aligned\", its characters placed by the "
                         "forced alignment of its labels over its own frames")
    ap.add_argument("--align-out", default=None, metavar="FILE.jsonl",
                    help="also write the forced alignment of every line's transcript (--labels) against the model's output: the located "
                         "JSON with \"decoder\": \"align\", each character where the best CTC path puts it, plus \"logp\" and \"feasible\"")
    ap.add_argument("--spot-words", default=None, metavar="FILE",
                    help="keyword spotting: the words to look for in every line, one per line (UTF-8); needs --spot-out; single process only")
    ap.add_argument("--spot-patterns", default=None, metavar="FILE",
                    help="regular-expression spotting: the expressions to look for in every line, one per line (UTF-8; literals, classes, "
                         "\\d \\w \\s, groups, |, * + ? {m,n}); shares --spot-out, --spot-min-conf and --spot-max-hits with --spot-words; "
                         "single process only")
    ap.add_argument("--spot-length-bonus", type=float, default=None,
                    help="what every character adds to the key an expression's hits grow and are ranked by (default: -ln of --spot-min-conf, "
                         "0 without a bar)")
    ap.add_argument("--spot-out", default=None, metavar="FILE.jsonl",
                    help="one JSON object per hit: the line's id, the word, conf, ratio, the ranks it covers, its box in the source image's "
                         "pixels and its characters")
    ap.add_argument("--spot-min-conf", type=float, default=0.5, help="a hit needs exp(ratio / length) >= this (0: the best hit of every word)")
    ap.add_argument("--spot-max-hits", type=int, default=4, help="hits per (line, word), 1..16")
    ap.add_argument("--device-metrics", action="store_true",
                    help="run the edit-distance lattices of the metrics (CER, WER, CR) on the device, batched over the whole pass; the "
                         "figures and files are those of the host path")
    ap.add_argument("--confusion-out", default=None, metavar="FILE.json",
                    help="also write the confusion report of the label-level alignment of all scored lines: substitutions per (gt, pred), "
                         "deletions, insertions, recall per character; implies --device-metrics; needs a single decoder setting")
    ap.add_argument("--confusion-top", type=int, default=50, help="entries kept in each list of --confusion-out, most frequent first")
    return ap


def check_metrics_args(args) -> None:
    """the refusals of --confusion-out / --confusion-top, before any work (main calls it first); without --confusion-out the other is
    not read"""
    if not args.confusion_out:
        return
    if args.confusion_top < 1:
        raise SystemExit(f"--confusion-top {args.confusion_top} must be at least 1")
    if args.NMS_inference and (args.NMS is None or args.TH is None):
        raise SystemExit("--confusion-out needs one decoder setting (--TH and --NMS, or neither), not the --NMS_inference grid")


def write_confusion(path: str, report: "E.ConfusionReport", charset: Sequence, top: int) -> Dict:
    """`--confusion-out`: ConfusionReport.to_json as one JSON object"""
    obj = report.to_json(charset, top)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(obj, f, ensure_ascii=False, indent=1)
    return obj


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    args = build_parser().parse_args(argv)
    check_lexicon_args(args)
    check_word_beam_args(args)
    check_metrics_args(args)
    from .dino import DINO, PostProcess
    rank, local, world = ddist.init_from_env()
    if bool(args.spot_words or args.spot_patterns) != bool(args.spot_out):
        raise SystemExit(f"--spot-{'patterns' if args.spot_patterns and not args.spot_words else 'words'} and --spot-out go together")
    if args.spot_words and world > 1:
        raise SystemExit(f"--spot-words runs in a single process (this job has {world} ranks): hits are not merged across ranks")
    if args.spot_patterns and world > 1:
        raise SystemExit(f"--spot-patterns runs in a single process (this job has {world} ranks): hits are not merged across ranks")
    if not torch.cuda.is_available():
        raise SystemExit("dtlr_amd.evaluation needs an MI355X (no CPU path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    charset = load_charset(args.charset)
    if args.config in ("latin", "chinese"):
        cfg = {"latin": DTLRConfig.latin, "chinese": DTLRConfig.chinese}[args.config]()
    elif args.config == "tiny":                 # reduced network of the test-suite (same topology, KB-sized assets)
        cfg = DTLRConfig.tiny(num_classes=len(charset))
    else:
        cfg = DTLRConfig.from_reference_file(args.config)
    rows = load_labels(args.labels, args.mode)
    if args.limit:
        rows = rows[: args.limit]
    model = DINO(cfg, compute_dtype={"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32s": "f32s"}[args.dtype])
    model = E.load_model(model, args.weights, device=dev, new_class_embedding=args.new_class_embedding, charset_size=len(charset),
                         new_label_enc=args.new_label_enc, fix_enc_out_class=args.fix_enc_out_class)
    # TH / NM grids exactly as evaluation.py:38-49
    if args.NMS is not None and args.TH is not None:
        list_TH, list_NM, nms_inference = [args.TH], [args.NMS], True
    elif not args.NMS_inference:
        list_TH, list_NM, nms_inference = [None], [None], False
    else:
        list_TH = list_NM = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
        nms_inference = True
    paths = [find_image(args.images, name) for name, _ in rows]
    def header_size(p):                                        # an unreadable file is a per-sample error: it fails (and is skipped) when its shard decodes it
        try:
            return image_size(p)
        except Exception:
            return (size_fallback, size_fallback)
    size_fallback = 32
    sizes = [header_size(p) for p in paths]                    # headers only; pixels are decoded per shard, inside predict_labels
    images = lambda i: read_rgb(paths[i])                      # noqa: E731
    texts = [t for _, t in rows]
    post = PostProcess(num_select=cfg.num_select, nms_iou_threshold=cfg.nms_iou_threshold)
    bundle = ngram_bundle(args, charset, dev) or lexicon_bundle(args, charset, dev) or word_beam_bundle(args, charset, dev)
    extra = {"ngram": bundle} if bundle is not None else {}
    last = {}
    spot = None
    if args.spot_words or args.spot_patterns:
        cs_str = [chr(c) if args.unicode else str(c) for c in charset]
        spot = spot_bundle(load_spot_words(args.spot_words) if args.spot_words else [], cs_str, args.spot_min_conf, args.spot_max_hits,
                           load_spot_patterns(args.spot_patterns) if args.spot_patterns else (), args.spot_length_bonus)
    if args.layout_out and len(list_TH) * len(list_NM) > 1:
        raise SystemExit("--layout-out needs one decoder setting (--TH and --NMS, or neither), not the --NMS_inference grid")
    if args.align_out:                                         # the transcripts against the model's output; apart from the decoders
        cs_str = [chr(c) if args.unicode else str(c) for c in charset]
        aligned = predict_located(model, images, args.batch, args.batching == "exact", None, None, dev, args.size, args.max_size,
                                  rank=rank, world=world, sizes=sizes, per_line=args.batching == "ragged", decoder="align",
                                  space_label=E.space_label_of(cs_str), targets=transcript_labels(texts, cs_str))
        if rank == 0:
            k = write_aligned(args.align_out, [name for name, _ in rows], aligned, cs_str)
            print(f"wrote {k} aligned lines to {args.align_out}", file=sys.stderr)
    for TH in list_TH:
        for NM in list_NM:
            if args.layout_out:                                # the same decode with its records kept: the labels are the metrics' input
                cs_str = [chr(c) if args.unicode else str(c) for c in charset]
                located = predict_located(model, images, args.batch, args.batching == "exact", TH, NM, dev, args.size, args.max_size,
                                          rank=rank, world=world, sizes=sizes, per_line=args.batching == "ragged", ngram=bundle,
                                          decoder="ngram" if bundle is not None else ("nms" if nms_inference else "blank"),
                                          space_label=E.space_label_of(cs_str), align_rewritten=args.layout_align and bundle is not None,
                                          spot=spot)
                preds = [None if line is None else list(line.labels) for line in located]
                if rank == 0:
                    k = write_layout(args.layout_out, [name for name, _ in rows], located, cs_str)
                    print(f"wrote {k} located lines to {args.layout_out}", file=sys.stderr)
            else:
                preds = predict_labels(model, images, args.batch, args.batching == "exact", TH, NM, post, dev, args.size, args.max_size,
                                       rank=rank, world=world, sizes=sizes, per_line=args.batching == "ragged", spot=spot, **extra)
            if spot is not None:                               # the first pass over the images carries the search
                k = write_spotted(args.spot_out, [name for name, _ in rows], spot, cs_str)
                what = f"{len(spot['words'])} words" + (f" and {len(spot['patterns'])} patterns" if args.spot_patterns else "")
                print(f"wrote {k} hits of {what} to {args.spot_out}", file=sys.stderr)
                spot = None
            if rank == 0:
                if args.device_metrics or args.confusion_out:
                    report = E.ConfusionReport() if args.confusion_out else None
                    res = evaluate_predictions(preds, texts, charset, args.dataset, args.metrics, args.unicode, device=dev, confusion=report)
                    if report is not None:
                        write_confusion(args.confusion_out, report, [chr(c) if args.unicode else str(c) for c in charset], args.confusion_top)
                        print(f"wrote the confusion report of {report.lines} lines to {args.confusion_out}", file=sys.stderr)
                else:
                    res = evaluate_predictions(preds, texts, charset, args.dataset, args.metrics, args.unicode)
                d = write_outputs(res, args.out, args.dataset, TH, NM)
                tail = f", TH {TH}, NM {NM}" if nms_inference else ""
                if args.metrics == "chinese":
                    print(f"AR {res['ar'][0]:.6f} +- {res['ar'][1]:.6f}, CR {res['cr'][0]:.6f} +- {res['cr'][1]:.6f}, lines {len(preds)}{tail}")
                elif args.metrics == "cipher":
                    print(f"SER {res['cer'][0]:.6f} +- {res['cer'][1]:.6f}, WA {res['wa'][0]:.6f} +- {res['wa'][1]:.6f}, lines {len(preds)}{tail}")
                elif args.metrics == "CER_only":
                    print(f"cer {res['cer'][0]:.6f} +- {res['cer'][1]:.6f}, lines {len(preds)}{tail}")
                else:
                    print(f"cer {res['cer'][0]:.6f} +- {res['cer'][1]:.6f}, wer {res['wer'][0]:.6f} +- {res['wer'][1]:.6f}, lines {len(preds)}{tail}")
                print(f"wrote {d}", file=sys.stderr)
                last = res
            if not nms_inference:
                break
        if not nms_inference:
            break
    ddist.finalize()
    return last


if __name__ == "__main__":
    main()
