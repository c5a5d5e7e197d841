"""Adapt the class head of a pretrained model to a new charset, on the device.

  finetuning.py --new_class_embedding (+ engine.train_one_epoch_CTC)   ->   new_class_head / smart_mapping_init + HeadTrainer
  `python -m dtlr_amd.adapt`                                           ->   a checkpoint that
                                                                            evaluation.load_model(new_class_embedding=True,
                                                                            fix_enc_out_class=True) loads

The reference adapts a model to a new script by rebuilding the class heads for the new charset (finetuning.py:422-539) and training
them against the CTC loss (engine.py:160-260).  That loop calls `criterion.loss_CTC(outputs, targets, None, None)` (engine.py:200): the
CTC loss on the FINAL pred_logits only, and with --new_class_embedding the optimizer holds only the class heads.  With
dec_pred_class_embed_share (every shipped config) pred_logits = class_embed(hs[-1]) is one shared Linear; the decoder's own copy and the
two-stage head receive no gradient from this loss (the top-k is not differentiable, the reference points are detached) and AdamW skips
parameters without a gradient.  dropout = 0, use_dn = False and FrozenBN make the training-mode forward equal the eval forward.  So one
step is: the frozen forward this package already has, the CTC loss's gradient with respect to the logits
(dtlr_ctc_loss_interleaved_backward), dW = dlogits^T hs (dtlr_head_grad), clip (dtlr_grad_norm_scale), AdamW (dtlr_adamw_step) -- four
HIP entry points, no backward through the trunk.  Nothing in a step waits for the device: the host's part is packing the label lists
into the targets tensor and its (pageable) copy to the device; the loss stays a device tensor until the caller reads it.
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import evaluation as E
from . import ops


def smart_mapping_init(old_head, old_charset: Sequence, new_charset: Sequence, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """--smart_mapping (finetuning.py:454-510): the rows of the new head are rows of the old one.  A character present in both charsets
    takes its own old row (first occurrence in old_charset); the other new characters take the old rows no shared character uses, in a
    seeded random order.  When there are fewer unused rows than new characters, the list is first topped up with seeded random rows, as
    the reference does.  old_head: an nn.Linear or a (weight [C_old, D], bias [C_old]) pair.  Returns (weight [C_new, D], bias [C_new]).

    NOT the reference's random stream: it draws from the unseeded global np.random; here the draws come from
    np.random.Generator(PCG64(seed)), so the same inputs always give the same head."""
    w, b = (old_head.weight, old_head.bias) if isinstance(old_head, nn.Linear) else old_head
    w, b = w.detach(), b.detach()
    old_charset, new_charset = list(old_charset), list(new_charset)
    if w.shape[0] != len(old_charset):
        raise ValueError(f"smart_mapping_init: the old head has {w.shape[0]} rows, old_charset {len(old_charset)} characters")
    mapping = smart_mapping(old_charset, new_charset, seed)
    idx = torch.as_tensor(mapping, dtype=torch.long, device=w.device)
    return w[idx].clone(), b[idx].clone()


def smart_mapping(old_charset: Sequence, new_charset: Sequence, seed: int = 0) -> List[int]:
    """new class index -> old class index of smart_mapping_init."""
    old_charset, new_charset = list(old_charset), list(new_charset)
    first = {}
    for i, ch in enumerate(old_charset):
        first.setdefault(ch, i)
    mapping: Dict[int, int] = {}
    unused = list(range(len(old_charset)))
    not_mapped = []
    for i, ch in enumerate(new_charset):
        if ch in first:
            mapping[i] = first[ch]
            if mapping[i] in unused:                      # a character listed twice in new_charset shares its old row
                unused.remove(mapping[i])
        else:
            not_mapped.append(i)
    g = np.random.Generator(np.random.PCG64(seed))
    while len(unused) < len(not_mapped):
        unused.append(int(g.integers(0, len(old_charset))))
    unused = [unused[k] for k in g.permutation(len(unused))]
    for k, i in enumerate(not_mapped):
        mapping[i] = unused[k]
    return [mapping[i] for i in range(len(new_charset))]


def new_class_head(model, num_classes: int, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
    """The head rebuild of finetuning.py:422-452,524-529 on `model` (a dtlr_amd DINO): one fresh Linear(hidden -> num_classes) shared by
    the decoder layers under `class_embed`, a separate bare Linear under `transformer.decoder.class_embed` (the reference creates it;
    no forward uses it), `enc_out_class_embed` KEPT (the non-smart branch, :364-366 / :524-529).  weight / bias: the initial head
    (smart_mapping_init's result); default: nn.Linear's own initialisation, as in the reference.  The resulting state dict is what
    evaluation.load_model(new_class_embedding=True, fix_enc_out_class=True, charset_size=num_classes) loads."""
    if not model.dec_pred_class_embed_share:
        raise NotImplementedError("new_class_head: written for dec_pred_class_embed_share (every shipped config)")
    old = model.class_embed[0]
    d, dev = old.weight.shape[1], old.weight.device
    head = nn.Linear(d, int(num_classes))
    if weight is not None:
        with torch.no_grad():
            head.weight.copy_(weight)
            head.bias.copy_(bias)
    model.class_embed = nn.ModuleList([head for _ in range(model.transformer.num_decoder_layers)]).to(dev)
    model.transformer.decoder.class_embed = nn.Linear(d, int(num_classes)).to(dev)
    model._engine = None
    model.eval()
    return model


class HeadTrainer:
    """Trains `model.class_embed` (the Linear shared by the decoder layers) against the CTC loss with AdamW, everything on the device.

    The fp32 master copy of the head lives in one flat buffer (W row-major, then b) beside its AdamW moments; before every forward it is
    handed to the engine (DTLREngine.set_class_head), so the logits always come from the engine's own class-head path -- the 16-bit
    engines' hi + lo products, the f32s engine's split products -- on the current master weights.  The trunk is frozen: `cache` returns
    the decoder states and boxes of a batch, and `step_cached` trains on them without running the trunk again.

    Defaults are the reference's (config/Latin_CTC.py:5,14,18: lr 1e-5, weight_decay 1e-4, clip_max_norm 0.01; AdamW's own betas / eps).

    Two deviations from the reference's loop (engine.train_one_epoch_CTC):
      * the clip norm is taken over the head's gradient only.  The reference clips over model.parameters() (engine.py:213-214), trunk
        included, which needs a full backward that this package does not have;
      * `enc_out_class_embed` is kept as it is (finetuning.py:364-366 / 524-529, the non-smart branch): the two-stage selection keeps
        scoring with the pretrained head.
    `transformer.decoder.class_embed` and `enc_out_class_embed` get no gradient from this loss in the reference either, and AdamW skips
    parameters without one (no weight decay on them), so leaving them alone is not a deviation.

    step / step_cached return {"loss_CTC": 0-d fp32 CUDA tensor} -- the loss BEFORE the update, as the reference logs it; reading it is
    the caller's (only) host synchronisation.  max_norm None or <= 0: no clipping.

    loss: "ctc" (default: the above, unchanged), "set" or "ctc+set".  The set modes train against the reference's detection criterion
    (dtlr_amd/criterion.py: Hungarian matching of the main output against the line's character boxes, then the sigmoid focal loss):
    step / step_cached take `target_boxes` (per line [T,4] cxcywh in 0..1, one box a label) as well, the head's dlogits is
    CTC_loss_coef dCTC + cls_loss_coef dfocal (the coefficients of config/Latin_CTC.py:77,81, both 1), the matcher's costs are the
    reference's (set_cost_class 2, set_cost_bbox 5, set_cost_giou 2, focal_alpha 0.25), and the returned dict also carries loss_ce,
    loss_bbox, loss_giou, cardinality_error and class_error of the main output.  The matcher reads the solver's status: one host
    synchronisation a step.  A third deviation, in the set modes only:
      * the focal loss is taken on the main output only, because `return_hidden` returns the last decoder layer's states.  The
        reference also sums the auxiliary layers' and the intermediate output's loss_ce, which reach the shared head too."""

    def __init__(self, model, lr: float = 1e-5, weight_decay: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_norm: Optional[float] = 0.01, loss: str = "ctc", CTC_loss_coef: float = 1.0, cls_loss_coef: float = 1.0):
        if not model.dec_pred_class_embed_share:
            raise NotImplementedError("HeadTrainer: written for dec_pred_class_embed_share (every shipped config)")
        head = model.class_embed[0]
        if model.training:
            raise RuntimeError("HeadTrainer: call model.eval() -- the frozen trunk runs its inference forward")
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.max_norm = float(max_norm) if max_norm is not None else 0.0
        if loss not in ("ctc", "set", "ctc+set"):
            raise ValueError(f"HeadTrainer: loss {loss!r} is not one of ctc, set, ctc+set")
        self.loss, self.CTC_loss_coef, self.cls_loss_coef = loss, float(CTC_loss_coef), float(cls_loss_coef)
        self.matcher = None
        if loss != "ctc":
            from .criterion import HungarianMatcher
            self.matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, focal_alpha=0.25)
        self.C, self.D = int(head.weight.shape[0]), int(head.weight.shape[1])
        dev = head.weight.device
        n = self.C * self.D + self.C
        self.param = torch.cat([head.weight.detach().float().reshape(-1), head.bias.detach().float().reshape(-1)]).to(dev).contiguous()
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.scale = torch.ones(2, dtype=torch.float32, device=dev)         # (clip coefficient, gradient norm) of the last step
        self.step_count = 0
        self.last_outputs: Optional[Dict[str, torch.Tensor]] = None         # pred_logits / pred_boxes of the last step (before its update)

    # -- the master head ---------------------------------------------------------------------------------------------------------
    @property
    def weight(self) -> torch.Tensor:
        return self.param[: self.C * self.D].view(self.C, self.D)

    @property
    def bias(self) -> torch.Tensor:
        return self.param[self.C * self.D:]

    def _engine(self):
        eng = self.model.engine()
        eng.set_class_head(self.weight, self.bias)
        return eng

    # -- steps -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def cache(self, samples, per_line: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(hs [B,nq,hidden] in the engine's dtype, pred_boxes [B,nq,4]) of a batch: the frozen trunk's part of a step."""
        self._engine()
        out = self.model(samples, per_line=per_line, return_hidden=True)
        return out["hs"], out["pred_boxes"]

    @torch.no_grad()
    def step(self, samples, target_labels: Sequence[Sequence[int]], per_line: bool = False, target_boxes=None) -> Dict[str, torch.Tensor]:
        """One training step through the full forward (engine.train_one_epoch_CTC's loop body, engine.py:190-216)."""
        self._engine()
        out = self.model(samples, per_line=per_line, return_hidden=True)
        return self._update(out["pred_logits"], out["hs"], out["pred_boxes"], target_labels, target_boxes)

    @torch.no_grad()
    def step_cached(self, hs: torch.Tensor, boxes: torch.Tensor, target_labels: Sequence[Sequence[int]], target_boxes=None) -> Dict[str, torch.Tensor]:
        """The same step on cached decoder states: only the class head runs forward."""
        logits = self._engine()._class_head(hs)
        return self._update(logits, hs, boxes, target_labels, target_boxes)

    def _set_backward(self, logits, boxes, target_labels, target_boxes):
        """the main output's set losses and cls_loss_coef x the focal loss's gradient with respect to the logits"""
        if target_boxes is None:
            raise ValueError(f"HeadTrainer(loss={self.loss!r}): the step needs target_boxes")
        tg = ops.set_targets([{"labels": torch.as_tensor(l, dtype=torch.int64), "boxes": torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4)}
                              for l, b in zip(target_labels, target_boxes)], logits.device, self.C)
        match = self.matcher.match(logits, boxes, tg)
        r = ops.set_loss(logits, boxes, tg, match, max(float(sum(tg.sizes)), 1.0), [[self.cls_loss_coef, 0.0, 0.0]], [True], self.matcher.focal_alpha)
        v = r["losses"][0]
        return {"loss_ce": v[0], "loss_bbox": v[1], "loss_giou": v[2], "cardinality_error": v[5], "class_error": v[6]}, r["dlogits"][0]

    def _update(self, logits, hs, boxes, target_labels, target_boxes=None):
        self.last_outputs = {"pred_logits": logits, "pred_boxes": boxes}
        if self.loss == "ctc":
            loss, dlogits = E.loss_ctc_backward(self.last_outputs, target_labels)
            result = {"loss_CTC": loss}
        else:
            result, dlogits = self._set_backward(logits, boxes, target_labels, target_boxes)
            if self.loss == "ctc+set":
                loss, dctc = E.loss_ctc_backward(self.last_outputs, target_labels)
                dlogits.add_(dctc, alpha=self.CTC_loss_coef)
                result["loss_CTC"] = loss
        ops.head_grad(dlogits.view(-1, self.C), hs.reshape(-1, self.D), out=self.grad)
        clip = self.max_norm > 0
        if clip:
            ops.grad_norm_scale(self.grad, self.max_norm, out=self.scale)
        self.step_count += 1
        ops.adamw_step(self.param, self.exp_avg, self.exp_avg_sq, self.grad, self.step_count, self.lr, self.betas, self.eps,
                       self.weight_decay, grad_scale=self.scale if clip else None)
        return result

    # -- state -------------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict:
        return {"head": self.param.detach().cpu().clone(), "exp_avg": self.exp_avg.cpu().clone(), "exp_avg_sq": self.exp_avg_sq.cpu().clone(),
                "step": int(self.step_count), "num_classes": self.C, "hidden_dim": self.D}

    def load_state_dict(self, sd: Dict) -> None:
        if int(sd["num_classes"]) != self.C or int(sd["hidden_dim"]) != self.D:
            raise ValueError(f"HeadTrainer.load_state_dict: the state is of a Linear({sd['hidden_dim']} -> {sd['num_classes']}), "
                             f"this trainer's head is Linear({self.D} -> {self.C})")
        self.param.copy_(sd["head"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step"])

    @torch.no_grad()
    def write_back(self):
        """Copy the master head into model.class_embed (the shared Linear): model.state_dict() then is the adapted checkpoint."""
        head = self.model.class_embed[0]
        head.weight.copy_(self.weight)
        head.bias.copy_(self.bias)
        self.model._engine = None                                           # the packed model is rebuilt from the new parameters
        return self.model


# ------------------------------------------------------------------------------------------------------------------------- CLI
def build_parser() -> argparse.ArgumentParser:
    from .transforms import EVAL_MAX_SIZE, EVAL_SIZE
    ap = argparse.ArgumentParser(prog="python -m dtlr_amd.adapt",
                                 description="train the class head of a pretrained DTLR checkpoint for a new charset (CTC loss, AdamW), on the GPU")
    ap.add_argument("--config", default="latin", help="a reference config file (config/*.py) or a preset: latin | chinese | tiny")
    ap.add_argument("--weights", required=True, help="the pretrained checkpoint.pth")
    ap.add_argument("--images", required=True, help="folder with the line images (<id>.jpg / .png)")
    ap.add_argument("--labels", required=True, help="labels.pkl (reference layout), .json or .tsv")
    ap.add_argument("--mode", default="train", help="split of a labels.pkl")
    ap.add_argument("--charset", required=True, help="the NEW charset (.json list / .pkl list)")
    ap.add_argument("--old-charset", default=None, help="charset of the checkpoint (--smart-mapping; default: the package's default_charset.json)")
    ap.add_argument("--smart-mapping", action="store_true", help="initialise the new head from the old head's rows (finetuning.py --smart_mapping)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the head initialisation and of the batch order")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--epochs", type=int, default=None)
    g.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batching", default="exact", choices=["exact", "padded", "ragged"])
    ap.add_argument("--cache-features", action="store_true", help="run the frozen trunk once per batch and train on the cached decoder states")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32s", "f32"])
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--clip-max-norm", type=float, default=0.01, help="<= 0: no clipping")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--limit", type=int, default=0, help="train on the first N lines only")
    ap.add_argument("--size", type=int, default=EVAL_SIZE)
    ap.add_argument("--max_size", type=int, default=EVAL_MAX_SIZE)
    ap.add_argument("--loss", default="ctc", choices=["ctc", "set", "ctc+set"],
                    help="ctc: the CTC loss (default); set: Hungarian matching against character boxes + the focal loss; ctc+set: both")
    ap.add_argument("--boxes-from", default="labels", choices=["labels", "align"],
                    help="where the set loss's character boxes come from: labels = the --boxes file; align = the CTC forced alignment of "
                         "each transcript under the initial head (evaluation.align_ctc), lines without a feasible alignment are skipped")
    ap.add_argument("--boxes", default=None, help="JSON {image id: [[cx, cy, w, h], ...]}: one box a character, normalised to 0..1 (--boxes-from labels)")
    ap.add_argument("--out", required=True, help="the adapted checkpoint ({'model': state_dict, 'charset', 'trainer'})")
    return ap


def text_to_labels(text: str, charset: Sequence) -> List[int]:
    index = {ch: i for i, ch in reversed(list(enumerate(charset)))}
    try:
        return [index[ch] for ch in text]
    except KeyError as e:
        raise ValueError(f"character {e.args[0]!r} of a transcription is not in the charset") from None


def save_checkpoint(path: str, model, charset: Sequence, trainer: Optional[HeadTrainer] = None) -> None:
    ck = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "charset": list(charset)}
    if trainer is not None:
        ck["trainer"] = trainer.state_dict()
    torch.save(ck, path)


def load_char_boxes(args, trainer: HeadTrainer, rows, labels, batches, load_batch, per_line: bool):
    """The set loss's targets: line index -> [T,4] cxcywh boxes in 0..1, one a label, and the batches without the lines that have none.
    --boxes-from labels: the --boxes file.  --boxes-from align: the forced alignment of each transcript on the forward under the
    initial head (evaluation.align_ctc_records); a line whose transcript does not fit is skipped, the count goes to the log."""
    boxes: Dict[int, torch.Tensor] = {}
    if args.boxes_from == "labels":
        import json
        if not args.boxes:
            raise SystemExit("--loss set / ctc+set with --boxes-from labels needs --boxes")
        with open(args.boxes, encoding="utf-8") as f:
            table = json.load(f)
        for i, (name, _) in enumerate(rows):
            b = torch.as_tensor(table[name], dtype=torch.float32).reshape(-1, 4)
            if b.shape[0] != len(labels[i]):
                raise SystemExit(f"--boxes: {name} has {b.shape[0]} boxes for {len(labels[i])} characters")
            boxes[i] = b
        return boxes, batches
    skipped = 0
    trainer._engine()
    for idx in batches:
        with torch.no_grad():
            out = trainer.model(load_batch(idx), per_line=per_line)
        rec = E.align_ctc_records(out, [labels[i] for i in idx])
        lengths, xyxy = rec["lengths"].cpu().tolist(), rec["box"].cpu()
        for k, i in enumerate(idx):
            if lengths[k] < 0:
                skipped += 1
                continue
            b = xyxy[k, : lengths[k]]
            boxes[i] = torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], dim=1)
    print(f"--boxes-from align: {skipped} of {len(rows)} lines have no feasible alignment and are skipped", flush=True)
    kept = [[i for i in idx if i in boxes] for idx in batches]
    return boxes, [idx for idx in kept if idx]


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    args = build_parser().parse_args(argv)
    from . import eval_harness as H
    from . import weights as W
    from .config import DTLRConfig
    from .dino import DINO
    from .transforms import EvalTransform
    if not torch.cuda.is_available():
        raise SystemExit("dtlr_amd.adapt needs an MI355X (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    charset = H.load_charset(args.charset)
    sd = W.load_checkpoint_state_dict(args.weights)
    n_old = W.num_classes_of(sd)
    if args.config in ("latin", "chinese"):
        cfg = {"latin": DTLRConfig.latin, "chinese": DTLRConfig.chinese}[args.config]()
    elif args.config == "tiny":
        cfg = DTLRConfig.tiny(num_classes=n_old)
    else:
        cfg = DTLRConfig.from_reference_file(args.config)
    model = DINO(cfg, compute_dtype={"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32s": "f32s"}[args.dtype])
    model = E.load_model(model, sd, device=dev, new_class_embedding=n_old != cfg.num_classes, charset_size=n_old, fix_enc_out_class=True)
    torch.manual_seed(args.seed)
    if args.smart_mapping:
        w0, b0 = smart_mapping_init(model.class_embed[0], H.load_charset(args.old_charset), charset, args.seed)
        new_class_head(model, len(charset), w0, b0)
    else:
        new_class_head(model, len(charset))
    trainer = HeadTrainer(model, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm, loss=args.loss)

    rows = H.load_labels(args.labels, args.mode)
    if args.limit:
        rows = rows[: args.limit]
    paths = [H.find_image(args.images, name) for name, _ in rows]
    labels = [text_to_labels(t, charset) for _, t in rows]
    sizes = [H.image_size(p) for p in paths]
    per_line = args.batching == "ragged"
    batches = H.plan_batches(sizes, args.batch, args.batching == "exact", args.size, args.max_size)
    tf = EvalTransform(args.size, args.max_size)
    char_boxes: Dict[int, torch.Tensor] = {}
    if args.loss != "ctc":
        char_boxes, batches = load_char_boxes(args, trainer, rows, labels, batches, lambda idx: tf([H.read_rgb(paths[i]) for i in idx], device=dev),
                                              per_line)
    total = args.max_steps if args.max_steps is not None else (args.epochs if args.epochs is not None else 1) * len(batches)
    rng = np.random.Generator(np.random.PCG64(args.seed))
    cached: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
    step, last = 0, {}
    while step < total:
        for bi in rng.permutation(len(batches)):
            if step >= total:
                break
            idx = batches[int(bi)]
            tl = [labels[i] for i in idx]
            tb = [char_boxes[i] for i in idx] if args.loss != "ctc" else None
            if args.cache_features:
                if int(bi) not in cached:
                    cached[int(bi)] = trainer.cache(tf([H.read_rgb(paths[i]) for i in idx], device=dev), per_line=per_line)
                r = trainer.step_cached(*cached[int(bi)], tl, tb)
            else:
                r = trainer.step(tf([H.read_rgb(paths[i]) for i in idx], device=dev), tl, per_line=per_line, target_boxes=tb)
            step += 1
            if step % max(args.log_every, 1) == 0 or step == total:
                ev = E.evaluate_ctc_step(trainer.last_outputs, tl)            # the batch's loss and CER before this step's update
                last = {"step": step, **{k: float(v.item()) for k, v in r.items()}, "cer": ev["cer_sum"] / max(ev["n"], 1)}
                shown = "  ".join(f"{k} {last[k]:.6f}" for k in ("loss_CTC", "loss_ce") if k in last)
                print(f"step {step}/{total}  {shown}  train CER {last['cer']:.4f}", flush=True)
    trainer.write_back()
    save_checkpoint(args.out, model, charset, trainer)
    print(f"wrote {args.out}", file=sys.stderr)
    return last


if __name__ == "__main__":
    main()
