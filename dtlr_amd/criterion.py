"""The reference's training criterion on the device: HungarianMatcher (models/dino/matcher.py) and SetCriterion.forward_standard
(models/dino/dino.py:780-964: loss_labels, loss_boxes, loss_cardinality over the main, auxiliary and intermediate outputs), under the
reference's names and constructor arguments, on the three operators of include/dtlr_setloss.h.

What the reference does per output -- a [B nq, sum T] cost matrix, its copy to the host, scipy's linear_sum_assignment per line -- is here
one launch of dtlr_set_cost (each line against its own targets only), one of dtlr_hungarian (a workgroup a line and output) and one of
dtlr_set_loss for ALL outputs together; the only host synchronisation is reading the solver's status (and, for HungarianMatcher.forward,
the indices it returns).

Not built: the denoising losses (`*_dn`: NotImplementedError for a dn_meta with known boxes; the reference's zero-valued `*_dn` entries
are left out), masks, `enc_outputs`, and loss_CTC (dtlr_amd/evaluation.py has it)."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
from torch import nn

from . import ops
from .setloss import LOSS_COLUMNS, SetTargets


class HungarianMatcher(nn.Module):
    """models/dino/matcher.py HungarianMatcher: the assignment between each line's targets and the queries of ONE output that minimises
    cost_bbox L1 + cost_class (focal class cost) + cost_giou (-GIoU).  The cost is evaluated in fp64 from the fp32 outputs (the reference:
    in fp32), the assignment is the solver's own optimum over it: where two assignments differ by less than the cost's rounding, this
    matcher and the reference may return either."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, focal_alpha: float = 0.25):
        super().__init__()
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha = cost_class, cost_bbox, cost_giou, focal_alpha

    @torch.no_grad()
    def match(self, logits, boxes, tg: SetTargets, threads: int = 0):
        """logits [L,B,nq,C] (or [B,nq,C]), boxes, packed targets (ops.set_targets) -> match_q [L B, Tmax] int32 on the device: the
        query matched to target t, -1 for padding and for targets left out when a line has more targets than queries.  ValueError when
        a line's cost block holds a non-finite value."""
        cost = ops.set_cost(logits, boxes, tg, self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha)
        L = cost.shape[0] // len(tg.sizes)
        match, _ = ops.hungarian(cost, tg.sizes * L, threads=threads, check=True)
        return match

    @torch.no_grad()
    def forward(self, outputs, targets) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """The reference's result: per line (index_i, index_j), int64 CPU tensors -- the matched queries in ascending order and their
        targets; min(nq, T) pairs."""
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        tg = ops.set_targets(targets, logits.device, logits.shape[-1])
        return indices_of(self.match(logits, boxes, tg).cpu(), tg.sizes)


def indices_of(match_q, sizes: Sequence[int]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """rows of match_q (CPU, one per line) -> the reference's (index_i, index_j) pairs"""
    out = []
    for b, T in enumerate(sizes):
        q = match_q[b, :T].to(torch.int64)
        t = torch.nonzero(q >= 0).reshape(-1)
        order = torch.argsort(q[t])
        out.append((q[t][order], t[order]))
    return out


class _SetLoss(torch.autograd.Function):
    """losses [L,8] of the stacked outputs; differentiable in columns 0..2 (loss_ce, loss_bbox, loss_giou) with respect to every output's
    logits and boxes.  backward runs dtlr_set_loss once more with the incoming gradient's columns 0..2 as the weights -- a device
    tensor, no synchronisation -- so any weighting of the returned values gets its exact gradient; only the outputs whose logits need a
    gradient get a dlogits slice."""

    @staticmethod
    def forward(ctx, state, *tensors):
        L = len(tensors) // 2
        logits = torch.stack([t.float() for t in tensors[:L]])
        boxes = torch.stack([t.float() for t in tensors[L:]])
        ctx.state, ctx.L = state, L
        ctx.save_for_backward(logits, boxes)
        r = ops.set_loss(logits, boxes, state["tg"], state["match"], state["num_boxes"], [[0.0, 0.0, 0.0]] * L, [False] * L, state["alpha"])
        return r["losses"]

    @staticmethod
    def backward(ctx, grad):
        logits, boxes = ctx.saved_tensors
        L, st = ctx.L, ctx.state
        want = [bool(f) for f in ctx.needs_input_grad[1:1 + L]]
        r = ops.set_loss(logits, boxes, st["tg"], st["match"], st["num_boxes"], grad[:, :3].float().contiguous(), want, st["alpha"])
        dl = [g if f else None for g, f in zip(r["dlogits"], want)]
        db = [r["dboxes"][l] if ctx.needs_input_grad[1 + L + l] else None for l in range(L)]
        return (None, *dl, *db)


class SetCriterion(nn.Module):
    """models/dino/dino.py SetCriterion, forward_standard: every output (main, aux_outputs, interm_outputs) is matched separately
    against the targets and contributes loss_labels (sigmoid focal), loss_boxes (L1, GIoU; loss_xy / loss_hw for logging) and
    loss_cardinality under the reference's keys: loss_ce, loss_bbox, loss_giou, loss_xy, loss_hw, cardinality_error, class_error (main
    output only), with the suffixes _0.._4 and _interm.  The values are differentiable: `sum(weight_dict[k] * losses[k])` and
    `.backward()` deliver the gradients to the outputs' logits and boxes (those that require one)."""

    def __init__(self, num_classes, matcher, weight_dict, focal_alpha, losses=("labels", "boxes", "cardinality")):
        super().__init__()
        for name in losses:
            if name not in ("labels", "boxes", "cardinality"):
                raise NotImplementedError(f"SetCriterion: the loss {name!r} is not built (labels, boxes, cardinality are)")
        self.num_classes, self.matcher, self.weight_dict, self.focal_alpha, self.losses = num_classes, matcher, weight_dict, focal_alpha, list(losses)

    @staticmethod
    def stacked_outputs(outputs) -> List[Tuple[str, Dict]]:
        """(key suffix, output) in the reference's order: main, aux_outputs 0.., interm_outputs"""
        if "enc_outputs" in outputs:
            raise NotImplementedError("SetCriterion: enc_outputs are not built")
        dn = outputs.get("dn_meta")
        if dn and "output_known_lbs_bboxes" in dn:
            raise NotImplementedError("SetCriterion: the denoising losses (dn_meta with known labels and boxes) are not built")
        outs = [("", outputs)]
        outs += [(f"_{i}", o) for i, o in enumerate(outputs.get("aux_outputs", []))]
        if "interm_outputs" in outputs:
            outs.append(("_interm", outputs["interm_outputs"]))
        return outs

    @staticmethod
    def num_boxes_of(sizes, device) -> float:
        """max(sum T / world size, 1), summed over the ranks when a process group is up"""
        n = float(sum(sizes))
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            t = torch.tensor([n], dtype=torch.float32, device=device)
            torch.distributed.all_reduce(t)
            n = float(t.item()) / torch.distributed.get_world_size()
        return max(n, 1.0)

    def forward(self, outputs, targets, return_indices: bool = False):
        outs = self.stacked_outputs(outputs)
        logits = [o["pred_logits"] for _, o in outs]
        boxes = [o["pred_boxes"] for _, o in outs]
        dev = logits[0].device
        tg = ops.set_targets(targets, dev, logits[0].shape[-1])
        with torch.no_grad():
            match = self.matcher.match(torch.stack([t.detach().float() for t in logits]), torch.stack([t.detach().float() for t in boxes]), tg)
        state = {"tg": tg, "match": match, "num_boxes": self.num_boxes_of(tg.sizes, dev), "alpha": self.focal_alpha}
        values = _SetLoss.apply(state, *logits, *boxes)
        col = {k: i for i, k in enumerate(LOSS_COLUMNS)}
        losses = {}
        for l, (suffix, _) in enumerate(outs):
            if "labels" in self.losses:
                losses["loss_ce" + suffix] = values[l, col["loss_ce"]]
                if not suffix:
                    losses["class_error"] = values[l, col["class_error"]].detach()
            if "cardinality" in self.losses:
                losses["cardinality_error" + suffix] = values[l, col["cardinality_error"]].detach()
            if "boxes" in self.losses:
                losses["loss_bbox" + suffix] = values[l, col["loss_bbox"]]
                losses["loss_giou" + suffix] = values[l, col["loss_giou"]]
                losses["loss_xy" + suffix] = values[l, col["loss_xy"]].detach()
                losses["loss_hw" + suffix] = values[l, col["loss_hw"]].detach()
        if return_indices:
            B = len(tg.sizes)
            m = match.cpu()
            per = [indices_of(m[l * B:(l + 1) * B], tg.sizes) for l in range(len(outs))]
            return losses, per[1:] + per[:1]                       # the reference's order: the auxiliary outputs, then the main one
        return losses
