"""The operators of the seventh C header, include/dtlr_setloss.h (the set criterion: matching cost, Hungarian assignment, focal / L1 /
GIoU losses and gradients), over the launch seam of dtlr_amd/_lib.py: `_lib.launch` / `_lib.query` name each
symbol once, `@_lib.op` scopes a call to the device of its first tensor.  dtlr_amd/ops.py serves these functions under its own name too
(ops.set_cost, ops.hungarian, ops.set_loss, ops.set_targets); dtlr_amd/criterion.py builds the reference's HungarianMatcher and
SetCriterion on them."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib

SET_COST_MAX_TARGETS = 2048                # targets a line dtlr_set_cost takes
LOSS_COLUMNS = ("loss_ce", "loss_bbox", "loss_giou", "loss_xy", "loss_hw", "cardinality_error", "class_error", "n_matched")


class SetTargets(NamedTuple):
    """the targets of B lines as the kernels read them: labels [n] int32, offsets [B + 1] int32, tboxes [n,4] fp32 on the device; sizes:
    the B target counts (host list); Tmax = max(sizes, 1)"""
    labels: torch.Tensor
    offsets: torch.Tensor
    tboxes: torch.Tensor
    sizes: List[int]
    Tmax: int


def set_targets(targets: Sequence[Dict], device, num_classes: Optional[int] = None) -> SetTargets:
    """The reference's list of {"labels": [T] int, "boxes": [T,4] cxcywh} -> SetTargets on `device` (one host-to-device copy each).
    ValueError for a label outside [0, num_classes), unequal counts, or more than SET_COST_MAX_TARGETS targets on a line."""
    labels, boxes, sizes = [], [], []
    for k, t in enumerate(targets):
        lab = torch.as_tensor(t["labels"]).detach().reshape(-1).cpu().to(torch.int64)
        box = torch.as_tensor(t["boxes"]).detach().cpu().to(torch.float32).reshape(-1, 4)
        if lab.numel() != box.shape[0]:
            raise ValueError(f"set_targets: line {k} has {lab.numel()} labels and {box.shape[0]} boxes")
        if lab.numel() and (int(lab.min()) < 0 or (num_classes is not None and int(lab.max()) >= num_classes)):
            raise ValueError(f"set_targets: line {k} holds a label outside 0..{num_classes - 1 if num_classes else '?'}")
        if lab.numel() > SET_COST_MAX_TARGETS:
            raise ValueError(f"set_targets: line {k} has {lab.numel()} targets, the limit is {SET_COST_MAX_TARGETS}")
        labels.append(lab)
        boxes.append(box)
        sizes.append(int(lab.numel()))
    off = np.zeros(len(sizes) + 1, dtype=np.int32)
    np.cumsum(np.asarray(sizes, dtype=np.int64), out=off[1:])
    lab = torch.cat(labels).to(torch.int32) if labels else torch.zeros(0, dtype=torch.int32)
    box = torch.cat(boxes) if boxes else torch.zeros((0, 4), dtype=torch.float32)
    return SetTargets(lab.to(device), torch.from_numpy(off).to(device), box.contiguous().to(device), sizes, max(max(sizes, default=0), 1))


def _stacked(logits, boxes):
    if not logits.is_cuda or not boxes.is_cuda or logits.device != boxes.device:
        raise RuntimeError(f"dtlr_amd: the set criterion runs on one GPU (no CPU path; got {logits.device} and {boxes.device})")
    if logits.dim() == 3:
        logits, boxes = logits[None], boxes[None]
    if logits.dim() != 4 or boxes.dim() != 4 or boxes.shape[-1] != 4 or tuple(boxes.shape[:3]) != tuple(logits.shape[:3]):
        raise ValueError(f"set criterion: logits {tuple(logits.shape)} against boxes {tuple(boxes.shape)}")
    return logits.float().contiguous(), boxes.float().contiguous()


def _check_targets(tg: SetTargets, B: int, device):
    if len(tg.sizes) != B or tg.offsets.numel() != B + 1:
        raise ValueError(f"set criterion: {len(tg.sizes)} target lists for {B} lines")
    for t in (tg.labels, tg.offsets, tg.tboxes):
        if t.device != device:
            raise RuntimeError(f"dtlr_amd: the targets live on {t.device}, the outputs on {device}")
    assert tg.labels.dtype == torch.int32 and tg.offsets.dtype == torch.int32 and tg.tboxes.dtype == torch.float32
    assert tg.Tmax >= max(max(tg.sizes, default=0), 1) and tg.tboxes.shape[0] == tg.labels.numel() == sum(tg.sizes)


@_lib.op
def set_cost(logits, boxes, tg: SetTargets, cost_class: float = 2.0, cost_bbox: float = 5.0, cost_giou: float = 2.0, alpha: float = 0.25):
    """dtlr_set_cost: logits [L,B,nq,C] (or [B,nq,C]: L = 1), boxes [.., nq, 4] cxcywh, the lines' targets -> cost [L B, Tmax, nq] fp32,
    target-major: each line against its own targets only.  Rows past a line's target count are zeros."""
    logits, boxes = _stacked(logits, boxes)
    L, B, nq, C = logits.shape
    _check_targets(tg, B, logits.device)
    cost = torch.empty((L * B, tg.Tmax, nq), dtype=torch.float32, device=logits.device)
    n = int(tg.labels.numel())
    _lib.launch(_lib.lib(), "dtlr_set_cost", logits.data_ptr(), boxes.data_ptr(), tg.labels.data_ptr() if n else None, tg.offsets.data_ptr(),
                tg.tboxes.data_ptr() if n else None, n, L, B, nq, C, tg.Tmax, float(cost_class), float(cost_bbox), float(cost_giou), float(alpha),
                cost.data_ptr())
    return cost


@_lib.op
def hungarian(cost, sizes, threads: int = 0, check: bool = True):
    """dtlr_hungarian: the minimum-cost assignment of a batch of rectangular blocks.  cost [P,Rmax,ncols] fp32 on the GPU; sizes: the
    rows each problem uses ([P] ints or an int32 tensor) -> (match [P,Rmax] int32: the column of each row, -1 for padding and for rows
    left out when a problem has more rows than columns; status [P] int32: 0, -1 non-finite costs, -2 a loop bound exhausted).
    check (default): read status back and raise ValueError naming the first problem that was not solved; check=False leaves both on the
    device unsynchronised.  threads: 0 (the library's default, 1024), 256 or 1024 threads a problem."""
    if not cost.is_cuda:
        raise RuntimeError(f"dtlr_amd: the cost blocks must live on a GPU (no CPU path; got {cost.device})")
    if cost.dim() != 3 or cost.dtype != torch.float32:
        raise ValueError(f"hungarian: cost must be [P, rows, columns] fp32, got {tuple(cost.shape)} {cost.dtype}")
    cost = cost.contiguous()
    P, Rmax, ncols = cost.shape
    sizes = torch.as_tensor(sizes, dtype=torch.int32).reshape(-1).to(cost.device)
    if sizes.numel() != P:
        raise ValueError(f"hungarian: {sizes.numel()} sizes for {P} problems")
    match = torch.empty((P, Rmax), dtype=torch.int32, device=cost.device)
    status = torch.empty((P,), dtype=torch.int32, device=cost.device)
    if P == 0 or Rmax == 0 or ncols == 0:
        match.fill_(-1)
        status.zero_()
        return match, status
    _lib.launch(_lib.lib(), "dtlr_hungarian", cost.data_ptr(), sizes.data_ptr(), P, Rmax, ncols, int(threads), match.data_ptr(), status.data_ptr())
    if check:
        st = status.cpu()
        if bool((st != 0).any()):
            p = int(torch.nonzero(st)[0])
            raise ValueError(f"hungarian: problem {p} " + ("holds a non-finite cost" if int(st[p]) == -1 else "exhausted the solver's loop bound")
                             + f" (status {int(st[p])}; {int((st != 0).sum())} of {P} problems not solved)")
    return match, status


@_lib.op
def set_loss(logits, boxes, tg: SetTargets, match_q, num_boxes: float, weights, want_dlogits=None, alpha: float = 0.25):
    """dtlr_set_loss: losses and gradients given the assignment.  logits [L,B,nq,C] (or [B,nq,C]), boxes, the targets, match_q
    [L B, Tmax] int32 (hungarian's match over set_cost's block), num_boxes > 0, weights [L,3] = (w_ce, w_bbox, w_giou) per output (a
    tensor or nested list) -> {"losses": [L,8] fp32 in LOSS_COLUMNS order, "dboxes": [L,B,nq,4] fp32, "dlogits": a list of L entries,
    [B,nq,C] fp32 for the outputs named by want_dlogits (a list of L flags; default: all) and None for the others -- those take no
    memory}.  The gradients are those of sum_l (w_ce loss_ce + w_bbox loss_bbox + w_giou loss_giou)."""
    logits, boxes = _stacked(logits, boxes)
    L, B, nq, C = logits.shape
    dev = logits.device
    _check_targets(tg, B, dev)
    assert match_q.dtype == torch.int32 and match_q.device == dev and tuple(match_q.shape) == (L * B, tg.Tmax)
    match_q = match_q.contiguous()
    if not float(num_boxes) > 0:
        raise ValueError(f"set_loss: num_boxes {num_boxes}")
    w = torch.as_tensor(weights, dtype=torch.float32).to(dev).reshape(L, 3).contiguous()
    want = [True] * L if want_dlogits is None else [bool(f) for f in want_dlogits]
    assert len(want) == L
    slots, n_slots = [], 0
    for f in want:
        slots.append(n_slots if f else -1)
        n_slots += f
    slot = torch.tensor(slots, dtype=torch.int32).to(dev)
    dlogits = torch.empty((n_slots, B, nq, C), dtype=torch.float32, device=dev) if n_slots else None
    dboxes = torch.empty((L, B, nq, 4), dtype=torch.float32, device=dev)
    losses = torch.empty((L, 8), dtype=torch.float32, device=dev)
    L_ = _lib.lib()
    ws = torch.empty((_lib.query(L_, "dtlr_set_loss_workspace_bytes", L, B, nq) // 8,), dtype=torch.float64, device=dev)
    n = int(tg.labels.numel())
    _lib.launch(L_, "dtlr_set_loss", logits.data_ptr(), boxes.data_ptr(), tg.labels.data_ptr() if n else None, tg.offsets.data_ptr(),
                tg.tboxes.data_ptr() if n else None, n, match_q.data_ptr(), L, B, nq, C, tg.Tmax, float(alpha), float(num_boxes), w.data_ptr(),
                slot.data_ptr(), dlogits.data_ptr() if n_slots else None, dboxes.data_ptr(), losses.data_ptr(), ws.data_ptr())
    return {"losses": losses, "dboxes": dboxes, "dlogits": [dlogits[s] if s >= 0 else None for s in slots]}
