"""CPU yardsticks of the class-head adaptation tests (not a test module).

  restated_loss      differentiable PyTorch restatement of SetCriterion.loss_CTC (models/dino/dino.py:457-551), operation by operation:
                     stable sort by box cx, gather, sigmoid, blank channel by masked assignment, filler rows,
                     F.ctc_loss(blank=0, zero_infinity=True, reduction="mean") on the log.  Runs in the dtype of its inputs (fp32 / fp64).
  loss_and_grad      its value and torch.autograd's gradient with respect to the logits.
  hand_loss_and_grad NumPy fp64, no autograd: explicit alpha / beta recursions over the 2 nq frames and the closed-form gradient the
                     device kernels implement (csrc/ctc_grad.hip) -- the independent derivation the autograd result is checked against.
  adamw_numpy        NumPy fp64 AdamW (torch.optim.AdamW's update rule) with clip_grad_norm_'s coefficient.
  head_loop          the head-adaptation loop in CPU PyTorch (restated loss + torch.optim.AdamW) on given features.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F


def restated_loss(logits, boxes, labels, eps: float = 0.003, filler: float = 1e-5):
    B, nq, C = logits.shape
    _, idx = torch.sort(boxes[:, :, 0], stable=True)
    p = torch.gather(logits, 1, idx.unsqueeze(-1).expand(-1, -1, C)).sigmoid()
    new = torch.zeros((B, nq, C + 1), dtype=logits.dtype)
    new[:, :, 1:] = p
    mask = p.sum(-1) < 1 - eps
    new[:, :, 0][mask] = 1 - p[mask].sum(-1)
    mask = ~mask
    new[:, :, 0][mask] = eps
    new[:, :, 1:][mask] = (1 - eps) * p[mask] / p[mask].sum(-1).unsqueeze(-1)
    blank = torch.zeros_like(new) + filler
    blank[:, :, 0] = 1
    padded = torch.zeros((B, 2 * nq, C + 1), dtype=logits.dtype)
    padded[:, ::2, :] = new
    padded[:, 1::2, :] = blank
    lengths = torch.tensor([len(t) for t in labels], dtype=torch.int64)
    tt = torch.zeros((B, max([len(t) for t in labels] + [0])))
    for i, t in enumerate(labels):
        if len(t):
            tt[i, : len(t)] = torch.as_tensor([int(v) for v in t], dtype=tt.dtype) + 1
    return F.ctc_loss(torch.log(padded.permute(1, 0, 2)), tt, torch.full((B,), 2 * nq, dtype=torch.int64), lengths,
                      blank=0, reduction="mean", zero_infinity=True)


def loss_and_grad(logits, boxes, labels, dtype=torch.float64, eps: float = 0.003, filler: float = 1e-5):
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    loss = restated_loss(x, boxes.detach().to(dtype), labels, eps, filler)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def _lse(*a):
    m = max(a)
    if m == -math.inf:
        return -math.inf
    return m + math.log(sum(math.exp(v - m) for v in a))


def hand_loss_and_grad(logits, boxes, labels, eps: float = 0.003, filler: float = 1e-5):
    """fp64: (loss, dlogits [B,nq,C], per-line nll with inf -> 0)."""
    x = np.asarray(logits, dtype=np.float64)
    bx = np.asarray(boxes, dtype=np.float64)
    B, nq, C = x.shape
    grad = np.zeros_like(x)
    nlls = np.zeros(B)
    T = 2 * nq
    for b in range(B):
        lab = [int(v) + 1 for v in labels[b]]
        L = len(lab)
        ext = [0] * (2 * L + 1)
        ext[1::2] = lab
        S = len(ext)
        order = np.argsort(bx[b, :, 0], kind="stable")
        p = 1.0 / (1.0 + np.exp(-x[b, order]))                      # [nq, C], reading order
        s = p.sum(-1)
        low = s < 1 - eps
        y = np.empty((T, C + 1))
        y[0::2, 0] = np.where(low, 1 - s, eps)
        y[0::2, 1:] = np.where(low[:, None], p, (1 - eps) * p / s[:, None])
        y[1::2, 0] = 1.0
        y[1::2, 1:] = filler
        with np.errstate(divide="ignore"):
            ly = np.log(y)
        la = np.full((T, S), -math.inf)
        lb = np.full((T, S), -math.inf)
        la[0, 0] = ly[0, 0]
        if S > 1:
            la[0, 1] = ly[0, ext[1]]
        for t in range(1, T):
            for k in range(S):
                a = [la[t - 1, k]]
                if k >= 1:
                    a.append(la[t - 1, k - 1])
                if k >= 2 and ext[k] != 0 and ext[k] != ext[k - 2]:
                    a.append(la[t - 1, k - 2])
                la[t, k] = _lse(*a) + ly[t, ext[k]]
        lb[T - 1, S - 1] = ly[T - 1, ext[S - 1]]
        if S > 1:
            lb[T - 1, S - 2] = ly[T - 1, ext[S - 2]]
        for t in range(T - 2, -1, -1):
            for k in range(S):
                a = [lb[t + 1, k]]
                if k + 1 < S:
                    a.append(lb[t + 1, k + 1])
                if k + 2 < S and ext[k] != 0 and ext[k] != ext[k + 2]:
                    a.append(lb[t + 1, k + 2])
                lb[t, k] = _lse(*a) + ly[t, ext[k]]
        logP = _lse(la[T - 1, S - 1], la[T - 1, S - 2]) if S > 1 else la[T - 1, S - 1]
        if logP == -math.inf:
            continue                                                # zero_infinity: loss 0, gradient 0
        nlls[b] = -logP
        scale = 1.0 / (B * max(L, 1))
        for r in range(nq):
            t = 2 * r
            om = np.zeros(C + 1)                                    # posterior occupancy of every channel at this frame
            for k in range(S):
                if la[t, k] > -math.inf and lb[t, k] > -math.inf:
                    om[ext[k]] += math.exp(la[t, k] + lb[t, k] - ly[t, ext[k]] - logP)
            pr = p[r]
            coef = om[0] / (1 - s[r]) if low[r] else (1 - om[0]) / s[r]
            grad[b, order[r]] = scale * (1 - pr) * (pr * coef - om[1:])
    loss = float(np.mean([nlls[b] / max(len(labels[b]), 1) for b in range(B)]))
    return loss, grad, nlls


def adamw_numpy(p, m, v, g, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0):
    """One AdamW step in fp64, in place on p, m, v (NumPy float64 arrays); g is clipped by clip_grad_norm_'s coefficient first."""
    g = np.asarray(g, dtype=np.float64)
    if max_norm > 0:
        g = g * min(1.0, max_norm / (math.sqrt(float((g * g).sum())) + 1e-6))
    b1, b2 = betas
    p *= 1 - lr * weight_decay
    m += (g - m) * (1 - b1)
    v *= b2
    v += (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p -= (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p


def head_loop(hs, boxes, labels, W0, b0, steps, dtype, lr, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=0.0,
              record=None):
    """The adaptation loop in CPU PyTorch on fixed features hs [B,nq,D]: logits = hs W^T + b, restated loss, clip_grad_norm_,
    torch.optim.AdamW.  Returns (W, b, losses) in `dtype`; record(step, W, b) is called after every step when given."""
    hs = hs.detach().to(dtype)
    boxes = boxes.detach().to(dtype)
    W = torch.nn.Parameter(W0.detach().to(dtype).clone())
    b = torch.nn.Parameter(b0.detach().to(dtype).clone())
    opt = torch.optim.AdamW([W, b], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    losses = []
    for k in range(steps):
        opt.zero_grad()
        loss = restated_loss(hs @ W.t() + b, boxes, labels)
        loss.backward()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([W, b], max_norm)
        opt.step()
        losses.append(float(loss.detach()))
        if record is not None:
            record(k, W.detach(), b.detach())
    return W.detach(), b.detach(), losses
