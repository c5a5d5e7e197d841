"""CPU yardsticks of the last decoder layer's self-attention gradient with everything below it frozen (csrc/self_grad.hip,
dtlr_amd/adapt.py).

      t, p --in_proj--> Q, K (of t + p), V (of t) --softmax(Q K^T / sqrt(32)) V per head--> a --out_proj--> + t --norm2--> s --> the cross block (cross_grad_ref)

  mha                           the attention core in torch, in the dtype of its inputs (heads are channel slices of 32)
  mha_grads / mha_grads_closed  the operator alone: (dq, dk, dv) by autograd / by the closed form the kernels implement
  block                         the restatement of the block: t, p are constants of the frozen trunk
  block_grads / block_grads_closed   the six self gradients of <s, ds> by autograd / by hand
  chain_grads                   autograd's gradient of seeded cotangents on every output with respect to the six self, the eight cross and
                                the eight tail tensors, in the dtype asked for
  chain_grads_at                the same in the trainer's convention (the engine's h_l are inputs of the heads' gradients)
  bound / report                the rule of DESIGN section 20 (tail_grad_ref's)
"""
import math

import torch

from tests import box_grad_ref as RB
from tests import cross_grad_ref as RC
from tests import tail_grad_ref as RT

D, HEADS, HD = 256, 8, 32
NAMES = ("in_proj_W", "in_proj_b", "out_proj_W", "out_proj_b", "norm2_w", "norm2_b")
SHAPES = ((768, 256), (768,), (256, 256), (256,), (256,), (256,))
bound, report, U = RT.bound, RT.report, RT.U


def flat(grads):
    return torch.cat([g.reshape(-1) for g in grads])


def unflat(v):
    out, o = [], 0
    for s in SHAPES:
        k = s[0] * (s[1] if len(s) > 1 else 1)
        out.append(v[o:o + k].view(s))
        o += k
    assert o == v.numel()
    return out


def _heads(x, H):
    B, L, C = x.shape
    return x.view(B, L, H, C // H).transpose(1, 2)                  # [B,H,L,hd]


def mha(q, k, v, H=HEADS):
    """q, k, v [B,L,H*hd] -> softmax(q k^T / sqrt(hd)) v per head, heads side by side [B,L,H*hd]"""
    B, L, C = q.shape
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    P = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(C // H), -1)
    return (P @ vh).transpose(1, 2).reshape(B, L, C)


def mha_grads(q, k, v, g, dtype, H=HEADS):
    """(dq, dk, dv) of <mha(q, k, v), g> by autograd in `dtype`"""
    q, k, v = [x.detach().to(dtype).requires_grad_(True) for x in (q, k, v)]
    return list(torch.autograd.grad((mha(q, k, v, H) * g.detach().to(dtype)).sum(), [q, k, v]))


def mha_grads_closed(q, k, v, g, H=HEADS):
    """(dq, dk, dv) by hand, in the inputs' dtype: dV = P^T dO, dP = dO V^T, Delta = <dO, O>, dS = P o (dP - Delta), dQ = dS K / sqrt(hd),
    dK = dS^T Q / sqrt(hd)"""
    B, L, C = q.shape
    sc = 1 / math.sqrt(C // H)
    qh, kh, vh, gh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(g, H)
    P = torch.softmax(qh @ kh.transpose(-1, -2) * sc, -1)
    dP = gh @ vh.transpose(-1, -2)
    delta = (gh * (P @ vh)).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    back = lambda x: x.transpose(1, 2).reshape(B, L, C)
    return [back(dS @ kh * sc), back(dS.transpose(-1, -2) @ qh * sc), back(P.transpose(-1, -2) @ gh)]


def block(t, p, sp):
    """the self-attention block: t, p [B,nq,256], sp: the six tensors in NAMES' order -> dict(x, qkv, a, x0, s), rows flattened to M = B nq"""
    Win, bin_, Wo, bo, g2, b2 = sp
    x = t + p
    qk = x @ Win[:2 * D].t() + bin_[:2 * D]
    v = t @ Win[2 * D:].t() + bin_[2 * D:]
    a = mha(qk[..., :D], qk[..., D:], v)
    x0 = t + a @ Wo.t() + bo
    s = RT.ln(x0, g2, b2)
    return {"x": x.reshape(-1, D), "qkv": torch.cat([qk, v], -1).reshape(-1, 3 * D), "a": a.reshape(-1, D), "x0": x0.reshape(-1, D), "s": s.reshape(-1, D)}


def block_grads(t, p, sp, ds, dtype):
    """the six gradients of <s, ds> by autograd in `dtype`"""
    c = lambda v: v.detach().to(dtype)
    sp = [c(w).requires_grad_(True) for w in sp]
    return list(torch.autograd.grad((block(c(t), c(p), sp)["s"] * c(ds).reshape(-1, D)).sum(), sp))


def block_grads_closed(t, p, sp, ds):
    """the closed form of block_grads, no autograd: fp64"""
    d = lambda v: v.detach().double()
    t, p, ds = d(t), d(p), d(ds).reshape(-1, D)
    Win, bin_, Wo, bo, g2, b2 = [d(w) for w in sp]
    B, nq = t.shape[:2]
    f = block(t, p, [Win, bin_, Wo, bo, g2, b2])
    dx0, dg2, db2 = RT.ln_backward(f["x0"], g2, ds)
    dbo, dWo, da = dx0.sum(0), dx0.t() @ f["a"], dx0 @ Wo
    qkv = f["qkv"].view(B, nq, 3 * D)
    dq, dk, dv = [g.reshape(-1, D) for g in mha_grads_closed(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], da.view(B, nq, D))]
    dW = torch.cat([dq.t() @ f["x"], dk.t() @ f["x"], dv.t() @ t.reshape(-1, D)])
    return [dW, torch.cat([dq.sum(0), dk.sum(0), dv.sum(0)]), dWo, dbo, dg2, db2]


def _cin(cin, s, dtype):
    """cross_grad_ref's block arguments with the state after norm2 replaced by the recomputed one"""
    _, p, R, V, shapes = RC._cin(cin, dtype)
    return s.view(p.shape), p, R, V, shapes


def chain_grads(sin, sp, cin, cross, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes, dtype, used=None):
    """autograd's gradient of sum_(l in used) <logits_l, cl_l> + <boxes_l, cb_l> with respect to the six self, the eight cross and the
    eight tail tensors, in `dtype`; sin: dict(t, qpos); cin: cross_grad_ref's dict, its "s" unused.  -> (self, cross, tail grads)"""
    c = lambda v: v.detach().to(dtype)
    sp = [c(w).requires_grad_(True) for w in sp]
    cross = [c(w).requires_grad_(True) for w in cross]
    tail = [c(w).requires_grad_(True) for w in tail]
    s = block(c(sin["t"]), c(sin["qpos"]), sp)["s"]
    u = RC.block(*_cin(cin, s, dtype), cross)["u"]
    logits, boxes, _, _ = RT.chain_outputs(u, [c(v) for v in t_below], [c(v) for v in refs], tail, c(Wc), c(bc), [c(w) for w in P])
    used = range(len(logits)) if used is None else used
    total = sum((logits[l] * c(cot_logits[l])).sum() + (boxes[l] * c(cot_boxes[l])).sum() for l in used)
    g = torch.autograd.grad(total, sp + cross + tail)
    return list(g[:6]), list(g[6:14]), list(g[14:])


def chain_grads_at(sin, sp, cin, cross, t_below, hs, tail, Wc, P, cot_logits, dz, dtype, used=None):
    """The trainer's convention (DESIGN sections 11, 22 .. 24): the heads' input gradients are taken AT the engine's h_l (hs), then the
    gradient of sum_l <decoder.norm(t_l), dh_l>, t_(L-1) recomputed from the layer's input, with respect to the self, cross and tail tensors."""
    c = lambda v: v.detach().to(dtype)
    L = len(t_below) + 1
    used = list(range(L)) if used is None else list(used)
    Wc_, P_ = c(Wc), [c(w) for w in P]
    dh = {}
    for l in used:
        h = c(hs[l]).requires_grad_(True)
        total = h.sum() * 0
        if cot_logits[l] is not None:
            total = total + ((h @ Wc_.t()) * c(cot_logits[l])).sum()
        if dz[l] is not None:
            total = total + (RB.mlp(h, P_) * c(dz[l])).sum()
        dh[l] = torch.autograd.grad(total, h)[0]
    sp = [c(w).requires_grad_(True) for w in sp]
    cross = [c(w).requires_grad_(True) for w in cross]
    tail = [c(w).requires_grad_(True) for w in tail]
    W1, b1, W2, b2, g3, be3, gd, bd = tail
    s = block(c(sin["t"]), c(sin["qpos"]), sp)["s"]
    u = RC.block(*_cin(cin, s, dtype), cross)["u"]
    t = [c(v) for v in t_below] + [RT.ln(RT.ffn(u, W1, b1, W2, b2)[1], g3, be3)]
    total = sum((RT.ln(t[l], gd, bd) * dh[l]).sum() for l in used)
    g = torch.autograd.grad(total, sp + cross + tail)
    return list(g[:6]), list(g[6:14]), list(g[14:])


# ---------------------------------------------------------------------------------------------------------------- cases
def self_params(seed):
    """a seeded block: projections that give scores of order one on states of order one, the norm's affine parameters away from 1 / 0"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g) * 2 - 1
    return [r(768, 256) / 8, r(768) / 4, r(256, 256) / 16, r(256) / 16, 1 + 0.3 * r(256), 0.2 * r(256)]


def mha_case(B, L, H, seed, qscale=1.0):
    """(q, k, v, g) [B,L,H*32] fp32, seeded; qscale stretches the scores"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn((B, L, H * HD), generator=gen)
    return r() * qscale, r(), r(), r()
