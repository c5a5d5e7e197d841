"""CPU yardsticks of the decoder tail's gradient with the trunk frozen (csrc/tail_grad.hip, dtlr_amd/adapt.py).

      u --FFN(linear1, ReLU, linear2)--> + u --norm3--> t_(L-1) --decoder.norm--> h_(L-1) --class_embed / bbox_embed--> main output
      t_l (l < L - 1, constants) ----------------------------------decoder.norm--> h_l     --class_embed / bbox_embed--> output l

  chain_outputs / chain_grads   the restatement in torch: u, t_l (l < L - 1) and the reference points r_l are constants of the frozen
                                trunk; gradients of seeded cotangents with respect to the eight tail tensors by autograd in the dtype
                                asked for
  chain_grads_at                the same with the engine's h_l as inputs of the heads' gradients: what the trainer computes
  closed_grads                  the closed form the kernels implement, written out without autograd (fp64)
  ln_backward / ffn_grads_closed / box_dx_closed   its pieces ; ln_grads / ffn_grads / box_dx: the same by autograd
  ffn_case                      seeded inputs of the kernel tests, conditioned as the bound needs (no pre-activation near a ReLU's kink;
                                the box MLP's come from box_grad_ref.kernel_case)
  bound / report                the rule of DESIGN section 20: E <= max(4 E_cpu32, 16 * 2^-24 max|g|) per tensor
"""
import torch
import torch.nn.functional as Fn

from tests import box_grad_ref as RB

D = 256
LN_EPS = 1e-5
U = 2.0 ** -24
NAMES = ("W1", "b1", "W2", "b2", "norm3_w", "norm3_b", "dec_norm_w", "dec_norm_b")
KINK = 1e-4


def shapes(F):
    return ((F, D), (F,), (D, F), (D,), (D,), (D,), (D,), (D,))


def flat(grads):
    return torch.cat([g.reshape(-1) for g in grads])


def unflat(v, F):
    out, o = [], 0
    for s in shapes(F):
        k = 1
        for d in s:
            k *= d
        out.append(v[o:o + k].view(s))
        o += k
    assert o == v.numel()
    return out


def ln(x, w, b):
    return Fn.layer_norm(x, (D,), w, b, LN_EPS)


def ffn(u, W1, b1, W2, b2):
    """-> (a, y): linear1's pre-activation and the FFN block's output before norm3"""
    a = u @ W1.t() + b1
    return a, u + torch.relu(a) @ W2.t() + b2


def chain_outputs(u, t_below, refs, tail, Wc, bc, P):
    """logits and boxes of the L = len(t_below) + 1 decoder outputs.  u [M,256]; t_below: t_l, l < L - 1; refs: r_0 .. r_(L-1) [M,4];
    tail: the eight tensors in NAMES' order; Wc, bc: the class head; P: the box MLP (box_grad_ref)."""
    W1, b1, W2, b2, g3, be3, gd, bd = tail
    t = list(t_below) + [ln(ffn(u, W1, b1, W2, b2)[1], g3, be3)]
    h = [ln(x, gd, bd) for x in t]
    return [x @ Wc.t() + bc for x in h], [torch.sigmoid(RB.mlp(x, P) + RB.isg(r)) for x, r in zip(h, refs)], t, h


def chain_grads(u, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes, dtype, used=None):
    """autograd's gradient of sum_(l in used) <logits_l, cl_l> + <boxes_l, cb_l> with respect to the eight tail tensors, in `dtype`"""
    c = lambda v: v.detach().to(dtype)
    tail = [c(p).requires_grad_(True) for p in tail]
    logits, boxes, _, _ = chain_outputs(c(u), [c(v) for v in t_below], [c(v) for v in refs], tail, c(Wc), c(bc), [c(p) for p in P])
    used = range(len(logits)) if used is None else used
    total = sum((logits[l] * c(cot_logits[l])).sum() + (boxes[l] * c(cot_boxes[l])).sum() for l in used)
    return list(torch.autograd.grad(total, tail))


def chain_grads_at(u, t_below, hs, tail, Wc, P, cot_logits, dz, dtype, used=None):
    """The trainer's convention (DESIGN sections 11, 22): the engine's states are inputs.  The heads' input gradients are taken AT the
    engine's h_l (hs), with the box gradient dz_l given at the MLP's output:  dh_l = d/dh [<h Wc^T, cl_l> + <f(h), dz_l>] at h = hs[l];
    then the gradient of sum_l <decoder.norm(t_l), dh_l> with respect to the eight tail tensors, t_(L-1) recomputed from u.  By autograd
    in `dtype`.  cot_logits / dz: per output, None for a term that is absent."""
    c = lambda v: v.detach().to(dtype)
    L = len(t_below) + 1
    used = list(range(L)) if used is None else list(used)
    Wc, P = c(Wc), [c(p) for p in P]
    dh = {}
    for l in used:
        h = c(hs[l]).requires_grad_(True)
        total = h.sum() * 0
        if cot_logits[l] is not None:
            total = total + ((h @ Wc.t()) * c(cot_logits[l])).sum()
        if dz[l] is not None:
            total = total + (RB.mlp(h, P) * c(dz[l])).sum()
        dh[l] = torch.autograd.grad(total, h)[0]
    tail = [c(p).requires_grad_(True) for p in tail]
    W1, b1, W2, b2, g3, be3, gd, bd = tail
    t = [c(v) for v in t_below] + [ln(ffn(c(u), W1, b1, W2, b2)[1], g3, be3)]
    total = sum((ln(t[l], gd, bd) * dh[l]).sum() for l in used)
    return list(torch.autograd.grad(total, tail)), [dh[l] for l in used]


def ln_backward(x, gamma, g):
    """LayerNorm's backward by hand, in the inputs' dtype: (dx, dgamma, dbeta)"""
    mean = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    xhat = (x - mean) * rstd
    q = gamma * g
    dx = rstd * (q - q.mean(-1, keepdim=True) - xhat * (q * xhat).mean(-1, keepdim=True))
    return dx, (g * xhat).sum(0), g.sum(0)


def ffn_grads_closed(u, W1, b1, W2, dy):
    """(dW1, db1, dW2, db2) by hand"""
    a = u @ W1.t() + b1
    da = (dy @ W2) * (a > 0)
    return da.t() @ u, da.sum(0), dy.t() @ torch.relu(a), dy.sum(0)


def box_dx_closed(x, dz, P):
    """the box MLP's input gradient by hand"""
    W0, b0, W1, b1, W2 = P[:5]
    a0 = x @ W0.t() + b0
    a1 = torch.relu(a0) @ W1.t() + b1
    return (((dz @ W2) * (a1 > 0)) @ W1 * (a0 > 0)) @ W0


def closed_grads(u, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes, used=None):
    """the closed form of chain_grads, no autograd: fp64.  -> (the eight gradients, dh of the used outputs)"""
    d = lambda v: v.detach().double()
    u, t_below, refs, tail, Wc, P = d(u), [d(v) for v in t_below], [d(v) for v in refs], [d(p) for p in tail], d(Wc), [d(p) for p in P]
    W1, b1, W2, b2, g3, be3, gd, bd = tail
    L = len(t_below) + 1
    used = list(range(L)) if used is None else list(used)
    _, y = ffn(u, W1, b1, W2, b2)
    t = t_below + [ln(y, g3, be3)]
    dh = {}
    for l in used:
        h = ln(t[l], gd, bd)
        p = torch.sigmoid(RB.mlp(h, P) + RB.isg(refs[l]))
        dz = d(cot_boxes[l]) * p * (1 - p)
        dh[l] = d(cot_logits[l]) @ Wc + box_dx_closed(h, dz, P)
    dgd, dbd = torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    dt = torch.zeros_like(y)
    for l in used:
        dx, dg, db = ln_backward(t[l], gd, dh[l])
        dgd, dbd = dgd + dg, dbd + db
        if l == L - 1:
            dt = dx
    dy, dg3, db3 = ln_backward(y, g3, dt)
    return list(ffn_grads_closed(u, W1, b1, W2, dy)) + [dg3, db3, dgd, dbd], [dh[l] for l in used]


# ---------------------------------------------------------------------------------------------------------------- pieces by autograd
def ln_grads(x, gamma, beta, g, dtype):
    """(dx, dgamma, dbeta) of <LayerNorm(x), g> by autograd in `dtype`"""
    x, gamma, beta = [v.detach().to(dtype).requires_grad_(True) for v in (x, gamma, beta)]
    return list(torch.autograd.grad((ln(x, gamma, beta) * g.detach().to(dtype)).sum(), [x, gamma, beta]))


def ffn_grads(u, W, dy, dtype):
    """(dW1, db1, dW2, db2) of <y(u), dy> by autograd in `dtype`"""
    W = [w.detach().to(dtype).requires_grad_(True) for w in W]
    _, y = ffn(u.detach().to(dtype), *W)
    return list(torch.autograd.grad((y * dy.detach().to(dtype)).sum(), W))


def box_dx(x, dz, P, dtype):
    x = x.detach().to(dtype).requires_grad_(True)
    return torch.autograd.grad((RB.mlp(x, [p.detach().to(dtype) for p in P]) * dz.detach().to(dtype)).sum(), x)[0]


# ---------------------------------------------------------------------------------------------------------------- cases and the rule
def tail_params(F, seed):
    """a seeded tail at nn.Linear's scale, the norms' affine parameters away from their initial 1 / 0"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g) * 2 - 1
    return [r(F, D) / 16, r(F) / 16, r(D, F) / F ** 0.5, r(D) / 16, 1 + 0.3 * r(D), 0.2 * r(D), 1 + 0.3 * r(D), 0.2 * r(D)]


def ffn_clear(u, W1, b1, margin=KINK):
    """per row of u: no pre-activation of linear1 within `margin` of zero (fp64)"""
    return (u.double() @ W1.double().t() + b1.double()).abs().min(1).values > margin


def ffn_case(M, F, seed, dtype=torch.float32):
    """(u [M,256] rounded to `dtype`, the tail's eight tensors): rows with a pre-activation within 1e-4 of zero are redrawn -- a ReLU
    that flips under rounding is a discontinuity neither the device nor the fp32 yardstick answers for.  Asserted before returning."""
    g = torch.Generator().manual_seed(seed)
    tail = tail_params(F, seed + 1000)
    u = torch.randn((M, D), generator=g).to(dtype)
    for _ in range(200):
        bad = ~ffn_clear(u.float(), tail[0], tail[1])
        if not bool(bad.any()):
            break
        u[bad] = torch.randn((int(bad.sum()), D), generator=g).to(dtype)
    assert bool(ffn_clear(u.float(), tail[0], tail[1]).all())
    return u, tail


def bound(e_cpu32, gmax):
    return max(4 * e_cpu32, 16 * U * gmax)


def report(tag, got, g64, g32, names=NAMES):
    """per tensor: E = max|got - g64| against bound(E_cpu32, max|g64|); prints every figure, returns the failures"""
    bad = []
    for name, d, a, b in zip(names, got, g64, g32):
        a = a.double()
        gmax = float(a.abs().max())
        e, e_cpu = float((d.double() - a).abs().max()), float((b.double() - a).abs().max())
        lim = bound(e_cpu, gmax)
        print(f"\n[{tag} {name}] E {e:.3e}  E_cpu32 {e_cpu:.3e}  max|g| {gmax:.3e}  bound {lim:.3e}")
        if not (bool(torch.isfinite(d).all()) and e <= lim):
            bad.append((tag, name, e, e_cpu, gmax))
    return bad
