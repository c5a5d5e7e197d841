"""CPU yardsticks of the box head's gradient with the trunk frozen (csrc/box_grad.hip, dtlr_amd/adapt.py).

  chain_boxes / chain_grads   the restatement in torch: the decoder states t_l, h_l and r_0 are constants, the shared MLP f is applied
                              at 2 L - 1 places (models/dino/deformable_transformer.py:734-756, dino.py:339-354, "look forward
                              twice"), gradients by autograd in the dtype asked for
  closed_grads                the closed form the kernels implement, written out without autograd (fp64)
  refine_grad                 its elementwise part: dboxes -> (dz, du)
  mlp_grads / mlp_grads_closed  the MLP's parameter gradient of sum_a <f(x_a), dy_a>, by autograd and by hand
  kernel_case                 seeded inputs of the kernel tests, conditioned as the bound needs (no pre-activation near a ReLU's kink)
"""
import numpy as np
import torch

EPS = 1e-3
SHAPES = ((256, 256), (256,), (256, 256), (256,), (4, 256), (4,))
NAMES = ("W0", "b0", "W1", "b1", "W2", "b2")


def isg(x, eps=EPS):
    """util/misc.py inverse_sigmoid"""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def mlp(x, P):
    W0, b0, W1, b1, W2, b2 = P
    return torch.relu(torch.relu(x @ W0.t() + b0) @ W1.t() + b1) @ W2.t() + b2


def chain_boxes(t, h, r0, P):
    """pred_boxes of the L outputs and the reference points r_0 .. r_L, as the reference's graph has them"""
    r, boxes, refs = r0, [], [r0]
    for l in range(len(t)):
        boxes.append(torch.sigmoid(mlp(h[l], P) + isg(r)))                # r_l is NOT detached here for l >= 1
        r = torch.sigmoid(mlp(t[l], P) + isg(r.detach()))                 # what the next layer sees
        refs.append(r)
    return boxes, refs


def chain_grads(t, h, r0, P, cot, dtype):
    """autograd's gradient of sum_l <pred_boxes_l, cot_l> with respect to the six MLP parameters, computed in `dtype`"""
    c = lambda v: v.detach().to(dtype)
    P = [c(p).requires_grad_(True) for p in P]
    boxes, _ = chain_boxes([c(v) for v in t], [c(v) for v in h], c(r0), P)
    total = sum((b * c(g)).sum() for b, g in zip(boxes, cot))
    return list(torch.autograd.grad(total, P))


def refine_grad(g, p, r, eps=EPS):
    """g, p, r [L,..,4] (r_0 .. r_(L-1)) -> dz [L,..,4], du [L-1,..,4]: the closed form, in the inputs' dtype"""
    dz = g * p * (1 - p)
    x = r[1:]
    zero = torch.zeros_like(x)
    isgp = torch.where(x > eps, 1 / x, zero) + torch.where(1 - x > eps, 1 / (1 - x), zero)      # a clamp that binds passes nothing
    return dz, dz[1:] * isgp * x * (1 - x)


def mlp_grads_closed(xs, dys, P):
    """sum over the applications of the MLP's parameter gradient, by hand, in the inputs' dtype"""
    W0, b0, W1, b1, W2, b2 = P
    out = [torch.zeros_like(p) for p in P]
    for x, dy in zip(xs, dys):
        x, dy = x.reshape(-1, 256), dy.reshape(-1, 4)
        a0 = x @ W0.t() + b0
        h0 = torch.relu(a0)
        a1 = h0 @ W1.t() + b1
        h1 = torch.relu(a1)
        da1 = (dy @ W2) * (a1 > 0)
        da0 = (da1 @ W1) * (a0 > 0)
        for k, v in enumerate((da0.t() @ x, da0.sum(0), da1.t() @ h0, da1.sum(0), dy.t() @ h1, dy.sum(0))):
            out[k] += v
    return out


def closed_grads(t, h, r0, P, cot):
    """the closed form of chain_grads, no autograd: fp64"""
    d = lambda v: v.detach().double()
    t, h, P, cot = [d(v) for v in t], [d(v) for v in h], [d(p) for p in P], [d(g) for g in cot]
    L = len(t)
    refs = [d(r0)]
    for l in range(L):
        refs.append(torch.sigmoid(mlp(t[l], P) + isg(refs[l])))
    p = torch.stack([torch.sigmoid(mlp(h[l], P) + isg(refs[l])) for l in range(L)])
    dz, du = refine_grad(torch.stack(cot), p, torch.stack(refs[:L]))
    return mlp_grads_closed(h + t[:L - 1], list(dz) + list(du), P), dz, du, refs


def mlp_grads(xs, dys, P, dtype):
    """autograd's gradient of sum_a <f(x_a), dy_a> in `dtype`"""
    P = [p.detach().to(dtype).requires_grad_(True) for p in P]
    total = sum((mlp(x.detach().to(dtype), P) * dy.detach().to(dtype)).sum() for x, dy in zip(xs, dys))
    return list(torch.autograd.grad(total, P))


def flat(grads):
    return torch.cat([g.reshape(-1) for g in grads])


def unflat(v):
    out, o = [], 0
    for s in SHAPES:
        k = int(np.prod(s))
        out.append(v[o:o + k].view(s))
        o += k
    return out


def params(seed, scale=1.0):
    """a seeded MLP at nn.Linear's scale (uniform +-1/16 weights), biases away from zero so that both ReLU branches occur"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: (torch.rand(s, generator=g) * 2 - 1) / 16 * scale
    return [u(256, 256), u(256), u(256, 256), u(256), u(4, 256) * 4, u(4)]


def pre_activations_clear(x, P, margin=1e-4):
    """per row of x: no pre-activation of either hidden layer lies within `margin` of zero (fp64)"""
    W0, b0, W1, b1 = [p.double() for p in P[:4]]
    a0 = x.double() @ W0.t() + b0
    a1 = torch.relu(a0) @ W1.t() + b1
    return (a0.abs().min(1).values > margin) & (a1.abs().min(1).values > margin)


def kernel_case(A, M, seed, dtype=torch.float32, live=None):
    """(xs, dys, P) of a kernel test: xs[a] [M,256] unit Gaussian rounded to `dtype`, dys[a] [M,4] Gaussian, zero outside the rows
    `live(a)` names (a boolean [M] mask; default: every row).  Rows with a pre-activation within 1e-4 of zero are redrawn (about 4% of
    random rows): a ReLU that flips under rounding is a discontinuity neither the device nor the fp32 yardstick answers for.  The
    condition is asserted before the case is returned."""
    g = torch.Generator().manual_seed(seed)
    P = params(seed + 1000)
    xs, dys = [], []
    for a in range(A):
        x = torch.randn((M, 256), generator=g).to(dtype)
        for _ in range(20):
            bad = ~pre_activations_clear(x.float(), P)
            if not bool(bad.any()):
                break
            x[bad] = torch.randn((int(bad.sum()), 256), generator=g).to(dtype)
        assert bool(pre_activations_clear(x.float(), P).all())
        dy = torch.randn((M, 4), generator=g)
        if live is not None:
            dy = dy * live(a)[:, None]
        xs.append(x)
        dys.append(dy)
    return xs, dys, P


def refs_clear(refs, margin=1e-4, eps=EPS):
    """no reference point within `margin` of either clamp threshold of isg"""
    r = torch.stack([v.double() for v in refs])
    return bool(((r - eps).abs() > margin).all() and ((r - (1 - eps)).abs() > margin).all())
