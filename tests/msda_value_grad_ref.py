"""CPU yardsticks of the deformable attention's gradient with respect to `value` (csrc/msda_value_grad.hip).

  corners                 every sample's four corners: flat row of the value map, validity (inside the map, and the reference's test on the
                          point), and bilinear factor wy * wx -- cross_grad_ref.sample_parts' geometry with indices in place of gathers
  value_grad_closed       the closed form of the scatter: index_add_ of attn * wy * wx * g into [B,S,8,32], in the dtype given
  value_grad              autograd of <cross_grad_ref.sample(V, loc, A), g> with respect to V, in the dtype asked for
  touched                 [B,S,8] bool: the rows some valid corner lands on
  collide                 the heavy-collision inputs: every location of a head is one point
  value_map               the last decoder layer's value map from memory, the padding mask and value_proj, as the forward fills it
  chain_grads             section 24's chain (self_grad_ref.chain_grads) with value_proj as a seventh input of the block: autograd's
                          gradient of seeded cotangents on every output with respect to value_proj's two tensors, the six self, the eight
                          cross and the eight tail tensors, and the gradient at the value map
  chain_grads_at          the same in the trainer's convention (the engine's h_l are inputs of the heads' gradients)
  bound / report          the rule of DESIGN section 20 (tail_grad_ref's)
"""
import torch

from tests import box_grad_ref as RB
from tests import cross_grad_ref as RC
from tests import self_grad_ref as RS
from tests import tail_grad_ref as RT

HEADS, HD, LV, PT = RC.HEADS, RC.HD, RC.LV, RC.PT
bound, report, U = RC.bound, RC.report, RC.U
NAMES = ("value_proj_W", "value_proj_b")
SHAPES = ((256, 256), (256,))


def corners(shapes, loc):
    """loc [B,nq,8,4,4,2] -> per level four (idx, ok, w): idx [B,nq,8,4] int64 the corner's row of the flat map (clamped into its level),
    ok [B,nq,8,4] bool, w [B,nq,8,4] = wy * wx in loc's dtype; corners in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1)"""
    out = []
    for l, ((H, W), st) in enumerate(zip(shapes, RC.starts(shapes))):
        px, py = loc[..., l, :, 0] * W - 0.5, loc[..., l, :, 1] * H - 0.5
        x0, y0 = torch.floor(px), torch.floor(py)
        lx, ly = px - x0, py - y0
        inside = (px > -1) & (py > -1) & (px < W) & (py < H)
        x0, y0 = x0.long(), y0.long()
        lev = []
        for yi, wy in ((y0, 1 - ly), (y0 + 1, ly)):
            for xi, wx in ((x0, 1 - lx), (x0 + 1, lx)):
                ok = (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W) & inside
                lev.append((st + yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1), ok, wy * wx))
        out.append(lev)
    return out


def value_grad_closed(shapes, loc, A, g, S):
    """the scatter by hand, in loc's dtype: g [B,nq,256] the gradient at the sampler's output -> grad_value [B,S,8,32]"""
    B, nq = loc.shape[:2]
    gv = torch.zeros((B * S * HEADS, HD), dtype=loc.dtype)
    gh = g.view(B, nq, HEADS, 1, HD)
    b = torch.arange(B).view(B, 1, 1, 1)
    h = torch.arange(HEADS).view(1, 1, HEADS, 1)
    for l, lev in enumerate(corners(shapes, loc)):
        for idx, ok, w in lev:
            c = (A[..., l, :] * w * ok.to(loc.dtype))[..., None] * gh                    # [B,nq,8,4,32]
            gv.index_add_(0, (((b * S + idx) * HEADS + h)).reshape(-1), c.reshape(-1, HD))
    return gv.view(B, S, HEADS, HD)


def value_grad(shapes, loc, A, g, S, dtype):
    """grad_value of <sample(V, loc, A), g> by autograd in `dtype` (the sampling is linear in V: any V serves)"""
    c = lambda v: v.detach().to(dtype)
    V = torch.zeros((loc.shape[0], S, HEADS, HD), dtype=dtype, requires_grad=True)
    return torch.autograd.grad((RC.sample(V, shapes, c(loc), c(A)) * c(g)).sum(), V)[0]


def touched(shapes, loc, S):
    """[B,S,8] bool: the rows of the flat map that a valid corner of some sample lands on (from the fp64 corner indices)"""
    B = loc.shape[0]
    t = torch.zeros((B * S * HEADS,), dtype=torch.bool)
    b = torch.arange(B).view(B, 1, 1, 1)
    h = torch.arange(HEADS).view(1, 1, HEADS, 1)
    for lev in corners(shapes, loc.double()):
        for idx, ok, _ in lev:
            t[(((b * S + idx) * HEADS + h))[ok]] = True
    return t.view(B, S, HEADS)


def collide(B, nq, shapes, seed, outside=False):
    """query_case with every location of a (line, head) set to one point: nq * 16 samples of a head land on the same four pixels of each
    level (4 nq on each level).  outside: the point lies just left of the map (px in (-1, 0)), so that the two left corners drop out."""
    V, loc, A, g = RC.query_case(B, nq, shapes, seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    pt = torch.rand((B, 1, HEADS, 1, 1, 2), generator=gen) * 0.8 + 0.1
    if outside:
        pt[..., 0] = -0.3 / max(w for _, w in shapes)                    # px = -0.3 W_l / W_max - 0.5: in (-0.8, -0.5] on every level
    loc = RC.condition(pt.expand_as(loc).contiguous(), shapes)
    return V, loc, A, g


def value_map(memory, mask, vp):
    """memory [B,S,256], mask [B,S] bool or None, vp = (Wv, bv) -> V [B,S,8,32] = memory Wv^T + bv, the rows under the mask zero"""
    return _fill(memory @ vp[0].t() + vp[1], mask)


def _fill(proj, mask):
    V = proj if mask is None else proj.masked_fill(mask[..., None], 0.0)
    return V.view(*V.shape[:2], HEADS, HD)


def _u(vin, vp, sin, sp, cin, cross, dtype):
    """the state after norm1 from the layer's input, memory and the masters, and value_proj's output [B,S,256] before the rows under the
    mask are filled (the gradient at it is zero there, as the reference's is)"""
    c = lambda v: v.detach().to(dtype)
    proj = c(vin["memory"]) @ vp[0].t() + vp[1]
    V = _fill(proj, vin["mask"])
    s = RS.block(c(sin["t"]), c(sin["qpos"]), sp)["s"]
    _, p, R, _, shapes = RC._cin(cin, dtype)
    return RC.block(s.view(p.shape), p, R, V, shapes, cross)["u"], proj


def chain_grads(vin, vp, sin, sp, cin, cross, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes, dtype, used=None):
    """self_grad_ref.chain_grads with the value map recomputed from vin = dict(memory, mask) and vp = (Wv, bv); cin's "value" is unused.
    -> (value_proj grads, self grads, cross grads, tail grads, the gradient at value_proj's output [B,S,256]: zero under the mask)"""
    c = lambda v: v.detach().to(dtype)
    vp, sp, cross, tail = ([c(w).requires_grad_(True) for w in group] for group in (vp, sp, cross, tail))
    u, proj = _u(vin, vp, sin, sp, cin, cross, dtype)
    logits, boxes, _, _ = RT.chain_outputs(u, [c(v) for v in t_below], [c(v) for v in refs], tail, c(Wc), c(bc), [c(w) for w in P])
    used = range(len(logits)) if used is None else used
    total = sum((logits[l] * c(cot_logits[l])).sum() + (boxes[l] * c(cot_boxes[l])).sum() for l in used)
    g = torch.autograd.grad(total, vp + sp + cross + tail + [proj])
    return list(g[:2]), list(g[2:8]), list(g[8:16]), list(g[16:24]), g[24]


def chain_grads_at(vin, vp, sin, sp, cin, cross, t_below, hs, tail, Wc, P, cot_logits, dz, dtype, used=None):
    """self_grad_ref.chain_grads_at (the trainer's convention) with the value map recomputed from vin and vp
    -> (value_proj grads, self grads, cross grads, tail grads)"""
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
    vp, sp, cross, tail = ([c(w).requires_grad_(True) for w in group] for group in (vp, sp, cross, tail))
    W1, b1, W2, b2, g3, be3, gd, bd = tail
    u, _ = _u(vin, vp, sin, sp, cin, cross, dtype)
    t = [c(v) for v in t_below] + [RT.ln(RT.ffn(u, W1, b1, W2, b2)[1], g3, be3)]
    total = sum((RT.ln(t[l], gd, bd) * dh[l]).sum() for l in used)
    g = torch.autograd.grad(total, vp + sp + cross + tail)
    return list(g[:2]), list(g[2:8]), list(g[8:16]), list(g[16:])
