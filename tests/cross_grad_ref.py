"""CPU yardsticks of the last decoder layer's cross-attention gradient with everything below it frozen (csrc/cross_grad.hip,
dtlr_amd/adapt.py).

      s, p --[sampling_offsets ; attention_weights]--> off, A --> loc --sampling of V--> o --output_proj--> + s --norm1--> u --> the tail (tail_grad_ref)

  block                         the restatement in torch, in the dtype of its inputs: s, p, R and V are constants of the frozen trunk; the
                                sampling is an explicit four-corner gather (differentiable in loc and A)
  chain_grads                   autograd's gradient of seeded cotangents on every output with respect to the eight cross tensors (and the
                                eight tail tensors), in the dtype asked for
  chain_grads_at                the same in the trainer's convention (the engine's h_l are inputs of the heads' gradients)
  closed_grads                  the closed form the kernels implement, written out without autograd (fp64)
  query_grads / query_grads_closed   the operator alone: (grad_loc, grad_attn) by autograd / by hand
  query_case                    seeded inputs of the operator's tests, every coordinate 1e-3 px away from every integer and border
  kink_margin / coords          the distance of the sampling coordinates from the bilinear kinks
  bound / report                the rule of DESIGN section 20 (tail_grad_ref's)
"""
import torch

from tests import box_grad_ref as RB
from tests import tail_grad_ref as RT

D, HEADS, HD, LV, PT = 256, 8, 32, 4, 4
NAMES = ("so_W", "so_b", "aw_W", "aw_b", "out_W", "out_b", "norm1_w", "norm1_b")
SHAPES = ((256, 256), (256,), (128, 256), (128,), (256, 256), (256,), (256,), (256,))
KINK = 1e-3
# Inputs that come out of a model cannot be conditioned.  E_PX bounds the largest |px_fp32 - px_fp64| of the restatement, measured on the golden
# inputs (8.36e-7, asserted by the host test; an fp32 ulp of px at these map sizes is 9.5e-7); such inputs are asserted DELTA = 4 E_PX from
# every kink: no fp32 evaluation of the coordinate can then fall on the other side.
E_PX = 8.5e-7
DELTA = 4 * E_PX
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


def starts(shapes):
    out, o = [], 0
    for H, W in shapes:
        out.append(o)
        o += H * W
    return out


def coords(loc, shapes):
    """loc [..,4,4,2] -> (px, py) [..,4,4]: px = loc_x W_l - 0.5, py = loc_y H_l - 0.5"""
    Hs = torch.tensor([h for h, _ in shapes], dtype=loc.dtype).view(4, 1)
    Ws = torch.tensor([w for _, w in shapes], dtype=loc.dtype).view(4, 1)
    return loc[..., 0] * Ws - 0.5, loc[..., 1] * Hs - 0.5


def kink_margin(loc, shapes):
    """the smallest distance (px) of a coordinate of an in-map point from an integer, and of any coordinate from the border tests' values
    (-1 and the map's size): where the bilinear sampling's derivative jumps.  A point wholly outside the map (the reference's test) is
    compared with the border only: between integers out there everything is zero on both sides."""
    px, py = coords(loc.double(), shapes)
    Hs = torch.tensor([h for h, _ in shapes], dtype=torch.float64).view(4, 1)
    Ws = torch.tensor([w for _, w in shapes], dtype=torch.float64).view(4, 1)
    inside = (px > -1) & (py > -1) & (px < Ws) & (py < Hs)
    frac = lambda v: (v - torch.round(v)).abs()
    big = torch.full_like(px, 1e9)
    d_int = torch.minimum(torch.where(inside, frac(px), big), torch.where(inside, frac(py), big))
    d_border = torch.minimum(torch.minimum((px + 1).abs(), (px - Ws).abs()), torch.minimum((py + 1).abs(), (py - Hs).abs()))
    return float(d_int.min()), float(d_border.min())


def kink_rows(loc, shapes, margin=KINK):
    """loc [B,nq,8,4,4,2] -> [B,nq] bool: the rows with a coordinate within `margin` px of an integer (the borders' values are integers)"""
    px, py = coords(loc.double(), shapes)
    near = ((px - torch.round(px)).abs() < margin) | ((py - torch.round(py)).abs() < margin)
    return near.flatten(2).any(-1)


def sample_parts(V, shapes, loc):
    """V [B,S,8,32], loc [B,nq,8,4,4,2] -> per level (v00, v01, v10, v11 [B,nq,8,4,32] with corners outside the map and points the
    reference's test rejects zeroed, lx, ly [B,nq,8,4])"""
    B, nq = loc.shape[:2]
    parts = []
    for l, ((H, W), st) in enumerate(zip(shapes, starts(shapes))):
        Vl = V[:, st:st + H * W].permute(0, 2, 1, 3)                                    # [B,8,HW,32]
        px, py = loc[..., l, :, 0] * W - 0.5, loc[..., l, :, 1] * H - 0.5               # [B,nq,8,4]
        x0, y0 = torch.floor(px), torch.floor(py)
        lx, ly = px - x0, py - y0
        inside = (px > -1) & (py > -1) & (px < W) & (py < H)
        x0, y0 = x0.long(), y0.long()

        def corner(yi, xi):
            ok = (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W) & inside
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).permute(0, 2, 1, 3).reshape(B, HEADS, nq * PT)
            v = torch.gather(Vl, 2, idx[..., None].expand(-1, -1, -1, HD)).view(B, HEADS, nq, PT, HD).permute(0, 2, 1, 3, 4)
            return v * ok[..., None].to(v.dtype)
        parts.append((corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1), lx, ly))
    return parts


def sample(V, shapes, loc, A):
    """the deformable attention's sampling: -> o [B,nq,256]"""
    o = 0
    for l, (v00, v01, v10, v11, lx, ly) in enumerate(sample_parts(V, shapes, loc)):
        lx, ly = lx[..., None], ly[..., None]
        val = (1 - ly) * (1 - lx) * v00 + (1 - ly) * lx * v01 + ly * (1 - lx) * v10 + ly * lx * v11
        o = o + (A[..., l, :, None] * val).sum(-2)
    return o.flatten(-2)


def block(s, p, R, V, shapes, cross):
    """the cross-attention block: s, p [B,nq,256], R [B,nq,4,4], V [B,S,8,32], cross: the eight tensors in NAMES' order ->
    dict(qin, A, loc, o, x1, u), rows flattened to M = B nq where the kernels flatten them"""
    Wso, bso, Waw, baw, Wo, bo, g1, b1 = cross
    B, nq = s.shape[:2]
    qin = s + p
    off = (qin @ Wso.t() + bso).view(B, nq, HEADS, LV, PT, 2)
    A = torch.softmax((qin @ Waw.t() + baw).view(B, nq, HEADS, LV * PT), -1).view(B, nq, HEADS, LV, PT)
    loc = R[:, :, None, :, None, :2] + off / PT * R[:, :, None, :, None, 2:] * 0.5
    o = sample(V, shapes, loc, A)
    x1 = s + o @ Wo.t() + bo
    u = RT.ln(x1, g1, b1)
    return {"qin": qin.reshape(-1, D), "A": A, "loc": loc, "o": o.reshape(-1, D), "x1": x1.reshape(-1, D), "u": u.reshape(-1, D)}


def _cin(cin, dtype):
    c = lambda v: v.detach().to(dtype)
    return c(cin["s"]), c(cin["qpos"]), c(cin["ref_in"]), c(cin["value"]), [tuple(int(x) for x in hw) for hw in cin["shapes"]]


def chain_grads(cin, cross, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes, dtype, used=None):
    """autograd's gradient of sum_(l in used) <logits_l, cl_l> + <boxes_l, cb_l> with respect to the eight cross tensors and the eight
    tail tensors, in `dtype`; cin: dict(s, qpos, ref_in, value, shapes).  -> (cross grads, tail grads)"""
    c = lambda v: v.detach().to(dtype)
    cross = [c(w).requires_grad_(True) for w in cross]
    tail = [c(w).requires_grad_(True) for w in tail]
    u = block(*_cin(cin, dtype), cross)["u"]
    logits, boxes, _, _ = RT.chain_outputs(u, [c(v) for v in t_below], [c(v) for v in refs], tail, c(Wc), c(bc), [c(w) for w in P])
    used = range(len(logits)) if used is None else used
    total = sum((logits[l] * c(cot_logits[l])).sum() + (boxes[l] * c(cot_boxes[l])).sum() for l in used)
    g = torch.autograd.grad(total, cross + tail)
    return list(g[:8]), list(g[8:])


def chain_grads_at(cin, cross, t_below, hs, tail, Wc, P, cot_logits, dz, dtype, used=None):
    """The trainer's convention (DESIGN sections 11, 22, 23): the heads' input gradients are taken AT the engine's h_l (hs), then the
    gradient of sum_l <decoder.norm(t_l), dh_l>, t_(L-1) recomputed from the block's u, with respect to the cross and the tail tensors."""
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
    cross = [c(w).requires_grad_(True) for w in cross]
    tail = [c(w).requires_grad_(True) for w in tail]
    W1, b1, W2, b2, g3, be3, gd, bd = tail
    u = block(*_cin(cin, dtype), cross)["u"]
    t = [c(v) for v in t_below] + [RT.ln(RT.ffn(u, W1, b1, W2, b2)[1], g3, be3)]
    total = sum((RT.ln(t[l], gd, bd) * dh[l]).sum() for l in used)
    g = torch.autograd.grad(total, cross + tail)
    return list(g[:8]), list(g[8:])


def query_grads_closed(V, shapes, loc, A, g):
    """(grad_loc, grad_attn) by hand: g [B,nq,256] the gradient at o"""
    g = g.view(*g.shape[:2], HEADS, 1, HD)
    dloc, dA = torch.zeros_like(loc), torch.zeros_like(A)
    for l, ((H, W), (v00, v01, v10, v11, lx, ly)) in enumerate(zip(shapes, sample_parts(V, shapes, loc))):
        dot = lambda v: (g * v).sum(-1)
        lx_, ly_ = lx[..., None], ly[..., None]
        dA[..., l, :] = dot((1 - ly_) * (1 - lx_) * v00 + (1 - ly_) * lx_ * v01 + ly_ * (1 - lx_) * v10 + ly_ * lx_ * v11)
        dloc[..., l, :, 0] = A[..., l, :] * W * dot((1 - ly_) * (v01 - v00) + ly_ * (v11 - v10))
        dloc[..., l, :, 1] = A[..., l, :] * H * dot((1 - lx_) * (v10 - v00) + lx_ * (v11 - v01))
    return dloc, dA


def query_grads(V, shapes, loc, A, g, dtype):
    """(grad_loc, grad_attn) of <sample(V, loc, A), g> by autograd in `dtype`"""
    c = lambda v: v.detach().to(dtype)
    loc, A = c(loc).requires_grad_(True), c(A).requires_grad_(True)
    return list(torch.autograd.grad((sample(c(V), shapes, loc, A) * c(g)).sum(), [loc, A]))


def closed_grads(cin, cross, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes, used=None):
    """the closed form of chain_grads' cross gradients, no autograd: fp64"""
    d = lambda v: v.detach().double()
    s, p, R, V, shapes = _cin(cin, torch.float64)
    cross, tail = [d(w) for w in cross], [d(w) for w in tail]
    Wso, bso, Waw, baw, Wo, bo, g1, b1 = cross
    W1, bb1, W2, b2, g3, be3, gd, bd = tail
    f = block(s, p, R, V, shapes, cross)
    u = f["u"]
    L = len(t_below) + 1
    used = list(range(L)) if used is None else list(used)
    assert used[-1] == L - 1
    _, dh = RT.closed_grads(u, t_below, refs, tail, Wc, bc, P, cot_logits, cot_boxes, used=used)      # the heads' input gradients
    a, y = RT.ffn(u, W1, bb1, W2, b2)
    dt, _, _ = RT.ln_backward(RT.ln(y, g3, be3), gd, dh[-1])
    dy, _, _ = RT.ln_backward(y, g3, dt)
    da = (dy @ W2) * (a > 0)
    du = dy + da @ W1
    dx1, dg1, db1 = RT.ln_backward(f["x1"], g1, du)
    dbo, dWo, g = dx1.sum(0), dx1.t() @ f["o"], dx1 @ Wo
    B, nq = s.shape[:2]
    dloc, dA = query_grads_closed(V, shapes, f["loc"], f["A"], g.view(B, nq, D))
    A16, dA16 = f["A"].flatten(-2), dA.flatten(-2)
    dlogit = A16 * (dA16 - (A16 * dA16).sum(-1, keepdim=True))
    doff = dloc * R[:, :, None, :, None, 2:] * 0.5 / PT
    doff, dlogit = doff.reshape(-1, 256), dlogit.reshape(-1, 128)
    return [doff.t() @ f["qin"], doff.sum(0), dlogit.t() @ f["qin"], dlogit.sum(0), dWo, dbo, dg1, db1]


# ---------------------------------------------------------------------------------------------------------------- cases
def cross_params(seed):
    """a seeded block: offsets of a few pixels at the maps' sizes, logits of order one, the norm's affine parameters away from 1 / 0"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=g) * 2 - 1
    return [r(256, 256) / 16, r(256), r(128, 256) / 16, r(128) / 4, r(256, 256) / 16, r(256) / 16, 1 + 0.3 * r(256), 0.2 * r(256)]


def condition(loc, shapes, margin=KINK, redraw=None):
    """move every coordinate that lies within `margin` px of an integer or of a border test's value by 4 margins (in px), until none
    does: asserted"""
    loc = loc.clone()
    Hs = torch.tensor([h for h, _ in shapes], dtype=torch.float64).view(4, 1)
    Ws = torch.tensor([w for _, w in shapes], dtype=torch.float64).view(4, 1)
    for _ in range(8):
        px, py = coords(loc.double(), shapes)
        bx, by = (px - torch.round(px)).abs() < 2 * margin, (py - torch.round(py)).abs() < 2 * margin      # the borders' values are integers too
        if not bool(bx.any() or by.any()):
            break
        loc[..., 0] = (loc[..., 0].double() + bx * (8 * margin) / Ws).to(loc.dtype)
        loc[..., 1] = (loc[..., 1].double() + by * (8 * margin) / Hs).to(loc.dtype)
    px, py = coords(loc.double(), shapes)
    assert float((px - torch.round(px)).abs().min()) >= margin and float((py - torch.round(py)).abs().min()) >= margin
    return loc


def query_case(B, nq, shapes, seed, vdtype=torch.float32):
    """(V [B,S,8,32] rounded to vdtype, loc in [-0.1, 1.1] conditioned KINK px away from every integer, A a softmax, g)"""
    gen = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in shapes)
    V = torch.randn((B, S, HEADS, HD), generator=gen).to(vdtype)
    loc = condition(torch.rand((B, nq, HEADS, LV, PT, 2), generator=gen) * 1.2 - 0.1, shapes)
    A = torch.softmax(torch.randn((B, nq, HEADS, LV * PT), generator=gen), -1).view(B, nq, HEADS, LV, PT)
    return V, loc, A, torch.randn((B, nq, D), generator=gen)
