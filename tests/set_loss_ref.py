"""The yardstick of the set criterion, written from the formulas: the matching cost and the criterion in torch (so
that autograd gives the gradients, in fp64 and in fp32), a plain NumPy shortest-augmenting-path solver, and the seeded cases every test
of the feature draws from.  CPU only; nothing here touches the device or the reference tree."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

COSTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)           # the reference's set_cost_* and focal_alpha
ALPHA = 0.25
WEIGHTS = (1.0, 5.0, 2.0)                                            # cls / bbox / giou loss coefficients
# (L, B, nq, C, Tmin, Tmax) of the device tests, with the seed each is drawn with
CASES = {"empty_and_one": (11, 1, 3, 64, 23, 0, 11), "square": (12, 2, 2, 30, 23, 30, 30), "more_targets": (13, 1, 2, 12, 7, 5, 20),
         "mixed": (14, 3, 4, 64, 11, 1, 40), "model_shape": (15, 2, 2, 900, 166, 20, 100), "gather": (16, 1, 1, 900, 7356, 40, 40)}
GOLDEN_CASES = {"golden_0": (21, 7, 2, 30, 23, 0, 9), "golden_1": (22, 7, 3, 24, 11, 3, 30)}     # L = main + 5 auxiliary + intermediate
LOSS_COLUMNS = ("loss_ce", "loss_bbox", "loss_giou", "loss_xy", "loss_hw", "cardinality_error", "class_error", "n_matched")


def set_case(seed, L, B, nq, C, Tmin, Tmax):
    """logits [L,B,nq,C] fp32 (mostly negative, as a detector's), boxes [L,B,nq,4] cxcywh with positive width and height, and B targets
    {"labels": [T] int64 (duplicates allowed), "boxes": [T,4]}.  Line 0 has Tmin targets, the last line Tmax, line 1 of three or more
    min(Tmin + 1, Tmax), the others a uniform draw."""
    g = np.random.Generator(np.random.PCG64(seed))
    logits = (g.standard_normal((L, B, nq, C)) * 2.0 - 3.0).astype(np.float32)
    boxes = np.concatenate([g.uniform(0.1, 0.9, (L, B, nq, 2)), g.uniform(0.02, 0.2, (L, B, nq, 2))], -1).astype(np.float32)
    targets = []
    for b in range(B):
        T = Tmin if b == 0 else (Tmax if b == B - 1 else (min(Tmin + 1, Tmax) if b == 1 else int(g.integers(Tmin, Tmax + 1))))
        lab = g.integers(0, C, T).astype(np.int64)
        tb = np.concatenate([g.uniform(0.1, 0.9, (T, 2)), g.uniform(0.02, 0.2, (T, 2))], -1).astype(np.float32)
        targets.append({"labels": torch.from_numpy(lab), "boxes": torch.from_numpy(tb.reshape(T, 4))})
    return torch.from_numpy(logits), torch.from_numpy(boxes), targets


@functools.lru_cache(maxsize=None)
def case(name):
    return set_case(*{**CASES, **GOLDEN_CASES}[name])


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou_pairwise(a, b):
    """generalised IoU of every xyxy box of a [n,4] against every one of b [m,4] -> [n,m], with the reference's 1e-6 in both denominators"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[None, :, 2:]) - torch.max(a[:, None, :2], b[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a[:, None] + area_b[None, :] - inter
    hull = (torch.max(a[:, None, 2:], b[None, :, 2:]) - torch.min(a[:, None, :2], b[None, :, :2])).clamp(min=0)
    area = hull[..., 0] * hull[..., 1]
    return inter / (union + 1e-6) - (area - union) / (area + 1e-6)


def cost_block(logits, boxes, labels, tboxes, dtype, cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, alpha=ALPHA):
    """one line: logits [nq,C], boxes [nq,4], labels [T], tboxes [T,4] -> the matching cost [T,nq] (target-major) in `dtype`"""
    p = logits.to(dtype).sigmoid()[:, labels]
    neg = (1 - alpha) * p ** 2 * (-(1 - p + 1e-8).log())
    pos = alpha * (1 - p) ** 2 * (-(p + 1e-8).log())
    b, t = boxes.to(dtype), tboxes.to(dtype)
    l1 = (b[:, None, :] - t[None, :, :]).abs().sum(-1)
    c = cost_bbox * l1 + cost_class * (pos - neg) + cost_giou * -giou_pairwise(xyxy(b), xyxy(t))
    return c.t().contiguous()


def cost_blocks(logits, boxes, targets, dtype, **kw):
    """the stacked outputs -> [L B, Tmax, nq] with zero padding rows, as dtlr_set_cost lays it out"""
    L, B, nq, _ = logits.shape
    Tmax = max(max(len(t["labels"]) for t in targets), 1)
    out = torch.zeros((L * B, Tmax, nq), dtype=dtype)
    for l in range(L):
        for b, t in enumerate(targets):
            out[l * B + b, :len(t["labels"])] = cost_block(logits[l, b], boxes[l, b], t["labels"], t["boxes"], dtype, **kw)
    return out


def lsap(cost):
    """Minimum-cost assignment of a rectangular fp64 matrix by shortest augmenting paths with dual variables (Jonker-Volgenant as
    Crouse states it): -> (rows, cols), rows ascending, min(shape) pairs.  A plain port of the algorithm, a row at a time."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.shape[0] > cost.shape[1]:
        c, r = lsap(cost.T)
        order = np.argsort(r)
        return r[order], c[order]
    nr, nc = cost.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        short = np.full(nc, np.inf)
        path = np.full(nc, -1)
        seen_r, seen_c = np.zeros(nr, bool), np.zeros(nc, bool)
        i, minv, sink = cur, 0.0, -1
        while sink < 0:
            seen_r[i] = True
            free = ~seen_c
            r = minv + cost[i] - u[i] - v
            better = free & (r < short)
            short[better], path[better] = r[better], i
            cand = np.where(free, short, np.inf)
            best = cand.min()
            ties = np.nonzero(cand == best)[0]                      # among equals an unassigned column first, then the lowest index
            open_ = ties[row4col[ties] < 0]
            bj = int(open_[0]) if open_.size else int(ties[0])
            if not np.isfinite(best):
                raise ValueError("infeasible cost matrix")
            minv = best
            seen_c[bj] = True
            if row4col[bj] < 0:
                sink = bj
            else:
                i = row4col[bj]
        u[cur] += minv
        for i in range(nr):
            if seen_r[i] and i != cur:
                u[i] += minv - short[col4row[i]]
        v[seen_c] -= minv - short[seen_c]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return np.arange(nr), col4row.copy()


def match_rows(cost, sizes, solver):
    """cost [P,Tmax,nq] (NumPy), sizes [P] -> match_q [P,Tmax] int32 as dtlr_hungarian lays it out, by `solver` (lsap or scipy's)"""
    P, Tmax, _ = cost.shape
    out = np.full((P, Tmax), -1, dtype=np.int32)
    for p, T in enumerate(sizes):
        if T:
            t, q = solver(np.asarray(cost[p, :T], dtype=np.float64))
            out[p, t] = q
    return out


def indices_of(match_row, T):
    """a line's row of match_q -> the reference's (index_i, index_j): queries ascending, their targets"""
    q = np.asarray(match_row[:T], dtype=np.int64)
    t = np.nonzero(q >= 0)[0]
    order = np.argsort(q[t])
    return q[t][order], t[order]


def focal(x, onehot, alpha=ALPHA):
    """the element-wise sigmoid focal loss, gamma = 2"""
    p = x.sigmoid()
    ce = F.binary_cross_entropy_with_logits(x, onehot, reduction="none")
    p_t = p * onehot + (1 - p) * (1 - onehot)
    loss = ce * (1 - p_t) ** 2
    if alpha >= 0:
        loss = (alpha * onehot + (1 - alpha) * (1 - onehot)) * loss
    return loss


def losses_of(logits, boxes, targets, match, num_boxes, alpha=ALPHA):
    """one output: logits [B,nq,C], boxes [B,nq,4] (any float dtype, may require grad), the lines' match_q rows [B,Tmax] -> the eight
    values of LOSS_COLUMNS as 0-d tensors"""
    B, nq, C = logits.shape
    onehot = torch.zeros_like(logits)
    src, tgt, hit, card = [], [], 0, 0.0
    for b, t in enumerate(targets):
        q, k = indices_of(match[b], len(t["labels"]))
        onehot[b, q, t["labels"][k]] = 1
        src.append(boxes[b, q])
        tgt.append(t["boxes"][k].to(boxes.dtype))
        top = logits[b].detach().argmax(-1)
        hit += int((top[q] == t["labels"][k]).sum())
        card += abs(int((top != C - 1).sum()) - len(t["labels"]))
    src, tgt = torch.cat(src), torch.cat(tgt)
    l1 = (src - tgt).abs()
    n = src.shape[0]
    giou = torch.diag(giou_pairwise(xyxy(src), xyxy(tgt))) if n else src.new_zeros(0)
    z = logits.new_zeros(())
    return [focal(logits, onehot, alpha).mean(1).sum() / num_boxes * nq, l1.sum() / num_boxes, (1 - giou).sum() / num_boxes,
            l1[:, :2].sum().detach() / num_boxes, l1[:, 2:].sum().detach() / num_boxes, z + card / B,
            z + (100.0 - 100.0 * hit / n if n else 100.0), z + n]


def num_boxes_of(targets):
    return max(float(sum(len(t["labels"]) for t in targets)), 1.0)


def loss_and_grads(logits, boxes, targets, match, weights, dtype, alpha=ALPHA):
    """the stacked outputs [L,B,nq,C] / [L,B,nq,4], match_q [L B, Tmax], weights [L][3] -> (losses [L,8], dlogits, dboxes) in `dtype`:
    the gradients of sum_l (w_ce loss_ce + w_bbox loss_bbox + w_giou loss_giou) by autograd"""
    L, B = logits.shape[:2]
    x = logits.to(dtype).clone().requires_grad_(True)
    bx = boxes.to(dtype).clone().requires_grad_(True)
    nb = num_boxes_of(targets)
    rows, total = [], 0.0
    for l in range(L):
        v = losses_of(x[l], bx[l], targets, match[l * B:(l + 1) * B], nb, alpha)
        rows.append(torch.stack([t.detach() for t in v]))
        total = total + weights[l][0] * v[0] + weights[l][1] * v[1] + weights[l][2] * v[2]
    gl, gb = torch.autograd.grad(total, (x, bx), allow_unused=True)
    gb = torch.zeros_like(bx) if gb is None else gb
    return torch.stack(rows), gl, gb


def weight_dict(n_aux=5, interm=True, coef=WEIGHTS, interm_coef=1.0):
    """the reference's weight_dict without the denoising entries: loss_ce / loss_bbox / loss_giou, the same under _0.._{n_aux-1}, and
    under _interm scaled by interm_loss_coef"""
    base = {"loss_ce": coef[0], "loss_bbox": coef[1], "loss_giou": coef[2]}
    wd = dict(base)
    for i in range(n_aux):
        wd.update({f"{k}_{i}": v for k, v in base.items()})
    if interm:
        wd.update({f"{k}_interm": v * interm_coef for k, v in base.items()})
    return wd


def suffixes(L):
    """the key suffix of each stacked output: main, the auxiliary ones, the intermediate one last (L >= 3)"""
    return [""] + [f"_{i}" for i in range(L - 2)] + ["_interm"] if L >= 3 else [""] + [f"_{i}" for i in range(L - 1)]


def outputs_dict(logits, boxes):
    """the stacked outputs as the engine's dict: pred_*, aux_outputs, interm_outputs (the last one, for L >= 3)"""
    L = len(logits)
    out = {"pred_logits": logits[0], "pred_boxes": boxes[0]}
    n_aux = L - 2 if L >= 3 else L - 1
    if n_aux:
        out["aux_outputs"] = [{"pred_logits": logits[1 + i], "pred_boxes": boxes[1 + i]} for i in range(n_aux)]
    if L >= 3:
        out["interm_outputs"] = {"pred_logits": logits[L - 1], "pred_boxes": boxes[L - 1]}
    return out
