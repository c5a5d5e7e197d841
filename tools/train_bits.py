#!/usr/bin/env python3
"""The bits of the training path, for comparing two trees ("Bits against the parent"): run it on both on one MI355X, the two
files must be identical.

    python tools/train_bits.py --out FILE

One line per tensor: name, dtype, shape, SHA-256 of the raw bytes.
  * HeadTrainer on the tiny model (5 lines of 32 x 256 / 192, 30 queries, 23 classes), f32 and bf16 engines, every allowed combination of
    loss x train x aux_loss: three steps through `step` and, where the trainer allows it, through `cache` + `step_cached`.  After every
    step the losses, `grad`, `param`, both moments and the clip scale; then `state_dict()` (keys in order) and the forward after
    `write_back()`.
  * the standalone gradient operators on seeded inputs at small shapes, M = 150 rows (not a multiple of the 32-row tile): cross_recompute,
    msda_query_grad, cross_dow, self_recompute, mha_grad, ffn_recompute, ffn_grad, ln_backward, msda_value_grad, in fp32 / bf16 / fp16.
Reads nothing outside the repository."""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dtlr_amd import adapt, ops, synth, weights                 # noqa: E402
from dtlr_amd.config import DTLRConfig                          # noqa: E402
from dtlr_amd.dino import DINO                                  # noqa: E402

DEV = torch.device("cuda:0")
CLASSES, STEPS = 23, 3
CHAINS = ((), ("tail",), ("tail", "cross"), ("tail", "cross", "self"), ("tail", "cross", "self", "value"))
MAPS = [(4, 32), (2, 16), (1, 8), (1, 4)]                       # the operators' value map: S = 172


class Out:
    def __init__(self, path):
        self.f = open(path, "w")

    def line(self, text):
        self.f.write(text + "\n")

    def tensor(self, name, t):
        t = t.detach().contiguous().cpu()
        raw = t.reshape(-1).view(torch.uint8).numpy().tobytes()
        self.line(f"{name} {str(t.dtype).replace('torch.', '')} {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}")

    def value(self, name, v):
        if isinstance(v, torch.Tensor):
            self.tensor(name, v)
        elif isinstance(v, dict):
            for k, x in v.items():
                self.value(f"{name}.{k}", x)
        elif isinstance(v, (list, tuple)) and any(isinstance(x, torch.Tensor) for x in v):
            for i, x in enumerate(v):
                self.value(f"{name}[{i}]", x)
        else:
            self.line(f"{name} {v!r}")


def combinations():
    """every (loss, train, aux_loss) HeadTrainer accepts"""
    for loss, cls, box, chain, aux in itertools.product(("ctc", "set", "ctc+set"), (True, False), (False, True), CHAINS, (False, True)):
        train = (("class",) if cls else ()) + (("box",) if box else ()) + chain
        if train and not (loss == "ctc" and (box or aux)):
            yield loss, train, aux


def trainer_runs(out, engine, dtype, sd, cfg):
    imgs = [i.to(DEV) for i in synth.stroke_lines(3, 32, 256, seed=5) + synth.noise_lines(2, 32, 192, seed=6)]
    rng = np.random.Generator(np.random.PCG64(7))
    labels, tboxes = [], []
    for _ in imgs:
        T = int(rng.integers(3, 7))
        labels.append([int(v) for v in rng.integers(0, CLASSES, T)])
        tboxes.append(torch.from_numpy(np.concatenate([rng.uniform(0.1, 0.9, (T, 2)), rng.uniform(0.02, 0.2, (T, 2))], -1).astype(np.float32)))
    g = torch.Generator().manual_seed(17)
    head_w, head_b = torch.randn((CLASSES, cfg.hidden_dim), generator=g) * 0.05, torch.full((CLASSES,), -3.0)
    runs = 0
    for loss, train, aux in combinations():
        cached_ok = not aux and not set(train) & {"box", "cross", "self", "value"}
        for mode in ("step", "cached") if cached_ok else ("step",):
            model = DINO(cfg, compute_dtype=dtype)
            model.load_state_dict(sd)
            model = model.eval().to(DEV)
            adapt.new_class_head(model, CLASSES, head_w.clone(), head_b.clone())
            tr = adapt.HeadTrainer(model, lr=1e-3, weight_decay=1e-2, max_norm=0.5, loss=loss, train=train, aux_loss=aux)
            tag = f"{engine}/{loss}/{'+'.join(train)}/aux{int(aux)}/{mode}"
            kw = {} if loss == "ctc" else {"target_boxes": tboxes}
            if mode == "cached":
                hs, boxes = tr.cache(imgs)
                out.tensor(f"{tag}/cache.hs", hs)
                out.tensor(f"{tag}/cache.boxes", boxes)
            for k in range(STEPS):
                r = tr.step(imgs, labels, **kw) if mode == "step" else tr.step_cached(hs, boxes, labels, **kw)
                for name in sorted(r):
                    out.tensor(f"{tag}/step{k}/{name}", r[name])
                for name in ("grad", "param", "exp_avg", "exp_avg_sq", "scale"):
                    out.tensor(f"{tag}/step{k}/{name}", getattr(tr, name))
            out.value(f"{tag}/state_dict", tr.state_dict())
            tr.write_back()
            fwd = model(imgs)
            out.tensor(f"{tag}/write_back/pred_logits", fwd["pred_logits"])
            out.tensor(f"{tag}/write_back/pred_boxes", fwd["pred_boxes"])
            runs += 1
    return runs


def operators(out, name, dtype):
    g = torch.Generator().manual_seed(29)
    rn = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(DEV)
    N, Lq, D = 2, 75, 256
    M, S = N * Lq, sum(h * w for h, w in MAPS)
    shapes = torch.tensor(MAPS, dtype=torch.int64, device=DEV)
    lsi = torch.tensor([0] + list(np.cumsum([h * w for h, w in MAPS])[:-1]), dtype=torch.int64, device=DEV)
    s, qpos, value = rn(N, Lq, D).to(dtype), rn(N, Lq, D).to(dtype), rn(N, S, 8, 32).to(dtype)
    ref_in = torch.cat([torch.rand((N, Lq, 4, 2), generator=g) * 1.2 - 0.1, torch.rand((N, Lq, 4, 2), generator=g) * 0.3], -1).to(DEV)
    cross = [rn(*sh, scale=0.05) for sh in ops.CROSS_SHAPES]
    cross[6] = cross[6] + 1.0
    rec = ops.cross_recompute(s, qpos, ref_in, value, shapes, lsi, cross)
    out.value(f"ops/{name}/cross_recompute", rec)
    go = rn(N, Lq, D, scale=0.01)
    dloc, dA = ops.msda_query_grad(value, shapes, lsi, rec["loc"], rec["A"], go)
    out.tensor(f"ops/{name}/msda_query_grad.dloc", dloc)
    out.tensor(f"ops/{name}/msda_query_grad.dA", dA)
    out.value(f"ops/{name}/cross_dow", list(ops.cross_dow(rec["A"], dA, dloc, ref_in)))
    selfp = [rn(*sh, scale=0.05) for sh in ops.SELF_SHAPES]
    selfp[4] = selfp[4] + 1.0
    srec = ops.self_recompute(s, qpos, selfp)
    out.value(f"ops/{name}/self_recompute", srec)
    F = 192
    ffn = [rn(F, D, scale=0.05), rn(F, scale=0.05), rn(D, F, scale=0.05), rn(D, scale=0.05)]
    u = s.view(M, D)
    h, y = ops.ffn_recompute(u, ffn)
    out.tensor(f"ops/{name}/ffn_recompute.h", h)
    out.tensor(f"ops/{name}/ffn_recompute.y", y)
    dy = go.view(M, D)
    out.tensor(f"ops/{name}/ffn_grad", ops.ffn_grad(u, h, dy, ffn[2]))
    out.value(f"ops/{name}/ln_backward", list(ops.ln_backward(u, cross[6], dy)))
    if dtype == torch.float32:                                      # fp32 operands only
        qkv = srec["qkv"].view(N, Lq, 3 * D)
        out.value(f"ops/{name}/mha_grad", list(ops.mha_grad(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], go, 8)))
        out.tensor(f"ops/{name}/msda_value_grad", ops.msda_value_grad(shapes, lsi, rec["loc"], rec["A"], go, S))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_bits.py needs an MI355X (no CPU path)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = Out(args.out)
    cfg = DTLRConfig.tiny()
    sd = weights.synthetic_state_dict(cfg, seed=0)
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        operators(out, name, dtype)
    print("operators done", flush=True)
    for engine, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        print(f"{engine}: {trainer_runs(out, engine, dtype, sd, cfg)} runs", flush=True)
    out.f.close()
    with open(args.out, "rb") as f:
        print(f"{args.out}: {sum(1 for _ in f)} lines, SHA-256 {hashlib.sha256(open(args.out, 'rb').read()).hexdigest()}")


if __name__ == "__main__":
    main()
