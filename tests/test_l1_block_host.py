"""The ENGINE side of the one-launch layer1 bottlenecks (DTLREngine.use_l1_block), on CPU with torch stand-ins for the HIP operators:
which launches run, with which weights, and when the chained path stays."""
import pytest
import torch
import torch.nn.functional as F


def _setup(monkeypatch, blocks, H, W, dtype=torch.bfloat16, B=1):
    from dtlr_amd import ops
    from dtlr_amd.engine import DTLREngine
    g = torch.Generator().manual_seed(5)
    w = {}

    def conv_w(name, cout, cin, k):
        t = torch.randn((cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5
        w[name + ".w"] = (t.flatten(1) if k == 1 else t.permute(0, 2, 3, 1).contiguous()).to(dtype)       # 1x1: [Cout, Cin]; 3x3: OHWI
        w[name + ".b"] = torch.randn((cout,), generator=g) * 0.1
    widths = [(64, 64, 256), (256, 128, 512)]
    for li, nb in enumerate(blocks, start=1):
        cin, mid, cout = widths[li - 1]
        for bi in range(nb):
            conv_w(f"l{li}.{bi}.c1", mid, cin if bi == 0 else cout, 1)
            conv_w(f"l{li}.{bi}.c2", mid, mid, 3)
            conv_w(f"l{li}.{bi}.c3", cout, mid, 1)
            if bi == 0:
                conv_w(f"l{li}.{bi}.ds", cout, cin, 1)
    calls = []

    def lin(x, wt, b, residual=None, relu=True):           # fp32 accumulate, one rounding at the end: what every kernel does
        y = x.float() @ wt.float().t() + b
        y = y + residual.float() if residual is not None else y
        return (torch.relu(y) if relu else y).to(dtype)

    def conv3(x, wt, b):
        y = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float().permute(0, 3, 1, 2), b, stride=1, padding=1).permute(0, 2, 3, 1)
        return torch.relu(y).to(dtype)

    def fake_conv(self, name, x, stride, padding, relu=False, residual=None):
        wt = self.w[name + ".w"]
        calls.append(name)
        if wt.dim() == 2:
            return lin(x[:, ::stride, ::stride], wt, self.w[name + ".b"], residual, relu)
        y = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float().permute(0, 3, 1, 2), self.w[name + ".b"], stride=stride, padding=padding).permute(0, 2, 3, 1)
        return (torch.relu(y) if relu else y).to(dtype)

    def fake_chain(x, wp, b=None, x2=None, residual=None, relu=True, wp2=None, b2=None, n2=0):
        calls.append(f"chain{'+cat' if x2 is not None else '+res'}->{n2}")
        y = lin(torch.cat([x, x2], -1) if x2 is not None else x, wp, b, residual, relu)
        return y, (None if wp2 is None else lin(y, wp2, b2))

    def fake_cat_s2(t, x, wp, b=None, relu=True):
        calls.append("cat_s2")
        return lin(torch.cat([t, x[:, ::2, ::2]], -1), wp, b, None, relu)

    def fake_block(x, w1p, b1, w2, b2, w3p, b3, wnp=None, bn=None, n2=0, out=None, next_out=None):
        cin = x.shape[-1]
        calls.append(f"l1_bottleneck C{cin}->{n2}")
        assert w1p.shape == (64, cin) and w2.shape == (64, 3, 3, 64) and w3p.shape == (256, 128 if cin == 64 else 64)
        assert (n2 == 0) == (wnp is None) and (wnp is None or wnp.shape == (n2, 256))
        t2 = conv3(lin(x, w1p, b1), w2, b2)
        y = lin(torch.cat([t2, x], -1), w3p, b3) if cin == 64 else lin(t2, w3p, b3, residual=x)
        return y, (lin(y, wnp, bn) if n2 else None)
    monkeypatch.setattr(ops, "kres_pack", lambda wt, np_pairs=None: wt)
    monkeypatch.setattr(ops, "gemm_kres_chain", fake_chain)
    monkeypatch.setattr(ops, "gemm_kres_cat_s2", fake_cat_s2)
    monkeypatch.setattr(ops, "l1_bottleneck", fake_block)
    x0 = torch.relu(torch.randn((B, H, W, 64), generator=g)).to(dtype)
    monkeypatch.setattr(ops, "stem_conv7x7_pool", lambda *a, **k: x0)
    monkeypatch.setattr(ops, "stem_conv7x7_f32", lambda *a, **k: x0)
    monkeypatch.setattr(ops, "maxpool_nhwc", lambda x, **k: x)
    monkeypatch.setattr(ops, "zero_outside_extent", lambda *a, **k: calls.append("zero_ext"))
    monkeypatch.setattr(DTLREngine, "_conv", fake_conv)
    eng = object.__new__(DTLREngine)
    eng.w, eng.dtype, eng.use_stem_pool = dict(w, **{"conv1.frag": None, "conv1.b": None}), dtype, True
    eng.cfg = type("Cfg", (), {"backbone_blocks": blocks})()
    eng.use_l1_chain, eng.use_l1_chain_out, eng.use_l2_cat = True, True, True
    return eng, calls, x0


def _run(eng, calls, x0, ext=None):
    calls.clear()
    x = x0 if ext is None else x0.clone()
    return [t.float() for t in eng._backbone_layers(x, 1, len(eng.cfg.backbone_blocks), ext)], list(calls)


@pytest.mark.parametrize("H,W", [(128, 128), (126, 134)])
def test_l1_block_wiring_replaces_the_chain(monkeypatch, H, W):
    """flag on, qualifying shape: three l1_bottleneck launches (first-block form, identity, identity -> layer2.0.conv1), no conv1 / conv2 /
    chain / layer2.0.conv1 launch, and the maps of the chained path."""
    eng, calls, x0 = _setup(monkeypatch, (3, 2), H, W)
    want, chain_calls = _run(eng, calls, x0)                       # attributes absent: the present path
    assert chain_calls[:2] == ["l1.0.c1", "l1.0.c2"] and not any(c.startswith("l1_bottleneck") for c in chain_calls)
    eng.use_l1_block, eng.l1_block_min_wgs = 1, 1
    got, cl = _run(eng, calls, x0)
    assert [c for c in cl if c.startswith("l1_bottleneck")] == ["l1_bottleneck C64->0", "l1_bottleneck C256->0", "l1_bottleneck C256->128"]
    assert not any(c.startswith(("l1.", "chain")) for c in cl) and "l2.0.c1" not in cl
    assert cl[3:] == chain_calls[chain_calls.index("chain+res->128") + 1:]            # layer2 onwards: unchanged
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    # without the last link: two plain launches and an identity one, layer2.0.conv1 from its own launch
    eng.use_l1_chain_out = False
    eng.use_l1_block = 0
    want2, _ = _run(eng, calls, x0)
    eng.use_l1_block = 1
    got2, cl2 = _run(eng, calls, x0)
    assert [c for c in cl2 if c.startswith("l1_bottleneck")] == ["l1_bottleneck C64->0", "l1_bottleneck C256->0", "l1_bottleneck C256->0"]
    assert "l2.0.c1" in cl2 and all(torch.equal(a, b) for a, b in zip(got2, want2))


@pytest.mark.parametrize("case", ["flag off", "attributes absent", "ext", "fp32", "one-block layer1", "below the threshold"])
def test_l1_block_wiring_keeps_the_present_path(monkeypatch, case):
    """flag off, per-line extents, an fp32 map, a one-block layer1, too few workgroups: exactly the present call sequence"""
    blocks = (1, 1) if case == "one-block layer1" else (3, 2)
    dtype = torch.float32 if case == "fp32" else torch.bfloat16
    eng, calls, x0 = _setup(monkeypatch, blocks, 128, 130, dtype)
    ext = torch.tensor([[512, 520]]) if case == "ext" else None
    want, want_calls = _run(eng, calls, x0, ext)                   # no attribute set: off
    if case == "attributes absent":
        assert not hasattr(eng, "use_l1_block") and not hasattr(eng, "l1_block_min_wgs")
        assert "chain+cat->64" in want_calls and not any(c.startswith("l1_bottleneck") for c in want_calls)
        return
    eng.use_l1_block, eng.l1_block_min_wgs = 1, 1
    if case == "flag off":
        eng.use_l1_block = 0
    if case == "below the threshold":
        eng.l1_block_min_wgs = 4                                   # 1 image x 3 segments of 64 columns
    got, cl = _run(eng, calls, x0, ext)
    assert cl == want_calls and not any(c.startswith("l1_bottleneck") for c in cl)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    if case == "below the threshold":
        eng.l1_block_min_wgs = 3
        assert any(c.startswith("l1_bottleneck") for c in _run(eng, calls, x0)[1])
