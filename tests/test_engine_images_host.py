"""DTLREngine's memo of packed weight images (engine._IMAGES, DTLREngine._image / _has_image / _drop_images), on the CPU: stand-in packers
record (packer, argument shapes) and return tagged tensors, engines are bare objects with a small `w`."""
import pytest
import torch

PACKERS = ("kres_pack", "kres_pack_bcast384", "k256_pack", "proj_ln_k256_pack", "proj_pack_w", "ffn_pack_w2", "ffn32_pack", "ffn_split_pack",
           "k256s_pack", "head_ts_pack", "split_head_weight", "dq_pack")
PAIRS = ("ffn32_pack", "head_ts_pack", "split_head_weight")          # packers that return two tensors


def _engine(monkeypatch, w, dtype=torch.bfloat16):
    from dtlr_amd import ops
    from dtlr_amd.engine import DTLREngine
    calls = []

    def stand_in(packer):
        def pack(*args, **kw):
            calls.append((packer, tuple(tuple(a.shape) for a in args if torch.is_tensor(a))))
            tag = torch.full((1,), float(len(calls)))
            tag.packer, tag.args = packer, args
            return (tag, tag.clone()) if packer in PAIRS else tag
        return pack
    for p in PACKERS:
        monkeypatch.setattr(ops, p, stand_in(p))
    eng = object.__new__(DTLREngine)
    eng.w, eng.dtype = dict(w), dtype
    return eng, calls


def _rand(*shape, seed=0, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


# (kind, name, base weights the builder reads, fp32 sources it consumes)
KINDS = [
    ("kres", "l1.1.c3", {"l1.1.c3.w": (256, 64)}, ()),
    ("bcast384", "enc0.attn.ow", {"enc0.attn.ow.w": (384, 256)}, ()),
    ("k256", "enc0.attn.value", {"enc0.attn.value.w": (256, 256)}, ()),
    ("k256_slices", "dec.value_all", {"dec.value_all.w": (1536, 256)}, ()),
    ("pln_k256", "enc0.attn.out", {"enc0.attn.out.w": (256, 256)}, ()),
    ("proj", "enc0.attn.out", {"enc0.attn.out.w": (256, 256)}, ()),
    ("ffn_w2", "enc0.ff2", {"enc0.ff2.w": (256, 1024)}, ()),
    ("ffn32", "enc0.ff", {"enc0.ff1.w": (1024, 256), "enc0.ff2.w": (256, 1024)}, ()),
    ("ffn_split", "enc0.ff", {}, ("enc0.ff1", "enc0.ff2")),
    ("k256s", "enc0.attn.out", {}, ("enc0.attn.out",)),
    ("k256s_slices", "dec.value_all", {}, ("dec.value_all",)),
    ("head_ts", "class", {"class.w": (166, 256), "class.b": (166,)}, ()),
    ("head_hi_lo", "class", {"class.w": (166, 256)}, ()),
    ("head_split3", "enc_class", {"enc_class.w": (166, 256), "enc_class.b": (166,)}, ()),
    ("dq", "dec0.sa.qk", {"dec0.sa.qk.w": (512, 256)}, ()),
    ("kres_cat", "l2.0", {"l2.0.c3.w": (512, 128), "l2.0.ds.w": (512, 256), "l2.0.c3.b": (512,), "l2.0.ds.b": (512,)}, ()),
]


def test_the_table_covers_every_kind_once():
    from dtlr_amd.engine import _IMAGES, _F32_SOURCES
    assert sorted(k for k, *_ in KINDS) == sorted(_IMAGES)
    assert set(_F32_SOURCES) == {k for k, _, _, src in KINDS if src}


@pytest.mark.parametrize("kind,name,base,src", KINDS, ids=[k for k, *_ in KINDS])
def test_each_image_is_built_exactly_once(monkeypatch, kind, name, base, src):
    w = {k: _rand(*s, seed=i) for i, (k, s) in enumerate(base.items())}
    w.update({("f32", s): _rand(*((1024, 256) if s.endswith("ff1") else (256, 1024) if s.endswith("ff2") else (1536, 256) if s == "dec.value_all"
                                   else (256, 256)), seed=9) for s in src})
    eng, calls = _engine(monkeypatch, w)
    assert eng._has_image(kind, name)
    first = eng._image(kind, name)
    n = len(calls)
    assert n >= (0 if kind == "head_hi_lo" else 1)
    for _ in range(3):
        assert eng._image(kind, name) is first
    assert len(calls) == n and eng.w[kind, name] is first and eng._has_image(kind, name)
    assert [k for k in eng.w if isinstance(k, tuple) and k[0] != "f32"] == [(kind, name)]
    assert all(isinstance(k, tuple) or k in w for k in eng.w)                      # base keys untouched, no string key added
    for s in src:                                                                  # the fp32 sources are released, the image stays available
        assert not torch.is_tensor(eng.w.get(("f32", s)))


def test_two_kinds_of_one_name_are_two_entries(monkeypatch):
    """`.wk` was ops.kres_pack in _conv and ops.proj_ln_k256_pack in _proj_ln; `.wp` ops.proj_pack_w and ops.ffn_pack_w2"""
    eng, calls = _engine(monkeypatch, {"p.w": _rand(256, 256)})
    imgs = {kind: eng._image(kind, "p") for kind in ("kres", "pln_k256", "proj", "ffn_w2", "k256", "dq")}
    assert [c[0] for c in calls] == ["kres_pack", "proj_ln_k256_pack", "proj_pack_w", "ffn_pack_w2", "k256_pack", "dq_pack"]
    assert len({id(t) for t in imgs.values()}) == 6 and all(eng.w[kind, "p"] is t for kind, t in imgs.items())
    assert all(eng._image(kind, "p") is t for kind, t in imgs.items()) and len(calls) == 6


@pytest.mark.parametrize("name,cout,mid,cin", [("l1.0", 256, 64, 64), ("l2.0", 512, 128, 256)])
def test_kres_cat_is_one_builder_for_both_layers(monkeypatch, name, cout, mid, cin):
    bf = torch.bfloat16
    w = {name + ".c3.w": _rand(cout, mid, seed=1, dtype=bf), name + ".ds.w": _rand(cout, cin, seed=2, dtype=bf),
         name + ".c3.b": _rand(cout, seed=3), name + ".ds.b": _rand(cout, seed=4)}
    eng, calls = _engine(monkeypatch, w)
    img, bias = eng._image("kres_cat", name)
    assert calls == [("kres_pack", ((cout, mid + cin),))]
    arg, = img.args
    assert arg.is_contiguous() and torch.equal(arg, torch.cat([w[name + ".c3.w"], w[name + ".ds.w"]], 1))
    assert bias.dtype == torch.float32 and bias.is_contiguous() and torch.equal(bias, w[name + ".c3.b"] + w[name + ".ds.b"])
    assert eng._image("kres_cat", name)[0] is img and len(calls) == 1


def test_ffn_w2_of_a_box_mlp_packs_the_16_bit_copy(monkeypatch):
    eng, _ = _engine(monkeypatch, {"bbox1.w": _rand(256, 256), "bbox1.wh": _rand(256, 256, dtype=torch.bfloat16)})
    assert eng._image("ffn_w2", "bbox1").args[0] is eng.w["bbox1.wh"]


def test_k256s_slices(monkeypatch):
    wf = _rand(1536, 256, seed=3)
    eng, calls = _engine(monkeypatch, {("f32", "dec.value_all"): wf})
    sl = eng._image("k256s_slices", "dec.value_all")
    assert calls == [("k256s_pack", ((256, 256),))] * 6 and [(r0, n) for _, r0, n in sl] == [(256 * j, 256) for j in range(6)]
    assert all(torch.equal(img.args[0], wf[r0:r0 + 256]) and img.args[0].is_contiguous() for img, r0, _ in sl)
    wo = _rand(384, 256, seed=4)
    eng, calls = _engine(monkeypatch, {("f32", "enc0.attn.ow"): wo})
    (a, a0, an), (b, b0, bn) = eng._image("k256s_slices", "enc0.attn.ow")
    assert (a0, an, b0, bn) == (0, 256, 256, 128) and calls == [("k256s_pack", ((256, 256),))] * 2
    assert torch.equal(a.args[0], wo[:256]) and torch.equal(b.args[0][:128], wo[256:]) and not b.args[0][128:].any() and b.args[0].is_contiguous()


def test_fp32_sources_are_released_and_the_image_stays_available(monkeypatch):
    w1, w2, wo = _rand(1024, 256, seed=1), _rand(256, 1024, seed=2), _rand(256, 256, seed=3)
    eng, calls = _engine(monkeypatch, {("f32", "enc0.ff1"): w1, ("f32", "enc0.ff2"): w2, ("f32", "enc0.attn.out"): wo}, torch.float32)
    assert eng._has_image("ffn_split", "enc0.ff") and eng._has_image("k256s", "enc0.attn.out")
    img = eng._image("ffn_split", "enc0.ff")
    assert img.args[0] is w1 and img.args[1] is w2
    assert eng._image("k256s", "enc0.attn.out").args[0] is wo
    assert not any(torch.is_tensor(v) for k, v in eng.w.items() if k[0] == "f32")          # nothing holds the fp32 weights any more
    assert eng._has_image("ffn_split", "enc0.ff") and eng._has_image("k256s", "enc0.attn.out")
    assert eng._image("ffn_split", "enc0.ff") is img and len(calls) == 2


def test_an_image_without_source_is_unavailable_and_the_error_says_why(monkeypatch):
    eng, calls = _engine(monkeypatch, {("f32", "enc0.attn.ow"): _rand(384, 256), ("f32", "enc0.ff1"): _rand(1024, 256)}, torch.float32)
    for kind, name in (("k256s", "dec0.sa.out"), ("k256s_slices", "nowhere"), ("ffn_split", "enc0.ff")):       # the last: one of two sources
        assert not eng._has_image(kind, name)
        with pytest.raises(RuntimeError, match="no fp32 weight .* is held"):
            eng._image(kind, name)
        assert (kind, name) not in eng.w
    assert torch.is_tensor(eng.w["f32", "enc0.ff1"]), "a failed build must not release the source it did find"
    # two kinds on one released source: the second is refused by name, not by a KeyError inside a forward
    eng._image("k256s_slices", "enc0.attn.ow")
    assert not eng._has_image("k256s", "enc0.attn.ow")
    with pytest.raises(RuntimeError, match="'k256s'.*'enc0.attn.ow'.*'k256s_slices'"):
        eng._image("k256s", "enc0.attn.ow")
    assert not calls[2:]


def test_no_weight_is_kept_for_two_kinds():
    """the split engine's rule for which fp32 weights to keep lives with the builders; every name has at most one consumer"""
    from dtlr_amd.engine import _F32_SOURCES
    names = [f"{p}{n}.{s}" for p in ("enc", "dec") for n in range(6) for s in ("attn.ow", "attn.value", "attn.out", "sa.qk", "sa.v", "sa.out", "ff1", "ff2")]
    names += ["enc_output", "dec.value_all", "dec.rph0", "ip0", "swin.0.0.qkv", "swin.0.0.fc2"]
    kept = {}
    for name in names:
        for shape in ((256, 256), (384, 256), (1536, 256), (1024, 256), (256, 1024)):
            kinds = [kind for kind, (_, keeps) in _F32_SOURCES.items() if keeps(name, shape)]
            assert len(kinds) <= 1, (name, shape, kinds)
            if kinds:
                assert name in _F32_SOURCES[kinds[0]][0](name[:-1] if kinds[0] == "ffn_split" else name)
                kept.setdefault(kinds[0], set()).add((name, shape == (256, 256)))
    assert ("enc0.attn.out", True) in kept["k256s"] and ("dec5.sa.out", True) in kept["k256s"] and ("enc_output", True) in kept["k256s"]
    assert not any(n.startswith("dec") and n.endswith("attn.value") for n, _ in kept["k256s"]) and all(sq for _, sq in kept["k256s"])
    assert {n for n, _ in kept["k256s_slices"]} == {f"enc{n}.attn.ow" for n in range(6)} | {"dec.value_all"}
    assert {n for n, _ in kept["ffn_split"]} == {f"{p}{n}.ff{i}" for p in ("enc", "dec") for n in range(6) for i in (1, 2)}


def test_set_class_head_drops_the_images_of_class_and_nothing_else(monkeypatch):
    w = {"class.w": _rand(166, 256, seed=1), "class.b": _rand(166, seed=2), "enc_class.w": _rand(166, 256, seed=3), "enc_class.b": _rand(166, seed=4),
         "enc_output.w": _rand(256, 256, seed=5, dtype=torch.bfloat16)}
    eng, calls = _engine(monkeypatch, w)
    eng.cfg, eng.device, eng.split = type("Cfg", (), {"hidden_dim": 256})(), torch.device("cpu"), False
    keep = {k: eng._image(*k) for k in (("head_ts", "enc_class"), ("head_split3", "enc_class"), ("proj", "enc_output"))}
    gone = {k: eng._image(*k) for k in (("head_ts", "class"), ("head_hi_lo", "class"))}
    eng.w["dq", "class"] = torch.zeros(1)                 # an image kind of `class` that set_class_head has never heard of
    hi = w["class.w"].bfloat16()
    assert torch.equal(gone["head_hi_lo", "class"], torch.cat([hi, (w["class.w"] - hi.float()).bfloat16()], 1))
    nw, nb = _rand(40, 256, seed=7), _rand(40, seed=8)
    eng.set_class_head(nw, nb)
    assert not [k for k in eng.w if isinstance(k, tuple) and k[1] == "class"]
    assert all(eng.w[k] is v for k, v in keep.items()) and eng.w["enc_class.w"] is w["enc_class.w"]
    assert torch.equal(eng.w["class.w"], nw) and eng.w["class.w"] is not nw and eng.num_classes == 40
    n = len(calls)
    img, _ = eng._image("head_ts", "class")
    assert len(calls) == n + 1 and calls[-1] == ("head_ts_pack", ((40, 256), (40,))) and img is not gone["head_ts", "class"][0]
    assert eng._image("head_hi_lo", "class").shape == (40, 512)
    assert all(eng._image(*k) is v for k, v in keep.items()) and len(calls) == n + 1
