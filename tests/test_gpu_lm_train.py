"""Device tests of n-gram training: dtlr_sort_u64 against numpy.sort, exact; the estimator against the plain-Python
reference of tests/lm_train_ref.py -- n-grams, counts, adjusted counts and fallback orders exact, log10 p and log10 back-off within 1e-9
(both sides compute the same few dozen fp64 operations per n-gram from the same integers: about 1e-13 in log10 p; a wrong discount
or denominator shows at 1e-2) --; then through the ARPA file, through pack_lm, through the device decoder, the refusals and the CLI."""
import functools
import math

import numpy as np
import pytest
import torch

from dtlr_amd import lmtrain, ops
from dtlr_amd import ngram as NG
from tests import lm_train_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = lmtrain.SORT_TILE
TOL = 1e-9


# ---- the sort --------------------------------------------------------------------------------------------------------------------
def _sorted_on_device(keys: np.ndarray, bits: int) -> np.ndarray:
    t = torch.from_numpy(keys.view(np.int64).copy()).to(DEV)
    before = t.clone()
    out = ops.sort_u64(t, bits)
    assert out.dtype == torch.int64 and out.device == t.device and tuple(out.shape) == (keys.size,)
    assert torch.equal(t, before)                                    # the input is not written
    return out.cpu().numpy().view(np.uint64)


def _draw(n: int, bits: int, seed: int) -> np.ndarray:
    rng = np.random.RandomState(seed)
    k = rng.randint(0, 1 << 32, size=n, dtype=np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, size=n, dtype=np.uint64)
    return k if bits == 64 else k & np.uint64((1 << bits) - 1)


@pytest.mark.parametrize("bits", [8, 13, 40, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_sort_against_numpy(n, bits):
    keys = _draw(n, bits, 7 * n + bits)
    assert np.array_equal(_sorted_on_device(keys, bits), np.sort(keys))


@pytest.mark.parametrize("kind", ["equal", "sorted", "reversed", "top_digit"])
def test_sort_on_the_orders_that_break_a_radix_sort(kind):
    n = 3 * TILE + 17
    if kind == "equal":
        keys = np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    elif kind == "top_digit":                                        # equal but for the most significant byte
        keys = (np.random.RandomState(1).randint(0, 256, size=n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x00FFEEDDCCBBAA99)
    else:
        keys = np.sort(_draw(n, 64, 5))
        if kind == "reversed":
            keys = keys[::-1].copy()
    assert np.array_equal(_sorted_on_device(keys, 64), np.sort(keys))


def test_sort_is_stable_in_the_bits_it_does_not_read():
    """key_bits = 8 orders by the low byte alone: the bytes above keep their order of arrival"""
    n = 2 * TILE + 5
    keys = (np.arange(n, dtype=np.uint64) << np.uint64(8)) | np.random.RandomState(2).randint(0, 7, size=n).astype(np.uint64)
    got = _sorted_on_device(keys, 8)
    want = keys[np.argsort(keys & np.uint64(255), kind="stable")]
    assert np.array_equal(got, want)


def test_sort_of_nothing_does_nothing():
    out = ops.sort_u64(torch.empty((0,), dtype=torch.int64, device=DEV))
    assert out.numel() == 0 and out.dtype == torch.int64


# ---- the model -------------------------------------------------------------------------------------------------------------------
CASES = {f"{o}-{s}-{n}": (lambda key=(o, s, n): (R.corpus(key[1], key[2], R.SEEDS[key]), key[0])) for o, s, n in R.CORPORA}
CASES["big"] = lambda: (R.big_corpus(), 6)
CASES["edge"] = lambda: (R.edge_corpus(), 8)


@functools.lru_cache(maxsize=None)
def _both(name):
    """(the corpus, the reference model, the device model), each computed once"""
    lines, order = CASES[name]()
    return lines, R.train(lines, order), lmtrain.train_ngram(lines, order, device=DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_model_against_the_reference(name):
    lines, ref, got = _both(name)
    assert got.order == ref.order and got.vocab == ref.vocab and got.fallback_orders == ref.fallback_orders
    if name == "big":
        assert sum(len(line) + 2 for line in lines) > 3 * TILE and any(not line for line in lines) and any(len(line) == 1 for line in lines)
    if name == "edge":
        assert len(ref.vocab) == 255 and lmtrain.key_bits_of(len(ref.vocab) - 3) * ref.order == 64
    tabs = R.tables(ref)
    worst = 0.0
    for k in range(ref.order):
        ids = got.ids[k].cpu().tolist()
        assert got.ids[k].dtype == torch.int32 and got.logp[k].dtype == torch.float64 and got.counts[k].dtype == torch.int64
        grams = [tuple(got.vocab[i - 1] for i in g) for g in ids]
        assert grams == [g for g, _, _ in tabs[k]], k + 1               # the same n-grams, in the order of the word ids
        assert got.counts[k].cpu().tolist() == [ref.counts[k][g] for g in grams], k + 1
        assert got.adjusted[k].cpu().tolist() == [ref.adjusted[k][g] for g in grams], k + 1
        lp, bo = got.logp[k].cpu().tolist(), got.bo[k].cpu().tolist()
        for (g, rp, rb), p, b in zip(tabs[k], lp, bo):
            worst = max(worst, abs(p - rp), abs(b - rb))
    print(f"{name}: n-grams {[len(t) for t in tabs]}, fallback {got.fallback_orders}, worst |log10 difference| {worst:.3e}")
    assert worst <= TOL
    for D, RD in zip(got.discounts, ref.discounts):
        assert max(abs(a - b) for a, b in zip(D, RD)) <= 1e-12


@pytest.mark.parametrize("name", ["5-6-200", "big"])
def test_two_runs_give_the_same_bytes(name):
    lines, _, first = _both(name)
    again = lmtrain.train_ngram(lines, first.order, device=DEV)
    for k in range(first.order):
        for field in ("ids", "logp", "bo", "counts", "adjusted"):
            a, b = getattr(first, field)[k], getattr(again, field)[k]
            assert torch.equal(a.view(torch.uint8) if a.dtype != torch.float64 else a.view(torch.int64),
                               b.view(torch.uint8) if b.dtype != torch.float64 else b.view(torch.int64)), (k + 1, field)


# ---- through the file, the packer and a decoder ------------------------------------------------------------------------------------
def test_through_the_file(tmp_path):
    _, ref, got = _both("5-6-200")
    path = str(tmp_path / "lm.arpa")
    got.write_arpa(path)
    lm = NG.ArpaLM(path)
    assert lm.order == 5 and lm.grams == got.to_arpa_lm().grams       # the numbers read back as the same doubles
    worst, contexts = R.normalisation_errors(lm, ref)
    print(f"normalisation over {contexts} contexts: worst |sum - 1| {worst:.3e}")
    assert contexts > 500 and worst <= TOL
    rpath = str(tmp_path / "ref.arpa")
    R.write_arpa(ref, rpath)
    tokens = ["<ctc>"] + ref.vocab[3:]
    a, b = NG.pack_lm(got.to_arpa_lm(), tokens), NG.pack_lm(NG.ArpaLM(rpath), tokens)
    for key in ("tok", "child_lo", "child_hi", "suffix", "ctx"):
        assert torch.equal(a[key], b[key]), key
    for key in ("order", "bos_state", "eos_tok", "has_bos", "has_eos", "vocab"):
        assert a[key] == b[key], key
    assert float((a["logp"] - b["logp"]).abs().max()) <= TOL and float((a["bo"] - b["bo"]).abs().max()) <= TOL
    assert abs(a["unk"] - b["unk"]) <= TOL


def test_through_a_decoder(tmp_path):
    _, ref, got = _both("5-6-200")
    rpath = str(tmp_path / "ref.arpa")
    R.write_arpa(ref, rpath)
    tokens = ["<ctc>"] + ref.vocab[3:]
    V = len(tokens)
    em = torch.softmax(3.0 * torch.randn((4, 24, V), generator=torch.Generator().manual_seed(3), dtype=torch.float32), dim=-1).to(DEV)
    spans = [(b, 0, 24) for b in range(4)]
    mine = NG.DeviceNgramDecoder(tokens, got.to_arpa_lm(), lm_weight=0.5, beam_size=16, device=DEV).decode_spans(em, spans)
    theirs = NG.DeviceNgramDecoder(tokens, NG.ArpaLM(rpath), lm_weight=0.5, beam_size=16, device=DEV).decode_spans(em, spans)
    assert torch.equal(mine[1], theirs[1]) and int(mine[1].max()) > 0
    lengths = mine[1].cpu().tolist()
    for b, n in enumerate(lengths):
        assert mine[0][b, :n].cpu().tolist() == theirs[0][b, :n].cpu().tolist()
    assert float((mine[2].double() - theirs[2].double()).abs().max()) <= TOL


# ---- refusals and the CLI ----------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sort_u64(torch.zeros((4,), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lm_tables(torch.tensor([1, 4, 2], dtype=torch.int32), 2, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lmtrain.train_ngram([["a"]], 2, device="cpu")
    many = [[f"w{i}" for i in range(300)]]                            # 303 ids: 9 bits, order 8 would take 72
    with pytest.raises(ValueError, match="must fit 64"):
        lmtrain.train_ngram(many, 8, device=DEV)
    with pytest.raises(ValueError, match="must fit 64"):
        ops.lm_tables(torch.tensor([1, 4, 2], dtype=torch.int32, device=DEV), 8, 9)
    with pytest.raises(ValueError, match="outside 1..8"):
        lmtrain.train_ngram([["a"]], 9, device=DEV)
    with pytest.raises(ValueError, match="empty corpus"):
        lmtrain.train_ngram([], 3, device=DEV)
    with pytest.raises(ValueError, match="whitespace"):
        lmtrain.train_ngram([["a", "b c"]], 3, device=DEV)
    with pytest.raises(ValueError, match="int64 or uint64"):
        ops.sort_u64(torch.zeros((4,), dtype=torch.int32, device=DEV))
    lmtrain.train_ngram(many, 7, device=DEV)                          # 63 bits: fits


def test_a_corpus_of_one_empty_line():
    m = lmtrain.train_ngram([[]], 3, device=DEV)
    ref = R.train([[]], 3)
    assert [tuple(m.vocab[i - 1] for i in g) for g in m.ids[1].cpu().tolist()] == [("<s>", "</s>")]
    assert m.fallback_orders == ref.fallback_orders == [1, 2, 3]
    for k, rows in enumerate(R.tables(ref)):
        for (g, rp, rb), p, b in zip(rows, m.logp[k].cpu().tolist(), m.bo[k].cpu().tolist()):
            assert abs(p - rp) <= TOL and abs(b - rb) <= TOL


def test_the_cli(tmp_path):
    text = tmp_path / "text.txt"
    text.write_text("\n".join(["the cat sat", "on the mat", "", "a cat's hat", "the hat sat", "that cat", "at the mat", "sat on a hat",
                               "the cat", "a mat"]) + "\n", encoding="utf-8")
    out, toks, lex = tmp_path / "lm.arpa", tmp_path / "tokens.txt", tmp_path / "words.txt"
    model = lmtrain.main(["--text", str(text), "--level", "char-word", "--order", "3", "--out", str(out), "--tokens-out", str(toks),
                          "--lexicon-out", str(lex), "--device", DEV])
    lm = NG.ArpaLM(str(out))
    assert lm.order == 3 and ("t", "h", "e") in lm.grams and ("<s>",) in lm.grams and lm.grams[("<s>",)][0] == -99.0
    assert lm.grams == model.to_arpa_lm().grams
    assert toks.read_text(encoding="utf-8").split("\n")[:-1] == model.vocab[3:] == sorted(set("thecatsonmat'") | {"'"})
    first = lex.read_text(encoding="utf-8").split("\n")[0]
    assert first == "the\t5"
    total = math.fsum(10.0 ** lm.score(("t", "h"), w) for w in model.vocab if w != "<s>")
    assert abs(total - 1.0) <= TOL
