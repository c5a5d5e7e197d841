"""CPU tests of the n-gram beam decoder's host side: the reference search against exhaustive enumeration, the packed LM trie against
ArpaLM.score, and the new command-line flags."""
import itertools

import pytest

from tests import ngram_beam_ref as R


def _small_cases():
    cases = []
    for seed in range(48):
        T, V = 3 + seed % 4, 3 + seed % 2
        with_lm = seed % 3 != 0
        cases.append((seed, T, V, with_lm, bool(seed & 4), bool(seed & 8)))
    return cases


def test_reference_search_equals_exhaustive_enumeration():
    """Reference (a) with a beam that never cuts == oracle (b): same label sequence, score within 1e-9, on 48 seeded cases
    (T 3..6, V 3..4, with and without LM, bos / eos both ways)."""
    seen = set()
    for seed, T, V, with_lm, bos, eos in _small_cases():
        E = R.emissions(seed, T, V)
        tokens = R.token_table(V)
        lm = R.RefLM(R.random_arpa(seed, tokens, 1 + seed % 3, per_order=12, drop=seed % 2)) if with_lm else None
        w = (0.25, 1.0)[seed % 2]
        want_seq, want_score, table = R.exhaustive(E, lm, tokens, w, bos, eos)
        got_seq, got_score, cut, _ = R.beam_search(E, K=len(table) + 1, N=None, lm=lm, tokens=tokens, w=w, bos=bos, eos=eos)
        assert cut == float("inf")
        assert got_seq == want_seq, (seed, got_seq, want_seq)
        assert abs(got_score - want_score) <= 1e-9, (seed, got_score, want_score)
        seen.add((T, V, with_lm, bos, eos))
    assert {c[0] for c in seen} == {3, 4, 5, 6} and {c[1] for c in seen} == {3, 4}
    assert {c[2:] for c in seen} >= set(itertools.product((True,), (False, True), (False, True))) and any(not c[2] for c in seen)


@pytest.mark.parametrize("order", [1, 2, 3, 6])
def test_pack_lm_round_trip(tmp_path, order):
    """Walking the packed trie reproduces ArpaLM.score for every context shorter than the order and every token: unknown tokens,
    contexts that exist only as suffixes or only inside longer n-grams, <s> in front, </s> as the predicted word."""
    from dtlr_amd import ngram as NG
    tokens = R.token_table(6) + [" "]                      # " " is the LM's <space>
    text = R.random_arpa(order, tokens, order, per_order=60, drop=1)
    (tmp_path / "lm.arpa").write_text(text)
    lm = NG.ArpaLM(str(tmp_path / "lm.arpa"))
    assert lm.order == order
    P = NG.pack_lm(lm, tokens)
    V = len(tokens)
    assert P["vocab"] == V and P["eos_tok"] == V + 1 and P["has_bos"] and P["has_eos"]
    n = P["tok"].numel()
    for k in ("child_lo", "child_hi", "suffix", "ctx", "logp", "bo"):
        assert P[k].numel() == n
    for s in range(n):                                      # children sorted by token, ranges inside the table
        lo, hi = int(P["child_lo"][s]), int(P["child_hi"][s])
        assert 0 <= lo <= hi <= n
        ch = P["tok"][lo:hi].tolist()
        assert ch == sorted(set(ch))
    word = lambda c: "<s>" if c == V else "</s>" if c == V + 1 else NG._lm_word(tokens[c])       # noqa: E731
    checked = 0
    for L in range(0, max(order, 2)):
        firsts = list(range(1, V)) + [V]
        for ctx in itertools.product(*([firsts] + [list(range(1, V))] * (L - 1))) if L else [()]:
            state = NG.lm_state(P, ctx)
            for c in list(range(1, V)) + [V + 1]:
                got, new_state = NG.lm_walk(P, state, c)
                want = lm.score(tuple(word(x) for x in ctx), word(c))
                assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (ctx, c, got, want)
                if c <= V:
                    assert new_state == NG.lm_state(P, tuple(ctx) + (c,))
                checked += 1
    assert checked > 50
    # a token the LM does not hold (dropped from the table) scores <unk> behind the context's back-offs
    assert ("a",) not in lm.grams and abs(NG.lm_walk(P, 0, 1)[0] - lm.grams[("<unk>",)][0]) < 1e-12


def test_cli_flags_and_defaults(tmp_path):
    """build_parser() takes the n-gram flags; without --ngram-arpa the harness builds no decoder bundle."""
    import inspect
    from dtlr_amd import eval_harness as H
    ap = H.build_parser()
    a = ap.parse_args(["--images", "x", "--labels", "y"])
    assert a.ngram_arpa is None and a.ngram_weight == 0.25 and a.ngram_beam == 50 and a.ngram_beam_token is None
    assert a.ngram_tokens is None and a.ngram_ignore is None and a.multiply_pred_logits_by == 1.0
    assert not a.no_uppercase_words and not a.no_digits and not a.no_dash
    assert H.ngram_bundle(a, ["a", "b", " "], "cpu") is None
    b = ap.parse_args(["--images", "x", "--labels", "y", "--ngram-arpa", "lm.arpa", "--ngram-weight", "0.5", "--ngram-beam", "32",
                       "--ngram-beam-token", "8", "--ngram-ignore", " .", "--no_uppercase_words", "--no_digits", "--no_dash",
                       "--multiply_pred_logits_by", "2.0", "--ngram-tokens", "t.txt"])
    assert (b.ngram_arpa, b.ngram_weight, b.ngram_beam, b.ngram_beam_token, b.ngram_ignore) == ("lm.arpa", 0.5, 32, 8, " .")
    assert b.no_uppercase_words and b.no_digits and b.no_dash and b.multiply_pred_logits_by == 2.0 and b.ngram_tokens == "t.txt"
    assert inspect.signature(H.predict_labels).parameters["ngram"].default is None
    # a token table that repeats a token, or a never-rescored character outside the charset, is a usage error
    (tmp_path / "dup.txt").write_text("<ctc>\na\na\n<space>\n")
    bad = ap.parse_args(["--images", "x", "--labels", "y", "--ngram-arpa", "none.arpa", "--ngram-tokens", str(tmp_path / "dup.txt")])
    with pytest.raises(SystemExit, match="repeated"):
        H.ngram_bundle(bad, ["a", "b", " "], "cpu")
    bad = ap.parse_args(["--images", "x", "--labels", "y", "--ngram-arpa", "none.arpa", "--ngram-ignore", " ?"])
    with pytest.raises(SystemExit, match="not in the charset"):
        H.ngram_bundle(bad, ["a", "b", " "], "cpu")
    # the defaults of the token table and of the never-rescored characters
    cs = ["a", "B", "1", " ", "'", "-", ".", ","]
    assert H.default_ngram_tokens(cs) == ["<ctc>", "a", "B", "1", "<space>", "'", "-", ".", ","]
    assert H.default_ngram_ignore(cs) == [4, 6, 7, 8]


def test_batch_assembly_equals_per_line_assembly():
    """The refactored assembly behind get_word_per_word_pred / _2 and the batch path give the same strings with a fake decoder."""
    import torch
    from dtlr_amd import ngram as NG
    from oracle import dtlr_oracle as O
    from tests.util import fake_ctc_decoder, ngram_case
    for seed in range(6):
        outputs, charset, ngc, ign = ngram_case(seed)
        new = O.ngram_new_pred_logits(outputs)
        labels = new[0].argmax(-1).tolist()
        dec = fake_ctc_decoder(ngc)
        span = lambda lo, hi: dec(new[0, lo:hi][None])[0][0].words                                 # noqa: E731
        assert NG._join(NG._assemble_words(labels, ign, span), charset, 1) == O.ngram_word_per_word_pred(new, dec, ign, charset)
        for up, dg, ds in ((True, False, True), (False, True, True), (True, True, False)):
            assert NG._join(NG._assemble_words_2(labels, ign, ngc, up, dg, ds, span), ngc, 0) == \
                O.ngram_word_per_word_pred_2(new, dec, ign, ngc, up, dg, ds)
    assert isinstance(torch.zeros(1), torch.Tensor)
