"""CPU tests of the CTC forced alignment: the reference (tests/ctc_align_ref.py) against an exhaustive search,
against the forward sum and the real criterion's recorded loss, the greedy property, the boundary (symbols, the wrapper's host
checks), the switch that leaves the n-gram located objects alone, and the int32 record of an aligned line with its SUM merge at gloo
world size 2."""
import dataclasses
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_cases():
    """(E [F, V], labels, interleaved): 64 seeded tiny spans, both modes, L in 0..3, repeated labels and infeasible ones included"""
    cases = []
    for seed in range(32):
        g = np.random.Generator(np.random.PCG64(120000 + seed))
        for interleaved in (False, True):
            F = int(g.integers(1, 4 if interleaved else 6))
            V = int(g.integers(2, 5))
            L = seed % 4
            E = g.uniform(0.01, 0.99, (F, V)).astype(np.float32)
            z = g.integers(1, V, L).tolist()
            if L >= 2 and seed % 3 == 0:
                z[1] = z[0]                                       # a repeated label: needs a blank between
            cases.append((E, z, interleaved))
    return cases


def test_viterbi_equals_the_exhaustive_search():
    cases = _tiny_cases()
    assert len(cases) >= 48
    seen = dict(feasible=0, infeasible=0, repeat=0)
    for E, z, inter in cases:
        v = R.viterbi(E, z, inter)
        score, states = R.exhaustive(E, z, inter)
        assert v.states == states, (E.shape, z, inter)
        if states is None:
            assert v.score == R.NEG and score == R.NEG and v.length == -1 and not v.feasible
            seen["infeasible"] += 1
            continue
        assert abs(v.score - score) <= 1e-12 and v.margin > 0, (E.shape, z, inter, v.score, score)
        seen["feasible"] += 1
        seen["repeat"] += len(z) >= 2 and z[0] == z[1]
        for i in range(len(z)):                                   # the records restate the states
            js = [j for j, s in enumerate(states) if s == 2 * i + 1]
            real = [j // 2 if inter else j for j in js]
            assert (v.first[i], v.last[i]) == (real[0], real[-1]) and v.peak[i] in real
    assert min(seen.values()) >= 3, seen
    for inter in (False, True):                                   # the empty span
        assert R.viterbi(np.zeros((0, 3), np.float32), [], inter).score == 0.0
        assert R.viterbi(np.zeros((0, 3), np.float32), [1], inter).length == -1
    # ties: equal candidates take the smallest shift; equal ends take state 2L - 1; equal peaks the earliest frame
    E = np.full((3, 2), 0.5, dtype=np.float32)
    assert R.viterbi(E, [1], False).states == [1, 1, 1]
    assert R.viterbi(E, [1], False).peak[0] == 0


def test_score_is_below_the_forward_sum_and_the_lattice_is_the_criterions(golden_dir):
    from oracle import dtlr_oracle as O
    from tests.util import ctc_case
    for E, z, inter in _tiny_cases():
        assert R.viterbi(E, z, inter).score <= R.total(E, z, inter) + 1e-12
    g = np.load(os.path.join(golden_dir, "g5_ctc.npz"))
    for k, (seed, B, nq, C, bias, lmax) in enumerate(g["cases"].tolist()):
        outputs, labels = ctc_case(int(seed), int(B), int(nq), int(C), bias, int(lmax))
        probs = O.blank_probabilities(outputs, 0.003).numpy()     # [B, nq, C + 1], reading order, blank first
        nll = []
        for b in range(int(B)):
            z = [int(v) + 1 for v in labels[b]]
            t = R.total(probs[b], z, True)
            assert R.viterbi(probs[b], z, True).score <= t + 1e-12
            nll.append(0.0 if not np.isfinite(t) else -t / max(len(z), 1))          # zero_infinity, reduction "mean"
        got, want = float(np.mean(nll)), float(g[f"loss_{k}"])
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (k, got, want)


@pytest.mark.parametrize("seed,T,V", [(1, 7, 5), (2, 40, 24), (3, 120, 167)])
def test_greedy_property(seed, T, V):
    """interleaved: the un-collapsed frame-wise argmax string aligns to exactly the argmax frames, with the sum of the log maxima"""
    from tests.ngram_beam_ref import emissions
    E = emissions(seed, T, V)
    am = E.argmax(-1)
    frames = np.nonzero(am)[0]
    v = R.viterbi(E, am[frames].tolist(), True)
    assert v.feasible and np.array_equal(v.first, frames) and np.array_equal(v.last, frames) and np.array_equal(v.peak, frames)
    assert np.array_equal(v.prob, E[frames, am[frames]])
    want = float(np.log(E.max(-1).astype(np.float64)).sum())
    assert abs(v.score - want) <= 1e-12 * max(1.0, abs(want))


def test_symbols_are_declared_and_the_wrapper_checks_its_tables():
    from dtlr_amd import _lib, ops
    for name in ("dtlr_ctc_align", "dtlr_ctc_align_workspace_bytes", "dtlr_reading_order"):
        assert name in _lib._SIGNATURES, name                         # read from include/dtlr_hip.h
    for name in ("ctc_align", "reading_order"):
        assert hasattr(getattr(ops, name), "__wrapped__"), name
    B, T, V = 2, 10, 6
    ok = ops.ctc_align_tables([(0, 0, 10), (1, 3, 3)], [[1, 5, 2], [3, 0, 99]], [3, 1], B, T, V)     # padding is not checked
    assert [tuple(t.shape) for t in ok] == [(2, 3), (2, 3), (2,)]
    for spans in ([(0, 0, 11)], [(0, -1, 4)], [(2, 0, 4)], [(-1, 0, 4)], [(0, 5, 4)]):
        with pytest.raises(ValueError):
            ops.ctc_align_tables(spans, [[1]], [1], B, T, V)
    for label in (0, V, -3):
        with pytest.raises(ValueError):
            ops.ctc_align_tables([(0, 0, 10)], [[1, label]], [2], B, T, V)
    with pytest.raises(ValueError):
        ops.ctc_align_tables([(0, 0, 10)], [[1] * 512], [512], B, T, V)               # 1025 states
    ops.ctc_align_tables([(0, 0, 10)], [[1] * 511], [511], B, T, V)                   # 1023 states
    with pytest.raises(ValueError):
        ops.ctc_align_tables([(0, 0, 10)], [[1, 2]], [3], B, T, V)                    # a length beyond the row
    with pytest.raises(ValueError):
        ops.ctc_align_tables([(0, 0, 10)], [[1, 2]], [2, 2], B, T, V)


def test_the_switch_is_off_by_default_and_adds_nothing():
    from dtlr_amd import evaluation as E
    from dtlr_amd import ngram as NG
    from dtlr_amd import eval_harness as H
    from tests.test_located_host import _sample_lines
    assert inspect.signature(NG.rescored_located_batch).parameters["align_rewritten"].default is False
    assert inspect.signature(H.predict_located).parameters["align_rewritten"].default is False
    c = E.LocatedChar(3, 0.5, (0.0, 1.0, 2.0, 3.0), 7, 4)
    w = E.LocatedWord([3], (0.0, 1.0, 2.0, 3.0), 0.5, (0, 1), "ngram", False)
    line = E.LocatedLine([3], [c], [w], "ngram")
    assert (c.first, c.last, w.aligned, line.logp) == (None, None, None, None)       # the old constructions, the new fields at rest
    assert [f.name for f in dataclasses.fields(E.LocatedWord)][:6] == ["labels", "box", "score", "chars", "source", "same"]
    cs = list("a bcdefgh")
    for ln in _sample_lines():
        obj = E.located_line_to_json(ln, cs, "x")
        assert set(obj) == {"id", "decoder", "text", "chars", "words"}
        assert all(set(d) == {"c", "label", "score", "box", "query"} for d in obj["chars"])
        assert all(set(d) <= {"text", "box", "score", "chars", "source"} for d in obj["words"])
    before = E.located_line_to_json(line, cs, "x")
    w.aligned = [dataclasses.replace(c, first=4, last=5)]
    after = E.located_line_to_json(line, cs, "x")
    assert set(after["words"][0]) == set(before["words"][0]) | {"aligned"}
    assert after["words"][0]["aligned"] == [dict(before["chars"][0], rank=4, first=4, last=5)]
    del after["words"][0]["aligned"]
    assert after == before


def _aligned_lines():
    from dtlr_amd import evaluation as E
    ch = [E.LocatedChar(2, 0.75, (-0.0, 1.5, 2.0, 3.0), 5, 0, 0, 1), E.LocatedChar(1, float(np.float32(1e-5)), (-3.0, 0.0, 4.0, 1.0), 0, 2, 2, 2),
          E.LocatedChar(0, 0.5, (4.0, 0.0, 5.0, 1.0), 3, 4, 3, 4)]
    full = E.LocatedLine([2, 1, 0], ch, E.located_words(ch, 1), "align", -12.345678901234567)
    none = E.LocatedLine([4, 4], [], [], "align", float("-inf"))
    empty = E.LocatedLine([], [], [], "align", -0.25)
    return full, none, empty


def test_pack_and_unpack_an_aligned_line(tmp_path):
    from dtlr_amd import evaluation as E
    from dtlr_amd import eval_harness as H
    for line in _aligned_lines():
        row = H.pack_aligned(line, 4)
        assert row.dtype == np.int32 and row.shape == (H.aligned_row_width(4),)
        assert H.unpack_aligned(row, 4, line.labels, 1) == line
    with pytest.raises(ValueError):
        H.pack_aligned(_aligned_lines()[0], 2)
    # an n-gram line whose rewritten word carries aligned characters
    from tests.test_located_host import _sample_lines
    ng = _sample_lines()[2]
    ng.words[-1].aligned = [E.LocatedChar(2, 0.25, (-1.0, 0.0, 2.0, 6.0), 3, 7, 7, 7), E.LocatedChar(2, 0.5, (2.0, 0.0, 5.0, 6.0), 1, 9, 8, 9)]
    ng.words[0].aligned = []
    row = H.pack_located(ng, 6, True, True)
    assert row.shape == (H.located_row_width(6, True, True),) and H.unpack_located(row, 6, True, "ngram", None, True) == ng
    cs = list("a bcdefgh")
    path = tmp_path / "a.jsonl"
    assert H.write_aligned(str(path), ["l0", "l1", "l2", "l3"], list(_aligned_lines()) + [None], cs) == 3
    rows = [json.loads(s) for s in path.read_text(encoding="utf-8").splitlines()]
    assert [r["decoder"] for r in rows] == ["align"] * 3 and [r["feasible"] for r in rows] == [True, False, True]
    assert rows[0]["logp"] == -12.345678901234567 and rows[1]["logp"] is None and rows[1]["chars"] == []
    assert set(rows[0]) == {"id", "decoder", "text", "chars", "words", "logp", "feasible"}
    assert set(rows[0]["chars"][0]) == {"c", "label", "score", "box", "query", "rank", "first", "last"}
    assert H.transcript_labels(["ab", "a?"], cs) == [[0, 2], None]


_WORKER = r"""
import os, sys, torch, numpy as np
sys.path.insert(0, {root!r})
from dtlr_amd import dist as D
from dtlr_amd import eval_harness as H
from tests.test_ctc_align_host import _aligned_lines
rank, local, world = D.init_from_env("gloo")
full, none, empty = _aligned_lines()
lines, K = [full, none, empty, full, none], 4
n = len(lines)
packed = torch.stack([torch.from_numpy(H.pack_aligned(l, K)) for l in lines])
rows = torch.zeros_like(packed)
status = torch.full((n,), -1, dtype=torch.int32)
lo, hi = D.shard_bounds(n, rank, world)
rows[lo:hi] = packed[lo:hi]
status[lo:hi] = 0
merged, st = H.merge_located(rows, status)
assert torch.equal(merged, packed) and st.tolist() == [0] * n, rank           # bit for bit: the fp64 halves, -0.0 and negative coordinates
assert (packed[0] < 0).any() and (packed[0] == -2 ** 31).any()
for i, l in enumerate(lines):
    assert H.unpack_aligned(merged[i].numpy(), K, l.labels, 1) == l
D.barrier()
open(os.path.join({out!r}, f"rank{{rank}}.ok"), "w").write("ok")
D.finalize()
"""


def test_aligned_merge_world_size_2_gloo(tmp_path):
    """The int32 row of an aligned line -- the new int32 columns, the fp32 columns and the fp64 log-probability as two halves -- comes
    back bit for bit through the zero-fill + all_reduce(SUM) merge."""
    script = tmp_path / "w.py"
    script.write_text(_WORKER.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29643")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29643", str(script)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists()
