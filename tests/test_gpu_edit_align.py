"""Device tests of the edit distance and alignment: dtlr_edit_align against the plain-Python reference of
tests/edit_align_ref.py -- every figure is an integer, every comparison exact -- then the public interface: evaluate_predictions on
the device against the host path, the confusion report, and one pass of the CLI."""
import json

import numpy as np
import pytest
import torch

from dtlr_amd import _lib, ops
from dtlr_amd import eval_harness as H
from dtlr_amd import evaluation as E
from tests import edit_align_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -77


def _run(A, B, want_ops=True, device=DEV, sentinel=False):
    """one ops.edit_align call over the pairs -> host (dist list, counts list of tuples, per-pair ops lists or None)"""
    a, a_off, b, b_off = ops.edit_align_tables(A, B)
    if sentinel:                                                      # what edit_align allocates, filled beforehand: see _raw
        return _raw(a, a_off, b, b_off, device)
    dist, counts, n_ops, steps = ops.edit_align(a.to(device), a_off, b.to(device), b_off, want_ops)
    assert dist.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(counts.shape) == (len(A), 3) and dist.device == torch.device(device)
    if not want_ops:
        assert n_ops is None and steps is None
        return dist.cpu().tolist(), [tuple(c) for c in counts.cpu().tolist()], None
    assert tuple(steps.shape) == (int(a_off[-1]) + int(b_off[-1]), 2) and steps.dtype == torch.int32 and n_ops.dtype == torch.int32
    return dist.cpu().tolist(), [tuple(c) for c in counts.cpu().tolist()], _cut(steps, n_ops, a_off, b_off)


def _cut(steps, n_ops, a_off, b_off):
    st, k, start = steps.cpu().tolist(), n_ops.cpu().tolist(), (a_off + b_off).tolist()
    return [[tuple(r) for r in st[start[p]: start[p] + k[p]]] for p in range(len(k))]


def _raw(a, a_off, b, b_off, device=DEV, want_ops=1):
    """the entry point itself on buffers filled with a sentinel -> host (dist, counts, ops lists), after checking that nothing past
    n_ops[p] was written"""
    n = int(a_off.numel()) - 1
    ad, bd, ao, bo = a.to(device), b.to(device), a_off.to(device), b_off.to(device)
    la, lb = (a_off[1:] - a_off[:-1]), (b_off[1:] - b_off[:-1])
    ma, mb = int(la.max()), int(lb.max())
    dist = torch.full((n,), SENTINEL, dtype=torch.int32, device=device)
    counts = torch.full((n, 3), SENTINEL, dtype=torch.int32, device=device)
    n_ops = torch.full((n,), SENTINEL, dtype=torch.int32, device=device)
    steps = torch.full((int(a_off[-1]) + int(b_off[-1]) + 4, 2), SENTINEL, dtype=torch.int32, device=device)
    L_ = _lib.lib()
    need = _lib.query(L_, "dtlr_edit_align_workspace_bytes", n, ma, mb)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.launch(L_, "dtlr_edit_align", ad.data_ptr(), ao.data_ptr(), bd.data_ptr(), bo.data_ptr(), n, ma, mb, want_ops, dist.data_ptr(),
                    counts.data_ptr(), n_ops.data_ptr(), steps.data_ptr(), ws.data_ptr(), need)
    st, k, start = steps.cpu(), n_ops.cpu().tolist(), (a_off + b_off).tolist()
    if not want_ops:
        assert bool((st == SENTINEL).all()) and all(v == SENTINEL for v in k)
        return dist.cpu().tolist(), [tuple(c) for c in counts.cpu().tolist()], None
    for p in range(n):
        assert bool((st[start[p] + k[p]: start[p + 1]] == SENTINEL).all()), p       # entries past n_ops[p] keep the sentinel
    assert bool((st[start[n]:] == SENTINEL).all())
    return dist.cpu().tolist(), [tuple(c) for c in counts.cpu().tolist()], [[tuple(r) for r in st[start[p]: start[p] + k[p]].tolist()] for p in range(n)]


def _same(got, ref, what=""):
    dist, counts, steps = got
    for p, (d, c, o) in enumerate(ref):
        assert dist[p] == d, (what, p, dist[p], d)
        assert counts[p] == tuple(c), (what, p, counts[p], c)
        if steps is not None:
            assert steps[p] == o, (what, p)


def test_the_golden_cases_in_one_launch():
    cases = R.golden_cases()
    assert len(cases) == 24
    A, B = [c[0] for c in cases], [c[1] for c in cases]
    got = _run(A, B)
    assert got[1] == [c[2] for c in cases]                           # the reference's own compute_edit_operations(gt, pred)
    _same(got, [R.align(a, b) for a, b in zip(A, B)], "golden")
    assert got[0] == [E.levenshtein(a, b) for a, b in zip(A, B)]


def test_seeded_pairs_in_one_launch_and_one_per_launch():
    """400 pairs, both lengths from {0, 1, 2, 3, 31 .. 33, 63 .. 66, 127 .. 129, 200} (the lane count, the band of 64 rows, the word of
    16 moves), alphabets of 2 and 3 (ties everywhere: the tie-break decides), 80 and 7357 symbols.  The same pairs alone give the same
    outputs: no pair depends on its neighbours or on where its slot of the workspace lies."""
    A, B = R.draw_pairs()
    ref = R.draw_pairs_ref()
    assert len(A) == 400 and {(len(a), len(b)) for a, b in zip(A, B)} >= {(x, y) for x in R.LENGTHS for y in R.LENGTHS}
    got = _run(A, B, sentinel=True)
    _same(got, ref, "batch")
    assert _run(A, B, want_ops=False)[:2] == got[:2]
    for p in range(400):
        _same(_run([A[p]], [B[p]]), [ref[p]], f"alone {p}")


def test_the_extremes():
    ex, ref = R.extremes(), R.extremes_ref()
    A, B = [a for _, a, _ in ex], [b for _, _, b in ex]
    assert {(len(a), len(b)) for a, b in zip(A, B)} >= {(900, 900), (1, 900), (900, 1), (0, 900), (0, 0), (4096, 7)}
    got = _run(A, B, sentinel=True)
    _same(got, ref, "extremes")
    names = [nm for nm, _, _ in ex]
    k = names.index("identical")
    assert got[0][k] == 0 and got[1][k] == (0, 0, 0) and got[2][k] == [(i, i) for i in range(len(A[k]))]
    k = names.index("disjoint")
    assert got[0][k] == len(A[k]) and got[1][k] == (0, len(A[k]) - len(B[k]), len(B[k]))
    k = names.index("0x0")
    assert got[0][k] == 0 and got[2][k] == []
    # code points: a str is packed as its code points, the supplementary planes included
    d, c, al = E.edit_align_batch(["naïve \U0010ffff!", ""], ["naive \U0010fffe!!", "ab"], DEV, True)
    assert d == [3, 2] and c == [(1, 0, 2), (2, 0, 0)] and al[1] == [(-1, 0), (-1, 1)]


def test_without_ops_nothing_else_is_touched():
    A, B = R.draw_pairs()
    A, B, ref = A[:60], B[:60], R.draw_pairs_ref()[:60]
    a, a_off, b, b_off = ops.edit_align_tables(A, B)
    _same(_raw(a, a_off, b, b_off, want_ops=0), ref)                 # n_ops, ops keep the sentinel
    # null n_ops / ops / workspace are accepted
    ad, bd, ao, bo = a.to(DEV), b.to(DEV), a_off.to(DEV), b_off.to(DEV)
    dist = torch.empty((60,), dtype=torch.int32, device=DEV)
    counts = torch.empty((60, 3), dtype=torch.int32, device=DEV)
    _lib.launch(_lib.lib(), "dtlr_edit_align", ad.data_ptr(), ao.data_ptr(), bd.data_ptr(), bo.data_ptr(), 60, 200, 200, 0, dist.data_ptr(),
                counts.data_ptr(), None, None, None, 0)
    assert dist.cpu().tolist() == [r[0] for r in ref] and [tuple(c) for c in counts.cpu().tolist()] == [tuple(r[1]) for r in ref]


def test_refusals_and_nothing_to_do():
    """argument checks: nothing is launched"""
    L_ = _lib.lib()
    a, a_off, b, b_off = ops.edit_align_tables([[1, 2, 3]], [[1, 3]])
    ad, bd, ao, bo = a.to(DEV), b.to(DEV), a_off.to(DEV), b_off.to(DEV)
    dist = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((1, 3), SENTINEL, dtype=torch.int32, device=DEV)
    n_ops = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    steps = torch.full((5, 2), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.empty((1024,), dtype=torch.uint8, device=DEV)

    def raw(n, ma, mb, want, nbytes):
        _lib.launch(L_, "dtlr_edit_align", ad.data_ptr(), ao.data_ptr(), bd.data_ptr(), bo.data_ptr(), n, ma, mb, want, dist.data_ptr(),
                    counts.data_ptr(), n_ops.data_ptr(), steps.data_ptr(), ws.data_ptr(), nbytes)

    assert _lib.query(L_, "dtlr_edit_align_workspace_bytes", 1, 3, 2) == 128
    for args in ((1, 4097, 2, 1, 1 << 30), (1, 3, 4097, 0, 0), (1, 3, 2, 1, 127), (1, 3, 2, 1, 0)):
        with pytest.raises(_lib.DTLRError, match="code -3"):
            raw(*args)
    raw(0, 3, 2, 1, 0)                                                # n = 0: nothing is done
    _lib.launch(L_, "dtlr_edit_align", None, None, None, None, 0, 0, 0, 1, None, None, None, None, None, 0)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (dist, counts, n_ops, steps))
    raw(1, 3, 2, 1, 128)
    assert dist.item() == 1 and counts.cpu().tolist() == [[0, 1, 0]] and n_ops.item() == 3
    assert steps.cpu().tolist()[:3] == [[0, 0], [1, -1], [2, 1]] and bool((steps[3:] == SENTINEL).all())
    # the binding: refused on the host before any device work; nothing to do is an empty result
    with pytest.raises(ValueError, match="limit is 4096"):
        ops.edit_align(torch.zeros(4097, dtype=torch.int32, device=DEV), torch.tensor([0, 4097]), bd, torch.tensor([0, 2]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.edit_align(a, a_off, b, b_off)
    e = torch.empty((0,), dtype=torch.int32, device=DEV)
    d, c, k, st = ops.edit_align(e, torch.zeros(1, dtype=torch.int64), e, torch.zeros(1, dtype=torch.int64))
    assert tuple(d.shape) == (0,) and tuple(c.shape) == (0, 3) and tuple(k.shape) == (0,) and tuple(st.shape) == (0, 2)
    assert E.edit_distances([], [], DEV) == []


def test_several_launches_under_a_small_workspace_limit(monkeypatch):
    """the pairs cut into launches (here by a limit of 64 KiB): the same outputs as in one launch"""
    from dtlr_amd import metrics
    A, B = R.draw_pairs()
    A, B, ref = A[:120], B[:120], R.draw_pairs_ref()[:120]
    monkeypatch.setattr(metrics, "EDIT_WORKSPACE_LIMIT", 64 << 10)
    _, a_off, _, b_off = ops.edit_align_tables(A, B)
    assert len(metrics.edit_align_chunks(a_off, b_off)) >= 4
    _same(_run(A, B), ref, "chunks")


def test_a_side_stream():
    A, B = R.draw_pairs()
    A, B, ref = A[200:260], B[200:260], R.draw_pairs_ref()[200:260]
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got = _run(A, B)
    s.synchronize()
    _same(got, ref, "stream")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="one device")
def test_a_second_device():
    """the tensors' device, not the current one, takes the launch (@_lib.op)"""
    A, B = R.draw_pairs()
    A, B, ref = A[200:260], B[200:260], R.draw_pairs_ref()[200:260]
    assert torch.cuda.current_device() == 0
    _same(_run(A, B, device="cuda:1"), ref, "cuda:1")
    _same(_run(A, B, device="cuda:1", sentinel=True), ref, "cuda:1 raw")


CHARSET = [chr(ord("a") + i) for i in range(26)] + list("ABCDEFGH0123456789.,-'") + [" "]
MODES = [("default", "IAM"), ("default", "HWDB"), ("CER_only", "RIMES"), ("CER_only", "other"), ("chinese", "HWDB"), ("chinese", "READ"),
         ("cipher", "borg"), ("cipher", "IAM")]


@pytest.mark.parametrize("metrics,dataset", MODES)
def test_evaluate_predictions_on_the_device_equals_the_host_path(metrics, dataset):
    """64 synthetic lines: an empty prediction, a skipped line, and one line of 4100 characters that is above the device's limit and
    takes the host route"""
    preds, texts = R.draw_lines(11, 64, CHARSET, 20, 60, long_line=4100)
    assert preds[1] == [] and preds[2] is None and len(texts[3]) == 4100 > ops.EDIT_MAX_LEN
    host = H.evaluate_predictions(preds, texts, CHARSET, dataset, metrics)
    dev = H.evaluate_predictions(preds, texts, CHARSET, dataset, metrics, device=DEV)
    assert dev == host and len(host["CER_list"]) == 63
    rep = E.ConfusionReport()
    assert H.evaluate_predictions(preds, texts, CHARSET, dataset, metrics, device=DEV, confusion=rep) == host


def test_the_confusion_report_of_the_device_equals_the_references():
    preds, texts = R.draw_lines(12, 64, CHARSET, 20, 60, edit=0.15, long_line=4100)
    dev, host, want = E.ConfusionReport(), E.ConfusionReport(), E.ConfusionReport()
    H.evaluate_predictions(preds, texts, CHARSET, "IAM", "CER_only", device=DEV, confusion=dev)
    H.evaluate_predictions(preds, texts, CHARSET, "IAM", "CER_only", confusion=host)
    tot = [0, 0, 0]
    for p, t in zip(preds, texts):
        if p is None:
            continue
        gt = [CHARSET.index(c) for c in t]
        _, c, steps = R.align(gt, p)
        want.add_alignment(gt, p, steps)
        tot = [x + y for x, y in zip(tot, c)]
    assert dev == want and host == want and dev.lines == 63
    t = dev.totals()
    assert [t["ins"], t["del"], t["sub"]] == tot and t["n"] == sum(len(x) for p, x in zip(preds, texts) if p is not None)
    assert t["correct"] == t["n"] - t["del"] - t["sub"] and min(tot) > 0
    assert dev.to_json(CHARSET, 10) == want.to_json(CHARSET, 10)


def test_cli_device_metrics_and_confusion_out(tmp_path, capsys):
    """`--device-metrics --confusion-out`: the stats files are those of the same pass without the flags; the report's totals are the
    sums of the per-line operations"""
    from PIL import Image
    from dtlr_amd import weights
    from dtlr_amd.config import DTLRConfig
    from tests.util import preproc_image
    cs = H.load_charset(None)
    cfg = DTLRConfig.tiny(num_classes=len(cs))
    torch.save({"model": weights.synthetic_state_dict(cfg, 6), "epoch": 3}, tmp_path / "checkpoint.pth")
    img_dir = tmp_path / "lines"
    img_dir.mkdir()
    for k, (h, w) in enumerate([(40, 300), (33, 410), (40, 300)]):
        Image.fromarray(preproc_image(h, w, 20 + k), "RGB").save(img_dir / f"l{k:02d}.png")
    texts = ["hello world", "x - y", "abc def"]
    (tmp_path / "labels.json").write_text(json.dumps([[f"l{k:02d}", t] for k, t in enumerate(texts)]))
    base = ["--config", "tiny", "--weights", str(tmp_path / "checkpoint.pth"), "--images", str(img_dir), "--labels",
            str(tmp_path / "labels.json"), "--dataset", "IAM", "--dtype", "f32", "--batch", "2", "--size", "32", "--max_size", "256"]
    plain = H.main(base + ["--out", str(tmp_path / "plain")])
    dev = H.main(base + ["--out", str(tmp_path / "dev"), "--confusion-out", str(tmp_path / "conf.json"), "--confusion-top", "5"])
    only = H.main(base + ["--out", str(tmp_path / "only"), "--device-metrics"])
    assert "confusion report of 3 lines" in capsys.readouterr().err
    assert dev == plain and only == plain
    for name in ("cer_list.npy", "dict_char.json", "list_preds.txt", "list_gt.txt", "cer_TH_None_NMS_None.txt"):
        want = (tmp_path / "plain" / "IAM" / name).read_bytes()
        assert (tmp_path / "dev" / "IAM" / name).read_bytes() == want and (tmp_path / "only" / "IAM" / name).read_bytes() == want, name
    obj = json.loads((tmp_path / "conf.json").read_text(encoding="utf-8"))
    index = {}
    for i, c in enumerate(cs):
        index.setdefault(str(c), i)
    tot = np.zeros(3, dtype=np.int64)
    for t, p in zip(texts, plain["list_preds_str"]):
        tot += np.array(E.compute_edit_operations([index[c] for c in t], [index[c] for c in p]))
    assert [obj["totals"][k] for k in ("ins", "del", "sub")] == tot.tolist() and obj["totals"]["lines"] == 3
    assert obj["totals"]["n"] == sum(len(t) for t in texts) and all(len(obj[k]) <= 5 for k in ("substitutions", "deletions", "insertions", "characters"))
