"""The host side of the fused value + [offsets | logits] projection (dtlr_gemm_k256 with N = 640): the entry point's argument checks, the
weight image ops.gemm_k256_vow hands it, and the engine taking it exactly where the two launches ran."""
import ctypes

import torch


def test_the_header_gained_no_entry_point():
    """the fused form is a form of dtlr_gemm_k256: no symbol of its own, in the header or in the libraries"""
    from dtlr_amd import _lib, build
    assert not any("vow" in name for name in _lib.declared_symbols())
    build.build(verbose=False)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        assert not hasattr(ctypes.CDLL(path), "dtlr_gemm_k256_vow"), path


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """N = 640: a missing residual, a row mask, a short row stride and shapes the kernel does not take come back as error codes (nothing
    is enqueued: no GPU needed); the other widths are still refused"""
    from dtlr_amd import _lib, build
    build.build(verbose=False)
    L = ctypes.CDLL(_lib.LIB_PATH)
    f = L.dtlr_gemm_k256
    f.restype, f.argtypes = _lib._SIGNATURES["dtlr_gemm_k256"]
    q = 4096                                                     # any non-null address: never dereferenced on these paths
    #        A  Wp bias resid rows mask C  ldc  M   N   stream
    assert f(q, q, None, None, 64, None, q, 256, 64, 640, None) == _lib.DTLR_EINVAL          # no residual
    assert f(q, q, None, q, 0, None, q, 256, 64, 640, None) == _lib.DTLR_EINVAL
    assert f(q, q, None, q, 64, q, q, 256, 64, 640, None) == _lib.DTLR_EINVAL                # a row mask: padded batches take the two launches
    assert f(q, q, None, q, 64, None, q, 248, 64, 640, None) == _lib.DTLR_EINVAL             # ldc < 256
    assert f(q, q, None, q, 64, None, q, 260, 64, 640, None) == _lib.DTLR_EINVAL             # ldc not a multiple of 8
    assert f(q, q, None, q, 96, None, q, 256, 192, 640, None) == _lib.DTLR_ESHAPE            # res_rows not a multiple of 64
    assert f(q, q, None, q, 128, None, q, 256, 192, 640, None) == _lib.DTLR_ESHAPE           # M not a multiple of res_rows
    assert f(q, q, None, None, 0, None, q, 512, 64, 512, None) == _lib.DTLR_ESHAPE           # N = 512: still no such width


def test_the_two_images_are_joined_once_per_pair():
    from dtlr_amd import ops
    wv, wo = torch.arange(256 * 256, dtype=torch.float32).to(torch.bfloat16), torch.ones(384 * 256, dtype=torch.bfloat16)
    a = ops._vow_image(wv, wo)
    assert a.numel() == 640 * 256 and torch.equal(a[:256 * 256], wv) and torch.equal(a[256 * 256:], wo)
    assert ops._vow_image(wv, wo) is a
    wo.mul_(2)                                                   # written in place: joined again
    b = ops._vow_image(wv, wo)
    assert b is not a and torch.equal(b[256 * 256:], wo)
    assert ops._vow_image(wv.clone(), wo) is not b               # another tensor, equal or not: its own entry


class _Stop(Exception):
    pass


def _engine_stub(use_fused, dtype=torch.bfloat16, S=128, B=2, has_padding=False, use_kres=True):
    from dtlr_amd.config import DTLRConfig
    from dtlr_amd.engine import DTLREngine
    eng = DTLREngine.__new__(DTLREngine)
    eng.cfg = DTLRConfig.latin()
    eng.w = {"enc0.attn.ow.w": torch.zeros((384, 256), dtype=dtype), "enc0.attn.value.w": torch.zeros((256, 256), dtype=dtype),
             "enc0.attn.value.b": torch.zeros((256,))}
    eng.use_k256, eng.use_kres, eng.split, eng.use_k256s, eng.use_k256s_multi_enc = True, use_kres, False, False, False
    eng.use_k256_fused = use_fused
    src = torch.zeros((B, S, 256), dtype=dtype)
    ow_res = None if has_padding else torch.zeros((S, 384), dtype=dtype)
    g = {"has_padding": has_padding, "mask_flat": None}
    return eng, src, ow_res, g


def _first_projection(monkeypatch, **kw):
    """the name of the first projection operator DTLREngine._msda_module reaches, and the image kinds it asked for"""
    from dtlr_amd import ops
    from dtlr_amd.engine import DTLREngine
    eng, src, ow_res, g = _engine_stub(**kw)
    asked = []
    monkeypatch.setattr(DTLREngine, "_image", lambda self, kind, name: (asked.append((kind, name)), torch.zeros(1))[1])
    monkeypatch.setattr(DTLREngine, "_has_image", lambda self, kind, name: False)

    def stop(name):
        def f(*a, **k):
            raise _Stop(name)
        return f
    for name in ("gemm_k256_vow", "gemm_k256", "gemm_kres_bcast384", "gemm_k256s", "linear", "linear_resbcast"):
        monkeypatch.setattr(ops, name, stop(name))
    try:
        eng._msda_module("enc0.attn", src, None, None, src, g, 4, ow_res=ow_res)
    except _Stop as e:
        return str(e), asked
    raise AssertionError("no projection operator was reached")


def test_engine_takes_the_fused_launch_only_where_the_two_launches_ran(monkeypatch):
    op, asked = _first_projection(monkeypatch, use_fused=1)
    assert op == "gemm_k256_vow" and asked == [("k256", "enc0.attn.value"), ("k256", "enc0.attn.ow")]
    assert _first_projection(monkeypatch, use_fused=0)[0] == "gemm_k256"                      # the flag off: the parent's sequence
    assert _first_projection(monkeypatch, use_fused=1, S=680)[0] == "gemm_k256"               # S % 64 != 0
    assert _first_projection(monkeypatch, use_fused=1, has_padding=True)[0] == "gemm_k256"    # padded batch: no row-broadcast term
    assert _first_projection(monkeypatch, use_fused=1, use_kres=False)[0] == "gemm_k256"


def test_flag_defaults_on():
    import inspect
    from dtlr_amd.engine import DTLREngine
    assert "self.use_k256_fused = 1" in inspect.getsource(DTLREngine.__init__)
