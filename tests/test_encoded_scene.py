"""Encode-once ABI (rf_scene_kv, rf_decoder_desc.kv_all): argument validation and workspace sizing, before any
launch, so no GPU is needed."""
import ctypes
import os

import pytest


def _lib():
    import torch  # noqa: F401
    from renderformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librfhip.so not built (run __graft_entry__.build())")
    return _lib, _lib.load(require_device=False)


def _decoder_good():
    """The `good` descriptor of test_decoder_forward_validates_before_any_launch, and its out-of-order taps."""
    from renderformer_amd import _lib
    layers = (_lib.DecoderLayer * 2)()
    for L in layers:
        L.query_norm = L.w_q = L.w_out = L.ffn_norm = L.w13 = L.w2 = 256
    taps = (_lib.DecoderTap * 2)()
    taps[0].layer, taps[0].p_hi, taps[0].p_ld = 1, 256, 1024
    taps[1].layer, taps[1].p_hi, taps[1].p_ld = 0, 256, 1024  # out of layer order
    good = dict(n_layers=2, rows=4096, dim=1024, n_heads=8, ffn_dim=4096, operand_dtype=1, eps=1e-6,
                layers=ctypes.addressof(layers), ctx=256, ld_ctx=1024, ctx_rows=5649, ctx_dim=1024, ctx_norm=256,
                w_kv_all=256, kv_rows=5649, kv_src_rows=256, k_batch=1, cross_problems=256, n_cross=1,
                workspace=256, attn_ws=256)
    return good, layers, taps


def test_scene_kv_validates_before_any_launch():
    """rf_scene_kv rejects each bad argument with RF_ERR_INVALID and a message that names it."""
    _l, lib = _lib()
    assert "rf_scene_kv" in _l.SIGNATURES and hasattr(lib, "rf_scene_kv")
    good = dict(ctx=256, ld_ctx=1024, ctx_rows=77, ctx_dim=1024, ctx_norm=256, w_kv_all=256, width=4096,
                operand_dtype=1, eps=1e-6, scratch=256, kv_all=256, ld_kv_all=4096, gemm_ws=None, gemm_ws_bytes=0,
                stream=None)
    call = lambda **kw: int(lib.rf_scene_kv(*{**good, **kw}.values()))  # noqa: E731
    for bad, msg in ((dict(ctx=None), b"ctx"), (dict(ctx_norm=None), b"ctx_norm"), (dict(w_kv_all=None), b"w_kv_all"),
                     (dict(scratch=None), b"scratch"), (dict(kv_all=None), b"kv_all"),
                     (dict(ctx_dim=1000, ld_ctx=1000), b"ctx_dim"), (dict(width=4000), b"multiple of 128"),
                     (dict(ld_kv_all=4095), b"ld_kv_all"), (dict(operand_dtype=7), b"operand_dtype"),
                     (dict(scratch=384), b"scratch")):
        assert call(**bad) == 1, bad
        assert msg in lib.rf_last_error(), (bad, lib.rf_last_error())
    assert b"null pointer" in (call(kv_all=None), lib.rf_last_error())[1]
    assert b"256-B aligned" in (call(scratch=384), lib.rf_last_error())[1]
    assert call(ctx_rows=0) == 0  # an empty context: nothing to launch


def test_decoder_accepts_given_kv_all():
    """With kv_all set the decoder needs neither ctx_norm nor w_kv_all and allows k_batch: validation gets as far
    as the out-of-order taps; ld_kv_all below n_layers * 2 * dim is refused by name."""
    _l, lib = _lib()
    good, layers, taps = _decoder_good()
    fwd = lambda d: int(lib.rf_decoder_forward(1, 1024, ctypes.addressof(d), None))  # noqa: E731
    given = {**good, "kv_all": 256, "ld_kv_all": 4096, "w_kv_all": 0, "ctx_norm": 0, "k_batch": 1,
             "taps": ctypes.addressof(taps), "n_taps": 2}
    assert fwd(_l.DecoderDesc(**given)) == 1
    assert b"tap 1" in lib.rf_last_error(), lib.rf_last_error()
    assert fwd(_l.DecoderDesc(**{**given, "ld_kv_all": 1024})) == 1
    assert b"ld_kv_all" in lib.rf_last_error(), lib.rf_last_error()
    # without kv_all the same descriptor fails as it always did
    assert fwd(_l.DecoderDesc(**{**given, "kv_all": 0})) == 1
    assert b"k_batch" in lib.rf_last_error(), lib.rf_last_error()


def test_decoder_workspace_leaves_out_context_and_kv():
    """rf_decoder_workspace_bytes with kv_all set holds no normed context and no K/V region."""
    _l, lib = _lib()
    good, layers, taps = _decoder_good()
    d = _l.DecoderDesc(**good)
    full = int(lib.rf_decoder_workspace_bytes(ctypes.addressof(d)))
    g = _l.DecoderDesc(**{**good, "kv_all": 256, "ld_kv_all": 4096, "w_kv_all": 0, "ctx_norm": 0})
    given = int(lib.rf_decoder_workspace_bytes(ctypes.addressof(g)))
    assert 0 < given <= full - 2 * 5649 * (1024 + 2 * 2 * 1024), (full, given)
    # the rotated keys of every layer are still there (k_batch)
    assert given >= 2 * (4096 * (3 * 1024 + 4096) + 5649 * 2 * 1024)
