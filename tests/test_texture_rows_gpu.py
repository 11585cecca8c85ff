"""Material rows: a texture given as [B, N, C], one constant per triangle and channel (rf_texture_rows).

The compact form carries exactly the 13 numbers per triangle that the scan of an expanded to_h5-format texture
extracts, and both feed the same C-wide product (rf_texture_linear), so frames are compared with torch.equal; the
parity bar against the reference's CPU fp32 frame is the project's 1e-3 relative L2."""
import functools

import pytest
import torch

from golden_util import load_case, rel_l2
from kernel_checks import Guarded
from oracle import rf_ref

pytestmark = pytest.mark.gpu
HDR_TOL = 1e-3


@functools.lru_cache(maxsize=None)
def _case(name):
    return load_case(name)


def _pipeline(cfg, sd, **kw):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    return RenderFormerRenderingPipeline(RenderFormer(cfg, sd, **kw)).to("cuda")


def _dev(inp):
    return {k: v.cuda() for k, v in inp.items()}


def _rows(d):
    return d["texture"][:, :, :, 0, 0].contiguous()


def _render(pipe, d, tex, res):
    return pipe(d["triangles"], tex, d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)


def _overflow_sd(sd, scale=2000.0):
    """Stage-1 layer 0's SwiGLU w1 / w3 scaled so their fp16 product overflows (test_encoded_scene_gpu's recipe)."""
    sd = dict(sd)
    for k in ("transformer.layers.0.ffn.w1.weight", "transformer.layers.0.ffn.w3.weight"):
        sd[k] = sd[k] * scale
    return sd


@pytest.mark.parametrize("n_rows,log_ch,scatter", [(1, 3, False), (67, 3, True), (300, 0, True)])
def test_texture_rows_kernel(n_rows, log_ch, scatter):
    """rf_texture_rows alone: the in-place encode of every row (padded ones too) is bit for bit
    texture_scan's on the expanded form of the same constants, valid rows land in their coef row, and nothing
    outside the texture and the written coef rows is touched."""
    from renderformer_amd import ops
    from renderformer_amd.scenes import expand_texture
    C = 13
    g = torch.Generator().manual_seed(n_rows)
    ch = torch.rand(n_rows, C, generator=g)
    ch[:, 10:] *= 3000.0
    ch = ch.half().float()  # (expand_texture keeps fp16-representable values as they are)
    dst = torch.arange(n_rows, dtype=torch.int32)
    if scatter:
        dst[::3] = -1
        valid = dst >= 0
        dst[valid] = torch.randperm(int(valid.sum()), generator=g).int()
    T = int((dst >= 0).sum())
    tex = Guarded(n_rows, C, torch.float32, "cuda", ld=C).fill(ch)
    coef = Guarded(T, C, torch.float32, "cuda", ld=16)
    ops.texture_rows(tex.view, log_ch, dst.cuda(), coef.view)
    # the expanded route on the same constants
    big = torch.from_numpy(expand_texture(ch.numpy()[None])).cuda()
    coef2 = torch.zeros(T, 16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.texture_scan(big, log_ch, dst.cuda(), coef2, flag)
    torch.cuda.synchronize()
    assert int(flag) == 0
    assert torch.equal(tex.view, big[0, :, :, 0, 0])
    assert torch.equal(coef.view, coef2[:, :C])
    tex.assert_untouched(what="texture_rows texture")
    coef.assert_untouched(what="texture_rows coef")
    assert torch.equal(tex.view[:, :C - log_ch].cpu(), ch[:, :C - log_ch])  # the other channels are as they were


@pytest.mark.parametrize("name", ["tiny_swin", "tiny_full"])
def test_compact_equals_expanded(name):
    cfg, sd, inp, res, z = _case(name)
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    rows = _rows(d)
    assert tuple(rows.shape) == tuple(d["texture"].shape[:3])
    full = _render(pipe, d, d["texture"].clone(), res)
    assert int(pipe.model._w.tex_flag.item()) == 0  # the expanded call took the scan's fast path
    out = _render(pipe, d, rows, res)
    assert torch.equal(out, full)
    err = rel_l2(out.cpu(), z["hdr"])
    print(f"{name}: compact-texture frame rel L2 {err:.3e} vs the reference")
    assert err < HDR_TOL
    # log-encoded in place, exactly once
    assert torch.allclose(rows[:, :, 10].cpu(), torch.from_numpy(z["texture_after_ch10"]), rtol=1e-6, atol=1e-6)
    assert torch.equal(rows[:, :, :10], d["texture"][:, :, :10, 0, 0])


def test_compact_and_expanded_interleave_on_one_model():
    """expanded, compact, an expanded texture with one non-constant patch (general path, flag raised), compact,
    expanded: each frame equals that input's own frame from a fresh model, so the compact path neither reads nor
    disturbs the frame-parity flags of the expanded one."""
    cfg, sd, inp, res, z = _case("tiny_swin")
    d = _dev(inp)
    bad = d["texture"].clone()
    bad[0, 3, 2, 5, 7] += 0.25
    inputs = {"expanded": lambda: d["texture"].clone(), "compact": lambda: _rows(d), "bad": lambda: bad.clone()}
    own = {k: _render(_pipeline(cfg, sd), d, make(), res) for k, make in inputs.items()}
    assert not torch.equal(own["bad"], own["expanded"]) and torch.equal(own["compact"], own["expanded"])
    pipe = _pipeline(cfg, sd)
    for i, kind in enumerate(["expanded", "compact", "bad", "compact", "expanded"]):
        out = _render(pipe, d, inputs[kind](), res)
        assert torch.equal(out, own[kind]), (i, kind)
        if kind != "compact":
            assert int(pipe.model._w.tex_flag.item()) == (kind == "bad"), (i, kind)
        assert int(pipe.model._w.tex_rows_flag.item()) == 0


@pytest.mark.parametrize("name", ["tiny_swin", "tiny_full"])
def test_encoded_scene_from_compact_texture(name):
    cfg, sd, inp, res, z = _case(name)
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    full = _render(pipe, d, d["texture"].clone(), res)
    rows = _rows(d)
    scene = pipe.encode(d["triangles"], rows, d["mask"], d["vn"])
    assert scene.inputs[1] is rows  # the handle retains the compact tensor, nothing expanded
    out = pipe.render_encoded(scene, d["c2w"], d["fov"], res)
    assert torch.equal(out, full)
    assert torch.allclose(rows[:, :, 10].cpu(), torch.from_numpy(z["texture_after_ch10"]), rtol=1e-6, atol=1e-6)
    want = pipe.gbuffer(d["triangles"], d["texture"], d["mask"], d["vn"], d["c2w"], d["fov"], res)
    got = pipe.gbuffer_encoded(scene, d["c2w"], d["fov"], res)
    direct = pipe.gbuffer(d["triangles"], rows, d["mask"], d["vn"], d["c2w"], d["fov"], res)
    for f in want._fields:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
        assert torch.equal(getattr(direct, f), getattr(want, f)), f
    assert bool((want.albedo != 0).any())


def test_fp16_fallback_reencodes_from_the_compact_tensor():
    """The overflow recipe of test_encoded_scene_gpu: encode falls back to bf16 operands and encodes again from the
    retained [B, N, C] tensor, which is log-encoded once (the replay passes log_encode=False); so does render."""
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = _case("tiny_swin")
    big = _overflow_sd(sd)
    ref = rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                        inp["fov"], resolution=res)
    after = torch.from_numpy(z["texture_after_ch10"])
    d = _dev(inp)
    pipe = _pipeline(cfg, big)
    rows = _rows(d)
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        scene = pipe.encode(d["triangles"], rows, d["mask"], d["vn"])
    assert pipe.model.range_fallbacks == 1 and scene.precision[0] == "bf16"
    out = pipe.render_encoded(scene, d["c2w"], d["fov"], res)
    err = rel_l2(out.cpu(), ref)
    print(f"overflow during encode of a compact texture -> bf16 handle: rel L2 {err:.3e} vs the oracle")
    assert torch.isfinite(out).all() and err < HDR_TOL
    assert torch.allclose(rows[:, :, 10].cpu(), after, rtol=1e-6, atol=1e-6)
    # the same through render (RangeGuard.run's replay)
    pipe2 = _pipeline(cfg, big)
    rows2 = _rows(d)
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        out2 = _render(pipe2, d, rows2, res)
    err2 = rel_l2(out2.cpu(), ref)
    print(f"overflow during render of a compact texture: rel L2 {err2:.3e} vs the oracle")
    assert err2 < HDR_TOL and torch.allclose(rows2[:, :, 10].cpu(), after, rtol=1e-6, atol=1e-6)


def test_compact_texture_errors():
    cfg, sd, inp, res, z = _case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    with pytest.raises(ValueError, match="texture_channels"):
        _render(pipe, d, _rows(d)[:, :, :12].contiguous(), res)
    with pytest.raises(ValueError, match="float32"):
        _render(pipe, d, _rows(d).half(), res)
    with pytest.raises(ValueError, match="contiguous"):
        _render(pipe, d, d["texture"][:, :, :, 0, 0], res)


def test_patch_size_1_models_keep_their_own_path(monkeypatch):
    """For texture_encode_patch_size == 1 a [B, N, C] texture already is the native texture: it still goes to
    ops.texture_pack with patch_elems = 1, never to ops.texture_rows.  (That path's own outcome is not this file's
    subject: rf_texture_pack refuses patch_elems = 1 -- it needs a multiple of 4 -- before and after material rows.)"""
    import dataclasses
    from renderformer_amd import ops
    from renderformer_amd.weights import synthetic_state_dict
    cfg, _, inp, res, z = _case("tiny_swin")
    cfg1 = dataclasses.replace(cfg, texture_encode_patch_size=1)
    pipe = _pipeline(cfg1, synthetic_state_dict(cfg1, seed=1))
    d = _dev(inp)
    seen = []

    class _Stop(Exception):
        pass

    def pack(texture, log_channels, dst_row, out):
        seen.append((tuple(texture.shape), log_channels, tuple(out.shape)))
        raise _Stop

    def rows(*a, **k):
        raise AssertionError("a patch-size-1 model must not take the material-row path")

    monkeypatch.setattr(ops, "texture_pack", pack)
    monkeypatch.setattr(ops, "texture_rows", rows)
    for tex in (_rows(d), d["texture"].clone()):  # [B, N, C], and the 5-D form the pipeline slices to it
        with pytest.raises(_Stop):
            _render(pipe, d, tex, res)
    B, N = inp["mask"].shape
    assert seen == [((B, N, 13), 3, (int(inp["mask"].sum()), 13))] * 2
