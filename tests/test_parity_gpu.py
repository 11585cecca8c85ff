"""End-to-end parity of the HIP path with the reference, through the drop-in API.

Golden fixtures (tests/golden/*.npz) were produced by the reference itself on
CPU fp32; the oracle restatement is bit-identical to them (test_oracle_golden).
Bar (BASELINE.json north_star): <= 1e-3 relative L2 on the HDR pixels.
"""
import time

import numpy as np
import pytest
import torch

from golden_util import (BIG_CASES, CASES, PROD_TAP_CASES, REAL_CASES, hdr_shape, load_case, reference_hdr, rel_l2,
                         rel_l2_ac)
from oracle import rf_ref

pytestmark = pytest.mark.gpu
HDR_TOL = 1e-3
# deviation-from-the-mean bound at production size: the fp16-operand path measures 1-2e-4 (tools/
# precision_budget.py predicts 1.2e-4); bf16 operands would be 6-8e-4
AC_TOL = 4e-4


def _pipeline(cfg, sd, dpt_precision=None):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    return RenderFormerRenderingPipeline(RenderFormer(cfg, sd, dpt_precision=dpt_precision)).to("cuda")


@pytest.mark.parametrize("name,dpt", [(c, "f16") for c in CASES] + [("tiny_large", "bf16x3"), ("cbox_base", "bf16x3")])
def test_pipeline_matches_reference(name, dpt):
    cfg, sd, inp, res, z = load_case(name)
    pipe = _pipeline(cfg, sd, dpt)
    d = {k: v.cuda() for k, v in inp.items()}
    tex = d["texture"]
    out = pipe(d["triangles"], tex, d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
               torch_dtype=torch.bfloat16)
    assert tuple(out.shape) == z["hdr"].shape and out.dtype == torch.float32
    err = rel_l2(out.cpu(), z["hdr"])
    print(f"{name} (DPT {dpt}): rel L2 {err:.3e}")
    assert err < HDR_TOL
    assert int(pipe.model._w.tex_flag.item()) == 0  # to_h5-format textures: the texture fast path ran
    # in-place log encoding side effect (rendering_pipeline.py:67-68)
    assert torch.allclose(tex[:, :, 10, 0, 0].cpu(), torch.from_numpy(z["texture_after_ch10"]), rtol=1e-6, atol=1e-6)


def test_padding_invariance_and_view_independence():
    """Padded triangles must not change the image; a view rendered alone == inside a batch."""
    from renderformer_amd.scenes import batch_scenes, synthetic_scene
    cfg, sd, _, _, _ = load_case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    sc = synthetic_scene(50, 2, seed=21)

    def run(pad, views):
        s = synthetic_scene(50, 2, seed=21)
        s.c2w, s.fov = sc.c2w[views], sc.fov[views]
        b = batch_scenes([s], padding_length=pad)
        b = {k: v.cuda() for k, v in b.items()}
        return pipe(b["triangles"], b["texture"], b["mask"], b["vn"], b["c2w"], b["fov"], resolution=64).cpu()

    a = run(None, [0, 1])
    b = run(96, [0, 1])
    c = run(None, [1])
    assert rel_l2(b, a) < 1e-6
    assert rel_l2(c[0, 0], a[0, 1]) < 1e-6


def test_concurrent_renders_on_two_streams():
    """Two pipelines enqueued on two streams at once (stream-K GEMM/attention workspaces are per stream)
    give bit-identical images to the same renders run one after the other."""
    from renderformer_amd.scenes import batch_scenes, synthetic_scene
    cfg, sd, _, _, _ = load_case("tiny_swin")
    pipes = [_pipeline(cfg, sd), _pipeline(cfg, sd)]
    batches = []
    for seed, n in ((31, 70), (32, 45)):
        b = batch_scenes([synthetic_scene(n, 2, seed=seed)])
        batches.append({k: v.cuda() for k, v in b.items()})

    def render(p, b):
        return p(b["triangles"], b["texture"].clone(), b["mask"], b["vn"], b["c2w"], b["fov"], resolution=64)

    serial = [render(p, b).cpu() for p, b in zip(pipes, batches)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    main = torch.cuda.current_stream()
    outs = []
    for s, p, b in zip(streams, pipes, batches):
        s.wait_stream(main)
        with torch.cuda.stream(s):
            outs.append(render(p, b))
    torch.cuda.synchronize()
    for o, r in zip(outs, serial):
        assert torch.equal(o.cpu(), r)


def test_concurrent_bench_frames_on_two_streams():
    """Two full bench-shape frames (large-proxy, 14+10 layers, 512^2: cbox N=5,633 and cbox-bunny N=6,209) enqueued
    on two streams at once.  Here every stream-K launch cuts units (stage 1: 184 units of 89 tiles on 256
    workgroups), and two concurrent kernels can hold every CU between them: the owners' waits only go to
    earlier-dispatched blocks (common.h SkLayout), so both frames drain, raise no device error, and equal the
    same frames rendered one after the other bit for bit."""
    from renderformer_amd import _lib
    cases = [load_case("large_cbox_r512"), load_case("large_bunny_r512")]
    cfg, sd = cases[0][0], cases[0][1]
    pipes = [_pipeline(cfg, sd), _pipeline(cfg, sd)]
    batches = [{k: v.cuda() for k, v in c[2].items()} for c in cases]

    def render(p, b):
        return p(b["triangles"], b["texture"].clone(), b["mask"], b["vn"], b["c2w"], b["fov"], resolution=512)

    serial = [render(p, b).cpu() for p, b in zip(pipes, batches)]
    for p, b, c in zip(pipes, batches, cases):  # warm plans on both pipelines before the concurrent pass
        render(p, b)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    main = torch.cuda.current_stream()
    for _ in range(2):
        outs = []
        for s, p, b in zip(streams, pipes, batches):
            s.wait_stream(main)
            with torch.cuda.stream(s):
                outs.append(render(p, b))
        torch.cuda.synchronize()
        assert _lib.load().rf_device_error() == 0
        for o, r in zip(outs, serial):
            assert torch.equal(o.cpu(), r)
    for o, c in zip(serial, cases):
        ref, st = reference_hdr(c[4])
        assert rel_l2(o[:, :, ::st, ::st], ref) < HDR_TOL
    del pipes, batches
    torch.cuda.empty_cache()


def test_model_forward_reference_signature():
    """RenderFormer.forward with the reference's tensors (renderformer.py:171) vs the oracle's model_forward."""
    from renderformer_amd import RenderFormer
    cfg, sd, inp, res, z = load_case("tiny_swin")
    tex = inp["texture"].clone()
    tex[:, :, -3:] = torch.log10(tex[:, :, -3:] + 1)
    bs, nv = inp["c2w"].shape[:2]
    tris_v = rf_ref.cam_transform(inp["c2w"].reshape(-1, 4, 4), torch.repeat_interleave(inp["triangles"], nv, 0))
    c2w_v = torch.eye(4).repeat(bs * nv, 1, 1).reshape(bs, nv, 4, 4)
    ro, rd = rf_ref.ray_gen(c2w_v, inp["fov"] / 180.0 * torch.pi, res)
    args = (inp["triangles"].reshape(bs, -1, 9), tex, inp["mask"], inp["vn"].reshape(bs, -1, 9), ro, rd,
            tris_v.reshape(bs, nv, -1, 9))
    ref = rf_ref.model_forward(sd, cfg, *args)
    m = RenderFormer(cfg, sd).to("cuda")
    got = m(*[a.cuda() for a in args], tf32_view_tf=False)
    assert got.shape == ref.shape
    assert rel_l2(got.cpu(), ref) < 1e-3


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    import renderformer_amd._lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(L.HipLibraryError):
        L.load()


@pytest.mark.parametrize("mode", ["general", "perturbed"])
def test_texture_paths_match_reference(mode, monkeypatch):
    """The texture encoder's to_h5 fast path is proven per call on the device: forcing the general pack+GEMM
    path (RF_TEX_FAST=0), or feeding a texture that is NOT of the to_h5 form (one texel moved, which must
    raise the scan's flag and route through the gated general path), still matches the oracle."""
    cfg, sd, inp, res, z = load_case("tiny_swin")
    tex = inp["texture"].clone()
    if mode == "general":
        monkeypatch.setenv("RF_TEX_FAST", "0")
    else:
        tex[0, 3, 2, 5, 7] += 0.25  # diffuse channel 2 of triangle 3: no longer constant x mask
    ref = rf_ref.render(sd, cfg, inp["triangles"], tex.clone(), inp["mask"], inp["vn"], inp["c2w"], inp["fov"],
                        resolution=res)
    pipe = _pipeline(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    out = pipe(d["triangles"], tex.cuda(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
               torch_dtype=torch.bfloat16)
    err = rel_l2(out.cpu(), ref)
    print(f"texture {mode}: rel L2 {err:.3e}")
    assert err < HDR_TOL
    if mode == "perturbed":
        assert int(pipe.model._w.tex_flag.item()) == 1  # the scan rejected the fast path


def test_texture_flag_parity_across_frames():
    """The fast-path flag alternates between two device scalars by frame parity (rf_texture_scan2: each frame's
    scan clears the flag the next frame raises into, no reset launch): good / perturbed / good / perturbed /
    good textures in a row must each take the right path and match the oracle."""
    cfg, sd, inp, res, z = load_case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    bad = inp["texture"].clone()
    bad[0, 3, 2, 5, 7] += 0.25
    refs = {}
    for i, kind in enumerate(["good", "bad", "good", "bad", "good"]):
        tex = inp["texture"] if kind == "good" else bad
        if kind not in refs:
            refs[kind] = rf_ref.render(sd, cfg, inp["triangles"], tex.clone(), inp["mask"], inp["vn"], inp["c2w"],
                                       inp["fov"], resolution=res)
        out = pipe(d["triangles"], tex.clone().cuda(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
                   torch_dtype=torch.bfloat16)
        assert int(pipe.model._w.tex_flag.item()) == (kind == "bad"), (i, kind)
        assert rel_l2(out.cpu(), refs[kind]) < HDR_TOL, (i, kind)


def test_plan_cache_follows_in_place_mask_edits():
    """The per-call plan is reused only for the same, unmodified mask tensor: an in-place edit of the mask
    must produce the same image as a fresh tensor with the edited content."""
    from renderformer_amd.scenes import batch_scenes, synthetic_scene
    cfg, sd, _, _, _ = load_case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    b = {k: v.cuda() for k, v in batch_scenes([synthetic_scene(60, 1, seed=5)], padding_length=64).items()
         if k != "tex_channels"}

    def run(mask):
        return pipe(b["triangles"], b["texture"].clone(), mask, b["vn"], b["c2w"], b["fov"], resolution=64).cpu()

    mask = b["mask"].clone()
    run(mask)
    mask[0, 40:] = False  # in place: same object, new version
    got = run(mask)
    ref = run(mask.clone())
    assert rel_l2(got, ref) < 1e-6


@pytest.mark.parametrize("name", BIG_CASES)
def test_baseline_configs_match_reference(name):
    """Every BASELINE.json configuration at its own size and full depth vs the reference's own CPU fp32 output
    (tests/golden/make_golden.py): large-proxy 14+10 layers cbox N=5,633 at 512^2 (config 2, the bench
    workload), cbox-bunny N=6,209 at 512^2 (config 3), v1-base 12+6 layers at 256^2 (config 1's shape) and
    4 views of one scene at 1024^2 (config 5's shape; every 4th pixel row/column of the fixture)."""
    cfg, sd, inp, res, z = load_case(name)
    pipe = _pipeline(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    out = pipe(d["triangles"], d["texture"], d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
               torch_dtype=torch.bfloat16)
    assert tuple(out.shape) == hdr_shape(z)
    ref, st = reference_hdr(z)
    got = out[:, :, ::st, ::st].cpu()
    err, ac = rel_l2(got, ref), rel_l2_ac(got, ref)
    print(f"{name}: rel L2 {err:.3e} (deviation from the mean: {ac:.3e})")
    assert err < HDR_TOL
    assert ac < AC_TOL
    # discrimination guard: the error must be far below the distance between two DIFFERENT frames
    # of the fixtures, so a path that rendered the wrong view or scene cannot pass
    if "view01_rel_l2_ac" in z.files:  # two camera views of the same scene
        for v in range(1, got.shape[1]):
            assert rel_l2_ac(got[:, v], ref[:, v]) <= 0.25 * float(z["view01_rel_l2_ac"]), v
        assert rel_l2_ac(got[:, 1], ref[:, 0]) > 2.0 * rel_l2_ac(got[:, 0], ref[:, 0])  # view 1 is not view 0
    if name in ("large_cbox_r512", "large_bunny_r512"):  # cbox (N=5,633) vs cbox-bunny (N=6,209)
        other = load_case("large_bunny_r512" if name == "large_cbox_r512" else "large_cbox_r512")[4]["hdr"]
        dist = rel_l2_ac(other, ref)
        assert ac <= 0.25 * dist, (ac, dist)
        assert rel_l2_ac(got, other) > 0.75 * dist  # the other scene's reference is far from this frame
    if "hdr_sum" in z.files:  # the whole image, not only the sampled pixels
        o64 = out.double()
        assert abs(float(o64.sum()) - float(z["hdr_sum"])) / abs(float(z["hdr_sum"])) < 1e-3
        assert abs(float((o64 ** 2).sum()) - float(z["hdr_sumsq"])) / float(z["hdr_sumsq"]) < 2e-3
    del pipe, out, d
    torch.cuda.empty_cache()


TAP_TOL = 1e-3  # per-tap relative L2 bar at production size


@pytest.mark.parametrize("name", PROD_TAP_CASES)
def test_production_taps_match_reference(name):
    """The HIP path's intermediates at production size vs the reference's own (make_golden.PROD_TAPS): a fixed
    sample of stage-1 output rows (the 16 register tokens + seeded triangle rows) and every stage-1 row's norm,
    every decoder layer's output on seeded ray-token rows of the first views, and the DPT logits (the
    reference's pre-ELU out_dpt output through the ELU, vs log10(HDR + 1) of the GPU frame) every few pixels.
    A wrong view, scene, layer or token order is far outside these bars (the sampled rows are different
    triangles / rays: swapping them costs O(1) relative error)."""
    cfg, sd, inp, res, z = load_case(name)
    pipe = _pipeline(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    cap = pipe.model.capture_taps(enc_rows=z["enc_row_idx"], dec_rows=z["dec_row_idx"],
                                  dec_views=[int(v) for v in z["dec_views"]])
    out = pipe(d["triangles"], d["texture"], d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
               torch_dtype=torch.bfloat16)
    errs = {"enc_rows": rel_l2(cap["enc_rows"].cpu(), z["tap_enc_rows"])}
    if "enc_rownorm" in z.files:
        errs["enc_rownorm"] = rel_l2(cap["enc_rownorm"].cpu(), z["enc_rownorm"][0])
    dec = cap["dec_rows"].cpu()
    assert tuple(dec.shape) == z["tap_dec_rows"].shape
    for i in range(dec.shape[0]):
        errs[f"dec{i}"] = rel_l2(dec[i], z["tap_dec_rows"][i])
    st = int(z["dpt_sub_stride"])
    logits = torch.from_numpy(z["tap_dpt_sub"]).double()  # [B*V, 3, H/st, W/st], pre-ELU
    ref_log = torch.where(logits > 0, logits, 1e-3 * torch.expm1(logits))  # ELU(alpha=1e-3), view_transformer.py:86
    # [B, V, res, res, 3] -> [B*V, 3, res/st, res/st]
    got_log = torch.log10(out.double().cpu()[:, :, ::st, ::st, :3].flatten(0, 1).permute(0, 3, 1, 2) + 1.0)
    errs["dpt_logits"] = rel_l2(got_log, ref_log)
    # discrimination: the same sample against shuffled reference rows (a token-order / view mix-up)
    shuffled = rel_l2(cap["enc_rows"].cpu(), np.roll(z["tap_enc_rows"], 1, axis=0))
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"; rows shifted by one: {shuffled:.2e}")
    for k, v in errs.items():
        assert v < TAP_TOL, (k, v)
    assert shuffled > 100 * errs["enc_rows"]
    del pipe, out, d
    torch.cuda.empty_cache()


def test_reference_import_surface_readme_example(monkeypatch):
    """README.md:155-187 verbatim through `from renderformer import RenderFormerRenderingPipeline`: the hub id
    resolves offline (RF_SYNTHETIC_SEED: random-init weights of the named architecture), random inputs,
    output [2, 4, 512, 512, 3] float32."""
    monkeypatch.setenv("RF_SYNTHETIC_SEED", "0")
    from renderformer import RenderFormerRenderingPipeline
    pipeline = RenderFormerRenderingPipeline.from_pretrained("microsoft/renderformer-v1.1-swin-large")
    device = torch.device('cuda')
    pipeline.to(device)
    B, N, P, V = 2, 1024, 32, 4
    triangles = torch.randn((B, N, 3, 3), device=device)
    texture = torch.randn((B, N, 13, P, P), device=device)
    mask = torch.ones((B, N), dtype=torch.bool, device=device)
    vn = torch.randn((B, N, 3, 3), device=device)
    c2w = torch.randn((B, V, 4, 4), device=device)
    fov = torch.randn((B, V, 1), device=device)
    imgs = pipeline(triangles=triangles, texture=texture, mask=mask, vn=vn, c2w=c2w, fov=fov, resolution=512,
                    torch_dtype=torch.float16)
    assert tuple(imgs.shape) == (2, 4, 512, 512, 3) and imgs.dtype == torch.float32
    with pytest.warns(UserWarning, match="float32"):
        pipeline(triangles=triangles, texture=texture.clone(), mask=mask, vn=vn, c2w=c2w, fov=fov, resolution=64,
                 torch_dtype=torch.float32)
    assert pipeline.last_precision["computed"] == pipeline.model.precision


def test_model_on_non_current_device():
    """A model placed on cuda:1 while cuda:0 is current launches on cuda:1's stream (the reference's infer.py
    uses cuda:1): same image as on cuda:0.  Needs two devices; on a one-GPU box the placement must fail
    cleanly instead of launching on the wrong device."""
    cfg, sd, inp, res, z = load_case("tiny_swin")
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    if torch.cuda.device_count() < 2:
        with pytest.raises(Exception):
            RenderFormerRenderingPipeline(RenderFormer(cfg, sd)).to("cuda:1")
        return
    torch.cuda.set_device(0)
    outs = []
    for dev in ("cuda:0", "cuda:1"):
        pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd)).to(dev)
        d = {k: v.to(dev) for k, v in inp.items()}
        outs.append(pipe(d["triangles"], d["texture"], d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res).cpu())
    assert torch.cuda.current_device() == 0
    assert rel_l2(outs[1], outs[0]) < 1e-6 and rel_l2(outs[1], z["hdr"]) < HDR_TOL


@pytest.mark.parametrize("name", ["large_cbox_r512", "large_cbox_r1024_v4"])
def test_fp8_stage2_parity(name):
    """The opt-in fp8 mode (its default subset: the stage-2 cross-attention Q and the FFN W2 as MX fp8 GEMMs)
    against the same reference fixtures, at the north-star bar.  The other projections in fp8 miss it
    (per-projection errors: tools/fp8_study.py), so the mode does not take them by default."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    cfg, sd, inp, res, z = load_case(name)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd, fp8=True)).to("cuda")
    d = {k: v.cuda() for k, v in inp.items()}
    out = pipe(d["triangles"], d["texture"], d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    ref, st = reference_hdr(z)
    got = out[:, :, ::st, ::st].cpu()
    err, ac = rel_l2(got, ref), rel_l2_ac(got, ref)
    print(f"fp8 stage 2, {name}: rel L2 {err:.3e} (deviation from the mean: {ac:.3e}); bar 1e-3")
    assert err < 1e-3
    del pipe, out, d
    torch.cuda.empty_cache()


def _overflow_sd(sd, scale=2000.0):
    """The tiny_swin weights with stage-1 layer 0's SwiGLU w1 / w3 scaled so their fp16 product overflows
    (silu(w1 h) * (w3 h) ~ 1e5-1e6 > 65504): a stand-in for a checkpoint whose activations exceed fp16's range."""
    sd = dict(sd)
    for k in ("transformer.layers.0.ffn.w1.weight", "transformer.layers.0.ffn.w3.weight"):
        sd[k] = sd[k] * scale
    return sd


def test_f16_overflow_default_render_is_final_without_resolve():
    """the README-style call (default model, no resolve, no check_range) on a checkpoint whose
    activations exceed fp16 returns a finite frame within 1e-3 of the oracle: the default "sync" range check waits
    for the frame's own end event and re-renders it in bf16 before render returns."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    big = _overflow_sd(sd)
    ref = rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                        inp["fov"], resolution=res)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, big)).to("cuda")
    assert pipe.model.range_check == "sync"
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        out = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
                   torch_dtype=torch.float16)
    img = out.cpu()  # what the reference README does next
    assert torch.isfinite(img).all()
    err = rel_l2(img, ref)
    print(f"README-style call, overflowing checkpoint: rel L2 {err:.3e} vs the oracle")
    assert err < HDR_TOL
    assert pipe.model.range_fallbacks == 1 and pipe.last_precision["computed"].startswith("bf16 projection")


def test_f16_overflow_detected_and_rerendered_in_bf16():
    """ADVICE r3 / VERDICT r3 item 2, VERDICT r4 item 3: the fp16 writers raise the frame's own range word, the
    opt-in "lazy" range check reads it once the frame has completed — here in resolve(out) — renders the frame
    again IN PLACE with bf16 operands (which the model keeps), and the result is finite and matches the oracle's fp32
    render of the same weights; last_precision says which operands ran.  A normal frame never raises a word and
    reports fp16 operands."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline, ops
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    torch.cuda.synchronize()
    ops.clear_f16_range_flag()  # (earlier tests may have raised the process-wide word)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd, range_check="lazy")).to("cuda")
    out = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    assert pipe.resolve(out) is False and pipe.model.range_fallbacks == 0
    assert pipe.last_precision["computed"].startswith("fp16 projection operands")
    assert rel_l2(out.cpu(), z["hdr"]) < HDR_TOL

    big = _overflow_sd(sd)
    ref = rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                        inp["fov"], resolution=res)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, big, range_check="lazy")).to("cuda")
    tex = d["texture"].clone()
    out = pipe(d["triangles"], tex, d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        assert pipe.resolve(out) is True
    assert pipe.model.range_fallbacks == 1 and pipe.model.operands == "bf16"
    assert pipe.last_precision["computed"].startswith("bf16 projection operands")
    assert torch.isfinite(out).all()
    err = rel_l2(out.cpu(), ref)
    print(f"fp16 overflow -> bf16 re-render: rel L2 {err:.3e} vs the oracle")
    assert err < HDR_TOL
    # the texture was log-encoded once (in place, like the reference), not twice by the re-render
    assert torch.allclose(tex[:, :, 10, 0, 0].cpu(), torch.from_numpy(z["texture_after_ch10"]), rtol=1e-6, atol=1e-6)
    assert ops.f16_range_flag() == 0  # per-render words: the process-wide word is untouched
    # the same fp16 render with the check off really does overflow (the flag is what caught it)
    raw = RenderFormer(cfg, big, range_check="off").to("cuda")
    o2 = RenderFormerRenderingPipeline(raw)(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"],
                                            d["fov"], resolution=res)
    torch.cuda.synchronize()
    assert ops.f16_range_flag() != 0
    ops.clear_f16_range_flag()
    assert not torch.isfinite(o2).all() or rel_l2(o2.cpu(), ref) > HDR_TOL


def test_f16_overflow_sync_mode_rerenders_before_returning():
    """range_check="sync": the render waits for its own frame's end event and returns the re-rendered frame."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    big = _overflow_sd(sd)
    ref = rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                        inp["fov"], resolution=res)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, big, range_check="sync")).to("cuda")
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        out = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    assert pipe.model.range_fallbacks == 1 and pipe.last_precision["computed"].startswith("bf16 projection")
    assert rel_l2(out.cpu(), ref) < HDR_TOL


def _dpt_overflow_sd(sd, scale=1e5):
    """DPT tap projection 0 scaled by `scale` and the deconvolution that reads it by 1/scale: the same function in
    exact arithmetic (and in fp32), but the projection's fp16 planes overflow (a DPT-plane overflow,
    range code 8, not a transformer one)."""
    sd = dict(sd)
    pre = "view_transformer.out_dpt."
    sd[pre + "projects.0.weight"] = sd[pre + "projects.0.weight"] * scale
    sd[pre + "projects.0.bias"] = sd[pre + "projects.0.bias"] * scale
    sd[pre + "resize_layers.0.weight"] = sd[pre + "resize_layers.0.weight"] / scale
    return sd


def test_dpt_plane_overflow_falls_back_to_bf16x3():
    """a DPT-plane overflow (code 8) moves the DPT to bf16x3 planes (the projections keep
    fp16: no transformer writer overflowed), the re-render is checked again, and the frame matches the oracle.
    A model with bf16 projection operands still checks its fp16 DPT planes."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    big = _dpt_overflow_sd(sd)
    ref = rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                        inp["fov"], resolution=res)
    for operands in ("f16", "bf16"):
        pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, big, operands=operands, range_check="lazy")).to("cuda")
        out = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
        with pytest.warns(PrecisionWarning, match="DPT plane"):
            assert pipe.resolve(out) is True
        m = pipe.model
        assert m.dpt_precision == "bf16x3" and m.operands == operands and m.range_fallbacks == 1
        assert torch.isfinite(out).all()
        err = rel_l2(out.cpu(), ref)
        print(f"DPT plane overflow ({operands} projections) -> bf16x3 re-render: rel L2 {err:.3e} vs the oracle")
        assert err < HDR_TOL


def test_overflow_isolated_between_concurrent_renders():
    """an overflowing model and a normal one render concurrently on two streams; only the
    first falls back, and both frames match their oracle renders (each render raises a word of its own)."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    big = _overflow_sd(sd)
    ref_big = rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                            inp["fov"], resolution=res)
    bad = RenderFormerRenderingPipeline(RenderFormer(cfg, big, range_check="lazy")).to("cuda")
    good = RenderFormerRenderingPipeline(RenderFormer(cfg, sd, range_check="lazy")).to("cuda")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):  # twice: the second round renders with the words the first one released
        with torch.cuda.stream(sa):
            oa = bad(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
        with torch.cuda.stream(sb):
            ob = good(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
        assert good.resolve(ob) is False
        if bad.model.range_fallbacks == 0:
            with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
                assert bad.resolve(oa) is True
        else:
            assert bad.resolve(oa) is False  # bf16 from the first round on: nothing to check
        torch.cuda.synchronize()
        assert bad.model.range_fallbacks == 1 and good.model.range_fallbacks == 0
        assert good.model.operands == "f16" and bad.model.operands == "bf16"
        assert rel_l2(ob.cpu(), z["hdr"]) < HDR_TOL
        assert rel_l2(oa.cpu(), ref_big) < HDR_TOL


def test_render_returns_before_the_frame_completes():
    """with the opt-in "lazy" range check render() issues the frame and returns without a host
    wait (the reference's render has no sync inside, rendering_pipeline.py:105-125): with the stream held busy by a
    spin kernel queued in front, the frame is still pending when render returns; resolve() then waits for it."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd, range_check="lazy")).to("cuda")
    out = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    pipe.resolve(out)  # warm: plans, weights, workspaces
    tex = d["texture"].clone()
    torch.cuda.synchronize()
    torch.cuda._sleep(int(2e9))  # a ~1 s spin on the current stream ahead of the frame
    t0 = time.perf_counter()
    out = pipe(d["triangles"], tex, d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    t_ret = time.perf_counter() - t0
    pending = not torch.cuda.current_stream().query()
    assert pipe.resolve(out) is False
    t_done = time.perf_counter() - t0
    print(f"render returned after {t_ret * 1e3:.1f} ms, frame complete after {t_done * 1e3:.1f} ms")
    assert pending and t_ret < 0.5 * t_done
    assert rel_l2(out.cpu(), z["hdr"]) < HDR_TOL


def test_lazy_fallback_waits_for_frames_in_flight():
    """in lazy mode an overflow found by a LATER render's poll rebuilds the weights while other
    frames of the model may still run on non-default streams; the rebuild waits for them first (the old weight
    tensors go back to the caching allocator).  Frame a runs on stream s1 behind a short spin, frame b on s2 behind a
    long one; once a has completed, frame c's render polls and resolves a (overflow -> bf16 weights) while b still
    runs on the old weights.  The rebuild's wait lets b finish, so the same poll finds b's overflow too and renders
    it again on the new weights (no second rebuild): two frames re-rendered.
    Every frame ends finite and within 1e-3 of the oracle."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    big = _overflow_sd(sd)
    ref = rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                        inp["fov"], resolution=res)
    args = lambda: (d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"])  # noqa: E731
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, big, range_check="lazy")).to("cuda")
    import batch_infer
    s1 = torch.cuda.Stream()
    for _ in range(8):  # s2 on a hardware queue other than s1's (HIP maps streams onto 4 queues round robin)
        s2 = torch.cuda.Stream()
        if batch_infer._runs_beside(s2, s1):
            break
    # warm every per-model and per-stream cache (plan, camera constants, workspaces: some are built with a host
    # sync) with the check off, so nothing inside the timed renders below waits for the spins
    pipe.model.range_check = "off"
    for st in (s1, s2):
        with torch.cuda.stream(st):
            pipe(*args(), resolution=res)
    torch.cuda.synchronize()
    pipe.model.range_check = "lazy"
    with torch.cuda.stream(s1):
        ina = args()
        torch.cuda._sleep(int(1e9))  # a is still running when b's render polls
        a = pipe(*ina, resolution=res)
    with torch.cuda.stream(s2):
        inb = args()
        torch.cuda._sleep(int(6e9))  # b stays in flight while c's poll resolves a
        b = pipe(*inb, resolution=res)
    assert pipe.model.range_fallbacks == 0
    s1.synchronize()
    assert not s2.query()
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        with torch.cuda.stream(s1):
            c = pipe(*args(), resolution=res)
        w = pipe.model._w
        assert pipe.model.range_fallbacks == 2 and pipe.model.operands == "bf16"  # a and b, one rebuild
        pipe.model.check_range()  # nothing left pending
        assert pipe.model._w is w
    torch.cuda.synchronize()
    for name, o in (("a", a), ("b", b), ("c", c)):
        err = rel_l2(o.cpu(), ref)
        print(f"frame {name}: rel L2 {err:.3e}")
        assert torch.isfinite(o).all() and err < HDR_TOL
    pipe.model.close()
    assert not pipe.model._guard.free and not pipe.model._guard.pending


def test_f16_overflow_deferred_check_raises():
    """range_check="deferred" (bench.py's timed loop): no wait per frame; check_range() raises DeviceError naming
    the bf16 remedy, and the next frames render normally."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd._lib import DeviceError
    cfg, sd, inp, res, z = load_case("tiny_swin")
    d = {k: v.cuda() for k, v in inp.items()}
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, _overflow_sd(sd), range_check="deferred")).to("cuda")
    pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    with pytest.raises(DeviceError, match="operands='bf16'"):
        pipe.check_range()
    ok = RenderFormerRenderingPipeline(RenderFormer(cfg, sd, range_check="deferred")).to("cuda")
    ok(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res)
    ok.check_range()  # no overflow: no error


def test_plan_hint_matches_read_back():
    """plan_hint (the host copy of a device mask, batch_infer.py / bench.py): a new mask pattern's plan is built
    from the host copy without reading the mask back, and the frame equals the one planned from the read-back;
    a hint is ignored once the device mask is edited in place."""
    from renderformer_amd.scenes import batch_scenes, synthetic_scene
    cfg, sd, _, _, _ = load_case("tiny_swin")
    b = {k: v for k, v in batch_scenes([synthetic_scene(60, 2, seed=8), synthetic_scene(41, 2, seed=9)],
                                         padding_length=64).items() if k != "tex_channels"}
    d = {k: v.cuda() for k, v in b.items()}
    ref = _pipeline(cfg, sd)(d["triangles"], d["texture"].clone(), d["mask"].clone(), d["vn"], d["c2w"], d["fov"],
                             resolution=64).cpu()
    pipe = _pipeline(cfg, sd)
    pipe.model.plan_hint(d["mask"], b["mask"].numpy())
    got = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=64).cpu()
    assert torch.equal(got, ref)
    wrong = b["mask"].numpy().copy()
    wrong[0, :] = True  # a stale hint: must not be used after the in-place edit below
    pipe.model.plan_hint(d["mask"], wrong)
    d["mask"][1, 30:] = False
    edited = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=64).cpu()
    fresh = _pipeline(cfg, sd)(d["triangles"], d["texture"].clone(), d["mask"].clone(), d["vn"], d["c2w"], d["fov"],
                               resolution=64).cpu()
    assert torch.equal(edited, fresh)


@pytest.mark.parametrize("name,env", [("tiny_swin", {}), ("cbox_base", {}), ("tiny_full", {}),
                                      ("tiny_swin", {"RF_K_BATCH": "0"}), ("tiny_full", {"RF_KV_BATCH": "0"})])
def test_native_stacks_bit_identical(name, env, monkeypatch):
    """rf_encoder_forward / rf_decoder_forward (each stage as one library call) issue the same launches in the same
    order as the Python-issued per-op sequence, so the frames are bit-identical (Swin and full self-attention,
    batched and per-layer K/V and keys); the kernel timer still sees every stage-1 / cross-attention launch."""
    from renderformer_amd import ops
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, sd, inp, res, z = load_case(name)
    pipe = _pipeline(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    outs = []
    for native in (False, True, False, True):
        pipe.model.native_stages = native
        outs.append(pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"],
                         resolution=res, torch_dtype=torch.bfloat16))
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    assert rel_l2(outs[1].cpu(), z["hdr"]) < HDR_TOL
    for tag, n in (("attn_stage1", cfg.num_layers), ("attn_cross", cfg.view_transformer_n_layers)):
        timer = ops.KernelTimer(tag)
        ops.TIMER = timer
        try:
            pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
                 torch_dtype=torch.bfloat16)
        finally:
            ops.TIMER = None
        ms = timer.durations_ms()
        assert len(ms) == n and all(m > 0 for m in ms), (tag, ms)
