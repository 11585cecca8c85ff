"""Encode a scene once, render any number of cameras from the handle (pipe.encode / pipe.render_encoded).

An encoded frame launches exactly what a full render launches after its K/V GEMM, on the same data, so frames are
compared with torch.equal wherever the launch sequence is the same; the parity bar (1e-3 relative L2 against the
reference's CPU fp32 frame) is the project's."""
import functools
import threading

import pytest
import torch

from golden_util import load_case, rel_l2
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


def _scene(d, tex=None):
    return d["triangles"], d["texture"].clone() if tex is None else tex, d["mask"], d["vn"]


def _overflow_sd(sd, scale=2000.0):
    """Stage-1 layer 0's SwiGLU w1 / w3 scaled so their fp16 product overflows (test_parity_gpu's recipe)."""
    sd = dict(sd)
    for k in ("transformer.layers.0.ffn.w1.weight", "transformer.layers.0.ffn.w3.weight"):
        sd[k] = sd[k] * scale
    return sd


def _decoder_overflow_sd(sd, scale=2000.0):
    """The same recipe on the decoder's layer 0 (w1 / w3 x scale: the fp16 SwiGLU output overflows in stage 2 while
    stage 1 stays inside fp16's range), with that layer's w2 / scale^2.  Without the w2 factor the layer's output
    enters the residual stream scale^2 times larger, and the DPT taps of that stream leave the range of the fp16 DPT
    planes even with bf16 projections: a DPT-plane overflow (range code 8), which is not the one under test here."""
    sd = dict(sd)
    p = "view_transformer.transformer.layers.0.ffn."
    for k in (p + "w1.weight", p + "w3.weight"):
        sd[k] = sd[k] * scale
    sd[p + "w2.weight"] = sd[p + "w2.weight"] / (scale * scale)
    return sd


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """The oracle's CPU fp32 frame of tiny_swin with the overflowing weights (computed once per module)."""
    cfg, sd, inp, res, z = _case("tiny_swin")
    big = {"stage1": _overflow_sd, "decoder": _decoder_overflow_sd}[kind](sd)
    return big, rf_ref.render(big, cfg, inp["triangles"], inp["texture"].clone(), inp["mask"], inp["vn"], inp["c2w"],
                              inp["fov"], resolution=res)


def _count(tag, fn):
    """Launches tagged `tag` that `fn` issues (the kernel timer, as test_native_stacks_bit_identical arms it)."""
    from renderformer_amd import ops
    timer = ops.KernelTimer(tag)
    ops.TIMER = timer
    try:
        out = fn()
    finally:
        ops.TIMER = None
    ms = timer.durations_ms()
    assert all(m > 0 for m in ms), (tag, ms)
    return len(ms), out


@pytest.mark.parametrize("name,env", [("tiny_swin", {}), ("tiny_full", {}), ("tiny_swin", {"RF_KV_BATCH": "0"}),
                                      ("tiny_swin_r128", {})])
def test_encoded_frame_equals_full_render(name, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, sd, inp, res, z = _case(name)
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    full = pipe(*_scene(d), d["c2w"], d["fov"], resolution=res, torch_dtype=torch.bfloat16)
    tex = d["texture"].clone()
    after = torch.from_numpy(z["texture_after_ch10"])
    scene = pipe.encode(*_scene(d, tex))
    assert (scene.kv_all is None) == bool(env)
    assert scene.nbytes == sum(t.numel() * t.element_size() for t in (scene.x1, scene.kv_all) if t is not None)
    assert torch.allclose(tex[:, :, 10, 0, 0].cpu(), after, rtol=1e-6, atol=1e-6)
    out = pipe.render_encoded(scene, d["c2w"], d["fov"], res, torch_dtype=torch.bfloat16)
    again = pipe.render_encoded(scene, d["c2w"], d["fov"], res)
    assert tuple(out.shape) == z["hdr"].shape and out.dtype == torch.float32
    assert torch.equal(out, full) and torch.equal(again, full)
    err = rel_l2(out.cpu(), z["hdr"])
    print(f"{name} {env}: encoded frame rel L2 {err:.3e} vs the reference")
    assert err < HDR_TOL
    assert torch.allclose(tex[:, :, 10, 0, 0].cpu(), after, rtol=1e-6, atol=1e-6)  # log-encoded exactly once
    assert pipe.last_precision["computed"].startswith("fp16 projection operands")


def test_views_over_time_match_the_batched_render():
    cfg, sd, inp, res, z = _case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    full = pipe(*_scene(d), d["c2w"], d["fov"], resolution=res).cpu()
    scene = pipe.encode(*_scene(d))
    V = d["c2w"].shape[1]
    assert V == 2
    for v in reversed(range(V)):
        one = pipe.render_encoded(scene, d["c2w"][:, v:v + 1], d["fov"][:, v:v + 1], res).cpu()
        err = rel_l2(one[:, 0], full[:, v])
        print(f"view {v} alone from the handle vs in the batch: rel L2 {err:.3e}")
        assert err < 1e-6
    pipe.model.view_chunk = 1
    chunked = pipe.render_encoded(scene, d["c2w"], d["fov"], res).cpu()
    for v in range(V):
        assert rel_l2(chunked[:, v], full[:, v]) < 1e-6


def test_one_handle_several_resolutions():
    cfg, sd, inp, res, z = _case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    full128 = pipe(*_scene(d), d["c2w"], d["fov"], resolution=128)
    scene = pipe.encode(*_scene(d))
    a = pipe.render_encoded(scene, d["c2w"], d["fov"], 64)
    b = pipe.render_encoded(scene, d["c2w"], d["fov"], 128)
    c = pipe.render_encoded(scene, d["c2w"], d["fov"], 64)
    assert torch.equal(a, c)
    assert b.shape[2:4] == (128, 128) and torch.equal(b, full128)


def test_nothing_camera_independent_runs_per_frame():
    cfg, sd, inp, res, z = _case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    n, scene = _count("attn_stage1", lambda: pipe.encode(*_scene(d)))
    assert n == cfg.num_layers
    n, _ = _count("attn_stage1", lambda: pipe.render_encoded(scene, d["c2w"], d["fov"], res))
    assert n == 0
    n, _ = _count("attn_cross", lambda: pipe.render_encoded(scene, d["c2w"], d["fov"], res))
    assert n == cfg.view_transformer_n_layers


def test_native_and_per_op_paths_bit_identical_on_one_handle():
    cfg, sd, inp, res, z = _case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    scene = pipe.encode(*_scene(d))
    outs = []
    for native in (False, True, False, True):
        pipe.model.native_stages = native
        outs.append(pipe.render_encoded(scene, d["c2w"], d["fov"], res))
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    assert rel_l2(outs[1].cpu(), z["hdr"]) < HDR_TOL


def test_scene_kv_then_decoder_forward_writes_the_same_taps():
    """C level: rf_scene_kv + rf_decoder_forward(kv_all) against rf_decoder_forward(w_kv_all) on the tiny_full
    model's device weights."""
    from renderformer_amd import ops
    from renderformer_amd.model import EPS
    cfg, sd, inp, res, z = _case("tiny_full")
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    m = pipe.model
    scene = pipe.encode(*_scene(d))
    W, dev = m._w, m.device
    B, V = d["c2w"].shape[:2]
    P = B * V
    plan = m._plan_host(scene.mask_host, V, res)
    D, H, F = cfg.view_transformer_latent_dim, cfg.view_transformer_n_heads, cfg.view_transformer_ffn_hidden_dim
    c2w_v = d["c2w"].reshape(P, 4, 4).float().contiguous()
    eye = torch.eye(4, dtype=torch.float32).expand(P, 4, 4).contiguous().to(dev)
    rays_c2w, pos_c2w = (eye, c2w_v) if cfg.turn_to_cam_coord else (c2w_v, eye)
    ray_in = torch.empty(P * plan.R, 3 * cfg.patch_size ** 2, dtype=W.half, device=dev)
    ray_pos = torch.empty(P, 9, dtype=torch.float32, device=dev)
    ops.ray_tokens(rays_c2w, d["fov"].reshape(P).float().contiguous(), res, cfg.patch_size, ray_in, ray_pos)
    x2 = m._ray_embed(plan, ray_in)
    pos2 = torch.empty(plan.T_kv, 9, dtype=torch.float32, device=dev)
    ops.scene_pos(scene.tris, plan.valid_flat, plan.scene_off, pos_c2w, B, V, cfg.num_register_tokens, pos2,
                  plan.kv_off, max(plan.counts))
    n_dec = len(W.dec)
    layers = ops.decoder_layers(W.dec, cfg.qk_norm)
    out_idx = sorted(i for i in set(cfg.out_layers) if 0 <= i < n_dec)
    kv_all = ops.scene_kv(scene.x1, W.ctx_unit, W.wkv_all, EPS)
    assert kv_all.shape == (plan.T1, n_dec * 2 * D) and torch.equal(kv_all, scene.kv_all)

    def run(**kv_form):
        x = x2.clone()
        planes = [W.dpt.empty_tap_planes(j, P, plan.hp, plan.wp, D, dev) for j in range(len(out_idx))]
        kv = dict(k_batch=True, k_norm_all=W.k_norm_all if cfg.qk_norm else None, kv_src_rows=plan.kv_src_rows,
                  kv_pos=pos2, freqs=W.dec_freqs, **kv_form)
        cross = dict(ray_pos=ray_pos, ray_pos_div=plan.R, problems=plan.prob2, schedule=plan.sched2,
                     qk_fused=W.qk_fused)
        sa = dict(swin=False, problems=plan.prob_self)
        ops.decoder_forward(x, layers, n_dec, H, F, W.half, EPS, scene.x1, kv, cross, sa,
                            [(i, pl.hi, pl.lo, pl.hi.shape[-1]) for i, pl in zip(out_idx, planes)])
        return x, planes

    xa, pa = run(ctx_norm=W.ctx_unit, w_kv_all=W.wkv_all)
    xb, pb = run(kv_all=kv_all, w_kv_all=None, ctx_norm=None)
    torch.cuda.synchronize()
    assert len(pa) > 0 and torch.equal(xa, xb)
    for a, b in zip(pa, pb):
        assert torch.equal(a.hi, b.hi) and (a.lo is None or torch.equal(a.lo, b.lo))
    with pytest.raises(ValueError, match="kv_all"):
        run(kv_all=kv_all[:, :D], w_kv_all=None, ctx_norm=None)


def test_overflow_during_encode_falls_back_and_encodes_again():
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = _case("tiny_swin")
    big, ref = _oracle("stage1")
    d = _dev(inp)
    pipe = _pipeline(cfg, big)
    tex = d["texture"].clone()
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        scene = pipe.encode(*_scene(d, tex))
    assert pipe.model.range_fallbacks == 1 and pipe.model.operands == "bf16"
    assert scene.precision[0] == "bf16" and scene.weights is pipe.model._w
    out = pipe.render_encoded(scene, d["c2w"], d["fov"], res)
    assert pipe.model.range_fallbacks == 1
    assert pipe.last_precision["computed"].startswith("bf16 projection")
    assert torch.isfinite(out).all()
    err = rel_l2(out.cpu(), ref)
    print(f"overflow during encode -> bf16 handle: rel L2 {err:.3e} vs the oracle")
    assert err < HDR_TOL
    assert torch.allclose(tex[:, :, 10, 0, 0].cpu(), torch.from_numpy(z["texture_after_ch10"]), rtol=1e-6, atol=1e-6)


def test_overflow_during_encode_deferred_raises():
    from renderformer_amd._lib import DeviceError
    cfg, sd, inp, res, z = _case("tiny_swin")
    big, _ = _oracle("stage1")
    pipe = _pipeline(cfg, big, range_check="deferred")
    with pytest.raises(DeviceError, match="operands='bf16'"):
        pipe.encode(*_scene(_dev(inp)))


def test_overflow_during_render_encoded_reencodes_the_handle():
    """A decoder-side overflow: encode is clean, render_encoded falls back, the handle is encoded again with bf16
    (once), and a handle made before the fallback (stale) is refreshed at its next use."""
    from renderformer_amd import ops
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = _case("tiny_swin")
    big, ref = _oracle("decoder")
    d = _dev(inp)
    # the premise: with the check off, stage 1 alone raises nothing and the decoder does
    raw = _pipeline(cfg, big, range_check="off")
    torch.cuda.synchronize()
    ops.clear_f16_range_flag()
    s0 = raw.encode(*_scene(d))
    torch.cuda.synchronize()
    assert ops.f16_range_flag() == 0
    raw.render_encoded(s0, d["c2w"], d["fov"], res)
    torch.cuda.synchronize()
    assert ops.f16_range_flag() != 0
    ops.clear_f16_range_flag()

    pipe = _pipeline(cfg, big)
    stale = pipe.encode(*_scene(d))   # scene A, encoded before the fallback and not rendered until after it
    scene = pipe.encode(*_scene(d))   # scene B
    assert pipe.model.range_fallbacks == 0 and scene.precision[0] == "f16"
    w16 = pipe.model._w
    with pytest.warns(PrecisionWarning, match="fp16 operand overflow"):
        out = pipe.render_encoded(scene, d["c2w"], d["fov"], res)
    assert pipe.model.range_fallbacks == 1 and pipe.model.operands == "bf16"
    assert scene.precision[0] == "bf16" and scene.weights is pipe.model._w and scene.weights is not w16
    assert torch.isfinite(out).all()
    err = rel_l2(out.cpu(), ref)
    print(f"overflow during render_encoded -> bf16 re-encode + re-render: rel L2 {err:.3e} vs the oracle")
    assert err < HDR_TOL
    n, again = _count("attn_stage1", lambda: pipe.render_encoded(scene, d["c2w"], d["fov"], res))
    assert n == 0 and pipe.model.range_fallbacks == 1  # no second re-encode
    assert torch.equal(again, out)
    # the stale handle: encoded again with the model's present operands, then rendered
    assert stale.weights is w16 and stale.precision[0] == "f16"
    n, late = _count("attn_stage1", lambda: pipe.render_encoded(stale, d["c2w"], d["fov"], res))
    assert n == cfg.num_layers and stale.precision[0] == "bf16" and stale.weights is pipe.model._w
    assert pipe.model.range_fallbacks == 1
    err = rel_l2(late.cpu(), ref)
    print(f"stale handle after the fallback: rel L2 {err:.3e} vs the oracle")
    assert torch.isfinite(late).all() and err < HDR_TOL


def test_stale_handle_with_edited_inputs_is_refused():
    from renderformer_amd._lib import DeviceError
    from renderformer_amd.model import PrecisionWarning
    cfg, sd, inp, res, z = _case("tiny_swin")
    big, _ = _oracle("decoder")
    d = _dev(inp)
    pipe = _pipeline(cfg, big)
    vn = d["vn"].clone()
    stale = pipe.encode(d["triangles"], d["texture"].clone(), d["mask"], vn)
    scene = pipe.encode(*_scene(d))
    with pytest.warns(PrecisionWarning):
        pipe.render_encoded(scene, d["c2w"], d["fov"], res)
    vn.mul_(1.0)  # an in-place edit of a retained input: the re-encode can no longer be trusted
    with pytest.raises(DeviceError, match="modified in place"):
        pipe.render_encoded(stale, d["c2w"], d["fov"], res)


def test_handle_misuse_raises():
    cfg, sd, inp, res, z = _case("tiny_swin")
    pipe, other = _pipeline(cfg, sd), _pipeline(cfg, sd)
    d = _dev(inp)
    scene = pipe.encode(*_scene(d))
    with pytest.raises(ValueError, match="another RenderFormer"):
        other.render_encoded(scene, d["c2w"], d["fov"], res)
    with pytest.raises(ValueError, match="EncodedScene"):
        pipe.render_encoded(scene.x1, d["c2w"], d["fov"], res)
    with pytest.raises(ValueError, match="batch size"):
        pipe.render_encoded(scene, d["c2w"][:1], d["fov"][:1], res)
    pipe.render_encoded(scene, d["c2w"], d["fov"], res)  # still good
    pipe.model.load_state_dict(sd)
    with pytest.raises(ValueError, match="load_state_dict"):
        pipe.render_encoded(scene, d["c2w"], d["fov"], res)


def test_two_threads_render_different_cameras_from_one_handle():
    cfg, sd, inp, res, z = _case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = _dev(inp)
    scene = pipe.encode(*_scene(d))
    cams = [(d["c2w"][:, v:v + 1].contiguous(), d["fov"][:, v:v + 1].contiguous()) for v in range(2)]
    serial = [pipe.render_encoded(scene, c, f, res).cpu() for c, f in cams]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    main = torch.cuda.current_stream()
    outs, errors = [None, None], []

    def work(i):
        try:
            streams[i].wait_stream(main)
            with torch.cuda.stream(streams[i]):
                outs[i] = pipe.render_encoded(scene, cams[i][0], cams[i][1], res)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for o, r in zip(outs, serial):
        assert torch.equal(o.cpu(), r)
