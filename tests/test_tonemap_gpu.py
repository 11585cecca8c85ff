"""rf_tonemap_ldr8 on the device: the 8-bit display frame of an HDR frame (ops.tonemap_ldr8, pipeline.to_ldr, CLIs).

Shapes are chosen for the kernel's paths, not for the workload: a lane handles four pixels (three 16-byte loads, 12
packed bytes out) and the last n_pix % 4 pixels go through a scalar tail, so the pixel counts are 1, 3 (tail only),
4 (one group, no tail), 5, 255, 257, 45 * 99 (an overscan window of the camera tests: odd, no multiple of 4, several
blocks) and 2 * 64 * 64 (32 blocks, no tail).

The bound of the float output (E_FLOAT = 1e-5 absolute on v, test_tonemap.py) is derived, not measured: ahead of the
encode the operator is at most about ten fp32 roundings of values <= 1 (each <= 2^-24, 6e-8: 6e-7 in all), the
encode's slope is at most 12.92 (7.8e-6), and its power adds a few ulp of a value <= 1 (< 1e-6).  The bytes follow
from it by the banded rule of test_tonemap.py.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from golden_util import load_case  # noqa: E402
from kernel_checks import Guarded, assert_elementwise  # noqa: E402
from test_tonemap import E_FLOAT, assert_banded, display64, hdr_case, linear_case  # noqa: E402

pytestmark = pytest.mark.gpu

N_PIX = [1, 3, 4, 5, 255, 257, 45 * 99, 2 * 64 * 64]


def _ops():
    from renderformer_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ 1. none is exact
@pytest.mark.parametrize("n_pix", N_PIX)
def test_none_reproduces_hdr_to_ldr_bytes(n_pix):
    from renderformer_amd.images import hdr_to_ldr
    x = linear_case(n_pix, seed=n_pix)
    d = torch.from_numpy(x).cuda()
    got = _ops().tonemap_ldr8(d)
    assert got.dtype == torch.uint8 and got.shape == d.shape and got.device == d.device
    np.testing.assert_array_equal(got.cpu().numpy(), hdr_to_ldr(x))
    np.testing.assert_array_equal(_ops().tonemap_ldr8(d, "none", 1.0).cpu().numpy(), hdr_to_ldr(2 * x))
    assert torch.equal(d.cpu(), torch.from_numpy(x))  # the frame is only read


# ------------------------------------------------------------------------------------------------ 2. extreme values
@pytest.mark.parametrize("mapper", ["none", "pbr_neutral"])
def test_non_finite_and_extreme_values(mapper):
    """NaN -> 0, -inf -> 0, +inf -> 255 in that channel (pbr_neutral: an infinite channel makes the pixel white), 1e30
    -> 255, pbr_neutral at peak 1e3 -> 254 or 255, and every other pixel of the frame is what it is without them."""
    ops = _ops()
    base = linear_case(257, seed=9).clip(0.0, None)
    plain = ops.tonemap_ldr8(torch.from_numpy(base).cuda(), mapper).cpu().numpy()
    x = base.copy()
    spots = {0: [np.nan, 0.25, 0.5], 5: [0.25, -np.inf, 0.5], 6: [0.25, 0.5, np.inf], 130: [1e30, 0.25, 0.5],
             131: [1000.04, 1000.04, 1000.04], 255: [np.inf, np.inf, np.inf], 256: [np.nan, np.nan, np.nan]}
    for p, v in spots.items():  # (group lanes and the tail pixel 256)
        x[p] = v
    got = ops.tonemap_ldr8(torch.from_numpy(x).cuda(), mapper).cpu().numpy()
    others = np.setdiff1d(np.arange(257), list(spots))
    np.testing.assert_array_equal(got[others], plain[others])
    assert got[0, 0] == 0 and got[5, 1] == 0 and (got[256] == 0).all()
    assert got[6, 2] == 255 and got[130, 0] == 255 and (got[255] == 255).all()
    if mapper == "pbr_neutral":
        assert (got[6] == 255).all()
        assert set(got[131].tolist()) <= {254, 255} and len(set(got[131].tolist())) == 1
        # the finite channels beside a NaN / -inf are those of the same frame with a 0 there
        zeroed = np.where(np.isnan(x) | np.isneginf(x), np.float32(0), x)
        np.testing.assert_array_equal(got, ops.tonemap_ldr8(torch.from_numpy(zeroed).cuda(), mapper).cpu().numpy())
    else:
        assert got[131].tolist() == [255, 255, 255]
        assert got[0].tolist() == [0, 63, 127] and got[5].tolist() == [63, 0, 127] and got[6].tolist() == [63, 127, 255]


# ------------------------------------------------------------------------------------------------ 3. float output
def _float_inputs():
    """the byte test's decades, the linear range with an exposure whose gain is not a power of two, and a grid around
    the toe's end (min = 0.08), the knee (peak = 0.76 after the offset) and the encode's linear segment"""
    yield "decades", hdr_case(0), 0.0
    yield "linear", linear_case(45 * 99, seed=4), 0.5
    g = np.concatenate([np.linspace(0.0, 0.01, 301), np.linspace(0.079, 0.081, 301), np.linspace(0.79, 0.81, 301),
                        np.linspace(0.0, 12.0, 301)]).astype(np.float32)
    rng = np.random.default_rng(8)
    yield "edges", np.stack([g, rng.permutation(g), rng.permutation(g)], axis=-1), 0.0


@pytest.mark.parametrize("n_pix", N_PIX)
def test_pbr_neutral_float_output_sizes(n_pix):
    x = hdr_case(n_pix, shape=(n_pix, 3))
    q, v = _ops().tonemap_ldr8(torch.from_numpy(x).cuda(), "pbr_neutral", mapped=True)
    v64 = display64(x, "pbr_neutral")
    assert_elementwise(v, torch.from_numpy(v64), E_FLOAT, f"pbr_neutral v, {n_pix} pixels")
    assert_banded(q.cpu().numpy(), v64, what=f"pbr_neutral bytes, {n_pix} pixels")
    # the byte is the truncation of the kernel's own float, exactly
    assert torch.equal(q, (v * 255.0).to(torch.uint8))


def test_pbr_neutral_float_output_within_bound():
    worst = {}
    for name, x, exposure in _float_inputs():
        q, v = _ops().tonemap_ldr8(torch.from_numpy(x).cuda(), "pbr_neutral", exposure, mapped=True)
        assert v.dtype == torch.float32 and v.shape == x.shape
        v64 = display64(x, "pbr_neutral", exposure)
        worst[name] = assert_elementwise(v, torch.from_numpy(v64), E_FLOAT, f"pbr_neutral v ({name})") * E_FLOAT
        assert float(v.min()) >= 0.0 and float(v.max()) <= 1.0
    print("worst |v - v64|:", {k: f"{e:.3g}" for k, e in worst.items()}, f"(bound {E_FLOAT:g})")
    x = linear_case(257, seed=2)
    _, v = _ops().tonemap_ldr8(torch.from_numpy(x).cuda(), "none", mapped=True)
    assert torch.equal(v.cpu(), torch.from_numpy(np.clip(x, 0, 1)))  # none: v is the clipped frame, exactly


# ------------------------------------------------------------------------------------------------ 4. bytes, banded
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pbr_neutral_bytes_banded(seed):
    x = hdr_case(seed)
    v64 = display64(x, "pbr_neutral")
    q = _ops().tonemap_ldr8(torch.from_numpy(x).cuda(), "pbr_neutral").cpu().numpy()
    share = assert_banded(q, v64, cap=0.01, what=f"pbr_neutral bytes, seed {seed}")
    present = np.unique(q)
    print(f"seed {seed}: the band excludes {share:.4%}; {present.size} byte values present")
    assert set(range(255)) <= set(present.tolist())


# ------------------------------------------------------------------------------------------------ 5. nothing else
@pytest.mark.parametrize("n_pix", [1, 5, 257])
@pytest.mark.parametrize("mapper", ["none", "pbr_neutral"])
def test_writes_its_outputs_and_nothing_else(n_pix, mapper):
    """ldr and mapped inside sentinel margins (4 guard rows of n_pix * 3 elements before and after: the byte buffer
    starts 4-byte aligned and, at these sizes, not 16-byte aligned), pre-filled with the sentinel: every element of a
    given output is overwritten, the margins and a buffer that was not given keep the sentinel."""
    from renderformer_amd import _lib
    ops = _ops()
    x = torch.from_numpy(hdr_case(n_pix, shape=(n_pix, 3))).cuda()
    n = n_pix * 3
    ldr = Guarded(1, n, torch.uint8, "cuda", g=4, ld=n)
    mapped = Guarded(1, n, torch.float32, "cuda", g=4, ld=n)
    assert ldr.view.data_ptr() % 4 == 0 and ldr.view.data_ptr() % 16 != 0 and mapped.view.data_ptr() % 16 == 0
    want_q, want_v = ops.tonemap_ldr8(x, mapper, mapped=True)
    # a valid float is never the sentinel NaN; the byte sentinel 0xA5 = 165 may be a value: check against the result

    def launch(q, v):
        _lib.call("rf_tonemap_ldr8", _lib.ptr(x), _lib.ptr(q), _lib.ptr(v), n_pix, ops.TONEMAP[mapper], 1.0,
                  _lib.stream())
        torch.cuda.synchronize()

    launch(ldr.view, mapped.view)
    for g_ in (ldr, mapped):
        g_.assert_untouched(what=f"both outputs, {n_pix} pixels")
    assert torch.equal(ldr.view.reshape(n_pix, 3), want_q) and torch.equal(mapped.view.reshape(n_pix, 3), want_v)
    assert not torch.isnan(mapped.view).any()  # every float was overwritten

    ldr.reset(), mapped.reset()
    launch(ldr.view, None)  # ldr only
    ldr.assert_untouched(what="ldr only")
    assert torch.equal(ldr.view.reshape(n_pix, 3), want_q)
    assert bool((mapped.ibuf == mapped.sentinel).all())

    ldr.reset(), mapped.reset()
    launch(None, mapped.view)  # mapped only
    mapped.assert_untouched(what="mapped only")
    assert torch.equal(mapped.view.reshape(n_pix, 3), want_v)
    assert bool((ldr.ibuf == ldr.sentinel).all())

    # the byte sentinel could hide an unwritten byte that happens to equal its value: a second fill value settles it
    ldr.ibuf.fill_(0x5A)
    launch(ldr.view, None)
    assert torch.equal(ldr.view.reshape(n_pix, 3), want_q)
    assert bool((ldr.ibuf[ldr.outside()] == 0x5A).all())


def test_out_and_argument_checks():
    ops = _ops()
    x = torch.from_numpy(hdr_case(3, shape=(2, 7, 5, 3))).cuda()
    out = torch.full(x.shape, 0xA5, dtype=torch.uint8, device="cuda")
    got = ops.tonemap_ldr8(x, "pbr_neutral", out=out)
    assert got is out and torch.equal(out, ops.tonemap_ldr8(x, "pbr_neutral"))
    for bad, kw in ((x.double(), {}), (x[..., :2], {}), (x.transpose(1, 2), {}), (x.cpu(), {}),
                    (x, dict(out=out.float())), (x, dict(out=out[:1])), (x, dict(out=out.cpu())),
                    (x, dict(mapper="agx")), (x, dict(exposure=float("nan"))), (x, dict(exposure=200.0))):
        with pytest.raises(ValueError):
            ops.tonemap_ldr8(bad, **kw)
    empty = ops.tonemap_ldr8(x[:0])
    assert empty.shape == (0, 7, 5, 3) and empty.dtype == torch.uint8


# ------------------------------------------------------------------------------------------------ 6. it can fail
def _emulation(x: np.ndarray, drop_toe=False, gamma22=False, round_nearest=False):
    """The pbr_neutral kernel in fp32 torch on the CPU (exposure 0) -> (bytes, v), with one planted defect: the toe
    offset dropped, a 2.2 power law in place of the sRGB curve, round-to-nearest in place of truncation."""
    c = torch.from_numpy(x).float()
    c = torch.where(c > 0, c, torch.zeros_like(c))
    mn = c.min(dim=-1, keepdim=True).values
    offset = torch.where(mn < 0.08, mn - 6.25 * mn * mn, torch.full_like(mn, 0.04))
    if not drop_toe:
        c = c - offset
    peak = c.max(dim=-1, keepdim=True).values
    new_peak = 1.0 - 0.24 * 0.24 / (peak + 0.24 - 0.76)
    k = 1.0 - 1.0 / (0.15 * (peak - new_peak) + 1.0)
    m = c * (new_peak / peak) * (1.0 - k) + new_peak * k
    m = torch.where(peak < 0.76, c, m).clamp(0.0, 1.0)
    if gamma22:
        v = m.pow(1.0 / 2.2)
    else:
        v = torch.where(m <= 0.0031308, 12.92 * m, 1.055 * m.pow(1.0 / 2.4) - 0.055)
        v = torch.where(m >= 1.0, torch.ones_like(v), v)
    t = v * 255.0
    q = (t + 0.5 if round_nearest else t).to(torch.uint8)
    return q.numpy(), v


def _checks_3_and_4(q, v, v64):
    assert_elementwise(v, torch.from_numpy(v64), E_FLOAT, "emulation v")
    assert_banded(q, v64, cap=0.01, what="emulation bytes")


def test_the_checks_reject_planted_defects():
    x = hdr_case(0)
    v64 = display64(x, "pbr_neutral")
    _checks_3_and_4(*_emulation(x), v64)  # the faithful emulation passes
    for defect in ("drop_toe", "gamma22", "round_nearest"):
        with pytest.raises(AssertionError):
            _checks_3_and_4(*_emulation(x, **{defect: True}), v64)


# ------------------------------------------------------------------------------------------------ 7. end to end
def _pipeline(cfg, sd, **kw):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    return RenderFormerRenderingPipeline(RenderFormer(cfg, sd, **kw)).to("cuda")


def test_to_ldr_of_a_rendered_frame():
    ops = _ops()
    cfg, sd, inp, res, z = load_case("tiny_swin")
    pipe = _pipeline(cfg, sd)
    d = {k: v.cuda() for k, v in inp.items()}
    scene = pipe.encode(d["triangles"], d["texture"].clone(), d["mask"], d["vn"])
    hdr = pipe.render_encoded(scene, d["c2w"], d["fov"], 64)
    before = hdr.clone()
    ldr = pipe.to_ldr(hdr, "pbr_neutral")
    assert ldr.dtype == torch.uint8 and ldr.shape == hdr.shape and ldr.device == hdr.device
    assert torch.equal(hdr, before)  # bit-identical: the HDR frame is the product's contract
    assert torch.equal(ldr, ops.tonemap_ldr8(hdr, "pbr_neutral"))
    assert_banded(ldr.cpu().numpy(), display64(hdr.cpu().numpy(), "pbr_neutral"), what="rendered frame")
    from renderformer_amd.images import hdr_to_ldr
    np.testing.assert_array_equal(pipe.to_ldr(hdr).cpu().numpy(), hdr_to_ldr(hdr.cpu().numpy()))
    out = torch.empty_like(ldr)
    assert pipe.to_ldr(hdr, "pbr_neutral", 1.0, out=out) is out
    assert_banded(out.cpu().numpy(), display64(hdr.cpu().numpy(), "pbr_neutral", 1.0), what="rendered frame, +1 stop")
    with pytest.raises(ValueError, match="simple_ocio"):
        pipe.to_ldr(hdr, "filmic")
    # lazy range check: resolve first, then the display frame
    lazy = _pipeline(cfg, sd, range_check="lazy")
    frame = lazy.render(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=64)
    lazy.resolve(frame)
    assert torch.equal(lazy.to_ldr(frame, "pbr_neutral"), ops.tonemap_ldr8(frame, "pbr_neutral"))


def _snapshot_and_scene(tmp_path):
    from safetensors.torch import save_file

    from renderformer_amd import h5io
    cfg, sd, inp, res, z = load_case("tiny_swin")
    snap = tmp_path / "snap"
    snap.mkdir()
    (snap / "config.json").write_text(json.dumps(cfg.to_dict()))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(snap / "model.safetensors"))
    m = inp["mask"][0].numpy().astype(bool)
    h5 = tmp_path / "scenes" / "tiny.h5"
    h5.parent.mkdir()
    h5io.write_scene(str(h5), inp["triangles"][0].numpy()[m], inp["vn"][0].numpy()[m],
                     inp["texture"][0].numpy()[m].astype(np.float16), inp["c2w"][0].numpy(),
                     inp["fov"][0].numpy().reshape(-1), texture_dtype=np.float16)
    return snap, h5, res, z["hdr"].shape[1]


def _check_written(out, name, nv, mapper, exposure):
    from renderformer_amd.images import hdr_to_ldr, read_exr, read_png
    for i in range(nv):
        hdr = read_exr(str(out / f"{name}_view_{i}.exr"))
        png = read_png(str(out / f"{name}_view_{i}.png"))
        if mapper == "none" and exposure == 0.0:
            np.testing.assert_array_equal(png, hdr_to_ldr(hdr))  # what the parent commit writes
            continue
        # the EXR is the float32 frame, lossless: the PNG is the kernel's bytes of exactly these pixels
        dev = _ops().tonemap_ldr8(torch.from_numpy(np.ascontiguousarray(hdr)).cuda(), mapper, exposure)
        np.testing.assert_array_equal(png, dev.cpu().numpy())
        assert_banded(png, display64(hdr, mapper, exposure), what=f"{name} view {i}")


def test_infer_cli_writes_tone_mapped_pngs(tmp_path):
    import infer
    snap, h5, res, nv = _snapshot_and_scene(tmp_path)
    base = ["--h5_file", str(h5), "--model_id", str(snap), "--resolution", str(res)]
    for k, (mapper, exposure) in enumerate((("pbr_neutral", 0.0), ("none", 0.0), ("pbr_neutral", 1.5))):
        out = tmp_path / f"out{k}"
        flags = ["--tone_mapper", mapper] + (["--exposure", str(exposure)] if exposure else [])
        assert infer.main(base + ["--output_dir", str(out)] + flags) == 0
        _check_written(out, "tiny", nv, mapper, exposure)


@pytest.mark.parametrize("inline", ["0", "1"])
def test_batch_infer_cli_writes_tone_mapped_pngs(tmp_path, monkeypatch, inline):
    import batch_infer
    snap, h5, res, nv = _snapshot_and_scene(tmp_path)
    for i in (2, 3):
        os.link(h5, h5.parent / f"tiny{i}.h5")
    monkeypatch.setenv("RF_BATCH_INLINE", inline)
    out = tmp_path / "out"
    assert batch_infer.main(["--h5_folder", str(h5.parent), "--model_id", str(snap), "--resolution", str(res),
                             "--output_dir", str(out), "--batch_size", "1", "--tone_mapper", "pbr_neutral",
                             "--exposure", "-0.5"]) == 0
    for name in ("tiny", "tiny2", "tiny3"):
        _check_written(out, name, nv, "pbr_neutral", -0.5)
