"""Display (LDR) frames without a device: images.hdr_to_ldr's numpy form of the tone-map arithmetic, the argument
checks of rf_tonemap_ldr8 (made before any launch) and the CLI flags.

The arithmetic under test is restated here in fp64, independently of renderformer_amd/images.py (display64 and the
functions above it); tests/test_tonemap_gpu.py imports the restatement and the banded byte rule from this module.

The banded byte rule.  With v64 the fp64 display value of an element, t = 255 v64 and q the byte under test, whose
own fp32 value v is within E = 1e-5 of v64 (the bound of the float output, derived in test_tonemap_gpu.py): 255 v is
within 255 E of t, so q = floor(255 v) is within 1 of floor(t) everywhere, and equals floor(t) wherever t is farther
than 255 E from an integer.
"""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

E_FLOAT = 1e-5  # element-wise bound of the fp32 display value against fp64


# ------------------------------------------------------------------------------------------------ fp64 restatement
def pbr_neutral64(c: np.ndarray) -> np.ndarray:
    """Khronos PBR Neutral of fp64 c [..., 3] >= 0, before the display encode."""
    c = np.asarray(c, dtype=np.float64)
    x = c.min(axis=-1, keepdims=True)
    offset = np.where(x < 0.08, x - 6.25 * x * x, 0.04)
    c = c - offset
    peak = c.max(axis=-1, keepdims=True)
    d = 0.24
    with np.errstate(all="ignore"):
        new_peak = 1.0 - d * d / (peak + d - 0.76)
        scaled = c * (new_peak / peak)
        g = 1.0 - 1.0 / (0.15 * (peak - new_peak) + 1.0)
        m = scaled * (1.0 - g) + new_peak * g
    m = np.where(np.isposinf(peak), 1.0, m)
    return np.where(peak < 0.76, c, m)


def srgb64(t: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.where(t <= 0.0031308, 12.92 * t, 1.055 * np.power(t, 1.0 / 2.4) - 0.055)


def display64(hdr, mapper: str = "none", exposure: float = 0.0) -> np.ndarray:
    """Steps 1-3 in fp64 on the fp32 inputs: the display value v of every element (the gain is the float32 the entry
    point is handed)."""
    gain = float(np.float32(2.0 ** exposure))
    c = np.asarray(hdr, dtype=np.float32).astype(np.float64) * gain
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0, c, 0.0)  # NaN -> 0
    if mapper == "none":
        return np.minimum(c, 1.0)
    assert mapper == "pbr_neutral"
    return srgb64(np.clip(pbr_neutral64(c), 0.0, 1.0))


def assert_banded(q, v64, cap=None, what: str = "") -> float:
    """The banded byte rule of the module docstring; cap: the largest share of elements the band may exclude.
    Returns that share."""
    q = np.asarray(q).astype(np.int64)
    t = 255.0 * np.asarray(v64, dtype=np.float64)
    assert q.shape == t.shape, (what, q.shape, t.shape)
    fl = np.floor(t).astype(np.int64)
    far = np.abs(q - fl) > 1
    assert not far.any(), f"{what}: {int(far.sum())} bytes more than 1 from floor(255 v64), first {np.argwhere(far)[0]}"
    strict = np.abs(t - np.round(t)) > 255.0 * E_FLOAT
    excluded = 1.0 - float(strict.mean())
    if cap is not None:
        assert excluded <= cap, f"{what}: the band excludes {excluded:.4%} of the elements (cap {cap:.2%})"
    bad = strict & (q != fl)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {int(strict.sum())} bytes differ from floor(255 v64) outside "
                           f"the band; first at {np.argwhere(bad)[0]}: {q[bad][0]} vs {fl[bad][0]} (t = {t[bad][0]!r})")
    return excluded


# ------------------------------------------------------------------------------------------------ inputs
def byte_edges() -> np.ndarray:
    """every k / 255 as float32 with its two float32 neighbours: where (x * 255) truncates differently"""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    return np.concatenate([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))]).astype(np.float32)


def linear_case(n_pix: int, seed: int = 0) -> np.ndarray:
    """[n_pix, 3] finite float32 in [-0.5, 2] that carries the byte edges (as many as fit)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 2.0, size=n_pix * 3).astype(np.float32)
    e = byte_edges()
    n = min(e.size, x.size)
    x[rng.permutation(x.size)[:n]] = rng.permutation(e)[:n]
    return x.reshape(n_pix, 3)


def hdr_case(seed: int, shape=(45, 99, 3)) -> np.ndarray:
    """10^U(-3, 1) per channel: four decades around the toe and the knee"""
    return (10.0 ** np.random.default_rng(seed).uniform(-3.0, 1.0, size=shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ images.hdr_to_ldr
def test_default_hdr_to_ldr_keeps_its_bytes():
    from renderformer_amd import images
    assert images.TONE_MAPPERS == ("none", "pbr_neutral")
    x = np.concatenate([linear_case(4000, 3).ravel(), byte_edges()]).astype(np.float32)
    x = x[: x.size // 3 * 3].reshape(-1, 3)
    assert (x < 0).any() and (x > 1).any()
    legacy = (np.clip(x, 0, 1) * 255).astype(np.uint8)
    np.testing.assert_array_equal(images.hdr_to_ldr(x), legacy)
    np.testing.assert_array_equal(images.hdr_to_ldr(x, "none", 0.0), legacy)
    # an exposure goes through the general float32 path: one stop is an exact doubling
    np.testing.assert_array_equal(images.hdr_to_ldr(x, "none", 1.0), (np.clip(2 * x, 0, 1) * 255).astype(np.uint8))
    np.testing.assert_array_equal(images.hdr_to_ldr(x, exposure=-1.0), (np.clip(x / 2, 0, 1) * 255).astype(np.uint8))
    # the general path defines what the reference's expression leaves to the platform
    odd = np.array([[np.nan, -np.inf, np.inf], [1e30, -1e30, 0.5]], dtype=np.float32)
    np.testing.assert_array_equal(images.hdr_to_ldr(odd, exposure=1.0), [[0, 0, 255], [255, 0, 255]])
    with pytest.raises(ValueError, match="simple_ocio"):
        images.hdr_to_ldr(x, "agx")
    with pytest.raises(ValueError, match="unknown tone mapper"):
        images.hdr_to_ldr(x, "reinhard")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_numpy_pbr_neutral_matches_fp64(seed):
    from renderformer_amd import images
    x = hdr_case(seed)
    v64 = display64(x, "pbr_neutral")
    q = images.hdr_to_ldr(x, "pbr_neutral")
    assert q.dtype == np.uint8 and q.shape == x.shape
    share = assert_banded(q, v64, cap=0.01, what=f"numpy pbr_neutral seed {seed}")
    print(f"seed {seed}: band excludes {share:.4%}; byte values present: {np.unique(q).size}")
    assert set(range(255)) <= set(np.floor(255 * v64).ravel().astype(int).tolist())  # the whole curve is exercised
    x2 = linear_case(3000, seed)
    assert_banded(images.hdr_to_ldr(x2, "pbr_neutral", 1.5), display64(x2, "pbr_neutral", 1.5), what="exposure 1.5")
    odd = np.array([[np.nan, -np.inf, 0.25], [np.inf, 0.1, 0.2], [np.inf] * 3, [1e30, 0.0, 0.0], [0.0] * 3],
                   dtype=np.float32)
    got = images.hdr_to_ldr(odd, "pbr_neutral")
    np.testing.assert_array_equal(got[[1, 2]], 255)
    assert got[3, 0] == 255 and (got[4] == 0).all() and (got[0, :2] == 0).all()


def test_operator_pins():
    """Hand-computed values of the operator (fp64, 1e-12), and the same facts seen through images.hdr_to_ldr."""
    from renderformer_amd import images
    tol = 1e-12
    # below the knee it only subtracts the toe: min 0.5 >= 0.08 -> offset 0.04
    np.testing.assert_allclose(pbr_neutral64([0.5, 0.5, 0.5]), [0.46] * 3, rtol=0, atol=tol)
    np.testing.assert_allclose(pbr_neutral64([0.05, 0.3, 0.6]),
                               np.array([0.05, 0.3, 0.6]) - (0.05 - 6.25 * 0.0025), rtol=0, atol=tol)
    # continuous at x = 0.08: 0.08 - 6.25 * 0.0064 = 0.04 from the left, 0.04 from the right
    lo, hi = np.nextafter(0.08, 0), 0.08
    np.testing.assert_allclose(pbr_neutral64([lo, 0.3, 0.5]), pbr_neutral64([hi, 0.3, 0.5]), rtol=0, atol=tol)
    assert abs((0.08 - 6.25 * 0.08 * 0.08) - 0.04) < tol
    # continuous at peak = 0.76 (peak is taken after the offset: channel 0.80 with min >= 0.08): newPeak(0.76) =
    # 1 - 0.0576 / 0.24 = 0.76 and g = 0, so the compressed branch starts as the identity
    below = pbr_neutral64([0.2, 0.4, np.nextafter(0.80, 0)])
    above = pbr_neutral64([0.2, 0.4, np.nextafter(0.80, 1)])
    np.testing.assert_allclose(below, above, rtol=0, atol=tol)
    np.testing.assert_allclose(above, [0.16, 0.36, 0.76], rtol=0, atol=1e-9)
    # newPeak < 1 at peak = 1e3 (grey 1000.04): newPeak = 1 - 0.0576 / 999.48, and grey maps to newPeak itself
    new_peak = 1.0 - 0.0576 / (1000.0 + 0.24 - 0.76)
    out = pbr_neutral64([1000.04] * 3)
    assert new_peak < 1.0 and (out < 1.0).all()
    np.testing.assert_allclose(out, [new_peak] * 3, rtol=0, atol=tol)
    # equal channels stay equal; black stays black; an infinite channel is the curve's limit
    for grey in (0.0, 0.01, 0.08, 0.3, 0.9, 7.0, 1e30):
        o = pbr_neutral64([grey] * 3)
        assert o[0] == o[1] == o[2]
    np.testing.assert_array_equal(pbr_neutral64([0.0, 0.0, 0.0]), [0.0, 0.0, 0.0])
    np.testing.assert_array_equal(pbr_neutral64([np.inf, 0.2, 0.3]), [1.0, 1.0, 1.0])
    # the same through the float32 implementation
    px = np.array([[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.3, 0.3, 0.3], [7.0, 7.0, 7.0]], dtype=np.float32)
    q = images.hdr_to_ldr(px, "pbr_neutral")
    assert q[0, 0] == int(np.floor(255 * (1.055 * 0.46 ** (1 / 2.4) - 0.055)))
    assert (q[1] == 0).all() and all(len(set(row)) == 1 for row in q.tolist())


# ------------------------------------------------------------------------------------------------ the C entry point
def test_tonemap_entry_point_refuses_bad_arguments_without_device():
    import ctypes
    from renderformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librfhip.so not built")
    lib = _lib.load(require_device=False)
    P = ctypes.c_void_p
    good = dict(hdr=P(256), ldr=P(260), mapped=P(512), n_pix=5, mapper=1, gain=1.0)

    def rc(**bad):
        a = {**good, **bad}
        return lib.rf_tonemap_ldr8(a["hdr"], a["ldr"], a["mapped"], a["n_pix"], a["mapper"], a["gain"], None)

    for bad, msg in ((dict(ldr=None, mapped=None), b"null pointer"), (dict(hdr=None), b"null pointer"),
                     (dict(mapper=7), b"unknown mapper 7"), (dict(gain=0.0), b"gain"), (dict(gain=-1.0), b"gain"),
                     (dict(gain=float("nan")), b"gain"), (dict(gain=float("inf")), b"gain"),
                     (dict(hdr=P(260)), b"16-B aligned"), (dict(mapped=P(516)), b"16-B aligned"),
                     (dict(ldr=P(258)), b"4-B aligned"), (dict(n_pix=-1), b"pixels")):
        assert rc(**bad) == 1, bad  # RF_ERR_INVALID
        assert msg in lib.rf_last_error(), (bad, lib.rf_last_error())
    assert rc(n_pix=0) == 0  # nothing to do: RF_OK without a launch
    assert rc(n_pix=0, ldr=None) == 0 and rc(n_pix=0, mapped=None) == 0


def test_ops_wrapper_refuses_before_the_library_call():
    from renderformer_amd import ops
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="device tensor"):
        ops.tonemap_ldr8(x)
    with pytest.raises(ValueError, match="unknown mapper"):
        ops.tonemap_ldr8(x, "agx")


# ------------------------------------------------------------------------------------------------ CLI and pipeline
def test_cli_flags_and_unavailable_mappers(tmp_path):
    import argparse

    import batch_infer  # noqa: F401  (imports infer's helpers, device_ldr among them)
    import infer
    from renderformer_amd import RenderFormerRenderingPipeline
    p = argparse.ArgumentParser()
    infer.add_common_args(p)
    a = p.parse_args(["--tone_mapper", "pbr_neutral", "--exposure", "1.5"])
    assert a.tone_mapper == "pbr_neutral" and a.exposure == 1.5 and infer.device_ldr(a)
    d = p.parse_args([])
    assert d.tone_mapper == "none" and d.exposure == 0.0 and not infer.device_ldr(d)
    assert infer.device_ldr(p.parse_args(["--exposure", "-2"]))
    for name in ("agx", "filmic"):
        with pytest.raises(SystemExit) as e:
            infer.main(["--h5_file", str(tmp_path / "x.h5"), "--tone_mapper", name, "--model_id", "x"])
        assert f"tone mapper {name!r} needs simple_ocio's OCIO configs (not available); use --tone_mapper none" \
            == str(e.value)
        pipe = RenderFormerRenderingPipeline.__new__(RenderFormerRenderingPipeline)  # (the name is checked first)
        with pytest.raises(ValueError, match="needs simple_ocio's OCIO configs"):
            pipe.to_ldr(torch.zeros(2, 2, 3), name)
    with pytest.raises(ValueError, match="on the HIP device"):
        RenderFormerRenderingPipeline.__new__(RenderFormerRenderingPipeline).to_ldr(torch.zeros(2, 2, 3), "pbr_neutral")


def test_save_views_writes_the_given_ldr(tmp_path):
    import infer
    from renderformer_amd.images import hdr_to_ldr, read_png
    rng = np.random.default_rng(5)
    hdr = torch.from_numpy(rng.uniform(0, 2, size=(2, 6, 7, 3)).astype(np.float32))
    ldr = rng.integers(0, 256, size=(2, 6, 7, 3), dtype=np.uint8)
    for given in (ldr, torch.from_numpy(ldr)):
        paths = infer.save_views(hdr, str(tmp_path), "s", ldr=given)
        assert len(paths) == 4
        for i in range(2):
            np.testing.assert_array_equal(read_png(str(tmp_path / f"s_view_{i}.png")), ldr[i])
    infer.save_views(hdr, str(tmp_path), "s")
    np.testing.assert_array_equal(read_png(str(tmp_path / "s_view_1.png")), hdr_to_ldr(hdr[1].numpy()))
