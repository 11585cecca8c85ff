"""The phased 288x256 GEMM tile (RF_GEMM_TILE=288; csrc/gemm.hip phased_kernel<288>: 8 waves of 144 x 64, the A image's
18 sixteen-row pieces staged as 8 + 8 + 2): every epilogue of rf_gemm_bf16 / rf_gemm_f16, rf_gemm_qk_rope and the
deferred-RMSNorm consumer with the tile forced, against fp64 of the same rounded operands.  The shapes sit on the
tile's own edges: one row, either side of the 144-row wave boundary, a second m-tile with one valid row, one / two /
three / sixteen K-tiles (both LDS buffers and the prefetch tail)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import rf_ref

pytestmark = pytest.mark.gpu
dev = "cuda"

SHAPES = [(1, 256, 64), (143, 256, 128), (145, 512, 128), (289, 256, 192), (577, 768, 64), (300, 512, 1024)]
DTYPES = [torch.bfloat16, torch.float16]


def _ops():
    from renderformer_amd import ops
    return ops


def relerr(x, ref):
    return float((x.double() - ref).norm() / ref.norm())


@pytest.fixture(autouse=True)
def _force_tile(monkeypatch):
    monkeypatch.setenv("RF_GEMM_TILE", "288")  # (read per call)
    monkeypatch.setenv("RF_GEMM_PHASED", "1")


_cases = {}


def _case(m, n, k, dt):
    """Operands of one shape and operand type with their fp64 products, built once and left unchanged."""
    key = (m, n, k, dt)
    if key not in _cases:
        g = torch.Generator(device="cpu").manual_seed(m + 3 * n + k)
        a = torch.randn(m, k, generator=g).to(dt).to(dev)
        w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(dt).to(dev)
        bias = torch.randn(n, generator=g).to(dev)
        c0 = torch.randn(m, n, generator=g).to(dev)
        ref = a.double() @ w.double().t() + bias.double()
        h = n // 2
        refs = F.silu(a.double() @ w[:h].double().t()) * (a.double() @ w[h:].double().t())
        _cases[key] = (a, w, bias, c0, ref, refs)
    return _cases[key]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_tile288_epilogues(m, n, k, dt):
    """fp32, residual-add (accumulators started from the C tile), 16-bit (bf16 out of bf16 operands, fp16 out of fp16
    operands) and SwiGLU epilogues vs fp64, at test_gemm_256_tiles' tolerances."""
    ops = _ops()
    a, w, bias, c0, ref, refs = _case(m, n, k, dt)
    out = torch.empty(m, n, device=dev)
    ops.gemm(a, w, out, bias, ops.EPI_F32)
    e = relerr(out, ref)
    print(f"f32 {e:.2e}")
    assert e < 1e-5
    acc = c0.clone()
    ops.gemm(a, w, acc, bias, ops.EPI_ADD_F32)
    e = relerr(acc, c0.double() + ref)
    print(f"add {e:.2e}")
    assert e < 1e-5
    outh = torch.empty(m, n, device=dev, dtype=dt)
    ops.gemm(a, w, outh, bias, ops.EPI_BF16)
    e = relerr(outh, ref)
    print(f"16-bit {e:.2e}")
    assert e < 4e-3
    from renderformer_amd.model import _interleave_swiglu
    h = n // 2
    outs = torch.empty(m, h, device=dev, dtype=dt)
    ops.gemm(a, _interleave_swiglu(w[:h].cpu(), w[h:].cpu()).to(dev), outs, None, ops.EPI_SWIGLU)
    e = relerr(outs, refs)
    print(f"swiglu {e:.2e}")
    assert e < 5e-3


def _rope_ref(y, pos, freqs, H):
    """rope_apply of rope_cos_sin on the standard (half-split) layout, fp64; y [M, H*128]."""
    cos, sin = rf_ref.rope_cos_sin(pos.double()[None], freqs.double(), 128)
    return rf_ref.rope_apply(y.view(1, -1, H, 128).transpose(1, 2), cos, sin).transpose(1, 2).reshape(y.shape)


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("M,H", [(289, 2), (145, 4)])
def test_gemm_qk_rope_tile288(M, H, norm, f16):
    """rf_gemm_qk_rope on the 288-row tile: the fp64 restatement and bounds of test_qk_fused_gpu.py's
    test_gemm_qk_rope_matches_reference (5e-3 rel L2 per segment, rtol 2e-3 on the q/k sums), positions given.
    (289, 2): N = 768, one column tile each for q, k and v, the second m-tile with one valid row."""
    ops = _ops()
    D = H * 128
    K = D
    dt = torch.float16 if f16 else torch.bfloat16
    g = torch.Generator().manual_seed(M + H)
    xg = torch.randn(M, K, generator=g).to(dt)
    w = (torch.randn(3 * D, K, generator=g) / math.sqrt(K)).to(dt)
    ss = (torch.rand(M, ops.PRENORM_SLOTS, generator=g) * K / 4 + 1.0)
    ss[:, 5:] = 0
    gq = torch.rand(2 * D, generator=g) + 0.5
    pos = torch.rand(M, 9, generator=g) * 2 - 1
    freqs = 2 ** torch.linspace(0, math.log2(5), 6)
    perm = ops.rope_pair_perm(D)
    qkp = torch.cat([perm, perm + D, torch.arange(2 * D, 3 * D)])
    out = torch.empty(M, 3 * D, dtype=torch.bfloat16, device=dev)
    seg = torch.zeros(M, 2, ops.PRENORM_SLOTS, device=dev)
    qs = 0.37
    ops.gemm_qk_rope(xg.to(dev), w[qkp].contiguous().to(dev), out, ss.to(dev), 1e-6, D, 2,
                     gq[qkp[:2 * D]].to(dev) if norm else None, seg, pos.to(dev), freqs.to(dev), q_scale=qs)
    y = (xg.double() @ w.double().t()) / torch.sqrt(ss.double().sum(1, keepdim=True) / K + 1e-6)
    yq, yk, yv = y[:, :D], y[:, D:2 * D], y[:, 2 * D:]
    zq = _rope_ref(yq * (gq[:D].double() if norm else 1.0), pos, freqs, H) * qs
    zk = _rope_ref(yk * (gq[D:].double() if norm else 1.0), pos, freqs, H)
    ref = torch.cat([zq[:, perm], zk[:, perm], yv], 1)
    got = out.double().cpu()
    for name, a, b in (("q", got[:, :D], ref[:, :D]), ("k", got[:, D:2 * D], ref[:, D:2 * D]),
                       ("v", got[:, 2 * D:], ref[:, 2 * D:])):
        e = float((a - b).norm() / b.norm())
        print(f"{name}: rel L2 {e:.2e}")
        assert e < 5e-3, name
    if norm:
        sums = seg.sum(-1).double().cpu()
        for s_i, yy in ((0, yq), (1, yk)):
            exp = (yy ** 2).sum(1)
            print(f"sums {s_i}: max rel {float(((sums[:, s_i] - exp).abs() / exp).max()):.2e}")
            assert torch.allclose(sums[:, s_i], exp, rtol=2e-3), s_i


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_gemm_rownorm_tile288(dt):
    """The deferred-RMSNorm consumer (rf_gemm_rownorm with ss) on (289, 512, 128): out = (xg W^T) / rms from the staged
    slot sums, vs fp64, for the 16-bit epilogue with the q/k segment sums (whose partials this tile keeps in the rows'
    staged entries) and for SwiGLU.  Bounds: the 16-bit output's rounding as in test_gemm_tile288_epilogues (4e-3,
    5e-3); the segment sums are sums of squares of the values as written, summed in fp32 (256 terms: 1e-5)."""
    ops = _ops()
    m, n, k = 289, 512, 128
    a, w, _, _, _, _ = _case(m, n, k, dt)
    g = torch.Generator(device="cpu").manual_seed(7)
    ss = torch.rand(m, ops.PRENORM_SLOTS, generator=g) * k / 4 + 1.0
    ss[:, 3:] = 0
    ss = ss.to(dev)
    eps = 1e-6
    rs = 1.0 / torch.sqrt(ss.double().sum(1, keepdim=True) / k + eps)
    ref = (a.double() @ w.double().t()) * rs
    out = torch.empty(m, n, device=dev, dtype=dt)
    seg = torch.full((m, 2, ops.PRENORM_SLOTS), float("nan"), device=dev)
    ops.gemm_rownorm(a, w, out, ss, eps, ops.EPI_BF16, seg_ss=seg, seg_w=256)
    e = relerr(out, ref)
    print(f"rownorm 16-bit {e:.2e}")
    assert e < 4e-3
    written = (out.double() ** 2).view(m, 2, 256).sum(-1)
    es = float(((seg.double().sum(-1) - written).abs() / written).max())
    print(f"segment sums vs the written values: max rel {es:.2e}")
    assert es < 1e-5
    from renderformer_amd.model import _interleave_swiglu
    h = n // 2
    outs = torch.empty(m, h, device=dev, dtype=dt)
    ops.gemm_rownorm(a, _interleave_swiglu(w[:h].cpu(), w[h:].cpu()).to(dev), outs, ss, eps, ops.EPI_SWIGLU)
    refs = F.silu((a.double() @ w[:h].double().t()) * rs) * ((a.double() @ w[h:].double().t()) * rs)
    e = relerr(outs, refs)
    print(f"rownorm swiglu {e:.2e}")
    assert e < 5e-3
