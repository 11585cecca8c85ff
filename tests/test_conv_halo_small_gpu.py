"""conv3x3_hs_kernel: the halo-tiled 3x3 convolution for images too small for halo2 / halo3's 16 x 32 x 128 blocks
(RF_CONV_HALO_SMALL, default 1; 0 = the gathered engine launches; a geometry code forces one block geometry).
Tolerances are test_kernels_gpu.py::test_conv_halo3's: against an fp64 convolution of the same fp16-rounded operands,
fp32 output < 2e-5, SiLU fp16 planes < 1e-3, padded plane columns exactly zero; against the gathered engine kernel on
the same operands (same products, another fp32 summation order) < 1e-6.  Every case asks the planner
(rf_conv_plan_query) which kernel and block geometry its call launches before it launches it."""
import math

import pytest
import torch
import torch.nn.functional as F

from golden_util import load_case, rel_l2

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from renderformer_amd import _lib
    _lib.load()


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _h(t):
    """fp64 copy of an operand as the kernel sees it (fp16-rounded)."""
    return t.half().double()


# (cin, cout, height, width, images, knob)
CASES = [
    # host's choice (knob 1): all of these are too small for 256 blocks and take the smallest geometry, 8 x 16 x 32
    (32, 32, 8, 16, 1, "1"),     # one block whose every tap crosses the zero border
    (64, 64, 16, 32, 1, "1"),    # two chunks: double-buffer swap, last-chunk handling
    (96, 96, 16, 48, 3, "1"),    # tiles along x, image boundaries inside the grid, 3 filter tiles, odd chunk count
    (32, 32, 24, 16, 1, "1"),    # tiles along y
    (512, 32, 8, 16, 1, "1"),    # 16 chunks
    # host's choice reaching 256 blocks: the 128^2 level's 16 x 32 x 32 and the 64^2 level's 8 x 16 x 32
    (32, 256, 128, 128, 1, "1"),
    (32, 256, 64, 64, 1, "1"),
    # every geometry forced: tiles along both axes, two images, more than one filter tile, 2 or 3 chunks
    (64, 128, 32, 64, 2, "163264"),
    (96, 96, 16, 64, 2, "163232"),
    (64, 128, 16, 32, 2, "81664"),
    (96, 64, 16, 32, 2, "81632"),
]


@pytest.mark.parametrize("cin,cout,hh,ww,n_img,knob", CASES)
def test_conv_halo_small(cin, cout, hh, ww, n_img, knob, monkeypatch):
    """Bias + two residuals + SiLU fp16 planes with a padded row stride, and the plain fp32 form, for each shape:
    against fp64 on the same fp16 operands and against the gathered engine kernel (knob 0)."""
    from renderformer_amd.dpt import _Conv, split_planes
    monkeypatch.setenv("RF_CONV_HALO_SMALL", knob)
    g = torch.Generator(device="cpu").manual_seed(cin * hh + cout + ww + 23)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g)
    x = torch.randn(n_img, cin, hh, ww, generator=g)
    conv = _Conv(w, b, dev, f16=True)
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
    r1 = torch.randn(n_img, hh, ww, cout, generator=g)
    r2 = torch.randn(n_img, hh, ww, cout, generator=g)
    xs_silu = split_planes(xn, conv.cin_pad, silu=True, f16=True)
    xs = split_planes(xn, conv.cin_pad, f16=True)

    def fused():
        return conv(xs_silu, res1=r1.to(dev), res2=r2.to(dev), out_f32=True, planes_ld=cout + 32, planes_silu=True)

    def planned(kernels, code=None):
        from renderformer_amd._lib import CONVK
        for p in (conv.plan(xs_silu, planes_silu=True), conv.plan(xs)):
            assert p.kernel in [CONVK[k] for k in kernels] and code in (None, p.code) and not p.refuse, p

    planned(["hs"], int(knob) if knob != "1" else 163232 if hh == 128 else 81632)  # (the geometries CASES names)
    out, pl = fused()
    sx = _h(F.silu(x.double()).float())
    ref = F.conv2d(sx, _h(w), b.double(), padding=1).permute(0, 2, 3, 1) + r1 + r2
    e_out, e_pl = relerr(out.cpu(), ref), relerr(pl.hi.float()[..., :cout].cpu(), F.silu(ref))
    out2, _ = conv(xs, out_f32=True)
    ref2 = F.conv2d(_h(x), _h(w), b.double(), padding=1).permute(0, 2, 3, 1)
    e_out2 = relerr(out2.cpu(), ref2)
    monkeypatch.setenv("RF_CONV_HALO_SMALL", "0")  # the gathered engine kernel on the same operands
    planned(["ring", "ring_sk"])
    out3, pl3 = fused()
    out4, _ = conv(xs, out_f32=True)
    e_eng, e_eng2 = relerr(out.cpu(), out3.cpu()), relerr(out2.cpu(), out4.cpu())
    print(f"fused: fp32 {e_out:.2e} planes {e_pl:.2e}; plain: {e_out2:.2e}; vs engine: {e_eng:.2e} {e_eng2:.2e}")
    assert e_out < 2e-5
    assert e_pl < 1e-3
    assert (pl.hi[..., cout:] == 0).all()
    assert e_out2 < 2e-5
    assert e_eng < 1e-6 and e_eng2 < 1e-6
    assert relerr(pl.hi.float().cpu(), pl3.hi.float().cpu()) < 1e-3


def _frame(knob, monkeypatch):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    monkeypatch.setenv("RF_CONV_HALO_SMALL", knob)
    cfg, sd, inp, res, z = load_case("tiny_swin")
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd)).to("cuda")
    d = {k: v.cuda() for k, v in inp.items()}
    out = pipe(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"], d["fov"], resolution=res,
               torch_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    return out.float().cpu(), z


def test_frame_with_and_without_the_small_halo_kernel(monkeypatch):
    """tiny_swin rendered with the knob on and off: both inside the 1e-3 bar of the reference fixture and within 2e-4
    of each other (test_qk_fused_gpu.py's bar for two schedules of the same arithmetic)."""
    a, z = _frame("1", monkeypatch)
    b, _ = _frame("0", monkeypatch)
    ea, eb, d = rel_l2(a, z["hdr"]), rel_l2(b, z["hdr"]), rel_l2(a, b)
    print(f"knob 1 {ea:.3e}, knob 0 {eb:.3e}, 1 vs 0 {d:.3e}")
    assert ea < 1e-3 and eb < 1e-3 and d <= 2e-4
