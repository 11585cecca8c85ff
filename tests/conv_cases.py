"""The case table of the convolution kernel tests (test_conv_exact_gpu.py, the conv section of test_guard_bands_gpu.py
and the closure test in test_conv_cases.py).  Importable without a GPU.

A case names one call of a convolution entry point -- operand type, kind, shape, RF_CONV_* environment -- and the
(family, code) the planner (rf_conv_plan_query) must resolve it to; together the cases reach every production
instantiation listed in tests/golden/conv_plan_parent.json["kernels"] (test_conv_cases.py proves that from the built
library alone).  Shapes are the smallest at which a kernel can still go wrong: at least two images wherever the plan
allows (image seams inside the grid), tile seams on both axes where the kernel tiles, M-tails, padded filter banks.
Where a shape that an older test used does not plan to the wanted kernel with these image counts, the nearest one
that does is taken and the `note` says so.  RF_CONV_SMALL is never set (read once per process): an explicit
RF_CONV_TILE bypasses that rule.
"""
from collections import namedtuple

# prec: "f16" | "bf16x3"; kind: "conv" | "deconv" (k = kernel = stride) | "final" (the fused head, n_fin = 3)
Case = namedtuple("Case", "id prec kind cin cout k stride pad h w n env family code study note")


def _c(id, prec, kind, cin, cout, k, stride, pad, h, w, n, env, family, code, study=False, note=""):
    return Case(id, prec, kind, cin, cout, k, stride, pad, h, w, n, dict(env), family, code, study, note)


_H2 = {"RF_CONV_HALO2": "1", "RF_CONV_HALO3": "0", "RF_CONV_HK": "0"}
_HALO1 = {"RF_CONV_HALO": "1", "RF_CONV_SK": "0"}
_HALO0 = {"RF_CONV_HALO": "0", "RF_CONV_SK": "0"}

CASES = [
    # ---- conv3x3_hs_kernel: the host's choice, then each geometry forced (tiles along both axes, two images)
    _c("hs-one-block", "f16", "conv", 32, 32, 3, 1, 1, 8, 16, 1, {}, "hs", 81632,
       note="one block whose every tap crosses the zero border"),
    _c("hs-3img-3chunk", "f16", "conv", 96, 96, 3, 1, 1, 16, 48, 3, {}, "hs", 81632),
    _c("hs-163264", "f16", "conv", 64, 128, 3, 1, 1, 32, 64, 2, {"RF_CONV_HALO_SMALL": "163264"}, "hs", 163264),
    _c("hs-163232", "f16", "conv", 96, 96, 3, 1, 1, 16, 64, 2, {"RF_CONV_HALO_SMALL": "163232"}, "hs", 163232),
    _c("hs-81664", "f16", "conv", 64, 128, 3, 1, 1, 16, 32, 2, {"RF_CONV_HALO_SMALL": "81664"}, "hs", 81664),
    _c("hs-81632", "f16", "conv", 96, 64, 3, 1, 1, 16, 32, 2, {"RF_CONV_HALO_SMALL": "81632"}, "hs", 81632),
    # ---- halo2: every W ring depth on the 128- and the 64-channel block
    *[_c(f"halo2-{s}128", "f16", "conv", 32, 128, 3, 1, 1, 16, 32, 3, {**_H2, "RF_CONV_H2S": str(s)}, "halo2",
         1000 * s + 128) for s in (3, 4, 5)],
    *[_c(f"halo2-{s}064", "f16", "conv", 64, 64, 3, 1, 1, 32, 64, 2, {**_H2, "RF_CONV_H2S": str(s)}, "halo2",
         1000 * s + 64, note="tiles along both axes; (64, 64, 16, 32, 1) is the older test's") for s in (3, 4, 5)],
    _c("halo2-16chunk", "f16", "conv", 512, 128, 3, 1, 1, 16, 32, 3, {**_H2, "RF_CONV_SK": "0"}, "halo2", 4128),
    # ---- halo3
    _c("halo3", "f16", "conv", 32, 128, 3, 1, 1, 32, 64, 2, {"RF_CONV_HALO2": "1"}, "halo3", 0,
       note="(32, 128, 16, 32, 3) grown to 32 x 64 x 2 for tiles along both axes"),
    _c("halo3-16chunk", "f16", "conv", 512, 128, 3, 1, 1, 16, 32, 3, {"RF_CONV_HALO2": "1", "RF_CONV_SK": "0"},
       "halo3", 0),
    # ---- the fused head: conv3x3_c32_kernel, halo2's 64-channel block, the engine's 256x64 tile
    _c("head-c32", "f16", "final", 128, 32, 3, 1, 1, 32, 64, 2, {}, "c32", 0),
    _c("head-halo2", "f16", "final", 64, 32, 3, 1, 1, 32, 64, 2, {"RF_CONV_HALO2": "1", "RF_CONV_C32": "0"}, "halo2",
       4064),
    _c("head-ring", "f16", "final", 64, 32, 3, 1, 1, 24, 24, 2, {}, "ring", 25664),
    # ---- the gathered ring engine: M-tails, a padded filter bank, stride 2, 1x1
    _c("ring64-mtail", "f16", "conv", 64, 128, 3, 1, 1, 17, 17, 2, {}, "ring", 64),
    _c("ring64-padded-bank", "f16", "conv", 48, 200, 3, 1, 1, 9, 9, 2, {}, "ring", 64),
    _c("ring64-stride2", "f16", "conv", 128, 128, 3, 2, 1, 16, 16, 2, {}, "ring", 64),
    _c("sk1288-1x1", "f16", "conv", 1024, 128, 1, 1, 0, 16, 16, 2, {}, "ring_sk", 1288),
    _c("ring25664-bank32", "f16", "conv", 32, 32, 3, 1, 1, 9, 9, 2, {"RF_CONV_HALO_SMALL": "0"}, "ring", 25664,
       note="a bank of <= 64 filters outside the fused head: the 256x64 tile with an M-tail"),
    # ---- every RF_CONV_TILE code, gathered, data-parallel (RF_CONV_HALO=0) ...
    *[_c(f"tile{t}-gather", "f16", "conv", 64, 128, 3, 1, 1, 17, 17, 2, {**_HALO0, "RF_CONV_TILE": str(t)}, "ring", t)
      for t in (64, 128, 1288, 2561, 6412)],
    _c("tile256-gather", "f16", "conv", 64, 256, 3, 1, 1, 17, 17, 2, {**_HALO0, "RF_CONV_TILE": "256"}, "ring", 256),
    # ---- ... and halo-tiled (RF_CONV_HALO=1)
    *[_c(f"tile{t}-halo", "f16", "conv", 32, 128, 3, 1, 1, 16, 32, 3, {**_HALO1, "RF_CONV_TILE": str(t)}, "ring_halo", t)
      for t in (64, 128, 1288, 6412)],
    _c("tile256-halo", "f16", "conv", 32, 256, 3, 1, 1, 16, 32, 2, {**_HALO1, "RF_CONV_TILE": "256"}, "ring_halo", 256),
    _c("tile25664-halo", "f16", "conv", 32, 32, 3, 1, 1, 16, 32, 2, {**_HALO1, "RF_CONV_TILE": "64"}, "ring_halo", 25664),
    # (rows wider than the tile: seams along x too, which the 16 x 32 images above, narrower than every tile, lack)
    *[_c(f"tile{t}-halo-wide", "f16", "conv", 32, 128, 3, 1, 1, 4, wd, 2, {**_HALO1, "RF_CONV_TILE": str(t)}, "ring_halo",
         t) for t, wd in ((64, 128), (6412, 128), (128, 256), (1288, 256))],
    _c("tile256-halo-wide", "f16", "conv", 32, 256, 3, 1, 1, 2, 512, 2, {**_HALO1, "RF_CONV_TILE": "256"}, "ring_halo",
       256),
    _c("tile25664-halo-wide", "f16", "conv", 32, 32, 3, 1, 1, 2, 512, 2, {**_HALO1, "RF_CONV_TILE": "64"}, "ring_halo",
       25664),
    # ---- stream-K on the 64, 128 (4-wave) and 128w8 tiles (sk1288-1x1 above is the third)
    _c("sk64", "f16", "conv", 64, 128, 3, 1, 1, 17, 17, 2, {"RF_CONV_TILE": "6464"}, "ring_sk", 64),
    _c("sk128", "f16", "conv", 64, 128, 3, 1, 1, 17, 17, 2, {"RF_CONV_SKW8": "0", "RF_CONV_TILE": "128"}, "ring_sk", 128),
    _c("sk1288-3x3", "f16", "conv", 64, 128, 3, 1, 1, 17, 17, 2, {"RF_CONV_TILE": "1288"}, "ring_sk", 1288),
    # ---- deconvolutions (dense A): k = 2 and 4, each tile
    _c("deconv2", "f16", "deconv", 32, 32, 2, 0, 0, 9, 7, 2, {}, "ring", 1288),
    _c("deconv4", "f16", "deconv", 32, 16, 4, 0, 0, 9, 7, 2, {}, "ring", 1288),
    *[_c(f"deconv2-tile{t}", "f16", "deconv", 32, 32, 2, 0, 0, 9, 7, 2, {"RF_CONV_TILE": str(t)}, "ring", t)
      for t in (64, 128, 2561, 6412)],
    _c("deconv2-tile256", "f16", "deconv", 32, 64, 2, 0, 0, 9, 7, 2, {"RF_CONV_TILE": "256"}, "ring", 256),
    # ---- RF_CONV_PHASED=1: dense, gathered, and the persistent form (512 tiles of 256 x 256)
    _c("phased-dense", "f16", "deconv", 64, 64, 2, 0, 0, 9, 7, 2, {"RF_CONV_PHASED": "1", "RF_CONV_TILE": "256"},
       "phased", 0),
    _c("phased-gather", "f16", "conv", 64, 256, 3, 1, 1, 17, 17, 2, {"RF_CONV_PHASED": "1", "RF_CONV_TILE": "256",
                                                                   "RF_CONV_SK": "0"}, "phased", 0),
    _c("phased-persistent", "f16", "deconv", 64, 64, 2, 0, 0, 512, 256, 1, {"RF_CONV_PHASED": "1"}, "phased", 1,
       note="plane output only: 131,072 pixels, 512 tiles"),
    # ---- bf16x3: 128 and 256x128, data-parallel and stream-K, gathered and dense
    _c("bf-sk128", "bf16x3", "conv", 128, 32, 3, 1, 1, 5, 4, 2, {}, "ring_sk", 128),
    _c("bf-ring128", "bf16x3", "conv", 32, 32, 3, 1, 1, 5, 4, 2, {"RF_CONV_SK": "0"}, "ring", 128),
    _c("bf-ring2561", "bf16x3", "conv", 32, 200, 3, 1, 1, 17, 17, 2, {"RF_CONV_TILE": "256", "RF_CONV_SK": "0"}, "ring",
       2561),
    _c("bf-deconv2", "bf16x3", "deconv", 32, 32, 2, 0, 0, 9, 7, 2, {}, "ring", 128),
    _c("bf-deconv4", "bf16x3", "deconv", 32, 16, 4, 0, 0, 9, 7, 2, {}, "ring", 128),
    _c("bf-deconv2-2561", "bf16x3", "deconv", 32, 32, 2, 0, 0, 9, 7, 2, {"RF_CONV_TILE": "256"}, "ring", 2561),
    # ---- conv3x3_hk_kernel: study build only
    _c("hk", "f16", "conv", 32, 64, 3, 1, 1, 16, 32, 3, {"RF_CONV_HK": "1"}, "hk", 0, study=True),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# rf_conv2d_f16_group: test_conv_group_matches_single_launches' members (a deconvolution k = 4, a stride-2 3x3 with
# bias, two 3x3 of different sizes with fp32 + plane outputs); (kind, cin, cout, k, stride, pad, h, w, bias, out_f32)
GROUP = [("deconv", 64, 128, 4, 0, 0, 12, 12, True, False), ("conv", 96, 128, 3, 2, 1, 20, 20, True, False),
         ("conv", 64, 256, 3, 1, 1, 24, 24, False, True), ("conv", 256, 256, 3, 1, 1, 9, 9, False, True)]
# rf_conv1x1_f16_group: four 1x1 projections over one image size, one without bias, one cin_pad that is no multiple
# of 64 in a second group (the gathered 32-deep loop instead of the dense 64-deep one); (cin, cout, bias)
GROUP_1X1 = {"dense": [(128, 128, True), (64, 256, True), (192, 128, False), (64, 200, True)],
             "gathered": [(96, 128, True), (64, 128, False)]}
GROUP_1X1_HW = (9, 7, 2)  # h, w, images: 126 pixels, an M-tail on the 128-row tile

FLAG_FINAL = 4


def knobs():
    """The environment variables a case may set: cleared before each case so none leaks from the caller's shell."""
    import re
    return re.compile(r"RF_(CONV|H2|H3)_|RF_GEMM_(PHASED|PERSIST)")


def set_env(case, monkeypatch):
    """The case's environment and nothing else of the conv knobs; a study-only case skips on the production build."""
    import os
    for k in [k for k in os.environ if knobs().match(k)]:
        monkeypatch.delenv(k)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if case.study:
        from conftest import needs_study
        needs_study(case.id)


def assert_plan(case, launch, flags=0, n_fin=0):
    """The launch about to be made runs the kernel the case names (asked of the planner, with the call's own flags)."""
    from renderformer_amd._lib import CONVK
    p = launch.plan(flags, n_fin)
    assert (p.kernel, p.code, p.refuse) == (CONVK[case.family], case.code, 0), (case.id, p)


def launcher(case, x, w, bias=None, res1=None, res2=None, x_lo=None, device="cuda"):
    """kernel_checks.ConvLaunch of the case on these operands (weights through dpt._Conv's layout)."""
    import kernel_checks as kc
    from renderformer_amd.dpt import _Conv
    conv = _Conv(w, None, device, deconv=case.kind == "deconv", f16=case.prec == "f16")
    return kc.ConvLaunch(conv, x, x_lo, stride=case.stride or 1, pad=case.pad, bias=bias, res1=res1, res2=res2,
                         device=device)


def exact_case(case, device="cuda", seed=0, amax=3):
    """The random-integer form of a case: (launch, fp64 reference NHWC).  Bias and, for a convolution, two residuals."""
    import kernel_checks as kc
    dk = case.k if case.kind == "deconv" else 0
    x, w, b, r1, r2 = kc.int_conv_operands(case.n, case.cin, case.cout, case.k, case.k, case.h, case.w, seed=seed,
                                           amax=amax, stride=case.stride or 1, pad=case.pad, deconv=dk)
    if dk:
        r1 = r2 = None
    ref = kc.conv_ref(x, w, b, r1, r2, case.stride or 1, case.pad, dk)
    return launcher(case, x, w, b, r1, r2, device=device), ref


def mask_case(case, border, device="cuda"):
    """The tap-mask form of a case: (launch, fp64 reference NHWC); border: with the integer border-class bias rows."""
    import kernel_checks as kc
    dk = case.k if case.kind == "deconv" else 0
    x, w, b9 = kc.tap_mask_operands(case.n, case.cin, case.cout, case.k, case.k, case.h, case.w, deconv=dk)
    bias = b9 if border else None
    return launcher(case, x, w, bias, device=device), kc.conv_ref(x, w, bias, None, None, case.stride or 1, case.pad, dk)


def takes_border_bias(case):
    return case.kind == "conv" and case.k == 3 and case.stride == 1 and case.pad == 1 and case.h >= 2 and case.w >= 2


def plan_of(case):
    """The plan of the case under the environment as it stands (the caller has set case.env)."""
    from renderformer_amd import _lib
    f16 = case.prec == "f16"
    ws = int(_lib.load(require_device=False).rf_gemm_workspace_bytes())
    cin_pad = -(-case.cin // 32) * 32
    if case.kind == "deconv":
        return _lib.conv_plan(f16, case.n, case.h, case.w, cin_pad, case.cout, deconv_k=case.k, ws_bytes=ws)
    cout_pad = 64 if f16 and case.cout <= 64 else -(-case.cout // 128) * 128
    fin = case.kind == "final"
    return _lib.conv_plan(f16, case.n, case.h, case.w, cin_pad, case.cout, cout_pad, case.k, case.k, case.stride,
                          case.pad, FLAG_FINAL if fin else 0, 3 if fin else 0, 0, ws)
