"""The conv planner (gemm.hip conv_plan, queried through rf_conv_plan_query; host arithmetic, no GPU) chooses, for
every call and RF_CONV_* environment of tests/golden/conv_plan_parent.json, the kernel, grid and block that the commit
before the planner launched.  The table was recorded from that commit's own dispatch: its RF_LAUNCH redefined to
note the kernel's address (resolved to the instantiation's name with nm) and the launch dimensions instead of
launching, and rf_conv2d_* / rf_deconv2d_* called through ctypes under each environment.  It holds every DPT
convolution of the 512^2 frame and of tiny_swin with both operand types, with and without a stream-K workspace,
each conv3x3_hs_kernel geometry, shapes no halo kernel admits, several images per launch, and every conv knob of
DESIGN.md §3.1 at each of its values."""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

with open(os.path.join(REPO, "tests", "golden", "conv_plan_parent.json")) as _f:
    TABLE = json.load(_f)
KNOB = re.compile(r"RF_(CONV|H2|H3)_|RF_GEMM_(PHASED|PERSIST)")
ONCE = "RF_CONV_SMALL"  # read once per process: its cases run in a child process started with it set
GROUPS = [i for i, c in enumerate(TABLE["cases"]) if ONCE not in c["env"]]
CHILD_GROUPS = [i for i, c in enumerate(TABLE["cases"]) if ONCE in c["env"]]

# ConvTile code -> the tile's template arguments
TILES = {64: "64, 64, 2, 2, 8, 1", 128: "128, 128, 2, 2, 3, 1", 1288: "128, 128, 2, 4, 3, 1", 256: "256, 256, 2, 4, 4, 1",
         2561: "256, 128, 4, 2, 3, 1", 6412: "64, 128, 2, 2, 6, 1", 25664: "256, 64, 4, 1, 4, 1"}


def _lib():
    import torch  # noqa: F401
    from renderformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librfhip.so not built (run __graft_entry__.build())")
    return _lib


def kernel_name(plan, f16, gather):
    """The instantiation a plan names, as nm prints it (E_CONV = 16; operands: 2 = fp16, 3 = bf16x3)."""
    from renderformer_amd._lib import CONVK
    nt, g, k, c = 2 if f16 else 3, "true" if gather else "false", plan.kernel, plan.code
    if k in (CONVK["ring"], CONVK["ring_sk"]):
        return f"engine_kernel<Tile<{TILES[c]}>, 16, {nt}, {g}, {'true' if k == CONVK['ring_sk'] else 'false'}>"
    return {CONVK["ring_halo"]: lambda: f"halo_kernel<Tile<{TILES[c]}>, 16>",
            CONVK["phased"]: lambda: "phased_sk_kernel<16, 2>" if c else f"phased_kernel<256, 16, 2, {g}>",
            CONVK["halo2"]: lambda: f"halo2_kernel<{c // 1000}, {c % 1000}, {plan.dbg}>",
            CONVK["halo3"]: lambda: f"halo3_kernel<{plan.dbg}>",
            CONVK["c32"]: lambda: "conv3x3_c32_kernel",
            CONVK["hk"]: lambda: "conv3x3_hk_kernel",
            CONVK["hs"]: lambda: f"conv3x3_hs_kernel<{c // 10000}, {c // 100 % 100}, {c % 100}>"}[k]()


def mismatches(lib, group):
    """Rows of one environment group whose plan is not what the parent launched (the environment is already set)."""
    bad = []
    case = TABLE["cases"][group]
    for ci, rc, ki, grid, block in case["rows"]:
        call = dict(zip(TABLE["call_fields"], TABLE["calls"][ci]))
        ws = int(lib.load(require_device=False).rf_gemm_workspace_bytes()) if call.pop("ws") else 0
        f16 = bool(call.pop("f16"))
        plan = lib.conv_plan(f16, ws_bytes=ws, **call)
        if rc == 3:  # the parent refused: a study-only kernel asked of the production build
            got, want = (plan.refuse,), (1,)
        else:
            got = (plan.refuse, kernel_name(plan, f16, call["deconv_k"] == 0), plan.grid, plan.block)
            want = (0, TABLE["kernels"][ki], grid, block)
        if got != want:
            bad.append(f"{case['env']} {call} f16={f16} ws={ws > 0}: planned {got} {plan!r}, the parent launched {want}")
    return bad


def _production(lib):
    if lib.study_build():
        pytest.skip("the table was recorded from the production build (RF_LIB points at the study build)")


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: ",".join(f"{k[3:]}={v}" for k, v in
                                                                  TABLE["cases"][g]["env"].items()) or "default")
def test_plan_matches_what_the_parent_launched(group, monkeypatch):
    lib = _lib()
    _production(lib)
    for k in [k for k in os.environ if KNOB.match(k)]:
        monkeypatch.delenv(k)
    for k, v in TABLE["cases"][group]["env"].items():
        monkeypatch.setenv(k, v)
    bad = mismatches(lib, group)
    assert not bad, "\n".join(bad)


def test_plan_matches_the_parent_with_the_small_level_tiles_off():
    """RF_CONV_SMALL=0 is read once per process, so its cases are planned in a child process started with it."""
    lib = _lib()
    _production(lib)
    env = {k: v for k, v in os.environ.items() if not KNOB.match(k)}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env={**env, ONCE: "0"}, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert CHILD_GROUPS and f"{sum(len(TABLE['cases'][g]['rows']) for g in CHILD_GROUPS)} rows" in r.stdout


def test_table_covers_what_it_claims():
    """Every kernel family and ring tile, each hs geometry, refusals, both operand types, deconvolutions, calls without
    a workspace and several images appear in the recorded table."""
    names = " ".join(TABLE["kernels"])
    for part in ("engine_kernel", "true, true>", "halo_kernel", "phased_kernel", "phased_sk_kernel", "halo2_kernel<3, 64",
                 "halo2_kernel<5, 128", "halo3_kernel<0>", "conv3x3_c32_kernel", "<16, 32, 64>", "<16, 32, 32>",
                 "<8, 16, 64>", "<8, 16, 32>", ", 16, 3, true, false>", ", 16, 3, false, false>"):
        assert part in names, part
    for t in TILES.values():
        assert f"Tile<{t}>" in names, t
    rows = [r for c in TABLE["cases"] for r in c["rows"]]
    # (return code 2: launched; the recording machine had no device, so the launch's own status is an error)
    assert sum(r[1] == 3 for r in rows) >= 3 and all((r[1] == 3) == (r[2] < 0) and r[1] in (0, 2, 3) for r in rows)
    f = TABLE["call_fields"]
    assert {c[f.index("ws")] for c in TABLE["calls"]} == {0, 1} and max(c[f.index("n_img")] for c in TABLE["calls"]) >= 3
    knobs = {k for c in TABLE["cases"] for k in c["env"]}
    assert {"RF_CONV_TILE", "RF_CONV_HALO", "RF_CONV_HALO2", "RF_CONV_HALO3", "RF_CONV_H2S", "RF_CONV_C32", "RF_CONV_HK",
            "RF_CONV_HALO_SMALL", "RF_CONV_PHASED", "RF_CONV_SK", "RF_CONV_SKW8", "RF_CONV_SMALL", "RF_H2_DBG",
            "RF_H3_DBG"} <= knobs


# default knobs, one image, fp16: (cin, cout, hw, k, final head) -> family, grid, block
SPOT = [((256, 128, 512, 3, False), "halo3", 512, 512), ((128, 32, 512, 3, False), "halo2", 512, 512),
        ((128, 32, 512, 3, True), "c32", 512, 256), ((256, 256, 256, 3, False), "halo3", 256, 512),
        ((256, 256, 128, 3, False), "hs", 256, 256), ((256, 256, 64, 3, False), "hs", 256, 256),
        ((1024, 256, 64, 3, False), "hs", 256, 256), ((256, 256, 32, 3, False), "hs", 64, 256),
        ((1024, 256, 32, 3, False), "hs", 64, 256), ((256, 256, 20, 3, False), "ring", 28, 256),
        ((32, 32, 16, 3, False), "hs", 2, 256), ((256, 256, 64, 1, False), "ring", 64, 512)]


@pytest.mark.parametrize("shape,family,grid,block", SPOT)
def test_default_plans_of_the_frame(shape, family, grid, block, monkeypatch):
    lib = _lib()
    for k in [k for k in os.environ if KNOB.match(k)]:
        monkeypatch.delenv(k)
    cin, cout, hw, k, final = shape
    p = lib.conv_plan(True, 1, hw, hw, cin, cout, 64 if cout <= 64 else cout, k, k, 1, k // 2, 4 if final else 0,
                      3 if final else 0, ws_bytes=int(lib.load(require_device=False).rf_gemm_workspace_bytes()))
    assert (p.kernel, p.grid, p.block, p.refuse) == (lib.CONVK[family], grid, block, 0), p


def test_query_is_pure_and_validates():
    """A successful query leaves rf_last_error alone and repeats itself; shapes the entry points reject are
    RF_ERR_INVALID for the query too, zero kernel sizes and strides included.  Where no device is present the real
    entry points are given the same shapes with dummy pointers (they validate before they touch the device; with a
    device a loosened check would launch on those pointers, so there the query alone is asked)."""
    import ctypes
    lib = _lib()
    L = lib.load(require_device=False)
    out = lib.ConvPlan()
    q = lambda *a: L.rf_conv_plan_query(*a, ctypes.addressof(out))  # noqa: E731
    good = (1, 0, 1, 64, 64, 256, 256, 256, 3, 3, 1, 1, 0, 0, 0)
    assert q(1, 0, 1, 64, 64, 100, 256, 256, 3, 3, 1, 1, 0, 0, 0) == 1  # cin_pad % 32
    err = L.rf_last_error()
    assert b"cin_pad" in err
    assert q(*good) == 0 and L.rf_last_error() == err
    first = bytes(out)
    assert q(*good) == 0 and bytes(out) == first and L.rf_last_error() == err
    import torch
    d = ctypes.c_void_p(16)
    no_device = not torch.cuda.is_available()
    bad = {"stride 0": dict(stride=0), "kw 0": dict(kw=0), "kh 0": dict(kh=0),
           "cout_pad 96": dict(cout=96, cout_pad=96), "cout_pad < cout": dict(cout=256, cout_pad=128),
           "K >= 65536": dict(cin_pad=8192), "cout % 4": dict(cout=30, cout_pad=64),
           "final head of 128 filters": dict(cout=128, cout_pad=128, flags=4, n_fin=3),
           "final head without outputs": dict(cout=32, cout_pad=64, flags=4, n_fin=0),
           "border bias on a 1x1": dict(kh=1, kw=1, pad=0, flags=32),
           "border bias on the final head": dict(cout=32, cout_pad=64, flags=32 | 4, n_fin=3)}
    base = dict(n_img=1, hi=64, wi=64, cin_pad=256, cout=256, cout_pad=256, kh=3, kw=3, stride=1, pad=1, flags=0, n_fin=0)
    for what, change in bad.items():
        c = {**base, **change}
        with pytest.raises(ValueError):
            lib.conv_plan(True, **c)
        if no_device:
            rc = L.rf_conv2d_f16(d, c["n_img"], c["hi"], c["wi"], c["cin_pad"], d, c["cout"], c["cout_pad"], c["kh"],
                                 c["kw"], c["stride"], c["pad"], d, None, None, d, None, 0, c["flags"], d, d, c["n_fin"],
                                 1.0, None, 0, None)
            assert rc == 1, what
    with pytest.raises(ValueError):  # bf16x3 banks are multiples of 128 (64 is the fp16 path's)
        lib.conv_plan(False, **{**base, "cout": 32, "cout_pad": 64})
    with pytest.raises(ValueError):  # k*k*cout % 128
        lib.conv_plan(True, 1, 8, 8, 32, 24, deconv_k=2)
    if no_device:
        assert L.rf_deconv2d_f16(d, 1, 8, 8, 32, d, 24, 2, d, d, None, 0, None, 0, None) == 1
        assert L.rf_deconv2d_f16(d, 1, 8, 8, 32, d, 32, 0, d, d, None, 0, None, 0, None) == 1  # k = 0
    assert L.rf_conv_plan_query(7, 0, 1, 64, 64, 256, 256, 256, 3, 3, 1, 1, 0, 0, 0, ctypes.addressof(out)) == 1
    assert L.rf_conv_plan_query(1, 0, 1, 64, 64, 256, 256, 256, 3, 3, 1, 1, 0, 0, 0, None) == 1
    assert lib.conv_plan(True, 0, 64, 64, 256, 256, 256).kernel == lib.CONVK["none"]  # no output pixels: no launch


if __name__ == "__main__":  # the child of test_plan_matches_the_parent_with_the_small_level_tiles_off
    import torch  # noqa: F401
    from renderformer_amd import _lib as lib_
    n, failed = 0, []
    for g_ in CHILD_GROUPS:
        for k_ in [k for k in os.environ if KNOB.match(k)]:
            del os.environ[k_]
        os.environ.update(TABLE["cases"][g_]["env"])
        failed += mismatches(lib_, g_)
        n += len(TABLE["cases"][g_]["rows"])
    print("\n".join(failed))
    print(f"{n} rows")
    sys.exit(1 if failed else 0)
