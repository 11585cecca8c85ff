"""G-buffer: what can be checked without a device.  The two C entry points' argument checks against the built
library, pipe.gbuffer's argument errors, the fp64 reference of tests/visibility_checks.py against hand-computed
cases, the conformance meshes under that reference (and under the naive fp32 statements they are there to catch),
the band caps of the GPU cases' inputs, and the CLI flag."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import visibility_checks as vc  # noqa: E402
from golden_util import load_case  # noqa: E402

P = ctypes.c_void_p


# ------------------------------------------------------------------------------------------------ the C entry points
def test_primary_hits_refuses_bad_arguments_without_device():
    from renderformer_amd import _lib
    lib = _lib.load(require_device=False)
    good = dict(tris=P(256), valid_idx=P(512), scene_off=P(768), c2w=P(1024), fov=P(1280), intr=None, n_scenes=2,
                n_views=3, n_per=100, n_valid=150, h=45, w=99, depth=P(2048), tri_id=P(4096), bary=P(8192),
                alpha=P(16384), work=P(32768), work_floats=32 * 3 * 150)

    def rc(**bad):
        a = {**good, **bad}
        return lib.rf_primary_hits(a["tris"], a["valid_idx"], a["scene_off"], a["c2w"], a["fov"], a["intr"],
                                   a["n_scenes"], a["n_views"], a["n_per"], a["n_valid"], a["h"], a["w"], a["depth"],
                                   a["tri_id"], a["bary"], a["alpha"], a["work"], a["work_floats"], None)

    cases = [(dict(tris=None), b"null pointer"), (dict(valid_idx=None), b"null pointer"),
             (dict(scene_off=None), b"null pointer"), (dict(c2w=None), b"null pointer"),
             (dict(depth=None), b"null pointer"), (dict(tri_id=None), b"null pointer"),
             (dict(intr=P(1536)), b"exactly one of fov_deg and intr"), (dict(fov=None), b"exactly one of fov_deg and intr"),
             (dict(h=0), b"positive frame"), (dict(w=-3), b"positive frame"),
             (dict(h=65536, w=32768), b"do not fit a 32-bit index"), (dict(n_views=65536), b"at most 65535 views"),
             (dict(n_scenes=65536, n_per=1), b"at most 65535 scenes"), (dict(n_per=0), b"n_tris_per_scene"),
             (dict(n_scenes=65535, n_per=65535), b"n_tris_per_scene"), (dict(n_valid=-1), b"n_valid"),
             (dict(n_valid=201, work_floats=1 << 40), b"n_valid"),
             (dict(work_floats=32 * 3 * 150 - 1), b"32 * n_views * n_valid = 14400 are needed"),
             (dict(work=None), b"workspace"), (dict(work=P(32772)), b"16-B aligned")]
    for bad, msg in cases:
        assert rc(**bad) == 1, bad  # RF_ERR_INVALID, before any launch
        assert msg in lib.rf_last_error(), (bad, lib.rf_last_error())
    assert rc(n_scenes=0, n_valid=0, work_floats=0, work=None) == 0  # nothing to do: RF_OK without a launch
    assert rc(n_views=0, work_floats=0, work=None) == 0


def test_gbuffer_shade_refuses_bad_arguments_without_device():
    from renderformer_amd import _lib
    lib = _lib.load(require_device=False)
    good = dict(tri_id=P(256), bary=P(512), vn=P(768), texture=P(1024), row=13 * 1024, chan=1024, n_per=100, n_scenes=2,
                pix=4096, alpha=P(2048), normal=P(4096), albedo=P(8192))

    def rc(**bad):
        a = {**good, **bad}
        return lib.rf_gbuffer_shade(a["tri_id"], a["bary"], a["vn"], a["texture"], a["row"], a["chan"], a["n_per"],
                                    a["n_scenes"], a["pix"], a["alpha"], a["normal"], a["albedo"], None)

    cases = [(dict(tri_id=None), b"null pointer"), (dict(alpha=None, normal=None, albedo=None), b"null pointer"),
             (dict(bary=None), b"normal needs bary and vn"), (dict(vn=None), b"normal needs bary and vn"),
             (dict(texture=None), b"albedo needs texture"), (dict(chan=0), b"does not hold three channels"),
             (dict(row=2, chan=1), b"does not hold three channels"), (dict(n_per=0), b"n_tris_per_scene"),
             (dict(n_scenes=1 << 16, n_per=1 << 16), b"n_tris_per_scene"), (dict(pix=0), b"pix_per_scene"),
             (dict(pix=1 << 40), b"pix_per_scene")]
    for bad, msg in cases:
        assert rc(**bad) == 1, bad
        assert msg in lib.rf_last_error(), (bad, lib.rf_last_error())
    assert rc(n_scenes=0) == 0
    # an output that is not asked for needs none of its inputs
    assert rc(n_scenes=0, normal=None, bary=None, vn=None) == 0 and rc(n_scenes=0, albedo=None, texture=None) == 0


def test_python_constants_match_the_header():
    from renderformer_amd import ops
    text = open(os.path.join(REPO, "include", "rf.h")).read()
    assert f"#define RF_VIS_TILE {ops.VIS_TILE}\n" in text and f"#define RF_VIS_CHUNK {ops.VIS_CHUNK}\n" in text
    assert f"work: {ops.VIS_RECORD_FLOATS} * n_views * n_valid floats" in text


# ------------------------------------------------------------------------------------------------ pipeline arguments
def test_pipeline_gbuffer_argument_errors():
    from renderformer_amd import RenderFormerRenderingPipeline
    from renderformer_amd.gbuffer import OUTPUTS, check_outputs
    cfg = load_case("tiny_swin")[0]
    pipe = RenderFormerRenderingPipeline.__new__(RenderFormerRenderingPipeline)  # (no model: the checks come first)
    pipe.config = cfg
    tri, tex, mask, vn = torch.zeros(1, 4, 3, 3), torch.zeros(1, 4, 13, 32, 32), torch.ones(1, 4, dtype=torch.bool), \
        torch.zeros(1, 4, 3, 3)
    c2w, fov, k = torch.eye(4).repeat(1, 2, 1, 1), torch.full((1, 2), 40.0), torch.ones(1, 2, 4)
    with pytest.raises(ValueError, match="exactly one of fov and intrinsics"):
        pipe.gbuffer(tri, tex, mask, vn, c2w, fov, 64, intrinsics=k)
    with pytest.raises(ValueError, match="exactly one of fov and intrinsics"):
        pipe.gbuffer(tri, tex, mask, vn, c2w, None, 64)
    with pytest.raises(ValueError, match=r"intrinsics must be \[B, V, 4\]"):
        pipe.gbuffer(tri, tex, mask, vn, c2w, None, 64, intrinsics=torch.ones(1, 2, 3))
    with pytest.raises(ValueError, match="incompatible with patch/window size"):
        pipe.gbuffer(tri, tex, mask, vn, c2w, fov, (45, 99))
    with pytest.raises(ValueError, match="unknown outputs"):
        pipe.gbuffer(tri, tex, mask, vn, c2w, fov, 64, outputs=("alpha", "velocity"))
    # a valid call up to the tensors' device: host tensors are refused, with overscan too
    for kw in (dict(resolution=64), dict(resolution=(45, 99), overscan=True)):
        with pytest.raises(ValueError, match="must be a tensor on the HIP device"):
            pipe.gbuffer(tri, tex, mask, vn, c2w, fov, **kw)
    with pytest.raises(ValueError, match="needs an EncodedScene"):
        pipe.gbuffer_encoded(object(), c2w, fov, 64)
    assert check_outputs(None) == OUTPUTS and check_outputs(["depth", "alpha"]) == ("alpha", "depth")
    assert check_outputs("tri_id") == ("tri_id",)
    with pytest.raises(ValueError, match="empty"):
        check_outputs(())


def test_ops_wrappers_refuse_before_the_library_call():
    from renderformer_amd import ops
    t = torch.zeros(1, 4, 9)
    i = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        ops.primary_hits(t, i, i, 4, torch.eye(4).repeat(1, 1, 1, 1), torch.ones(1, 1), None, 8)
    with pytest.raises(ValueError, match="at least one of alpha, normal and albedo"):
        ops.gbuffer_shade(torch.zeros(1, 2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32 device tensor"):
        ops.gbuffer_shade(torch.zeros(1, 2, 2, dtype=torch.int32), alpha=True)


def test_scene_tables_are_the_plans_tables():
    from renderformer_amd.gbuffer import scene_tables
    from renderformer_amd.model import _build_plan
    m = np.zeros((3, 9), bool)
    m[0, [1, 4, 8]] = True
    m[2, :] = True
    valid, off, n = scene_tables(m, "cpu")
    plan = _build_plan(m, 1, 64, 8, 16, "cpu")
    assert n == 12 == plan.T_tri and valid.dtype == torch.int32 and off.dtype == torch.int32
    assert torch.equal(valid, plan.valid_flat) and torch.equal(off, plan.scene_off)
    assert off.tolist() == [0, 3, 3, 12] and valid[:3].tolist() == [1, 4, 8]


# ------------------------------------------------------------------------------------------------ the reference, by hand
def _one_view(tris, frame=(1, 1), origin=(0.0, 0.0, 0.0)):
    """hits_ref of triangles [n, 9] for an identity camera at `origin` with a 90 degree field of view: pixel (0, 0)
    of the 1 x 1 frame looks straight down -z."""
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor(origin)
    t = torch.tensor(tris, dtype=torch.float32).reshape(1, -1, 9)
    mask = torch.ones(1, t.shape[1], dtype=torch.bool)
    return vc.scene_ref(t, mask, c2w[None, None], torch.tensor([[90.0]]), None, frame)[0][0]


FRONT = [-1.0, -1.0, -2.0, 3.0, -1.0, -2.0, -1.0, 3.0, -2.0]  # counter-clockwise seen from the origin, in z = -2


def test_reference_single_triangle_by_hand():
    r = _one_view([FRONT])
    # the ray (0, 0, -1) meets z = -2 at (0, 0, -2) = v0 + 0.25 e1 + 0.25 e2, at distance 2
    assert r["tri_id"][0, 0] == 0 and r["depth"][0, 0] == 2.0
    assert r["u"][0, 0] == 0.25 and r["v"][0, 0] == 0.25 and not r["band"][0, 0]
    assert r["f32_depth"][0, 0] == 2.0 and r["tol"] == vc.DEPTH_FLOOR
    # a 2 x 2 frame: the corner pixels look along (+-0.5, +-0.5, -1) / |.|, distance 2 |(0.5, 0.5, 1)| = sqrt(6)
    r2 = _one_view([FRONT], frame=(2, 2))
    np.testing.assert_allclose(r2["depth"], np.sqrt(6.0), rtol=1e-15)
    # pixel (x = 1, y = 0): camera direction (+0.5, +0.5, -1) meets the plane at (1, 1, -2): u = v = 0.5, on the
    # hypotenuse; (x = 0, y = 1) meets it at (-1, -1, -2), the vertex v0; the other two at the midpoints of the legs.
    # Edges are closed (all four are hits) and every one of them is banded
    assert abs(r2["u"][0, 1] - 0.5) < 1e-15 and abs(r2["v"][0, 1] - 0.5) < 1e-15
    assert abs(r2["u"][1, 0]) < 1e-15 and abs(r2["v"][1, 0]) < 1e-15
    assert (r2["tri_id"] == 0).all() and r2["band"].all()


def test_reference_back_face_behind_degenerate_and_ties():
    back = FRONT[0:3] + FRONT[6:9] + FRONT[3:6]  # the other winding: still hit
    r = _one_view([back])
    assert r["tri_id"][0, 0] == 0 and r["depth"][0, 0] == 2.0 and r["u"][0, 0] == 0.25
    behind = [c if i % 3 != 2 else 2.0 for i, c in enumerate(FRONT)]  # the same triangle in z = +2
    r = _one_view([behind])
    assert r["tri_id"][0, 0] == -1 and np.isposinf(r["depth"][0, 0]) and r["u"][0, 0] == 0.0
    # zero area: a repeated vertex, and three collinear points whose segment the ray crosses
    for flat in ([-1.0, -1.0, -2.0, -1.0, -1.0, -2.0, 3.0, 3.0, -2.0], [-1.0, 0.0, -2.0, 0.0, 0.0, -2.0, 2.0, 0.0, -2.0]):
        r = _one_view([flat])
        assert r["tri_id"][0, 0] == -1 and not r["band"][0, 0]
    r = _one_view([[float("nan")] + FRONT[1:]])
    assert r["tri_id"][0, 0] == -1
    # two identical triangles: the lower index; a nearer one behind them in the list still wins
    r = _one_view([FRONT, FRONT])
    assert r["tri_id"][0, 0] == 0 and r["band"][0, 0]  # (the second hit lies at the same depth: banded)
    assert r["allowed"][0] == {0, 1}
    near = [c if i % 3 != 2 else -1.0 for i, c in enumerate(FRONT)]
    r = _one_view([FRONT, FRONT, near])
    assert r["tri_id"][0, 0] == 2 and r["depth"][0, 0] == 1.0
    # the origin is the camera's translation: moved to z = 5 the plane z = -2 is 7 away
    assert _one_view([FRONT], origin=(0.0, 0.0, 5.0))["depth"][0, 0] == 7.0


def test_ids_follow_the_input_axis_in_the_reference():
    t = torch.full((1, 5, 9), float("nan"))
    t[0, 3] = torch.tensor(FRONT)
    mask = torch.zeros(1, 5, dtype=torch.bool)
    mask[0, 3] = True
    r = vc.scene_ref(t, mask, torch.eye(4)[None, None], torch.tensor([[90.0]]), None, (1, 1))[0][0]
    assert r["tri_id"][0, 0] == 3


# ------------------------------------------------------------------------------------------------ conformance meshes
@pytest.mark.parametrize("kind", ["edge", "vertex"])
def test_conformance_meshes_under_the_reference_and_the_naive_statements(kind):
    """fp64: no pixel misses.  Plain fp32 Moeller-Trumbore misses pixels on every camera, which is what the meshes
    are for; the kernel's inside test restated in fp32 numpy misses none, and without its fp64 re-evaluation the
    vertex mesh shows holes (numpy does not contract to FMAs, so the canonical edge order cannot be shown here)."""
    naive, no_fp64 = [], []
    for c2w in vc.grid_cameras():
        tris, intr = vc.grid_mesh(kind, c2w)
        assert tris.shape == (648, 9)
        o, d, n = vc.rays_ref(c2w[None], None, intr[None], vc.GRID_FRAME)
        ref = vc.hits_ref(tris.numpy(), np.arange(648), o[0], d[0], n[0])
        assert (ref["tri_id"] >= 0).all(), f"{int((ref['tri_id'] < 0).sum())} misses in fp64"
        assert vc.footprint_ok(tris.numpy(), o[0], d[0], ref["tri_id"]).all()
        o32, d32 = vc.rays_f32(c2w[None], None, intr[None], vc.GRID_FRAME)
        naive.append(int((vc.hits_f32(tris.numpy(), np.arange(648), o32[0], d32[0])[1] < 0).sum()))
        assert vc.edge_emulation(tris.numpy(), o32[0], d32[0]).all()
        no_fp64.append(int((~vc.edge_emulation(tris.numpy(), o32[0], d32[0], fp64_fallback=False)).sum()))
    print(f"{kind} mesh: plain fp32 Moeller-Trumbore misses {naive}, edge functions without fp64 {no_fp64} of 4096")
    assert min(naive) > 0
    assert sum(no_fp64) > 0 if kind == "vertex" else True


def test_grid_geometry():
    cams = vc.grid_cameras()
    assert torch.equal(cams[0], torch.eye(4))
    for m in cams[1:]:
        r = m[:3, :3].double()
        assert torch.allclose(r @ r.T, torch.eye(3, dtype=torch.float64), atol=1e-6) and torch.det(r) > 0.99
    tv, _ = vc.grid_mesh("vertex", cams[0])
    te, _ = vc.grid_mesh("edge", cams[0])
    v = tv.reshape(-1, 3)
    assert (v[:, 2] == -vc.GRID_Z).all()
    # vertices at every 4th pixel centre: x = (px + 0.5 - 32) / 64 * 2 for px = -4, 0, .., 68
    px = v[:, 0].double() * 32.0 + 32.0 - 0.5
    assert torch.equal(px, px.round()) and set((px.long() % 4).tolist()) == {0} and px.min() == -4 and px.max() == 68
    py_e = -te.reshape(-1, 3)[:, 1].double() * 32.0 + 32.0 - 0.5
    assert set(((py_e - 0.5).long() % 4).tolist()) == {0} and torch.equal(py_e - 0.5, (py_e - 0.5).round())
    # every interior edge is shared by two triangles, in both directions somewhere (mixed winding)
    edges = {}
    for t in tv.reshape(-1, 3, 3).tolist():
        for a, b in ((0, 1), (1, 2), (2, 0)):
            edges.setdefault(frozenset((tuple(t[a]), tuple(t[b]))), []).append((tuple(t[a]), tuple(t[b])))
    shared = [e for e in edges.values() if len(e) == 2]
    assert len(shared) == 3 * 18 * 18 - 2 * 18 and any(e[0] == e[1] for e in shared) and any(e[0] != e[1] for e in shared)


# ------------------------------------------------------------------------------------------------ the GPU cases' bands
@pytest.mark.parametrize("name,frame,share,worst", [("cbox_base", (64, 64), 0.0107, 3.9e-6),
                                                    ("cbox_base", (45, 99), 0.0054, 1.2e-6),
                                                    ("tiny_swin", (64, 64), 0.0005, 8.6e-7)])
def test_band_caps_of_the_golden_cases(name, frame, share, worst):
    inp = load_case(name)[2]
    r = vc.scene_ref(inp["triangles"], inp["mask"], inp["c2w"][:, :1], inp["fov"][:, :1], None, frame)[0][0]
    band = float(r["band"].mean())
    print(f"{name} {frame}: band {band:.4%}, fp32 restatement's worst relative depth error {r['f32_worst']:.3e}")
    assert band <= vc.BAND_CAP and abs(band - share) < 2e-4
    assert abs(r["f32_worst"] - worst) < 0.05 * worst and r["tol"] == 4 * r["f32_worst"]
    # the plain fp32 statement agrees with fp64 on every pixel, inside the band too
    assert np.array_equal(r["f32_id"], r["tri_id"])
    assert (r["tri_id"] >= 0).mean() > 0.3


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_flag_and_files(tmp_path):
    import argparse

    import batch_infer  # noqa: F401  (imports infer's helpers, save_gbuffer among them)
    import infer
    from renderformer_amd.gbuffer import GBuffer
    from renderformer_amd.images import read_exr, read_png
    p = argparse.ArgumentParser()
    infer.add_common_args(p)
    assert p.parse_args(["--save_gbuffer"]).save_gbuffer is True and p.parse_args([]).save_gbuffer is False
    rng = np.random.default_rng(2)
    nv, h, w = 2, 5, 7
    alpha = np.where(rng.random((nv, h, w)) < 0.5, 255, 0).astype(np.uint8)
    depth = np.where(alpha == 255, rng.random((nv, h, w)) + 1.0, np.inf).astype(np.float32)
    normal = rng.standard_normal((nv, h, w, 3)).astype(np.float32)
    albedo = rng.random((nv, h, w, 3)).astype(np.float32)
    gb = GBuffer(alpha=torch.from_numpy(alpha), depth=torch.from_numpy(depth), normal=torch.from_numpy(normal),
                 albedo=torch.from_numpy(albedo))
    paths = infer.save_gbuffer(gb, str(tmp_path), "s")
    assert [os.path.basename(x) for x in paths[:4]] == ["s_view_0_alpha.png", "s_view_0_depth.exr",
                                                        "s_view_0_normal.exr", "s_view_0_albedo.exr"] and len(paths) == 8
    for i in range(nv):
        a = read_png(str(tmp_path / f"s_view_{i}_alpha.png"))
        np.testing.assert_array_equal(a.reshape(h, w, -1)[..., 0], alpha[i])
        d = read_exr(str(tmp_path / f"s_view_{i}_depth.exr"))
        np.testing.assert_array_equal(d.reshape(h, w), depth[i])  # one channel, +inf kept
        np.testing.assert_array_equal(read_exr(str(tmp_path / f"s_view_{i}_normal.exr")), normal[i])
        np.testing.assert_array_equal(read_exr(str(tmp_path / f"s_view_{i}_albedo.exr")), albedo[i])
