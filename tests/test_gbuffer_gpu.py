"""G-buffer kernels on the device (visibility.hip: rf_primary_hits, rf_gbuffer_shade) against the fp64 reference of
tests/visibility_checks.py.  Shapes target the kernels' seams (the triangle chunk VIS_CHUNK, the pixel tile VIS_TILE),
not the workload.  Outputs are written into kernel_checks.Guarded buffers: a store outside them fails the test.

Depth tolerance per case = 4 x the worst relative error of the fp32 numpy restatement against fp64 over the kept
pixels, floored at 2^-20 (visibility_checks.depth_tolerance).  Measured on the CPU for the golden cases:
  cbox_base 64 x 64   restatement 3.90e-6 -> tolerance 1.56e-5   (band 1.07 % of the pixels)
  cbox_base 45 x 99   restatement 1.19e-6 -> tolerance 4.75e-6   (band 0.54 %)
  tiny_swin 64 x 64   restatement 8.57e-7 -> tolerance 3.43e-6   (band 0.05 %)
The kernel's own worst relative depth error on one MI355X was 3.83e-6, 1.03e-6 and 6.77e-7 on these three, its worst
barycentric error 1.8e-6, 1.5e-6 and 1.9e-6 (bound 1e-4), and no id outside the band differed.
Each case prints its own figures before asserting (pytest -s).
"""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import kernel_checks as kc  # noqa: E402
import visibility_checks as vc  # noqa: E402
from golden_util import load_case  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CENTRE = torch.tensor([0.3, -0.2, 0.5])  # kernel_checks.scene_case puts its vertices around this point


# ------------------------------------------------------------------------------------------------ helpers
def look_at(pos, target=CENTRE):
    """c2w fp32 [4, 4] of a camera at `pos` looking at `target` (the camera looks along its -z axis)."""
    z = (pos - target).double()
    z = z / z.norm()
    x = torch.linalg.cross(torch.tensor([0.1, 1.0, 0.05], dtype=torch.float64), z)
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    m = torch.eye(4, dtype=torch.float64)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, pos.double()
    return m.float()


def synthetic_scene(counts, n_views, seed, n_per_scene=None):
    """(triangles fp32 [B, N, 9], mask bool [B, N], c2w [B, V, 4, 4], fov [B, V]) from kernel_checks.scene_case: scene
    b's counts[b] valid rows sit at shuffled places among the N rows, the other rows are NaN; the cameras of
    scene_case (random translations) are turned to look at the triangles."""
    B = len(counts)
    N = n_per_scene or max(max(counts) + max(counts) // 4 + 7, 8)
    tris = torch.full((B, N, 9), float("nan"))
    mask = torch.zeros(B, N, dtype=torch.bool)
    c2w = torch.zeros(B, n_views, 4, 4)
    for b, n in enumerate(counts):
        t, valid, _, cams = kc.scene_case((n,), n_views, seed + 17 * b)
        g = torch.Generator().manual_seed(7000 + seed + b)
        rows = torch.randperm(N, generator=g)[:n].sort().values
        tris[b, rows] = t[valid.long()]
        mask[b, rows] = True
        for v in range(n_views):
            c2w[b, v] = look_at(cams[v, :3, 3])
    fov = kc.camera_case(B * n_views, seed)[1].reshape(B, n_views)
    return tris, mask, c2w, fov


class Hits:
    """ops.primary_hits into Guarded outputs; .depth / .tri_id / .bary / .alpha as host numpy arrays."""

    def __init__(self, tris, mask, c2w, fov, intr, frame, bary=True, alpha=True):
        from renderformer_amd import gbuffer as gb, ops
        B, V = c2w.shape[:2]
        h, w = frame
        self.tris_dev = tris.reshape(B, -1, 9).to(DEV).contiguous()
        tables = gb.scene_tables(mask.numpy(), DEV)
        specs = {"depth": (w, torch.float32), "tri_id": (w, torch.int32)}
        if bary:
            specs["bary"] = (2 * w, torch.float32)
        if alpha:
            specs["alpha"] = (w, torch.uint8)
        self.guards = {k: kc.Guarded(B * V * h, c, dt, DEV, ld=c) for k, (c, dt) in specs.items()}
        out = {k: g.view.view(B, V, h, w, 2) if k == "bary" else g.view.view(B, V, h, w)
               for k, g in self.guards.items()}
        keep = self.tris_dev.clone()
        dev = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
        self.dev = ops.primary_hits(self.tris_dev, tables[0], tables[1], tables[2], dev(c2w), dev(fov), dev(intr), frame,
                                    bary=bary, alpha=alpha, out=out)
        torch.cuda.synchronize()
        for k, g in self.guards.items():
            g.assert_untouched(what=f"primary_hits {k}")
        assert torch.equal(self.tris_dev.view(torch.int32), keep.view(torch.int32)), "primary_hits wrote to tris"
        for k, t in self.dev.items():
            setattr(self, k, t.cpu().numpy())


def check_views(ref, hits, what, cap=vc.BAND_CAP):
    """Every view against its reference.  cap=None: no cap on the band share (a frame of a few pixels has no
    meaningful one; the caller bounds the kept pixels over its frames instead)."""
    for b, views in enumerate(ref):
        for v, r in enumerate(views):
            vc.compare(r, hits.depth[b, v], hits.tri_id[b, v], hits.bary[b, v], f"{what} scene {b} view {v}", cap=cap)
            a = hits.alpha[b, v]
            assert np.array_equal(a, np.where(hits.tri_id[b, v] >= 0, 255, 0).astype(np.uint8)), f"{what}: alpha"


@pytest.fixture(scope="module")
def cases():
    """The golden scenes' inputs, loaded once."""
    return {name: load_case(name) for name in ("tiny_swin", "cbox_base")}


# ------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("name,frame,use_intr", [("cbox_base", (64, 64), False), ("cbox_base", (45, 99), False),
                                                 ("tiny_swin", (64, 64), False), ("tiny_swin", (64, 64), True)])
def test_golden_scene_matches_fp64(cases, name, frame, use_intr):
    inp = cases[name][2]
    tris, mask, c2w = inp["triangles"], inp["mask"], inp["c2w"][:, :1].contiguous()
    B = c2w.shape[0]
    fov = inp["fov"][:, :1].reshape(B, 1).contiguous()
    intr = None
    if use_intr:  # off-centre, fx != fy
        intr, fov = torch.tensor([70.0, 82.0, 27.25, 36.5]).repeat(B, 1, 1), None
    ref = vc.scene_ref(tris, mask, c2w, fov, intr, frame)
    hits = Hits(tris, mask, c2w, fov, intr, frame)
    check_views(ref, hits, f"{name} {frame[0]} x {frame[1]}{' intrinsics' if use_intr else ''}")


def _frames():
    from renderformer_amd import ops
    return [(1, 1), (7, 5), (16, 16), (17, 33), (ops.VIS_TILE + 1, ops.VIS_TILE + 1)]


@pytest.mark.parametrize("which", ["1", "C-1", "C", "C+1", "2C+3"])
def test_chunk_and_tile_seams_match_fp64(which):
    from renderformer_amd import ops
    C = ops.VIS_CHUNK
    n = {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "2C+3": 2 * C + 3}[which]
    tris, mask, c2w, fov = synthetic_scene((n,), 1, seed=n % 11)
    kept = total = 0
    for frame in _frames():
        ref = vc.scene_ref(tris, mask, c2w, fov, None, frame)
        hits = Hits(tris, mask, c2w, fov, None, frame)
        check_views(ref, hits, f"{n} triangles, {frame[0]} x {frame[1]}", cap=None)
        kept += int((~ref[0][0]["band"]).sum())
        total += frame[0] * frame[1]
    assert kept > total // 2, f"{n} triangles: only {kept} of {total} pixels are outside the band"


# ------------------------------------------------------------------------------------------------ 2. index mapping
def test_ids_index_the_input_axis_per_scene():
    counts = (70, 300, 0)
    tris, mask, c2w, fov = synthetic_scene(counts, 2, seed=3, n_per_scene=400)
    assert not mask[2].any() and torch.isnan(tris[~mask]).all() and not mask[0, :5].all()
    frame = (17, 33)
    ref = vc.scene_ref(tris, mask, c2w, fov, None, frame)
    hits = Hits(tris, mask, c2w, fov, None, frame)
    check_views(ref, hits, "index mapping", cap=None)
    m = mask.numpy()
    for b in range(3):
        ids = hits.tri_id[b]
        assert ((ids == -1) | m[b][np.maximum(ids, 0)]).all(), f"scene {b} reports a masked-out or foreign row"
    assert (hits.tri_id[0] >= 0).any() and (hits.tri_id[1] >= 0).any()
    # the scene without valid triangles: -1 / +inf / 0 everywhere
    assert (hits.tri_id[2] == -1).all() and np.isposinf(hits.depth[2]).all()
    assert (hits.bary[2] == 0).all() and (hits.alpha[2] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. exact ties
@pytest.mark.parametrize("n", [37, "C"])
def test_duplicates_report_the_lower_index_and_runs_repeat(n):
    from renderformer_amd import ops
    n = ops.VIS_CHUNK if n == "C" else n  # duplicates at i and i + n: inside one chunk, and a whole chunk apart
    tris, mask, c2w, fov = synthetic_scene((n,), 1, seed=5)
    t = tris[0][mask[0]]
    both = torch.cat([t, t])[None]
    m2 = torch.ones(1, 2 * n, dtype=torch.bool)
    frame = (17, 33)
    a = Hits(both, m2, c2w, fov, None, frame)
    b = Hits(both, m2, c2w, fov, None, frame)
    single = Hits(t[None], torch.ones(1, n, dtype=torch.bool), c2w, fov, None, frame)
    assert (a.tri_id >= 0).any()
    assert (a.tri_id < n).all(), f"{int((a.tri_id >= n).sum())} pixel(s) report the duplicate at the higher index"
    for k in ("depth", "tri_id", "bary", "alpha"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), f"two runs differ in {k}"
        assert np.array_equal(getattr(a, k), getattr(single, k), equal_nan=True), f"the duplicates changed {k}"


# ------------------------------------------------------------------------------------------------ 4. watertightness
@pytest.mark.parametrize("kind", ["edge", "vertex"])
@pytest.mark.parametrize("cam", [0, 1, 2, 3])
def test_conformance_mesh_has_no_pinholes(kind, cam):
    c2w = vc.grid_cameras()[cam]
    tris, intr = vc.grid_mesh(kind, c2w)
    mask = torch.ones(1, tris.shape[0], dtype=torch.bool)
    hits = Hits(tris[None], mask, c2w[None, None], None, intr[None, None], vc.GRID_FRAME)
    misses = int((hits.tri_id[0, 0] < 0).sum())
    o, d, _ = vc.rays_ref(c2w[None], None, intr[None], vc.GRID_FRAME)
    inside = vc.footprint_ok(tris.numpy(), o[0], d[0], hits.tri_id[0, 0])
    print(f"{kind} mesh, camera {cam}: {misses} misses, {int((~inside).sum())} ids outside their widened footprint")
    assert misses == 0, f"{kind} mesh, camera {cam}: {misses} of 4096 pixels see through the grid"
    assert inside.all()
    assert (hits.alpha == 255).all() and np.isfinite(hits.depth).all()


# ------------------------------------------------------------------------------------------------ pipeline level
@pytest.fixture(scope="module")
def tiny(cases):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    cfg, sd, inp, res, z = cases["tiny_swin"]
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd)).to(DEV)
    d = {k: v.to(DEV) for k, v in inp.items()}
    return pipe, d, inp


def _same_bits(a, b, what):
    for name, x, y in zip(a._fields, a, b):
        assert (x is None) == (y is None), f"{what}: {name}"
        if x is not None:
            same = torch.equal(x, y) if not x.is_floating_point() else torch.equal(x.view(torch.int32), y.view(torch.int32))
            assert same, f"{what}: {name} differs"


# 5. the same rays as the frame
@pytest.mark.parametrize("mode", ["overscan", "intrinsics"])
def test_gbuffer_is_the_window_of_the_padded_frame(tiny, mode):
    pipe, d, _ = tiny
    args = (d["triangles"], d["texture"].clone(), d["mask"], d["vn"], d["c2w"])
    B, V = d["c2w"].shape[:2]
    if mode == "overscan":
        # the fov convention written as intrinsics (fx = fy = H / 2 / tan(fov / 2), cx = W / 2, cy = H / 2): the
        # padded call can only be handed a focal length as a number, and no host expression reproduces the bits of
        # the kernel's own tanf, so both calls take the same fp32 value
        H, W, Hp, Wp = 45, 99, 64, 128
        fov = d["fov"].reshape(B, V).float()
        f = (H / 2.0) / torch.tan(0.5 * torch.deg2rad(fov))
        k = torch.stack([f, f, torch.full_like(f, W / 2.0), torch.full_like(f, H / 2.0)], dim=-1).contiguous()
        got = pipe.gbuffer(*args, None, (H, W), intrinsics=k, overscan=True)
        # (the same frame by its fov: the same pixels up to the last bits of the focal length)
        by_fov = pipe.gbuffer(*args, fov, (H, W), overscan=True)
        assert (by_fov.tri_id == got.tri_id).float().mean() > 0.995
    else:
        H, W, Hp, Wp = 40, 72, 64, 128
        k = torch.tensor([61.0, 55.5, 30.25, 17.75], device=DEV).repeat(B, V, 1)
        got = pipe.gbuffer(*args, None, (H, W), intrinsics=k, overscan=True)
    y0, x0 = (Hp - H) // 2, (Wp - W) // 2
    kp = k + torch.tensor([0.0, 0.0, float(x0), float(y0)], device=DEV)
    pad = pipe.gbuffer(*args, None, (Hp, Wp), intrinsics=kp.contiguous())
    win = type(pad)(*(t[:, :, y0:y0 + H, x0:x0 + W].contiguous() for t in pad))
    assert (got.tri_id >= 0).any() and (got.tri_id < 0).any()
    _same_bits(got, win, mode)


# 6. shading
def test_shading_normal_albedo_alpha(tiny):
    from renderformer_amd import ops
    from renderformer_amd.gbuffer import scene_tables
    pipe, d, inp = tiny
    B, V = d["c2w"].shape[:2]
    fov = d["fov"].reshape(B, V)
    tex5 = d["texture"].clone()                     # [B, N, C, 32, 32]
    tex3 = tex5[:, :, :, 0, 0].contiguous()         # [B, N, C]
    keep = [t.clone() for t in (d["triangles"], tex5, d["mask"], d["vn"], d["c2w"], fov)]
    g = pipe.gbuffer(d["triangles"], tex5, d["mask"], d["vn"], d["c2w"], fov, 64)
    hits = ops.primary_hits(d["triangles"].reshape(B, -1, 9).contiguous(), *scene_tables(inp["mask"].numpy(), DEV),
                            d["c2w"].contiguous(), fov.contiguous(), None, 64)
    assert torch.equal(hits["tri_id"], g.tri_id)
    ids, bary = hits["tri_id"], hits["bary"]
    # through Guarded outputs, both texture layouts
    h = w = 64
    for tex in (tex5, tex3):
        gs = {"alpha": kc.Guarded(B * V * h, w, torch.uint8, DEV, ld=w),
              "normal": kc.Guarded(B * V * h, 3 * w, torch.float32, DEV, ld=3 * w),
              "albedo": kc.Guarded(B * V * h, 3 * w, torch.float32, DEV, ld=3 * w)}
        out = {"alpha": gs["alpha"].view.view(B, V, h, w), "normal": gs["normal"].view.view(B, V, h, w, 3),
               "albedo": gs["albedo"].view.view(B, V, h, w, 3)}
        sh = ops.gbuffer_shade(ids, bary, d["vn"].reshape(B, -1, 9).contiguous(), tex, alpha=True, normal=True,
                               albedo=True, out=out)
        torch.cuda.synchronize()
        for k_, gd in gs.items():
            gd.assert_untouched(what=f"gbuffer_shade {k_}")
        hit = ids >= 0
        assert hit.any() and (~hit).any()
        assert torch.equal(sh["alpha"], torch.where(hit, 255, 0).to(torch.uint8))
        # albedo: exactly texel (0, 0) of the diffuse channels of the hit triangle; zeros on a miss
        bi = torch.arange(B, device=DEV)[:, None, None, None].expand_as(ids)
        want = tex5[bi, ids.clamp_min(0).long()][..., :3, 0, 0] * hit[..., None]
        assert torch.equal(sh["albedo"], want)
        assert torch.equal(sh["albedo"], g.albedo) and torch.equal(sh["normal"], g.normal)
        # normal: fp64 of the same fp32 inputs; three products and a normalisation of unit-scale values -> 1e-5
        vn = d["vn"].reshape(B, -1, 3, 3).double()[bi, ids.clamp_min(0).long()]
        u, v_ = bary[..., 0].double(), bary[..., 1].double()
        nr = (1 - u - v_)[..., None] * vn[..., 0, :] + u[..., None] * vn[..., 1, :] + v_[..., None] * vn[..., 2, :]
        nr = nr / nr.norm(dim=-1, keepdim=True).clamp_min(1e-12) * hit[..., None]
        err = float((sh["normal"].double() - nr).abs().max())
        print(f"normal: worst absolute error against fp64 {err:.3e}")
        assert err <= 1e-5
    for t, k_ in zip((d["triangles"], tex5, d["mask"], d["vn"], d["c2w"], fov), keep):
        assert torch.equal(t, k_), "gbuffer modified an input"
    # subsets: only what was asked, the same bits
    sub = pipe.gbuffer(d["triangles"], tex5, d["mask"], d["vn"], d["c2w"], fov, 64, outputs=("alpha", "depth", "tri_id"))
    assert sub.normal is None and sub.albedo is None
    assert torch.equal(sub.alpha, g.alpha) and torch.equal(sub.depth, g.depth) and torch.equal(sub.tri_id, g.tri_id)
    one = pipe.gbuffer(d["triangles"], tex5, d["mask"], d["vn"], d["c2w"], fov, 64, outputs=["albedo"])
    assert [n for n, t in zip(one._fields, one) if t is not None] == ["albedo"] and torch.equal(one.albedo, g.albedo)
    # the EncodedScene's texture is log-encoded in its emission channels: the same albedo
    enc_tex = tex5.clone()
    scene = pipe.encode(d["triangles"], enc_tex, d["mask"], d["vn"])
    assert not torch.equal(enc_tex, tex5), "encode did not log-encode the texture: the case shows nothing"
    ge = pipe.gbuffer_encoded(scene, d["c2w"], fov, 64)
    _same_bits(ge, g, "gbuffer_encoded")


# 7. end to end
def test_gbuffer_encoded_matches_gbuffer_on_cbox(cases):
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    cfg, sd, inp, res, z = cases["cbox_base"]
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd)).to(DEV)
    d = {k: v.to(DEV) for k, v in inp.items()}
    c2w, fov = d["c2w"][:, :1].contiguous(), d["fov"][:, :1].contiguous()
    g = pipe.gbuffer(d["triangles"], d["texture"].clone(), d["mask"], d["vn"], c2w, fov, 64)
    scene = pipe.encode(d["triangles"], d["texture"], d["mask"], d["vn"])
    _same_bits(pipe.gbuffer_encoded(scene, c2w, fov, 64), g, "cbox_base")
    assert (g.tri_id >= 0).float().mean() > 0.5


def test_infer_cli_saves_the_gbuffer(tmp_path):
    import infer
    from test_cli import _snapshot_and_scene
    from renderformer_amd.images import read_exr, read_png
    snap, h5, res, z = _snapshot_and_scene(tmp_path)
    out = tmp_path / "out"
    assert infer.main(["--h5_file", str(h5), "--model_id", str(snap), "--resolution", str(res), "--output_dir",
                       str(out), "--save_gbuffer"]) == 0
    nv = z["hdr"].shape[1]
    for i in range(nv):
        stem = str(out / f"tiny_view_{i}")
        assert os.path.exists(stem + ".exr") and os.path.exists(stem + ".png")
        alpha = read_png(stem + "_alpha.png")
        depth = read_exr(stem + "_depth.exr")
        assert alpha.shape[:2] == (res, res) and depth.shape[:2] == (res, res)
        assert read_exr(stem + "_normal.exr").shape == (res, res, 3)
        assert read_exr(stem + "_albedo.exr").shape == (res, res, 3)
        a = alpha.reshape(res, res, -1)[..., 0]
        dd = depth.reshape(res, res)
        assert set(np.unique(a)) <= {0, 255} and (a == 255).any() and (a == 0).any()
        assert np.isposinf(dd[a == 0]).all() and np.isfinite(dd[a == 255]).all() and (dd[a == 255] > 0).all()
