"""pipe.pose / rf_pose_scene on the device against rig.pose_numpy (float64).

Exact cases: integer coordinates, signed permutations times power-of-two scales, integer translations and
axis-aligned normals make every operation of the kernel exact in fp32, so the outputs are compared bit for bit.
General case, per element (the bounds of tests/test_rig.py, on the same float32 inputs):
  triangles  4 * 2^-24 * (|A| |p| + |t|) + 0.5e-8  (the kernel's three fmas round three partial sums of at most
             |A| |p| + |t|, 2^-24 relative each);
  normals    8 * 2^-24  (the kernel rounds a unit vector's component to fp32 once: 2^-24 / 2)."""
import functools

import numpy as np
import pytest
import torch

from golden_util import load_case, rel_l2
from kernel_checks import Guarded
from oracle import rf_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
HDR_TOL = 1e-3


def _pipe_without_weights():
    """pose needs no model: a pipeline object around nothing."""
    from renderformer_amd.pipeline import RenderFormerRenderingPipeline
    return RenderFormerRenderingPipeline.__new__(RenderFormerRenderingPipeline)


def _exact_rig(B=2, N=67, K=3, M=5, seed=0):
    from renderformer_amd.rig import SceneRig
    rng = np.random.default_rng(seed)
    tris = rng.integers(-8, 9, (B, N, 3, 3)).astype(np.float32)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    vn = axes[rng.integers(0, 6, (B, N, 3))]
    oid = rng.integers(0, K, (B, N)).astype(np.int32)
    mid = rng.integers(0, M, (B, N)).astype(np.int32)
    pad = np.zeros((B, N), bool)
    pad[:, [5, N // 2, N - 1]] = True  # a few padding rows, the last row among them
    pad[0, 0] = True
    oid[pad] = mid[pad] = -1
    perms = [np.eye(3)[[1, 2, 0]], np.eye(3)[[0, 2, 1]], np.eye(3)[[2, 1, 0]], np.eye(3)]
    xf = np.zeros((B, K, 3, 4), np.float32)
    for b in range(B):
        for k in range(K):
            signs = rng.choice([-1.0, 1.0], 3)
            a = np.diag(signs * 2.0 ** rng.integers(-2, 3, 3)) @ perms[(b + k) % 4]
            xf[b, k, :, :3] = a
            xf[b, k, :, 3] = rng.integers(-5, 6, 3)
    xf[0, 1, :, :3] = np.diag([-2.0, 1.0, 0.5]) @ perms[0]  # det < 0 for certain ...
    xf[B - 1, 0, :, :3] = np.diag([4.0, 0.25, 1.0]) @ perms[3]  # ... and det > 0
    assert np.linalg.det(xf[0, 1, :, :3].astype(np.float64)) < 0 < np.linalg.det(xf[B - 1, 0, :, :3].astype(np.float64))
    mat = rng.integers(0, 256, (B, M, 13)).astype(np.float32) / 256.0
    return SceneRig(tris, vn, oid, mid, [f"o{k}" for k in range(K)], xf, mat)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def test_exact_integers():
    from renderformer_amd.rig import PosedScene, pose_numpy
    rig = _exact_rig()
    ref_t, ref_n, ref_r = pose_numpy(rig, rig.transforms0, rig.materials0)
    for ref in (ref_t, ref_n, ref_r):  # the premise: every reference value is a float32
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    dev = rig.to("cuda")
    pipe = _pipe_without_weights()
    posed = pipe.pose(dev, dev.transforms0, dev.materials0)
    assert isinstance(posed, PosedScene) and posed.mask is dev.mask
    assert tuple(posed.texture.shape) == (2, 67, 13) and tuple(posed.triangles.shape) == (2, 67, 3, 3)
    assert torch.equal(posed.triangles.cpu(), _t(ref_t))
    assert torch.equal(posed.vn.cpu(), _t(ref_n))
    assert torch.equal(posed.texture.cpu(), _t(ref_r))
    pad = ~rig.mask
    assert int(pad.sum()) == 7
    bits = lambda x: x.cpu().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(posed.triangles)[pad], bits(rig.triangles)[pad])
    assert torch.equal(bits(posed.vn)[pad], bits(rig.vn)[pad])
    assert torch.equal(bits(posed.texture)[pad], torch.zeros(7, 13, dtype=torch.int32))
    # materials=None is materials0; a [B, K, 4, 4] stack gives the same bits and its fourth row is never read
    xf44 = torch.full((2, 3, 4, 4), float("nan"), device="cuda")
    xf44[:, :, :3] = dev.transforms0
    for other in (pipe.pose(dev, dev.transforms0), pipe.pose(dev, xf44, dev.materials0)):
        for f in ("triangles", "vn", "texture"):
            assert torch.equal(bits(getattr(other, f)), bits(getattr(posed, f))), f


def _general_rig(N=257, seed=1):
    from renderformer_amd.rig import SceneRig, trs
    rng = np.random.default_rng(seed)
    B, K, M = 1, 6, 4
    tris = rng.uniform(-1, 1, (B, N, 3, 3)).astype(np.float32)
    vn = rng.standard_normal((B, N, 3, 3))
    vn = (vn / np.linalg.norm(vn, axis=-1, keepdims=True)).astype(np.float32)
    vn[0, 3] = 0.0          # zero rest normals
    vn[0, 100, 1] = 0.0
    oid = rng.integers(0, K, (B, N)).astype(np.int32)
    mid = rng.integers(0, M, (B, N)).astype(np.int32)
    oid[0, [7, N - 1]] = mid[0, [7, N - 1]] = -1
    oid[0, 3], oid[0, 100] = 1, 0  # the rows with zero normals belong to regular matrices
    xf = np.zeros((B, K, 3, 4), np.float32)
    scales = [(1.3, 1.3, 1.3), (0.5, 2.0, 1.0), (2.0, 0.5, 0.7), (-1.0, 1.5, 0.8), (1.0, 1.0, 1.0), (0.9, 1.9, 0.6)]
    for k, s in enumerate(scales):  # uniform, non-uniform, a mirror; rotations about all three axes
        xf[0, k] = trs(rng.uniform(-2, 2, 3), rng.uniform(-180, 180, 3), s).numpy()
    xf[0, 4, :, :3] = np.outer([1.0, 2.0, -0.5], [0.3, -0.7, 1.1]).astype(np.float32)  # singular (rank 1)
    mat = rng.uniform(0, 1, (B, M, 13)).astype(np.float32)
    return SceneRig(tris, vn, oid, mid, [f"o{k}" for k in range(K)], xf, mat)


def test_general_fp32():
    from renderformer_amd.rig import pose_numpy
    rig = _general_rig()
    ref_t, ref_n, ref_r = pose_numpy(rig, rig.transforms0, rig.materials0)
    dev = rig.to("cuda")
    posed = _pipe_without_weights().pose(dev, dev.transforms0, dev.materials0)
    out_t, out_n = posed.triangles.cpu().double().numpy(), posed.vn.cpu().double().numpy()
    assert np.isfinite(out_t).all() and np.isfinite(out_n).all()  # the singular matrix and the zero normals too
    oid = rig.object_id[0].numpy()
    a = rig.transforms0[0].double().numpy()[np.maximum(oid, 0)]
    mag = np.einsum("nij,nvj->nvi", np.abs(a[:, :, :3]), np.abs(rig.triangles[0].double().numpy())) \
        + np.abs(a[:, None, :, 3])
    bound = 4 * U * mag + 0.5e-8
    err_t, err_n = np.abs(out_t - ref_t)[0], np.abs(out_n - ref_n)[0]
    regular = oid != 4  # the rank-1 matrix: cof(A) is zero up to cancellation, the direction of g is not defined
    print(f"general: worst triangle error {(err_t / bound).max():.3f} of its bound, worst normal error "
          f"{err_n[regular].max():.3g} (bound {8 * U:.3g})")
    assert np.all(err_t <= bound)
    assert np.all(err_n[regular] <= 8 * U)
    ln = np.linalg.norm(out_n[0], axis=-1)
    assert np.all((np.abs(ln - 1) < 4 * U) | (ln == 0))
    assert np.all(out_n[0, 3] == 0) and np.all(out_n[0, 100, 1] == 0) and np.all(ln[100, [0, 2]] > 0)
    assert torch.equal(posed.texture.cpu(), _t(ref_r))
    mirror = oid == 3  # det < 0: still A^-T n up to a POSITIVE factor
    assert np.linalg.det(rig.transforms0[0, 3, :, :3].double().numpy()) < 0 and mirror.any()


@pytest.mark.parametrize("B,N", [(1, 1), (2, 67), (1, 600)])
def test_guard_bands(B, N):
    """Outputs inside sentinel margins: nothing outside the B * N rows is written (one row; a size that is no multiple
    of a wave or of the 256-row workgroup; three workgroups with a ragged last one)."""
    from renderformer_amd import ops
    from renderformer_amd.rig import pose_numpy
    rig = _exact_rig(B, max(N, 4), seed=N) if N >= 4 else None
    if rig is None:  # N = 1: one valid row
        from renderformer_amd.rig import SceneRig
        rig = SceneRig(np.full((1, 1, 3, 3), 2.0, np.float32), np.tile(np.float32([0, 0, 1]), (1, 1, 3, 1)),
                       np.zeros((1, 1), np.int32), np.zeros((1, 1), np.int32), ["o"],
                       np.float32([[[[0, 2, 0, 1], [1, 0, 0, 2], [0, 0, -1, 3]]]]), np.ones((1, 1, 13), np.float32))
    B, N = rig.object_id.shape
    C = rig.materials0.shape[2]
    dev = rig.to("cuda")
    outs = [Guarded(B * N, 9, torch.float32, "cuda", g=3, ld=9), Guarded(B * N, 9, torch.float32, "cuda", g=3, ld=9),
            Guarded(B * N, C, torch.float32, "cuda", g=3, ld=C)]
    views = (outs[0].view.view(B, N, 3, 3), outs[1].view.view(B, N, 3, 3), outs[2].view.view(B, N, C))
    ops.pose_scene(dev.triangles, dev.vn, dev.object_id, dev.material_id, dev.transforms0, dev.materials0, out=views)
    torch.cuda.synchronize()
    for g_, what in zip(outs, ("triangles", "vn", "texture")):
        g_.assert_untouched(what=f"pose_scene {what} [{B}, {N}]")
    ref = pose_numpy(rig, rig.transforms0, rig.materials0)
    for v, r in zip(views, ref):
        assert torch.equal(v.cpu(), _t(r))


def test_out_reuses_storage():
    rig = _exact_rig(seed=4).to("cuda")
    pipe = _pipe_without_weights()
    first = pipe.pose(rig, rig.transforms0)
    keep = [t.clone() for t in (first.triangles, first.vn, first.texture)]
    ptrs = [t.data_ptr() for t in (first.triangles, first.vn, first.texture)]
    xf2 = rig.transforms0.clone()
    xf2[:, :, :, 3] += 1.0
    moved = pipe.pose(rig, xf2, out=first)
    assert [t.data_ptr() for t in (moved.triangles, moved.vn, moved.texture)] == ptrs
    assert not torch.equal(moved.triangles, keep[0])
    back = pipe.pose(rig, rig.transforms0, rig.materials0, out=moved)
    assert [t.data_ptr() for t in (back.triangles, back.vn, back.texture)] == ptrs
    for t, k in zip((back.triangles, back.vn, back.texture), keep):
        assert torch.equal(t, k)


def test_pose_refuses_bad_arguments():
    rig = _exact_rig(seed=5)
    pipe = _pipe_without_weights()
    with pytest.raises(ValueError, match="HIP device"):
        pipe.pose(rig, rig.transforms0)
    dev = rig.to("cuda")
    xf = dev.transforms0
    for bad in (xf.cpu(), xf.double(), xf[:, :2].contiguous(), xf.transpose(2, 3), xf[0], xf.reshape(2, 3, 12)):
        with pytest.raises(ValueError, match="transforms"):
            pipe.pose(dev, bad)
    for bad in (dev.materials0.cpu(), dev.materials0[:, :4].contiguous(), dev.materials0.half()):
        with pytest.raises(ValueError, match="materials"):
            pipe.pose(dev, xf, bad)
    with pytest.raises(ValueError, match="PosedScene"):
        pipe.pose(dev, xf, out=(xf, xf, xf))
    with pytest.raises(ValueError, match="SceneRig"):
        pipe.pose(None, xf)


@functools.lru_cache(maxsize=None)
def _case(name):
    return load_case(name)


def test_posed_render_matches_the_oracle():
    """End to end: tiny_swin's triangles split into two objects, one given a rigid motion plus uniform scale and a new
    roughness and emission; pipe.render(*pipe.pose(...)) against the CPU fp32 oracle on the pose_numpy scene with the
    expanded texture of its rows: the project's 1e-3 bar against the reference, not against the code under test."""
    from renderformer_amd import RenderFormer, RenderFormerRenderingPipeline
    from renderformer_amd.rig import SceneRig, pose_numpy, trs
    from renderformer_amd.scenes import expand_texture
    cfg, sd, inp, res, z = _case("tiny_swin")
    B, N = inp["mask"].shape
    mask = inp["mask"].numpy()
    oid = np.where(mask, (np.arange(N)[None] % 2), -1).astype(np.int32)
    ch = inp["texture"][:, :, :, 0, 0].numpy()
    # one material row per triangle and object-1 triangles share an extra row whose values are changed below
    mats = np.concatenate([ch, ch[:, :1]], axis=1).astype(np.float32)
    mid = np.where(mask, np.arange(N)[None], -1).astype(np.int32)
    mid[(oid == 1) & (np.arange(N)[None] % 4 == 1)] = N
    xf0 = np.tile(trs().numpy(), (B, 2, 1, 1))
    rig = SceneRig(inp["triangles"].numpy(), inp["vn"].numpy(), oid, mid, ["rest", "moving"], xf0, mats)
    xf = rig.transforms0.clone()
    xf[:, 1] = trs((0.05, -0.03, 0.04), (10.0, -20.0, 35.0), 0.9)
    mat = rig.materials0.clone()
    mat[:, N, 6] = 0.75                                      # roughness
    mat[:, N, 10:13] = torch.tensor([30.0, 20.0, 10.0])      # emission
    mat = mat.half().float()                                 # (the expanded texture format holds fp16 values)
    ref_t, ref_n, ref_r = pose_numpy(rig, xf, mat)
    ref = rf_ref.render(sd, cfg, _t(ref_t), torch.from_numpy(expand_texture(ref_r.astype(np.float32))), inp["mask"],
                        _t(ref_n), inp["c2w"], inp["fov"], resolution=res)
    pipe = RenderFormerRenderingPipeline(RenderFormer(cfg, sd)).to("cuda")
    dev = rig.to("cuda")
    posed = pipe.pose(dev, xf.cuda(), mat.cuda())
    out = pipe.render(*posed, inp["c2w"].cuda(), inp["fov"].cuda(), resolution=res)
    err = rel_l2(out.cpu(), ref)
    rest = rel_l2(torch.from_numpy(z["hdr"]), ref)
    print(f"posed tiny_swin: rel L2 {err:.3e} vs the oracle on the pose_numpy scene (the rest-pose frame is {rest:.3e} "
          f"away from it)")
    assert err < HDR_TOL
    assert rest > HDR_TOL  # the pose did change the frame
    # and through encode / render_encoded, from a fresh pose (render log-encoded the first one's rows)
    scene = pipe.encode(*pipe.pose(dev, xf.cuda(), mat.cuda(), out=posed))
    assert torch.equal(pipe.render_encoded(scene, inp["c2w"].cuda(), inp["fov"].cuda(), res), out)
