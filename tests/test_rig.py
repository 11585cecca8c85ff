"""Rest-pose rigs (renderformer_amd.rig, scene_convert.scene_rig) against the scene converter; pose_numpy's
semantics; SceneRig's validation; the host-side refusals of rf_pose_scene / rf_texture_rows.  No GPU.

Bounds (derived, not measured).  The rig's rest arrays, matrices and translations are rounded to float32 (as the
device sees them) before pose_numpy applies them in float64, and the converter rounds its result to 8 decimals:
  triangles  4 * 2^-24 * (|A| |p| + |t|) + 0.5e-8 per element: the fp32 roundings of the three inputs (p, A, t;
             2^-24 relative each, A's acting on |A| |p|) with one to spare, plus half a unit of the 8th decimal;
  normals    8 * 2^-24.
Material rows are compared exactly, at the precision the device holds them: float32 (the converter's float64
channels cast once), and their expand_texture against the converter's texture after the cast its HDF5 writer applies
(float16), which is expand_texture's own."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from renderformer_amd import scene_convert as sc
from renderformer_amd.rig import SceneRig, pose_numpy, trs
from renderformer_amd.scenes import expand_texture

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(REPO, "examples")
U = 2.0 ** -24


def _tri_bound(rig, b=0):
    a = rig.transforms0[b].double().numpy()[rig.object_id[b].numpy()]          # [N, 3, 4]
    p = np.abs(rig.triangles[b].double().numpy())
    return 4 * U * (np.einsum("nij,nvj->nvi", np.abs(a[:, :, :3]), p) + np.abs(a[:, None, :, 3])) + 0.5e-8


@pytest.mark.parametrize("name", ["cbox", "cbox-teapot", "crystals"])
def test_rig_reproduces_the_converter(name):
    path = os.path.join(EX, name + ".json")
    cfg = sc.load_scene_config(path)
    ref = sc.scene_arrays(cfg, EX)
    rig = SceneRig.from_config(path)  # float32 rest arrays, matrices and materials
    assert rig.names == list(cfg.objects) and rig.materials0.shape[1] >= len(rig.names)
    tris, vn, rows = pose_numpy(rig, rig.transforms0, rig.materials0)
    assert tris.shape[1:] == ref["triangles"].shape and bool(rig.mask.all())  # same N (and order: elementwise below)
    err_t = np.abs(tris[0] - ref["triangles"])
    err_n = np.abs(vn[0] - ref["vn"])
    print(f"{name}: N {tris.shape[1]}, worst triangle error {err_t.max():.3g} ({(err_t / _tri_bound(rig)).max():.3f} "
          f"of its bound), worst normal error {err_n.max():.3g} (bound {8 * U:.3g})")
    assert np.all(err_t <= _tri_bound(rig))
    assert np.all(err_n <= 8 * U)
    # material rows: the converter's 13 channels, exactly (texel (0, 0) of every patch is inside the mask)
    ch = ref["texture"][:, :, 0, 0]
    got = rig.materials0[0].numpy()[rig.material_id[0].numpy()]
    assert got.dtype == np.float32 and np.array_equal(got, ch.astype(np.float32))
    assert np.array_equal(rows[0], got.astype(np.float64))
    assert np.array_equal(expand_texture(got), ref["texture"].astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("kind", ["per-triangle", "per-shading-group"])
def test_random_diffuse_rows_equal_object_arrays(tmp_path, kind):
    cfg = json.load(open(os.path.join(EX, "cbox.json")))
    name = "tall_box"
    obj = cfg["objects"][name]
    obj["mesh_path"] = os.path.join(EX, obj["mesh_path"])
    obj["material"].update(rand_tri_diffuse_seed=7, random_diffuse_type=kind, random_diffuse_max=0.8,
                           smooth_shading=True)
    cfg["objects"] = {name: obj, "light_0": dict(cfg["objects"]["light_0"],
                                                 mesh_path=os.path.join(EX, cfg["objects"]["light_0"]["mesh_path"]))}
    path = tmp_path / "rand.json"
    path.write_text(json.dumps(cfg))
    scfg = sc.load_scene_config(str(path))
    rig = SceneRig.from_config(str(path))
    r = sc.scene_rig(scfg, str(tmp_path))
    t, n, ch = sc.object_arrays(scfg.objects[name], str(tmp_path))
    sel = r["object_id"] == 0
    assert sel.sum() == len(t)
    assert np.array_equal(r["materials"][r["material_id"][sel]], ch)  # float64, exactly
    a, cnt = r["material_slots"][0]
    groups = len(t) if kind == "per-triangle" else len(np.unique(r["material_id"][sel]))
    assert (a, cnt) == (0, groups) and cnt > 1 and len(r["materials"]) == cnt + 1 > len(r["names"])
    assert rig.material_of(name) == slice(0, cnt) and rig.material_of("light_0") == cnt
    assert len(np.unique(ch[:, :3], axis=0)) > 1  # the colours do differ


def test_trs_matches_transform_vertices():
    rng = np.random.default_rng(3)
    for _ in range(20):
        tr = rng.uniform(-2, 2, 3)
        rot = rng.uniform(-180, 180, 3)
        s = rng.uniform(0.3, 3, 3) * rng.choice([-1, 1], 3)
        v = rng.uniform(-1, 1, (50, 3))
        ref = sc.transform_vertices(v, sc.TransformConfig(list(tr), list(rot), list(s), normalize=False))
        m = trs(tr, rot, s)
        assert m.dtype == torch.float32 and tuple(m.shape) == (3, 4)
        m64 = sc.transform_matrix(sc.TransformConfig(list(tr), list(rot), list(s)))
        assert np.array_equal(m.numpy(), m64.astype(np.float32))
        # the fp64 matrix against the converter's step-by-step form: a few fp64 roundings
        assert np.abs(v @ m64[:, :3].T + m64[:, 3] - ref).max() < 1e-14
        # the float32 matrix: its entries' rounding, 2^-24 (|A| |v| + |t|) each, with the bound's factor 4
        a = m.double().numpy()
        bound = 4 * U * (np.abs(v) @ np.abs(a[:, :3]).T + np.abs(a[:, 3]))
        assert np.all(np.abs(v @ a[:, :3].T + a[:, 3] - ref) <= bound)
    assert torch.equal(trs(scale=2.0), torch.tensor([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 2.0, 0]]))


def _one(normal, a, t=(0, 0, 0), vertex=(1.0, 2.0, 3.0)):
    arrays = dict(triangles=np.tile(np.asarray(vertex, dtype=np.float64), (1, 3, 1)),
                  vn=np.tile(np.asarray(normal, dtype=np.float64), (1, 3, 1)),
                  object_id=np.zeros(1, np.int32), material_id=np.zeros(1, np.int32))
    xf = np.concatenate([np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1)[None]
    return pose_numpy(arrays, xf, np.arange(13.0)[None])


def test_pose_numpy_semantics():
    # a mirror in x of a unit cube's +x face (outward normal +x): the face moves to x = -1, outward is now -x
    t, n, rows = _one((1, 0, 0), np.diag([-1.0, 1, 1]), vertex=(1.0, 0.5, 0.5))
    assert np.array_equal(t[0, 0], [-1.0, 0.5, 0.5]) and np.array_equal(n[0, 0], [-1.0, 0, 0])
    assert np.array_equal(rows[0], np.arange(13.0))
    # ... and its +y face keeps +y
    assert np.array_equal(_one((0, 1, 0), np.diag([-1.0, 1, 1]))[1][0, 0], [0, 1.0, 0])
    # non-uniform scale: diag(1, 2, 4) sends (1, 1, 0) / sqrt 2 to (1, 1/2, 0) / |.|  (A^-T n), not to A n
    n = _one(np.array([1, 1, 0]) / np.sqrt(2), np.diag([1.0, 2, 4]))[1][0, 0]
    assert np.allclose(n, np.array([1, 0.5, 0]) / np.linalg.norm([1, 0.5, 0]), rtol=0, atol=1e-15)
    # a zero normal stays zero; a singular matrix gives finite output
    assert np.array_equal(_one((0, 0, 0), np.diag([1.0, 2, 4]))[1][0, 0], [0, 0, 0])
    for a in (np.zeros((3, 3)), np.diag([1.0, 1, 0]), np.ones((3, 3))):
        for nrm in ((0, 0, 1.0), (1.0, 0, 0)):
            t, n, _ = _one(nrm, a)
            assert np.isfinite(t).all() and np.isfinite(n).all()
            assert np.all((np.abs(np.linalg.norm(n, axis=-1) - 1) < 1e-12) | (np.linalg.norm(n, axis=-1) == 0))
    # rank 2: the plane's normal survives
    assert np.array_equal(_one((0, 0, 1.0), np.diag([1.0, 1, 0]))[1][0, 0], [0, 0, 1.0])
    # padding rows pass through; their material row is zero
    arrays = dict(triangles=np.ones((2, 3, 3)), vn=np.full((2, 3, 3), 0.25), object_id=np.array([0, -1], np.int32),
                  material_id=np.array([0, -1], np.int32))
    t, n, rows = pose_numpy(arrays, np.array([[[2.0, 0, 0, 1], [0, 2, 0, 1], [0, 0, 2, 1]]]), np.ones((1, 13)))
    assert np.array_equal(t[1], np.ones((3, 3))) and np.array_equal(n[1], np.full((3, 3), 0.25))
    assert np.array_equal(rows[1], np.zeros(13)) and np.array_equal(t[0], np.full((3, 3), 3.0))


def _good(B=2, N=5, K=3, M=4, C=13):
    rng = np.random.default_rng(0)
    oid = rng.integers(0, K, (B, N)).astype(np.int32)
    mid = rng.integers(0, M, (B, N)).astype(np.int32)
    oid[:, -1] = mid[:, -1] = -1
    return dict(triangles=rng.standard_normal((B, N, 3, 3)).astype(np.float32),
                vn=rng.standard_normal((B, N, 3, 3)).astype(np.float32), object_id=oid, material_id=mid,
                names=[f"o{k}" for k in range(K)], transforms0=np.tile(trs().numpy(), (B, K, 1, 1)),
                materials0=rng.uniform(0, 1, (B, M, C)).astype(np.float32))


def test_scene_rig_accepts_a_valid_rig():
    g = _good()
    rig = SceneRig(**g)
    assert rig.batch_size == 2 and rig.mask.dtype == torch.bool and not bool(rig.mask[:, -1].any())
    assert rig.triangles.dtype == torch.float32 and rig.object_id.dtype == torch.int32
    assert tuple(rig.transforms0.shape) == (2, 3, 3, 4) and tuple(rig.materials0.shape) == (2, 4, 13)
    same = rig.to("cpu")
    assert same is not rig and torch.equal(same.triangles, rig.triangles) and same.names == rig.names
    with pytest.raises(ValueError, match="no object"):
        rig.material_of("nobody")


def _edit(g, key, fn):
    g = dict(g)
    g[key] = fn(g[key].copy() if isinstance(g[key], np.ndarray) else list(g[key]))
    return g


def _set(idx, val):
    def fn(a):
        a[idx] = val
        return a
    return fn


@pytest.mark.parametrize("key,fn,msg", [
    ("object_id", _set((0, 0), 3), "object_id must lie"),             # == K
    ("object_id", _set((1, 2), -2), "object_id must lie"),
    ("material_id", _set((0, 0), 4), "material_id must lie"),         # == M
    ("material_id", _set((0, 1), -2), "material_id must lie"),
    ("material_id", _set((0, 0), -1), "needs a material"),            # a valid row without a material
    ("object_id", lambda a: a.astype(np.int64), "int32"),
    ("material_id", lambda a: a.astype(np.int16), "int32"),
    ("triangles", lambda a: a.astype(np.float64), "float32"),
    ("vn", lambda a: a.astype(np.float16), "float32"),
    ("transforms0", lambda a: a.astype(np.float64), "float32"),
    ("materials0", lambda a: a.astype(np.float64), "float32"),
    ("triangles", lambda a: a.reshape(2, 5, 9), "triangles must be"),
    ("vn", lambda a: a[:, :4], "vn must be"),
    ("object_id", lambda a: a[0], "object_id must be"),
    ("material_id", lambda a: a[:, :4], "material_id must be"),
    ("transforms0", lambda a: a[:, :2], "transforms0 must be"),
    ("transforms0", lambda a: np.concatenate([a, a[:, :, :1]], axis=2), "transforms0 must be"),  # [B, K, 4, 4]
    ("materials0", lambda a: a[0], "materials0 must be"),
    ("materials0", lambda a: np.concatenate([a, a], axis=2), "materials0 must be"),              # C = 26 > 16
    ("names", lambda a: a[:2], "transforms0 must be"),
    ("transforms0", _set((0, 0, 0, 0), np.nan), "finite"),
])
def test_scene_rig_validation(key, fn, msg):
    with pytest.raises(ValueError, match=msg):
        SceneRig(**_edit(_good(), key, fn))


def test_host_refusals_of_the_new_entry_points():
    """rf_pose_scene / rf_texture_rows return RF_ERR_INVALID with a message before any HIP call (no device here)."""
    from renderformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librfhip.so not built")
    lib = _lib.load(require_device=False)
    p = ctypes.c_void_p(256)
    #        tris vn oid mid xf ld materials B  N  K  M  C  tris_out vn_out tex_out stream
    good = [p, p, p, p, p, 12, p, 2, 67, 3, 5, 13, p, p, p, None]

    def pose(**kw):
        names = ["tris", "vn", "oid", "mid", "xf", "ld", "materials", "B", "N", "K", "M", "C", "tris_out", "vn_out",
                 "tex_out", "stream"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return int(lib.rf_pose_scene(*a)), lib.rf_last_error()

    for name in ("tris", "vn", "oid", "mid", "xf", "materials", "tris_out", "vn_out", "tex_out"):
        rc, msg = pose(**{name: None})
        assert rc == 1 and b"null" in msg, (name, rc, msg)
    for ld in (0, 3, 9, 13, 15, 20, -12):
        rc, msg = pose(ld=ld)
        assert rc == 1 and b"ld_xf" in msg, (ld, rc, msg)
    rc, msg = pose(C=17)
    assert rc == 1 and b"channels" in msg
    for name in ("B", "N", "K", "M", "C"):
        rc, msg = pose(**{name: -1})
        assert rc == 1 and b"negative" in msg, (name, rc, msg)
    rc, msg = pose(B=1 << 16, N=1 << 15)
    assert rc == 1 and b"2^31" in msg
    assert pose(B=0)[0] == 0 and pose(N=0)[0] == 0  # nothing to do: no launch, no device needed

    rows = lambda *a: (int(lib.rf_texture_rows(*a)), lib.rf_last_error())  # noqa: E731
    assert rows(None, 10, 13, 3, p, p, 16, None)[0] == 1 and b"null" in lib.rf_last_error()
    assert rows(p, 10, 13, 3, p, None, 16, None)[0] == 1 and b"null" in lib.rf_last_error()
    assert rows(p, 10, 17, 3, p, p, 32, None)[0] == 1 and b"channels" in lib.rf_last_error()
    assert rows(p, 10, 0, 0, p, p, 16, None)[0] == 1
    assert rows(p, 10, 13, 3, p, p, 12, None)[0] == 1 and b"ldc" in lib.rf_last_error()
    assert rows(p, 10, 13, 14, p, p, 16, None)[0] == 1 and b"log_channels" in lib.rf_last_error()
    assert rows(p, 10, 13, -1, p, p, 16, None)[0] == 1
    assert rows(p, -1, 13, 3, p, p, 16, None)[0] == 1 and b"rows" in lib.rf_last_error()
    assert rows(p, 0, 13, 3, p, p, 16, None)[0] == 0


def test_pipeline_texture_lets_the_compact_form_through():
    """pipeline._texture lets [B, N, C] through with the checks of the expanded form (float32, contiguous)."""
    from renderformer_amd.pipeline import RenderFormerRenderingPipeline as P

    class _Cfg:
        texture_encode_patch_size = 32

    class _M:
        config = _Cfg()

    pipe = P(_M())
    t = torch.zeros(1, 4, 13)
    assert pipe._texture(t) is t
    with pytest.raises(ValueError, match="float32"):
        pipe._texture(t.double())
    with pytest.raises(ValueError, match="contiguous"):
        pipe._texture(torch.zeros(1, 13, 4).transpose(1, 2))
