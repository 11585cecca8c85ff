"""A scene in its rest pose, posed per frame on the device (``RenderFormerRenderingPipeline.pose``).

The converter (``scene_convert.scene_arrays``) bakes every object's transform and material into the triangles, the
normals and a [N, 13, 32, 32] texture: a moving object or a changing material means converting, expanding and
uploading the scene again.  A ``SceneRig`` keeps what does not change -- the rest-pose triangles and normals and,
per triangle, the index of its object and of its material -- and ``pose`` applies a 3 x 4 matrix per object and a
material table per frame in one HIP launch (rf.h rf_pose_scene), giving ``triangles``, ``vn`` and the compact
``texture`` [B, N, 13] that ``encode``, ``render`` and ``gbuffer`` take.

    rig = SceneRig.from_config("examples/cbox-teapot.json").to("cuda")
    xf, mat = rig.transforms0.clone(), rig.materials0.clone()      # the config's own values
    xf[0, rig.names.index("teapot")] = trs(translation, (0, 0, 30.0), scale)
    mat[0, rig.material_of("teapot"), 6] = 0.7                     # roughness
    hdr = pipe.render(*pipe.pose(rig, xf, mat), c2w, fov)

Arithmetic (the same in ``pose_numpy`` in float64 and in the kernel): with A = xf[:, :3] (rows a0, a1, a2) and
t = xf[:, 3], a vertex p goes to A p + t; a normal n to g / |g| with g = s cof(A) n, cof(A)'s rows a1 x a2, a2 x a0,
a0 x a1 and s = -1 if det A < 0 else +1 -- A^-T n up to a positive factor: right under non-uniform scale, on the
outward side under a mirror, (0, 0, 0) for a zero normal or when g vanishes (a singular A), never NaN.  Padding rows
(object id -1) pass through unchanged with a zero material row.

Parity with the converter: a rig posed with ``transforms0`` / ``materials0`` reproduces ``scene_arrays`` for every
object that is flat-shaded or uniformly scaled (up to the converter's 8-decimal rounding and fp32).  For a
smooth-shaded object under NON-uniform scale the converter measures its 30-degree smoothing groups and angle weights
on the transformed mesh, so its normals differ from the rest normals transformed geometrically, which is what a rig
gives.
"""
from __future__ import annotations

import math
import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch


class PosedScene(NamedTuple):
    """What ``pose`` returns: unpacks into ``encode`` / ``render`` / ``gbuffer`` (``texture`` is [B, N, C])."""
    triangles: torch.Tensor
    texture: torch.Tensor
    mask: torch.Tensor
    vn: torch.Tensor


def trs(translation=(0.0, 0.0, 0.0), rotation_deg=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)) -> torch.Tensor:
    """float32 [3, 4] ``[A | t]`` in the converter's order (scene_convert.transform_vertices): rotate about x, then
    y, then z (degrees), then scale per axis, then translate: A = diag(scale) Rz Ry Rx.  ``scale`` may be a number."""
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64), (3,))
    a = np.eye(3)
    for axis, deg in enumerate(rotation_deg):
        c, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        r = np.eye(3)
        r[i, i], r[i, j], r[j, i], r[j, j] = c, -sn, sn, c
        a = r @ a
    m = np.concatenate([s[:, None] * a, np.asarray(translation, dtype=np.float64).reshape(3, 1)], axis=1)
    return torch.from_numpy(m.astype(np.float32))


def pose_numpy(rig_arrays, xf, materials=None):
    """The pose in float64 numpy: the tests' reference and a CPU fallback.  ``rig_arrays``: a SceneRig or a mapping
    with 'triangles', 'vn' ([B, N, 3, 3] or [N, 3, 3]), 'object_id', 'material_id' ([B, N] or [N]; and 'materials'
    if ``materials`` is None); ``xf`` [(B,) K, 3 | 4, 4]; ``materials`` [(B,) M, C].  Returns (triangles, vn,
    texture rows [..., C]) as float64, batched like the input."""
    get = (lambda k: getattr(rig_arrays, k)) if isinstance(rig_arrays, SceneRig) else (lambda k: rig_arrays[k])
    as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)  # noqa: E731
    tris, vn = as_np(get("triangles")).astype(np.float64), as_np(get("vn")).astype(np.float64)
    oid, mid = as_np(get("object_id")).astype(np.int64), as_np(get("material_id")).astype(np.int64)
    if materials is None:
        materials = get("materials0") if isinstance(rig_arrays, SceneRig) else get("materials")
    xf, mat = as_np(xf).astype(np.float64), as_np(materials).astype(np.float64)
    single = oid.ndim == 1
    if single:
        tris, vn, oid, mid, xf, mat = tris[None], vn[None], oid[None], mid[None], xf[None], mat[None]
    B, N = oid.shape
    tris, vn = tris.reshape(B, N, 3, 3), vn.reshape(B, N, 3, 3)
    a, t = xf[:, :, :3, :3], xf[:, :, :3, 3]
    cof = np.stack([np.cross(a[:, :, 1], a[:, :, 2]), np.cross(a[:, :, 2], a[:, :, 0]),
                    np.cross(a[:, :, 0], a[:, :, 1])], axis=2)                      # [B, K, 3, 3]
    det = (a[:, :, 0] * cof[:, :, 0]).sum(-1)
    cof = np.where(det[..., None, None] < 0, -cof, cof)
    out_t, out_n = tris.copy(), vn.copy()
    rows = np.zeros((B, N, mat.shape[-1]))
    for b in range(B):
        sel = oid[b] >= 0
        o = oid[b][sel]
        out_t[b][sel] = np.einsum("nij,nvj->nvi", a[b][o], tris[b][sel]) + t[b][o][:, None, :]
        g = np.einsum("nij,nvj->nvi", cof[b][o], vn[b][sel])
        ln = np.linalg.norm(g, axis=-1, keepdims=True)
        out_n[b][sel] = np.where(ln > 0, g / np.where(ln > 0, ln, 1.0), 0.0)
        rows[b][sel] = mat[b][mid[b][sel]]
    if single:
        return out_t[0], out_n[0], rows[0]
    return out_t, out_n, rows


def _host(x, name) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    if not isinstance(x, np.ndarray):
        raise ValueError(f"SceneRig: {name} must be a numpy array or a tensor, got {type(x).__name__}")
    return x


class SceneRig:
    """Rest-pose scenes, batched: ``triangles`` / ``vn`` float32 [B, N, 3, 3], ``object_id`` / ``material_id`` int32
    [B, N] (-1 marks a padding row), ``mask`` bool [B, N] (object_id >= 0), ``names`` (the K objects),
    ``transforms0`` float32 [B, K, 3, 4] and ``materials0`` float32 [B, M, C], the values the rig was built with.

    The constructor validates everything once on the host (numpy) and raises ValueError: dtypes, shapes, object ids
    within [-1, K), material ids within [-1, M) and >= 0 on every row that has an object.  The kernel therefore
    needs no check against bad ids.  ``to(device)`` returns a rig on the device, validated already."""

    def __init__(self, triangles, vn, object_id, material_id, names: Sequence[str], transforms0, materials0,
                 material_slots: Optional[Sequence] = None):
        tris, vn_, oid, mid = (_host(x, n) for x, n in ((triangles, "triangles"), (vn, "vn"),
                                                         (object_id, "object_id"), (material_id, "material_id")))
        xf, mat = _host(transforms0, "transforms0"), _host(materials0, "materials0")
        for x, n in ((tris, "triangles"), (vn_, "vn"), (xf, "transforms0"), (mat, "materials0")):
            if x.dtype != np.float32:
                raise ValueError(f"SceneRig: {n} must be float32, got {x.dtype}")
        for x, n in ((oid, "object_id"), (mid, "material_id")):
            if x.dtype != np.int32:
                raise ValueError(f"SceneRig: {n} must be int32, got {x.dtype}")
        if oid.ndim != 2:
            raise ValueError(f"SceneRig: object_id must be [B, N], got {oid.shape}")
        B, N = oid.shape
        if mid.shape != (B, N):
            raise ValueError(f"SceneRig: material_id must be {(B, N)} like object_id, got {mid.shape}")
        for x, n in ((tris, "triangles"), (vn_, "vn")):
            if x.shape != (B, N, 3, 3):
                raise ValueError(f"SceneRig: {n} must be {(B, N, 3, 3)}, got {x.shape}")
        self.names: List[str] = [str(n) for n in names]
        K = len(self.names)
        if xf.shape != (B, K, 3, 4):
            raise ValueError(f"SceneRig: transforms0 must be {(B, K, 3, 4)} ({K} names), got {xf.shape}")
        if mat.ndim != 3 or mat.shape[0] != B or not 1 <= mat.shape[2] <= 16:
            raise ValueError(f"SceneRig: materials0 must be [{B}, M, C <= 16], got {mat.shape}")
        M = mat.shape[1]
        if oid.size and (oid.min() < -1 or oid.max() >= K):
            raise ValueError(f"SceneRig: object_id must lie in [-1, {K}), found [{oid.min()}, {oid.max()}]")
        if mid.size and (mid.min() < -1 or mid.max() >= M):
            raise ValueError(f"SceneRig: material_id must lie in [-1, {M}), found [{mid.min()}, {mid.max()}]")
        if np.any((oid >= 0) & (mid < 0)):
            raise ValueError("SceneRig: a triangle with an object needs a material (material_id -1 on a valid row)")
        if not (np.isfinite(xf).all() and np.isfinite(mat).all()):
            raise ValueError("SceneRig: transforms0 and materials0 must be finite")
        self.material_slots = None if material_slots is None else [tuple(int(v) for v in s) for s in material_slots]
        if self.material_slots is not None and (len(self.material_slots) != K or any(
                a < 0 or n < 1 or a + n > M for a, n in self.material_slots)):
            raise ValueError(f"SceneRig: material_slots must hold one (first row, count) inside [0, {M}) per object")
        f = torch.from_numpy
        self.triangles, self.vn = f(np.ascontiguousarray(tris)), f(np.ascontiguousarray(vn_))
        self.object_id, self.material_id = f(np.ascontiguousarray(oid)), f(np.ascontiguousarray(mid))
        self.mask = f(np.ascontiguousarray(oid >= 0))
        self.transforms0, self.materials0 = f(np.ascontiguousarray(xf)), f(np.ascontiguousarray(mat))

    _TENSORS = ("triangles", "vn", "object_id", "material_id", "mask", "transforms0", "materials0")

    @property
    def device(self):
        return self.triangles.device

    @property
    def batch_size(self) -> int:
        return int(self.object_id.shape[0])

    def to(self, device) -> "SceneRig":
        """The rig on ``device`` (a new object sharing nothing that is moved; no validation is repeated)."""
        new = object.__new__(SceneRig)
        new.names, new.material_slots = list(self.names), self.material_slots
        for n in self._TENSORS:
            setattr(new, n, getattr(self, n).to(device).contiguous())
        return new

    def material_of(self, name: str):
        """The row of ``materials0[b]`` that object ``name`` uses: an int, or a slice when the object owns several
        rows (``rand_tri_diffuse_seed``: one per colour group) -- either indexes ``mat[b, rig.material_of(name)]``."""
        if name not in self.names:
            raise ValueError(f"SceneRig: no object {name!r} (objects: {self.names})")
        k = self.names.index(name)
        if self.material_slots is not None:
            a, n = self.material_slots[k]
            return a if n == 1 else slice(a, a + n)
        ids = torch.unique(self.material_id[self.object_id == k]).tolist()
        if not ids:
            raise ValueError(f"SceneRig: object {name!r} has no triangles")
        if ids == list(range(ids[0], ids[0] + len(ids))):
            return ids[0] if len(ids) == 1 else slice(ids[0], ids[0] + len(ids))
        return ids

    @classmethod
    def from_arrays(cls, triangles, vn, object_id, material_id, names, transforms, materials, material_slots=None):
        """A one-scene rig (B = 1) from unbatched arrays as ``scene_convert.scene_rig`` returns them (any float /
        integer dtype: they are cast to float32 / int32 here, as the device will see them)."""
        f32 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32))[None]  # noqa: E731
        i32 = lambda x: np.ascontiguousarray(np.asarray(x).astype(np.int32))[None]  # noqa: E731
        xf = np.asarray(transforms, dtype=np.float64)
        if xf.ndim == 3 and xf.shape[1:] == (4, 4):
            xf = xf[:, :3]
        return cls(f32(triangles), f32(vn), i32(object_id), i32(material_id), names, f32(xf), f32(materials),
                   material_slots)

    @classmethod
    def from_config(cls, path: str) -> "SceneRig":
        """The rest-pose rig of a scene description (examples/*.json): ``transforms0`` / ``materials0`` are the
        config's own transforms and materials, so posing with them gives the converted scene."""
        from .scene_convert import load_scene_config, scene_rig
        r = scene_rig(load_scene_config(path), os.path.dirname(os.path.abspath(path)))
        return cls.from_arrays(r["triangles"], r["vn"], r["object_id"], r["material_id"], r["names"], r["transforms"],
                               r["materials"], r["material_slots"])
