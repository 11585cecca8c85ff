"""Reference, band rule and conformance meshes of the G-buffer tests (a helper, imported by name: not a test).

hits_ref       the hit rule of rf.h rf_primary_hits in fp64 numpy: the rays by kernel_checks.ray_tokens_ref's formula
               in fp64 from the fp32 inputs, then Moeller-Trumbore against every valid triangle.  Double-sided; hit
               iff det != 0, u >= 0, v >= 0, u + v <= 1 and t > 0; nearest t, lowest index among equal t; a zero-area
               or non-finite triangle is never hit.  Chunked over pixels (a [P, N, 3] fp64 temporary of a 64 x 64
               frame against 5,633 triangles would be 0.55 GB).
hits_f32       the same statement in plain fp32 numpy.  It only sets the depth tolerance of a case: 4 x its worst
               relative depth error against hits_ref over the kept pixels, floored at 2^-20 (the factor covers another,
               algebraically equal evaluation order and FMA contraction).
band           with EPS = 1e-4 a pixel is left out of the exact comparison iff, in fp64, some triangle with t > 0 and
               t <= t_nearest (1 + EPS) + EPS has |min(u, v, 1 - u - v)| < EPS (the ray grazes an edge of something at
               least as near as the hit), or the second-nearest hit lies within EPS max(1, t) of the nearest.  Inside
               the band the id must still be a candidate: a triangle with t > 0 whose footprint widened by EPS holds
               the pixel and that is no farther than the nearest robust hit (by the same margin); a miss is allowed
               iff there is no robust hit.
grid_mesh      the two watertightness meshes: a planar grid of 18 x 18 quads (648 triangles, mixed winding) in front
               of a 64 x 64 camera with intrinsics fx = fy = 64, cx = cy = 32, so pixel-centre directions are exact in
               camera space.  'vertex': grid vertices at every 4th pixel centre (edges and vertices pass through pixel
               centres); 'edge': the same offset half a pixel in y (only edges do).  The grid extends a cell past the
               frame on every side and moves rigidly with the camera (GRID_CAMERAS: identity and three rotated,
               translated ones).
edge_emulation the kernel's inside test restated in numpy fp32 (edge functions with canonically ordered cross products,
               fp64 re-evaluation inside the per-edge threshold), with a switch that plants the defect the
               vertex mesh is there to catch: no fp64 re-evaluation.  (The canonical order matters only under FMA
               contraction, which numpy does not do: there p x q = -(q x p) exactly.)
"""
import math

import numpy as np
import torch

import kernel_checks as kc

EPS = 1e-4
BAND_CAP = 0.02  # a case's band holds at most 2 % of its pixels
DEPTH_FLOOR = 2.0 ** -20


# ------------------------------------------------------------------------------------------------ rays
def rays_ref(c2w, fov, intr, frame):
    """(origins fp64 [v, 3], rotated directions BEFORE normalisation fp64 [v, h, w, 3], their norms [v, h, w]) by
    kernel_checks.ray_tokens_ref's formula (patch 1, no overscan), checked against it.  The hit rule does not depend
    on the direction's length, so hits_ref evaluates it on the unnormalised direction and scales t: where the inputs
    are exact (the identity camera of the conformance meshes) so is the inside test, which a direction normalised
    and rounded again would miss by 1e-17."""
    h, w = frame
    m = c2w.double().reshape(-1, 4, 4).numpy()
    nv = m.shape[0]
    if intr is not None:
        k = intr.double().reshape(nv, 4).numpy()
        fx, fy, cx, cy = k[:, 0], k[:, 1], k[:, 2], k[:, 3]
    else:
        fx = fy = h / 2.0 / np.tan(0.5 * (fov.double().reshape(nv).numpy() / 180.0 * math.pi))
        cx, cy = np.full(nv, w / 2.0), np.full(nv, h / 2.0)
    xs = np.arange(w, dtype=np.float64)[None, None, :] + 0.5
    ys = np.arange(h, dtype=np.float64)[None, :, None] + 0.5
    v3 = lambda a: a[:, None, None]  # noqa: E731
    dcam = np.stack(np.broadcast_arrays((xs - v3(cx)) / v3(fx), -((ys - v3(cy)) / v3(fy)), -np.ones((nv, h, w))), -1)
    r = np.einsum("vhwb,vab->vhwa", dcam, m[:, :3, :3])
    nrm = np.maximum(np.linalg.norm(r, axis=-1), 1e-12)
    tok, pos, _ = kc.ray_tokens_ref(c2w, fov, intr, (h, w), (h, w), (0, 0), 1)
    assert np.abs(r / nrm[..., None] - tok.reshape(nv, h, w, 3).numpy()).max() < 1e-14
    return pos[:, :3].numpy(), r, nrm


def rays_f32(c2w, fov, intr, frame):
    """The same rays in fp32 numpy, operation for operation as the kernels write them."""
    h, w = frame
    m = c2w.reshape(-1, 4, 4).numpy().astype(np.float32)
    nv = m.shape[0]
    f32 = np.float32
    if intr is not None:
        k = intr.reshape(nv, 4).numpy().astype(np.float32)
        fx, fy, cx, cy = k[:, 0], k[:, 1], k[:, 2], k[:, 3]
    else:
        rad = fov.reshape(nv).numpy().astype(np.float32) / f32(180.0) * f32(math.pi)
        fx = fy = f32(h) / f32(2.0) / np.tan(f32(0.5) * rad).astype(np.float32)
        cx, cy = np.full(nv, f32(w) / f32(2.0), np.float32), np.full(nv, f32(h) / f32(2.0), np.float32)
    xs = np.arange(w, dtype=np.float32)[None, None, :] + f32(0.5)
    ys = np.arange(h, dtype=np.float32)[None, :, None] + f32(0.5)
    v3 = lambda a: a[:, None, None]  # noqa: E731
    dx = np.broadcast_to((xs - v3(cx)) / v3(fx), (nv, h, w))
    dy = np.broadcast_to(-((ys - v3(cy)) / v3(fy)), (nv, h, w))
    dz = np.full((nv, h, w), -1.0, np.float32)
    r = np.stack([dx * m[:, a, 0, None, None] + dy * m[:, a, 1, None, None] + dz * m[:, a, 2, None, None]
                  for a in range(3)], axis=-1).astype(np.float32)
    nrm = np.maximum(np.sqrt((r * r).sum(-1, keepdims=True, dtype=np.float32)), f32(1e-12))
    return m[:, :3, 3].copy(), (r / nrm).astype(np.float32)


# ------------------------------------------------------------------------------------------------ Moeller-Trumbore
def _mt(tris, origin, d, dtype):
    """t, u, v, ok [P, N] of rays d [P, 3] from `origin` against tris [N, 9] in `dtype` (ok: the plane is not parallel
    and the triangle is finite with a non-zero area)."""
    t9 = tris.astype(dtype)
    v0, e1, e2 = t9[:, 0:3], t9[:, 3:6] - t9[:, 0:3], t9[:, 6:9] - t9[:, 0:3]
    dead = ~np.isfinite(t9).all(axis=1) | (np.cross(e1.astype(np.float64), e2.astype(np.float64)) == 0).all(axis=1)
    with np.errstate(all="ignore"):
        p = np.cross(d[:, None, :], e2[None, :, :])            # [P, N, 3]
        det = (e1[None] * p).sum(-1)
        s = (origin.astype(dtype) - v0)[None]                   # [1, N, 3]
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1[None])
        v = (d[:, None, :] * q).sum(-1) / det
        t = (e2[None] * q).sum(-1) / det
    ok = (det != 0) & ~dead[None] & np.isfinite(t) & np.isfinite(u) & np.isfinite(v)
    return t, u, v, ok


def _nearest(t, hit):
    """(index of the smallest t among hit, lowest index among equal t; -1 where nothing is hit, its t)."""
    tm = np.where(hit, t, np.inf)
    k = tm.argmin(axis=1)  # (argmin returns the first of equal minima: the lowest index)
    tk = tm[np.arange(t.shape[0]), k]
    return np.where(np.isfinite(tk), k, -1), tk


def hits_ref(tris, ids, origin, dirs, norms=None, chunk_pairs=1 << 21):
    """fp64 reference for one view: tris fp32 [N, 9] (the valid rows) with their input-axis ids [N], origin [3], dirs
    [h, w, 3] fp64 of length norms [h, w] (None: unit length).  Returns a dict of [h, w] arrays: depth along the unit
    direction (inf on a miss), tri_id (-1), u, v (0), band (bool) and
    `allowed`, a list over pixels of the id sets a banded pixel may report (None for a kept pixel)."""
    h, w, _ = dirs.shape
    d_all = dirs.reshape(-1, 3).astype(np.float64)
    n_all = np.ones(h * w) if norms is None else norms.reshape(-1).astype(np.float64)
    P, N = d_all.shape[0], tris.shape[0]
    out = dict(depth=np.full(P, np.inf), tri_id=np.full(P, -1, np.int64), u=np.zeros(P), v=np.zeros(P),
               band=np.zeros(P, bool))
    allowed = [None] * P
    ids = np.asarray(ids, np.int64)
    step = max(1, chunk_pairs // max(N, 1))
    for p0 in range(0, P, step if N else P):
        d = d_all[p0:p0 + step]
        n = d.shape[0]
        if N == 0:
            break
        t, u, v, ok = _mt(tris, np.asarray(origin, np.float64), d, np.float64)
        t = t * n_all[p0:p0 + n, None]  # distance along the unit direction
        mb = np.minimum(np.minimum(u, v), 1.0 - u - v)
        front = ok & (t > 0)
        hit = front & (mb >= 0)
        k, tk = _nearest(t, hit)
        rows = np.arange(n)
        got = k >= 0
        out["depth"][p0:p0 + n] = tk
        out["tri_id"][p0:p0 + n] = np.where(got, ids[np.maximum(k, 0)], -1)
        out["u"][p0:p0 + n] = np.where(got, u[rows, np.maximum(k, 0)], 0.0)
        out["v"][p0:p0 + n] = np.where(got, v[rows, np.maximum(k, 0)], 0.0)
        # band: a grazed edge at least as near as the hit, or a second hit within EPS max(1, t)
        near = front & (t <= (tk * (1 + EPS) + EPS)[:, None])
        graze = (near & (np.abs(mb) < EPS)).any(axis=1)
        t2 = np.where(hit, t, np.inf)
        t2[rows[got], k[got]] = np.inf
        with np.errstate(invalid="ignore"):  # (inf - inf where nothing is hit: False)
            second = got & (t2.min(axis=1) - tk <= EPS * np.maximum(1.0, tk))
        band = graze | second
        out["band"][p0:p0 + n] = band
        # candidates of a banded pixel
        wide = front & (mb >= -EPS)
        robust = front & (mb >= EPS)
        tr = np.where(robust, t, np.inf).min(axis=1)
        cand = wide & (t <= (tr * (1 + EPS) + EPS)[:, None])
        for i in np.flatnonzero(band):
            s = set(int(x) for x in ids[np.flatnonzero(cand[i])])
            if not np.isfinite(tr[i]):
                s.add(-1)
            allowed[p0 + i] = s
    res = {k_: a.reshape(h, w) for k_, a in out.items()}
    res["allowed"] = allowed
    return res


def hits_f32(tris, ids, origin, dirs, chunk_pairs=1 << 21):
    """The hit rule in plain fp32 numpy: depth and tri_id [h, w] (tolerance setting only)."""
    h, w, _ = dirs.shape
    d_all = dirs.reshape(-1, 3).astype(np.float32)
    P, N = d_all.shape[0], tris.shape[0]
    depth, tid = np.full(P, np.inf, np.float32), np.full(P, -1, np.int64)
    ids = np.asarray(ids, np.int64)
    step = max(1, chunk_pairs // max(N, 1))
    for p0 in range(0, P if N else 0, step):
        t, u, v, ok = _mt(tris, np.asarray(origin, np.float32), d_all[p0:p0 + step], np.float32)
        with np.errstate(invalid="ignore"):
            hit = ok & (t > 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        k, tk = _nearest(t, hit)
        depth[p0:p0 + len(k)] = tk
        tid[p0:p0 + len(k)] = np.where(k >= 0, ids[np.maximum(k, 0)], -1)
    return depth.reshape(h, w), tid.reshape(h, w)


def depth_tolerance(ref, f32_depth):
    """4 x the worst relative depth error of the fp32 restatement against fp64 over the kept hit pixels, floored."""
    keep = ~ref["band"] & np.isfinite(ref["depth"]) & np.isfinite(f32_depth)
    if not keep.any():
        return DEPTH_FLOOR, 0.0
    worst = float(np.max(np.abs(f32_depth[keep].astype(np.float64) - ref["depth"][keep]) / ref["depth"][keep]))
    return max(4.0 * worst, DEPTH_FLOOR), worst


def scene_ref(triangles, mask, c2w, fov, intr, frame, want_f32=True):
    """References of a whole call: triangles fp32 [B, N, 9] (or [B, N, 3, 3]), mask bool [B, N], c2w [B, V, 4, 4], fov
    [B, V(, 1)] or intr [B, V, 4] (torch, host).  Returns ref[b][v] (hits_ref dicts, plus 'f32_depth' and 'tol')."""
    B, V = c2w.shape[:2]
    tris = triangles.reshape(B, -1, 9).numpy()
    m = mask.numpy().astype(bool)
    out = []
    for b in range(B):
        ids = np.flatnonzero(m[b])
        cam_f = None if fov is None else fov[b].reshape(V)
        cam_i = None if intr is None else intr[b]
        o64, d64, n64 = rays_ref(c2w[b], cam_f, cam_i, frame)
        o32, d32 = rays_f32(c2w[b], cam_f, cam_i, frame)
        views = []
        for v in range(V):
            r = hits_ref(tris[b][ids], ids, o64[v], d64[v], n64[v])
            if want_f32:
                r["f32_depth"], r["f32_id"] = hits_f32(tris[b][ids], ids, o32[v], d32[v])
                r["tol"], r["f32_worst"] = depth_tolerance(r, r["f32_depth"])
            views.append(r)
        out.append(views)
    return out


def compare(ref, depth, tri_id, bary=None, what="", cap=BAND_CAP):
    """One view's kernel outputs ([h, w] numpy; bary [h, w, 2]) against its hits_ref dict: the band cap, exact ids and
    alpha outside the band, bary within 1e-4 and depth within ref['tol'] there, candidates inside it.  cap: the largest band share (None: no cap).
    Prints the figures before it asserts; returns them."""
    band = ref["band"]
    share = float(band.mean())
    keep = ~band
    id_bad = int((tri_id[keep] != ref["tri_id"][keep]).sum())
    hitk = keep & (ref["tri_id"] >= 0)
    ok_ids = hitk & (tri_id == ref["tri_id"])
    rel = np.abs(depth[ok_ids].astype(np.float64) - ref["depth"][ok_ids]) / ref["depth"][ok_ids]
    worst_rel = float(rel.max()) if rel.size else 0.0
    miss_ok = bool(np.isposinf(depth[keep & (ref["tri_id"] < 0)]).all())
    worst_b = 0.0
    if bary is not None and ok_ids.any():
        worst_b = float(max(np.abs(bary[..., 0][ok_ids] - ref["u"][ok_ids]).max(),
                            np.abs(bary[..., 1][ok_ids] - ref["v"][ok_ids]).max()))
    flat_id = tri_id.reshape(-1)
    cand_bad = [int(i) for i in np.flatnonzero(band.reshape(-1)) if int(flat_id[i]) not in ref["allowed"][i]]
    tol = ref.get("tol", DEPTH_FLOOR)
    print(f"{what}: band {share:.4%}, id mismatches outside the band {id_bad}, worst relative depth error "
          f"{worst_rel:.3e} (tolerance {tol:.3e}; the fp32 restatement's worst {ref.get('f32_worst', 0.0):.3e}), worst "
          f"bary error {worst_b:.3e}, banded pixels outside their candidates {len(cand_bad)}")
    assert cap is None or share <= cap, f"{what}: the band holds {share:.2%} of the pixels (cap {cap:.0%})"
    assert id_bad == 0, f"{what}: {id_bad} pixel(s) outside the band report another triangle than the fp64 reference"
    assert miss_ok, f"{what}: a missed pixel's depth is not +inf"
    assert worst_rel <= tol, f"{what}: relative depth error {worst_rel:.3e} > {tol:.3e}"
    assert worst_b <= 1e-4, f"{what}: barycentric error {worst_b:.3e} > 1e-4"
    assert not cand_bad, f"{what}: banded pixel(s) {cand_bad[:5]} report an id outside their candidate set"
    return dict(band=share, depth=worst_rel, bary=worst_b, tol=tol)


# ------------------------------------------------------------------------------------------------ conformance meshes
GRID_FRAME = (64, 64)
GRID_INTR = (64.0, 64.0, 32.0, 32.0)
GRID_Z = 2.0  # the plane's camera-space distance: a power of two, so the vertices are exact in fp32


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def grid_cameras():
    """c2w fp32 [4, 4, 4]: the identity and three fixed rotated and translated cameras."""
    cams = [np.eye(4)]
    for axis, deg, t in (((0.3, 1.0, 0.2), 37.0, (0.7, -1.3, 2.1)), ((1.0, -0.4, 0.6), 121.0, (-3.2, 0.4, 0.9)),
                         ((-0.2, 0.5, 1.0), 263.0, (11.0, 7.0, -5.0))):
        m = np.eye(4)
        m[:3, :3] = _rot(axis, deg)
        m[:3, 3] = t
        cams.append(m)
    return torch.from_numpy(np.stack(cams).astype(np.float32))


def grid_mesh(kind: str, c2w: torch.Tensor):
    """(triangles fp32 [648, 9] in world space, intr fp32 [4]) of the 'vertex' or 'edge' mesh for the camera c2w fp32
    [4, 4]: the camera-space grid moved by the camera's own (fp32) matrix, in fp64, rounded to fp32 once."""
    assert kind in ("vertex", "edge")
    fx, fy, cx, cy = GRID_INTR
    off = 0.5 if kind == "edge" else 0.0
    px = np.arange(-4, 69, 4, dtype=np.float64) + 0.5        # 19 pixel-centre columns from -3.5 to 68.5
    py = np.arange(-4, 69, 4, dtype=np.float64) + 0.5 + off
    X = (px - cx) / fx * GRID_Z
    Y = -(py - cy) / fy * GRID_Z
    vert = np.stack(np.broadcast_arrays(X[None, :], Y[:, None], np.full((19, 19), -GRID_Z)), axis=-1)  # [y, x, 3]
    m = c2w.double().numpy()
    world = (vert @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
    tris = []
    for j in range(18):
        for i in range(18):
            a, b, c, d = world[j, i], world[j, i + 1], world[j + 1, i + 1], world[j + 1, i]
            if (i + j) % 2 == 0:  # mixed winding and vertex order: a shared edge appears in both directions
                tris += [np.concatenate([a, b, c]), np.concatenate([d, c, a])]
            else:
                tris += [np.concatenate([c, b, a]), np.concatenate([a, c, d])]
    return torch.from_numpy(np.stack(tris)), torch.tensor(GRID_INTR)


def footprint_ok(ref_tris, origin, dirs, tri_id):
    """bool [h, w]: the reported triangle's closed fp64 footprint, widened by EPS, holds the pixel (dirs: of any
    length)."""
    h, w, _ = dirs.shape
    t, u, v, ok = _mt(ref_tris, np.asarray(origin, np.float64), dirs.reshape(-1, 3).astype(np.float64), np.float64)
    mb = np.minimum(np.minimum(u, v), 1.0 - u - v)
    wide = ok & (t > 0) & (mb >= -EPS)
    ids = tri_id.reshape(-1)
    return ((ids >= 0) & wide[np.arange(h * w), np.maximum(ids, 0)]).reshape(h, w)


# ------------------------------------------------------------------------------------------------ the kernel's inside test
EDGE_EPS = np.float32(2.5e-6)


def edge_emulation(tris, origin, dirs, fp64_fallback=True):
    """covered bool [h, w]: some triangle passes the inside test of visibility.hip, restated in numpy fp32 (without
    FMA contraction): edge functions d . (p x q) of the origin-relative vertices, the cross product with the vertices
    in lexicographic order and negated afterwards, re-evaluated in fp64 where |E| <= EDGE_EPS |p| |q|.
    fp64_fallback=False trusts the fp32 signs."""
    h, w, _ = dirs.shape
    f32 = np.float32
    d = dirs.reshape(-1, 3).astype(f32)
    t9 = tris.astype(f32)
    o = np.asarray(origin, f32)
    vs = [t9[:, 0:3] - o, t9[:, 3:6] - o, t9[:, 6:9] - o]
    sign_ok_pos = np.ones((d.shape[0], t9.shape[0]), bool)
    sign_ok_neg = np.ones_like(sign_ok_pos)
    for p, q in ((vs[1], vs[2]), (vs[2], vs[0]), (vs[0], vs[1])):
        sw = (q[:, 0] < p[:, 0]) | ((q[:, 0] == p[:, 0]) & ((q[:, 1] < p[:, 1]) |
                                                          ((q[:, 1] == p[:, 1]) & (q[:, 2] < p[:, 2]))))
        lo, hi = np.where(sw[:, None], q, p), np.where(sw[:, None], p, q)
        sgn = np.where(sw, f32(-1), f32(1))
        n = np.cross(lo, hi).astype(f32) * sgn[:, None]
        e = (d[:, None, 0] * n[None, :, 0] + d[:, None, 1] * n[None, :, 1] + d[:, None, 2] * n[None, :, 2]).astype(f32)
        e = e.astype(np.float64)
        if fp64_fallback:
            thr = EDGE_EPS * (np.linalg.norm(p, axis=1).astype(f32) * np.linalg.norm(q, axis=1).astype(f32))
            n64 = np.cross(lo.astype(np.float64), hi.astype(np.float64)) * sgn[:, None].astype(np.float64)
            e64 = d.astype(np.float64) @ n64.T
            e = np.where(np.abs(e) <= thr[None, :], e64, e)
        sign_ok_pos &= e >= 0
        sign_ok_neg &= e <= 0
    return (sign_ok_pos | sign_ok_neg).any(axis=1).reshape(h, w)
