"""Drop-in ``RenderFormerRenderingPipeline`` (renderformer/pipelines/rendering_pipeline.py:8-128).

Same constructor, ``from_pretrained``, ``device``, ``to``, ``render`` and
``__call__`` with the same argument names, shapes, dtypes and return value
``[bs, num_views, H, W, 3]`` float32 linear HDR.  Like the reference it
log-encodes the emission channels of ``texture`` **in place**
(rendering_pipeline.py:67-68).

Precision: the reference GPU path switches stage precision with
``torch_dtype`` (rendering_pipeline.py:98-99, view_transformer.py:119: half ->
stage 1 half, stage 2 fp32, DPT half; fp32 -> stage 1 fp32, stage 2 bf16).  This
path runs ONE policy for every ``torch_dtype``: fp16 projection operands (bf16 with
``operands="bf16"``, or after an fp16 overflow: ``RenderFormer.range_check``), bf16
attention q/k/v, fp32 accumulation / softmax / residual streams in both transformer
stages, and fp16-operand, fp32-accumulate DPT convolutions — the policy measured
within the 1e-3 relative-L2 parity budget of the reference CPU fp32 output at every
BASELINE configuration (tests/test_parity_gpu.py).  The argument is validated
exactly like the reference; ``torch.float32`` (which in the reference selects
fp32 stage-1 arithmetic) emits a one-time ``PrecisionWarning`` saying so, and
``last_precision`` records what ran (``RenderFormer.precision``).

fp16 range check: by default (``RenderFormer(range_check="sync")``) ``render`` waits for its own
frame's end event — no device sync, the wait the caller's ``.cpu()`` would do anyway — and
re-renders an overflowed frame with bf16 operands before returning, so unchanged callers of the
reference API (README example, ``infer.py``) never see a non-finite frame.  Pipelining callers
(``batch_infer.py``) opt in to ``range_check="lazy"`` and call ``resolve(out)`` / ``check_range()``.

Cameras that arrive over time (a viewer, an orbit rendered frame by frame, "same scene, new camera"):
``scene = pipe.encode(triangles, texture, mask, vn)`` runs everything that does not depend on the camera
once — the triangle embedding, stage 1 and every decoder layer's K/V — and ``pipe.render_encoded(scene,
c2w, fov, resolution)`` renders any number of cameras from the handle, each frame bit-identical to
``render`` of the same inputs.  The handle keeps the stage-1 output and the K/V on the device,
``T1 * (4 * D + n_layers * 4 * Dv)`` bytes (``scene.nbytes``; T1 = 16 register tokens + the valid triangles
per scene), and the input tensors, which must stay unmodified while it is in use.  After an fp16 overflow
fallback (in ``encode``, in ``render_encoded`` or in any other render of the model) the model computes with
bf16 operands: a handle made before it is encoded again from its retained inputs, once, at its next
``render_encoded``.  A handle belongs to the model that made it; ``to()`` / ``load_state_dict`` invalidate it.
"""
from __future__ import annotations

import warnings
from typing import Tuple, Union

import torch

from .model import PrecisionWarning, RenderFormer  # noqa: F401  (PrecisionWarning re-exported)


class RenderFormerRenderingPipeline:
    def __init__(self, model: RenderFormer):
        self.model = model
        self.config = model.config
        self.last_precision = None
        self._warned_fp32 = False

    @classmethod
    def from_pretrained(cls, model_id: str, **kwargs):
        model = RenderFormer.from_pretrained(model_id, **kwargs)
        model.eval()
        return cls(model)

    @property
    def device(self):
        return self.model.device

    def to(self, device):
        self.model.to(device)
        return self

    def _check_dtype(self, torch_dtype, stacklevel):
        assert torch_dtype in [torch.bfloat16, torch.float16, torch.float32], (
            f"Invalid precision: {torch_dtype}\nChoose from: torch.bfloat16, torch.float16, torch.float32")
        if torch_dtype == torch.float32 and not self._warned_fp32:
            self._warned_fp32 = True
            warnings.warn("torch_dtype=torch.float32: this MI355X path has no fp32-operand mode; it computes with "
                          f"{self.model.precision} (within 1e-3 relative L2 of the reference's CPU fp32 output)",
                          PrecisionWarning, stacklevel=stacklevel)

    def _texture(self, texture):
        """The texture as the model takes it: the reference's [bs, N, C, p, p], or material rows [bs, N, C] (one
        constant per triangle and channel: what ``pose`` returns); float32 and contiguous either way, since it is
        log-encoded in place."""
        if self.config.texture_encode_patch_size == 1 and texture.dim() == 5:
            texture = texture[:, :, :, 0, 0].contiguous()
        if not texture.is_contiguous():
            raise ValueError("texture must be contiguous (it is log-encoded in place)")
        if texture.dtype != torch.float32:
            raise ValueError("texture must be float32 (it is log-encoded in place)")
        return texture

    def render(self, triangles, texture, mask, vn, c2w, fov, resolution: Union[int, Tuple[int, int]] = 512,
               torch_dtype: torch.dtype = torch.float16, *, intrinsics=None, overscan: bool = False):
        """Render [bs, nv, H, W, 3] HDR images (rendering_pipeline.py:28-125).  ``resolution`` is an int (the
        reference's square frame, H = W = resolution) or ``(height, width)``; each side must be a multiple of the
        patch size (x 8 with Swin attention: 64 for the released models).  ``fov`` is the VERTICAL field of view of
        the full frame height in degrees (for a square frame the reference's own convention); a horizontal field of
        view converts as ``fov_v = 2 atan(tan(fov_h / 2) * H / W)``.

        ``intrinsics``: a pinhole camera instead of ``fov`` (exactly one of the two is given; ``fov`` may be None
        only when ``intrinsics`` is passed).  float32 ``[bs, nv, 4]`` holding ``(fx, fy, cx, cy)`` in pixels of the
        requested H x W frame, origin at the top-left corner, pixel (x, y) centred at (x + 0.5, y + 0.5).  The
        camera-space direction is ``((x + 0.5 - cx) / fx, -(y + 0.5 - cy) / fy, -1)``, rotated by ``c2w`` and
        L2-normalised; the fov convention is the special case ``fx = fy = H / 2 / tan(fov / 2)``, ``cx = W / 2``,
        ``cy = H / 2``.  Focal lengths must be positive (not checked: the values are never read back).

        ``overscan=True`` renders ANY positive H x W (1280 x 720, 1920 x 1080).  With u the frame unit (64 with
        Swin attention, otherwise the patch size) the model renders the padded frame ``H' = ceil(H / u) u``,
        ``W' = ceil(W / u) u`` with the same focal lengths; the requested frame sits at ``y0 = (H' - H) // 2``,
        ``x0 = (W' - W) // 2`` inside it (the padded frame's principal point is ``(cx + x0, cy + y0)``), so the
        border pixels are real rays of a slightly wider view, not padding values, and the call returns only the
        window ``[y0 : y0 + H, x0 : x0 + W]``.  The border costs under u pixels per side (1080 -> 1088 rows, 0.7 %;
        720 -> 768 rows, 6.7 %).  With ``overscan=False`` (the default) a non-multiple side raises; on a frame
        whose sides are multiples of u already ``overscan=True`` issues the same launches and returns the same
        bits."""
        self._check_dtype(torch_dtype, stacklevel=3)
        cfg = self.config
        texture = self._texture(texture)
        out = self.model.render_views(triangles, texture, mask, vn, c2w, fov, resolution, log_encode=not cfg.use_ldr,
                                      intrinsics=intrinsics, overscan=overscan)
        self.last_precision = {"requested": str(torch_dtype), "computed": self.model.precision}
        return out

    def encode(self, triangles, texture, mask, vn):
        """Encode a batch of scenes once (RenderFormer.encode_scene): everything ``render`` computes before it needs
        a camera.  ``texture`` is handled as in ``render`` — log-encoded **in place**, once.  Returns the handle
        ``render_encoded`` takes; it holds ``nbytes`` of device memory and the input tensors."""
        return self.model.encode_scene(triangles, self._texture(texture), mask, vn,
                                       log_encode=not self.config.use_ldr)

    def render_encoded(self, scene, c2w, fov, resolution: Union[int, Tuple[int, int]] = 512,
                       torch_dtype: torch.dtype = torch.float16, *, intrinsics=None, overscan: bool = False):
        """Render the cameras ``c2w`` [bs, nv, 4, 4] / ``fov`` of an encoded batch: [bs, nv, H, W, 3] HDR
        (``resolution``: an int or ``(height, width)``; ``intrinsics`` [bs, nv, 4] with ``fov=None``, and
        ``overscan``, as in ``render``), bit-identical to ``render`` of the same
        scene and cameras, without stage 1 and the K/V projection.  One handle renders any frame size."""
        self._check_dtype(torch_dtype, stacklevel=3)
        out = self.model.render_encoded(scene, c2w, fov, resolution, intrinsics=intrinsics, overscan=overscan)
        self.last_precision = {"requested": str(torch_dtype), "computed": self.model.precision}
        return out

    def pose(self, rig, transforms, materials=None, *, out=None):
        """Pose a rest-pose ``SceneRig`` (renderformer_amd.rig) for one frame, on the device: one HIP launch
        (``ops.pose_scene``), no model weights.  Returns ``PosedScene(triangles, texture, mask, vn)``, which unpacks
        into ``encode``, ``render`` and ``gbuffer``; its ``texture`` is the compact [B, N, C] form (one constant per
        triangle and channel: no [B, N, C, 32, 32] tensor is made), NOT yet log-encoded -- ``render`` / ``encode``
        do that in place, once, as for any texture, so pose again (or pass ``out=``) for the next frame.

        ``transforms``: float32 [B, K, 3, 4] or [B, K, 4, 4] (the last row is ignored), contiguous, on the rig's
        device: ``[A | t]`` per object, ``rig.transforms0`` being the config's own (``rig.trs`` builds one).
        ``materials``: float32 [B, M, C] like ``rig.materials0`` (None: ``rig.materials0``).  ``out``: a previous
        ``PosedScene`` of this rig whose buffers are written again.  Anything else raises ValueError.

        Vertices go to ``A p + t``, normals to the normalised ``sign(det A) cof(A) n`` (right under non-uniform scale
        and mirrors, zero for a zero normal, never NaN), padding rows pass through with a zero material row.  A rig
        posed with its own ``transforms0`` / ``materials0`` reproduces the scene converter for every object that is
        flat-shaded or uniformly scaled; for a smooth-shaded object under NON-uniform scale the converter measures
        its 30-degree smoothing groups and angle weights after the transform, so its normals differ from the
        geometrically transformed rest normals a rig gives."""
        from . import ops
        from .rig import PosedScene, SceneRig
        if not isinstance(rig, SceneRig):
            raise ValueError(f"pose needs a SceneRig, got {type(rig)}")
        dev = rig.device
        if dev.type != "cuda":
            raise ValueError("pose: the rig must be on the HIP device (rig.to('cuda')); renderformer_amd.rig.pose_numpy is the CPU form")
        B, K = rig.batch_size, len(rig.names)
        if materials is None:
            materials = rig.materials0
        for t, n, shapes in ((transforms, "transforms", ((B, K, 3, 4), (B, K, 4, 4))),
                             (materials, "materials", (tuple(rig.materials0.shape),))):
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise ValueError(f"pose: {n} must be a tensor on the rig's device {dev}")
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) not in shapes:
                raise ValueError(f"pose: {n} must be contiguous float32 {' or '.join(map(str, shapes))}, got "
                                 f"{t.dtype} {tuple(t.shape)}" + ("" if t.is_contiguous() else " (not contiguous)"))
        bufs = None
        if out is not None:
            if not isinstance(out, PosedScene):
                raise ValueError(f"pose: out must be a PosedScene of this rig, got {type(out)}")
            bufs = (out.triangles, out.vn, out.texture)
        with torch.cuda.device(dev):
            tris, vn, tex = ops.pose_scene(rig.triangles, rig.vn, rig.object_id, rig.material_id, transforms,
                                           materials, out=bufs)
        return PosedScene(tris, tex, rig.mask, vn)

    def to_ldr(self, hdr: torch.Tensor, tone_mapper: str = "none", exposure: float = 0.0, out: torch.Tensor = None):
        """The 8-bit display frame of rendered HDR frames, made on the device (one HIP kernel, ``ops.tonemap_ldr8``):
        ``hdr`` [bs, nv, H, W, 3] (or any contiguous [..., 3]) float32 on the device -> ``torch.uint8`` of the same
        shape on the same device, a quarter of the bytes to copy to the host.  ``hdr`` is only read.

        ``tone_mapper`` takes the reference CLI's names: ``"none"`` clips to [0, 1] (what the reference's
        ``infer.py`` writes without a tone mapper: no transfer function); ``"pbr_neutral"`` is Khronos PBR Neutral,
        written from the Khronos definition, followed by the sRGB encode.  ``"agx"`` and ``"filmic"`` are LUT
        transforms of ``simple_ocio``'s OCIO configuration, whose data is not available: ValueError.  ``exposure``
        (stops) scales the frame by ``2 ** exposure`` first.  Then ``* 255`` and truncation, like numpy's
        ``(x * 255).astype(uint8)``; NaN and negative values give 0, +inf gives 255.  ``out``: a uint8 tensor of
        hdr's shape to reuse.  ``images.hdr_to_ldr`` is the same arithmetic in numpy.

        With ``range_check="lazy"`` call ``to_ldr`` AFTER ``resolve(out)``: ``resolve`` may render the HDR frame
        again in place, and a display frame made before it would show the overflowed one.  The default ``"sync"``
        mode has resolved the frame when ``render`` returns, so there is no such order."""
        from . import ops
        from .images import check_tone_mapper
        check_tone_mapper(tone_mapper)
        if not isinstance(hdr, torch.Tensor) or not hdr.is_cuda:
            raise ValueError("to_ldr: hdr must be a tensor on the HIP device (images.hdr_to_ldr is the numpy form)")
        with torch.cuda.device(hdr.device):
            return ops.tonemap_ldr8(hdr, tone_mapper, exposure, out=out)

    def _unit(self) -> int:
        """The smallest frame side a plan takes: the valid-triangle tables do not depend on views or resolution."""
        from .model import SWIN_WINDOW
        return self.config.patch_size * (SWIN_WINDOW if self.config.view_transformer_use_swin_attn else 1)

    def gbuffer(self, triangles, texture, mask, vn, c2w, fov, resolution: Union[int, Tuple[int, int]] = 512, *,
                intrinsics=None, overscan: bool = False, outputs=None):
        """Geometry buffers of the frames ``render`` would render from the same arguments: a ``GBuffer`` (``alpha``
        uint8, ``depth`` float32, ``tri_id`` int32, each [bs, nv, H, W]; ``normal`` and ``albedo`` float32 [bs, nv,
        H, W, 3]) on the device, from one brute-force visibility pass over the primary rays and the input triangles
        (``renderformer_amd.gbuffer``: two HIP kernels, no model weights).

        Same argument order, camera conventions (``fov`` or ``intrinsics``) and acceptance rule as ``render``: a
        call is valid iff the same ``render`` call is, so a side that is no multiple of the frame unit needs
        ``overscan=True``.  That flag only relaxes the check here: a G-buffer pixel (x, y) is the ray of pixel
        (x, y) of the requested frame, which is the ray ``render`` traces for it with or without overscan, so the
        padded frame is never needed.

        ``depth`` is the distance along the normalised ray, +inf where nothing is hit (z-depth: ``t / |d_cam|``);
        ``tri_id`` indexes the N axis of ``triangles[b]`` (-1: no hit); ``normal`` is the world-space shading normal
        interpolated from ``vn``, not flipped toward the camera; ``albedo`` is the diffuse colour of the hit
        triangle, texel (0, 0) of channels 0..2 of its texture (textures that vary over a triangle's patch are not
        sampled).  Composite over a backplate with ``rgb * a + backplate * (1 - a)``, ``a = alpha / 255``.

        ``texture`` is only READ here -- unlike ``render`` it is NOT log-encoded in place; the diffuse channels are
        not among the log-encoded ones, so a texture gives the same albedo before and after a ``render``.
        ``outputs``: a subset of ``("alpha", "depth", "tri_id", "normal", "albedo")`` (None = all); a buffer that is
        not asked for is not computed (its field is None)."""
        from . import gbuffer as gb
        from .model import _check_camera, frame_layout
        H, W = frame_layout(self.config, resolution, overscan)[:2]
        _check_camera(c2w, fov, intrinsics)
        names = gb.check_outputs(outputs)
        cam = fov if intrinsics is None else intrinsics
        for t, n in ((triangles, "triangles"), (texture, "texture"), (mask, "mask"), (vn, "vn"), (c2w, "c2w"),
                     (cam, "fov" if intrinsics is None else "intrinsics")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"gbuffer: {n} must be a tensor on the HIP device")
        dev = c2w.device
        with torch.cuda.device(dev):
            if self.model._w is not None and self.model.device == dev:
                plan = self.model._plan(mask, 1, self._unit())  # (cached per mask: no read-back the next time)
                tables = (plan.valid_flat, plan.scene_off, plan.T_tri)
            else:
                tables = gb.scene_tables(mask.cpu().numpy(), dev)
            return gb.trace(triangles, texture, vn, tables, c2w, fov, intrinsics, (H, W), names)

    def gbuffer_encoded(self, scene, c2w, fov, resolution: Union[int, Tuple[int, int]] = 512, *, intrinsics=None,
                        overscan: bool = False, outputs=None):
        """``gbuffer`` of the cameras ``c2w`` / ``fov`` (or ``intrinsics``) for an encoded batch, from the inputs the
        handle retains (their texture is log-encoded by ``encode``, which leaves the diffuse channels as they
        were): the same buffers, bit for bit, as ``gbuffer`` of the scene's inputs."""
        from . import gbuffer as gb
        from .model import EncodedScene, _check_camera, frame_layout
        H, W = frame_layout(self.config, resolution, overscan)[:2]
        _check_camera(c2w, fov, intrinsics)
        names = gb.check_outputs(outputs)
        if not isinstance(scene, EncodedScene):
            raise ValueError(f"gbuffer_encoded needs an EncodedScene (pipeline.encode), got {type(scene)}")
        cam = fov if intrinsics is None else intrinsics
        for t, n in ((c2w, "c2w"), (cam, "fov" if intrinsics is None else "intrinsics")):
            if not isinstance(t, torch.Tensor) or t.device != scene.device:
                raise ValueError(f"gbuffer_encoded: {n} must be a tensor on {scene.device}")
        if c2w.shape[0] != scene.batch_size:
            raise ValueError(f"c2w has batch size {c2w.shape[0]}, the encoded scene {scene.batch_size}")
        triangles, texture, _, vn = scene.inputs
        with torch.cuda.device(scene.device):
            plan = scene.model._plan_host(scene.mask_host, 1, self._unit())  # (the plan encode built)
            return gb.trace(triangles, texture, vn, (plan.valid_flat, plan.scene_off, plan.T_tri), c2w, fov,
                            intrinsics, (H, W), names)

    def resolve(self, out=None) -> bool:
        """RenderFormer.resolve: finish the fp16 range check of the frame ``out`` (every pending frame if None),
        waiting for it; an overflowed frame is rendered again in place.  Only needed with range_check="lazy" (the
        default "sync" render has resolved its frame already; then this only reports whether it was re-rendered)."""
        redo = self.model.resolve(out)
        if self.last_precision is not None:
            self.last_precision["computed"] = self.model.precision
        return redo

    def check_range(self):
        """RenderFormer.check_range: resolve every pending frame (deferred mode: raise DeviceError if one
        overflowed; lazy: re-render it in place)."""
        try:
            self.model.check_range()
        finally:
            if self.last_precision is not None:
                self.last_precision["computed"] = self.model.precision

    def __call__(self, *args, **kwargs):
        return self.render(*args, **kwargs)
