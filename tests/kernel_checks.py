"""Shared helpers of the exact-arithmetic and guard-band kernel tests (not a conftest: imported by name).

Three tools, all plain torch and usable on any device:

  Guarded              a 2-D view inside a larger allocation pre-filled with a sentinel (a quiet NaN with a payload
                       for floating types), so a store outside the view, or a load from outside it that reaches an
                       output, is seen;
  assert_elementwise   |out - ref| <= bound for EVERY element (a whole-tensor L2 norm hides a wrong row);
  dot_bound & co.      forward-error bounds of an fp32-accumulated dot product, derived from the number formats;

plus builders of inputs on which the kernels' arithmetic is exact (integer GEMM operands, attention whose weights
are powers of two, one-hot V that names every key), and plain torch emulations of the kernels with switches that
plant the defects the GPU tests are there to catch (tests/test_kernel_checks.py proves each one is flagged).

The last section is the same for the DPT convolutions: integer and tap-mask operands (the tap mask names, per output
element, the taps that fell inside the image), conv_bound, conv_emulation, and ConvLaunch, which calls the C entry
points with pointers into Guarded buffers.

The section after it serves the prologue and output kernels (prologue.hip): fp64 references of the vertex-normal
encoding, the RoPE positions and register centres, the HDR decode, the texture Linear and the ray tokens, a bound
beside each, LIBM_ULPS (the one assumed figure: the device math library's accuracy) and fp32 emulations with planted
defects.
"""
import math

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------ sentinels
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# quiet NaNs (exponent all ones, top mantissa bit set) with a recognisable payload
_FLOAT_SENTINEL = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FED, torch.float16: 0x7EED,
                   torch.float64: 0x7FF80000DEADBEEF}


def sentinel_bits(dtype: torch.dtype) -> int:
    """The sentinel of `dtype` as the (signed, except for bytes) integer its same-sized integer view holds."""
    size = torch.empty((), dtype=dtype).element_size()
    if dtype in _FLOAT_SENTINEL:
        return _FLOAT_SENTINEL[dtype]  # (all below the sign bit: positive in the signed view)
    bits = int.from_bytes(b"\xA5" * size, "little")  # integer types: the byte 0xA5 repeated
    return bits if size == 1 or bits < (1 << (8 * size - 1)) else bits - (1 << (8 * size))


class Guarded:
    """A logical [rows, cols] tensor of `dtype` inside one larger allocation.

    The allocation is [g + rows + g, ld] with ld > cols (ld == cols for a buffer an op needs dense: guard rows only);
    the view starts `col_off` columns into a row, so there
    are g guard rows before and after it and ld - cols padding columns around every row.  Everything is pre-filled
    with the sentinel.  `.view` is the strided tensor to hand to an op.  For an output, assert_untouched() proves
    the op wrote nothing outside the view; for an input, fill() the view and the NaN surround proves that nothing
    outside it reaches an output (outputs stay finite)."""

    def __init__(self, rows: int, cols: int, dtype: torch.dtype, device="cpu", g: int = 2, pad: int = 8,
                 col_off: int = 0, ld: int = None):
        self.rows, self.cols, self.g, self.col_off, self.dtype = rows, cols, g, col_off, dtype
        self.ld = ld if ld is not None else col_off + cols + pad
        assert self.ld >= cols and col_off + cols <= self.ld and g >= 1
        self.buf = torch.empty(rows + 2 * g, self.ld, dtype=dtype, device=device)
        self.ibuf = self.buf.view(_INT_VIEW[self.buf.element_size()])
        self.sentinel = sentinel_bits(dtype)
        self.ibuf.fill_(self.sentinel)
        self.view = self.buf[g:g + rows, col_off:col_off + cols]
        assert self.view.stride(0) == self.ld and self.view.stride(1) == 1

    def fill(self, data: torch.Tensor) -> "Guarded":
        self.view.copy_(data.to(self.dtype))
        return self

    def reset(self) -> "Guarded":
        """The whole allocation back to the sentinel, the view included (an output about to be written again)."""
        self.ibuf.fill_(self.sentinel)
        return self

    def outside(self) -> torch.Tensor:
        """bool [g + rows + g, ld]: the elements that are not part of the view."""
        m = torch.ones(self.ibuf.shape, dtype=torch.bool, device=self.buf.device)
        m[self.g:self.g + self.rows, self.col_off:self.col_off + self.cols] = False
        return m

    def assert_untouched(self, written_rows: torch.Tensor = None, what: str = "") -> None:
        """Every element outside the view still holds the sentinel, bit for bit.  written_rows (bool [rows]):
        only these rows of the view may have been written; the others must hold the sentinel too (gap rows between
        attention problems, holes of a scatter).  Reports the first offender in view coordinates."""
        must = self.outside()
        if written_rows is not None:
            keep = ~written_rows.to(self.buf.device).bool()
            must[self.g:self.g + self.rows][keep] = True
        bad = must & (self.ibuf != self.sentinel)
        n = int(bad.sum())
        if n:
            r, c = (int(v) for v in bad.nonzero()[0])
            raise AssertionError(
                f"{what}: {n} element(s) outside the written region changed; first at (row {r - self.g}, col "
                f"{c - self.col_off}) of the [{self.rows}, {self.cols}] view (guard rows {self.g}, ld {self.ld}, "
                f"col_off {self.col_off}): bits {int(self.ibuf[r, c]) & ((1 << 8 * self.buf.element_size()) - 1):#x}")


def assert_finite(t: torch.Tensor, what: str = "") -> None:
    bad = ~torch.isfinite(t)
    n = int(bad.sum())
    if n:
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} non-finite output element(s), first at {idx}: something outside the "
                             f"inputs' views was read")


def assert_elementwise(out: torch.Tensor, ref: torch.Tensor, bound, what: str = "") -> float:
    """|out - ref| <= bound for every element (bound: tensor or scalar; fp64 arithmetic; NaN / inf in out fail).
    Returns the worst |out - ref| / bound over the elements with a non-zero bound (for reporting)."""
    o, r = out.detach().double().cpu(), ref.detach().double().cpu()
    assert o.shape == r.shape, (what, tuple(o.shape), tuple(r.shape))
    b = torch.as_tensor(bound, dtype=torch.float64).cpu().expand_as(r)
    err = (o - r).abs()
    bad = ~(err <= b)  # (NaN compares false: flagged)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    n = int(bad.sum())
    if n:
        score = torch.where(bad, torch.where(b > 0, ratio, torch.full_like(err, float("inf"))), torch.zeros_like(err))
        flat = int(score.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), r.shape))
        raise AssertionError(
            f"{what}: {n} of {r.numel()} elements beyond their bound; worst at {idx}: out {float(o[idx])!r}, ref "
            f"{float(r[idx])!r}, |diff| {float(err[idx]):.4g}, bound {float(b[idx]):.4g}, ratio "
            f"{float(err[idx] / b[idx]) if float(b[idx]) > 0 else float('inf'):.3g}")
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ error bounds
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # RNE unit roundoffs
F32_ULP = 2.0 ** -23  # one full fp32 ulp per operation: covers an accumulator that truncates instead of rounding


def out_rounding(ref_abs: torch.Tensor, e: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """Error of rounding a value within e of ref to out_dtype: u_out (|ref| + e), plus half the subnormal spacing
    2^-24 of fp16 (2^-25) where the value is below fp16's normal range."""
    r = U_OUT[out_dtype] * (ref_abs + e)
    return r + 2.0 ** -25 if out_dtype == torch.float16 else r


def acc_bound(a: torch.Tensor, w: torch.Tensor, bias, k: int) -> torch.Tensor:
    """e_acc of a K-term dot product accumulated in fp32 in any order, bias added: every one of the K - 1 adds, the
    bias add and one extra operation perturb the running sum by at most one fp32 ulp of a partial sum, and every
    partial sum is at most sum |a_i| |w_i| + |bias|: (k + 1) 2^-23 (|a| |w|^T + |bias|), the products being exact
    (16-bit operands: 22-bit products)."""
    mag = a.double().abs() @ w.double().abs().t()
    if bias is not None:
        mag = mag + bias.double().abs()
    return (k + 1) * F32_ULP * mag


def dot_bound(a, w, bias, k: int, out_dtype: torch.dtype) -> torch.Tensor:
    """Per-element bound on |C - (a w^T + bias)| for C written as out_dtype from an fp32 accumulator."""
    ref = a.double() @ w.double().t()
    if bias is not None:
        ref = ref + bias.double()
    e = acc_bound(a, w, bias, k)
    return e + out_rounding(ref.abs(), e, out_dtype)


def swiglu_ref(a, w1, w3) -> torch.Tensor:
    return F.silu(a.double() @ w1.double().t()) * (a.double() @ w3.double().t())


def swiglu_bound(a, w1, w3, k: int, out_dtype: torch.dtype, e_g=None, e_u=None, g=None, u=None) -> torch.Tensor:
    """Bound for silu(g) u with g = a w1^T, u = a w3^T both within e_g / e_u (default: acc_bound) of exact:
    |silu'| <= 1.1, so silu moves by at most 1.1 e_g; the product of the two perturbed factors differs from s u by
    at most 1.1 e_g |u| + |s| e_u + 1.1 e_g e_u; the fast exponential / reciprocal of silu and the final multiply
    are covered by 2^-20 |ref| (8 fp32 ulps); then the output rounding."""
    g = a.double() @ w1.double().t() if g is None else g
    u = a.double() @ w3.double().t() if u is None else u
    e_g = acc_bound(a, w1, None, k) if e_g is None else e_g
    e_u = acc_bound(a, w3, None, k) if e_u is None else e_u
    s = F.silu(g)
    ref = s * u
    e = 1.1 * e_g * u.abs() + s.abs() * e_u + 1.1 * e_g * e_u + 2.0 ** -20 * ref.abs()
    return e + out_rounding(ref.abs(), e, out_dtype)


# 1 / rms(x) of the deferred RMSNorm as the GEMM epilogue computes it in fp32 from 8 slot sums: 7 adds, a divide, the
# eps add, sqrtf, a reciprocal and the multiply with the accumulator: 12 operations of at most one fp32 ulp each
# (the sqrt and the reciprocal may be the 1-ulp hardware approximations).  Relative to the exact 1 / rms:
ROWSCALE_REL = 12 * F32_ULP


def interleave_swiglu(w1: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """W rows in RF_EPI_SWIGLU order (rf.h): 16-row groups [w1[16 g : 16 g + 16]; w3[16 g : 16 g + 16]]."""
    f, k = w1.shape
    return torch.stack([w1.view(f // 16, 16, k), w3.view(f // 16, 16, k)], dim=1).reshape(2 * f, k)


# ------------------------------------------------------------------------------------------------ exact inputs
def int_gemm_operands(m: int, n: int, k: int, dtype: torch.dtype, seed: int = 0, amax: int = 3, bmax: int = 8):
    """Integer-valued A [m, k], W [n, k] in [-amax, amax] (exact in bf16 and fp16) and an integer fp32 bias in
    [-bmax, bmax].  Every partial sum of a dot product is an integer of magnitude <= amax^2 k + bmax, which must
    stay below 2^24 so fp32 holds it exactly: the product then does not depend on the accumulation order."""
    assert amax * amax * k + bmax < 2 ** 24
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randint(-amax, amax + 1, (m, k), generator=g).to(dtype)
    w = torch.randint(-amax, amax + 1, (n, k), generator=g).to(dtype)
    bias = torch.randint(-bmax, bmax + 1, (n,), generator=g).float()
    return a, w, bias


def onehot_v(rows: int, n_heads: int, coarse: bool = False, dtype=torch.bfloat16) -> torch.Tensor:
    """V [rows, n_heads * 128] naming its row: row j sets, in head h, channel (j + 17 h) % 128 (fine code) or
    (j // 128) % 128 (coarse code); the two codes together identify any key of a sequence of up to 16,384 rows.
    Rows are numbered over the whole buffer, so the neighbours of every problem carry their own code too."""
    j = torch.arange(rows)
    v = torch.zeros(rows, n_heads, 128)
    for h in range(n_heads):
        ch = ((j // 128) % 128) if coarse else ((j + 17 * h) % 128)
        v[j, h, ch] = 1.0
    return v.view(rows, n_heads * 128).to(dtype)


def exponent_keys(k_len: int, seed: int = 0, span: int = 12, spikes=()):
    """Integer exp2 exponents e_j in [-span, 0] for the exact-exponent attention form: a low plateau in
    [-span, -span + 3] with late steps up.  spikes: (position, exponent) pairs placed on top (positions >= k_len are
    dropped), e.g. just after a piece boundary, a step of at most 8 above the plateau (the rescale is deferred) or
    above 8 (it happens)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    e = -span + torch.randint(0, 4, (k_len,), generator=g)
    for pos, val in spikes:
        if 0 <= pos < k_len:
            e[pos] = val
    return e


def exact_exponent_qk(q_rows: int, k_rows: int, n_heads: int, e: torch.Tensor, dtype=torch.bfloat16):
    """q with a single 1 in channel 0 of each head, k with e[j] in channel 0 of each head of row j: with
    q_prescaled=True every score is the integer e[j] and every softmax weight a power of two."""
    d = n_heads * 128
    q = torch.zeros(q_rows, d)
    q[:, ::128] = 1.0
    k = torch.zeros(k_rows, d)
    k[:, ::128] = e.double().float()[:, None]
    return q.to(dtype), k.to(dtype)


def weighted_onehot_expected(v: torch.Tensor, e, out_dtype: torch.dtype):
    """O and its bound for attention over keys whose weights are exactly 2^e[j] (e None: all equal, the counting
    form) and one-hot V [k_len, D]: channel c = sum of the weights of the keys coded c / sum of all weights.  Numerator
    and denominator are exact in fp32 (k_len <= 1000 terms spanning 12 binades: 22 bits), so the only errors are the
    division (or reciprocal and multiply: 2^-18 covers 32 fp32 ulps) and the output rounding: (u_out + 2^-18)
    expected, which is exactly 0 where no key carries the channel."""
    w = torch.ones(v.shape[0], dtype=torch.float64) if e is None else torch.exp2(e.double())
    exp = (w[:, None] * v.double()).sum(0) / w.sum()
    # (the relative output rounding needs a normal number: the inputs keep every non-zero channel above fp16's 2^-14)
    assert not bool(((exp > 0) & (exp < 2.0 ** -14)).any()), "a channel below fp16's normal range"
    bound = (U_OUT[out_dtype] + 2.0 ** -18) * exp
    return exp, bound


# ------------------------------------------------------------------------------------------------ emulations
def gemm_emulation(a, w, bias, out_dtype, drop_slice=None, scale_row=None, chunk: int = 32):
    """C = a w^T + bias accumulated in fp32 in 32-wide K slices (the kernels' MFMA depth), rounded once to out_dtype.
    Planted defects: drop_slice = (row, slice) loses one 32-wide K slice of one row; scale_row = (row, factor)
    scales one row of the accumulator."""
    m, k = a.shape
    acc = torch.zeros(m, w.shape[0], dtype=torch.float32)
    for s in range(0, k, chunk):
        part = a[:, s:s + chunk].float() @ w[:, s:s + chunk].float().t()
        if drop_slice is not None and drop_slice[1] == s // chunk:
            part[drop_slice[0]] = 0.0
        acc += part
    if bias is not None:
        acc += bias.float()
    if scale_row is not None:
        acc[scale_row[0]] *= scale_row[1]
    return acc.to(out_dtype)


def attention_emulation(q, k, v, n_heads: int, p_dtype, out_dtype, log2_scores: bool = False, dup=None, drop=None,
                        mask=None):
    """One attention problem in fp64 with the two roundings of the kernels: P rounded to the operand type before
    P V (the row sum from the unrounded P, as the kernels' fp32 softmax keeps it), O rounded to the output type.
    log2_scores: the scores are exp2 exponents (q_prescaled).  Planted defects: dup = (row, key) counts that key
    twice for that query row (every head); drop = (row, key) leaves it out.  mask: bool [lq, lk], True = attend."""
    lq, lk = q.shape[0], k.shape[0]
    qh = q.double().view(lq, n_heads, 128).transpose(0, 1)
    kh = k.double().view(lk, n_heads, 128).transpose(0, 1)
    vh = v.double().view(lk, n_heads, 128).transpose(0, 1)
    s = qh @ kh.transpose(1, 2)
    s = s if log2_scores else s / math.sqrt(128) / math.log(2.0)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    if dup is not None:
        p[:, dup[0], dup[1]] *= 2.0
    if drop is not None:
        p[:, drop[0], drop[1]] = 0.0
    pr = p.to(p_dtype).double() if p_dtype is not None else p
    o = (pr @ vh) / p.sum(-1, keepdim=True)
    o = o.transpose(0, 1).reshape(lq, n_heads * 128)
    return o.to(out_dtype) if out_dtype is not None else o


def attention_ref(q, k, v, n_heads: int, log2_scores: bool = False) -> torch.Tensor:
    """fp64 attention, no rounding."""
    return attention_emulation(q, k, v, n_heads, None, None, log2_scores)


def worst_row_relerr(out: torch.Tensor, ref: torch.Tensor) -> float:
    """max over rows of ||out_r - ref_r|| / ||ref_r|| (fp64)."""
    o, r = out.double().cpu(), ref.double().cpu()
    return float(((o - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-300)).max())


def swin_attend(grid_h: int, grid_w: int, window: int, shift: int) -> torch.Tensor:
    """bool [T, T] over the tokens t = y * grid_w + x of one grid: attend[i, j] iff shifted-window attention lets query
    i see key j.  The bookkeeping is the oracle's: the token ids are rolled by -shift and partitioned into windows as
    rf_ref.swin_attn does with the activations, and inside a window rf_ref.swin_mask decides (no mask at shift 0)."""
    from oracle import rf_ref
    ws, t = window, grid_h * grid_w
    idx = torch.arange(t).view(grid_h, grid_w)
    if shift:
        idx = torch.roll(idx, shifts=(-shift, -shift), dims=(0, 1))
    win = idx.view(grid_h // ws, ws, grid_w // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    mask = rf_ref.swin_mask(grid_h, grid_w, ws, shift) if shift else torch.ones(win.shape[0], ws * ws, ws * ws,
                                                                                dtype=torch.bool)
    att = torch.zeros(t, t, dtype=torch.bool)
    for i in range(win.shape[0]):
        att[win[i][:, None], win[i][None, :]] = mask[i]
    return att


# ------------------------------------------------------------------------------------------------ convolutions
# Everything below serves the DPT convolution kernels (rf_conv2d_* / rf_deconv2d_* / the grouped launches): operands
# on which the arithmetic is exact, the per-element bound for the others, a torch emulation that plants the defects
# the GPU tests are there to catch, and a launcher that hands the C entry points pointers into Guarded buffers.
def conv_ref(x, w, bias=None, res1=None, res2=None, stride: int = 1, pad: int = 0, deconv: int = 0) -> torch.Tensor:
    """fp64 NHWC [n, ho, wo, cout] of x [n, cin, h, w] with w [cout, cin, kh, kw] (deconv = k: ConvTranspose2d weights
    [cin, cout, k, k], kernel == stride == k); bias [cout] or, border-class rows, [9, cout]; residuals NHWC."""
    x, w = x.double(), w.double()
    b = bias.double() if bias is not None and bias.dim() == 1 else None
    y = F.conv_transpose2d(x, w, b, stride=deconv) if deconv else F.conv2d(x, w, b, stride=stride, padding=pad)
    y = y.permute(0, 2, 3, 1)
    if bias is not None and bias.dim() == 2:
        y = y + bias.double()[border_classes(y.shape[1], y.shape[2])]
    for r in (res1, res2):
        if r is not None:
            y = y + r.double()
    return y.contiguous()


def border_classes(h: int, w: int) -> torch.Tensor:
    """long [h, w]: the RF_CONV_BORDER_BIAS class 3 ry + rx of each pixel (rf.h: 0 first, 2 last, 1 elsewhere)."""
    ry, rx = torch.ones(h, dtype=torch.long), torch.ones(w, dtype=torch.long)
    ry[0], ry[-1], rx[0], rx[-1] = 0, 2, 0, 2
    return 3 * ry[:, None] + rx[None, :]


def int_conv_operands(n: int, cin: int, cout: int, kh: int, kw: int, h: int, w: int, seed: int = 0, amax: int = 3,
                      bmax: int = 8, stride: int = 1, pad: int = 0, deconv: int = 0):
    """Integer-valued x [n, cin, h, w], W ([cout, cin, kh, kw]; deconv = k: [cin, cout, k, k]) in [-amax, amax], an
    integer bias [cout] and two integer residuals NHWC of the output's shape in [-bmax, bmax].  Every partial sum is an
    integer below amax^2 kh kw cin + 3 bmax < 2^24, so fp32 holds it exactly in any order and over any stream-K split:
    with fp16 operands, and with bf16x3 ones, whose lo planes are then zero."""
    assert amax * amax * kh * kw * cin + 3 * bmax < 2 ** 24 and amax <= 256
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randint(-amax, amax + 1, (n, cin, h, w), generator=g).float()
    if deconv:
        wt = torch.randint(-amax, amax + 1, (cin, cout, deconv, deconv), generator=g).float()
        ho, wo = h * deconv, w * deconv
    else:
        wt = torch.randint(-amax, amax + 1, (cout, cin, kh, kw), generator=g).float()
        ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    bias = torch.randint(-bmax, bmax + 1, (cout,), generator=g).float()
    res1 = torch.randint(-bmax, bmax + 1, (n, ho, wo, cout), generator=g).float()
    res2 = torch.randint(-bmax, bmax + 1, (n, ho, wo, cout), generator=g).float()
    return x, wt, bias, res1, res2


def exact_planes(ref: torch.Tensor, f16: bool):
    """The planes of an exact value: rounded once.  fp16: (fp16(v), None); bf16x3: hi = bf16(v), lo = bf16(v - hi)."""
    if f16:
        return ref.to(torch.float16), None
    hi = ref.to(torch.bfloat16)
    return hi, (ref - hi.double()).to(torch.bfloat16)


def tap_mask_operands(n: int, cin: int, cout: int, kh: int, kw: int, h: int, w: int, deconv: int = 0):
    """x = 1 in every channel; W[co, co % cin, ty, tx] = 2^(kw ty + tx), 0 elsewhere; no bias.  Each output element is
    then the bit mask of the taps that fell inside its image (3x3 pad 1: 511 inside, the 8 border patterns on the
    border).  A deconvolution (W[co % cin, co, dy, dx] = 2^(k dy + dx)) names the position in the k x k block it
    scatters to.  b9: the integer border-class rows 1024 (class + 1) for RF_CONV_BORDER_BIAS."""
    x = torch.ones(n, cin, h, w)
    co = torch.arange(cout)
    if deconv:
        wt = torch.zeros(cin, cout, deconv, deconv)
        wt[co % cin, co] = (2.0 ** torch.arange(deconv * deconv)).view(deconv, deconv)
    else:
        wt = torch.zeros(cout, cin, kh, kw)
        wt[co, co % cin] = (2.0 ** torch.arange(kh * kw)).view(kh, kw)
    b9 = (1024.0 * (torch.arange(9) + 1))[:, None].expand(9, cout).contiguous()
    return x, wt, b9


def decode_tap_mask(expected: float, observed: float, kh: int, kw: int, border: bool = False) -> str:
    """What an observed tap-mask element says against the expected one, in words."""
    if not (math.isfinite(observed) and observed == int(observed)):
        return f"value {observed!r} is no integer (expected mask {int(expected)})"
    e, o, parts = int(expected), int(observed), []
    if border:
        ce, co_ = e // 1024 - 1, (o - o % 1024) // 1024 - 1
        if ce != co_:
            parts.append(f"border class {co_} instead of {ce}")
        e, o = e % 1024, o % 1024
    d = o - e
    if d and abs(d) & (abs(d) - 1) == 0 and abs(d) < 2 ** (kh * kw):  # one tap once too often / too seldom
        t = abs(d).bit_length() - 1
        had = (e >> t) & 1
        parts.append(f"tap ({t // kw}, {t % kw}) counted {had + (1 if d > 0 else -1)} times, expected {had}")
    elif d:
        for t in range(kh * kw):
            if (e >> t) & 1 != (o >> t) & 1:
                parts.append(f"tap ({t // kw}, {t % kw}) " + ("missing" if (e >> t) & 1 else "counted from the padding"))
        if o >> (kh * kw):
            parts.append(f"sum {o} beyond the full mask {2 ** (kh * kw) - 1}")
    return "; ".join(parts) or "equal"


def assert_tap_mask(out: torch.Tensor, ref: torch.Tensor, kh: int, kw: int, border: bool = False, what: str = ""):
    """out == ref bit for bit ([n, ho, wo, cout]); the first offender decoded."""
    o, r = out.detach().double().cpu(), ref.detach().double().cpu()
    assert o.shape == r.shape, (what, tuple(o.shape), tuple(r.shape))
    bad = ~(o == r)
    cnt = int(bad.sum())
    if cnt:
        i, y, x, f = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {cnt} of {r.numel()} elements differ; image {i}, pixel ({y}, {x}), filter {f}: "
                             + decode_tap_mask(float(r[i, y, x, f]), float(o[i, y, x, f]), kh, kw, border))


def conv_bound(x, w, bias, res1, res2, k_terms: int, out_dtype: torch.dtype, silu: bool = False, stride: int = 1,
               pad: int = 0, deconv: int = 0, ref: torch.Tensor = None, operand_rel: float = 0.0) -> torch.Tensor:
    """Per-element bound on |out - ref| for v = conv(x, w) + bias + res1 + res2 accumulated in fp32 in any order and
    written as out_dtype (of silu(v) with `silu`).  acc_bound's argument: each of the k_terms - 1 adds of the dot
    product and the three epilogue adds perturbs a partial sum by at most one fp32 ulp, and every partial sum is at
    most mag = |x| * |w| + |bias| + |res1| + |res2|: e = (k_terms + 3) 2^-23 mag, the products being exact.
    operand_rel: what the products themselves omit, relative to |x| * |w| (bf16x3 leaves out lo * lo: 2^-16).
    silu: swiglu_bound's silu step, 1.1 e + 2^-20 |silu(ref)| (|silu'| <= 1.1; the fast exponential and reciprocal
    within 8 fp32 ulps).  Then out_rounding."""
    prod = conv_ref(x.abs(), w.abs(), None, None, None, stride, pad, deconv)
    mag = conv_ref(x.abs(), w.abs(), None if bias is None else bias.abs(), None if res1 is None else res1.abs(),
                   None if res2 is None else res2.abs(), stride, pad, deconv)
    e = (k_terms + 3) * F32_ULP * mag + operand_rel * prod
    if ref is None:
        ref = conv_ref(x, w, bias, res1, res2, stride, pad, deconv)
    if silu:
        ref = F.silu(ref)
        e = 1.1 * e + 2.0 ** -20 * ref.abs()
    return e + out_rounding(ref.abs(), e, out_dtype)


def conv_emulation(x, w, bias=None, res1=None, res2=None, pad: int = 1, drop_chunk=None, halo_col_zero=None,
                   prev_image_row=None, wrong_class=None, chunk: int = 32) -> torch.Tensor:
    """A stride-1 convolution as the kernels compute it, in fp32 (NHWC out), with planted defects:
      drop_chunk = (img, y, x, tap, c)   one `chunk`-channel slice c of tap (ty, tx) = divmod(tap, kw) is missing at
                                         one pixel, for every filter;
      halo_col_zero = x0                 the tile whose first column is x0 reads its left halo column (x0 - 1) as zero;
      prev_image_row = img               image img reads its row -1 from the last row of image img - 1 (adjacent in
                                         memory) instead of the zero row;
      wrong_class = (corner y, corner x, cls)   RF_CONV_BORDER_BIAS (bias [9, cout]): that pixel of every image takes
                                         the bias row of class cls."""
    x, w = x.float(), w.float()
    n, cin, h, wd = x.shape
    kh, kw = w.shape[2], w.shape[3]
    y = F.conv2d(x, w, None, padding=pad).permute(0, 2, 3, 1).contiguous()
    xp = F.pad(x, (pad, pad, pad, pad))
    if drop_chunk is not None:
        i, py, px, tap, c = drop_chunk
        ty, tx = divmod(tap, kw)
        sl = slice(c * chunk, (c + 1) * chunk)
        y[i, py, px] -= w[:, sl, ty, tx] @ xp[i, sl, py + ty, px + tx]
    if halo_col_zero is not None:
        x0 = halo_col_zero
        assert pad == 1 and 0 < x0 < wd
        for ty in range(kh):  # tap column 0 of output column x0 reads input column x0 - 1
            y[:, :, x0] -= torch.einsum("nch,oc->nho", xp[:, :, ty:ty + h, x0], w[:, :, ty, 0])
    if prev_image_row is not None:
        i = prev_image_row
        assert pad == 1 and 0 < i < n
        last = F.pad(x[i - 1, :, h - 1], (1, 1))  # [cin, w + 2]
        for tx in range(kw):
            y[i, 0] += last[:, tx:tx + wd].t() @ w[:, :, 0, tx].t()
    if bias is not None and bias.dim() == 2:
        cls = border_classes(h, wd)
        if wrong_class is not None:
            cls[wrong_class[0], wrong_class[1]] = wrong_class[2]
        y = y + bias.float()[cls]
    elif bias is not None:
        y = y + bias.float()
    for r in (res1, res2):
        if r is not None:
            y = y + r.float()
    return y


def emulated_store(g: "Guarded", values: torch.Tensor, past_cout: bool = False) -> "Guarded":
    """Write `values` ([rows, cols]) into a Guarded output as a kernel's epilogue would.  past_cout plants a 4-element
    store one channel group past the last real channel in the LAST row (rows before it would be overwritten by their
    successors in a dense buffer): zeros, the value a padded accumulator column holds -- which an `== 0` check of
    caller-zeroed padding columns cannot see."""
    g.fill(values)
    if past_cout:
        flat = g.buf.view(-1)
        at = (g.g + g.rows - 1) * g.ld + g.col_off + g.cols
        flat[at:at + 4] = 0
    return g


def _gptr(g_) -> int:
    return 0 if g_ is None else g_.view.data_ptr()


class ConvLaunch:
    """One convolution / deconvolution call through the C entry points (rf_conv2d_f16, rf_conv2d_bf16x3, rf_deconv2d_*)
    with every device buffer but the weights inside a Guarded allocation.  `conv` (dpt._Conv) supplies the weight
    layout and the plan.

    Inputs (NaN surround): the operand planes [pixels, cin_pad] (padded channels zero, as rf.h requires; the guard
    rows are what a kernel reads as row -1 of image 0 or row h of the last image if it does not take the zero row),
    the residuals [pixels, cout], the bias [1 | 9, cout].  Outputs (OUT_GUARD = 256 guard rows, the tallest tile, so an
    overrun of a tile's height lands inside the allocation and is reported): `out` dense [pixels, cout] (the head:
    [pixels, n_fin] or, NCHW, [n n_fin, ho wo]) and the planes [pixels, cout] inside rows of ld > cout starting
    col_off columns in."""
    OUT_GUARD = 256

    def __init__(self, conv, x: torch.Tensor, x_lo: torch.Tensor = None, stride: int = 1, pad: int = None,
                 bias: torch.Tensor = None, res1=None, res2=None, device="cuda"):
        self.conv, self.dev = conv, device
        n, cin, h, w = x.shape
        assert cin == conv.cin
        self.n, self.h, self.w, self.stride = n, h, w, stride
        self.pad = conv.kh // 2 if pad is None else pad
        if conv.k:
            self.ho, self.wo = h * conv.k, w * conv.k
        else:
            self.ho = (h + 2 * self.pad - conv.kh) // stride + 1
            self.wo = (w + 2 * self.pad - conv.kw) // stride + 1
        self.pix = n * self.ho * self.wo
        dt = torch.float16 if conv.f16 else torch.bfloat16
        gin = 2 * (w + 2)  # more than one image row and its two halo pixels before and after the images

        def plane(v):
            rows = torch.zeros(n * h * w, conv.cin_pad)
            rows[:, :cin] = v.permute(0, 2, 3, 1).reshape(-1, cin)
            assert torch.equal(rows.to(dt).float(), rows), "operand planes must hold values exact in their type"
            return Guarded(n * h * w, conv.cin_pad, dt, device, g=gin, ld=conv.cin_pad).fill(rows)

        self.x_hi = plane(x)
        self.x_lo = None if conv.f16 else plane(torch.zeros_like(x) if x_lo is None else x_lo)
        self.bias = None if bias is None else Guarded(bias.numel() // conv.cout, conv.cout, torch.float32, device,
                                                      ld=conv.cout).fill(bias.view(-1, conv.cout))
        self.res = [None if r is None else Guarded(self.pix, conv.cout, torch.float32, device, g=4, ld=conv.cout)
                    .fill(r.reshape(self.pix, conv.cout)) for r in (res1, res2)]
        self.out = self.p_hi = self.p_lo = None

    def plan(self, flags: int = 0, n_fin: int = 0):
        from renderformer_amd import _lib
        c = self.conv
        return _lib.conv_plan(c.f16, self.n, self.h, self.w, c.cin_pad, c.cout, c.cout_pad, c.kh, c.kw, self.stride,
                              self.pad, flags, n_fin, c.k, int(_lib.load(require_device=False).rf_gemm_workspace_bytes()))

    def alloc(self, want_out: bool = True, plane_ld: int = None, col_off: int = 0, flags: int = 0, final=None) -> int:
        """Fresh Guarded outputs for one launch (and the head's operands); returns the flags to pass."""
        c, dev, G = self.conv, self.dev, self.OUT_GUARD
        self.out = self.p_hi = self.p_lo = self.w_fin = self.b_fin = None
        self.plane_ld, self.n_fin, self.alpha = plane_ld or 0, 0, 0.0
        if final is not None:
            self.n_fin, self.alpha = final[0].shape[0], final[2]
            self.w_fin = Guarded(self.n_fin, c.cout, torch.float32, dev, ld=c.cout).fill(final[0])
            self.b_fin = Guarded(1, self.n_fin, torch.float32, dev, ld=self.n_fin).fill(final[1][None])
            flags |= 4
            hw = self.ho * self.wo
            self.out = (Guarded(self.n * self.n_fin, hw, torch.float32, dev, g=G, ld=hw) if flags & 16 else
                        Guarded(self.pix, self.n_fin, torch.float32, dev, g=G, ld=self.n_fin))
        elif want_out:
            self.out = Guarded(self.pix, c.cout, torch.float32, dev, g=G, ld=c.cout)
        if plane_ld:
            assert col_off % 4 == 0 and plane_ld % 4 == 0 and col_off + c.cout <= plane_ld and plane_ld > c.cout
            dt = torch.float16 if c.f16 else torch.bfloat16
            self.p_hi = Guarded(self.pix, c.cout, dt, dev, g=G, ld=plane_ld, col_off=col_off)
            self.p_lo = None if c.f16 else Guarded(self.pix, c.cout, dt, dev, g=G, ld=plane_ld, col_off=col_off)
        return flags

    def views(self):
        return tuple(None if g_ is None else g_.view for g_ in (self.out, self.p_hi, self.p_lo))

    def __call__(self, want_out: bool = True, plane_ld: int = None, col_off: int = 0, flags: int = 0, final=None):
        """Launch.  final = (w_fin [n_fin, cout], b_fin [n_fin], elu_alpha): the fused head (flags gets RF_CONV_FINAL).
        Returns (out view or None, plane hi view or None, plane lo view or None); the Guarded buffers stay on self."""
        from renderformer_amd._lib import call, ptr, stream
        from renderformer_amd.ops import _gemm_workspace
        c = self.conv
        ws = _gemm_workspace(self.x_hi.buf.device)
        flags = self.alloc(want_out, plane_ld, col_off, flags, final)
        p = _gptr
        tail = (p(self.out), p(self.p_hi)) + (() if c.f16 else (p(self.p_lo),)) + (self.plane_ld,)
        head = (p(self.x_hi),) + (() if c.f16 else (p(self.x_lo),)) + (self.n, self.h, self.w, c.cin_pad, ptr(c.w_hi)) + \
               (() if c.f16 else (ptr(c.w_lo),))
        if c.k:
            assert not flags and self.res == [None, None]
            call("rf_deconv2d_f16" if c.f16 else "rf_deconv2d_bf16x3", *head, c.cout, c.k, p(self.bias), *tail, ptr(ws),
                 ws.numel(), stream())
        else:
            call("rf_conv2d_f16" if c.f16 else "rf_conv2d_bf16x3", *head, c.cout, c.cout_pad, c.kh, c.kw, self.stride,
                 self.pad, p(self.bias), p(self.res[0]), p(self.res[1]), *tail, flags, p(self.w_fin), p(self.b_fin),
                 self.n_fin, self.alpha, ptr(ws), ws.numel(), stream())
        torch.cuda.synchronize()
        return self.views()

    def assert_untouched(self, what: str = ""):
        for name, g_ in (("out", self.out), ("plane hi", self.p_hi), ("plane lo", self.p_lo)):
            if g_ is not None:
                g_.assert_untouched(what=f"{what} {name}")

    def shaped(self, view: torch.Tensor) -> torch.Tensor:
        """A [pixels, cout] output view as NHWC [n, ho, wo, cout] on the CPU."""
        return view.detach().cpu().reshape(self.n, self.ho, self.wo, -1)


def conv_group_launch(members, flags) -> None:
    """rf_conv2d_f16_group over ConvLaunch members whose outputs alloc() made (fp16; residuals are not part of a
    grouped launch); flags: one per member (RF_CONV_PLANE_SILU / RF_CONV_BORDER_BIAS)."""
    import ctypes
    from renderformer_amd._lib import call, ptr, stream
    from renderformer_amd.dpt import _ConvDesc
    descs = (_ConvDesc * len(members))()
    for d, m, fl in zip(descs, members, flags):
        c = m.conv
        assert c.f16 and m.res == [None, None]
        d.in_, d.w, d.bias, d.out, d.p_out = _gptr(m.x_hi), ptr(c.w_hi), _gptr(m.bias), _gptr(m.out), _gptr(m.p_hi)
        d.n_img, d.hi, d.wi, d.cin_pad, d.cout, d.cout_pad = m.n, m.h, m.w, c.cin_pad, c.cout, c.cout_pad
        d.kh, d.kw, d.stride, d.pad, d.deconv_k, d.p_ld, d.flags = c.kh, c.kw, m.stride, m.pad, c.k, m.plane_ld, fl
    call("rf_conv2d_f16_group", len(members), ctypes.cast(descs, ctypes.c_void_p), stream())
    torch.cuda.synchronize()


def conv1x1_group_launch(members) -> None:
    """rf_conv1x1_f16_group over ConvLaunch members (fp16 1x1 convolutions over images of one size, plane outputs)."""
    import ctypes
    from renderformer_amd._lib import call, ptr, stream
    k = len(members)
    arrs = []

    def arr(ct, vals):
        a = (ct * k)(*vals)
        arrs.append(a)
        return ctypes.cast(a, ctypes.c_void_p)

    m0 = members[0]
    assert all(m.conv.f16 and m.conv.kh == 1 and not m.conv.k and (m.n, m.h, m.w) == (m0.n, m0.h, m0.w) for m in members)
    call("rf_conv1x1_f16_group", k, arr(ctypes.c_void_p, [_gptr(m.x_hi) for m in members]),
         arr(ctypes.c_int, [m.conv.cin_pad for m in members]), arr(ctypes.c_void_p, [ptr(m.conv.w_hi) for m in members]),
         arr(ctypes.c_int, [m.conv.cout for m in members]), arr(ctypes.c_int, [m.conv.cout_pad for m in members]),
         arr(ctypes.c_void_p, [_gptr(m.bias) for m in members]), arr(ctypes.c_void_p, [_gptr(m.p_hi) for m in members]),
         arr(ctypes.c_int, [m.plane_ld for m in members]), m0.n, m0.h, m0.w, stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ prologue and output
# Everything below serves prologue.hip (scene -> stage-1 tokens and RoPE positions, cameras -> ray tokens, logits ->
# HDR frame): fp64 references computed from the fp32 inputs the kernels read, a bound next to each that counts one
# F32_ULP per fp32 operation of the kernel's chain (FMA contraction only removes roundings), and fp32 emulations of
# the kernels' order of operations with switches that plant one defect each.
#
# What this project cannot derive is the accuracy of the device math library (sinf, tanf, log10f, expm1f, powf).
# LIBM_ULPS is the number of fp32 ulps of the result allowed per library call.  ASSUMED: the ROCm installation this
# was written against ships no math-accuracy table, so the value is 4, which is at or above the figures the HIP
# documentation has published for these five functions; the GPU tests print the share of each bound that is used.
LIBM_ULPS = 4
_HALF_PI = math.pi / 2.0
_SIN_ABS = LIBM_ULPS * 2.0 ** -24  # LIBM_ULPS ulps of a sine: |sin| <= 1, so an ulp is at most 2^-24


def _f32(v: float) -> float:
    """The fp32 value a kernel receives for the host float v, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- vertex normals
def _vn_scaled(vn: torch.Tensor, n_freqs: int) -> torch.Tensor:
    """fp64 [n, 9 L]: x_d 2^l, d-major and l-minor (exact in fp32 as well: a power-of-two scale)."""
    x = vn.double().reshape(-1, 9)
    return (x[:, :, None] * 2.0 ** torch.arange(n_freqs, dtype=torch.float64)).reshape(-1, 9 * n_freqs)


def vn_encode_ref(vn: torch.Tensor, n_freqs: int, ld: int) -> torch.Tensor:
    """fp64 [n, ld]: [x | sin(x_d 2^l) | sin(x_d 2^l + pi / 2)], zero-padded to ld (rf.h, rf_ref.nerf_encode)."""
    x, s, ns = vn.double().reshape(-1, 9), _vn_scaled(vn, n_freqs), 9 * n_freqs
    assert ld >= 9 + 2 * ns
    out = torch.zeros(x.shape[0], ld, dtype=torch.float64)
    out[:, :9], out[:, 9:9 + ns], out[:, 9 + ns:9 + 2 * ns] = x, torch.sin(s), torch.sin(s + _HALF_PI)
    return out


def vn_encode_bound(vn: torch.Tensor, n_freqs: int, ld: int, out_dtype: torch.dtype) -> torch.Tensor:
    """x is copied and x_d 2^l is exact; a sine term is one library call: LIBM_ULPS 2^-24; a phase-shifted term first
    rounds s + fl(pi / 2), one F32_ULP of a sum below |s| + 2 (which also covers fl(pi / 2) - pi / 2 = 4.4e-8), and
    |sin'| <= 1 carries that into the result: F32_ULP (|s| + 2) + LIBM_ULPS 2^-24.  The padding is exactly 0.  Then
    the output rounding."""
    s, ns = _vn_scaled(vn, n_freqs), 9 * n_freqs
    e = torch.zeros(s.shape[0], ld, dtype=torch.float64)
    e[:, 9:9 + ns] = _SIN_ABS
    e[:, 9 + ns:9 + 2 * ns] = F32_ULP * (s.abs() + 2.0) + _SIN_ABS
    return e + out_rounding(vn_encode_ref(vn, n_freqs, ld).abs(), e, out_dtype)


def vn_encode_emulation(vn: torch.Tensor, n_freqs: int, ld: int, out_dtype: torch.dtype, freq_off_by_one=None,
                        swap_sin_cos: bool = False, dirty_padding: bool = False) -> torch.Tensor:
    """vn_encode_kernel in fp32.  Planted defects: freq_off_by_one = d takes 2^(l + 1) for input dimension d only;
    swap_sin_cos writes the phase-shifted block first; dirty_padding leaves the smallest fp16 subnormal (what a
    buffer that held other data would show is larger) in the columns past 9 (2 L + 1)."""
    x, ns = vn.float().reshape(-1, 9), 9 * n_freqs
    lvl = torch.arange(n_freqs, dtype=torch.float32).expand(9, n_freqs).clone()
    if freq_off_by_one is not None:
        lvl[freq_off_by_one] += 1.0
    s = (x[:, :, None] * torch.exp2(lvl)).reshape(-1, ns)
    a, b = torch.sin(s), torch.sin(s + torch.tensor(_HALF_PI, dtype=torch.float32))
    if swap_sin_cos:
        a, b = b, a
    out = torch.full((x.shape[0], ld), 2.0 ** -24 if dirty_padding else 0.0, dtype=torch.float32)
    out[:, :9], out[:, 9:9 + ns], out[:, 9 + ns:9 + 2 * ns] = x, a, b
    return out.to(out_dtype)


# ---- RoPE positions and register-token centres
def _scene_sets(scene_off, c2w, n_views: int):
    off = [int(v) for v in scene_off]
    n_scenes = len(off) - 1
    sets = n_scenes * n_views if c2w is not None else n_scenes
    return off, [(s // n_views if c2w is not None else s) for s in range(sets)]


def scene_pos_ref(tris, valid_idx, scene_off, c2w, n_views: int, n_reg: int):
    """(rows, centres) in fp64.  rows: one [n_s, 9] tensor per set (set s = scene b without c2w, else b n_views + v):
    the scene's valid triangles, with c2w [sets, 4, 4] each vertex p as R^T (p - t).  centres [sets, 3]: per
    coordinate sum / (n + 1e-5) over the set's rows, averaged over the three vertices (rf.h; n_reg rows of
    [c | c | c] precede the triangle rows in pos_out: scene_pos_pack)."""
    off, scene_of = _scene_sets(scene_off, c2w, n_views)
    t64, idx = tris.double().reshape(-1, 9), valid_idx.long()
    rows, centres = [], []
    for s, b in enumerate(scene_of):
        v = t64[idx[off[b]:off[b + 1]]]
        if c2w is not None:
            m = c2w.double().reshape(-1, 4, 4)[s]
            v = ((v.view(-1, 3, 3) - m[:3, 3]) @ m[:3, :3]).reshape(-1, 9)  # (R^T p)_a = sum_b R_ba p_b: p @ R
        rows.append(v)
        centres.append((v.sum(0) / (v.shape[0] + 1e-5)).view(3, 3).mean(0))
    return rows, torch.stack(centres)


def scene_pos_bound(tris, valid_idx, scene_off, c2w, n_views: int, n_reg: int):
    """(row bounds, centre bounds), shaped as scene_pos_ref's results.
    Rows: a copy without c2w (bound 0).  With it the kernel forms tinv_a = -(sum_b R_ba t_b), 3 products and 2 adds,
    then sum_b R_ba p_b + tinv_a, 3 products and 3 adds, every one within one F32_ULP of a partial sum that is at
    most Mp + Mt (Mp = sum_b |R_ba| |p_b|, Mt = sum_b |R_ba| |t_b|; Mt alone for tinv): F32_ULP (6 (Mp + Mt) + 5 Mt).
    Centres: the issue's count, (6 + 2 + nb + 4) 2^-24 mean|x| with nb = ceil(n / 256): every add is correctly
    rounded (2^-24 relative) and an element passes through the 6 butterfly adds of its wave, the 2 adds over the 4
    waves, the nb - 1 serial adds over the blocks (the first adds to 0: exact), and then fl(n + 1e-5), the division,
    two vertex adds and the division by 3.  mean|x| = sum |x| / (n + 1e-5) averaged over the three vertices bounds
    every partial sum of that chain; the rows' own error enters the sum the same way (their bound, averaged)."""
    off, scene_of = _scene_sets(scene_off, c2w, n_views)
    rows, _ = scene_pos_ref(tris, valid_idx, scene_off, c2w, n_views, n_reg)
    t64, idx = tris.double().reshape(-1, 9), valid_idx.long()
    e_rows, e_centres = [], []
    for s, b in enumerate(scene_of):
        v = t64[idx[off[b]:off[b + 1]]]
        e = torch.zeros_like(v)
        if c2w is not None:
            m = c2w.double().reshape(-1, 4, 4)[s].abs()
            mp, mt = v.abs().view(-1, 3, 3) @ m[:3, :3], m[:3, 3] @ m[:3, :3]
            e = (F32_ULP * (6.0 * (mp + mt) + 5.0 * mt)).reshape(-1, 9)
        n = v.shape[0]
        ops = 6 + 2 + (n + 255) // 256 + 4
        mean_abs = ((rows[s].abs() + e).sum(0) / (n + 1e-5)).view(3, 3).mean(0)
        e_rows.append(e)
        e_centres.append(ops * 2.0 ** -24 * mean_abs + (e.sum(0) / (n + 1e-5)).view(3, 3).mean(0))
    return e_rows, torch.stack(e_centres)


def scene_pos_pack(rows, centres, n_reg: int):
    """pos_out's layout from per-set rows and centres: ([total, 9] fp64, set_off int32 [sets + 1], centre-row mask)."""
    parts, off, is_centre = [], [0], []
    for r, c in zip(rows, centres):
        parts += [c.repeat(3)[None].expand(n_reg, 9), r]
        is_centre += [torch.ones(n_reg, dtype=torch.bool), torch.zeros(r.shape[0], dtype=torch.bool)]
        off.append(off[-1] + n_reg + r.shape[0])
    return torch.cat(parts), torch.tensor(off, dtype=torch.int32), torch.cat(is_centre)


def scene_centre_emulation(rows: torch.Tensor, drop_second_round: bool = False, divide_by_n: bool = False):
    """The centre [3] of one set's rows [n, 9] in fp32 in the kernels' order: per block of 256 the xor butterfly of each
    64-lane wave (wave_sum), (w0 + w1) + (w2 + w3), then the block partials serially in block order, / (n + 1e-5),
    the three vertices added and / 3.  Planted defects: drop_second_round stops after the first 64 blocks;
    divide_by_n divides by n (0 / 0 in an empty set)."""
    n = rows.shape[0]
    nb = (n + 255) // 256
    v = torch.zeros(max(nb, 1) * 256, 9, dtype=torch.float32)
    v[:n] = rows.float()
    v = v.view(-1, 4, 64, 9)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    acc = torch.zeros(9, dtype=torch.float32)
    for b in range(min(nb, 64) if drop_second_round else nb):
        acc = acc + part[b]
    den = torch.tensor(float(n), dtype=torch.float32)
    tot = acc / (den if divide_by_n else den + torch.tensor(1e-5, dtype=torch.float32))
    return (tot[0:3] + tot[3:6] + tot[6:9]) / torch.tensor(3.0, dtype=torch.float32)


# ---- HDR output
def hdr_ref(logits: torch.Tensor, alpha: float, log_decode: bool, channels_last: bool) -> torch.Tensor:
    """fp64 decode(elu(logits [n, c, h, w], fl32(alpha))), decode = 10^y - 1 if log_decode; [n, h, w, c] when
    channels_last.  A window of the output is this function of the same window of the logits."""
    y = logits.double()
    y = torch.where(y > 0, y, _f32(alpha) * torch.expm1(y))
    if log_decode:
        y = torch.pow(10.0, y) - 1.0
    return (y.permute(0, 2, 3, 1) if channels_last else y).contiguous()


def hdr_bound(logits: torch.Tensor, alpha: float, log_decode: bool, channels_last: bool) -> torch.Tensor:
    """y > 0 passes through.  Otherwise alpha expm1f(y): the library call within LIBM_ULPS ulps of its result and one
    multiply: e1 = (LIBM_ULPS + 1) F32_ULP |elu|.  Log decode: powf within LIBM_ULPS ulps of 10^y', y' within e1 of
    y (10^y (10^e1 - 1) exactly), and the subtraction one ulp of its result:
    10^y (10^e1 - 1) + LIBM_ULPS F32_ULP 10^y + F32_ULP |10^y - 1|."""
    x = logits.double()
    y = torch.where(x > 0, x, _f32(alpha) * torch.expm1(x))
    e = torch.where(x > 0, torch.zeros_like(y), (LIBM_ULPS + 1) * F32_ULP * y.abs())
    if log_decode:
        p = torch.pow(10.0, y)
        e = p * (torch.pow(10.0, e) - 1.0) + LIBM_ULPS * F32_ULP * p + F32_ULP * (p - 1.0).abs()
    return (e.permute(0, 2, 3, 1) if channels_last else e).contiguous()


def hdr_emulation(logits: torch.Tensor, alpha: float, log_decode: bool, channels_last: bool,
                  wrong_layout_index: bool = False, exp_for_expm1: bool = False) -> torch.Tensor:
    """hdr_output_kernel in fp32.  Planted defects: wrong_layout_index stores a channels-last output at the
    channels-first index (img c + ch) hw + px; exp_for_expm1 computes alpha exp(y) on the negative branch."""
    x = logits.float()
    a = torch.tensor(alpha, dtype=torch.float32)
    y = torch.where(x > 0, x, a * (torch.exp(x) if exp_for_expm1 else torch.expm1(x)))
    if log_decode:
        y = torch.pow(torch.tensor(10.0, dtype=torch.float32), y) - 1.0
    n, c, h, w = y.shape
    if channels_last and wrong_layout_index:
        return y.contiguous().view(n, h, w, c)
    return (y.permute(0, 2, 3, 1) if channels_last else y).contiguous()


# ---- texture encoder
def log_encode_ref(x: torch.Tensor):
    """(fp64 log10(fl32(x + 1)), its bound): the add is the kernel's own fp32 operation, so only the library call is
    left: LIBM_ULPS ulps of the result."""
    ref = torch.log10((x.float() + 1.0).double())
    return ref, LIBM_ULPS * F32_ULP * ref.abs()


def texture_linear_ref(coef: torch.Tensor, wsum: torch.Tensor, bias) -> torch.Tensor:
    """fp64 [rows, n] = bias + coef[:, :channels] wsum (wsum [channels, n])."""
    ref = coef[:, :wsum.shape[0]].double() @ wsum.double()
    return ref if bias is None else ref + bias.double()


def texture_linear_bound(coef: torch.Tensor, wsum: torch.Tensor, bias) -> torch.Tensor:
    """The accumulator starts at the bias and takes one fused multiply-add per channel (the padded channels add an
    exact 0): `channels` roundings, each within one F32_ULP of a partial sum of at most |bias| + |coef| |wsum|."""
    ch = wsum.shape[0]
    mag = coef[:, :ch].double().abs() @ wsum.double().abs()
    return ch * F32_ULP * (mag if bias is None else mag + bias.double().abs())


def texture_linear_emulation(coef, wsum, bias, bias_per_trip: bool = False,
                             skip_last_partial_block: bool = False) -> torch.Tensor:
    """texture_linear_kernel in fp32: acc = bias, then acc = fma(coef[r, c], wsum[c, o], acc) in channel order (the
    product exact in fp64, the sum rounded to fp32).  Unwritten elements are NaN.  Planted defects: bias_per_trip adds
    the bias once per 1024-column trip of a thread, so columns 1024 t .. 1024 t + 1023 get it t + 1 times;
    skip_last_partial_block leaves the rows of a last block of fewer than 16 rows unwritten."""
    ch, n = wsum.shape
    rows = coef.shape[0]
    b = torch.zeros(n, dtype=torch.float32) if bias is None else bias.float()
    acc = b.expand(rows, n).clone()
    if bias_per_trip:
        acc = acc * (1 + torch.arange(n) // 1024).float()
    for c in range(ch):
        acc = (acc.double() + coef[:, c:c + 1].double() * wsum[c].double()).float()
    if skip_last_partial_block and rows % 16:
        acc[rows - rows % 16:] = float("nan")
    return acc


# ---- rays
def patchify_ref(rays: torch.Tensor, patch: int) -> torch.Tensor:
    """[v, h, w, 3] -> tokens [v (h / p) (w / p), 3 p p]: out[view R + py (w / p) + px, c p p + p1 p + p2] (rf.h)."""
    v, h, w, _ = rays.shape
    p = patch
    return rays.view(v, h // p, p, w // p, p, 3).permute(0, 1, 3, 5, 2, 4).reshape(v * (h // p) * (w // p), 3 * p * p)


def ray_tokens_ref(c2w, fov, intr, frame, token_frame, origin, patch: int, out_dtype: torch.dtype = None):
    """(tokens fp64, ray_pos fp64 [v, 9], bound or None) by the formula of rf.h: token pixel (x, y) of the h x w token
    frame is pixel (x - x0, y - y0) of the requested frame_h x frame_w frame's camera; direction ((x' + 0.5 - cx) / fx,
    -(y' + 0.5 - cy) / fy, -1) rotated by c2w and L2-normalised; fov mode (degrees, vertical): fx = fy = frame_h / 2 /
    tan(fov / 2), cx = frame_w / 2, cy = frame_h / 2; intr [v, 4] = (fx, fy, cx, cy).  ray_pos = the camera origin
    three times.
    bound (with out_dtype), one F32_ULP per operation, to first order:
      f       fov / 180, * pi (fl(pi) is within 2^-24 of pi), tanf, the division: the argument's 2 F32_ULP pass
              through tan as theta (1 + t^2) / t relative, plus LIBM_ULPS + 1 ulps: rel_f (0 with intrinsics);
      dx, dy  the subtraction of cx rounds once, F32_ULP (|x' + 0.5| + |cx|), then the division: e_d = (e_num + |num|
              (F32_ULP + rel_f)) / |f|;
      r_a     3 products and 2 adds within F32_ULP of Mr = |dx| |m0| + |dy| |m1| + |m2|, plus the inputs' errors;
      nrm     3 products, 2 adds (5 F32_ULP of nrm^2, plus 2 sum |r_a| e_a), the square root halves that and adds one;
      out     r_a / nrm: e_a / nrm + |r_a| / nrm (rel_nrm + F32_ULP); then the output rounding."""
    m = c2w.double().reshape(-1, 4, 4)
    nv = m.shape[0]
    (fh, fw), (h, w), (y0, x0) = frame, token_frame, origin
    if intr is not None:
        k = intr.double().reshape(nv, 4)
        fx, fy, cx, cy = k[:, 0], k[:, 1], k[:, 2], k[:, 3]
        rel_f = torch.zeros(nv, dtype=torch.float64)
    else:
        theta = 0.5 * (fov.double().reshape(nv) / 180.0 * math.pi)
        t = torch.tan(theta)
        fx = fy = fh / 2.0 / t
        cx, cy = torch.full((nv,), fw / 2.0, dtype=torch.float64), torch.full((nv,), fh / 2.0, dtype=torch.float64)
        rel_f = F32_ULP * (2.0 * theta * (1.0 + t * t) / t + LIBM_ULPS + 1.0)
    xs = (torch.arange(w, dtype=torch.float64) - x0 + 0.5)[None, None, :]
    ys = (torch.arange(h, dtype=torch.float64) - y0 + 0.5)[None, :, None]
    v3 = lambda a: a[:, None, None]  # noqa: E731  ([v] -> [v, 1, 1])
    nx, ny = (xs - v3(cx)).expand(nv, h, w), (ys - v3(cy)).expand(nv, h, w)
    dx, dy = nx / v3(fx), -(ny / v3(fy))
    d = torch.stack([dx, dy, -torch.ones_like(dx)], dim=-1)  # [v, h, w, 3]
    rot = m[:, :3, :3]
    r = torch.einsum("vhwb,vab->vhwa", d, rot)
    nrm = r.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    rays = r / nrm
    ray_pos = m[:, :3, 3].repeat(1, 3)
    bound = None
    if out_dtype is not None:
        e_dx = (F32_ULP * (xs.abs() + v3(cx).abs()) + nx.abs() * (F32_ULP + v3(rel_f))) / v3(fx).abs()
        e_dy = (F32_ULP * (ys.abs() + v3(cy).abs()) + ny.abs() * (F32_ULP + v3(rel_f))) / v3(fy).abs()
        e_d = torch.stack([e_dx.expand(nv, h, w), e_dy.expand(nv, h, w), torch.zeros(nv, h, w, dtype=torch.float64)], -1)
        e_r = 5.0 * F32_ULP * torch.einsum("vhwb,vab->vhwa", d.abs(), rot.abs()) + \
            torch.einsum("vhwb,vab->vhwa", e_d, rot.abs())
        rel_n = 0.5 * (5.0 * F32_ULP + 2.0 * (r.abs() * e_r).sum(-1, keepdim=True) / (nrm * nrm)) + F32_ULP
        e = e_r / nrm + rays.abs() * (rel_n + F32_ULP)
        bound = patchify_ref(e + out_rounding(rays.abs(), e, out_dtype), patch)
    return patchify_ref(rays, patch), ray_pos, bound


# ---- the inputs the GPU tests run and the CPU proofs plant their defects into
VN_ROWS = (1, 6, 257)  # one row, 4 < n < 8 (a ragged second block), 64 blocks and one row
VN_SHAPES = ((6, 128), (6, 117), (6, 192), (1, 27), (1, 32))  # (L, ldo); L = 1: n_sin = 9
SCENE_COUNTS = (16700, 0, 256, 257)  # 66 blocks (two rounds of the centre kernel), empty, 256 k, 256 k + 1
SCENE_COUNTS_VIEWS = (300, 0, 513)  # with c2w and 3 views
HDR_SHAPES = ((1, 1, 1), (1, 15, 17), (1, 1, 257), (2, 3, 7))  # (n, h, w): 1, 255, 257 and 42 pixels
HDR_SPECIALS = (0.0, -0.0, 1e-8, -1e-8, -50.0, 10.0, -1e-3)
TEXTURE_LINEAR_SHAPES = ((1, 1, 4), (17, 13, 1024), (33, 16, 1028), (16, 13, 2048))  # (rows, channels, n)


def vn_case(n_rows: int, seed: int = 0):
    """(vn f32 [n_rows, 9], dst_row int32 [n_rows], written bool [n_rows]).  Unit normals, three to a row; row 0 starts
    with the exact values 1, -1, 0, -0.0 and row 3 (if there is one) holds nothing else.  dst_row sends every input
    row to a row of its own of an n_rows-row output, in shuffled order, except every fifth one (from row 2), which is a
    hole (-1): `written` marks the output rows that receive a row."""
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    v = torch.randn(n_rows, 3, 3, generator=g)
    vn = (v / v.norm(dim=-1, keepdim=True)).reshape(n_rows, 9).contiguous()
    vn[0, :4] = torch.tensor([1.0, -1.0, 0.0, -0.0])
    if n_rows > 3:
        vn[3] = torch.tensor([1.0, 0.0, -0.0, -1.0, 0.0, 1.0, -0.0, -1.0, 0.0])
    dst = torch.randperm(n_rows, generator=g).to(torch.int32)
    dst[2::5] = -1
    written = torch.zeros(n_rows, dtype=torch.bool)
    written[dst[dst >= 0].long()] = True
    return vn, dst, written


def vn_scatter(values: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """values [n, ld] of the input rows -> the output's rows (unwritten rows 0; compare written rows only)."""
    out = torch.zeros_like(values)
    keep = dst >= 0
    out[dst[keep].long()] = values[keep]
    return out


def scene_case(counts, n_views: int = 0, seed: int = 0):
    """(tris f32 [m, 9], valid_idx int32, scene_off int32, c2w f32 [scenes n_views, 4, 4] or None).  The valid rows are
    a shuffled subset of the m rows of tris (a mask with holes, its rows in no order); the rows outside it are NaN.
    Vertices are normal around (0.3, -0.2, 0.5), so no centre is a sum that cancels.  c2w: a random rotation (QR of a
    normal matrix, determinant +1: no axis-aligned or symmetric R, so a transposed R shows) and a translation of a few
    units per view."""
    g = torch.Generator(device="cpu").manual_seed(2000 + seed)
    total = sum(counts)
    m = total + total // 4 + 7
    valid = torch.randperm(m, generator=g)[:total]
    tris = torch.full((m, 9), float("nan"))
    tris[valid] = 0.5 * torch.randn(total, 9, generator=g) + torch.tensor([0.3, -0.2, 0.5]).repeat(3)
    scene_off = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32)
    c2w = None
    if n_views:
        sets = len(counts) * n_views
        q, r = torch.linalg.qr(torch.randn(sets, 3, 3, generator=g).double())
        q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
        q[:, :, 0] *= torch.linalg.det(q)[:, None]
        c2w = torch.eye(4).repeat(sets, 1, 1)
        c2w[:, :3, :3] = q.float()
        c2w[:, :3, 3] = 2.0 * torch.randn(sets, 3, generator=g) + torch.tensor([1.0, -3.0, 2.0])
    return tris, valid.to(torch.int32), scene_off, c2w


def hdr_logits(n: int, c: int, h: int, w: int, seed: int = 0) -> torch.Tensor:
    """Normal logits (sigma 2) [n, c, h, w] whose first elements are HDR_SPECIALS (as many as fit)."""
    g = torch.Generator(device="cpu").manual_seed(3000 + seed)
    x = 2.0 * torch.randn(n, c, h, w, generator=g)
    k = min(x.numel(), len(HDR_SPECIALS))
    x.view(-1)[:k] = torch.tensor(HDR_SPECIALS[:k])
    return x


def texture_linear_case(rows: int, channels: int, n: int, seed: int = 0):
    """(coef f32 [rows, channels], wsum f32 [channels, n], bias f32 [n]), normal."""
    g = torch.Generator(device="cpu").manual_seed(4000 + seed)
    return torch.randn(rows, channels, generator=g), torch.randn(channels, n, generator=g), torch.randn(n, generator=g)


def camera_case(n_views: int, seed: int = 0):
    """(c2w f32 [v, 4, 4], fov degrees f32 [v] in [25, 70], intr f32 [v, 4] = (fx, fy, cx, cy) for a frame of about
    24 x 40 pixels, fx != fy and the principal point off the centre)."""
    g = torch.Generator(device="cpu").manual_seed(5000 + seed)
    c2w = scene_case((1,), n_views, seed)[3]
    fov = 25.0 + 45.0 * torch.rand(n_views, generator=g)
    intr = torch.tensor([30.0, 33.0, 19.0, 13.0]) + torch.rand(n_views, 4, generator=g) * torch.tensor([9.0, 9.0, 3.0, 3.0])
    return c2w, fov, intr
