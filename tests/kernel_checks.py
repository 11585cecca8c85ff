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
