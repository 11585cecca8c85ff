"""The helpers of tests/kernel_checks.py against plain torch emulations of the kernels (CPU only).

The evidence that the exact-arithmetic and guard-band GPU tests can fail: every defect planted in an emulation (a lost
K slice, a scaled row, a key counted twice or dropped, a store into a guard row or the ld padding, a load from the
input padding) is flagged by the helper the GPU tests use, and the unmodified emulation passes every helper.  The
last section does the same for the convolution helpers: a dropped 32-channel chunk of one tap at one pixel, a halo
column read as zero, a row read from the previous image, a wrong border class and a store past cout are each flagged
by the exact form, the tap mask, conv_bound or the guard band -- and the first of them passes the whole-tensor
`relerr < 1e-3` plane bar of the older conv tests.  The section after it covers the prologue and output kernels: each
emulation passes its bound, each planted defect (a frequency index off by one, swapped sine blocks, dirty padding, a
dropped reduction round, a division by n, a channels-first index, exp for expm1, a bias added per trip, a skipped
partial block) fails it, and the fp32 oracle lies inside the bounds of the fp64 references.
"""
import math

import pytest
import torch

import kernel_checks as kc

HALF = [torch.bfloat16, torch.float16]


def _gauss(m, n, k, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn(m, k, generator=g).to(dtype)
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(dtype)
    bias = torch.randn(n, generator=g)
    return a, w, bias


# ------------------------------------------------------------------------------------------------ Guarded
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int32])
def test_guarded_layout_and_sentinel(dtype):
    gd = kc.Guarded(5, 16, dtype, g=2, pad=8, col_off=4)
    assert gd.view.shape == (5, 16) and gd.view.stride(0) == gd.ld == 28 and gd.buf.shape == (9, 28)
    assert gd.view.data_ptr() - gd.buf.data_ptr() == (2 * 28 + 4) * gd.buf.element_size()
    if dtype.is_floating_point:
        assert torch.isnan(gd.buf).all()  # the sentinel is a NaN: a read of it poisons whatever it reaches
        bits = kc.sentinel_bits(dtype)
        size = gd.buf.element_size() * 8
        quiet = 1 << {16: 6 if dtype == torch.bfloat16 else 9, 32: 22}[size]
        assert bits & quiet and bits & (quiet - 1), "a quiet NaN with a payload"
    else:
        assert (gd.buf.view(torch.uint8) == 0xA5).all()
    gd.assert_untouched()
    gd.fill(torch.ones(5, 16))
    gd.assert_untouched()  # writing the view itself is allowed
    assert (gd.view == 1).all()


@pytest.mark.parametrize("where", ["guard_row_before", "guard_row_after", "ld_padding_right", "ld_padding_left"])
def test_guarded_flags_one_stray_element(where):
    gd = kc.Guarded(7, 32, torch.bfloat16, g=2, pad=8, col_off=4)
    gd.fill(torch.zeros(7, 32))
    r, c = {"guard_row_before": (1, 10), "guard_row_after": (9, 4), "ld_padding_right": (4, 36),
            "ld_padding_left": (4, 3)}[where]
    gd.buf[r, c] = 1.0
    with pytest.raises(AssertionError, match=rf"first at \(row {r - 2}, col {c - 4}\)"):
        gd.assert_untouched(what=where)


def test_guarded_flags_a_rewritten_sentinel_value():
    """A store of another NaN (or of the same value with another payload) is a change: the compare is on bits."""
    gd = kc.Guarded(3, 8, torch.float32)
    gd.buf[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="first at"):
        gd.assert_untouched()


def test_guarded_written_rows():
    gd = kc.Guarded(6, 8, torch.float32)
    written = torch.tensor([True, False, True, True, False, True])
    gd.view[written] = 2.0
    gd.assert_untouched(written_rows=written)
    gd.view[4, 3] = 0.0  # a hole of the scatter / a gap row was written
    with pytest.raises(AssertionError, match=r"first at \(row 4, col 3\)"):
        gd.assert_untouched(written_rows=written)


def test_nan_read_from_input_padding_is_flagged():
    """A K tail 'masked' by multiplying with zero instead of by select: finite on ordinary neighbouring data, NaN on
    a Guarded input, which assert_finite and assert_elementwise both report."""
    a, w, bias = kc.int_gemm_operands(9, 16, 32, torch.bfloat16)
    ga = kc.Guarded(9, 32, torch.bfloat16).fill(a)
    gw = kc.Guarded(16, 32, torch.bfloat16, pad=24).fill(w)
    ref = a.double() @ w.double().t()
    good = ga.view.float() @ gw.view.float().t()
    kc.assert_finite(good)
    assert kc.assert_elementwise(good, ref, 0.0) == 0.0
    # the defect: one more K column is loaded from the padding and multiplied by a zero weight
    a_over = ga.buf[ga.g:ga.g + 9, :33].float()
    w_over = torch.cat([gw.view.float(), torch.zeros(16, 1)], dim=1)
    bad = a_over @ w_over.t()
    with pytest.raises(AssertionError, match="non-finite"):
        kc.assert_finite(bad)
    with pytest.raises(AssertionError, match="beyond their bound"):
        kc.assert_elementwise(bad, ref, 1.0)


# ------------------------------------------------------------------------------------------------ GEMM bounds
SHAPES = [(333, 512, 192), (300, 256, 4096)]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_dot_bound_holds_for_the_fp32_accumulating_emulation(m, n, k, dtype):
    a, w, bias = _gauss(m, n, k, dtype, seed=m + k)
    ref = a.double() @ w.double().t() + bias.double()
    for odt in (torch.float32, dtype):
        out = kc.gemm_emulation(a, w, bias, odt)
        ratio = kc.assert_elementwise(out, ref, kc.dot_bound(a, w, bias, k, odt), f"{odt}")
        assert 0.0 < ratio <= 1.0
        if odt != torch.float32 and k <= 192:  # (at k = 4096 the (k + 1) 2^-23 accumulation term takes over)
            assert ratio > 0.5, "a short K leaves the output rounding alone: the 16-bit bound must be sharp"


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("defect,m,n,k", [("dropped_k_slice", 333, 512, 192), ("dropped_k_slice", 300, 256, 4096),
                                          ("scaled_row", 333, 512, 192)])
def test_dot_bound_flags_planted_gemm_defects(defect, m, n, k, dtype):
    """The two defects of the issue in one row of the accumulator: hundreds of violations in that row at k = 192,
    where the bound is sharp (the lost slice also at k = 4096; a row scaled by 1 + 2^-7 hides below the accumulation
    term there, which is why the GPU tests use a short K), while the whole-tensor relative L2 error stays below the
    older tests' 4e-3 bar (the scaled row; the lost 32-wide slice at k = 4096, where it is 1 / 128 of the row)."""
    a, w, bias = _gauss(m, n, k, dtype, seed=7)
    ref = a.double() @ w.double().t() + bias.double()
    kw = {"drop_slice": (200, 3)} if defect == "dropped_k_slice" else {"scale_row": (200, 1 + 2.0 ** -7)}
    out = kc.gemm_emulation(a, w, bias, dtype, **kw)
    if defect == "scaled_row" or k == 4096:
        assert float((out.double() - ref).norm() / ref.norm()) < 4e-3, "invisible to the whole-tensor bar"
    bound = kc.dot_bound(a, w, bias, k, dtype)
    with pytest.raises(AssertionError, match=r" (\d{3}) of \d+ elements beyond their bound; worst at \(200, "):
        kc.assert_elementwise(out, ref, bound, defect)
    keep = torch.arange(m) != 200  # the other rows are clean
    kc.assert_elementwise(out[keep], ref[keep], bound[keep])


@pytest.mark.parametrize("dtype", HALF)
def test_integer_operands_are_exact_in_any_order(dtype):
    m, n, k = 65, 256, 4096
    a, w, bias = kc.int_gemm_operands(m, n, k, dtype, seed=3)
    assert torch.equal(a.float(), a.float().round()) and int(a.abs().max()) == 3 and int(w.abs().max()) == 3
    ref = a.double() @ w.double().t() + bias.double()
    fwd = kc.gemm_emulation(a, w, bias, torch.float32)
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(1))
    rev = kc.gemm_emulation(a[:, perm], w[:, perm], bias, torch.float32, chunk=64)
    assert torch.equal(fwd.double(), ref) and torch.equal(rev, fwd)
    assert torch.equal(kc.gemm_emulation(a, w, bias, dtype), ref.to(dtype))
    # and torch.equal sees both planted defects
    assert not torch.equal(kc.gemm_emulation(a, w, bias, torch.float32, drop_slice=(64, 127)).double(), ref)
    assert not torch.equal(kc.gemm_emulation(a, w, bias, dtype, scale_row=(0, 1 + 2.0 ** -7)), ref.to(dtype))


@pytest.mark.parametrize("dtype", HALF)
def test_swiglu_bound(dtype):
    m, f, k = 77, 256, 192
    a, w1, _ = _gauss(m, f, k, dtype, seed=11)
    _, w3, _ = _gauss(m, f, k, dtype, seed=12)
    g = kc.gemm_emulation(a, w1, None, torch.float32)
    u = kc.gemm_emulation(a, w3, None, torch.float32)
    ref = kc.swiglu_ref(a, w1, w3)
    bound = kc.swiglu_bound(a, w1, w3, k, dtype)
    out = (torch.nn.functional.silu(g) * u).to(dtype)
    assert 0.0 < kc.assert_elementwise(out, ref, bound) <= 1.0
    bad = out.clone()
    bad[5] = (bad[5].float() * (1 + 2.0 ** -7)).to(dtype)
    with pytest.raises(AssertionError, match=r"worst at \(5, "):
        kc.assert_elementwise(bad, ref, bound)
    wi = kc.interleave_swiglu(w1, w3)
    assert torch.equal(wi[:16], w1[:16]) and torch.equal(wi[16:32], w3[:16]) and torch.equal(wi[32:48], w1[16:32])


# ------------------------------------------------------------------------------------------------ attention
def _counting_case(k_len, coarse, out_dtype, **defect):
    H = 2
    v = kc.onehot_v(k_len + 5, H, coarse)  # (the rows after the problem carry their own code)
    q = torch.zeros(3, H * 128, dtype=torch.bfloat16)
    k = torch.randn(k_len, H * 128).bfloat16()  # q = 0: the keys' values do not matter
    out = kc.attention_emulation(q, k, v[:k_len], H, torch.bfloat16, out_dtype, **defect)
    exp, bound = kc.weighted_onehot_expected(v[:k_len], None, out_dtype)
    return out, exp.expand(3, -1), bound.expand(3, -1)


@pytest.mark.parametrize("out_dtype", HALF)
@pytest.mark.parametrize("k_len", [1, 63, 65, 129, 1000])
def test_counting_form_clean(k_len, out_dtype):
    for coarse in (False, True):
        out, exp, bound = _counting_case(k_len, coarse, out_dtype)
        kc.assert_elementwise(out, exp, bound)
        assert (out[:, exp[0] == 0] == 0).all()


@pytest.mark.parametrize("out_dtype", HALF)
@pytest.mark.parametrize("defect", ["dup", "drop"])
def test_counting_form_flags_one_key(defect, out_dtype):
    """The last key of a 1,000-key problem counted twice, or dropped, in one query row: one channel moves by about
    1 / k_len (12 % of its value with 8 keys a channel), far outside (u_out + 2^-18) of it."""
    out, exp, bound = _counting_case(1000, False, out_dtype, **{defect: (1, 999)})
    with pytest.raises(AssertionError, match=r"worst at \(1, "):
        kc.assert_elementwise(out, exp, bound)
    kc.assert_elementwise(out[[0, 2]], exp[[0, 2]], bound[[0, 2]])


def test_counting_form_flags_a_leaked_neighbour_key():
    """One key past k_len attended to (a tail mask off by one): its fine code may collide with a counted channel, the
    coarse code of the same launch pair may not; either way a channel moves by 1 / (k_len + 1)."""
    H, k_len = 2, 200
    v = kc.onehot_v(k_len + 5, H, False)
    q = torch.zeros(2, H * 128, dtype=torch.bfloat16)
    out = kc.attention_emulation(q, torch.zeros(k_len + 1, H * 128), v[:k_len + 1], H, torch.bfloat16, torch.bfloat16)
    exp, bound = kc.weighted_onehot_expected(v[:k_len], None, torch.bfloat16)
    with pytest.raises(AssertionError, match="beyond their bound"):
        kc.assert_elementwise(out, exp.expand(2, -1), bound.expand(2, -1))


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("defect", [None, "dup", "drop"])
def test_exact_exponent_form(defect, dtype):
    H, k_len = 2, 700
    e = kc.exponent_keys(k_len, seed=5, spikes=[(5, -6), (64, -2), (640, 0), (699, -1)])
    assert int(e.min()) >= -12 and int(e.max()) == 0
    q, k = kc.exact_exponent_qk(4, k_len, H, e, dtype)
    v = kc.onehot_v(k_len, H, False, dtype)
    s = q.double().view(4, H, 128).transpose(0, 1) @ k.double().view(k_len, H, 128).transpose(0, 1).transpose(1, 2)
    assert torch.equal(s, e.double().expand(H, 4, k_len)), "every score is the integer exponent"
    kw = {} if defect is None else {defect: (2, 640 if defect == "drop" else 3)}  # the largest key / a plateau key
    out = kc.attention_emulation(q, k, v, H, dtype, dtype, log2_scores=True, **kw)
    exp, bound = kc.weighted_onehot_expected(v, e, dtype)
    # every weight is a power of two within 12 binades: P is exact in either operand type
    p = torch.exp2(e.double() - e.max())
    assert torch.equal(p.to(dtype).double(), p)
    if defect is None:
        kc.assert_elementwise(out, exp.expand(4, -1), bound.expand(4, -1))
    else:
        with pytest.raises(AssertionError, match=r"worst at \(2, "):
            kc.assert_elementwise(out, exp.expand(4, -1), bound.expand(4, -1))


@pytest.mark.parametrize("dtype", HALF)
def test_per_row_bar_flags_a_key_counted_twice(dtype):
    """The per-row form: Gaussian q/k/v, max over rows of the relative row error against fp64.  The emulation (P
    rounded to the operand type, O to the output type) sets the bar; a key counted twice in one row of a 1,000-key
    problem is several times 2x that bar while the whole-tensor error stays below the older tests' 6e-3."""
    H, n = 2, 1000
    g = torch.Generator(device="cpu").manual_seed(9)
    q, k, v = [torch.randn(n if i else 64, H * 128, generator=g).to(dtype) for i in range(3)]
    ref = kc.attention_ref(q, k, v, H)
    emu = kc.worst_row_relerr(kc.attention_emulation(q, k, v, H, dtype, dtype), ref)
    assert 0 < emu < (4e-3 if dtype == torch.bfloat16 else 6e-4)
    bad = kc.attention_emulation(q, k, v, H, dtype, dtype, dup=(17, n - 1))  # the last key, as a tail re-read would
    assert float((bad.double() - ref).norm() / ref.norm()) < 6e-3
    assert kc.worst_row_relerr(bad, ref) > 2 * emu


def test_swin_attend_matches_roll_partition_and_mask():
    """swin_attend (token-pair form) against the oracle's roll + window partition + rf_ref.swin_mask on a one-hot
    probe: attention over windows with uniform weights must spread each token over exactly the tokens it attends."""
    from oracle import rf_ref
    for gh, gw, shift in [(8, 8, 0), (8, 8, 4), (16, 8, 4), (8, 24, 4), (8, 24, 0)]:
        att = kc.swin_attend(gh, gw, 8, shift)
        t = gh * gw
        assert att.shape == (t, t) and torch.equal(att, att.t()) and bool(att.diagonal().all())
        x = torch.eye(t).view(1, gh, gw, t)
        if shift:
            x = torch.roll(x, (-shift, -shift), (1, 2))
        win = x.view(1, gh // 8, 8, gw // 8, 8, t).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, t)
        mask = rf_ref.swin_mask(gh, gw, 8, shift).double() if shift else torch.ones(win.shape[0], 64, 64,
                                                                                     dtype=torch.float64)
        o = (mask @ win.double()).reshape(1, gh // 8, gw // 8, 8, 8, t).permute(0, 1, 3, 2, 4, 5).reshape(1, gh, gw, t)
        if shift:
            o = torch.roll(o, (shift, shift), (1, 2))
        assert torch.equal(o.reshape(t, t) > 0, att), (gh, gw, shift)
        if shift == 0:
            assert int(att.sum(1).min()) == int(att.sum(1).max()) == 64
        else:
            assert int(att.sum(1).min()) < 64


# ------------------------------------------------------------------------------------------------ convolutions
def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_int_conv_operands_are_exact_in_fp32():
    """3x3, cin 512: every partial sum stays an integer below 2^24 (bound 9 * 9 * 512 + 3 * 8 = 41,496; the largest
    |v| of this draw is about 1,100), so the fp32 convolution equals the fp64 one bit for bit, in another summation
    order (the emulation adds the bias and residuals after the taps) too; the planes are that value rounded once."""
    x, w, b, r1, r2 = kc.int_conv_operands(2, 512, 64, 3, 3, 8, 8, seed=1, pad=1)
    ref = kc.conv_ref(x, w, b, r1, r2, pad=1)
    assert 1000 < float(ref.abs().max()) < 3 * 3 * 9 * 512 + 24
    assert torch.equal(ref, ref.round()) and ref.dtype == torch.float64
    assert torch.equal(kc.conv_emulation(x, w, b, r1, r2).double(), ref)
    halves = kc.conv_emulation(x[:, :256], w[:, :256]) + kc.conv_emulation(x[:, 256:], w[:, 256:], b, r1, r2)
    assert torch.equal(halves.double(), ref)  # a two-way split of K
    hi, lo = kc.exact_planes(ref, f16=True)
    assert lo is None and torch.equal(hi.double(), ref)  # |v| <= 2,048: fp16 holds these integers exactly
    big = ref * 37.0  # up to about 41,000: fp16 rounds (spacing 32), bf16 hi + lo holds 16 bits
    hi, lo = kc.exact_planes(big, f16=False)
    assert not torch.equal(hi.double(), big) and float((hi.double() + lo.double() - big).abs().max()) <= 2 ** -16 * 41496
    with pytest.raises(AssertionError):
        kc.int_conv_operands(1, 2048, 4, 3, 3, 4, 4, amax=32)  # 1,024 * 9 * 2,048 > 2^24
    xd, wd, bd, _, _ = kc.int_conv_operands(2, 64, 16, 1, 1, 3, 5, seed=2, deconv=4)
    rd = kc.conv_ref(xd, wd, bd, deconv=4)
    assert rd.shape == (2, 12, 20, 16) and torch.equal(rd, rd.round())


def test_tap_mask_names_the_taps():
    x, w, b9 = kc.tap_mask_operands(2, 32, 64, 3, 3, 4, 5)
    m = kc.conv_ref(x, w, None, pad=1)
    assert (m[:, 1:-1, 1:-1] == 511).all()
    # corners and edges: the taps that read the zero border are missing (tap t = 3 ty + tx has the value 2^t)
    assert [int(m[1, y, x_, 33]) for y, x_ in ((0, 0), (0, 2), (0, 4), (2, 0), (3, 0), (3, 4))] == \
        [432, 504, 216, 438, 54, 27]
    mb = kc.conv_ref(x, w, b9, pad=1)
    assert torch.equal(mb - m, (1024.0 * (kc.border_classes(4, 5) + 1))[None, :, :, None].expand_as(m).double())
    xd, wd, _ = kc.tap_mask_operands(1, 32, 64, 1, 1, 2, 3, deconv=2)
    md = kc.conv_ref(xd, wd, None, deconv=2)
    assert torch.equal(md[0, :, :, 40], torch.tensor([[1., 2.] * 3, [4., 8.] * 3] * 2, dtype=torch.float64))
    assert kc.decode_tap_mask(511, 513, 3, 3) == "tap (0, 1) counted 2 times, expected 1"
    assert kc.decode_tap_mask(511, 447, 3, 3) == "tap (2, 0) counted 0 times, expected 1"
    assert kc.decode_tap_mask(432, 438, 3, 3) == \
        "tap (0, 1) counted from the padding; tap (0, 2) counted from the padding"
    assert kc.decode_tap_mask(1024 * 5 + 511, 1024 * 4 + 511, 3, 3, border=True) == "border class 3 instead of 4"
    kc.assert_tap_mask(m.float(), m, 3, 3)
    bad = m.clone()
    bad[1, 0, 4, 96 % 64] += 2.0
    with pytest.raises(AssertionError, match=r"image 1, pixel \(0, 4\), filter 32: tap \(0, 1\) counted 1 times, expected 0"):
        kc.assert_tap_mask(bad, m, 3, 3, what="planted")


DEFECTS = ["dropped_chunk", "halo_column_zero", "previous_image_row", "wrong_border_class", "store_past_cout"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_conv_planted_defect_is_flagged(defect):
    """Each defect of conv_emulation against the assertion the GPU tests make: the exact form (torch.equal with the
    fp64 reference), the tap mask with its decoded message, and the guard band."""
    n, cin, cout, h, w = 2, 64, 32, 6, 16
    x, wt, b, r1, r2 = kc.int_conv_operands(n, cin, cout, 3, 3, h, w, seed=3, pad=1)
    ref = kc.conv_ref(x, wt, b, r1, r2, pad=1)
    assert torch.equal(kc.conv_emulation(x, wt, b, r1, r2).double(), ref)
    xm, wm, b9 = kc.tap_mask_operands(n, cin, cout, 3, 3, h, w)
    mask = kc.conv_ref(xm, wm, None, pad=1)
    kc.assert_tap_mask(kc.conv_emulation(xm, wm), mask, 3, 3)
    if defect == "dropped_chunk":
        assert not torch.equal(kc.conv_emulation(x, wt, b, r1, r2, drop_chunk=(1, 2, 7, 5, 1)).double(), ref)
        with pytest.raises(AssertionError, match=r"image 1, pixel \(2, 7\), filter 32: tap \(1, 2\) counted 0 times"):
            # (filters 32 .. 63 read channels 32 .. 63, chunk 1)
            xm2, wm2, _ = kc.tap_mask_operands(n, cin, 64, 3, 3, h, w)
            kc.assert_tap_mask(kc.conv_emulation(xm2, wm2, drop_chunk=(1, 2, 7, 5, 1)),
                               kc.conv_ref(xm2, wm2, None, pad=1), 3, 3)
    elif defect == "halo_column_zero":
        assert not torch.equal(kc.conv_emulation(x, wt, b, r1, r2, halo_col_zero=8).double(), ref)
        with pytest.raises(AssertionError, match=r"image 0, pixel \(0, 8\), filter 0: tap \(1, 0\) missing; tap \(2, 0\) "
                                                 r"missing"):
            kc.assert_tap_mask(kc.conv_emulation(xm, wm, halo_col_zero=8), mask, 3, 3)
    elif defect == "previous_image_row":
        assert not torch.equal(kc.conv_emulation(x, wt, b, r1, r2, prev_image_row=1).double(), ref)
        with pytest.raises(AssertionError, match=r"image 1, pixel \(0, 0\), filter 0: tap \(0, 1\) counted from the "
                                                 r"padding; tap \(0, 2\) counted from the padding"):
            kc.assert_tap_mask(kc.conv_emulation(xm, wm, prev_image_row=1), mask, 3, 3)
    elif defect == "wrong_border_class":
        maskb = kc.conv_ref(xm, wm, b9, pad=1)
        kc.assert_tap_mask(kc.conv_emulation(xm, wm, b9), maskb, 3, 3, border=True)
        with pytest.raises(AssertionError, match=r"image 0, pixel \(5, 15\), filter 0: border class 7 instead of 8"):
            kc.assert_tap_mask(kc.conv_emulation(xm, wm, b9, wrong_class=(5, 15, 7)), maskb, 3, 3, border=True)
    else:
        vals = ref.reshape(-1, cout)
        for g_ in (kc.Guarded(vals.shape[0], cout, torch.float32, g=256, ld=cout),            # dense out: guard rows
                   kc.Guarded(vals.shape[0], cout, torch.float16, g=256, ld=cout + 8, col_off=4)):  # planes: ld padding
            kc.emulated_store(g_, vals).assert_untouched()
            assert torch.equal(g_.view.double(), vals)
            with pytest.raises(AssertionError, match=rf"first at \(row {vals.shape[0] if g_.ld == cout else vals.shape[0] - 1}"
                                                     rf", col {0 if g_.ld == cout else cout}\)"):
                kc.emulated_store(g_.reset(), vals, past_cout=True).assert_untouched(what=defect)
        # what the suite had: padding columns the caller zeroed compared with zero -- the stray store of zeros passes
        pl = torch.zeros(vals.shape[0], cout + 8, dtype=torch.float16)
        pl[:, :cout] = vals.half()
        pl[-1, cout:cout + 4] = 0
        assert (pl[:, cout:] == 0).all()


@pytest.mark.parametrize("cin,cout,hh,ww,n_img,score", [(256, 256, 64, 64, 1, 6.03e-4), (256, 128, 32, 64, 2, 8.09e-4)])
def test_one_pixel_defect_passes_the_plane_bar_and_fails_the_bound(cin, cout, hh, ww, n_img, score):
    """test_conv_halo2's operands at two of its shapes (randn weights / sqrt(9 cin), bias, two residuals, SiLU fp16
    planes), one 32-channel chunk of the centre tap missing at the centre pixel of the last image, for every filter.
    Measured whole-tensor relative L2 of the SiLU planes against fp64:
        (256, 256, 64, 64, 1): 6.03e-4 with the defect, 2.08e-4 without (fp16 rounding alone); fp32 out 5.4e-4
        (256, 128, 32, 64, 2): 8.09e-4 with the defect, 2.08e-4 without;                       fp32 out 6.9e-4
    (other pixels score 6e-4 to 1.0e-3): the defect passes the suite's `relerr < 1e-3` plane bar -- and fails
    assert_elementwise with conv_bound at about 200 / 80 elements, all of that pixel, while the clean emulation stays
    within 0.4 of the bound."""
    import torch.nn.functional as F
    g = torch.Generator(device="cpu").manual_seed(cin * hh + cout + ww)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g)
    x = torch.randn(n_img, cin, hh, ww, generator=g)
    r1 = torch.randn(n_img, hh, ww, cout, generator=g)
    r2 = torch.randn(n_img, hh, ww, cout, generator=g)
    sx, wq = F.silu(x.double()).float().half().double(), w.half().double()  # the operands as the kernel sees them
    ref = kc.conv_ref(sx, wq, b, r1, r2, pad=1)
    pixel = (n_img - 1, hh // 2, ww // 2)
    bad = F.silu(kc.conv_emulation(sx, wq, b, r1, r2, drop_chunk=(*pixel, 4, 3))).half()
    good = F.silu(kc.conv_emulation(sx, wq, b, r1, r2)).half()
    e_bad, e_good = relerr(bad, F.silu(ref)), relerr(good, F.silu(ref))
    print(f"planes relerr: planted defect {e_bad:.3e}, clean {e_good:.3e}")
    assert e_good < 2.2e-4 and abs(e_bad - score) < 0.02 * score and e_bad < 1e-3  # the old bar passes the defect
    bound = kc.conv_bound(sx, wq, b, r1, r2, 9 * cin, torch.float16, silu=True, pad=1, ref=ref)
    assert kc.assert_elementwise(good, F.silu(ref), bound, "clean") < 0.5
    with pytest.raises(AssertionError, match=rf"worst at \({pixel[0]}, {pixel[1]}, {pixel[2]}, "):
        kc.assert_elementwise(bad, F.silu(ref), bound, "planted")


def test_conv_bound_terms():
    """conv_bound on a case small enough to check by hand: one pixel, one tap, two channels."""
    x = torch.tensor([1.0, -2.0]).view(1, 2, 1, 1)
    w = torch.tensor([0.5, 0.25]).view(1, 2, 1, 1)
    b, r1 = torch.tensor([-1.0]), torch.full((1, 1, 1, 1), 3.0)
    mag = 0.5 + 0.5 + 1.0 + 3.0  # |x| |w| + |bias| + |res1|; ref = 0.5 - 0.5 - 1 + 3 = 2
    e = (2 + 3) * 2.0 ** -23 * mag
    assert float(kc.conv_bound(x, w, b, r1, None, 2, torch.float32)) == pytest.approx(e, rel=1e-12)
    assert float(kc.conv_bound(x, w, b, r1, None, 2, torch.float16)) == \
        pytest.approx(e + 2.0 ** -11 * (2.0 + e) + 2.0 ** -25, rel=1e-12)
    s = 2.0 / (1.0 + math.exp(-2.0))
    es = 1.1 * e + 2.0 ** -20 * s
    assert float(kc.conv_bound(x, w, b, r1, None, 2, torch.float16, silu=True)) == \
        pytest.approx(es + 2.0 ** -11 * (s + es) + 2.0 ** -25, rel=1e-12)
    assert float(kc.conv_bound(x, w, b, r1, None, 2, torch.float32, operand_rel=2.0 ** -16)) == \
        pytest.approx(e + 2.0 ** -16 * 1.0, rel=1e-12)


# ------------------------------------------------------------------------------------------------ prologue and output
# The references, bounds and emulations of the prologue kernels, at the shapes tests/test_prologue_exact_gpu.py runs:
# every clean emulation passes its check, every planted defect fails it, and the fp32 oracle (which the goldens pin to
# the reference project) lies inside the bounds of the fp64 references.
def _vn_check(out, vn, dst, written, n_freqs, ld, dtype, what=""):
    ref = kc.vn_scatter(kc.vn_encode_ref(vn, n_freqs, ld), dst)
    bound = kc.vn_scatter(kc.vn_encode_bound(vn, n_freqs, ld, dtype), dst)
    return kc.assert_elementwise(out[written], ref[written], bound[written], what)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("n_freqs,ld", kc.VN_SHAPES)
@pytest.mark.parametrize("n_rows", kc.VN_ROWS)
def test_vn_encode_emulation_and_its_planted_defects(n_rows, n_freqs, ld, dtype):
    vn, dst, written = kc.vn_case(n_rows)
    assert n_rows == 1 or not bool(written.all()), "the case must have holes"
    clean = kc.vn_scatter(kc.vn_encode_emulation(vn, n_freqs, ld, dtype), dst)
    ratio = _vn_check(clean, vn, dst, written, n_freqs, ld, dtype, "clean")
    assert 0.0 < ratio <= 1.0
    defects = [{"freq_off_by_one": 8}, {"swap_sin_cos": True}]
    if ld > 9 * (2 * n_freqs + 1):
        defects.append({"dirty_padding": True})
    for kw in defects:
        bad = kc.vn_scatter(kc.vn_encode_emulation(vn, n_freqs, ld, dtype, **kw), dst)
        with pytest.raises(AssertionError, match="beyond their bound"):
            _vn_check(bad, vn, dst, written, n_freqs, ld, dtype, str(kw))


def test_vn_encode_older_bar_passes_a_wrong_frequency_on_small_values():
    """Why atol = 1e-2 on bf16 was not enough: the frequency index off by one in the lowest level of one input dimension
    moves sin(x) to sin(2 x), which for |x| < 1e-2 is a change below 1e-2 -- and beyond the per-element bound."""
    vn = torch.full((4, 9), 2.0 ** -7)
    bad = kc.vn_encode_emulation(vn, 6, 128, torch.bfloat16, freq_off_by_one=0)
    ref = kc.vn_encode_ref(vn, 6, 128)
    assert float((bad.double() - ref.to(torch.bfloat16).double()).abs()[:, 9].max()) < 1e-2
    with pytest.raises(AssertionError, match="beyond their bound"):
        kc.assert_elementwise(bad, ref, kc.vn_encode_bound(vn, 6, 128, torch.bfloat16))


def test_nerf_encode_oracle_lies_inside_the_vn_bound():
    g = torch.Generator(device="cpu").manual_seed(11)
    v = torch.randn(5000, 3, 3, generator=g)
    vn = (v / v.norm(dim=-1, keepdim=True)).reshape(5000, 9)
    from oracle import rf_ref
    ratio = kc.assert_elementwise(rf_ref.nerf_encode(vn, 6), kc.vn_encode_ref(vn, 6, 117),
                                  kc.vn_encode_bound(vn, 6, 117, torch.float32), "oracle")
    print(f"nerf_encode oracle: worst |err| / bound {ratio:.3f}")
    assert 0.0 < ratio < 0.5


def _centres_f32(rows, **kw):
    return torch.stack([kc.scene_centre_emulation(r, **kw) for r in rows])


@pytest.mark.parametrize("counts,n_views", [(kc.SCENE_COUNTS, 0), (kc.SCENE_COUNTS_VIEWS, 3)])
def test_scene_centre_emulation_and_its_planted_defects(counts, n_views):
    tris, valid, off, c2w = kc.scene_case(counts, n_views)
    rows, centres = kc.scene_pos_ref(tris, valid, off, c2w, n_views, 16)
    e_rows, e_centres = kc.scene_pos_bound(tris, valid, off, c2w, n_views, 16)
    assert len(rows) == len(counts) * max(n_views, 1) and [r.shape[0] for r in rows[::max(n_views, 1)]] == list(counts)
    assert all(bool(torch.isfinite(r).all()) for r in rows), "no hole of the mask among the valid rows"
    f32_rows = [r.float() for r in rows]  # (the kernel's rows, up to their own bound, which e_centres carries)
    ratio = kc.assert_elementwise(_centres_f32(f32_rows), centres, e_centres, "clean")
    assert ratio < 0.5
    empty = counts.index(0) * max(n_views, 1)
    assert float(centres[empty].abs().max()) == 0.0 and float(e_centres[empty].max()) == 0.0  # exactly 0 / 1e-5
    with pytest.raises(AssertionError, match=rf"worst at \({empty}, "):
        kc.assert_elementwise(_centres_f32(f32_rows, divide_by_n=True), centres, e_centres, "divide_by_n")
    if max(counts) > 64 * 256:
        with pytest.raises(AssertionError, match=r"worst at \(0, "):
            kc.assert_elementwise(_centres_f32(f32_rows, drop_second_round=True), centres, e_centres, "second round")


def test_oracle_positions_lie_inside_the_scene_bounds():
    """rf_ref.center_pos (no c2w, 66 blocks) and rf_ref.cam_transform + center_pos (3 views) against scene_pos_ref."""
    from oracle import rf_ref
    for counts, n_views in ((kc.SCENE_COUNTS, 0), (kc.SCENE_COUNTS_VIEWS, 3)):
        tris, valid, off, c2w = kc.scene_case(counts, n_views)
        rows, centres = kc.scene_pos_ref(tris, valid, off, c2w, n_views, 16)
        e_rows, e_centres = kc.scene_pos_bound(tris, valid, off, c2w, n_views, 16)
        nmax, v = max(counts), max(n_views, 1)
        pos = torch.zeros(len(counts), nmax, 9)
        mask = torch.zeros(len(counts), nmax, dtype=torch.bool)
        for b, n in enumerate(counts):
            pos[b, :n] = tris[valid[int(off[b]):int(off[b + 1])].long()]
            mask[b, :n] = True
        if n_views:
            pos = rf_ref.cam_transform(c2w, torch.repeat_interleave(pos, v, 0).view(-1, nmax, 3, 3)).reshape(-1, nmax, 9)
            mask = torch.repeat_interleave(mask, v, 0)
        got, _ = rf_ref.center_pos(pos * mask[..., None], mask, 16)
        for s, r in enumerate(rows):
            n = r.shape[0]
            worst_r = kc.assert_elementwise(got[s, 16:16 + n], r, e_rows[s], f"oracle rows of set {s}")
            worst_c = kc.assert_elementwise(got[s, :16], centres[s].repeat(3).expand(16, 9),
                                            e_centres[s].repeat(3).expand(16, 9), f"oracle centre of set {s}")
            assert worst_c <= 0.5 and worst_r <= 0.5


@pytest.mark.parametrize("log_decode", [True, False])
@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("n,h,w", kc.HDR_SHAPES)
def test_hdr_emulation_and_its_planted_defects(n, h, w, c, channels_last, log_decode):
    x = kc.hdr_logits(n, c, h, w)
    ref, bound = kc.hdr_ref(x, 1e-3, log_decode, channels_last), kc.hdr_bound(x, 1e-3, log_decode, channels_last)
    assert ref.shape == ((n, h, w, c) if channels_last else (n, c, h, w))
    ratio = kc.assert_elementwise(kc.hdr_emulation(x, 1e-3, log_decode, channels_last), ref, bound, "clean")
    assert ratio <= 1.0
    if n * h * w * c >= 5:  # (an element of the negative branch is among the specials)
        with pytest.raises(AssertionError, match="beyond their bound"):
            kc.assert_elementwise(kc.hdr_emulation(x, 1e-3, log_decode, channels_last, exp_for_expm1=True), ref, bound)
    if channels_last and c > 1 and h * w > 1:
        with pytest.raises(AssertionError, match="beyond their bound"):
            kc.assert_elementwise(kc.hdr_emulation(x, 1e-3, log_decode, True, wrong_layout_index=True), ref, bound)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("rows,channels,n", kc.TEXTURE_LINEAR_SHAPES)
def test_texture_linear_emulation_and_its_planted_defects(rows, channels, n, with_bias):
    coef, wsum, bias = kc.texture_linear_case(rows, channels, n)
    bias = bias if with_bias else None
    ref, bound = kc.texture_linear_ref(coef, wsum, bias), kc.texture_linear_bound(coef, wsum, bias)
    ratio = kc.assert_elementwise(kc.texture_linear_emulation(coef, wsum, bias), ref, bound, "clean")
    assert 0.0 < ratio <= 0.5
    if rows % 16:
        with pytest.raises(AssertionError, match=rf"worst at \({rows - rows % 16}, "):
            kc.assert_elementwise(kc.texture_linear_emulation(coef, wsum, bias, skip_last_partial_block=True), ref, bound)
    bad = kc.texture_linear_emulation(coef, wsum, bias, bias_per_trip=True)
    if n > 1024 and with_bias:
        with pytest.raises(AssertionError, match=r"worst at \(\d+, 1\d{3}\)"):
            kc.assert_elementwise(bad, ref, bound)
        kc.assert_elementwise(bad[:, :1024], ref[:, :1024], bound[:, :1024])  # the first trip is clean
    else:
        kc.assert_elementwise(bad, ref, bound)  # nothing to see without a second trip or a bias


def test_texture_linear_defects_are_each_reached_by_a_gpu_shape():
    shapes = kc.TEXTURE_LINEAR_SHAPES
    assert any(n > 1024 for _, _, n in shapes) and any(r % 16 for r, _, _ in shapes) and any(r % 16 == 0 for r, _, _ in shapes)
    assert {c for _, c, _ in shapes} >= {1, 16} and any(n < 1024 for _, _, n in shapes)


def test_ray_gen_oracle_lies_inside_the_ray_bound():
    """rf_ref.ray_gen (square frames, fov) against ray_tokens_ref; and the overscan identity of the reference itself:
    the token frame's rays are the requested frame's rays where the two overlap."""
    from oracle import rf_ref
    c2w, fov, intr = kc.camera_case(3)
    res, p = 24, 8
    ro, rd = rf_ref.ray_gen(c2w, (fov / 180.0 * torch.pi)[:, None], res)
    tok, pos, bound = kc.ray_tokens_ref(c2w, fov, None, (res, res), (res, res), (0, 0), p, torch.float32)
    ratio = kc.assert_elementwise(kc.patchify_ref(rd, p), tok, bound, "oracle rays")
    print(f"ray_gen oracle: worst |err| / bound {ratio:.3f}")
    assert 0.0 < ratio <= 0.5
    assert torch.equal(ro.repeat(1, 3).double(), pos)
    inner, _, _ = kc.ray_tokens_ref(c2w, None, intr, (8, 24), (8, 24), (0, 0), p)
    outer, _, _ = kc.ray_tokens_ref(c2w, None, intr, (8, 24), (24, 40), (8, 8), p)
    assert torch.equal(outer.view(3, 3, 5, -1)[:, 1, 1:4], inner.view(3, 1, 3, -1)[:, 0])


def test_ray_bound_flags_a_transposed_rotation_and_a_shifted_principal_point():
    c2w, fov, intr = kc.camera_case(3)
    for dtype in HALF:
        tok, _, bound = kc.ray_tokens_ref(c2w, None, intr, (8, 24), (24, 40), (8, 8), 8, dtype)
        kc.assert_elementwise(tok.to(dtype), tok, bound, "rounded reference")
        c2w_t = c2w.clone()
        c2w_t[:, :3, :3] = c2w[:, :3, :3].transpose(1, 2)
        for bad in (kc.ray_tokens_ref(c2w_t, None, intr, (8, 24), (24, 40), (8, 8), 8)[0],
                    kc.ray_tokens_ref(c2w, None, intr, (8, 24), (24, 40), (8, 7), 8)[0]):
            with pytest.raises(AssertionError, match="beyond their bound"):
                kc.assert_elementwise(bad.to(dtype), tok, bound)
