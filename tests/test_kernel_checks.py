"""The helpers of tests/kernel_checks.py against plain torch emulations of the kernels (CPU only).

The evidence that the exact-arithmetic and guard-band GPU tests can fail: every defect planted in an emulation (a lost
K slice, a scaled row, a key counted twice or dropped, a store into a guard row or the ld padding, a load from the
input padding) is flagged by the helper the GPU tests use, and the unmodified emulation passes every helper.
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
