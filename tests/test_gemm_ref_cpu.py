"""The GEMM checker and references of tests/helpers/gemm_ref.py bite: float64 / numpy "kernels" with ONE defect each must be rejected by
check_exact (tolerance 0, integer operands) or by the rounding-regime bound, several of them pass the criteria the suite had before
(whole-tensor `rel L2 < 4e-3` for bf16 outputs, `dbias` to 1.5e-2 of its norm), and the properties the exact regime rests on hold."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_mask as AM  # noqa: E402
import gemm_ref as GR  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
BM, BN = 128, 64                   # the macro-tile the defects are placed against
M, N, K = 136, 72, 200             # ragged against it: last row tile has 8 rows, last column tile 8 columns, K has a tail of 8
SEED = 0x5EED1234


def ints(shape, amp, seed):
    return torch.randint(-amp, amp + 1, shape, generator=torch.Generator().manual_seed(seed)).to(BF16)


@pytest.fixture(scope="module")
def case():
    a, b = ints((M, K), 15, 1), ints((N, K), 15, 2)
    acc, absprod = GR.product(a, b, 0, 0)
    bias = torch.randint(-64, 65, (N,), generator=torch.Generator().manual_seed(3)).float()
    GR.assert_exact_regime(absprod, bias=bias, scale=2.0, slope=0.25, dbias_rows=True, what="cpu case")
    return a.double().numpy(), b.double().numpy(), acc, absprod, bias


def filled(ref, dtype, ld=None, rows_after=2):
    """what a correct kernel leaves in a poisoned buffer"""
    m, n = ref.shape
    buf = GR.poisoned(m, n, n + 8 if ld is None else ld, dtype, rows_after)
    buf[:m, :n] = torch.from_numpy(np.ascontiguousarray(ref)).to(dtype)
    return buf


def rejected(buf, ref, **kw):
    with pytest.raises(GR.Mismatch) as e:
        GR.check_exact(buf, ref, tile=(BM, BN), what="mutant", **kw)
    return str(e.value)


# ------------------------------------------------------------------------------------------------------------------ the checker accepts the truth
def test_correct_results_pass(case):
    a, b, acc, absprod, bias = case
    GR.check_exact(filled(acc, F32), acc, tile=(BM, BN))
    GR.check_exact(filled(acc, BF16), acc, tile=(BM, BN))
    keep = GR.keep_elementwise(M, N, 0.5, SEED)
    y = GR.mode1(acc, bias, 0.25, keep, 0.5)
    GR.check_exact(filled(y, BF16), y, tile=(BM, BN))


# ------------------------------------------------------------------------------------------------------------------ one defect each
def test_dropped_k_term_in_one_element(case):
    a, b, acc, absprod, bias = case
    m, n = M - 1, N - 1                                    # the corner of the ragged edge tile
    k = int(np.nonzero(a[m] * b[n])[0][-1])
    bad = acc.copy()
    bad[m, n] -= a[m, k] * b[n, k]
    msg = rejected(filled(bad, F32), acc)
    assert "1 of" in msg and f"(m={m}, n={n})" in msg and "tile (row 1, col 1)" in msg
    # a bf16 output shows it wherever the term exceeds half an ulp of the result: K = 8 keeps every sum below 2^8 * 8, take |sum| < 256
    a8, b8 = a[:, :8], b[:, :8]
    acc8 = a8 @ b8.T
    mm, nn = np.nonzero((np.abs(acc8) < 128) & ((a8[:, 7:8] * b8[None, :, 7]) != 0))
    bad8 = acc8.copy()
    bad8[mm[0], nn[0]] -= a8[mm[0], 7] * b8[nn[0], 7]
    rejected(filled(bad8, BF16), acc8)


def test_last_chunk_of_ragged_tile_left_unwritten(case):
    a, b, acc, absprod, bias = case
    for dtype in (BF16, F32):
        buf = filled(acc, dtype)
        buf[BM:M, N - 8:N] = float("nan")                  # poison survives in the last 8-column chunk of the corner tile
        msg = rejected(buf, acc)
        assert "64 of" in msg and "tile (row 1, col 1)" in msg


def test_element_written_into_the_ldc_gap(case):
    a, b, acc, absprod, bias = case
    for dtype in (BF16, F32):
        buf = filled(acc, dtype)
        buf[M - 1, N] = 0.0
        assert "guard" in rejected(buf, acc)
        buf = filled(acc, dtype)
        buf[M, 0] = 1.0                                     # a row behind the matrix
        assert "guard" in rejected(buf, acc)


def test_bias_missing_in_last_column_tile(case):
    a, b, acc, absprod, bias = case
    keep = GR.keep_elementwise(M, N, 0.5, SEED)
    ref = GR.mode1(acc, bias, 0.25, keep, 0.5)
    b2 = bias.clone()
    b2[BN:] = 0
    assert (bias[BN:] != 0).any()
    msg = rejected(filled(GR.mode1(acc, b2, 0.25, keep, 0.5), BF16), ref)
    assert "col 1" in msg and "col 0" not in msg


def _keep_variant(M_, N_, p, seed, variant):
    k0, k1 = AM.drop_key(seed)
    idx = np.arange(M_ * N_, dtype=np.uint64)
    h = AM.drop_hash(idx if variant == "idx" else idx >> np.uint64(1), k0, k1)
    odd = (idx & np.uint64(1)) == 1
    if variant == "swapped":
        odd = ~odd
    return (np.where(odd, h >> np.uint32(16), h & np.uint32(0xffff)) >= AM.thr16(p)).reshape(M_, N_)


@pytest.mark.parametrize("variant", ["idx", "swapped"])
def test_wrong_keep_bits(case, variant):
    a, b, acc, absprod, bias = case
    keep = GR.keep_elementwise(M, N, 0.5, SEED)
    wrong = _keep_variant(M, N, 0.5, SEED, variant)
    assert (keep != wrong).mean() > 0.3
    ref = GR.mode1(acc, bias, 0.25, keep, 0.5)
    rejected(filled(GR.mode1(acc, bias, 0.25, wrong, 0.5), BF16), ref)
    y = torch.from_numpy(ref).to(BF16)
    rejected(filled(GR.mode2(acc, y, 0.25, wrong, 0.5), BF16), GR.mode2(acc, y, 0.25, keep, 0.5))
    rejected(torch.from_numpy(GR.mask_words(wrong, GR.y_negative(y)).astype(np.int32)), GR.mask_words(keep, GR.y_negative(y)))


def test_negative_zero_counted_as_negative(case):
    a, b, acc, absprod, bias = case
    keep = np.ones((M, N), dtype=bool)
    y = torch.from_numpy(GR.mode1(acc, bias, 0.0, keep, 0.0)).to(BF16)      # slope 0: every negative pre-activation is stored as -0.0
    minus_zero = (y.view(torch.int16) == -32768).numpy()
    assert minus_zero.mean() > 0.3 and not GR.y_negative(y)[minus_zero].any()
    ref = GR.mode2(acc, y, 0.25, keep, 0.0)
    bad = np.where(np.signbit(y.double().numpy()), acc * 0.25, acc)           # the sign bit alone
    rejected(filled(bad, BF16), ref)
    rejected(torch.from_numpy(GR.mask_words(keep, np.signbit(y.double().numpy())).astype(np.int32)), GR.mask_words(keep, GR.y_negative(y)))


def test_dbias_summed_after_bf16_rounding(case):
    a, b, acc, absprod, bias = case
    keep = GR.keep_elementwise(M, N, 0.5, SEED)
    y = torch.from_numpy(GR.mode1(acc, bias, 0.25, keep, 0.5)).to(BF16)
    t = GR.mode2(acc, y, 0.25, keep, 0.5)
    ref = GR.dbias(t)[None, :]
    late = torch.from_numpy(t).to(BF16).double().numpy().sum(0)[None, :]
    GR.check_exact(filled(ref, F32, rows_after=0), ref, tile=(BM, BN))
    rejected(filled(late, F32, rows_after=0), ref)


def test_mask_sign_byte_shifted_by_one_element(case):
    a, b, acc, absprod, bias = case
    keep = GR.keep_elementwise(M, N, 0.5, SEED)
    y = torch.from_numpy(GR.mode1(acc, bias, 0.25, keep, 0.5)).to(BF16)
    neg = GR.y_negative(y)
    ref = GR.mask_words(keep, neg)
    assert ref.dtype == np.uint16 and ref.shape == (M, N // 8)
    m, w = 5, 3                                              # the definition, bit by bit
    assert all(((int(ref[m, w]) >> e) & 1) == int(keep[m, 8 * w + e]) and ((int(ref[m, w]) >> (8 + e)) & 1) == int(neg[m, 8 * w + e]) for e in range(8))
    GR.check_exact(torch.from_numpy(ref.astype(np.int32)), ref, tile=(BM, BN // 8))
    rejected(torch.from_numpy(GR.mask_words(keep, np.roll(neg, 1, axis=1)).astype(np.int32)), ref)


def test_split_k_reduction_skips_the_short_last_slab(case):
    a, b, acc, absprod, bias = case
    kchunk = 128                                             # K = 200 in 2 forced splits: slabs of 128 and 72
    slabs = [(a[:, k:k + kchunk].astype(np.float32) @ b[:, k:k + kchunk].astype(np.float32).T) for k in range(0, K, kchunk)]
    assert len(slabs) == 2
    good = (slabs[0] + slabs[1]).astype(np.float64)
    GR.check_exact(filled(good, F32), acc, tile=(BM, BN))
    rejected(filled(slabs[0].astype(np.float64), F32), acc)


# ------------------------------------------------------------------------------------------------------------------ rounding regime
def _gauss(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF16)


def test_rounding_regime_rejects_a_bf16_accumulator():
    Kl = 2048
    a, b = _gauss((96, Kl), 4), _gauss((80, Kl), 5)
    ref, absprod = GR.product(a, b, 0, 0)
    good = (a.float() @ b.float().t())
    u = GR.f32_units(good, ref, absprod)
    assert u < 4.0 and GR.f32_ok(good, ref, absprod, 8.0)          # an fp32 accumulator: a fraction of one unit
    acc = torch.zeros(96, 80, dtype=BF16)
    for k in range(0, Kl, 16):                                     # the same product with the running sum rounded to bf16 every 16 terms
        acc = (acc.float() + a[:, k:k + 16].float() @ b[:, k:k + 16].float().t()).to(BF16)
    ub = GR.f32_units(acc, ref, absprod)
    assert ub > 100 * 8.0 and not GR.f32_ok(acc, ref, absprod, 8.0)
    assert not GR.bf16_ok(acc, ref, absprod, 8.0)                  # as a bf16 output too
    assert GR.bf16_ok(good.to(BF16), ref, absprod, 8.0) and GR.bf16_excess_units(good.to(BF16), ref, absprod) < 8.0


def test_rounding_regime_rejects_rounding_before_the_dropout_scale():
    Mr, Nr, Kr, p = 256, 256, 256, 0.1                             # p = 0.1: the scale 65536 / 58982 is no power of two
    a, b = _gauss((Mr, Kr), 6), _gauss((Nr, Kr), 7)
    acc, absprod = GR.product(a, b, 0, 0)
    keep = GR.keep_elementwise(Mr, Nr, p, SEED)
    ks = GR.keep_scale(p)
    ref = GR.mode1(acc, None, 0.25, keep, p)
    acc32 = (a.float() @ b.float().t()).numpy()
    good = torch.from_numpy(GR.mode1(acc32.astype(np.float64), None, 0.25, keep, p)).to(BF16)
    assert GR.bf16_ok(good, ref, absprod, 8.0, ks)
    early = torch.from_numpy(GR.mode1(acc32.astype(np.float64), None, 0.25, keep, 0.0)).to(BF16)     # rounded to bf16 ...
    early = torch.where(torch.from_numpy(keep), early.float() * np.float32(ks), torch.zeros(())).to(BF16)   # ... then scaled and rounded again
    assert not GR.bf16_ok(early, ref, absprod, 8.0, ks)
    rel = float((early.double() - torch.from_numpy(ref)).norm() / torch.from_numpy(ref).norm())
    assert rel < 4e-3                                               # and the whole-tensor criterion lets it through


# ------------------------------------------------------------------------------------------------------------------ the earlier criteria
def test_defects_that_pass_the_earlier_criteria():
    """At the training shape 8000 x 2048 x 256 with the Gaussian operands of test_gemm_bf16_layouts: `||got - ref|| / ||ref|| < 4e-3` on the
    bf16 output (bf16 rounding alone gives ~1.7e-3) accepts a dropped k-term, a dead row of an edge tile, 8-wide store chunks of stale
    zeros in the corner tile, and truncation instead of rounding; 1.5e-2 of the norm accepts dbias summed after rounding."""
    Mt, Nt, Kt = 8000, 2048, 256
    g = torch.Generator().manual_seed(Mt + Nt + Kt)
    a = torch.randn(Mt, Kt, generator=g).to(BF16)
    b = torch.randn(Nt, Kt, generator=g).to(BF16)
    ref32 = a.float() @ b.float().t()
    ref, nrm = ref32.double(), float(ref32.double().norm())
    good = ref32.to(BF16)
    rel = lambda x: float((x.double() - ref).norm()) / nrm  # noqa: E731
    base = rel(good)
    assert 1e-3 < base < 2.5e-3
    passed = []
    x = ref32.clone()                                               # one k-term dropped in one element
    x[Mt - 1, Nt - 1] -= a[Mt - 1, 7].float() * b[Nt - 1, 7].float()
    passed.append(("k-term", rel(x.to(BF16))))
    x = ref32.clone()                                               # a whole row of the last tile misses its last k-tile
    x[Mt - 1, Nt - 128:] -= a[Mt - 1, 192:].float() @ b[Nt - 128:, 192:].float().t()
    passed.append(("row", rel(x.to(BF16))))
    x = good.clone()                                                # the last 8-wide chunk of eight rows of the last row tile never stored
    x[Mt - 8:, Nt - 8:] = 0
    passed.append(("chunk", rel(x)))
    x = (ref32.view(torch.int32) & -65536).view(torch.float32).to(BF16)   # truncation to bf16 instead of round-to-nearest
    passed.append(("truncate", rel(x)))
    for name, r in passed:
        assert r < 4e-3, (name, r)
        assert r >= base                                            # (each one is a defect, none is closer to the reference)
    assert len(passed) >= 3
    db_ref = ref.sum(0)
    db_late = good.double().sum(0)
    assert float((db_late - db_ref).norm() / db_ref.norm()) < 1.5e-2 and not torch.equal(db_late, db_ref)


# ------------------------------------------------------------------------------------------------------------------ what the exact regime rests on
def test_assert_exact_regime_raises():
    ones = np.full((4, 4), float(1 << 22))
    GR.assert_exact_regime(ones, what="ok")
    GR.assert_exact_regime(ones, scale=2.0, what="ok")
    with pytest.raises(AssertionError, match="2\\^24"):
        GR.assert_exact_regime(ones * 4, what="sum")
    with pytest.raises(AssertionError, match="2\\^24"):
        GR.assert_exact_regime(ones, scale=2.0, slope=0.25, what="scaled")
    with pytest.raises(AssertionError, match="2\\^24"):
        GR.assert_exact_regime(ones, c0=np.full((4, 4), 3.0 * (1 << 22)), what="c0")
    with pytest.raises(AssertionError, match="2\\^24"):
        GR.assert_exact_regime(ones, bias=np.full(4, 3.0 * (1 << 22)), what="bias")
    with pytest.raises(AssertionError, match="dbias"):
        GR.assert_exact_regime(np.full((8, 4), float(1 << 22)), dbias_rows=True, what="dbias")
    with pytest.raises(AssertionError, match="power of two"):
        GR.assert_exact_regime(ones, slope=0.3, what="slope")
    with pytest.raises(AssertionError, match="power of two"):
        GR.assert_exact_regime(ones, scale=GR.keep_scale(0.1), what="p")
    assert GR.keep_scale(0.5) == 2.0 and AM.thr16(0.5) == 32768 and GR.keep_scale(0.0) == 1.0


def test_fp32_product_of_integer_operands_is_the_float64_product():
    a, b = ints((512, 2048), 15, 8), ints((384, 2048), 15, 9)
    ref, absprod = GR.product(a, b, 0, 0)
    GR.assert_exact_regime(absprod, what="fp32 == float64")
    assert np.array_equal((a.float() @ b.float().t()).double().numpy(), ref)
    at = a.t().contiguous()                                         # the layouts of product()
    assert np.array_equal(GR.product(at, b.t().contiguous(), 1, 1)[0], ref) and np.array_equal(GR.product(at, b, 1, 0)[0], ref)


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_keep_share(p):
    Mk, Nk = 512, 1024
    keep = GR.keep_elementwise(Mk, Nk, p, SEED)
    q = 1 - AM.thr16(p) / 65536
    assert abs(keep.mean() - q) < 4 * (q * (1 - q) / (Mk * Nk)) ** 0.5
    assert GR.keep_elementwise(Mk, Nk, 0.0, SEED).all()
    assert (keep != GR.keep_elementwise(Mk, Nk, p, SEED + 1)).mean() > 0.1
    idx = 12345                                                     # the definition on one element, from the scalar twins
    k0, k1 = AM.drop_key(SEED)
    h = int(AM.drop_hash(np.array([idx >> 1]), k0, k1)[0])
    assert bool(keep.reshape(-1)[idx]) == (((h >> 16) if idx & 1 else (h & 0xffff)) >= AM.thr16(p))


@pytest.mark.parametrize("Kc", [256, 1024, 1088])
def test_bf16_cases_need_rounding(Kc):
    """integers in [-15, 15] at K >= 256: at least a quarter of the reference outputs are NOT bf16 numbers, i.e. the exact bf16 cases
    check the rounding (and its direction), not only the sum."""
    a, b = ints((192, Kc), 15, 10), ints((136, Kc), 15, 11)
    ref, _ = GR.product(a, b, 0, 0)
    assert (~GR.bf16_representable(ref)).mean() >= 0.25


def test_kernel_trace_lists_every_selectable_instantiation():
    """profiles/gemm_paths_kernel_stats.csv (the kernel trace of tests/test_gemm_paths_gpu.py on the MI355X) names every GEMM kernel the
    dispatcher can select: 36 register-staged + 34 ring instantiations (the wave-K kernel shadows the 64x64 tt fp32 ring kernels for good),
    both wave-K kernels in their 3 forms, the 10 gemm_big forms and the slab reduction - and not the lab kernel."""
    import csv
    import itertools
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gemm_paths_kernel_stats.csv")
    with open(path, newline="") as f:
        names = "\n".join(r["Name"] for r in csv.DictReader(f))
    tf = lambda v: "true" if v else "false"  # noqa: E731
    want = ["gemm_tt64_wavek_kernel<1>", "gemm_tt64_wavek_kernel<2>", "gemm_nn64_wavek_kernel", "gemm_slab_reduce_kernel"]
    for (bm, bn), ta, tb, om in itertools.product([(128, 128), (128, 64), (64, 64)], [0, 1], [0, 1], [0, 1, 2]):
        want.append(f"gemm_bf16_kernel<{bm}, {bn}, {tf(ta)}, {tf(tb)}, {om}>")
        shadowed = (bm, bn) == (64, 64) and ta and tb and om
        ring = f"gemm_bf16_ring_kernel<{bm}, {bn}, {tf(ta)}, {tf(tb)}, {om}, 3>"
        assert (ring in names) != bool(shadowed), ring
    want += [f"gemm_big_kernel<{bm}, {mode}, {mask}>" for bm in (256, 128) for mode, mask in [(0, "false"), (1, "false"), (2, "false"), (1, "true"), (2, "true")]]
    missing = [w for w in want if w not in names]
    assert not missing, missing
    assert "lab_kernel" not in names
