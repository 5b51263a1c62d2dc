"""float64 references and checkers for the bf16 GEMM kernels (csrc/gemm.hip, csrc/gemm_big.hip). Test infrastructure only.

Two regimes:

  exact     operands are small integers, so every product is exact in fp32 and every partial sum is an integer below 2^24: EVERY fp32
            summation order (MFMA internals, the wave-K partial tiles, split-K slabs and their reduction) gives the same bits, and the
            result must EQUAL the float64 product - a bf16 output must equal that number rounded to nearest-even. The fused epilogues
            stay exact with an integer bias, a power-of-two LeakyReLU slope and dropout p in {0, 0.5} (scale exactly 2).
            assert_exact_regime() proves the precondition from |A|.|B|; check_exact() compares with tolerance 0.
  rounding  Gaussian operands: per-element bounds in units of 2^-24 * (|A|.|B|), see f32_ok / bf16_ok.

Layouts as in include/tsasr_hip.h: A is [M, K] (transA = 0) or [K, M]; B is [N, K] (transB = 0) or [K, N].
The dropout keep-bit of output element (m, n) is a pure function of (seed, m * N + n): csrc/common.h drop_key / drop_hash / drop_keep1."""
import numpy as np
import torch

import attn_mask as AM

TWO24 = float(1 << 24)
U64 = np.uint64


# ------------------------------------------------------------------------------------------------------------------ dropout stream
def keep_scale(p):
    return 65536.0 / (65536 - AM.thr16(p))


def keep_elementwise(M, N, p, seed):
    """bool [M, N]: element idx = m * N + n is kept iff its 16-bit half of drop_hash(idx >> 1) is >= thr16(p) (odd idx: high half)."""
    k0, k1 = AM.drop_key(seed)
    idx = np.arange(M * N, dtype=U64)
    h = AM.drop_hash(idx >> U64(1), k0, k1)
    half = np.where((idx & U64(1)) == 1, h >> np.uint32(16), h & np.uint32(0xffff))
    return (half >= AM.thr16(p)).reshape(M, N)


# ------------------------------------------------------------------------------------------------------------------ references
def _f64(x):
    return x.detach().cpu().to(torch.float64).numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def product(a, b, ta, tb):
    """(op(A).op(B), |op(A)|.|op(B)|) in float64 from the operands AS STORED ([K, M] when ta, [K, N] when tb)."""
    a, b = _f64(a), _f64(b)
    am = a.T if ta else a            # [M, K]
    bm = b if tb else b.T            # [K, N]
    return am @ bm, np.abs(am) @ np.abs(bm)


def lrelu(x, slope):
    """x > 0 ? x : x * slope (csrc/common.h); slope None or negative: no activation. Keeps the sign of a zero (-3 * 0 = -0)."""
    if slope is None or slope < 0:
        return x
    return np.where(x > 0, x, x * slope)


def mode1(acc, bias, slope, keep, p):
    """dropout_p(LeakyReLU(acc + bias[n])), float64, before the bf16 rounding; a dropped element is +0."""
    t = acc if bias is None else acc + _f64(bias)[None, :]
    t = lrelu(t, slope)
    if p > 0:
        t = np.where(keep, t * keep_scale(p), 0.0)
    return t


def mode2(acc, y, slope, keep, p):
    """acc * keep / (1 - p) * LeakyReLU'(y): the factor is `slope` iff the saved activation y is negative AND non-zero. float64, before
    the bf16 rounding; its column sums are the bias gradient (the kernel sums the fp32 values, not the stored bf16)."""
    t = acc
    if p > 0:
        t = np.where(keep, t * keep_scale(p), 0.0)
    if slope is not None and slope >= 0:
        t = np.where(y_negative(y), t * slope, t)
    return t


def y_negative(y):
    y = _f64(y)
    return (y < 0) & (y != 0)        # -0.0 is NOT negative


def dbias(t):
    return t.sum(axis=0)


def mask_words(keep, y_neg):
    """uint16 [M, N / 8]: bits 0-7 = keep-bits of 8 consecutive outputs, bits 8-15 = "stored activation negative"."""
    M, N = keep.shape
    assert N % 8 == 0
    w = (1 << np.arange(8)).astype(np.uint32)
    lo = (keep.reshape(M, N // 8, 8).astype(np.uint32) * w).sum(-1)
    hi = (y_neg.reshape(M, N // 8, 8).astype(np.uint32) * w).sum(-1)
    return (lo | (hi << 8)).astype(np.uint16)


def bf16_bits(x):
    """int16 bit patterns of float64 / fp32 values rounded to bf16 (nearest-even, torch's CPU conversion)."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.float().to(torch.bfloat16).contiguous().view(torch.int16).numpy()


def bf16_representable(x):
    x = np.asarray(x, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(x)).float().to(torch.bfloat16).to(torch.float64).numpy() == x


# ------------------------------------------------------------------------------------------------------------------ exact regime
def assert_exact_regime(absprod, c0=None, bias=None, scale=1.0, slope=None, dbias_rows=False, what=""):
    """Raise unless every quantity the kernel holds in fp32 is an exactly representable number: |partial sum| <= absprod (+ |C0|, + |bias|),
    times the dropout scale; a slope 2^-s makes the values multiples of 2^-s, i.e. integers after a factor 1 / slope. With dbias_rows the
    column sums over M of those values count too. An assertion, never a skip."""
    bound = np.asarray(absprod, dtype=np.float64).copy()
    if c0 is not None:
        bound = bound + np.abs(_f64(c0))
    if bias is not None:
        bound = bound + np.abs(_f64(bias))[None, :]
    f = float(scale)
    if slope is not None and 0 < slope < 1:
        assert np.log2(slope) == np.floor(np.log2(slope)), f"{what}: slope {slope} is not a power of two"
        f /= slope
    assert f == np.floor(f) and (int(f) & (int(f) - 1)) == 0, f"{what}: scale / slope = {f} is not a power of two"
    worst = float(bound.max()) * f
    if worst >= TWO24:
        raise AssertionError(f"{what}: not in the exact regime: a sum can reach {worst:.0f} >= 2^24")
    if dbias_rows:
        col = float(bound.sum(axis=0).max()) * f
        if col >= TWO24:
            raise AssertionError(f"{what}: not in the exact regime: a dbias column sum can reach {col:.0f} >= 2^24")
    return worst


def int_operand(rows, cols, amp, gen):
    """bf16 [rows, cols] of uniform integers in [-amp, amp] (CPU)."""
    return torch.randint(-amp, amp + 1, (rows, cols), generator=gen).to(torch.bfloat16)


def place(x, ld=None, offset=0, device="cpu"):
    """x [rows, cols] as a view into a larger NaN-poisoned allocation on `device`: row stride `ld` >= cols, first element `offset`
    elements in (a multiple of 8 bf16 keeps the 16-byte alignment the kernels ask for)."""
    rows, cols = x.shape
    ld = cols if ld is None else ld
    assert ld >= cols
    store = torch.full((offset + rows * ld + 8,), float("nan"), dtype=x.dtype)
    store[offset:offset + rows * ld].view(rows, ld)[:, :cols] = x
    store = store.to(device)
    return store[offset:offset + rows * ld].view(rows, ld)[:, :cols]


def poisoned(M, N, ld, dtype, rows_after=2, c0=None):
    """Output buffer [M + rows_after, ld], NaN everywhere except (accumulate cases) the [M, N] window, which holds C0."""
    assert ld >= N
    buf = torch.full((M + rows_after, ld), float("nan"), dtype=dtype)
    if c0 is not None:
        buf[:M, :N] = torch.as_tensor(c0).to(dtype)
    return buf


class Mismatch(AssertionError):
    pass


def check_exact(got_buffer, ref, M=None, N=None, tile=(64, 64), what="", guards=True):
    """tolerance 0. got_buffer: 2-D CPU tensor [>= M, ld] (bf16 / fp32 / int16 mask words as int). (1) its [M, N] window equals `ref`
    (float64): bf16 by BIT PATTERN of ref rounded to bf16, fp32 by value; (2) every other element of the buffer is still NaN.
    A failure names the count, the first (m, n) and its macro-tile."""
    got = got_buffer.detach().cpu() if isinstance(got_buffer, torch.Tensor) else torch.as_tensor(got_buffer)
    ref = np.asarray(ref)
    M = ref.shape[0] if M is None else M
    N = ref.shape[1] if N is None else N
    assert ref.shape == (M, N) and got.dim() == 2 and got.shape[0] >= M and got.shape[1] >= N, (what, ref.shape, tuple(got.shape))
    win = got[:M, :N]
    if got.dtype == torch.bfloat16:
        g, r = win.contiguous().view(torch.int16).numpy(), bf16_bits(ref)
        bad = g != r
        show = lambda m, n: f"got {float(win[m, n])!r} (0x{int(g[m, n]) & 0xffff:04x}), want {float(ref[m, n])!r} -> bf16 0x{int(r[m, n]) & 0xffff:04x}"  # noqa: E731
    else:
        g = win.to(torch.float64).numpy() if got.dtype.is_floating_point else win.numpy().astype(np.int64)
        r = ref.astype(np.float64) if got.dtype.is_floating_point else ref.astype(np.int64)
        bad = ~(g == r)              # a NaN left in the window is a mismatch
        show = lambda m, n: f"got {g[m, n]!r}, want {r[m, n]!r}"  # noqa: E731
    if bad.any():
        mm, nn = np.nonzero(bad)
        m, n = int(mm[0]), int(nn[0])
        tiles = sorted({(int(a) // tile[0], int(b) // tile[1]) for a, b in zip(mm[:4096], nn[:4096])})
        raise Mismatch(f"{what}: {int(bad.sum())} of {M * N} elements differ; first at (m={m}, n={n}) = tile (row {m // tile[0]}, col {n // tile[1]}) "
                       f"of {tile[0]}x{tile[1]}: {show(m, n)}; tiles hit: {tiles[:12]}")
    if guards and got.dtype.is_floating_point:
        guard = torch.ones(got.shape, dtype=torch.bool)
        guard[:M, :N] = False
        alive = guard & ~torch.isnan(got)
        if alive.any():
            m, n = (int(v) for v in torch.nonzero(alive)[0])
            raise Mismatch(f"{what}: {int(alive.sum())} guard elements were written; first at buffer (row {m}, col {n}) = {float(got[m, n])!r} "
                           f"(window is {M} x {N}, row stride {got.shape[1]})")


# ------------------------------------------------------------------------------------------------------------------ rounding regime
def f32_units(got, ref, absprod):
    """worst |got - ref| / (2^-24 * absprod): the accumulation error of an fp32 result in units of the fp32 epsilon of its |A|.|B|."""
    unit = np.maximum(np.asarray(absprod, dtype=np.float64), 1e-30) / TWO24
    return float((np.abs(_f64(got) - ref) / unit).max())


def bf16_half_ulp(ref):
    """half a unit in the last place of bf16 (8 significand bits) at |ref|: 2^(floor(log2 |ref|) - 8); the most round-to-nearest can move a
    value. Between 2^-9 |ref| (top of a binade) and 2^-8 |ref| (bottom)."""
    r = np.abs(np.asarray(ref, dtype=np.float64))
    return np.where(r > 0, 2.0 ** (np.floor(np.log2(np.maximum(r, 1e-300))) - 8), 0.0)


def bf16_excess_units(got, ref, absprod, scale=1.0):
    """worst (|got - ref| - the bf16 round-to-nearest allowance half_ulp(ref) (1 + 2^-7)) / (2^-24 * absprod * scale), floored at 0."""
    unit = np.maximum(np.asarray(absprod, dtype=np.float64) * scale, 1e-30) / TWO24
    exc = np.abs(_f64(got) - ref) - bf16_half_ulp(ref) * (1 + 2.0 ** -7)
    return float(np.maximum(exc / unit, 0.0).max())


def f32_ok(got, ref, absprod, c):
    return bool((np.abs(_f64(got) - ref) <= c * np.asarray(absprod) / TWO24).all())


def bf16_ok(got, ref, absprod, c, scale=1.0):
    bound = bf16_half_ulp(ref) * (1 + 2.0 ** -7) + c * np.asarray(absprod) * scale / TWO24
    return bool((np.abs(_f64(got) - ref) <= bound).all())
