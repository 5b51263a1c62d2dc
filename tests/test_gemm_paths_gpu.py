"""Every bf16 GEMM kernel path of csrc/gemm.hip and csrc/gemm_big.hip, element by element, against float64 (tests/helpers/gemm_ref.py).

EXACT regime (tolerance 0): operands are integers in [-15, 15] (smaller where a bias-gradient column sum asks for it), so every fp32
partial sum is an integer below 2^24 and every summation order - MFMA internals, wave-K partial tiles, split-K slabs, the slab reduction -
gives the same bits: the fp32 result must EQUAL the float64 product, a bf16 result must equal it rounded to nearest-even, bit for bit.
Epilogues stay exact with an integer bias, slope in {none, 0, 0.25} and dropout p in {0, 0.5} (scale exactly 2); seed_dev = NULL, so the
keep-bits are a pure function of (SEED, m * N + n). gemm_ref.assert_exact_regime proves the precondition for every case from |A|.|B|.
Every output buffer starts as NaN, is wider than N and has rows behind it: whatever the kernel does not own must still be NaN afterwards.
Every case runs twice and must give the same bits.

Which kernel a case runs (kernel() below mirrors plan() / launch() of csrc/gemm.hip; verified once with a kernel trace of this module,
profiles/gemm_paths_kernel_stats.csv):

    case group                                forced (tile, ring)        kernel
    general, main loop "reg"                  (t, 0)                     gemm_bf16_kernel<BM, BN, AT, BT, OUT>
    general, main loop "ring"                 (t, 2), K % 64 == 0        gemm_bf16_ring_kernel<BM, BN, AT, BT, OUT, 3>, except
        64x64, tt, fp32 store / accumulate    (2, 2)                     gemm_tt64_wavek_kernel<OUT>    (always: it shadows the ring kernel,
                                                                         gemm_bf16_ring_kernel<64, 64, true, true, 1 | 2, 3> cannot be reached)
        64x64, nn, bf16, K per chunk >= 1024  (2, 2)                     gemm_nn64_wavek_kernel         (K < 1024: the ring kernel it shadows)
    split-K (fp32 out, splits > 1)            (t, 0 | 2) + splits        the OUT = 1 kernel of the row above + gemm_slab_reduce_kernel
                                                                         (accumulate = 2 inside a deferral: the batched reduction instead)
    fused epilogues, general kernels          (t, 0 | 2)                 the OUT = 0 kernel, EpiArgs.mode 1 (in registers) / 2 (fp32 LDS tile)
    gemm_big                                  automatic                  gemm_big_kernel<256 | 128, mode, MASK>
    nt_batched                                -                          gemm_bf16_ring_kernel<64, 64, false, false, 0, 3>, grid.y = batch
    project shapes                            automatic                  as kernel() says, per case (AUTO_CASES)

ROUNDING regime (Gaussian operands rounded to bf16; what integers cannot show: a bf16 accumulator, an early rounding, a narrow slab), one
case per kernel family at K = 256 and at the longest K the family sees, bounds per element:
    fp32 out   |got - ref| <= c * 2^-24 * absprod                              absprod = |A|.|B| (+ |bias|)
    bf16 out   |got - ref| <= half_ulp_bf16(ref) * (1 + 2^-7) + c * 2^-24 * absprod * scale
half_ulp_bf16(ref) = 2^(floor(log2 |ref|) - 8) is what round-to-nearest of an 8-bit significand can move a value: between 2^-9 |ref| at the
top of a binade and 2^-8 |ref| at its bottom (a flat 2^-9 |ref| rejects a correctly rounded fp32 result: 24.3075 -> 24.25 is 1.2 * 2^-9).
c = twice the worst value measured on the MI355X (ROUNDING_C, the measured value beside each); every c is far below K, the worst case of
any fp32 summation order - a measured value near K would mean that the accumulator is not fp32."""
import contextlib
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SEED = 0x5EED1234
AMP = 15
TILE = {0: (128, 128), 1: (128, 64), 2: (64, 64)}
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]                      # (transA, transB): nn, nt, tn, tt
LNAME = {(0, 0): "nn", (0, 1): "nt", (1, 0): "tn", (1, 1): "tt"}
OUTS = ["bf16", "f32", "acc"]                                   # OUT_MODE 0 / 1 / 2
EPI = [(0.5, 0.25), (0.0, None), (0.5, 0.0), (0.0, 0.25), (0.5, None), (0.0, 0.0)]     # (dropout p, LeakyReLU slope)


def cdiv(a, b):
    return -(-a // b)


def up8(x):
    return cdiv(x, 8) * 8


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


@pytest.fixture(scope="module")
def L(C):
    return C.lib()


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("ts-asr_amd.ops")


@pytest.fixture
def force(L):
    """force(tile, splits, ring): a context in which plan() / launch() take that macro-tile, split-K factor and main loop; the automatic
    plan comes back when it ends, however it ends."""
    @contextlib.contextmanager
    def ctx(tile, splits, ring):
        L.tsasr_gemm_set_plan(tile, splits)
        L.tsasr_gemm_set_ring(ring)
        try:
            yield
        finally:
            L.tsasr_gemm_set_plan(-1, 0)
            L.tsasr_gemm_set_ring(1)
    yield ctx
    L.tsasr_gemm_set_plan(-1, 0)
    L.tsasr_gemm_set_ring(1)


# ---------------------------------------------------------------------------------------------- the host's launch rules (csrc/gemm.hip)
def plan(M, N, K, out_f32, tile=-1, splits=0):
    if tile >= 0:
        s = splits if (out_f32 and splits > 0) else 1
    else:
        t0, t1, t2 = cdiv(M, 128) * cdiv(N, 128), cdiv(M, 128) * cdiv(N, 64), cdiv(M, 64) * cdiv(N, 64)
        tile = 0 if t0 >= 512 else (1 if t1 >= 192 else 2)
        tiles = (t0, t1, t2)[tile]
        s = 1
        if out_f32 and tiles < 256 and K >= 384:
            s = max(1, min(cdiv(768, tiles), max(1, K // 128), 32))
    kchunk = cdiv(cdiv(K, s), 64) * 64
    return tile, cdiv(K, kchunk), kchunk


def big_bm(M, N, K):
    if N % 256 or K % 64 or N < 1024 or K > 1024 or M < 256:
        return 0
    return 256 if cdiv(M, 256) * (N // 256) >= 200 else (128 if cdiv(M, 128) * (N // 256) >= 96 else 0)


def kernel(M, N, K, ta, tb, out, tile=-1, splits=0, ring=1, ldc_ok=True):
    """name of the GEMM kernel tsasr_gemm_bf16 launches (out: 0 bf16, 1 fp32 store, 2 fp32 accumulate)"""
    if out == 0 and not ta and not tb and tile < 0 and ldc_ok and big_bm(M, N, K):
        return f"gemm_big_kernel<{big_bm(M, N, K)}, 0, false>"
    tile, s, kchunk = plan(M, N, K, out != 0, tile, splits)
    om = 1 if s > 1 else out
    bm, bn = TILE[tile]
    kk = min(K, kchunk)
    use_ring = bool(ring) and K % 64 == 0 and (ring == 2 or kk >= 1024 or bm * bn < 128 * 128) and (M >= 8 or not ta) and (N >= 8 or not tb)
    tf = lambda v: "true" if v else "false"  # noqa: E731
    if use_ring and tile == 2 and ta and tb and om != 0:
        return f"gemm_tt64_wavek_kernel<{om}>"
    if use_ring and tile == 2 and not ta and not tb and om == 0 and kk >= 1024:
        return "gemm_nn64_wavek_kernel"
    if use_ring:
        return f"gemm_bf16_ring_kernel<{bm}, {bn}, {tf(ta)}, {tf(tb)}, {om}, 3>"
    return f"gemm_bf16_kernel<{bm}, {bn}, {tf(ta)}, {tf(tb)}, {om}>"


def test_kernel_map():
    """the table of the module docstring, as kernel() gives it (no device work)"""
    assert kernel(128, 128, 64, 1, 1, 1, tile=2, ring=2) == "gemm_tt64_wavek_kernel<1>"
    assert kernel(128, 128, 72, 1, 1, 2, tile=2, ring=0) == "gemm_bf16_kernel<64, 64, true, true, 2>"
    assert kernel(65, 65, 1024, 0, 0, 0, tile=2, ring=2) == "gemm_nn64_wavek_kernel"
    assert kernel(65, 65, 256, 0, 0, 0, tile=2, ring=2) == "gemm_bf16_ring_kernel<64, 64, false, false, 0, 3>"
    assert kernel(129, 65, 64, 0, 1, 0, tile=1, ring=2) == "gemm_bf16_ring_kernel<128, 64, false, true, 0, 3>"
    assert kernel(8000, 2048, 256, 0, 0, 0) == "gemm_big_kernel<256, 0, false>"
    assert kernel(8000, 256, 2048, 0, 0, 0) == "gemm_bf16_ring_kernel<128, 64, false, false, 0, 3>"
    assert kernel(2048, 256, 8000, 1, 1, 2) == "gemm_tt64_wavek_kernel<1>" and plan(2048, 256, 8000, True)[1] > 1
    for _, M, N, K, ta, tb, out, want in AUTO_CASES:
        assert kernel(M, N, K, ta, tb, out) == want, (M, N, K, ta, tb, out, kernel(M, N, K, ta, tb, out))


# ---------------------------------------------------------------------------------------------- calls through the C ABI
def stored(x, trans):
    """operand [rows, K] -> as the ABI wants it ([K, rows] when transposed), CPU"""
    return x.t().contiguous() if trans else x


def gemm(C, L, A, B, Cbuf, M, N, K, ta, tb, accumulate=0, ws=None):
    od = C.F32 if Cbuf.dtype == F32 else C.BF16
    return L.tsasr_gemm_bf16(C.ptr(A), C.ptr(B), C.ptr(Cbuf), M, N, K, A.stride(0), B.stride(0), Cbuf.stride(0), ta, tb, od, accumulate,
                             C.ptr(ws), 0 if ws is None else ws.numel(), C.stream_ptr())


def fused(C, L, A, B, Cbuf, M, N, K, ta, tb, mode, bias=None, y=None, slope=None, p=0.0, dbias=None, mask=None, ws=None, ws_bytes=None):
    return L.tsasr_gemm_bf16_fused(C.ptr(A), C.ptr(B), C.ptr(Cbuf), M, N, K, A.stride(0), B.stride(0), Cbuf.stride(0), ta, tb, mode,
                                   C.ptr(bias), C.ptr(y), 0 if y is None else y.stride(0), -1.0 if slope is None else float(slope), float(p),
                                   SEED, None, C.ptr(dbias), C.ptr(mask), C.ptr(ws),
                                   (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, C.stream_ptr())


def twice(run, make_out):
    """run(out) on two fresh output buffers: the same bits (NaN guards included) both times; returns the first, on the CPU"""
    outs = []
    for _ in range(2):
        o = make_out().to(DEV)
        rc = run(o)
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append(o.cpu())
    a, b = (o.contiguous().view(torch.int16 if o.dtype == BF16 else torch.int32) for o in outs)
    assert torch.equal(a, b), "two runs of the same call differ"
    return outs[0]


def operands(M, N, K, ta, tb, seed, amp=AMP, pad=False):
    """integer operands in the ABI's layouts on the device; pad: row strides beyond the row length and base pointers 16 / 32 bytes into a
    larger allocation (whose other elements are NaN)"""
    g = torch.Generator().manual_seed(seed)
    a, b = stored(GR.int_operand(M, K, amp, g), ta), stored(GR.int_operand(N, K, amp, g), tb)
    A = GR.place(a, a.shape[1] + 8 if pad else None, 8 if pad else 0, DEV)
    B = GR.place(b, b.shape[1] + 16 if pad else None, 16 if pad else 0, DEV)
    return a, b, A, B


# ---------------------------------------------------------------------------------------------- general kernels: 72 instantiations x edges
REG_K = [8, 64, 72, 200]
RING_K = [64, 128, 192, 256, 1024, 1088]                        # 1 - 4 k-tiles on a 3-slot ring, then 16 and 17


def edge_shapes(tile, ta, tb):
    bm, bn = TILE[tile]
    em, en = (8 if ta else 1), (8 if tb else 1)                 # a transposed side has 8-element rows
    return [(bm, bn), (bm + em, bn + en), (em, en), (2 * bm + 24 + (0 if ta else 1), 2 * bn + 16 + (0 if tb else 3))]


@pytest.mark.parametrize("loop", ["reg", "ring"])
@pytest.mark.parametrize("out", OUTS)
@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=[LNAME[x] for x in LAYOUTS])
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_general_exact(C, L, force, tile, ta, tb, out, loop):
    ring = 0 if loop == "reg" else 2
    shapes, ks = edge_shapes(tile, ta, tb), (REG_K if loop == "reg" else RING_K)
    cases = [(shapes[i % 4], k) for i, k in enumerate(ks)] + [(shapes[3], ks[0]), (shapes[1], ks[-1]), (shapes[2], ks[1])]
    om = OUTS.index(out)
    names = set()
    for i, ((M, N), K) in enumerate(cases):
        pad = i % 2 == 1
        a, b, A, B = operands(M, N, K, ta, tb, 1000 * tile + 100 * i + 10 * ta + tb, pad=pad)
        ref, absprod = GR.product(a, b, ta, tb)
        c0 = None
        if out == "acc":
            c0 = torch.randint(-1000, 1001, (M, N), generator=torch.Generator().manual_seed(i)).float()
            ref = ref + c0.double().numpy()
        GR.assert_exact_regime(absprod, c0=c0, what=f"general {M}x{N}x{K}")
        if out == "bf16" and K >= 256 and M * N >= 4096:       # a condition on the INPUTS: these cases check the rounding, not only the sum
            assert (~GR.bf16_representable(ref)).mean() >= 0.25, (M, N, K)
        ldc = (up8(N) + 8) if pad else N
        what = f"tile {TILE[tile]} {LNAME[ta, tb]} {out} {loop} M={M} N={N} K={K} lda={A.stride(0)} ldb={B.stride(0)} ldc={ldc}"
        with force(tile, 0, ring):
            names.add(kernel(M, N, K, ta, tb, om, tile=tile, ring=ring))
            got = twice(lambda o: gemm(C, L, A, B, o, M, N, K, ta, tb, accumulate=int(out == "acc")),
                        lambda: GR.poisoned(M, N, ldc, BF16 if out == "bf16" else F32, 2, c0))
        GR.check_exact(got, ref, M, N, TILE[tile], what)
    bm, bn = TILE[tile]
    if loop == "reg":
        assert names == {f"gemm_bf16_kernel<{bm}, {bn}, {'true' if ta else 'false'}, {'true' if tb else 'false'}, {om}>"}
    elif tile == 2 and ta and tb and om:
        assert names == {f"gemm_tt64_wavek_kernel<{om}>"}
    elif tile == 2 and not ta and not tb and not om:
        assert names == {"gemm_nn64_wavek_kernel", "gemm_bf16_ring_kernel<64, 64, false, false, 0, 3>"}
    else:
        assert names == {f"gemm_bf16_ring_kernel<{bm}, {bn}, {'true' if ta else 'false'}, {'true' if tb else 'false'}, {om}, 3>"}


# ---------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("loop", ["reg", "ring"])
@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=[LNAME[x] for x in LAYOUTS])
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_split_k_exact(C, L, ops, force, tile, ta, tb, loop):
    """forced splits 2, 3 and one the cap cuts down (at least one k-tile per split): fp32 slabs in a NaN-poisoned workspace of exactly the
    size the ABI asks for + the fixed-order reduction. ring: a shorter last chunk (K = 320); register-staged: K % 64 != 0 (200, 3872)."""
    ring = 0 if loop == "reg" else 2
    bm, bn = TILE[tile]
    M, N = bm + 8, bn + (8 if tb else 4)
    dev = torch.device(DEV)
    for K, forced_s, want_s in ([(320, 2, 2), (320, 3, 3), (320, 64, 5)] if loop == "ring" else
                                [(200, 2, 2), (200, 64, 4), (3872, 2, 2), (3872, 3, 3), (3872, 32, 31)]):
        a, b, A, B = operands(M, N, K, ta, tb, 7000 + 100 * tile + K + forced_s, pad=(forced_s == 3))
        ref, absprod = GR.product(a, b, ta, tb)
        c0 = torch.randint(-1000, 1001, (M, N), generator=torch.Generator().manual_seed(K)).float()
        GR.assert_exact_regime(absprod, c0=c0, what=f"split-K {M}x{N}x{K}")
        what = f"split-K tile {TILE[tile]} {LNAME[ta, tb]} {loop} M={M} N={N} K={K} splits={forced_s}->{want_s}"
        with force(tile, forced_s, ring):
            assert plan(M, N, K, True, tile, forced_s)[1] == want_s
            nws = L.tsasr_gemm_bf16_workspace_bytes(M, N, K, C.F32)
            assert nws >= want_s * M * N * 4 and nws < want_s * M * N * 4 + 256, (what, nws)
            ws = torch.full((nws // 4,), float("nan"), dtype=F32, device=DEV).view(torch.uint8)
            store = twice(lambda o: gemm(C, L, A, B, o, M, N, K, ta, tb, 0, ws), lambda: GR.poisoned(M, N, N, F32, 2))
            GR.check_exact(store, ref, M, N, TILE[tile], what + " store")
            ldc = N + 4                                          # a multiple of 4, not of 8
            acc1 = twice(lambda o: gemm(C, L, A, B, o, M, N, K, ta, tb, 1, ws), lambda: GR.poisoned(M, N, ldc, F32, 2, c0))
            GR.check_exact(acc1, ref + c0.double().numpy(), M, N, TILE[tile], what + f" accumulate ldc={ldc}")

            def deferred(o):
                ops.reduce_defer_begin(dev)
                try:
                    rc = gemm(C, L, A, B, o, M, N, K, ta, tb, 2, ws)
                    ops.reduce_flush()
                finally:
                    ops.reduce_defer_end()
                return rc
            ops.reduce_defer_prepare(dev)
            acc2 = twice(deferred, lambda: GR.poisoned(M, N, N, F32, 2, c0))
            GR.check_exact(acc2, ref + c0.double().numpy(), M, N, TILE[tile], what + " accumulate = 2 (deferred)")
            assert torch.equal(acc2[:M, :N], acc1[:M, :N])


# ---------------------------------------------------------------------------------------------- fused epilogues in the general kernels
@pytest.mark.parametrize("loop", ["reg", "ring"])
@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=[LNAME[x] for x in LAYOUTS])
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_fused_general_exact(C, L, force, tile, ta, tb, loop):
    """modes 1 (in registers) and 2 (fp32 LDS tile) under a forced tile (which bypasses gemm_big): M over 1, 2 and 3 row tiles, ragged;
    N = tile + 8 (the `n + 8 <= N` guard and the bias load at the edge); ldc, ldy > N; dbias from cdiv(M, BM) partial rows; bias = NULL and
    dbias = NULL once each."""
    ring, K = (0, 72) if loop == "reg" else (2, 128)
    bm, bn = TILE[tile]
    N = bn + 8
    for i, M in enumerate([bm - 24, 2 * bm - 8, 2 * bm + 8]):
        p, slope = EPI[(i + tile + 2 * ta + tb) % 4]
        a, b, A, B = operands(M, N, K, ta, tb, 9000 + 100 * tile + 10 * i + 2 * ta + tb, amp=7, pad=(i == 1))   # 7: the dbias column sums
        acc, absprod = GR.product(a, b, ta, tb)
        bias = None if i == 2 else torch.randint(-64, 65, (N,), generator=torch.Generator().manual_seed(i)).float()
        GR.assert_exact_regime(absprod, bias=bias, scale=GR.keep_scale(p), slope=slope, dbias_rows=True, what=f"fused {M}x{N}x{K}")
        keep = GR.keep_elementwise(M, N, p, SEED)
        ldc = N + 8
        what = f"fused tile {TILE[tile]} {LNAME[ta, tb]} {loop} M={M} N={N} K={K} p={p} slope={slope} bias={'yes' if bias is not None else 'NULL'}"
        with force(tile, 0, ring):
            assert L.tsasr_gemm_bf16_fused_mask_ok(M, N, K) == 0
            bias_d = None if bias is None else bias.to(DEV)
            y = twice(lambda o: fused(C, L, A, B, o, M, N, K, ta, tb, 1, bias=bias_d, slope=slope, p=p), lambda: GR.poisoned(M, N, ldc, BF16, 2))
            ref1 = GR.mode1(acc, bias, slope, keep, p)
            GR.check_exact(y, ref1, M, N, TILE[tile], what + " mode 1")
            y_d = y.to(DEV)[:M, :N]                                # row stride ldy = ldc > N, NaN in the gap
            t = GR.mode2(acc, y[:M, :N], slope, keep, p)
            nws = L.tsasr_gemm_bf16_fused_workspace_bytes(M, N)
            for with_dbias in ([True, False] if i == 1 else [True]):
                db = torch.full((1, N + 8), float("nan"), dtype=F32, device=DEV) if with_dbias else None
                ws = torch.full((nws // 4,), float("nan"), dtype=F32, device=DEV).view(torch.uint8) if with_dbias else None
                dx = twice(lambda o: fused(C, L, A, B, o, M, N, K, ta, tb, 2, y=y_d, slope=slope, p=p, dbias=db, ws=ws),
                           lambda: GR.poisoned(M, N, ldc, BF16, 2))
                GR.check_exact(dx, t, M, N, TILE[tile], what + f" mode 2 dbias={'yes' if with_dbias else 'NULL'}")
                if with_dbias:
                    torch.cuda.synchronize()
                    GR.check_exact(db.cpu(), GR.dbias(t)[None, :], 1, N, (1, bn), what + " dbias")


# ---------------------------------------------------------------------------------------------- gemm_big (automatic plan)
BIG_SHAPES = [(6400, 2048, 256), (6350, 2048, 64), (6350, 2048, 128), (6400, 2048, 192), (6350, 2048, 1024), (12600, 1024, 64),     # bm = 256
              (1536, 2048, 1024), (1500, 2048, 64), (1500, 2048, 192), (3000, 1024, 256), (3000, 1024, 128)]                        # bm = 128


def big_amp(M, K, p, slope):
    """largest operand range whose bias-gradient column sums stay below 2^24: M * K * amp^2 * scale / slope < 2^24 (worst case; the
    case's own |A|.|B| is checked by assert_exact_regime afterwards)"""
    f = GR.keep_scale(p) / (slope if slope else 1.0)
    for amp in (15, 7, 3, 2, 1):
        if M * K * amp * amp * f < GR.TWO24:
            return amp, 1.0
    return 1, min(1.0, GR.TWO24 / (M * K * f) * 0.9)             # {-1, 0, 1} with that share of non-zero entries in A


@pytest.mark.parametrize("combo", [0, 1])
@pytest.mark.parametrize("M,N,K", BIG_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in BIG_SHAPES])
def test_gemm_big_exact(C, L, M, N, K, combo):
    bm = big_bm(M, N, K)
    assert bm == (256 if BIG_SHAPES.index((M, N, K)) < 6 else 128) and L.tsasr_gemm_bf16_fused_mask_ok(M, N, K) == 1
    p, slope = EPI[(2 * BIG_SHAPES.index((M, N, K)) + combo) % 6]
    g = torch.Generator().manual_seed(M + N + K + combo)
    a, b = GR.int_operand(M, K, AMP, g), GR.int_operand(N, K, AMP, g)
    A, B = GR.place(a, K + 8, 8, DEV), GR.place(b, K + 16, 16, DEV)
    acc, absprod = GR.product(a, b, 0, 0)
    bias = torch.randint(-64, 65, (N,), generator=g).float()
    GR.assert_exact_regime(absprod, bias=bias, scale=GR.keep_scale(p), slope=slope, what=f"gemm_big {M}x{N}x{K}")
    tile, ldc = (bm, 256), N + 8
    what = f"gemm_big<{bm}> M={M} N={N} K={K} p={p} slope={slope}"
    if combo == 0:
        got = twice(lambda o: gemm(C, L, A, B, o, M, N, K, 0, 0), lambda: GR.poisoned(M, N, ldc, BF16, 1))
        GR.check_exact(got, acc, M, N, tile, what + " mode 0")
    keep = GR.keep_elementwise(M, N, p, SEED)
    ref1 = GR.mode1(acc, bias, slope, keep, p)
    bias_d = bias.to(DEV)
    y = twice(lambda o: fused(C, L, A, B, o, M, N, K, 0, 0, 1, bias=bias_d, slope=slope, p=p), lambda: GR.poisoned(M, N, ldc, BF16, 1))
    GR.check_exact(y, ref1, M, N, tile, what + " mode 1")
    words = torch.full((M + 1, N // 8), -1, dtype=torch.int16, device=DEV)       # one row of 0xffff behind the M rows the kernel owns
    ym = twice(lambda o: fused(C, L, A, B, o, M, N, K, 0, 0, 1, bias=bias_d, slope=slope, p=p, mask=words), lambda: GR.poisoned(M, N, ldc, BF16, 1))
    GR.check_exact(ym, ref1, M, N, tile, what + " mode 1 + mask words")
    torch.cuda.synchronize()
    w = words.cpu().numpy().view(np.uint16)
    GR.check_exact(torch.from_numpy(w[:M].astype(np.int32)), GR.mask_words(keep, GR.y_negative(y[:M, :N])), M, N // 8, (bm, 32), what + " mask words")
    assert (w[M] == 0xffff).all(), "mask words written behind row M"
    # mode 2 with operands of its own: the bias gradient sums M values per column, which asks for a smaller range (big_amp)
    amp, dens = big_amp(M, K, p, slope)
    a2, b2 = GR.int_operand(M, K, amp, g), GR.int_operand(N, K, amp, g)
    if dens < 1.0:
        a2 = a2 * (torch.rand(M, K, generator=g) < dens).to(BF16)
    A, B = GR.place(a2, K + 8, 8, DEV), GR.place(b2, K + 16, 16, DEV)
    acc, absprod = GR.product(a2, b2, 0, 0)
    GR.assert_exact_regime(absprod, scale=GR.keep_scale(p), slope=slope, dbias_rows=True, what=f"gemm_big dbias {M}x{N}x{K} amp={amp}")
    t = GR.mode2(acc, y[:M, :N], slope, keep, p)
    y_d = y.to(DEV)[:M, :N]
    nws = L.tsasr_gemm_bf16_fused_workspace_bytes(M, N)
    for src in ("y", "mask"):
        db = torch.full((1, N + 8), float("nan"), dtype=F32, device=DEV)
        ws = torch.full((nws // 4,), float("nan"), dtype=F32, device=DEV).view(torch.uint8)
        dx = twice(lambda o: fused(C, L, A, B, o, M, N, K, 0, 0, 2, y=y_d, slope=slope, p=p, dbias=db, ws=ws, mask=words if src == "mask" else None),
                   lambda: GR.poisoned(M, N, ldc, BF16, 1))
        GR.check_exact(dx, t, M, N, tile, what + f" mode 2 from {src}")
        torch.cuda.synchronize()
        GR.check_exact(db.cpu(), GR.dbias(t)[None, :], 1, N, (1, 256), what + f" dbias from {src}")


def test_fused_refusals(C, L, force):
    """a refused call returns an error and leaves the output poisoned"""
    M, N, K = 1536, 2048, 64
    a, b, A, B = operands(M, N, K, 0, 0, 5)
    out = GR.poisoned(M, N, N, BF16, 0).to(DEV)
    words = torch.zeros(M, N // 8, dtype=torch.int16, device=DEV)
    y = torch.zeros(M, N, dtype=BF16, device=DEV)
    db = torch.zeros(N, dtype=F32, device=DEV)
    ws = torch.zeros(L.tsasr_gemm_bf16_fused_workspace_bytes(M, N), dtype=torch.uint8, device=DEV)
    assert L.tsasr_gemm_bf16_fused_mask_ok(M, N, K) == 1 and L.tsasr_gemm_bf16_fused_mask_ok(M, N - 8, K) == 0
    assert fused(C, L, A, B, out, M, N - 8, K, 0, 0, 1, mask=words) != 0                      # no mask words for this shape
    assert fused(C, L, A, B, out, M, N, K, 0, 0, 1, slope=1.5, mask=words) != 0               # slope > 1 together with a mask
    assert fused(C, L, A, B, out, M, N, K, 0, 0, 2, y=y, dbias=db, ws=ws, ws_bytes=ws.numel() - 256) != 0   # too small a dbias workspace
    assert fused(C, L, A, B, out, M, N, K, 0, 0, 2, y=y, dbias=db, ws=None) != 0
    with force(2, 0, 1):
        assert L.tsasr_gemm_bf16_fused_mask_ok(M, N, K) == 0
        assert fused(C, L, A, B, out, M, N, K, 0, 0, 1, mask=words) != 0                      # a forced tile bypasses gemm_big
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and int(words.abs().sum()) == 0 and float(db.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------- the project's own shapes (automatic plan)
def _auto_cases():
    """forward (nn), data gradient (nt) and weight gradient (tt, fp32 accumulate, inner dimension = rows) of one encoder layer's Linear
    layers d_in -> d_out at B*T' = 8000 rows and at a ragged count (7995; 7992 where the rows are the 8-element inner dimension)"""
    out = []
    for rows in (8000, 7995):
        for d_in, d_out in [(256, 768), (256, 256), (256, 2048), (2048, 256), (256, 2560), (768, 256)]:
            out.append((f"fwd {rows} {d_in}->{d_out}", rows, d_out, d_in, 0, 0, 0))
            out.append((f"dgrad {rows} {d_in}->{d_out}", rows, d_in, d_out, 0, 1, 0))
            out.append((f"wgrad {rows} {d_in}->{d_out}", d_out, d_in, rows - rows % 8, 1, 1, 2))
    return [c + (kernel(*c[1:]),) for c in out]


AUTO_CASES = _auto_cases()
AUTO_EXPECT = {   # written out by hand from plan() / launch() for one case of each kind; kernel() must agree
    "fwd 8000 256->2048": "gemm_big_kernel<256, 0, false>",                       # 32 x 8 tiles of 256 x 256
    "fwd 7995 256->2560": "gemm_big_kernel<256, 0, false>",
    "fwd 8000 256->768": "gemm_bf16_ring_kernel<128, 64, false, false, 0, 3>",    # 63 x 6 = 378 < 512 tiles of 128x128 -> 128x64, ring at any K
    "fwd 8000 2048->256": "gemm_bf16_ring_kernel<128, 64, false, false, 0, 3>",
    "dgrad 8000 2048->256": "gemm_bf16_kernel<128, 128, false, true, 0>",         # 63 x 16 tiles of 128x128, K = 256 < 1024: register-staged
    "dgrad 7995 256->2048": "gemm_bf16_ring_kernel<128, 64, false, true, 0, 3>",
    "wgrad 8000 256->256": "gemm_tt64_wavek_kernel<1>",                           # 16 tiles of 64x64 -> 32 slabs of 256
    "wgrad 8000 256->2560": "gemm_tt64_wavek_kernel<1>",
    "wgrad 7995 2048->256": "gemm_bf16_kernel<64, 64, true, true, 1>",            # K = 7992 is no multiple of 64: the register-staged loop, 6 slabs
    "wgrad 7995 256->256": "gemm_bf16_kernel<64, 64, true, true, 1>",
}


@pytest.mark.parametrize("case", AUTO_CASES, ids=[c[0] for c in AUTO_CASES])
def test_project_shapes_exact(C, L, case):
    name, M, N, K, ta, tb, out, want = case
    if name in AUTO_EXPECT:
        assert want == AUTO_EXPECT[name], (name, want)
    a, b, A, B = operands(M, N, K, ta, tb, M + N + K + ta)
    ref, absprod = GR.product(a, b, ta, tb)
    c0 = torch.randint(-1000, 1001, (M, N), generator=torch.Generator().manual_seed(1)).float() if out else None
    GR.assert_exact_regime(absprod, c0=c0, what=name)
    tile, splits, _ = plan(M, N, K, out != 0)
    nws = L.tsasr_gemm_bf16_workspace_bytes(M, N, K, C.F32 if out else C.BF16)
    assert (nws > 0) == (splits > 1)
    ws = torch.full((max(nws, 4) // 4,), float("nan"), dtype=F32, device=DEV).view(torch.uint8) if nws else None
    got = twice(lambda o: gemm(C, L, A, B, o, M, N, K, ta, tb, int(out == 2), ws), lambda: GR.poisoned(M, N, N + 8, F32 if out else BF16, 1, c0))
    GR.check_exact(got, ref if c0 is None else ref + c0.double().numpy(), M, N, (256, 256) if "big" in want else TILE[tile], f"{name}: {want}")


# ---------------------------------------------------------------------------------------------- tsasr_gemm_bf16_nt_batched
def batched(C, L, A, Bs, out, M, N, K, ldc, c_batch):
    tab = torch.tensor([b.data_ptr() for b in Bs], dtype=torch.int64, device=DEV)          # the pointer table is a DEVICE array
    rc = L.tsasr_gemm_bf16_nt_batched(C.ptr(A), C.ptr(tab), C.ptr(out), M, N, K, A.stride(0), Bs[0].stride(0), ldc, c_batch, len(Bs), C.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("K", [64, 192, 1088])
@pytest.mark.parametrize("nbatch", [1, 3, 18])
def test_nt_batched_exact(C, L, nbatch, K):
    M, N = 100, 136                                             # ragged against the 64x64 tile
    ldc, gap = N + 8, 16
    c_batch = M * ldc + gap                                     # > M * ldc: the elements between two matrices stay NaN
    g = torch.Generator().manual_seed(nbatch * 1000 + K)
    a = GR.int_operand(M, K, AMP, g)
    bs = [GR.int_operand(N, K, AMP, g) for _ in range(nbatch)]
    A = GR.place(a, K + 8, 8, DEV)
    Bs = [GR.place(b, K + 16, 16, DEV) for b in bs]
    outs = []
    for _ in range(2):
        out = torch.full((nbatch * c_batch + 8,), float("nan"), dtype=BF16, device=DEV)
        assert batched(C, L, A, Bs, out, M, N, K, ldc, c_batch) == 0
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two runs differ"
    flat = outs[0]
    for i, b in enumerate(bs):
        ref, absprod = GR.product(a, b, 0, 0)
        GR.assert_exact_regime(absprod, what="nt_batched")
        GR.check_exact(flat[i * c_batch:i * c_batch + M * ldc].view(M, ldc), ref, M, N, (64, 64), f"nt_batched nbatch={nbatch} K={K} matrix {i}")
        assert bool(torch.isnan(flat[i * c_batch + M * ldc:(i + 1) * c_batch]).all()), f"gap behind matrix {i} written"
    assert bool(torch.isnan(flat[nbatch * c_batch:]).all())


def test_nt_batched_refusals(C, L):
    M, N, K = 64, 72, 128
    g = torch.Generator().manual_seed(3)
    A, B = GR.int_operand(M, K, AMP, g).to(DEV), GR.int_operand(N, K, AMP, g).to(DEV)
    out = torch.full((M * N,), float("nan"), dtype=BF16, device=DEV)
    assert batched(C, L, A, [B], out, M, N, 72, N, M * N) != 0          # K % 64
    assert batched(C, L, A, [B], out, M, N - 4, K, N, M * N) != 0       # N % 8
    assert bool(torch.isnan(out).all())
    assert batched(C, L, A, [B], out, M, N, K, N, M * N) == 0 and not bool(torch.isnan(out).any())


# ---------------------------------------------------------------------------------------------- rounding regime
# c per kernel family = 2 x the worst |got - ref| / (2^-24 * absprod) (bf16 outputs: of what exceeds the rounding allowance) measured on the
# MI355X against float64, over the family's cases; the measured value stands beside each. The fp32 families sit at 1 - 2 units where the
# CPU's fp32 matmul gives 0.24: the MFMA adds its 16 products and the accumulator without rounding each step to nearest, and the error
# grows with the number of k-steps - still a thousandth of K. The bf16-only families show next to nothing, because the (1 + 2^-7) allowance
# on the rounding term covers the accumulation noise wherever |ref| is not tiny.
ROUNDING_C = {
    "reg": 3.7,            # measured 1.8113 (64x64 tt accumulate, K = 256); fp32 store at K = 2560: 1.5611; bf16: 0.1337
    "ring": 3.2,           # measured 1.5611 (128x64 nn fp32 store, K = 2560); accumulate at K = 256: 1.3181; bf16: 0.1958
    "tt64_wavek": 2.0,     # measured 0.9838 (K = 256); K = 8000: 0.5534
    "nn64_wavek": 0.023,   # measured 0.0111 (bf16 out, K = 2560); K = 1024: 0.0000
    "split_k": 1.7,        # measured 0.8389 (64x64 tt, 2 slabs, K = 256); K = 8000: 0.5197 (4 slabs), 0.2124 (16 slabs)
    "big0": 0.70,          # measured 0.3500 (K = 256); K = 1024: 0.2553
    "big1": 0.73,          # measured 0.3627 (K = 256); K = 1024: 0.2521
    "big2": 0.62,          # measured 0.3086 (K = 1024); K = 256: 0.2704
    "big2_dbias": 0.16,    # measured 0.0786 (K = 256, 6400 rows per column); K = 1024: 0.0380
    "nt_batched": 0.015,   # measured 0.0074 (K = 1088); K = 256: 0.0000
}


def judge(family, K, units, ok_fn):
    """print the measured figure, then hold it to the family's bound"""
    print(f"GEMM_ROUNDING {family} K={K} worst={units:.4f} units of 2^-24 * absprod")
    c = ROUNDING_C[family]
    assert c is not None, f"{family}: no bound set (measured {units:.4f})"
    assert c < K, f"{family}: c = {c} is not below K = {K}"
    assert ok_fn(c), f"{family} K={K}: worst {units:.4f} units exceeds c = {c}"


def gauss(M, N, K, ta, tb, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = stored(torch.randn(M, K, generator=g).to(BF16), ta), stored(torch.randn(N, K, generator=g).to(BF16), tb)
    return a, b, a.to(DEV), b.to(DEV)


# K = 256 and the longest K the family sees in the model (2560: the widest Linear; 8000: the rows of a weight gradient). gemm_nn64_wavek_kernel
# is only selected from 1024 of K per chunk, so its short case is K = 1024.
ROUND_GENERAL = [   # family, forced (tile, splits, ring) or None, layout, out, M, N, K
    ("reg", (0, 0, 0), (0, 0), "bf16", 300, 200, 256), ("reg", (0, 0, 0), (0, 0), "f32", 300, 200, 2560),
    ("reg", (1, 0, 0), (0, 1), "bf16", 300, 200, 2560), ("reg", (2, 0, 0), (1, 1), "acc", 304, 200, 256),
    ("ring", (1, 0, 2), (0, 1), "bf16", 300, 200, 256), ("ring", (1, 0, 2), (0, 0), "f32", 300, 200, 2560),
    ("ring", (0, 0, 2), (1, 0), "bf16", 304, 200, 2560), ("ring", (0, 0, 2), (0, 0), "acc", 300, 200, 256),
    ("tt64_wavek", (2, 0, 2), (1, 1), "f32", 256, 256, 256), ("tt64_wavek", (2, 0, 2), (1, 1), "acc", 256, 256, 8000),
    ("nn64_wavek", (2, 0, 2), (0, 0), "bf16", 300, 200, 1024), ("nn64_wavek", (2, 0, 2), (0, 0), "bf16", 300, 200, 2560),
    ("split_k", (2, 2, 2), (1, 1), "acc", 256, 256, 256), ("split_k", None, (1, 1), "acc", 768, 256, 8000),
    ("split_k", (1, 4, 0), (1, 0), "f32", 256, 256, 8000),
]


@pytest.mark.parametrize("case", ROUND_GENERAL, ids=[f"{c[0]}-{LNAME[c[2]]}-{c[3]}-K{c[6]}" for c in ROUND_GENERAL])
def test_general_rounding(C, L, force, case):
    family, forced_plan, (ta, tb), out, M, N, K = case
    a, b, A, B = gauss(M, N, K, ta, tb, M + N + K)
    ref, absprod = GR.product(a, b, ta, tb)
    c0 = torch.randn(M, N, generator=torch.Generator().manual_seed(2)) if out == "acc" else None
    if c0 is not None:
        ref, absprod = ref + c0.double().numpy(), absprod + c0.abs().double().numpy()
    with force(*(forced_plan or (-1, 0, 1))):
        if family in ("tt64_wavek", "nn64_wavek"):
            assert kernel(M, N, K, ta, tb, OUTS.index(out), *(forced_plan or ())).startswith("gemm_" + family)
        nws = L.tsasr_gemm_bf16_workspace_bytes(M, N, K, C.F32 if out != "bf16" else C.BF16)
        assert (nws > 0) == (family == "split_k")
        ws = torch.full((nws // 4,), float("nan"), dtype=F32, device=DEV).view(torch.uint8) if nws else None
        got = twice(lambda o: gemm(C, L, A, B, o, M, N, K, ta, tb, int(out == "acc"), ws), lambda: GR.poisoned(M, N, N + 8, BF16 if out == "bf16" else F32, 1, c0))
    got = got[:M, :N]
    if out == "bf16":
        judge(family, K, GR.bf16_excess_units(got, ref, absprod), lambda c: GR.bf16_ok(got, ref, absprod, c))
    else:
        judge(family, K, GR.f32_units(got, ref, absprod), lambda c: GR.f32_ok(got, ref, absprod, c))


@pytest.mark.parametrize("M,N,K", [(6400, 2048, 256), (1536, 2048, 1024)])
def test_gemm_big_rounding(C, L, M, N, K):
    """p = 0.1: the dropout scale 65536 / 58982 is no power of two, so a value rounded to bf16 BEFORE the scale shows"""
    p, slope = 0.1, 0.25
    ks = GR.keep_scale(p)
    a, b, A, B = gauss(M, N, K, 0, 0, M + K)
    acc, absprod = GR.product(a, b, 0, 0)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(4))
    got0 = twice(lambda o: gemm(C, L, A, B, o, M, N, K, 0, 0), lambda: GR.poisoned(M, N, N, BF16, 0))
    judge("big0", K, GR.bf16_excess_units(got0, acc, absprod), lambda c: GR.bf16_ok(got0, acc, absprod, c))
    keep = GR.keep_elementwise(M, N, p, SEED)
    bias_d = bias.to(DEV)
    y = twice(lambda o: fused(C, L, A, B, o, M, N, K, 0, 0, 1, bias=bias_d, slope=slope, p=p), lambda: GR.poisoned(M, N, N, BF16, 0))
    ref1, abs1 = GR.mode1(acc, bias, slope, keep, p), absprod + bias.abs().double().numpy()[None, :]
    judge("big1", K, GR.bf16_excess_units(y, ref1, abs1, ks), lambda c: GR.bf16_ok(y, ref1, abs1, c, ks))
    t = GR.mode2(acc, y, slope, keep, p)
    db = torch.full((1, N), float("nan"), dtype=F32, device=DEV)
    ws = torch.full((L.tsasr_gemm_bf16_fused_workspace_bytes(M, N) // 4,), float("nan"), dtype=F32, device=DEV).view(torch.uint8)
    y_d = y.to(DEV)
    dx = twice(lambda o: fused(C, L, A, B, o, M, N, K, 0, 0, 2, y=y_d, slope=slope, p=p, dbias=db, ws=ws), lambda: GR.poisoned(M, N, N, BF16, 0))
    judge("big2", K, GR.bf16_excess_units(dx, t, absprod, ks), lambda c: GR.bf16_ok(dx, t, absprod, c, ks))
    torch.cuda.synchronize()
    col = (absprod * ks).sum(0)[None, :]                         # >= sum_m |t|: the same unit over the column
    judge("big2_dbias", K, GR.f32_units(db.cpu(), GR.dbias(t)[None, :], col), lambda c: GR.f32_ok(db.cpu(), GR.dbias(t)[None, :], col, c))


@pytest.mark.parametrize("K", [256, 1088])
def test_nt_batched_rounding(C, L, K):
    M, N, nbatch = 100, 136, 3
    g = torch.Generator().manual_seed(K)
    a = torch.randn(M, K, generator=g).to(BF16)
    bs = [torch.randn(N, K, generator=g).to(BF16) for _ in range(nbatch)]
    A, Bs = a.to(DEV), [b.to(DEV) for b in bs]
    out = torch.full((nbatch * M * N,), float("nan"), dtype=BF16, device=DEV)
    assert batched(C, L, A, Bs, out, M, N, K, N, M * N) == 0
    got = out.cpu().view(nbatch, M, N)
    refs = [GR.product(a, b, 0, 0) for b in bs]
    worst = max(GR.bf16_excess_units(got[i], r, ap) for i, (r, ap) in enumerate(refs))
    judge("nt_batched", K, worst, lambda c: all(GR.bf16_ok(got[i], r, ap, c) for i, (r, ap) in enumerate(refs)))


# ---------------------------------------------------------------------------------------------- last: the automatic plan is back
def test_zz_automatic_plan_restored(C, L):
    assert L.tsasr_gemm_bf16_fused_mask_ok(8000, 2048, 256) == 1
    assert L.tsasr_gemm_bf16_workspace_bytes(2048, 256, 8000, C.F32) > 0 and L.tsasr_gemm_bf16_workspace_bytes(128, 128, 256, C.F32) == 0
