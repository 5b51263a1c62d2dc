"""The gradient tail - everything between a finished backward pass and next step's weights - path by path through the C-ABI against
float64 (tests/helpers/gradtail_ref.py):

    clip + AdamW          tsasr_clip_adamw_step       sumsq_partials_kernel (unrolled / single-load / scalar tail / empty parts), clip_adamw_kernel
                                                      (16-byte groups, scalar tail, grid-stride second pass), every clip regime, the bf16 shadow
    non-finite counter    tsasr_count_nonfinite
    deferred adds         tsasr_accumulate_many       16 workgroups per vector, interleaved 256-element pieces
    weight transposes     tsasr_transpose_many_bf16   vectorised whole-tile path / guarded general path, the per-workgroup job search
    grouped dW            tsasr_wgrad_queue / _flush  <32, 4> and <32, 2> rings, one workgroup per tile and the persistent tile walk, 1 .. 7 k-tiles
                                                      with and without a ragged last one, the K-descending job order, the 64-ary job search, the
                                                      XCD remap at every remainder
    batched reductions    tsasr_reduce_flush{,_stream}  tall and wide jobs, 1 .. 300 jobs, two streams
    the arena             dp.GradArena + optim.FusedClipAdamW   alignment of every bf16 view, shadows, transposed copies, pad words, re-layout

Every case: outputs start as a sentinel or NaN, a guard block sits behind every buffer, inputs are compared bit for bit afterwards. Exact-regime
cases (small integers: every fp32 summation order gives the float64 result) have tolerance 0; Gaussian optimizer cases are held to
gradtail_ref.TOL (4 x the deltas of an fp32 restatement measured on the CPU) and to the derived norm bound; Gaussian weight gradients to
ceil(K / 16) + 2 units of 2^-24 (|dy|^T |x| + |dW0|): one rounding of at most an fp32 ulp (2 units: the MFMA need not round to nearest) of
the partial sum so far per 16-row MFMA step - (J + 1) units over J steps - and one for the final read-add-store."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_ref as G  # noqa: E402
import gradtail_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SENT, GUARD = -7.0, 64
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


@pytest.fixture(scope="module")
def ops():
    o = importlib.import_module("ts-asr_amd.ops")
    o.reduce_defer_prepare(torch.device(DEV))
    yield o
    o.discard_queues()


def gbuf(n, dtype=F32, fill=0.0, guard=SENT):
    """[n] of `fill` with GUARD elements of `guard` behind it, one allocation"""
    t = torch.full((n + GUARD,), guard, dtype=dtype, device=DEV)
    t[:n] = fill
    return t


def put(x, dtype=F32, guard=SENT):
    x = torch.as_tensor(x)
    t = gbuf(x.numel(), dtype, 0, guard)
    t[:x.numel()] = x.reshape(-1).to(dtype)
    return t


def guard_ok(t, n, guard=SENT):
    g = t[n:]
    return bool((g != g).all()) if guard != guard else bool((g == guard).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


# ================================================================================================== clip + AdamW
class Opt:
    """p, m, v, g, the bf16 shadow, the workspace (exactly tsasr_clip_adamw_workspace_bytes() with a guard behind it), one-float norm and
    skip-counter slots in the middle of sentinel blocks"""

    def __init__(self, C, p, m=None, v=None, shadow=True):
        self.C, self.lib, self.n = C, C.lib(), int(np.asarray(p).size)
        n = self.n
        self.p = put(p)
        self.m = put(np.zeros(n, np.float32) if m is None else m)
        self.v = put(np.zeros(n, np.float32) if v is None else v)
        self.g = gbuf(n)
        self.p16 = gbuf(n, BF16, float("nan"), SENT) if shadow else None
        self.ws_bytes = int(self.lib.tsasr_clip_adamw_workspace_bytes())
        self.ws = torch.full((self.ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.slots = torch.full((64,), 7.0, dtype=F32, device=DEV)       # [31] = norm, [47] = skipped steps
        self.slots[47] = 0.0
        self.hyper = torch.zeros(3, dtype=F32, device=DEV)

    def step(self, g, hyper, max_norm, norm=True, skipped=False, adam=R.ADAM):
        C, n = self.C, self.n
        if g is not None:
            self.g[:n] = torch.as_tensor(g).to(DEV)
        g0 = self.g.clone()
        self.hyper.copy_(torch.from_numpy(np.asarray(hyper, dtype=np.float32)))
        self.slots[31] = 7.0
        C.check(self.lib.tsasr_clip_adamw_step(C.ptr(self.p), C.ptr(self.p16), C.ptr(self.g), C.ptr(self.m), C.ptr(self.v), C.ptr(self.hyper),
                                               C.ptr(self.slots[31:32]) if norm else None, C.ptr(self.slots[47:48]) if skipped else None, n,
                                               adam["beta1"], adam["beta2"], adam["eps"], adam["wd"], float(max_norm), C.ptr(self.ws), self.ws_bytes,
                                               C.stream_ptr()), "tsasr_clip_adamw_step")
        torch.cuda.synchronize()
        assert same_bits(self.g, g0), "the gradient was modified"
        for name in ("p", "m", "v", "g"):
            assert guard_ok(getattr(self, name), n), f"{name}: written past its end"
        assert bool((self.ws[self.ws_bytes:] == 0xA5).all()), "workspace: written past tsasr_clip_adamw_workspace_bytes()"
        keep = torch.ones(64, dtype=torch.bool)
        keep[31], keep[47] = False, False
        assert bool((self.slots.cpu()[keep] == 7.0).all()), "norm_out / skipped_out: a neighbour was written"
        if not norm:
            assert float(self.slots[31]) == 7.0
        if self.p16 is not None:
            assert guard_ok(self.p16, n), "p16: written past its end"
            bad = torch.nonzero(bits(self.p16[:n]) != bits(self.p[:n].to(BF16)))
            assert len(bad) == 0, f"p16 is not bf16(p) at {len(bad)} of {n} elements, first at {int(bad[0])}"
        return float(self.slots[31]) if norm else None

    def state(self):
        n = self.n
        return {k: getattr(self, k)[:n].cpu().numpy() for k in ("p", "m", "v")}


def hold(got, ref, prev, n, what):
    """p, m, v within gradtail_ref.TOL of adamw_step64 (computed from the kernel's own previous state), the norm within the derived bound"""
    e = R.update_errors(got, ref, prev)
    print(f"GRADTAIL_ADAMW {what}: errors {({k: round(x, 3) for k, x in e.items()})} (fp32 ulps; bounds {R.TOL['gpu']}, norm in units of 2^-24 norm: "
          f"bound {R.norm_bound(n, ref['norm'] ** 2) / (R.U * max(ref['norm'], 1e-300)):.1f})")
    for k in ("p", "m", "v"):
        assert e[k] <= R.TOL["gpu"][k], f"{what}: {k} is {e[k]:.2f} fp32 ulps from float64, bound {R.TOL['gpu'][k]}"
    assert abs(got["norm"] - ref["norm"]) <= R.norm_bound(n, ref["norm"] ** 2), f"{what}: norm {got['norm']!r} vs {ref['norm']!r}"


@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_adamw_exact_norm(C, n):
    """A gradient in {-2 .. 2} with sum of squares S < 2^24: every partial sum is an integer, so norm_out must be sqrtf(S) bit for bit - one
    element dropped, doubled or read from a wrong place changes S. Then single non-zeros at element 0, n - 1 and the ends of a middle part."""
    g, ss = R.exact_gradient(n, n)
    o = Opt(C, np.zeros(n, np.float32))
    h = R.hyper3(1e-3, 0.9, 0.98, 1)
    norm = o.step(g, h, 0.0)
    want = float(np.sqrt(np.float32(ss)))
    assert norm == want, f"n = {n}: norm_out {norm!r}, sqrtf({ss}) = {want!r}: the partials summed to {norm * norm:.1f}"
    for pos in R.single_positions(n):
        o.g[:n] = 0.0
        o.g[pos] = -2.0
        assert o.step(None, h, 5.0) == 2.0, f"n = {n}: a single -2 at element {pos} gave norm {float(o.slots[31])!r}"
    o.g[:n] = 0.0
    assert o.step(None, h, 5.0) == 0.0


@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_adamw_gaussian_three_steps(C, n):
    """3 steps, t and lr changing through the device array; p, m, v after every step against adamw_step64, p16 = bf16(p) bit for bit"""
    p0, gs = R.gaussian_case(n, 100 + n % 97)
    o = Opt(C, p0)
    for t in (1, 2, 3):
        h = R.hyper3(R.STEP_LR[t - 1], 0.9, 0.98, t)
        prev = {k: x.astype(np.float64) for k, x in o.state().items()}
        norm = o.step(gs[t - 1], h, 5.0)
        ref = R.adamw_step64(prev["p"], gs[t - 1], prev["m"], prev["v"], h, max_norm=5.0, **R.ADAM)
        assert n < 64 or ref["clip"] < 1
        got = o.state()
        got["norm"] = norm
        hold(got, ref, prev, n, f"n={n} t={t}")


@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("n", [1025, 4099])
def test_adamw_clip_regimes(C, n, regime):
    max_norm = R.REGIMES[regime]
    p0, gs = R.gaussian_case(n, 7, regime)
    o = Opt(C, p0)
    for t in (1, 2, 3):
        h = R.hyper3(R.STEP_LR[t - 1], 0.9, 0.98, t)
        prev = {k: x.astype(np.float64) for k, x in o.state().items()}
        norm = o.step(gs[t - 1], h, max_norm)
        ref = R.adamw_step64(prev["p"], gs[t - 1], prev["m"], prev["v"], h, max_norm=max_norm, **R.ADAM)
        assert (ref["clip"] < 1) == (regime == "clipped")
        got = o.state()
        got["norm"] = norm
        hold(got, ref, prev, n, f"{regime} n={n} t={t}")
        if regime == "zero_grad":       # parameters only decay, moments stay zero, nothing becomes NaN
            assert norm == 0.0 and not got["m"].any() and not got["v"].any() and np.isfinite(got["p"]).all()
            decay = (np.float32(1) - np.float32(h[0]) * np.float32(0.01), np.float32(1.0 - float(h[0]) * R.r32(0.01)))    # separate roundings | one fused
            assert any(np.array_equal(got["p"], prev["p"].astype(np.float32) * d) for d in decay)


def test_adamw_optional_outputs(C):
    """norm_out and skipped_out NULL in each combination: the same update bit for bit, nothing written where a pointer was not given"""
    n = 1025
    p0, gs = R.gaussian_case(n, 9)
    h = R.hyper3(1e-3, 0.9, 0.98, 1)
    res = []
    for norm in (True, False):
        for skipped in (True, False):
            o = Opt(C, p0)
            o.step(gs[0], h, 5.0, norm=norm, skipped=skipped)
            assert float(o.slots[47]) == 0.0
            res.append(o.state())
    for r in res[1:]:
        for k in ("p", "m", "v"):
            assert np.array_equal(r[k], res[0][k]), k


def test_adamw_largest_finite_norm_is_a_normal_step(C):
    """The largest norm the kernel can form is finite for `finite`: sqrtf of a sum of squares just below FLT_MAX (1.8e19). A normal step,
    with and without a counter."""
    n = 1025
    p0, _ = R.gaussian_case(n, 9)
    g = np.zeros(n, np.float32)
    g[3], g[1024] = 1.3e19, -1.3e19
    h = R.hyper3(1e-3, 0.9, 0.98, 1)
    for skipped in (True, False):
        o = Opt(C, p0)
        prev = {k: x.astype(np.float64) for k, x in o.state().items()}
        norm = o.step(g, h, 5.0, skipped=skipped)
        ref = R.adamw_step64(prev["p"], g, prev["m"], prev["v"], h, max_norm=5.0, skip=skipped, **R.ADAM)
        got = o.state()
        got["norm"] = norm
        assert float(o.slots[47]) == 0.0 and np.isfinite(norm)
        hold(got, ref, prev, n, f"norm 1.8e19 skipped={skipped}")


def test_adamw_norm_between_3e38_and_flt_max_is_a_normal_step(C):
    """A gradient whose L2 norm lies in (3.0e38, FLT_MAX] is finite, so with a counter passed the step is a normal one (float64: norm 3.2e38,
    clip factor 1.56e-38, an ordinary update), not a skipped one. The plain fp32 sum of squares is +Inf above sqrt(FLT_MAX) = 1.84e19 (the
    kernel used to report norm_out = inf and skip the step there); sumsq_partials_kernel keeps a second row of partials of (g 2^-64)^2 for
    that case. One element of 3.2e38; two of 2e38 in different parts; and a norm of 5.2e38, which is no fp32 number:
    that one IS non-finite for the kernel and is skipped."""
    n = 5000
    p0, _ = R.gaussian_case(n, 9)
    h = R.hyper3(1e-3, 0.9, 0.98, 1)
    grads = {"one": np.zeros(n, np.float32), "two": np.zeros(n, np.float32), "max": np.zeros(n, np.float32)}
    grads["one"][5] = 3.2e38
    grads["two"][7], grads["two"][n - 2] = 2.0e38, -2.0e38
    grads["max"][n - 1] = -FLT_MAX
    for name, g in grads.items():
        for skipped in (True, False):
            o = Opt(C, p0)
            prev = {k: x.astype(np.float64) for k, x in o.state().items()}
            norm = o.step(g, h, 5.0, skipped=skipped)
            ref = R.adamw_step64(prev["p"], g, prev["m"], prev["v"], h, max_norm=5.0, skip=skipped, **R.ADAM)
            assert ref["skipped"] == 0 and 2.8e38 < ref["norm"] <= FLT_MAX
            got = o.state()
            got["norm"] = norm
            print(f"GRADTAIL_ADAMW {name}: norm_out {norm!r} (float64 {ref['norm']!r}), skipped {float(o.slots[47])}")
            assert float(o.slots[47]) == 0.0, f"{name}: the step was skipped (norm_out = {norm!r})"
            hold(got, ref, prev, n, f"huge norm, {name}, counter {skipped}")
    g = np.zeros(n, np.float32)
    g[1], g[2500], g[n - 1] = 3.0e38, 3.0e38, -3.0e38
    o = Opt(C, p0)
    o.p16[:n] = o.p[:n].to(BF16)          # (a skipped step leaves the shadow alone)
    assert o.step(g, h, 5.0, skipped=True) == float("inf") and float(o.slots[47]) == 1.0 and np.array_equal(o.state()["p"], p0)


# ================================================================================================== tsasr_count_nonfinite
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_count_nonfinite(C, n):
    """NaN, +-Inf, several per lane, none, a counter that starts non-zero; 3.2e38 and FLT_MAX are finite. The guard behind x is NaN: a read
    past n would be counted."""
    lib = C.lib()
    rng = np.random.default_rng(n)
    base = rng.standard_normal(n).astype(np.float32)
    base[rng.integers(0, n, size=max(1, n // 7))] = 3.2e38
    base[rng.integers(0, n, size=max(1, n // 9))] = -FLT_MAX
    base[0] = FLT_MAX
    cases = {"none": []}
    cases["nan_first"], cases["inf_last"], cases["ninf_mid"] = [(0, np.nan)], [(n - 1, np.inf)], [(n // 2, -np.inf)]
    cases["several"] = [(i, (np.nan, np.inf, -np.inf)[i % 3]) for i in sorted({0, n - 1, n // 2, n // 3, *range(1, n, 64), *range(5, n, 129)})]
    cases["all"] = [(i, np.nan) for i in range(n)]
    for name, bad in cases.items():
        x = base.copy()
        for i, val in bad:
            x[i] = val
        want = int((~np.isfinite(x)).sum())
        assert want == len(bad)
        for start in (0, 41):
            xd = put(x, F32, float("nan"))
            x0 = xd.clone()
            cnt = torch.full((64,), -77, dtype=torch.int32, device=DEV)
            cnt[31] = start
            C.check(lib.tsasr_count_nonfinite(C.ptr(xd), n, C.ptr(cnt[31:32]), C.stream_ptr()), "tsasr_count_nonfinite")
            torch.cuda.synchronize()
            assert int(cnt[31]) == start + want, f"n = {n}, {name}: counted {int(cnt[31]) - start}, {want} are NaN / Inf"
            assert int((cnt == -77).sum()) == 63 and same_bits(xd, x0)


# ================================================================================================== tsasr_accumulate_many
def _acc_table(srcs, dsts, lens):
    n = len(srcs)
    tab = np.empty(n * 20, np.uint8)         # as dp.GradArena._flush_deferred lays it out
    tab[:n * 8].view(np.uint64)[:] = [s.data_ptr() for s in srcs]
    tab[n * 8:n * 16].view(np.uint64)[:] = [d.data_ptr() for d in dsts]
    tab[n * 16:].view(np.int32)[:] = lens
    return torch.from_numpy(tab).to(DEV)


@pytest.mark.parametrize("count", R.ACC_COUNTS)
def test_accumulate_many(C, count):
    """dst slices of ONE arena at odd element offsets, a sentinel gap between slots; dst0 + src in fp32 is a single rounding: exact"""
    lens = R.acc_lengths(count)
    if count == 70:
        assert set(lens) == set(R.ACC_LENS)
    gen = torch.Generator().manual_seed(count)
    offs, off = [], 3
    for ln in lens:
        offs.append(off)
        off += ln + 5 + (ln % 2 == 0)          # every offset odd
    assert all(o % 2 == 1 for o in offs)
    arena0 = torch.full((off + GUARD,), SENT)
    srcs, want = [], arena0.clone()
    for o, ln in zip(offs, lens):
        d0, s = torch.randn(ln, generator=gen), torch.randn(ln, generator=gen) * 3
        arena0[o:o + ln] = d0
        want[o:o + ln] = d0 + s
        srcs.append(put(s, F32, float("nan")))
    arena = arena0.to(DEV)
    src0 = [s.clone() for s in srcs]
    tab = _acc_table(srcs, [arena[o:] for o in offs], lens)
    C.check(C.lib().tsasr_accumulate_many(C.ptr(tab), count, C.stream_ptr()), "tsasr_accumulate_many")
    torch.cuda.synchronize()
    bad = torch.nonzero(bits(arena.cpu()) != bits(want))
    assert len(bad) == 0, f"{len(bad)} elements of the arena differ from dst0 + src (or a gap was written), first at element {int(bad[0])} (slots start at {offs[:8]})"
    assert all(same_bits(a, b) for a, b in zip(srcs, src0))


# ================================================================================================== tsasr_transpose_many_bf16
@pytest.mark.parametrize("pad", [R.PAD, 1])
@pytest.mark.parametrize("njobs", [1, 2, 33])
def test_transpose_many(C, njobs, pad):
    """Job list as dp.GradArena.refresh_shadow builds it (pad = 64: transposed copies at multiples of 64 elements; pad = 1: packed back to back,
    so the odd 17 x 241 pushes every later copy - the aligned 128 x 128 among them - to an odd offset and onto the general path, which moves
    2 bytes at a time). Every element a distinct 16-bit pattern; dst must be .t() of each source bit for bit, gaps and guards untouched."""
    mats = R.tr_mats(njobs)
    jobs, tiles, t_total = R.transpose_jobs(mats, pad=pad)
    if pad == 1 and njobs > 1:
        assert any((r, c) == (128, 128) and do % 2 == 1 for _, do, r, c, _ in jobs)
    s_total = jobs[-1][0] + mats[-1][0] * mats[-1][1]
    src = torch.full((s_total + GUARD,), 0x1234, dtype=torch.int16)
    src[:s_total] = R.distinct_bits(s_total)
    dst0 = torch.full((t_total + GUARD,), -21555, dtype=torch.int16)
    want = dst0.clone()
    for so, do, r, c, _ in jobs:
        want[do:do + r * c] = src[so:so + r * c].view(r, c).t().reshape(-1)
    sd, dd = src.to(DEV), dst0.to(DEV)
    jt = torch.tensor(jobs, dtype=torch.int32).reshape(-1).to(DEV)
    C.check(C.lib().tsasr_transpose_many_bf16(C.ptr(sd), C.ptr(dd), C.ptr(jt), len(jobs), tiles, C.stream_ptr()), "tsasr_transpose_many_bf16")
    torch.cuda.synchronize()
    got = dd.cpu()
    if not torch.equal(got, want):
        e = int(torch.nonzero(got != want)[0])
        j = max((k for k in range(len(jobs)) if jobs[k][1] <= e), default=0)
        raise AssertionError(f"{int((got != want).sum())} elements differ, first at dst element {e} (job {j} = {jobs[j]}, fast path "
                             f"{[R.transpose_fast(jobs[j], lt) for lt in range(min(8, R.cdiv(jobs[j][2], 64) * R.cdiv(jobs[j][3], 64)))]}): "
                             f"got {int(got[e]) & 0xffff:#06x}, want {int(want[e]) & 0xffff:#06x}")
    assert torch.equal(sd.cpu(), src)


# ================================================================================================== grouped weight gradients
class WJob:
    """one dW [M, N] (+)= dy [K, M]^T . x [K, N]: operands row-strided inside NaN-poisoned allocations, dW a window of a poisoned [M + 2, ldc]"""

    def __init__(self, M, N, K, gen, amp=3, onehot=None, gauss=False, strided=True):
        self.M, self.N, self.K = M, N, K
        if onehot is not None:
            k, m, n = onehot
            dy, x = torch.zeros(K, M, dtype=BF16), torch.zeros(K, N, dtype=BF16)
            dy[k, m], x[k, n] = 1.0, 1.0
            w0 = torch.zeros(M, N)
        elif gauss:
            dy, x, w0 = torch.randn(K, M, generator=gen).to(BF16), torch.randn(K, N, generator=gen).to(BF16), torch.randn(M, N, generator=gen)
        else:
            dy, x = G.int_operand(K, M, amp, gen), G.int_operand(K, N, amp, gen)
            w0 = torch.randint(-64, 65, (M, N), generator=gen).float()
        self.dy_cpu, self.x_cpu, self.w0 = dy, x, w0
        self.dy = G.place(dy, M + 8 if strided else M, 8 if strided else 0, DEV)
        self.x = G.place(x, N + 16 if strided else N, 0, DEV)
        self.ldc = N + 8 if strided else N
        self.dy_bits, self.x_bits = bits(self.dy).clone(), bits(self.x).clone()

    def fresh(self):
        self.buf = G.poisoned(self.M, self.N, self.ldc, F32, c0=self.w0).to(DEV)
        return self.buf[:self.M, :self.N]

    def reference(self):
        prod, absprod = G.product(self.dy_cpu, self.x_cpu, 1, 1)
        return prod + self.w0.double().numpy(), absprod


def flush(ops, C, jobs, slots=0, wgs=0):
    """queue every job on a fresh dW, set the one-shot knobs, flush; returns the dW buffers (guards included) on the CPU"""
    views = [j.fresh() for j in jobs]
    for i, (j, w) in enumerate(zip(jobs, views)):
        assert ops.wgrad_queue(None, w, j.dy, j.x, key=("gradtail", i))
    assert ops.wgrad_pending() == len(jobs) == C.lib().tsasr_wgrad_pending()
    if slots:
        C.lib().tsasr_wgrad_next_flush_slots(slots)
    if wgs:
        C.lib().tsasr_wgrad_next_flush_wgs(wgs)
    ops.wgrad_flush()
    torch.cuda.synchronize()
    assert ops.wgrad_pending() == 0 == C.lib().tsasr_wgrad_pending()
    for j in jobs:
        assert torch.equal(bits(j.dy), j.dy_bits) and torch.equal(bits(j.x), j.x_bits), "an operand was modified"
    return [j.buf.cpu() for j in jobs]


def all_variants(ops, C, jobs, what, variants=None):
    """every launch variant on the same inputs: exact against float64 (guards NaN), and bit-identical to the default launch; then a flush
    WITHOUT knobs, which must again be the default (the knobs are one-shot)"""
    _, _, tiles = R.wgrad_plan([(j.M, j.N, j.K) for j in jobs])
    refs = []
    for j in jobs:
        ref, absprod = j.reference()
        G.assert_exact_regime(absprod, c0=j.w0, what=what)
        refs.append(ref)
    base = None
    for name, slots, wgs in (variants or R.wg_variants(tiles)) + [("default_again", 0, 0)]:
        got = flush(ops, C, jobs, slots, wgs)
        for k, (j, buf, ref) in enumerate(zip(jobs, got, refs)):
            G.check_exact(buf, ref, j.M, j.N, tile=(256, 256), what=f"{what} [{name}] job {k} ({j.M} x {j.N}, K = {j.K}, {tiles} tiles)")
        if base is None:
            base = got
        assert all(torch.equal(bits(a[:j.M, :j.N]), bits(b[:j.M, :j.N])) for a, b, j in zip(base, got, jobs)), f"{what}: {name} differs from the default launch"
    return tiles


@pytest.mark.parametrize("M,N", R.WG_MN)
def test_wgrad_exact_every_k(ops, C, M, N):
    """K = 1 .. 200: 1 - 7 k-tiles of 32 rows, each with and without a ragged last tile, across the wrap of the 4-slot and the 2-slot ring; one
    flush holds all 13 (so the K-descending sort reorders them); row-strided operands, a dW window with ldc > N, integer initial dW"""
    gen = torch.Generator().manual_seed(M * 1000 + N)
    jobs = [WJob(M, N, K, gen) for K in R.WG_K]
    all_variants(ops, C, jobs, f"{M}x{N}")


def test_wgrad_one_hot_rows(ops, C):
    """a single 1 in dy at (k, m) and in x at (k, n), k at the first and last row of every k-tile and the last valid row of the ragged tail:
    dW changes at (m, n) only - a k-row dropped, taken twice or taken from a stale ring slot shows as 0 or 2"""
    K, M, N = 200, 264, 256
    ks = sorted({0, K - 1, *[32 * t for t in range(7)], *[32 * t + 31 for t in range(6)]})
    gen = torch.Generator().manual_seed(0)
    for Kj, rows in ((K, ks), (33, [0, 31, 32]), (1, [0])):
        jobs = [WJob(M, N, Kj, gen, onehot=(k, (k * 37 + 5) % M, (k * 91 + 3) % N)) for k in rows]
        for name, slots, wgs in (("default", 0, 0), ("slots2", 2, 0), ("wgs3", 0, 3), ("slots2_wgs3", 2, 3)):
            for k, buf in zip(rows, flush(ops, C, jobs, slots, wgs)):
                want = np.zeros((M, N))
                want[(k * 37 + 5) % M, (k * 91 + 3) % N] = 1.0
                G.check_exact(buf, want, M, N, tile=(256, 256), what=f"one-hot k = {k} of K = {Kj} [{name}]")


@pytest.mark.parametrize("count", R.WG_MANY)
def test_wgrad_many_jobs(ops, C, count):
    """1 .. 200 small jobs with distinct K in scrambled order and one 520 x 264 job in the middle: the stable K-descending sort and both
    levels of the 64-ary job search"""
    shapes = R.many_jobs(count)
    gen = torch.Generator().manual_seed(count)
    jobs = [WJob(M, N, K, gen, strided=False) for M, N, K in shapes]
    tiles = all_variants(ops, C, jobs, f"{count} jobs", variants=[("default", 0, 0), ("slots2", 2, 0), ("wgs3", 0, 3), ("slots2_wgs3", 2, 3)])
    assert tiles == sum(R.wgrad_tiles(M, N) for M, N, _ in shapes)


@pytest.mark.parametrize("tiles", range(1, 18))
def test_wgrad_every_tile_count(ops, C, tiles):
    """total tiles 1 .. 17: every remainder of the XCD remap (total & 7) with runs of one and of two tiles per XCD, every variant"""
    gen = torch.Generator().manual_seed(tiles)
    jobs = [WJob(M, N, K, gen, strided=False) for M, N, K in R.tiles_jobs(tiles)]
    assert all_variants(ops, C, jobs, f"{tiles} tiles") == tiles


WG_GAUSS = [
    [(2048, 256, 8000), (256, 2048, 8000), (768, 256, 8000), (256, 256, 8000)],
    [(2048, 256, 4000), (512, 256, 4000), (640, 256, 8000), (640, 512, 3872), (256, 2560, 8000)],
    [(8, 8, 1), (24, 40, 63), (264, 256, 65), (256, 264, 128), (136, 520, 200)],
]


@pytest.mark.parametrize("shapes", WG_GAUSS, ids=["layer", "ragged", "tiny"])
def test_wgrad_gaussian_per_element(ops, C, shapes):
    """the three shape lists of tests/test_wgrad_gpu.py, held per element to ceil(K / 16) + 2 units of 2^-24 (|dy|^T |x| + |dW0|) (module
    docstring) instead of one absolute tolerance per matrix; float64 products by torch on the GPU. Default launch and the persistent walk."""
    gen = torch.Generator().manual_seed(len(shapes) * 13)
    jobs = [WJob(M, N, K, gen, gauss=True, strided=False) for M, N, K in shapes]
    refs = []
    for j in jobs:
        a, b = j.dy_cpu.to(DEV).double(), j.x_cpu.to(DEV).double()
        refs.append(((a.t() @ b).cpu().numpy() + j.w0.double().numpy(), (a.abs().t() @ b.abs()).cpu().numpy() + j.w0.abs().double().numpy()))
    base = None
    for name, slots, wgs in (("default", 0, 0), ("wgs5", 0, 5)):
        got = flush(ops, C, jobs, slots, wgs)
        for j, buf, (ref, unit) in zip(jobs, got, refs):
            w = buf[:j.M, :j.N].numpy()
            c = R.cdiv(j.K, 16) + 2
            print(f"GRADTAIL_WGRAD {j.M}x{j.N} K={j.K} [{name}]: worst {G.f32_units(w, ref, unit):.3f} units of 2^-24 (|dy|^T |x| + |dW0|), bound {c}")
            assert G.f32_ok(w, ref, unit, c), f"{j.M}x{j.N} K={j.K} [{name}]: worst {G.f32_units(w, ref, unit):.2f} units, bound {c}"
        if base is not None:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(base, got))
        base = got


# ================================================================================================== batched reductions
class RJob:
    def __init__(self, C, spec, gen):
        self.C, self.lib, self.spec = C, C.lib(), spec
        if spec[0] == "colsum":
            _, M, N, acc = spec
            self.x = torch.randint(-3, 4, (M, N), generator=gen).float()
            self.out0 = torch.randint(-50, 51, (N,), generator=gen).float() if acc else torch.full((N,), SENT)
            self.ref = self.x.double().sum(0) + (self.out0.double() if acc else 0)
            self.nparts, self.width = R.colsum_parts(M), N
            self.xd = self.x.to(DEV)
            self.ws_bytes = int(self.lib.tsasr_colsum_workspace_bytes(M, N))
        else:
            _, M, N, K = spec
            self.a, self.b = G.int_operand(M, K, 3, gen), G.int_operand(N, K, 3, gen)
            self.out0 = torch.randint(-50, 51, (M * N,), generator=gen).float()
            prod, absprod = G.product(self.a, self.b, 0, 0)
            G.assert_exact_regime(absprod, c0=self.out0.view(M, N), what=str(spec))
            self.ref = torch.from_numpy(prod).reshape(-1) + self.out0.double()
            self.nparts, self.width = R.gemm_splits(M, N, K)[0], M * N
            self.ad, self.bd = self.a.to(DEV), self.b.to(DEV)
            self.ws_bytes = int(self.lib.tsasr_gemm_bf16_workspace_bytes(M, N, K, C.F32))
            assert self.ws_bytes == R.gemm_splits(M, N, K)[1] and R.reduce_wide(self.nparts, self.width)

    def submit(self):
        C, lib = self.C, self.lib
        self.out = put(self.out0)
        self.ws = torch.full((self.ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        if self.spec[0] == "colsum":
            _, M, N, acc = self.spec
            C.check(lib.tsasr_colsum(C.ptr(self.xd), C.ptr(self.out), M, N, acc, C.F32, C.ptr(self.ws), self.ws_bytes, C.stream_ptr()), "tsasr_colsum")
        else:
            _, M, N, K = self.spec
            C.check(lib.tsasr_gemm_bf16(C.ptr(self.ad), C.ptr(self.bd), C.ptr(self.out), M, N, K, K, K, N, 0, 0, C.F32, 2, C.ptr(self.ws), self.ws_bytes,
                                        C.stream_ptr()), "tsasr_gemm_bf16")

    def untouched(self):
        return same_bits(self.out[:self.width].cpu(), self.out0)

    def check(self, what):
        got = self.out.cpu()
        assert guard_ok(got, self.width) and bool((self.ws[self.ws_bytes:] == 0xA5).all()), f"{what}: guard written"
        bad = torch.nonzero(got[:self.width].double() != self.ref)
        assert len(bad) == 0, f"{what} {self.spec}: {len(bad)} of {self.width} outputs differ from float64, first at column {int(bad[0])}: {float(got[int(bad[0])])} vs {float(self.ref[int(bad[0])])}"
        return got[:self.width].clone()


@pytest.mark.parametrize("count", R.RD_COUNTS)
def test_reduce_many(ops, C, count):
    """J deferred reductions - tsasr_colsum (tall jobs; widths 8, 64, 72, 520, accumulate on every other one) and split-K tsasr_gemm_bf16 with
    accumulate = 2 (wide jobs: width M N >= 4096, always a multiple of 4 because the launcher requires N % 4 == 0, so the ragged end of the
    wide branch cannot be reached through the C-ABI) - in one launch: exact against float64, equal to the immediate path bit for bit"""
    lib = C.lib()
    gen = torch.Generator().manual_seed(count)
    jobs = [RJob(C, s, gen) for s in R.reduce_jobs(count)]
    for j in jobs:                                   # immediate path
        j.submit()
    torch.cuda.synchronize()
    now = [j.check("immediate") for j in jobs]
    try:
        C.check(lib.tsasr_reduce_defer(1), "tsasr_reduce_defer")
        for j in jobs:
            j.submit()
        torch.cuda.synchronize()
        assert lib.tsasr_reduce_pending() == count and all(j.untouched() for j in jobs), "a deferred reduction ran before the flush"
        ops._reduce_flush("tsasr_reduce_flush")
        torch.cuda.synchronize()
        assert lib.tsasr_reduce_pending() == 0
        C.check(lib.tsasr_reduce_defer(0), "tsasr_reduce_defer")
        for k, (j, a) in enumerate(zip(jobs, now)):
            assert same_bits(j.check(f"deferred job {k} of {count}"), a), f"job {k}: batched and immediate results differ"
    finally:
        ops.discard_queues()


def test_reduce_flush_stream(ops, C):
    """jobs queued from two streams, interleaved: tsasr_reduce_flush_stream runs exactly the calling stream's jobs (the others' outputs keep
    their initial contents, tile0 of what is left is renumbered), the final flush completes the rest"""
    lib = C.lib()
    gen = torch.Generator().manual_seed(5)
    specs = R.reduce_jobs(37)
    jobs = [RJob(C, s, gen) for s in specs]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    try:
        C.check(lib.tsasr_reduce_defer(1), "tsasr_reduce_defer")
        for k, j in enumerate(jobs):
            with torch.cuda.stream(s2 if k % 3 == 1 else s1):
                j.submit()
        mine = [j for k, j in enumerate(jobs) if k % 3 != 1]
        rest = [j for k, j in enumerate(jobs) if k % 3 == 1]
        assert lib.tsasr_reduce_pending() == len(jobs)
        with torch.cuda.stream(s1):
            ops._reduce_flush("tsasr_reduce_flush_stream")
        assert lib.tsasr_reduce_pending() == len(rest)
        e1, e2 = torch.cuda.Event(), torch.cuda.Event()
        e1.record(s1)
        e2.record(s2)
        torch.cuda.current_stream().wait_event(e1)
        torch.cuda.current_stream().wait_event(e2)
        torch.cuda.synchronize()
        for j in mine:
            j.check("stream flush")
        assert all(j.untouched() for j in rest), "the stream flush ran another stream's job"
        ops._reduce_flush("tsasr_reduce_flush")
        torch.cuda.synchronize()
        assert lib.tsasr_reduce_pending() == 0
        for j in jobs:
            j.check("final flush")
        C.check(lib.tsasr_reduce_defer(0), "tsasr_reduce_defer")
    finally:
        ops.discard_queues()


# ================================================================================================== the arena, end to end
class _Bias(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.b = torch.nn.Parameter(torch.randn(n))


def _toy():
    torch.manual_seed(3)
    return torch.nn.ModuleDict({
        "wide": torch.nn.Linear(64, 640, bias=False), "bias": _Bias(29), "odd": torch.nn.Linear(241, 17, bias=False),     # [17, 241]: 4097 elements
        "sq": torch.nn.Linear(256, 256, bias=False), "conv": torch.nn.Conv1d(128, 256, 1, bias=False)}).to(DEV)


def _arena_invariants(arena, what):
    """every bf16 view 16-byte aligned; transposed copies inside flat_params16_t and disjoint; shadows equal to their parameter"""
    base, end = arena.flat_params16_t.data_ptr(), arena.flat_params16_t.data_ptr() + arena.flat_params16_t.numel() * 2
    spans, bad = [], []
    for p in arena.params_ordered:
        if p._bf16.data_ptr() % 16:
            bad.append(f"_bf16 of {tuple(p.shape)} at byte offset {p._bf16.data_ptr() - arena.flat_params16.data_ptr()}")
        if p._bf16_t is not None:
            lo = p._bf16_t.data_ptr()
            if lo % 16:
                bad.append(f"_bf16_t of {tuple(p.shape)} at byte offset {lo - base} of flat_params16_t")
            assert base <= lo and lo + p.numel() * 2 <= end, what
            spans.append((lo, lo + p.numel() * 2))
    assert not bad, f"{what}: bf16 views that are not 16-byte aligned (tsasr_gemm_bf16 requires it): {bad}"
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), f"{what}: transposed copies overlap"
    assert len(spans) == 4


def _arena_shadows(arena, what):
    torch.cuda.synchronize()
    for p in arena.params_ordered:
        assert same_bits(p._bf16, p.data.to(BF16)), f"{what}: _bf16 of {tuple(p.shape)} is not bf16(p)"
        assert p._bf16_ver == p._version
        if p._bf16_t is not None:
            assert same_bits(p._bf16_t, p._bf16.reshape(p.shape[0], p.shape[1]).t()), f"{what}: _bf16_t of {tuple(p.shape)} is not the transpose"
        else:
            assert p.numel() == 29
    pad = torch.ones(arena.numel, dtype=torch.bool, device=DEV)
    for p in arena.params_ordered:
        o = arena.offset[id(p)]
        assert o % R.PAD == 0
        pad[o:o + p.numel()] = False
    return pad


def test_arena_alignment_invariant():
    """On construction: every p._bf16 / p._bf16_t starts on a 16-byte boundary (pointer arithmetic only). With transposed copies packed back
    to back, the 4097 elements of the [17, 241] matrix put every later copy at an odd element offset."""
    dp = importlib.import_module("ts-asr_amd.dp")
    arena = dp.GradArena(_toy())
    _arena_invariants(arena, "construction")
    arena.refresh_shadow()
    _arena_invariants(arena, "refresh_shadow")


def test_arena_end_to_end(ops, C):
    dp, optim = importlib.import_module("ts-asr_amd.dp"), importlib.import_module("ts-asr_amd.optim")
    mods = _toy()
    arena = dp.GradArena(mods)
    _arena_invariants(arena, "construction")
    pad = _arena_shadows(arena, "construction")
    opt = optim.FusedClipAdamW(arena, lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01, max_grad_norm=5.0)
    n = arena.numel
    rng = np.random.default_rng(1)
    for t in (1, 2, 3):
        g = torch.from_numpy((rng.standard_normal(n) * 2).astype(np.float32)).to(DEV)
        g[pad] = 0.0
        arena.grads.copy_(g)
        opt.param_groups[0]["lr"] = R.STEP_LR[t - 1]
        prev = {"p": arena.flat_params.cpu().double().numpy(), "m": opt.exp_avg.cpu().double().numpy(), "v": opt.exp_avg_sq.cpu().double().numpy()}
        opt.step()
        torch.cuda.synchronize()
        ref = R.adamw_step64(prev["p"], g.cpu().numpy(), prev["m"], prev["v"], R.hyper3(R.STEP_LR[t - 1], 0.9, 0.98, t), max_norm=5.0, **R.ADAM)
        got = {"p": arena.flat_params.cpu().numpy(), "m": opt.exp_avg.cpu().numpy(), "v": opt.exp_avg_sq.cpu().numpy(), "norm": float(opt.last_grad_norm)}
        hold(got, ref, prev, n, f"arena t={t}")
        for name, buf in (("flat_params", arena.flat_params), ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
            assert not bool(buf[pad].any()), f"t = {t}: pad words of {name} are no longer zero"
        assert same_bits(arena.grads, g)
        _arena_shadows(arena, f"step {t}")
    # deferred small gradients: one tsasr_accumulate_many at the end of backward
    arena.grads.copy_(torch.arange(n, device=DEV) % 7)
    g0 = arena.grads.clone()
    bias, add = mods["bias"].b, torch.randn(29, device=DEV)
    arena.begin_backward(False)
    try:
        assert arena.defer_add(bias, add)
        arena.finish_backward()
    finally:
        arena.abort_backward()
        ops.discard_queues()
    torch.cuda.synchronize()
    o = arena.offset[id(bias)]
    g0[o:o + 29] += add
    assert same_bits(arena.grads, g0)
    # dx = dy . W through the arena's transposed copy of the 256 x 256 weight that sits BEHIND the odd matrix
    w = mods["sq"].weight
    assert ops._bf16_weight_t(w) is w._bf16_t and w._bf16_t.data_ptr() > mods["odd"].weight._bf16_t.data_ptr()
    dy = torch.randn(72, 256, generator=torch.Generator().manual_seed(4)).to(BF16).to(DEV)
    dx = ops._dgrad(dy, w, w._bf16, 72, 256, 256)
    torch.cuda.synchronize()
    a, b = dy.cpu().double().numpy(), w._bf16.cpu().double().numpy()
    assert G.bf16_ok(dx.cpu(), a @ b, np.abs(a) @ np.abs(b), R.cdiv(256, 16) + 2), "dgrad through the arena's transposed copy"
    # forced re-layout: parameters, both moments and both shadows follow their parameter
    before = {id(p): (p.data.clone(), opt.exp_avg[arena.offset[id(p)]:arena.offset[id(p)] + p.numel()].clone(),
                      opt.exp_avg_sq[arena.offset[id(p)]:arena.offset[id(p)] + p.numel()].clone()) for p in arena.params_ordered}
    order0 = list(arena.params_ordered)
    arena._order_seen, arena._reorder_pending = list(reversed(order0)), True
    arena.zero_()
    torch.cuda.synchronize()
    assert arena.params_ordered == list(reversed(order0)) and not bool(arena.grads.any())
    _arena_invariants(arena, "re-layout")
    pad2 = _arena_shadows(arena, "re-layout")
    for p in arena.params_ordered:
        o, k = arena.offset[id(p)], p.numel()
        pv, mv, vv = before[id(p)]
        assert same_bits(p.data, pv) and same_bits(opt.exp_avg[o:o + k], mv.reshape(-1)) and same_bits(opt.exp_avg_sq[o:o + k], vv.reshape(-1))
        assert p.data.data_ptr() == arena.flat_params.data_ptr() + 4 * o and p.grad.data_ptr() == arena.grads.data_ptr() + 4 * o
    for buf in (arena.flat_params, opt.exp_avg, opt.exp_avg_sq):
        assert not bool(buf[pad2].any())
    for h in arena._hooks:
        h.remove()
