"""tests/helpers/gradtail_ref.py on the CPU: adamw_step64 against torch.optim.AdamW + clip_grad_norm_ in float64, the fp32 restatement of the
kernel against it (its measured deltas ARE the tolerances of the GPU file), the mirrors of the host-side plans against hand-computed values and
against the library's own numbers where the C-ABI exposes them, and the case matrix reaching every path it promises. No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_ref as G  # noqa: E402
import gradtail_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------------ the model is the operation
@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_adamw_step64_is_clip_grad_norm_plus_torch_adamw(regime):
    n, max_norm = 1237, R.REGIMES[regime]
    p0, gs = R.gaussian_case(n, 11, regime)
    if regime == "unclipped":
        max_norm = 1e4
    pt = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.AdamW([pt], lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
    st = {"p": p0.astype(np.float64), "m": np.zeros(n), "v": np.zeros(n)}
    for t in range(1, 4):
        lr = R.STEP_LR[t - 1]
        opt.param_groups[0]["lr"] = lr
        pt.grad = torch.from_numpy(gs[t - 1]).double()
        total = float(pt.grad.norm())
        if max_norm > 0:
            total = float(torch.nn.utils.clip_grad_norm_([pt], max_norm))
        opt.step()
        hyper = np.array([lr, 1 - 0.9 ** t, 1 - 0.98 ** t])
        st = R.adamw_step64(st["p"], gs[t - 1], st["m"], st["v"], hyper, 0.9, 0.98, 1e-8, 0.01, max_norm, round_scalars=False)
        assert st["norm"] == pytest.approx(total, rel=1e-14)
        assert (st["clip"] < 1) == (regime == "clipped"), (regime, st["clip"])
        np.testing.assert_allclose(st["p"], pt.detach().numpy(), rtol=1e-13, atol=1e-15)
        # (torch forms m with lerp: a few float64 roundings of the largest term, |g| <= 50, where the two terms cancel)
        np.testing.assert_allclose(st["m"], opt.state[pt]["exp_avg"].numpy(), rtol=1e-13, atol=50 * 2.0 ** -50)
        np.testing.assert_allclose(st["v"], opt.state[pt]["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-300)
    if regime == "zero_grad":
        assert not st["m"].any() and not st["v"].any() and np.isfinite(st["p"]).all()
        np.testing.assert_allclose(st["p"], p0 * np.prod([1 - lr * 0.01 for lr in R.STEP_LR]), rtol=1e-14)


def test_adamw_step64_nonfinite_norms():
    p, g = np.ones(8), np.ones(8)
    g[3] = np.inf
    h = R.hyper3(1e-3, 0.9, 0.98, 1)
    s = R.adamw_step64(p, g, p * 0, p * 0, h, 0.9, 0.98, 1e-8, 0.01, 5.0, skip=True)
    assert s["skipped"] == 1 and (s["p"] == p).all() and not s["m"].any()
    s = R.adamw_step64(p, g, p * 0, p * 0, h, 0.9, 0.98, 1e-8, 0.01, 5.0)
    assert s["clip"] == 0.0 and np.isnan(s["p"][3]) and s["skipped"] == 0       # Inf * 0
    g[3] = np.nan
    assert np.isnan(R.adamw_step64(p, g, p * 0, p * 0, h, 0.9, 0.98, 1e-8, 0.01, 5.0)["clip"])
    assert R.clip_coef64(np.inf, 0.0) == 1.0 and R.clip_coef64(3.0, -1.0) == 1.0
    # float64 has room above fp32: a norm of 3.2e38 is an ordinary, finite norm for the reference
    g = np.zeros(8)
    g[0] = R.r32(3.2e38)
    s = R.adamw_step64(p, g, p * 0, p * 0, h, 0.9, 0.98, 1e-8, 0.01, 5.0, skip=True)
    assert s["skipped"] == 0 and s["norm"] == R.r32(3.2e38) and 0 < s["clip"] < 1e-37


# ------------------------------------------------------------------------------------------------------ the tolerances
def _measure(n=200_003):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}
    for regime, max_norm in R.REGIMES.items():
        p0, gs = R.gaussian_case(n, 5, regime)
        s32 = {"p": p0, "m": np.zeros(n, np.float32), "v": np.zeros(n, np.float32)}
        for t in range(1, 4):
            h = R.hyper3(R.STEP_LR[t - 1], 0.9, 0.98, t)
            prev = {k: s32[k].astype(np.float64) for k in ("p", "m", "v")}
            ref = R.adamw_step64(prev["p"], gs[t - 1], prev["m"], prev["v"], h, max_norm=max_norm, **R.ADAM)      # from the emulation's own state
            s32 = R.adamw_step32(s32["p"], gs[t - 1], s32["m"], s32["v"], h, max_norm=max_norm, **R.ADAM)
            e = R.update_errors(s32, ref, prev)
            assert e["norm"] * R.U * ref["norm"] <= R.norm_bound(n, ref["norm"] ** 2), (regime, t, e)
            worst = {k: max(worst[k], e[k]) for k in worst}
    return worst


def test_fp32_emulation_sets_the_tolerances():
    """The fp32 restatement against adamw_step64, each step from the emulation's own previous state (so errors do not chain): the worst
    delta per output, in fp32 ulps of max(|result|, |largest term|), is what TOL records; the GPU gets 4 x that. Two sizes: m and v carry the
    clip coefficient's rounding, which is one number per gradient, not a maximum over elements."""
    w1, w2 = _measure(200_003), _measure(1_000_003)
    w = {k: max(w1[k], w2[k]) for k in w1}
    print("\nmeasured (fp32 ulps of max(|result|, |largest term|); norm in units of 2^-24 norm):", {k: round(v, 3) for k, v in w.items()})
    for k in ("p", "m", "v"):
        assert w[k] <= R.TOL["measured"][k], (k, w[k])
        assert w[k] >= 0.5 * R.TOL["measured"][k], f"TOL['measured'][{k!r}] = {R.TOL['measured'][k]} is not what this measures ({w[k]:.3f})"
        assert R.TOL["gpu"][k] == pytest.approx(4 * R.TOL["measured"][k])


def test_update_errors_sees_one_ulp():
    n = 1000
    p0, gs = R.gaussian_case(n, 2)
    h = R.hyper3(1e-3, 0.9, 0.98, 1)
    prev = {"p": p0.astype(np.float64), "m": np.zeros(n), "v": np.zeros(n)}
    ref = R.adamw_step64(p0, gs[0], prev["m"], prev["v"], h, max_norm=5.0, **R.ADAM)
    got = {k: np.array(ref[k], dtype=np.float32) for k in ("p", "m", "v")}
    got["norm"] = ref["norm"]
    assert max(R.update_errors(got, ref, prev)[k] for k in ("p", "m", "v")) <= 0.5
    for k in ("p", "m", "v"):       # a planted error of 64 ulp in ONE element is far outside 4 x measured
        bad = dict(got)
        bad[k] = got[k].copy()
        for _ in range(64):
            bad[k][n // 2] = np.nextafter(bad[k][n // 2], np.float32(np.inf))
        assert R.update_errors(bad, ref, prev)[k] > R.TOL["gpu"][k]


def test_norm_bound_is_derived_not_measured():
    for n in R.OPT_SIZES:
        d = R.norm_depth(n)
        assert d == 27 + R.cdiv(R.sumsq_per(n), 1024)
        assert R.norm_bound(n, 4.0) == pytest.approx((0.505 * d + 1) * 2.0 ** -24 * 2.0)
    assert R.norm_depth(8_392_709) == 36


# ------------------------------------------------------------------------------------------------------ mirrors of the host plans
def test_sumsq_partition():
    assert [R.sumsq_per(n) for n in (1, 4099, 1_000_003, 3_149_824, 5_000_003, 8_392_709)] == [4, 8, 980, 3076, 4884, 8200]
    for n in R.OPT_SIZES:
        parts = R.sumsq_parts(n)
        assert len(parts) == 1024 and parts[0][0] == 0 and max(hi for _, hi in parts) == n
        assert all(a[1] == b[0] or b[0] == n for a, b in zip(parts, parts[1:]))         # contiguous, then empty
        assert all(lo % 4 == 0 or lo == n for lo, _ in parts)
    assert R.sumsq_paths(1_000_003) == {"single", "tail", "empty"}
    assert "unrolled1" not in R.sumsq_paths(1_000_003)                                    # what the old single-size test never ran
    assert R.sumsq_paths(3_149_824) == {"unrolled1", "single"}
    assert R.sumsq_paths(5_000_003) == {"unrolled1", "unrolled_all", "single", "tail"}
    assert {"unrolled2", "tail"} <= R.sumsq_paths(8_392_709)
    assert R.sumsq_paths(4099) >= {"empty", "tail"} and R.sumsq_paths(1) == {"tail", "empty"}
    lo, hi = R.sumsq_parts(5_000_003)[-1]
    assert (hi - lo) % 4 == 3
    assert [R.opt_wgs(n) for n in (1, 3, 4, 1024, 1025, 2_097_152, 2_097_153, 8_392_709)] == [1, 1, 1, 1, 2, 2048, 2048, 2048]
    assert "grid_stride" not in R.opt_paths(2_097_152) and "grid_stride" in R.opt_paths(5_000_003)


def test_exact_gradients_are_exact():
    for n in R.OPT_SIZES:
        g, ss = R.exact_gradient(n, n)
        assert set(np.unique(g)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and ss == int((g.astype(np.float64) ** 2).sum()) < (1 << 24)
        assert float(R.sumsq32(g)) == float(ss)                     # the fp32 restatement is exact there too
        pos = R.single_positions(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and all(0 <= q < n for q in pos)


def test_xcd_remap_is_a_permutation():
    for total in range(1, 41):
        ids = [R.xcd_id(b, total) for b in range(total)]
        assert sorted(ids) == list(range(total)), total
    assert [R.xcd_id(b, 17) for b in range(9)] == [0, 3, 5, 7, 9, 11, 13, 15, 1]      # 17 & 7 = 1: XCD 0 owns three tiles, the rest two


def test_search64_finds_the_job():
    rng = np.random.default_rng(0)
    for njobs in (1, 2, 63, 64, 65, 200, 301, 4097):
        sizes = rng.integers(1, 5, size=njobs)
        tile0 = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
        total = int(sizes.sum())
        levels = set()
        for tid in sorted({0, 1, total - 1, total // 2, *rng.integers(0, total, size=50).tolist()}):
            j, lv = R.search64(tile0, tid)
            assert tile0[j] <= tid and (j + 1 == njobs or tile0[j + 1] > tid), (njobs, tid, j)
            levels.add(lv)
        assert max(levels) == (0 if njobs == 1 else 1 if njobs <= 64 else 2 if njobs <= 4096 else 3)


def test_wgrad_plan():
    jobs = [(8, 8, 5), (512, 512, 9), (264, 256, 9), (256, 264, 2), (136, 520, 9)]
    order, tile0, total = R.wgrad_plan(jobs)
    assert order == [1, 2, 4, 0, 3] and tile0 == [0, 4, 6, 9, 10] and total == 12          # K descending, queue order among equals
    assert [R.wgrad_ktiles(K) for K in (1, 32, 33, 128, 129, 200)] == [(1, 1), (1, 0), (2, 1), (4, 0), (5, 1), (7, 8)]
    capi = importlib.import_module("ts-asr_amd._capi")
    assert capi.lib().tsasr_wgrad_table_bytes(3) == 3 * 72          # WgradJob: 3 pointers, 3 strides, 6 ints
    for t in range(1, 18):
        assert R.wgrad_plan(R.tiles_jobs(t))[2] == t
    for count in R.WG_MANY:
        ks = [j[2] for j in R.many_jobs(count)]
        assert len(ks) == count + (count >= 2)


def test_transpose_predicate():
    jobs, tiles, total = R.transpose_jobs(list(R.TR_MATS))
    assert all(j[0] % 64 == 0 and j[1] % 64 == 0 for j in jobs)
    assert tiles == 1 + 4 * 32 + 32 * 4 + 2 * 4 + 1 * 10 + 1 * 4 + 1 * 64 + 4
    fast = {(j[2], j[3]): [R.transpose_fast(j, lt) for lt in range(R.cdiv(j[2], 64) * R.cdiv(j[3], 64))] for j in jobs}
    assert all(fast[(64, 64)]) and all(fast[(256, 2048)]) and all(fast[(2048, 256)]) and all(fast[(128, 128)])
    assert fast[(72, 200)] == [True, True, True, False, False, False, False, False]      # whole tiles of the first row band only
    assert not any(fast[(29, 640)]) and not any(fast[(17, 241)]) and not any(fast[(16, 4096)])
    packed, _, total1 = R.transpose_jobs([(17, 241), (128, 128)], pad=1)                  # the layout before the fix: 4097 elements, then the next copy
    assert packed[1][1] == 4097 and total1 == 4097 + 16384 and not any(R.transpose_fast(packed[1], lt) for lt in range(4))
    padded, _, total2 = R.transpose_jobs([(17, 241), (128, 128)])
    assert padded[1][1] == 4160 and total2 == 4160 + 16384 and all(R.transpose_fast(padded[1], lt) for lt in range(4))
    b = R.distinct_bits(65535)
    assert len(np.unique(b.numpy())) == 65535


def test_reduce_classification_against_the_library():
    assert R.reduce_wide(31, 4096) and not R.reduce_wide(32, 4096) and not R.reduce_wide(4, 4095)
    assert R.reduce_tiles(4, 4097) == 5 and R.reduce_tiles(40, 72) == 2 and R.reduce_tiles(4, 520) == 9
    lib = importlib.import_module("ts-asr_amd._capi").lib()
    assert lib.tsasr_reduce_table_bytes(2) == 2 * 48                   # ReduceJob: 2 pointers, a stride, 6 ints
    assert lib.tsasr_clip_adamw_workspace_bytes() == 2 * 4 * R.OPT_PARTS      # plain and 2^-128-scaled partial sums
    for M in (1, 64, 65, 200, 1100, 3000, 65536, 70000):
        for N in (8, 72):
            assert lib.tsasr_colsum_workspace_bytes(M, N) == R.cdiv(R.colsum_parts(M) * N * 4, 256) * 256, (M, N)
    for (M, N, K) in R.RD_GEMM + ((256, 256, 8000), (2048, 256, 4000), (64, 64, 383), (8, 8, 64)):
        s, nbytes = R.gemm_splits(M, N, K)
        assert lib.tsasr_gemm_bf16_workspace_bytes(M, N, K, 0) == nbytes, (M, N, K, s)
    for (M, N, K) in R.RD_GEMM:
        s, _ = R.gemm_splits(M, N, K)
        assert 1 < s < 32 and R.reduce_wide(s, M * N)
    # a split-K output is M x N with N % 4 == 0 (the launcher requires it), so no deferred GEMM has a width that is not a multiple of 4:
    # the ragged end of reduce_tile's wide branch is not reachable through the C-ABI
    assert all((M * N) % 4 == 0 for M, N, _ in R.RD_GEMM)


def test_accumulate_lengths():
    assert set(R.acc_lengths(70)) == set(R.ACC_LENS)
    assert R.acc_paths(0) == {"empty"} and R.acc_paths(256) == {"one_piece"} and R.acc_paths(4097) == {"many_wgs", "second_round", "ragged_piece"}


# ------------------------------------------------------------------------------------------------------ the matrix
def test_matrix_reaches_every_path():
    cs = R.matrix()
    keys = [c["key"] for c in cs]
    assert len(set(keys)) == len(keys)
    reached = set().union(*(c["paths"] for c in cs))
    missing = [p for p in R.REQUIRED_PATHS if p not in reached]
    assert not missing, missing
    many = {c["key"]: c for c in cs if c["fam"] == "wg_many"}
    assert many["wg_many200"]["paths"] >= {"wg:search_levels2", "wg:sort_reorders"} and "wg:search_levels1" in many["wg_many63"]["paths"]
    assert {c["tiles"] for c in cs if c["fam"] == "wg_tiles"} == set(range(1, 18))


def test_exact_wgrad_operands_stay_exact():
    """amplitude 3 operands, K <= 200, |dW0| <= 64: every partial sum is an integer below 2^24 (gemm_ref.assert_exact_regime)"""
    gen = torch.Generator().manual_seed(1)
    a, b = G.int_operand(200, 8, 3, gen), G.int_operand(200, 8, 3, gen)
    _, absprod = G.product(a, b, 1, 1)
    assert G.assert_exact_regime(absprod, c0=np.full((8, 8), 64.0), what="wgrad") <= 200 * 9 + 64
