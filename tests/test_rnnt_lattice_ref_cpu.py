"""tests/helpers/rnnt_lattice_ref.py checked on the CPU: the fp32 restatement is tied to float64 in every regime, the closed form of the
flat lattice, the frame-boundary invariant and brute-force path sums hold, the Python mirror of rnnt_plan enumerates the 33
instantiations of launch_alphabeta and the GPU case table covers them, and planted defects are rejected by the matrix - with a record
of which of them the tolerances of tests/test_rnnt_gpu.py would have let through."""
import numpy as np
import pytest

from tests.helpers import rnnt_lattice_ref as LR

SHAPE = dict(B=2, T=19, U1=27, V=4, tlen=(19, 12), ulen=(26, 9))


def small(regime, **kw):
    s = dict(SHAPE, **kw)
    return LR.case(regime, s["B"], s["T"], s["U1"], s["V"], s["tlen"], s["ulen"], seed=3, allowed=(1, 2))


@pytest.mark.parametrize("regime", LR.REGIMES)
def test_restatement_is_tied_to_float64(regime):
    """Bounds that do not come from the restatement itself: rnnt_lp's planes within 4 ulp of their magnitude (V + 2 roundings), alpha /
    beta within 3 ulp of the plane's largest magnitude PER STEP of the perimeter, in the plain and in the perturbed run; and the
    restatement passes the matrix it defines at 1 / FACTOR, and with another seed of the perturbation."""
    inputs, ref, tol = small(regime)
    for perturb in (None, 5):
        out = LR.planes32(*inputs[:6], gscale=inputs[6], perturb=perturb)
        m = LR.metrics(out, ref)
        for b in range(SHAPE["B"]):
            per = int(ref["Tb"][b] + ref["Ub"][b])
            big = np.abs(ref["lse"][b][ref["live"][b]]).max()        # a log-probability x - lse carries the rounding of lse, however small it is
            for name in ("lse", "lpb", "lpe_out", "lpe_in"):
                err, _, mag = m[name]
                assert err[b].max() <= 4 * LR._ulp(max(mag[b], big)), (name, b)
            for name in ("alpha", "beta"):
                err, _, mag = m[name]
                assert err[b].max() <= 3 * per * LR._ulp(max(mag[b], big)), (name, b, err[b].max())
            assert m["cost"][0][b] <= 3 * per * LR._ulp(max(ref["costs"][b], big))
        fails, frac = LR.judge(out, ref, tol)
        assert not fails and max(frac.values()) <= 1.0, (fails, frac)      # (another seed of the perturbation than the tolerance's own)
    for perturb in (None, 20260):                                         # the two runs the tolerance is made of: 1 / FACTOR at the most
        fails, frac = LR.judge(LR.planes32(*inputs[:6], gscale=inputs[6], perturb=perturb), ref, tol)
        assert not fails and max(frac.values()) <= 1.0 / LR.FACTOR + 1e-12, (fails, frac)
    # the oracle's own float32 gradient is the float64 formula rounded once (relative to the larger of its two terms)
    assert np.all(np.abs(ref["oracle_grads"] * ref["gs"][:, None, None, None] - ref["grads"]) <= 2e-7 * ref["gscale_mag"] + 1e-37)


def test_flat_lattice_has_a_closed_form():
    inputs, ref, tol = small("flat")
    out = LR.planes32(*inputs[:6], gscale=inputs[6])
    for b in range(SHAPE["B"]):
        want = LR.flat_cost(int(ref["Tb"][b]), int(ref["Ub"][b]), SHAPE["V"])
        assert abs(ref["costs"][b] - want) <= 1e-12 * want
        assert abs(out["costs"][b] - want) <= tol["cost"][b]


@pytest.mark.parametrize("regime", LR.REGIMES)
def test_frame_boundary_invariant(regime):
    """logsumexp_u(alpha(t, u) + lpb(t, u) + beta(t + 1, u)) = logP for every t < Tb - 1, on the float64 planes to 1e-9."""
    inputs, ref, tol = small(regime)
    as_out = dict(lse=ref["lse"], lpb=ref["lpb"], lpe_out=ref["lpe"], lpe_in=LR._shift(ref["lpe"], 2, -1, 0.0), alpha=ref["alpha"], beta=ref["beta"],
                  logp=ref["logp"], costs=ref["costs"], dlogits=ref["grads"])
    m = LR.metrics(as_out, ref)
    assert m["invariant"][0].max() <= 1e-9 * max(1.0, np.abs(ref["logp"]).max())
    for name in ("alpha_local", "beta_local", "grad_local", "grad", "logp_local"):
        assert m[name][0].max() <= 1e-9 * max(1.0, np.abs(ref["logp"]).max()), name


@pytest.mark.parametrize("T,U", [(1, 0), (1, 2), (4, 0), (3, 2), (4, 3), (2, 3)])
def test_brute_force_on_tiny_lattices(T, U):
    rng = np.random.default_rng(T * 10 + U)
    V, U1 = 4, U + 1
    lg = (2 * rng.standard_normal((1, T, U1, V))).astype(np.float32)
    tg = rng.integers(1, V, size=(1, max(U, 1))).astype(np.int32)
    want = LR.brute_force_cost(lg[0], tg[0], T, U, 0)
    ref = LR.planes64(lg, tg, [T], [U], 0, V)
    assert abs(ref["costs"][0] - want) <= 1e-12 * max(1.0, abs(want))
    out = LR.planes32(lg, tg, [T], [U], 0, V)
    assert abs(out["costs"][0] - want) <= 4 * (T + U + 1) * LR._ulp(want)


def test_plan_mirror_enumerates_the_dispatch_table():
    """Every (U1, plan) the library can be asked for lands on one of the 33 instantiations of launch_alphabeta, all 33 are reached, and the
    GPU case tables cover every one of them (ramp-only) and every form (steady state)."""
    assert len(LR.ALL_INSTANTIATIONS) == 33
    reached = set()
    for U1 in list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1000, 1024, 1025, 1500, 2047, 2048]:
        for B in (1, 2, 3, 8, 40):
            for skew in (-1, 0, 1, 2):
                for waves in (-1, 1, 2, 3, 4, 8, 16):
                    for mc in (-1, 0, 1, 2, 4):
                        kt, nw, nc, sk = LR.instantiation(B, U1, (skew, waves, mc))
                        assert kt * nw * nc == LR.lattice_K(U1) and (nc == 1 or (nw == 1 and sk == 1))
                        reached.add(LR.inst_key((kt, nw, nc, sk)))
    assert reached == set(LR.ALL_INSTANTIATIONS)
    ramp = LR.ramp_cases()
    assert {LR.inst_key(c[3]) for c in ramp} == set(LR.ALL_INSTANTIATIONS)
    for B, U1, plan, inst in ramp:                                   # both ends of the K range of every instantiation; resident split lattices
        assert inst[2] == 1 or 2 * B * inst[2] <= 64
        ul = LR.ramp_ulens(U1, inst, B)
        assert len(ul) == B and all(0 <= v <= U1 - 1 for v in ul)
    by_inst = {}
    for B, U1, plan, inst in ramp:
        by_inst.setdefault(LR.inst_key(inst), set()).add(U1)
    assert all(len(v) >= 2 for v in by_inst.values()), by_inst
    steady = {LR.inst_key(LR.instantiation(B, U1, plan)) for _, B, _, U1, _, plan in LR.steady_cases()}
    assert {(k[1], k[3]) for k in steady if not k[2]} == {(nw, s) for nw in (1, 2, 4, 8, 16) for s in (0, 1)}
    assert {k[0] for k in steady if k[2]} == {1, 2, 4}
    # the default plans of the benchmark's lattice and of a single long utterance
    assert LR.instantiation(32, 121) == (2, 1, 1, 0) and LR.instantiation(1, 1921) == (2, 1, 16, 1) and LR.instantiation(8, 401) == (2, 4, 1, 1)


def test_clamp_at_minus_20_is_not_a_defect():
    """The issue lists 'the clamp at -20' among the defects to plant. It cannot be one: exp(-20) = 2.1e-9 < 2^-24, so 1 + e rounds to 1 for
    every d <= -16.7 and logaddexp_f returns m whatever the clamp is below that. Shown here bit for bit in every regime; the nearest
    clamp that IS a defect (-5, planted below) changes values."""
    for regime in LR.REGIMES:
        inputs, ref, tol = small(regime)
        a = LR.planes32(*inputs[:6], gscale=inputs[6])
        b = LR.planes32(*inputs[:6], gscale=inputs[6], clamp=-20.0)
        for k in a:
            assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), (regime, k)


def _planted(regime):
    """(name, outputs with the defect) on the K = 8 lattice: columns 128 .. are the second wave of the (2, 4) instantiation, the second
    column block of the split (2, 1) one."""
    inputs, ref, tol = LR.case(regime, 2, 150, 300, 5, (150, 90), (299, 140), seed=9, allowed=(1, 2, 3))
    run = lambda **kw: LR.planes32(*inputs[:6], gscale=inputs[6], **kw)  # noqa: E731
    good = run()
    assert not LR.judge(good, ref, tol)[0]
    # a label entry whose emit occupancy is small in absolute terms: the gradient entry that forgets it is wrong by its own size
    with np.errstate(all="ignore"):
        occ = np.exp(ref["alpha"] + ref["lpe"] + LR._shift(ref["beta"], 2, 1, -np.inf) - ref["logp"][:, None, None])
    occ = np.where(ref["live"] & (np.arange(300)[None, None, :] < ref["Ub"][:, None, None]) & (occ < 1e-5), occ, 0.0)
    b0, t0, u0 = (int(v) for v in np.unravel_index(np.argmax(occ), occ.shape))        # the largest one below 1e-5
    assert occ[b0, t0, u0] > 1e-12
    defects = [
        ("alpha corner cell + 1e-3", dict(kind="alpha_cell", b=0, t=3, u=290, by=1e-3)),
        ("hand-off into column 128 = -inf", dict(kind="left_inf", b=0, t=12, u=128)),
        ("hand-off into column 128 one step old", dict(kind="left_stale", b=0, t=12, u=128)),
        ("lpe_in shifted by one column", dict(kind="lpe_in_shift")),
        ("blank from the neighbouring lane", dict(kind="blank_neighbour")),
        ("beta(Tb-1, Ub) seeded with 0", dict(kind="beta_seed_zero")),
        ("steady step reuses frame t-1 operands", dict(kind="stale_operands", b=0, t=80, u=77)),
        ("label entry misses -gemit", dict(kind="miss_gemit", b=b0, t=t0, u=u0)),
    ]
    rows = [(name, run(defect=d)) for name, d in defects]
    rows.append(("clamp at -5", run(clamp=-5.0)))
    return ref, tol, rows


def test_planted_defects_are_rejected():
    """Every planted defect misses the matrix; the table records which of them the old tolerances (costs rtol 2e-5, gradient atol 3e-5 /
    rtol max(1e-3, 5e-5 (T + U1))) accept. The corner cell and at least one defect of the peaked regime must be among those: that is
    the gap this suite closes."""
    assert set(LR.DEFECTS) == {"alpha_cell", "left_inf", "left_stale", "lpe_in_shift", "blank_neighbour", "beta_seed_zero", "stale_operands", "miss_gemit"}
    table, old_ok = [], {}
    for regime in ("normal", "peaked"):
        ref, tol, rows = _planted(regime)
        for name, out in rows:
            # named as the four-wave form sees the cell; the one-wave form for the stale step (150 frames hold no steady state of 256 threads)
            fails, frac = LR.judge(out, ref, tol, (8, 1, 1, 1) if "steady" in name else (2, 4, 1, 1))
            assert "steady" not in name or "(steady)" in fails[0]
            old = LR.old_tolerances_accept(out, ref)
            table.append((regime, name, bool(fails), old, fails[0] if fails else "-"))
            old_ok[(regime, name)] = old
    print("\nregime  | defect                                   | new matrix | old tolerances | first failure")
    for regime, name, rej, old, first in table:
        print(f"{regime:7s} | {name:40s} | {'REJECTS' if rej else 'accepts':10s} | {'accept' if old else 'reject':14s} | {first[:150]}")
    assert all(rej for _, _, rej, _, _ in table), [r[:3] for r in table if not r[2]]
    assert old_ok[("normal", "alpha corner cell + 1e-3")]
    assert any(v for (regime, _), v in old_ok.items() if regime == "peaked")
    assert sum(old_ok.values()) >= 2


def test_failure_message_names_the_thread_and_the_step():
    msg = LR.where((2, 4, 1, 1), 300, 12, 128, "alpha")
    assert msg == "thread g=64 wave=1 block=0 step s=76 (ramp)"
    assert "steady" in LR.where((2, 4, 1, 1), 300, 200, 128, "alpha") and "block=1" in LR.where((2, 1, 4, 1), 300, 12, 128, "beta")
