"""tests/helpers/joint_ref.py without a GPU: the plain form is the oracle's joint (and autograd through it), every planted fault of the fp32
restatement is rejected by the case matrix at the tolerances tests/test_joint_paths_gpu.py uses, and the stored tolerance constants are the
restatement's own errors."""
import numpy as np
import pytest
import torch

from oracle import tsasr_ref as R
from tests.helpers import joint_ref as JR

FWD = {c[0]: c for c in JR.forward_cases()}
BWD = {c[0]: c for c in JR.backward_cases()}


@pytest.mark.parametrize("B,T,U1,J,V", [(2, 5, 7, 48, 29), (1, 1, 1, 16, 1), (3, 4, 33, 32, 32)])
def test_plain_is_the_oracle(B, T, U1, J, V):
    """plain == oracle/tsasr_ref.joint_logits in float64, and its analytic backward == autograd through it, at 1e-12."""
    assert R.LRELU_SLOPE == 0.01
    enc, dec, W, bias = JR.make_inputs(f"o{B}{T}{U1}", JR.F32, B, T, U1, J, V)
    dl = np.random.default_rng(T).standard_normal((B, T, U1, V)).astype(np.float32)
    t = [torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (enc, dec, W, bias)]
    lo = R.joint_logits(t[0], t[1], {"w.weight": t[2], "w.bias": t[3]}, "")
    got, _ = JR.forward("generic", "plain", enc, dec, W, bias, 0.01, V, V)
    np.testing.assert_allclose(got, lo.detach().numpy(), rtol=0, atol=1e-12)
    (lo * torch.from_numpy(dl.astype(np.float64))).sum().backward()
    out, _, _ = JR.backward("bwd32", "plain", dl, enc, dec, W, 0.01, V)
    for k, g in zip(("denc", "ddec", "dW", "dbias"), t):
        np.testing.assert_allclose(out[k], g.grad.numpy(), rtol=0, atol=1e-12 * max(1.0, float(g.grad.abs().max())), err_msg=k)


def test_tile_tree_rows_cover_a_tile_once():
    assert sorted(JR._TREE.reshape(-1)) == list(range(32)) and sorted(JR._ROWS.reshape(-1)) == list(range(32))


def test_launcher_mirror_reaches_every_path():
    """The tables reach every branch of the launchers, by the mirror of the launchers at 256 compute units (the GPU test repeats this with the
    device's own count and fails if a path is missing)."""
    f = [JR.fwd_path(c[1], c[2], c[3], c[4], c[5], c[8]) for c in FWD.values()]
    assert {p[0] for p in f} == {"joint_fwd_kernel<float>", "joint_fwd_kernel<bf16>", "regw<40,true>", "regw<40,false>"}
    assert {p[1] for p in f} >= {1, 2, 4, 8}
    assert any(p[2] > 65536 for p in f if p[0] == "joint_fwd_kernel<float>") and any(p[2] > 65536 for p in f if p[0] == "joint_fwd_kernel<bf16>")
    b = [JR.bwd_path(c[1], c[2], c[3], c[4]) for c in BWD.values()]
    assert {p[0] for p in b} == {1, 2, 3, 4} and {p[1] for p in b} == {1, 2} and any(p[2] > 0 for p in b if p[1] == 2)
    assert {c[6] == 32 for c in BWD.values()} == {True, False}


def _fwd_fraction(case, fault=None):
    name, io, B, T, U1, J, V, ldl, slope, flavor = case
    enc, dec, W, bias = JR.make_inputs("f." + name, io, B, T, U1, J, V, flavor)
    path = JR.forward_kernel_path(case)
    split = JR.fwd_path(io, B, T, U1, J, slope)[1]
    r, S = JR.forward(path, "rounded", enc, dec, W, bias, slope, V, ldl)
    f, _ = JR.forward(path, "f32", enc, dec, W, bias, slope, V, ldl, split, fault)
    return JR.fraction(f, r, JR.tolerance(r, S, JR.TOL["fwd/" + name]["logits"]))


def _bwd_fractions(case, path, fault=None):
    name, B, T, U1, J, V, ldl, slope, tlen, ulen, flavor, scale = case
    io = JR.F32 if path == "bwd32" else JR.BF16
    enc, dec, W, dl = JR.backward_inputs(case, io)
    r, S, flip = JR.backward(path, "rounded", dl, enc, dec, W, slope, V, tlen, ulen)
    f, _, _ = JR.backward(path, "f32", dl, enc, dec, W, slope, V, tlen, ulen, JR.bwd_path(B, T, U1, J)[0], fault)
    tol = JR.TOL[f"bwd/{name}/{'f32' if io == JR.F32 else 'bf16'}"]
    out = {}
    for k in r:
        store = io == JR.BF16 and k in ("denc", "ddec")          # the kernel leaves these as bf16: the GPU test's allowance, and the store itself
        with np.errstate(invalid="ignore"):
            got = JR.bf16(f[k]) if store else f[k]
        out[k] = JR.fraction(got, r[k], JR.tolerance(r[k], S[k], tol[k], flip.get(k), store))
    return out


def test_restatement_passes_its_own_matrix():
    for case in FWD.values():
        assert _fwd_fraction(case) <= 1.0 / JR.MARGIN + 1e-3, case[0]
    for case in BWD.values():
        for path in ("bwd32", "bwd16"):
            fr = _bwd_fractions(case, path)
            for k, v in fr.items():      # (a bf16 store may use all of its own half ulp)
                assert v <= (1.0 if path == "bwd16" and k in ("denc", "ddec") else 1.0 / JR.MARGIN + 1e-3), (case[0], path, fr)


@pytest.mark.parametrize("fault", sorted(JR.FAULTS))
def test_planted_fault_is_rejected(fault):
    direction, path, switch, ids = JR.FAULTS[fault]
    for cid in ids:
        if direction == "fwd":
            frac = _fwd_fraction(FWD[cid], switch)
        else:
            frac = max(_bwd_fractions(BWD[cid], path, switch).values())
        print(f"{fault} on {cid}: {frac:.3g} of the tolerance")
        assert frac > 1.0, f"{fault}: case {cid} accepts it ({frac:.3g} of its tolerance)"


def test_at_least_ten_faults_are_planted():
    assert len({v[2] for v in JR.FAULTS.values()}) >= 10


def test_stored_tolerances_are_the_restatement_s_errors():
    """TOL is what compute_tol() measures (python -m tests.helpers.joint_ref rewrites it). The fp32 matrix products of the restatement
    may be summed in another order by another BLAS build, so a constant may move by a small factor; beyond a factor of 2 - half of the
    margin - the table is stale. Constants under the 2^-23 floor all act as the floor."""
    now = JR.compute_tol()
    assert sorted(now) == sorted(JR.TOL)
    for key, d in now.items():
        for k, v in d.items():
            a, b = max(v, JR.FLOOR), max(JR.TOL[key][k], JR.FLOOR)
            assert a <= 2 * b and b <= 2 * a, (key, k, v, JR.TOL[key][k])


def test_rounded_forms_stay_inside_the_whole_tensor_figures():
    """The figures tests/test_rnnt_gpu.py holds the kernels to against the un-rounded oracle (forward atol 6e-2 / rtol 2e-2; gradients 6e-3
    in fp32 storage and 1.2e-2 in bf16, relative L2) already hold for the rounded forms at gradient scale 1, bf16 store included."""
    for case in FWD.values():
        name, io, B, T, U1, J, V, ldl, slope, flavor = case
        if flavor == "big":
            continue
        enc, dec, W, bias = JR.make_inputs("f." + name, io, B, T, U1, J, V, flavor)
        r, _ = JR.forward(JR.forward_kernel_path(case), "rounded", enc, dec, W, bias, slope, V, ldl)
        p, _ = JR.forward("generic", "plain", enc, dec, W, bias, slope, V, ldl)
        assert np.all(np.abs(r - p) <= 6e-2 + 2e-2 * np.abs(p)), name
    for case in BWD.values():
        name, B, T, U1, J, V, ldl, slope, tlen, ulen, flavor, scale = case
        if scale != 1.0:
            continue
        for io, path, lim in ((JR.F32, "bwd32", 6e-3), (JR.BF16, "bwd16", 1.2e-2)):
            enc, dec, W, dl = JR.backward_inputs(case, io)
            r, _, _ = JR.backward(path, "rounded", dl, enc, dec, W, slope, V, tlen, ulen)
            p, _, _ = JR.backward(path, "plain", dl, enc, dec, W, slope, V, tlen, ulen)
            for k in ("denc", "ddec", "dW"):
                got = JR.bf16(r[k].astype(np.float32)) if io == JR.BF16 and k != "dW" else r[k]
                rel = np.linalg.norm(got - p[k]) / np.linalg.norm(p[k])
                assert rel < lim, (name, path, k, rel)
