"""Wide-vocabulary joint + head (csrc/joint_wide.hip through rnnt.fused_joint_logits, 32 < V <= 1024) against the float64 helper of
tests/helpers/joint_wide_ref.py and the reference-pin fixture: forward, the joint -> loss -> backward chain (the first V > 32 coverage of
rnnt_lp / rnnt_grad / rnnt_align too), zero gradients outside the lengths, bitwise reproducibility, independence of the length skip.

Tolerances are the project's own for the same rounding: forward atol 2e-3 / rtol 1e-3 against the identically rounded helper and atol 6e-2 /
rtol 2e-2 against un-rounded fp32 (tests/test_rnnt_gpu.py test_joint_forward: the inner dimension is J, not V); loss rel 1e-4 and gradient
relative L2 6e-3 (fp32 storage) / 1.2e-2 (bf16) (test_joint_loss_backward_chain). Measured values: profiles/wide_vocab_notes.md."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import rnnt_ref as RR
from oracle.golden_recipe import det_tensor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import align_ref as AR  # noqa: E402
import joint_wide_ref as JW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [
    # B, T, U1, J, V, tlen, ulen
    (1, 1, 1, 32, 33, [1], [0]),                          # one cell, one column past a tile
    (2, 7, 33, 64, 64, [7, 7], [32, 32]),                 # exactly two vocabulary tiles; u one past a tile
    (2, 19, 40, 64, 100, [19, 19], [39, 39]),             # ragged last tile
    (2, 9, 21, 160, 257, [9, 9], [20, 20]),               # odd V, padded stride
    (1, 5, 3, 640, 1024, [5], [2]),                       # the maximum V at the recipe's J
    (2, 70, 33, 640, 500, [70, 66], [32, 7]),             # the chain case
    (3, 6, 5, 64, 40, [6, 4, 1], [4, 2, 0]),              # T = 1 and an empty target
    # beyond the issue's table: the widest joint (the dh kernel splits J > 640 over two workgroups, the forward holds two frames per
    # workgroup) at the widest vocabulary (one staging thread per four columns) under ragged lengths, u one past a tile
    (2, 5, 34, 1024, 1024, [5, 3], [33, 6]),
]
IDS = [f"B{c[0]}-T{c[1]}-U{c[2]}-J{c[3]}-V{c[4]}" for c in CASES]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def rn():
    return importlib.import_module("ts-asr_amd.rnnt")


def bf(x):
    return x.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def inputs(i, dtype):
    B, T, U1, J, V, _, _ = CASES[i]
    enc = torch.from_numpy(det_tensor(f"jw.enc{i}", (B, T, J), 1.0))
    dec = torch.from_numpy(det_tensor(f"jw.dec{i}", (B, U1, J), 1.0))
    W = torch.from_numpy(det_tensor(f"jw.W{i}", (V, J), 1.0 / np.sqrt(J)))
    b = torch.from_numpy(det_tensor(f"jw.b{i}", (V,), 0.1))
    tg = torch.from_numpy(np.random.default_rng(i).integers(1, V, size=(B, max(U1 - 1, 1))).astype(np.int32))
    if dtype == torch.bfloat16:
        enc, dec = bf(enc), bf(dec)
    return enc, dec, W, b, tg


@functools.lru_cache(maxsize=None)
def reference(i, dtype):
    """float64 oracle of case i, computed once: rounded logits, loss, (denc, ddec, dW, dbias) of the mean cost."""
    B, T, U1, J, V, tlen, ulen = CASES[i]
    enc, dec, W, b, tg = inputs(i, dtype)
    logits = JW.forward(enc, dec, W, b)
    lg = logits.clone().requires_grad_()
    tl, ul = torch.tensor(tlen, dtype=torch.int32), torch.tensor(ulen, dtype=torch.int32)
    loss = RR.RnntLossRefFn.apply(lg, tg, tl, ul, 0).mean()
    loss.backward()
    return logits, float(loss.detach()), JW.backward(enc, dec, W, lg.grad)


def run_chain(rn, i, dtype, lens=True):
    B, T, U1, J, V, tlen, ulen = CASES[i]
    enc, dec, W, b, tg = inputs(i, dtype)
    eg, dg = enc.to(DEV, dtype).requires_grad_(), dec.to(DEV, dtype).requires_grad_()
    Wg, bg = W.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    tl, ul = torch.tensor(tlen, dtype=torch.int32, device=DEV), torch.tensor(ulen, dtype=torch.int32, device=DEV)
    logits = rn.fused_joint_logits(eg, dg, Wg, bg, 0.01, tl if lens else None, ul if lens else None)
    loss = rn.rnnt_costs(logits, tg.to(DEV), tl, ul, 0).mean()
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach(), (eg.grad, dg.grad, Wg.grad, bg.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_forward(rn, i, dtype):
    B, T, U1, J, V, _, _ = CASES[i]
    enc, dec, W, b, _ = inputs(i, dtype)
    out = rn.fused_joint_logits(enc.to(DEV, dtype), dec.to(DEV, dtype), W.to(DEV), b.to(DEV))
    ldl = (V + 31) // 32 * 32
    assert out.shape == (B, T, U1, V) and out.dtype == torch.float32 and out.stride(-2) == ldl
    got = out.cpu().double()
    ref = reference(i, dtype)[0]
    plain = JW.forward(enc, dec, W, b, rounded=False)
    print(f"case {IDS[i]} {dtype}: max |got - rounded helper| {float((got - ref).abs().max()):.2e}, max |got - plain| {float((got - plain).abs().max()):.2e}")
    torch.testing.assert_close(got, ref, atol=2e-3, rtol=1e-3)
    torch.testing.assert_close(got, plain, atol=6e-2, rtol=2e-2)
    full = out.as_strided((B, T, U1, ldl), (T * U1 * ldl, U1 * ldl, ldl, 1))
    assert torch.all(full[..., V:] == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", JW.FIXTURE_VOCABS)
def test_forward_matches_the_reference_fixture(rn, golden, V, dtype):
    enc, dec, W, b = (torch.from_numpy(x) for x in JW.fixture_inputs(V))
    if dtype == torch.bfloat16:
        enc, dec = bf(enc), bf(dec)
    out = rn.fused_joint_logits(enc.to(DEV, dtype), dec.to(DEV, dtype), W.to(DEV), b.to(DEV)).cpu()
    stored = torch.from_numpy(golden["c1_wide_vocab"][f"logits_v{V}"])
    print(f"V={V} {dtype}: max |got - reference fp32| {float((out - stored).abs().max()):.2e}")
    torch.testing.assert_close(out, stored, atol=6e-2, rtol=2e-2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_loss_chain(rn, i, dtype):
    B, T, U1, J, V, tlen, ulen = CASES[i]
    _, loss_o, grads_o = reference(i, dtype)
    _, loss, grads = run_chain(rn, i, dtype)
    print(f"case {IDS[i]} {dtype}: loss {loss.item():.6f} oracle {loss_o:.6f}")
    assert loss.item() == pytest.approx(loss_o, rel=1e-4)
    budget = 6e-3 if dtype == torch.float32 else 1.2e-2
    worst = {}
    for a, r, name in zip(grads, grads_o, ("denc", "ddec", "dW", "dbias")):
        worst[name] = float((a.double().cpu() - r).norm() / r.norm())
    print(f"case {IDS[i]} {dtype}: relative L2 {worst} (budget {budget})")
    for name, rel in worst.items():
        assert rel < budget, (name, rel)
    # nothing flows to frames >= tlen or to lattice columns > ulen
    for bi in range(B):
        assert torch.all(grads[0][bi, tlen[bi]:] == 0)
        assert torch.all(grads[1][bi, ulen[bi] + 1:] == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_two_runs_and_the_length_skip_give_the_same_bits(rn, i, dtype):
    first = run_chain(rn, i, dtype)
    second = run_chain(rn, i, dtype)
    unskipped = run_chain(rn, i, dtype, lens=False)        # tlen = ulen = None: every cell processed, the zero cells add +0
    for other in (second, unskipped):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
        for a, c in zip(first[2], other[2]):
            assert torch.equal(a, c)


@pytest.mark.parametrize("i", [3, 5, 6], ids=[IDS[3], IDS[5], IDS[6]])
def test_align_on_wide_logits(rn, i):
    B, T, U1, J, V, tlen, ulen = CASES[i]
    enc, dec, W, b, tg = inputs(i, torch.float32)
    logits = rn.fused_joint_logits(enc.to(DEV), dec.to(DEV), W.to(DEV), b.to(DEV))
    tl, ul = torch.tensor(tlen, dtype=torch.int32, device=DEV), torch.tensor(ulen, dtype=torch.int32, device=DEV)
    frames, scores = rn.rnnt_align(logits, tg.to(DEV), tl, ul, 0)
    frames, scores, lg = frames.cpu().numpy(), scores.cpu().numpy().astype(np.float64), logits.cpu().numpy()
    for bi in range(B):
        lp = AR.log_softmax(lg[bi])
        fr, opt, gap = AR.viterbi(lp, tg[bi].numpy(), tlen[bi], ulen[bi], return_gap=True)
        tol = 1e-4 + 2e-5 * abs(opt)                    # the project's budget for a (T+U)-term fp32 lattice sum (tests/test_align_gpu.py)
        own = AR.path_score(lp, tg[bi].numpy(), frames[bi], tlen[bi], ulen[bi])
        print(f"case {IDS[i]} b={bi}: score {scores[bi]:.6f} own {own:.6f} optimum {opt:.6f} gap {gap:.2e}")
        assert np.all(frames[bi, ulen[bi]:] == -1)
        assert abs(scores[bi] - own) <= tol and own >= opt - 2 * tol
        if gap > 4 * tol:                               # a unique optimum beyond the budget: the same path
            assert np.array_equal(frames[bi, :ulen[bi]], fr)
