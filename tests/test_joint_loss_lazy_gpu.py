"""The fused joint + RNN-T loss for subword vocabularies ("lazy logits": rnnt.fused_joint_logits(..., materialize=False) -> JointLogits ->
rnnt_costs / rnnt_align, csrc/joint_wide.hip joint_wide_lp / joint_wide_lazy_x / joint_wide_lazy_w) against the float64 helper of
tests/helpers/joint_wide_ref.py + oracle/rnnt_ref.py: the joint -> loss -> backward chain, the lattice plans, memory, graph capture,
alignment, argument errors, and the narrow-vocabulary detour.

Budgets are the project's own for this rounding (tests/test_joint_wide_gpu.py): loss rel 1e-4, gradient relative L2 6e-3 (fp32 storage) /
1.2e-2 (bf16), exact zeros outside the lengths; alignment scores 1e-4 + 2e-5 |score|. The difference between the two routes' costs is
printed, not asserted: they sum the same rounded operands in different orders (measured values: profiles/wide_vocab_notes.md)."""
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
import joint_wide_ref as JW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [
    # B, T, U1, J, V, tlen, ulen      (the table of tests/test_joint_wide_gpu.py: the smallest shapes at which the vocabulary tiling can go wrong)
    (1, 1, 1, 32, 33, [1], [0]),                          # one cell, one column past a tile
    (2, 7, 33, 64, 64, [7, 7], [32, 32]),                 # exactly two vocabulary tiles; u one past a tile
    (2, 19, 40, 64, 100, [19, 19], [39, 39]),             # ragged last tile
    (2, 9, 21, 160, 257, [9, 9], [20, 20]),               # odd V
    (1, 5, 3, 640, 1024, [5], [2]),                       # the maximum V at the recipe's J
    (2, 70, 33, 640, 500, [70, 66], [32, 7]),             # the chain case
    (3, 6, 5, 64, 40, [6, 4, 1], [4, 2, 0]),              # T = 1 and an empty target
    (2, 5, 34, 1024, 1024, [5, 3], [33, 6]),              # the widest joint at the widest vocabulary, ragged
]
IDS = [f"B{c[0]}-T{c[1]}-U{c[2]}-J{c[3]}-V{c[4]}" for c in CASES]
DTYPES = [torch.float32, torch.bfloat16]
CHAIN = 5
# (case, variant): every case plain, then the chain case with another blank, with labels from the first and the last vocabulary tile only,
# and with per-utterance weights on the costs
RUNS = [(i, "plain") for i in range(len(CASES))] + [(CHAIN, "blank5"), (CHAIN, "edge_labels"), (CHAIN, "weights")]
RUN_IDS = [IDS[i] if v == "plain" else f"{IDS[i]}-{v}" for i, v in RUNS]
WEIGHTS = [0.25, 3.0]


@pytest.fixture(scope="module")
def rn():
    return importlib.import_module("ts-asr_amd.rnnt")


def bf(x):
    return x.to(torch.bfloat16).float()


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def inputs(i, dtype, variant="plain"):
    """(enc, dec, W, bias, targets, blank) of a run, on the CPU; the activations are bf16 values for the bf16 runs."""
    B, T, U1, J, V, _, _ = CASES[i]
    enc = torch.from_numpy(det_tensor(f"jw.enc{i}", (B, T, J), 1.0))
    dec = torch.from_numpy(det_tensor(f"jw.dec{i}", (B, U1, J), 1.0))
    W = torch.from_numpy(det_tensor(f"jw.W{i}", (V, J), 1.0 / np.sqrt(J)))
    b = torch.from_numpy(det_tensor(f"jw.b{i}", (V,), 0.1))
    tg = np.random.default_rng(i).integers(1, V, size=(B, max(U1 - 1, 1))).astype(np.int32)
    blank = 0
    if variant == "blank5":
        blank = 5
        tg[tg == 5] = 0                                   # 0 is an ordinary label when the blank is 5
    elif variant == "edge_labels":                        # first and last vocabulary tile only, V - 1 among them
        pool = np.concatenate([np.arange(1, 32), np.arange((V - 1) // 32 * 32, V)]).astype(np.int32)
        tg = pool[np.random.default_rng(77).integers(0, len(pool), size=tg.shape)]
        tg[:, 0] = V - 1
    if dtype == torch.bfloat16:
        enc, dec = bf(enc), bf(dec)
    return enc, dec, W, b, torch.from_numpy(tg), blank


def total(costs, variant):
    if variant == "weights":
        return (costs * torch.tensor(WEIGHTS, dtype=costs.dtype, device=costs.device)).sum()
    return costs.mean()


@functools.lru_cache(maxsize=None)
def reference(i, dtype, variant="plain"):
    """float64 oracle of a run, computed once: loss and (denc, ddec, dW, dbias)."""
    _, _, _, _, _, tlen, ulen = CASES[i]
    enc, dec, W, b, tg, blank = inputs(i, dtype, variant)
    lg = JW.forward(enc, dec, W, b).requires_grad_()
    costs = RR.RnntLossRefFn.apply(lg, tg, torch.tensor(tlen, dtype=torch.int32), torch.tensor(ulen, dtype=torch.int32), blank)
    loss = total(costs, variant)
    loss.backward()
    return float(loss.detach()), JW.backward(enc, dec, W, lg.grad)


def run_chain(rn, i, dtype, variant="plain", lens=True, lazy=True):
    _, _, _, _, _, tlen, ulen = CASES[i]
    enc, dec, W, b, tg, blank = inputs(i, dtype, variant)
    eg, dg = enc.to(DEV, dtype).requires_grad_(), dec.to(DEV, dtype).requires_grad_()
    Wg, bg = W.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    tl, ul = i32(tlen), i32(ulen)
    logits = rn.fused_joint_logits(eg, dg, Wg, bg, 0.01, tl if lens else None, ul if lens else None, materialize=not lazy)
    assert isinstance(logits, rn.JointLogits) == lazy
    costs = rn.rnnt_costs(logits, tg.to(DEV), tl, ul, blank)
    loss = total(costs, variant)
    loss.backward()
    torch.cuda.synchronize()
    return costs.detach(), loss.detach(), (eg.grad, dg.grad, Wg.grad, bg.grad)


def check_against_oracle(tag, dtype, loss, grads, loss_o, grads_o, tlen, ulen):
    print(f"{tag}: loss {loss:.6f} oracle {loss_o:.6f} rel {abs(loss - loss_o) / abs(loss_o):.2e}")
    budget = 6e-3 if dtype == torch.float32 else 1.2e-2
    worst = {name: float((a.double().cpu() - r).norm() / r.norm()) for a, r, name in zip(grads, grads_o, ("denc", "ddec", "dW", "dbias"))}
    print(f"{tag}: relative L2 {worst} (budget {budget})")
    assert loss == pytest.approx(loss_o, rel=1e-4)
    for name, rel in worst.items():
        assert rel < budget, (name, rel)
    for bi in range(len(tlen)):                           # nothing flows to frames >= tlen or to lattice columns > ulen
        assert torch.all(grads[0][bi, tlen[bi]:] == 0)
        assert torch.all(grads[1][bi, ulen[bi] + 1:] == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("i,variant", RUNS, ids=RUN_IDS)
def test_chain_against_float64(rn, i, variant, dtype):
    _, _, _, _, _, tlen, ulen = CASES[i]
    loss_o, grads_o = reference(i, dtype, variant)
    costs, loss, grads = run_chain(rn, i, dtype, variant)
    costs_m = run_chain(rn, i, dtype, variant, lazy=False)[0]
    print(f"{IDS[i]}-{variant} {dtype}: max |lazy costs - materialised costs| {float((costs - costs_m).abs().max()):.3e} "
          f"(relative {float(((costs - costs_m).abs() / costs_m.abs()).max()):.3e})")
    check_against_oracle(f"{IDS[i]}-{variant} {dtype}", dtype, loss.item(), grads, loss_o, grads_o, tlen, ulen)


@pytest.mark.parametrize("i", [2, CHAIN], ids=[IDS[2], IDS[CHAIN]])
def test_materialize_is_the_eager_call(rn, i):
    _, _, _, _, _, tlen, ulen = CASES[i]
    enc, dec, W, b, _, _ = inputs(i, torch.float32)
    args = (enc.to(DEV), dec.to(DEV), W.to(DEV), b.to(DEV), 0.01, i32(tlen), i32(ulen))
    handle = rn.fused_joint_logits(*args, materialize=False)
    eager = rn.fused_joint_logits(*args)
    got = handle.materialize()
    assert handle.shape == eager.shape and got.stride() == eager.stride() and torch.equal(got, eager)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_two_runs_and_the_handle_lengths_give_the_same_bits(rn, i, dtype):
    first = run_chain(rn, i, dtype)
    second = run_chain(rn, i, dtype)
    no_lens = run_chain(rn, i, dtype, lens=False)         # a handle without lengths: the lengths given to the loss are the ones used
    for other in (second, no_lens):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
        for a, c in zip(first[2], other[2]):
            assert torch.equal(a, c)


PLAN_CASES = [
    (1, 20, 300, 64, 100, [20], [299]),
    (2, 5, 300, 64, 40, [5, 1], [299, 0]),                # fewer frames than one prefetch window; an empty target
]
PLANS = [(0, 4, 0), (1, 4, 0), (1, 8, 0), (1, 16, 0), (2, 1, 0), (1, 8, 1), (1, 8, 2), (1, 8, 4), (-1, -1, -1)]      # tests/test_rnnt_gpu.py's nine


@pytest.mark.parametrize("B,T,U1,J,V,tlen,ulen", PLAN_CASES, ids=["B1-T20-U300-V100", "B2-T5-U300-V40"])
def test_lattice_plans_give_the_same_bits(rn, B, T, U1, J, V, tlen, ulen):
    C = importlib.import_module("ts-asr_amd._capi")
    enc = torch.from_numpy(det_tensor(f"jl.plan.enc{B}", (B, T, J), 1.0))
    dec = torch.from_numpy(det_tensor(f"jl.plan.dec{B}", (B, U1, J), 1.0))
    W = torch.from_numpy(det_tensor(f"jl.plan.W{B}", (V, J), 1.0 / np.sqrt(J)))
    b = torch.from_numpy(det_tensor(f"jl.plan.b{B}", (V,), 0.1))
    tg = torch.from_numpy(np.random.default_rng(B * 31 + U1).integers(1, V, size=(B, U1 - 1)).astype(np.int32))
    lg = JW.forward(enc, dec, W, b).requires_grad_()
    loss_o = RR.RnntLossRefFn.apply(lg, tg, torch.tensor(tlen, dtype=torch.int32), torch.tensor(ulen, dtype=torch.int32), 0).mean()
    loss_o.backward()
    grads_o = JW.backward(enc, dec, W, lg.grad)
    outs = []
    try:
        for plan in PLANS:
            C.lib().tsasr_rnnt_lattice_plan(*plan)
            leaves = [x.to(DEV).requires_grad_() for x in (enc, dec, W, b)]
            handle = rn.fused_joint_logits(*leaves, 0.01, materialize=False)
            costs = rn.rnnt_costs(handle, tg.to(DEV), i32(tlen), i32(ulen), 0)
            costs.mean().backward()
            torch.cuda.synchronize()
            outs.append((costs.detach(), [x.grad for x in leaves]))
    finally:
        C.lib().tsasr_rnnt_lattice_plan(-1, -1, -1)
    check_against_oracle(f"plan {PLANS[0]} U1={U1} V={V}", torch.float32, outs[0][0].mean().item(), outs[0][1], float(loss_o.detach()), grads_o,
                         tlen, ulen)
    for plan, (c, g) in zip(PLANS[1:], outs[1:]):
        assert torch.equal(c, outs[0][0]), plan
        for a, r in zip(g, outs[0][1]):
            assert torch.equal(a, r), plan


def test_no_logits_sized_allocation(rn):
    """A condition, not a measurement: B = 4, T = 128, U1 = 65, J = 64, V = 1024 - one logits tensor is 136 MB, the fused loss's lattice
    planes and backward workspace come to under 20 MB. The lazy chain must stay below half a logits tensor; the
    materialised chain on the same inputs must exceed one, which proves that the probe sees what it should."""
    B, T, U1, J, V = 4, 128, 65, 64, 1024
    one_logits = B * T * U1 * V * 4
    g = torch.Generator().manual_seed(5)
    enc, dec = torch.randn(B, T, J, generator=g), torch.randn(B, U1, J, generator=g)
    W, b = torch.randn(V, J, generator=g) / 8, torch.randn(V, generator=g) / 10
    tg = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32).to(DEV)
    tl, ul = i32([T] * B), i32([U1 - 1] * B)
    rise = {}
    for lazy in (True, False):
        leaves = [x.to(DEV).requires_grad_() for x in (enc, dec, W, b)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        logits = rn.fused_joint_logits(*leaves, 0.01, tl, ul, materialize=not lazy)
        rn.rnnt_costs(logits, tg, tl, ul, 0).mean().backward()
        torch.cuda.synchronize()
        rise[lazy] = torch.cuda.max_memory_allocated() - base
        del logits, leaves
    print(f"peak rise: lazy {rise[True] / 1e6:.1f} MB, materialised {rise[False] / 1e6:.1f} MB (one logits tensor {one_logits / 1e6:.1f} MB)")
    assert rise[True] < one_logits // 2
    assert rise[False] > one_logits


def test_captured_in_a_graph_gives_the_same_bits(rn):
    """tsasr_joint_wide_loss_fwd + _bwd captured on one stream and replayed twice (workspace and outputs scribbled over in between) == eager."""
    C = importlib.import_module("ts-asr_amd._capi")
    lib = C.lib()
    B, T, U1, J, V, tlen, ulen = CASES[CHAIN]
    enc, dec, W, b, tg, blank = (x.to(DEV) if torch.is_tensor(x) else x for x in inputs(CHAIN, torch.float32))
    tl, ul, gs = i32(tlen), i32(ulen), torch.tensor(WEIGHTS, device=DEV)
    costs = torch.empty(B, device=DEV)
    outs = [torch.empty_like(enc), torch.empty_like(dec), torch.empty_like(W), torch.empty_like(b)]
    ws = torch.empty(lib.tsasr_joint_wide_loss_workspace_bytes(B, T, U1, J, V), device=DEV, dtype=torch.uint8)

    def launch():
        C.check(lib.tsasr_joint_wide_loss_fwd(C.ptr(enc), C.ptr(dec), C.ptr(W), C.ptr(b), C.ptr(tg), tg.stride(0), C.ptr(tl), C.ptr(ul), C.ptr(costs),
                                              B, T, U1, J, V, blank, C.F32, 0.01, C.ptr(ws), ws.numel(), C.stream_ptr()), "fwd")
        C.check(lib.tsasr_joint_wide_loss_bwd(C.ptr(enc), C.ptr(dec), C.ptr(W), C.ptr(b), C.ptr(tg), tg.stride(0), C.ptr(tl), C.ptr(ul), C.ptr(gs),
                                              *(C.ptr(o) for o in outs), B, T, U1, J, V, blank, C.F32, 0.01, C.ptr(ws), ws.numel(),
                                              C.stream_ptr()), "bwd")

    launch()
    torch.cuda.synchronize()
    eager = [costs.clone()] + [o.clone() for o in outs]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        ws.fill_(0xFF)
        for o in [costs] + outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip([costs] + outs, eager):
            assert torch.equal(got, want)


@pytest.mark.parametrize("i", [3, 5, 6], ids=[IDS[3], IDS[5], IDS[6]])
def test_align_on_a_handle(rn, i):
    _, _, _, _, _, tlen, ulen = CASES[i]
    enc, dec, W, b, tg, _ = inputs(i, torch.float32)
    handle = rn.fused_joint_logits(enc.to(DEV), dec.to(DEV), W.to(DEV), b.to(DEV), materialize=False)
    tl, ul = i32(tlen), i32(ulen)
    frames, scores = rn.rnnt_align(handle, tg.to(DEV), tl, ul, 0)
    frames_m, scores_m = rn.rnnt_align(handle.materialize(), tg.to(DEV), tl, ul, 0)
    print(f"case {IDS[i]}: scores {scores.tolist()} materialised {scores_m.tolist()}")
    assert torch.equal(frames, frames_m)
    assert torch.all((scores - scores_m).abs() <= 1e-4 + 2e-5 * scores_m.abs())


def test_argument_errors(rn):
    C = importlib.import_module("ts-asr_amd._capi")
    lib = C.lib()
    one = i32([1])

    def handle(J, V):
        return rn.fused_joint_logits(torch.zeros(1, 2, J, device=DEV), torch.zeros(1, 3, J, device=DEV), torch.zeros(V, J, device=DEV),
                                     torch.zeros(V, device=DEV), materialize=False)

    good_tg = torch.ones(1, 2, device=DEV, dtype=torch.int32)
    for J, V in ((64, 1025), (48, 100)):
        with pytest.raises(ValueError):
            rn.rnnt_costs(handle(J, V), good_tg, one, one, 0)
        with pytest.raises(ValueError):
            rn.rnnt_align(handle(J, V), good_tg, one, one, 0)
    with pytest.raises(ValueError):
        rn.rnnt_costs(handle(64, 100), torch.ones(1, 1, device=DEV, dtype=torch.int32), one, one, 0)      # targets shorter than U1 - 1
    # the launchers themselves: the same ranges, and a workspace one byte short
    B, T, U1, J, V = 1, 2, 3, 64, 100
    h = handle(J, V)
    costs = torch.empty(B, device=DEV)
    nws = lib.tsasr_joint_wide_loss_workspace_bytes(B, T, U1, J, V)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)

    def fwd(J_, V_, ldt, nbytes):
        return lib.tsasr_joint_wide_loss_fwd(C.ptr(h.enc), C.ptr(h.dec), C.ptr(h.weight), C.ptr(h.bias), C.ptr(good_tg), ldt, C.ptr(one), C.ptr(one),
                                             C.ptr(costs), B, T, U1, J_, V_, 0, C.F32, 0.01, C.ptr(ws), nbytes, C.stream_ptr())

    assert fwd(J, V, 2, nws) == 0
    for bad in ((J, 1025, 2, nws), (48, V, 2, nws), (J, V, 1, nws), (J, V, 2, nws - 1)):
        with pytest.raises(C.TsasrHipError):
            C.check(fwd(*bad), "tsasr_joint_wide_loss_fwd")
    gs = torch.ones(B, device=DEV)
    outs = [torch.empty_like(h.enc), torch.empty_like(h.dec), torch.empty_like(h.weight), torch.empty_like(h.bias)]
    with pytest.raises(C.TsasrHipError):
        C.check(lib.tsasr_joint_wide_loss_bwd(C.ptr(h.enc), C.ptr(h.dec), C.ptr(h.weight), C.ptr(h.bias), C.ptr(good_tg), 2, C.ptr(one), C.ptr(one),
                                              C.ptr(gs), *(C.ptr(o) for o in outs), B, T, U1, J, V, 0, C.F32, 0.01, C.ptr(ws), nws - 1,
                                              C.stream_ptr()), "tsasr_joint_wide_loss_bwd")
    frames, scores = torch.empty(B, 2, device=DEV, dtype=torch.int32), torch.empty(B, device=DEV)
    aws = torch.empty(lib.tsasr_joint_wide_align_workspace_bytes(B, T, U1, J, V), device=DEV, dtype=torch.uint8)
    with pytest.raises(C.TsasrHipError):
        C.check(lib.tsasr_joint_wide_align(C.ptr(h.enc), C.ptr(h.dec), C.ptr(h.weight), C.ptr(h.bias), C.ptr(good_tg), 2, C.ptr(one), C.ptr(one),
                                           C.ptr(frames), 2, C.ptr(scores), B, T, U1, J, V, 0, C.F32, 0.01, C.ptr(aws), aws.numel() - 1,
                                           C.stream_ptr()), "tsasr_joint_wide_align")
    torch.cuda.synchronize()


def test_a_narrow_handle_takes_the_materialised_route(rn):
    """V = 29: the handle is materialised inside transducer_loss; loss and gradients are the eager route's bits."""
    B, T, U1, J, V = 2, 11, 6, 64, 29
    g = torch.Generator().manual_seed(3)
    enc, dec, W, b = torch.randn(B, T, J, generator=g), torch.randn(B, U1, J, generator=g), torch.randn(V, J, generator=g) / 8, torch.randn(V, generator=g)
    tg = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32).to(DEV)
    rel_t, rel_u = torch.tensor([1.0, 0.8], device=DEV), torch.tensor([1.0, 0.6], device=DEV)
    res = []
    for lazy in (True, False):
        leaves = [x.to(DEV).requires_grad_() for x in (enc, dec, W, b)]
        logits = rn.fused_joint_logits(*leaves, 0.01, materialize=not lazy)
        assert isinstance(logits, rn.JointLogits) == lazy
        loss = rn.transducer_loss(logits, tg, rel_t, rel_u, 0)
        loss.backward()
        res.append([loss.detach()] + [x.grad for x in leaves])
    for a, c in zip(*res):
        assert torch.equal(a, c)
