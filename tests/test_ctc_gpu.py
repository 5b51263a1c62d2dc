"""csrc/ctc.hip against the float64 helper (tests/helpers/ctc_ref.py, itself pinned to brute force and to torch's CPU function in
tests/test_ctc_ref_cpu.py) on exactly the values the kernels see (bf16 scores are upcast), over tests/helpers/ctc_cases.py.

Tolerances are the issue's, applied to the values the kernel writes (gscale included): costs rtol 2e-5, atol 1e-4; gradients atol 3e-5, rtol
max(1e-3, 5e-5 * (T + S)), bf16 dlogits 2^-8 relative more; row sums of dlogits within 5e-6 * |gscale|. One of them cannot hold as written and is set,
as the issue prescribes, at twice the measured worst value (profiles/ctc_notes.md section 1 has the figure and the cause): the row sums
of bf16 dlogits, whose elements are each rounded to 8 bits on the way out (measured 3.97e-3 * |gscale| at scale-30 scores, where single
elements are near 1; bound 7.94e-3). Every other bound, the gradient's at gscale = 1e3 included, is the issue's.

Every case runs three times through the C entry points: outputs and workspace filled with zeros, then twice with 0xFF bytes (NaN as
floats, -1 as integers); all three must give the same bits. Rows of `logits` are padded to ld = 8 * ceil(V / 8) with a large finite value
in the pad columns, `targets` to ldt = U + 3 with out-of-range ids: neither may reach a result."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import ctc_cases, ctc_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}
ROWSUM_BF16 = 2 * 3.97e-3      # x |gscale|: twice the measured worst (ragged_bf16_s30), see the docstring


def C():
    return importlib.import_module("ts-asr_amd._capi")


def reference(name):
    """The helper's result for a case, computed once and shared by every test that needs it."""
    if name not in _REF:
        c = ctc_cases.get(name)
        _REF[name] = ctc_ref.ctc_ref(ctc_cases.seen(c), c["targets"], c["tlen"], c["ulen"], c["blank"], c["gscale"])
    return _REF[name]


def run_raw(case, fill):
    """tsasr_ctc_loss_fwd + _bwd on freshly filled buffers: (costs [B], dlogits [B,T,ld] as float32, rc)."""
    cap, lib = C(), C().lib()
    B, T, V = case["x"].shape
    U, ld = case["targets"].shape[1], ctc_cases.ld_of(V)
    dt = torch.bfloat16 if case["dtype"] == "bf16" else torch.float32
    x = torch.full((B, T, ld), 77.0, dtype=dt, device=DEV)
    x[..., :V] = torch.from_numpy(case["x"]).to(dt)
    ldt = U + 3
    tg = torch.full((B, ldt), 2 ** 31 - 1, dtype=torch.int32, device=DEV)
    tg[:, :U] = torch.from_numpy(np.clip(case["targets"], -(2 ** 31), 2 ** 31 - 1).astype(np.int32))
    tlen = torch.from_numpy(case["tlen"].astype(np.int32)).to(DEV)
    ulen = torch.from_numpy(case["ulen"].astype(np.int32)).to(DEV)
    gs = torch.from_numpy(case["gscale"].astype(np.float32)).to(DEV)
    nws = lib.tsasr_ctc_loss_workspace_bytes(B, T, U, V)
    assert nws > 0
    ws = torch.full((nws,), fill, dtype=torch.uint8, device=DEV)
    costs = torch.full((B,), fill, dtype=torch.uint8, device=DEV).repeat_interleave(4).view(torch.float32)
    dl = torch.full((B * T * ld * (2 if dt == torch.bfloat16 else 4),), fill, dtype=torch.uint8, device=DEV).view(dt).view(B, T, ld)
    st = cap.stream_ptr()
    rc = lib.tsasr_ctc_loss_fwd(cap.ptr(x), cap.ptr(tg), ldt, cap.ptr(tlen), cap.ptr(ulen), cap.ptr(costs), B, T, U, V, ld, case["blank"],
                                cap.io_dtype(x), cap.ptr(ws), nws, st)
    assert rc == 0, lib.tsasr_last_error()
    rc = lib.tsasr_ctc_loss_bwd(cap.ptr(x), cap.ptr(tg), ldt, cap.ptr(tlen), cap.ptr(ulen), cap.ptr(gs), cap.ptr(dl), B, T, U, V, ld,
                                case["blank"], cap.io_dtype(x), cap.ptr(ws), nws, st)
    assert rc == 0, lib.tsasr_last_error()
    torch.cuda.synchronize()
    return costs.cpu().numpy(), dl.float().cpu().numpy()


@pytest.mark.parametrize("name", ctc_cases.NAMES)
def test_loss_and_gradient_against_float64(name):
    case, ref = ctc_cases.get(name), reference(name)
    B, T, V = case["x"].shape
    U = case["targets"].shape[1]
    S = 2 * U + 1
    bf16 = case["dtype"] == "bf16"
    costs, dl = run_raw(case, 0)
    for fill in (255, 255):      # NaN-filled outputs and workspace, twice: the same bits as the zero-filled run
        c2, d2 = run_raw(case, fill)
        assert np.array_equal(costs.view(np.uint32), c2.view(np.uint32)) and np.array_equal(dl.view(np.uint32), d2.view(np.uint32)), fill
    bad = sorted(np.nonzero(~ref["feasible"])[0])
    if not name.startswith("grid"):
        assert bad == sorted(case["infeasible"])
    tl, ul = ctc_ref.lengths(case["tlen"], case["ulen"], T, U)
    g = case["gscale"]
    rtol = max(1e-3, 5e-5 * (T + S)) + (2.0 ** -8 if bf16 else 0.0)
    worst_c = np.max(np.abs(costs - ref["costs"]) / (1e-4 + 2e-5 * np.abs(ref["costs"])))
    print(f"{name}: costs {costs[:6]} worst cost error / bound {worst_c:.3f}")
    assert np.all(np.isfinite(costs)) and np.all(np.isfinite(dl))
    np.testing.assert_allclose(costs, ref["costs"], rtol=2e-5, atol=1e-4)
    assert np.all(dl[..., V:] == 0)                                          # pad columns
    for b in range(B):
        assert np.all(dl[b, tl[b]:] == 0)                                    # dead rows
        if b in bad:                                                         # infeasible: cost 0, zero gradient (the others ARE compared)
            assert costs[b] == 0 and np.all(dl[b] == 0)
            continue
        live = dl[b, :tl[b], :V].astype(np.float64)
        if g[b] == 0:
            assert np.all(live == 0)
            continue
        want = ref["grad"][b, :tl[b]]
        need = float(np.max(np.abs(live - want) - rtol * np.abs(want)))          # the atol this utterance needs beside the issue's rtol
        rowsum = float(np.max(np.abs(live.sum(-1))) / abs(g[b]))
        print(f"  MEAS {name} b={b} gscale={g[b]:g} atol-needed {need:.3e} rowsum/|gscale| {rowsum:.3e}")
        assert need <= 3e-5, (b, need)
        assert rowsum <= (ROWSUM_BF16 if bf16 else 5e-6), (b, rowsum)


def test_limit_case_cost_is_the_single_path():
    case = ctc_cases.get("limit")
    costs, dl = run_raw(case, 255)
    lp = ctc_ref.log_softmax(case["x"][0, :9])
    assert costs[0] == pytest.approx(-sum(lp[t, k] for t, k in enumerate(ctc_cases.LIMIT_PATH)), rel=2e-5, abs=1e-4)
    assert costs[1] == 0 and np.all(dl[1] == 0)       # one frame fewer: no path


def test_autograd_entry_and_reductions():
    """ctc_costs / ctc_loss through autograd on tensors that need the padding copy (V = 29 contiguous) and on ones that do not; the five
    reductions on relative lengths; log-probs and raw scores give the same value."""
    ctc = importlib.import_module("ts-asr_amd.ctc")
    case, ref = ctc_cases.get("ragged_fp32_s1"), reference("ragged_fp32_s1")
    B, T, V = case["x"].shape
    U = case["targets"].shape[1]
    x = torch.from_numpy(case["x"]).to(DEV).requires_grad_()
    tg = torch.from_numpy(np.clip(case["targets"], -(2 ** 31), 2 ** 31 - 1)).to(DEV)
    tl, ul = torch.from_numpy(case["tlen"]).to(DEV), torch.from_numpy(case["ulen"]).to(DEV)
    costs = ctc.ctc_costs(x, tg, tl, ul, 0)
    costs.backward(torch.from_numpy(case["gscale"]).float().to(DEV))
    np.testing.assert_allclose(costs.detach().cpu().numpy(), ref["costs"], rtol=2e-5, atol=1e-4)
    assert x.grad.shape == x.shape
    np.testing.assert_allclose(x.grad.cpu().numpy(), ref["grad"], atol=3e-5, rtol=max(1e-3, 5e-5 * (T + 2 * U + 1)))
    rel_t, rel_u = (tl.float() / T), (ul.float() / U)
    c = torch.from_numpy(ref["costs"]).float()
    ulc = torch.from_numpy(case["ulen"]).float()
    want = {"none": c, "sum": c.sum(), "batchmean": c.sum() / B, "mean": (c / ulc.clamp(min=1)).mean(), "batch": c / ulc}
    lp = torch.log_softmax(x.detach(), -1)
    for red, w in want.items():
        for scores in (x.detach(), lp):
            got = ctc.ctc_loss(scores, tg, rel_t, rel_u, 0, reduction=red).cpu()
            torch.testing.assert_close(got, w, rtol=3e-5, atol=1e-4, equal_nan=True)     # ("batch": 0 / 0 for the empty target, as the reference)


def test_out_of_range_shapes_raise_before_any_launch(monkeypatch):
    ctc = importlib.import_module("ts-asr_amd.ctc")
    cap, lib = C(), C().lib()
    ok = dict(B=2, T=4, U=3, V=8, ld=8, blank=0)
    x = torch.zeros(2, 4, 1032, device=DEV)
    tg = torch.zeros(2, 2048, dtype=torch.int32, device=DEV)
    ln = torch.ones(2, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    costs = torch.full((2,), 7.0, device=DEV)
    for bad in (dict(V=1025, ld=1032), dict(V=0), dict(U=2048), dict(U=-1), dict(T=0), dict(B=0), dict(ld=12), dict(ld=4), dict(blank=8),
                dict(blank=-1)):
        a = dict(ok, **bad)
        rc = lib.tsasr_ctc_loss_fwd(cap.ptr(x), cap.ptr(tg), 2048, cap.ptr(ln), cap.ptr(ln), cap.ptr(costs), a["B"], a["T"], a["U"], a["V"], a["ld"],
                                    a["blank"], 0, cap.ptr(ws), ws.numel(), cap.stream_ptr())
        assert rc == -1, bad
        rc = lib.tsasr_ctc_loss_bwd(cap.ptr(x), cap.ptr(tg), 2048, cap.ptr(ln), cap.ptr(ln), cap.ptr(costs), cap.ptr(x), a["B"], a["T"], a["U"],
                                    a["V"], a["ld"], a["blank"], 0, cap.ptr(ws), ws.numel(), cap.stream_ptr())
        assert rc == -1, bad
        if "U" not in bad:
            rc = lib.tsasr_ctc_greedy(cap.ptr(x), cap.ptr(ln), cap.ptr(tg), 2048, cap.ptr(ln), a["B"], a["T"], a["V"], a["ld"], a["blank"], 0,
                                      cap.stream_ptr())
            assert rc == -1, bad
    assert lib.tsasr_ctc_loss_workspace_bytes(2, 4, 2048, 8) == 0 and lib.tsasr_ctc_loss_workspace_bytes(2, 4, 3, 1025) == 0
    rc = lib.tsasr_ctc_loss_fwd(cap.ptr(x), cap.ptr(tg), 2048, cap.ptr(ln), cap.ptr(ln), cap.ptr(costs), 2, 4, 3, 8, 8, 0, 0, cap.ptr(ws), 16,
                                cap.stream_ptr())
    assert rc == -1                                  # workspace too small
    torch.cuda.synchronize()
    assert torch.all(costs == 7.0)                   # nothing ran
    # the host mirror raises ValueError without reaching the library
    real = cap.lib

    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(cap, "lib", no_lib)
    try:
        z = torch.zeros(2, 4, 1025, device=DEV)
        t3 = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError):
            ctc.ctc_costs(z, t3, ln, ln, 0)
        with pytest.raises(ValueError):
            ctc.ctc_costs(z[..., :8], torch.zeros(2, 2048, dtype=torch.int64, device=DEV), ln, ln, 0)
        with pytest.raises(ValueError):
            ctc.ctc_costs(z[..., :8], t3, ln, ln, 8)
        with pytest.raises(ValueError):
            ctc.ctc_greedy_tokens(z, ln, 0)
    finally:
        monkeypatch.setattr(cap, "lib", real)


def _greedy_scores(want, V, rng):
    """Scores [T,V] without ties whose per-frame argmax is want[t]: a permutation of distinct quarter-integers (exact in bf16 up to V = 1024
    would need more than 8 bits, so the maximum is lifted well clear of the rest instead)."""
    T = len(want)
    x = rng.permuted(np.tile(np.arange(V, dtype=np.float32) % 64, (T, 1)), axis=1) / 4.0
    x[np.arange(T), want] = 40.0
    return x


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V,blank", [(5, 0), (29, 28), (1024, 0)])
def test_greedy_equals_the_python_collapse(V, blank, dtype):
    ctc = importlib.import_module("ts-asr_amd.ctc")
    rng = np.random.default_rng(V)
    T, B = 600, 6
    a, c = (blank + 1) % V, (blank + 2) % V
    want = np.full((B, T), blank, np.int64)
    want[0] = rng.integers(0, V, T)                                       # arbitrary labels, few repeats
    want[1] = np.repeat(rng.integers(0, min(V, 4), T // 4), 4)            # runs and blanks, across the 256-frame chunks
    want[1, 250:262] = a                                                  # one run over the first chunk boundary
    want[3, :] = a                                                        # one run that crosses tlen (and the chunk boundaries)
    want[4, :300] = a
    want[4, 300:] = c                                                     # the label after tlen must not appear
    want[5, 0] = c                                                        # a single live frame
    tlen = np.array([T, T, T, 257, 300, 1])                               # [2]: all-blank rows
    x = np.stack([_greedy_scores(want[b], V, rng) for b in range(B)])
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    xd = torch.from_numpy(x).to(dt).to(DEV)
    tokens, ntok = ctc.ctc_greedy_tokens(xd, torch.from_numpy(tlen).to(DEV), blank)
    ref = ctc_ref.greedy_ref(xd.float().cpu().numpy(), tlen, blank)
    assert ref[2] == [] and ref[3] == [a] and ref[4] == [a] and ref[5] == [c]
    tokens, ntok = tokens.cpu().numpy(), ntok.cpu().numpy()
    assert tokens.shape == (B, T)
    for b in range(B):
        assert ntok[b] == len(ref[b]) and list(tokens[b, :ntok[b]]) == ref[b], b
        assert np.all(tokens[b, ntok[b]:] == -1)
    # the drop-in: relative lengths, list of lists; and its device form
    rel = torch.from_numpy(tlen / T).float().to(DEV)
    assert ctc.ctc_greedy_decode(xd, rel, blank) == ref
    t2, n2 = ctc.ctc_greedy_decode(xd, rel, blank - V, return_tensors=True)        # a negative blank id counts from the end
    assert t2.is_cuda and np.array_equal(t2.cpu().numpy(), tokens) and np.array_equal(n2.cpu().numpy(), ntok)


def test_greedy_tie_takes_the_lowest_index():
    ctc = importlib.import_module("ts-asr_amd.ctc")
    x = torch.zeros(1, 4, 200, device=DEV)
    x[0, 0, [70, 3, 130]] = 5.0           # equal maxima in three different lanes' strides: 3 wins
    x[0, 1, [199, 64]] = 5.0              # 64
    x[0, 2, :] = 1.0                      # every column equal: 0 = blank
    x[0, 3, [64, 65]] = 2.0               # 64 again, after a blank: emitted again
    tokens, ntok = ctc.ctc_greedy_tokens(x, torch.tensor([4], device=DEV), 0)
    assert int(ntok[0]) == 3 and tokens[0, :3].tolist() == [3, 64, 64] and torch.all(tokens[0, 3:] == -1)


def _host_route(poison):
    """ctc.project + ctc_costs + backward for the bf16 29-row head (the padded GEMM whose pad columns the loss reads in place), optionally
    with every torch.empty / empty_like on the GPU filled with NaN / 0xFF first, as tests/helpers/poison_empty.py does for the step."""
    ctc = importlib.import_module("ts-asr_amd.ctc")
    nnet = importlib.import_module("ts-asr_amd.nnet")
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_cuda and t.numel():
            t.fill_(float("nan")) if t.dtype.is_floating_point else t.fill_(255 if t.dtype == torch.uint8 else -1)
        return t

    torch.manual_seed(3)
    head = nnet.Linear(input_size=64, n_neurons=29).to(DEV)
    case = ctc_cases.get("ragged_bf16_s1")
    B, T, V = case["x"].shape
    x = (torch.randn(B, T, 64) * 0.5).to(torch.bfloat16).to(DEV).requires_grad_()
    tg = torch.from_numpy(np.clip(case["targets"], -(2 ** 31), 2 ** 31 - 1)).to(DEV)
    tl, ul = torch.from_numpy(case["tlen"]).to(DEV), torch.from_numpy(case["ulen"]).to(DEV)
    if poison:
        torch.empty, torch.empty_like = (lambda *a, **k: fill(empty(*a, **k))), (lambda *a, **k: fill(empty_like(*a, **k)))
    try:
        s = ctc.project(head, x)
        costs = ctc.ctc_costs(s, tg, tl, ul, 0)
        costs.backward(torch.from_numpy(case["gscale"]).float().to(DEV))
        torch.cuda.synchronize()
    finally:
        torch.empty, torch.empty_like = empty, empty_like
    return [t.detach().float().cpu() for t in (s, costs, x.grad, head.w.weight.grad, head.w.bias.grad)]


def test_host_route_does_not_depend_on_uninitialised_memory():
    clean, dirty, again = _host_route(False), _host_route(True), _host_route(True)
    for a, b, c in zip(clean, dirty, again):
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("V", [29, 32, 5])
def test_projection_against_fp32_linear(V):
    """ctc.project (V = 29, 5: the zero-padded bf16 GEMMs of _ProjPaddedFn; V = 32: nnet.Linear's own route) and its three gradients
    against F.linear in fp32 on the SAME bf16-rounded operands. What differs is the rounding of the outputs to bf16 (2^-9 relative
    each) and, in the backward, of dy: rtol 2^-7, atol 2^-7 x the tensor's root-mean-square (sums of up to 640 rounded terms)."""
    ctc = importlib.import_module("ts-asr_amd.ctc")
    nnet = importlib.import_module("ts-asr_amd.nnet")
    ops = importlib.import_module("ts-asr_amd.ops")
    nnet.set_compute_dtype(torch.bfloat16)
    ops.LIB_FALLBACKS.clear()
    torch.manual_seed(V)
    B, T, K = 3, 41, 64
    head = nnet.Linear(input_size=K, n_neurons=V).to(DEV)
    with torch.no_grad():
        head.w.bias.copy_(torch.randn(V))
    x = torch.randn(B, T, K).to(torch.bfloat16).to(DEV).requires_grad_()
    dy = torch.randn(B, T, V).to(torch.bfloat16).to(DEV)
    y = ctc.project(head, x)
    assert tuple(y.shape) == (B, T, V) and y.dtype == torch.bfloat16
    y.backward(dy)
    torch.cuda.synchronize()
    xr = x.detach().float().cpu().requires_grad_()
    wr = head.w.weight.detach().to(torch.bfloat16).float().cpu().requires_grad_()
    br = head.w.bias.detach().float().cpu().requires_grad_()
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(dy.float().cpu())
    tol = 2.0 ** -7
    for name, got, want in (("y", y, yr), ("dx", x.grad, xr.grad), ("dW", head.w.weight.grad, wr.grad), ("db", head.w.bias.grad, br.grad)):
        got, want = got.detach().float().cpu(), want.detach()
        assert got.shape == want.shape, name
        err = (got - want).abs()
        print(f"V={V} {name}: worst error / bound {float((err / (tol * want.pow(2).mean().sqrt() + tol * want.abs())).max()):.3f}")
        torch.testing.assert_close(got, want, rtol=tol, atol=tol * float(want.pow(2).mean().sqrt()), msg=lambda m, n=name: f"{n}: {m}")
    assert not ops.LIB_FALLBACKS, ops.LIB_FALLBACKS
