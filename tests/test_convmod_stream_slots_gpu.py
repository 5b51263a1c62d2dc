"""tsasr_convmod_stream_slots_fwd (csrc/stream.hip) through the C-ABI at the recipe's D = 144, K = 31: the active slots' z and hist_out
rows are the bits of tsasr_convmod_stream_fwd on the same rows; the idle slot's hist_out equals its hist_in bit for bit and its z rows
are zeros. Chunks shorter (7) and longer (40) than the K - 1 history rows; `z` and `hist_out` start as NaN."""
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.golden_recipe import CFG1  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, D, K = 3, CFG1["d_model"], CFG1["kernel_size"]


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("ts-asr_amd._capi")


def ibits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [7, 40])
@pytest.mark.parametrize("t0s", [(0, -1, 5), (-1, 16, -1)], ids=["idle1", "idle02"])
def test_convmod_slots_bits(capi, dtype, C, t0s):
    assert (D, K) == (144, 31)
    g = torch.Generator().manual_seed(C * 7 + len(t0s))
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    y2 = r(B, C, 2 * D).to(DEV).to(dtype).contiguous()
    b2, w, cb, gam, bet = (t.to(DEV).contiguous() for t in (r(2 * D) * 0.1, r(D, K) * 0.2, r(D) * 0.1, 1 + 0.1 * r(D), r(D) * 0.1))
    hin = r(B, K - 1, D).to(DEV).contiguous()
    nan = float("nan")
    outs = {}
    for name in ("tsasr_convmod_stream_fwd", "tsasr_convmod_stream_slots_fwd"):
        hout = torch.full((B, K - 1, D), nan, device=DEV)
        z = torch.full((B, C, D), nan, dtype=dtype, device=DEV)
        hin0 = hin.clone()
        extra = (capi.ptr(torch.tensor(t0s, dtype=torch.int32, device=DEV)),) if name.endswith("slots_fwd") else ()
        capi.check(getattr(capi.lib(), name)(capi.ptr(y2), capi.ptr(b2), capi.ptr(w), capi.ptr(cb), capi.ptr(gam), capi.ptr(bet), capi.ptr(hin0),
                                             capi.ptr(hout), capi.ptr(z), B, C, D, K, 1e-5, 0.01, capi.io_dtype(y2), *extra, capi.stream_ptr()),
                   name)
        torch.cuda.synchronize()
        assert torch.equal(hin0, hin), "hist_in was written"
        outs[name] = (z, hout)
    (z0, h0), (z1, h1) = outs["tsasr_convmod_stream_fwd"], outs["tsasr_convmod_stream_slots_fwd"]
    assert bool(torch.isfinite(z0.float()).all()) and bool(torch.isfinite(h0).all())
    for b, t0 in enumerate(t0s):
        if t0 >= 0:
            assert torch.equal(ibits(z1[b]), ibits(z0[b])), f"slot {b}: z bits differ from the lockstep launch"
            assert torch.equal(ibits(h1[b]), ibits(h0[b])), f"slot {b}: hist_out bits differ from the lockstep launch"
        else:
            assert torch.equal(ibits(h1[b]), ibits(hin[b])), f"idle slot {b}: hist_out is not hist_in"
            assert bool((ibits(z1[b]) == 0).all()), f"idle slot {b}: z rows are not exact zeros"
            assert not torch.equal(ibits(h0[b]), ibits(hin[b]))        # (the lockstep launch does move this history)


def test_ops_wrapper_and_argument_checks(capi):
    ops = importlib.import_module("ts-asr_amd.ops")
    g = torch.Generator().manual_seed(3)
    C = 7
    y2 = torch.randn(B, C, 2 * D, generator=g).to(DEV)
    w, gam, bet = torch.randn(D, 1, K, generator=g).to(DEV), torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    hin, hout = torch.randn(B, K - 1, D, generator=g).to(DEV), torch.zeros(B, K - 1, D, device=DEV)
    t0s = torch.tensor([3, -1, 0], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        z = ops.convmod_stream(y2, None, w, None, gam, bet, hin, hout, 1e-5, 0.01, t0s)
        ref_h = torch.zeros_like(hout)
        ref = ops.convmod_stream(y2, None, w, None, gam, bet, hin, ref_h, 1e-5, 0.01)
        assert torch.equal(z[0], ref[0]) and torch.equal(z[2], ref[2]) and bool((z[1] == 0).all())
        assert torch.equal(hout[1], hin[1]) and torch.equal(hout[0], ref_h[0]) and torch.equal(hout[2], ref_h[2])
        with pytest.raises(ValueError):
            ops.convmod_stream(y2, None, w, None, gam, bet, hin, hout, 1e-5, 0.01, t0s.long())
        with pytest.raises(ValueError):
            ops.convmod_stream(y2, None, w, None, gam, bet, hin, hout, 1e-5, 0.01, t0s[:2].contiguous())
