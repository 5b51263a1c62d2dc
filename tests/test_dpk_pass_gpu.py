"""The d(pk) pass that reads dS once (csrc/dpk_pass.h, dpk_once_body) against the body it replaces on the short path (dpk_body), through the
lab entry tsasr_lab_dpk: seeded normal dS and q + v rounded to bf16, NaN wherever the pass must not look, partial planes pre-filled with
0xFF bytes and d(pk) with NaN. The new body issues the same MFMAs on the same operands in the same order per accumulator, so the check is
plain equality of d(pk) and of every partial plane, bit for bit. On top of it both bodies are held to a float64 sum over the same
tensors: the output is rounded once to bf16 (<= 2^-9 |ref|) after an fp32 accumulation of n <= B T' <= 2^13 products (<= n 2^-24 S,
S = the float64 sum of |dS| |q + v| over the same terms), so |out - ref| <= 2^-8 |ref| + 2^-11 S per element."""
import importlib

import pytest
import torch

from tests.helpers import dpk_walk
from tests.helpers.attn_ref import allowed_mask

pytestmark = pytest.mark.gpu

SHAPES = [2, 63, 64, 65, 125, 128, 250, 256]
CASES = [(5, 2, T, causal, True) for T in SHAPES for causal in (0, 1, 16)] + [(32, 4, 250, 0, False), (32, 4, 125, 0, False)]


def lens_for(T, B):
    return [T, 1, max(1, T // 2), max(1, T - 1), min(T, 65)][:B]


def run(capi, body, ds, qv, lens, B, T, H, causal):
    nbytes = capi.lab().tsasr_lab_dpk_part_bytes(B, T, H)
    assert nbytes == dpk_walk.part_bytes(B, T, H)
    part = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    dpk = torch.full((2 * T - 1, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    rc = capi.lab().tsasr_lab_dpk(body, capi.ptr(ds), capi.ptr(qv), capi.ptr(lens) if lens is not None else None, capi.ptr(part), capi.ptr(dpk),
                                  B, T, H, causal, capi.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return part.view(torch.int32), dpk


def float64_sums(ds, qv, allowed, B, T, H):
    """(ref, S) [2T-1, H*64] float64: sum and sum of magnitudes of dS[b,h,i,j] (q+v)[h,b,i,:] over the allowed pairs with j - i + T - 1 = r."""
    R = 2 * T - 1
    i = torch.arange(T, device="cuda")
    r = torch.arange(R, device="cuda")
    j = r[:, None] + i[None, :] - (T - 1)                                           # [R, T]
    inside = (j >= 0) & (j < T)
    jc = j.clamp(0, T - 1)
    ref = torch.zeros(R, H, 64, dtype=torch.float64, device="cuda")
    mag = torch.zeros_like(ref)
    for b in range(B):
        ok = inside & allowed[b][i[None, :].expand(R, T), jc]                      # [R, T]
        for h in range(H):
            skew = torch.where(ok, ds[b, h][i[None, :].expand(R, T), jc].double(), torch.zeros((), dtype=torch.float64, device="cuda"))
            x = qv[h, b * T:(b + 1) * T].double()
            ref[:, h] += skew @ x
            mag[:, h] += skew.abs() @ x.abs()
    return ref.reshape(R, H * 64), mag.reshape(R, H * 64)


@pytest.mark.parametrize("B,H,T,causal,ragged", CASES)
def test_one_pass_body_is_the_old_body_bit_for_bit(pkg, B, H, T, causal, ragged):
    capi = importlib.import_module("ts-asr_amd._capi")
    Tp = dpk_walk.cdiv(T, 64) * 64
    g = torch.Generator().manual_seed(1000 * T + 10 * causal + B)
    lens_list = lens_for(T, B) if ragged else [T] * B
    allowed = allowed_mask(T, lens_list, causal).cuda()                            # [B, i, j]
    ds = torch.full((B, H, T, Tp), float("nan"), dtype=torch.bfloat16)
    vals = torch.randn(B, H, T, T, generator=g).to(torch.bfloat16)
    ds[..., :T] = torch.where(allowed.cpu()[:, None], vals, torch.full((), float("nan"), dtype=torch.bfloat16))
    ds = ds.cuda()
    qv = torch.randn(H, B * T, 64, generator=g).to(torch.bfloat16).cuda()
    lens = torch.tensor(lens_list, dtype=torch.int32, device="cuda") if ragged else None

    part_old, dpk_old = run(capi, 0, ds, qv, lens, B, T, H, causal)
    part_new, dpk_new = run(capi, 1, ds, qv, lens, B, T, H, causal)
    part_again, dpk_again = run(capi, 1, ds, qv, lens, B, T, H, causal)
    assert torch.equal(part_new, part_old), "partial planes differ from dpk_body's"
    assert torch.equal(dpk_new.view(torch.int16), dpk_old.view(torch.int16)), "d(pk) differs from dpk_body's"
    assert torch.equal(part_again, part_new) and torch.equal(dpk_again.view(torch.int16), dpk_new.view(torch.int16)), "not run-to-run identical"

    ref, mag = float64_sums(torch.nan_to_num(ds.float(), nan=0.0), qv, allowed, B, T, H)
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -11 * mag
    worst = {}
    for name, got in (("new", dpk_new), ("old", dpk_old)):
        assert torch.isfinite(got.float()).all(), name
        err = (got.double() - ref).abs()
        live = bound > 0
        worst[name] = float((err[live] / bound[live]).max()) if live.any() else 0.0
        assert torch.all(got.float()[~live] == 0), f"{name}: a band row no (query, key) pair reaches is not exactly zero"
    print(f"d(pk) B={B} H={H} T={T} causal={causal}: worst |out - ref| / bound: new {worst['new']:.3f} old {worst['old']:.3f} (bound 1)")
    assert worst["new"] <= 1.0 and worst["old"] <= 1.0
