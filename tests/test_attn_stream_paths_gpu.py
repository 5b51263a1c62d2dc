"""The streaming relative-position attention kernels (csrc/stream.hip), path by path and push by push, against the float64 reference
(tests/helpers/attn_stream_ref.py). Every call goes through the C-ABI (tsasr_relpos_attn_stream_fwd), so the test owns every buffer:
`out` starts as NaN and the workspace as 0xFF bytes before every push, the K / V caches as NaN before the first, and the cache is longer
than the frames pushed. After every push the cache rows pushed so far equal the K and V parts of qkv bit for bit and the rows behind
them still hold the poison; after the last push the output is checked globally, per row and structurally.

The host picks the kernels by dtype, head size and stream_split(B, C, H, Tmax):

    f32    / f32_split      attn_stream_kernel<float>      (+ attn_stream_merge_kernel<float>)     fp32; Dh 36 and 64
    mfma64 / mfma64_split   attn_stream_mfma_kernel<64>    (+ attn_stream_merge_kernel<bf16>)      bf16, Dh 64
    mfma32 / mfma32_split   attn_stream_mfma_kernel<32>    (+ merge)                               bf16, Dh 32
    bf16s  / bf16s_split    attn_stream_kernel<bf16>       (+ merge)                               bf16, Dh 36 and 16
    *_nows                  the split shape called with workspace = NULL: one pass over the keys

Shapes (H = 2): unsplit Tmax 200 with 170 frames pushed (three 64-key tiles, the last ragged, 30 poisoned rows never touched), lengths
full / one past a tile edge / on a tile edge / none; split Tmax 330 (6 tiles: 3 splits of 2) with 300 frames pushed, lengths full / inside
the last split piece that holds keys / one. Early pushes leave the later splits without a key."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_stream_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
H = 2

MIX = (7, 40, 1, 16, 64, 33, 17, 65, 15, 31, 100)   # C = 1, around the 16-row, 32- and 64-query blocks, two query groups, seams off 32
P40 = (40,)                                         # the product's push
M8 = (8, 40, 16, 64, 24)                            # multiples of 8 for block-causal 8
SCHED = {"MIX": MIX, "P40": P40, "M8": M8}

UNSPLIT = dict(B=4, Tmax=200, T=170, lens=(170, 129, 64, 0))
SPLIT = dict(B=3, Tmax=330, T=300, lens=(300, 193, 1))
COMBOS = ((F32, 36), (F32, 64), (BF16, 64), (BF16, 32), (BF16, 36), (BF16, 16))
PATHS = {f + s for f in ("f32", "mfma64", "mfma32", "bf16s") for s in ("", "_split", "_nows")}

# (shape, causal, schedule, ragged lens, kind, workspace)
UNSPLIT_CASES = [("unsplit", 1, "MIX", True, "o1", True), ("unsplit", 8, "M8", True, "o1", True), ("unsplit", 8, "MIX", False, "o1", True),
                 ("unsplit", 0, "MIX", True, "o1", True), ("unsplit", 1, "P40", True, "peaked", True)]
SPLIT_CASES = [("split", 1, "MIX", True, "o1", True), ("split", 40, "P40", False, "o1", True), ("split", 1, "MIX", True, "peaked", True),
               ("split", 1, "MIX", True, "o1", False)]
CASES = [(dt, Dh) + c for dt, Dh in COMBOS for c in UNSPLIT_CASES + SPLIT_CASES]


def case_id(c):
    dt, Dh, shape, causal, sched, ragged, kind, ws = c
    return f"{'bf16' if dt == BF16 else 'f32'}-Dh{Dh}-{shape}-c{causal}-{sched}-{'ragged' if ragged else 'full'}-{kind}" + ("" if ws else "-nows")


def path_name(dtype, Dh, B, Tmax, pushes, ws):
    fam = "f32" if dtype == F32 else {64: "mfma64", 32: "mfma32"}.get(Dh, "bf16s")
    split = {SR.stream_split(B, C, H, Tmax)[0] > 1 for _, C in pushes}
    assert len(split) == 1, "a schedule that mixes split and unsplit launches"
    return fam + (("_split" if ws else "_nows") if split.pop() else "")


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("ts-asr_amd._capi")


def ibits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def run_stream(C, qkv, pkh, u, v, lens, scale, causal, pushes, Tmax, dtype, use_ws=True, check_cache=True):
    """Push by push through the C-ABI -> (out [B,T,D] on the CPU, whether any launch had a workspace)."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    Dh = D // H
    qkv, pkh = qkv.to(DEV).to(dtype), pkh.to(DEV).to(dtype).contiguous()
    u, v = u.to(DEV), v.to(DEV)
    klen = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    nan = float("nan")
    kc = torch.full((B, H, Tmax, Dh), nan, dtype=dtype, device=DEV)
    vc = torch.full((B, H, Tmax, Dh), nan, dtype=dtype, device=DEV)
    poison = int(ibits(kc)[0, 0, 0, 0])
    q5 = qkv.view(B, T, H, 3, Dh)
    kbits, vbits = ibits(q5[:, :, :, 1].transpose(1, 2).contiguous()), ibits(q5[:, :, :, 2].transpose(1, 2).contiguous())   # [B,H,T,Dh]
    outs, any_ws = [], False
    for t0, Cn in pushes:
        ns, tps = SR.stream_split(B, Cn, H, Tmax)
        n = C.lib().tsasr_relpos_attn_stream_workspace_bytes(B, Cn, H, Dh, Tmax)
        assert n == (B * H * Cn * ns * (Dh + 2) * 4 if ns > 1 else 0), (n, ns, tps)
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV) if n and use_ws else None
        any_ws |= ws is not None
        chunk = qkv[:, t0:t0 + Cn].contiguous()
        out = torch.full((B, Cn, D), nan, dtype=dtype, device=DEV)
        C.check(C.lib().tsasr_relpos_attn_stream_fwd(C.ptr(chunk), C.ptr(kc), C.ptr(vc), C.ptr(pkh), C.ptr(u), C.ptr(v), C.ptr(klen), C.ptr(out),
                                                     B, Cn, H, Dh, Tmax, t0, causal, scale, C.io_dtype(chunk), C.ptr(ws),
                                                     0 if ws is None else n, C.stream_ptr()), "tsasr_relpos_attn_stream_fwd")
        outs.append(out)
        if check_cache:
            e = t0 + Cn
            assert torch.equal(ibits(kc)[:, :, :e], kbits[:, :, :e]) and torch.equal(ibits(vc)[:, :, :e], vbits[:, :, :e]), \
                f"cache rows [0, {e}) after the push at {t0}"
            assert bool((ibits(kc)[:, :, e:] == poison).all()) and bool((ibits(vc)[:, :, e:] == poison).all()), \
                f"cache rows [{e}, {Tmax}) touched by the push at {t0}"
    torch.cuda.synchronize()
    return torch.cat(outs, 1).cpu(), any_ws


_REF = {}


def reference(shape, Dh, causal, sched, ragged, kind):
    """Shared between the dtypes (and the workspace / no-workspace cases) of a shape: both store the same bf16-representable values."""
    key = (shape, Dh, causal, sched, ragged, kind)
    if key not in _REF:
        s = UNSPLIT if shape == "unsplit" else SPLIT
        args = SR.inputs(s["B"], s["T"], H, Dh, s["Tmax"], kind)
        pushes = SR.schedule(SCHED[sched], s["T"])
        allowed = SR.allowed(pushes, s["lens"] if ragged else None, causal, s["B"])
        _REF[key] = args, pushes, allowed, SR.reference(*args[:4], H, args[4], allowed)
    return _REF[key]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_attn_stream_path_vs_float64(capi, case):
    dtype, Dh, shape, causal, sched, ragged, kind, use_ws = case
    s = UNSPLIT if shape == "unsplit" else SPLIT
    B, T, Tmax, lens = s["B"], s["T"], s["Tmax"], s["lens"] if ragged else None
    (qkv, pkh, u, v, scale), pushes, allowed, ref = reference(shape, Dh, causal, sched, ragged, kind)
    path = path_name(dtype, Dh, B, Tmax, pushes, use_ws)
    assert path in PATHS and path.partition("_")[2] == {"unsplit": "", "split": "split" if use_ws else "nows"}[shape], path
    got, any_ws = run_stream(capi, qkv, pkh, u, v, lens, scale, causal, pushes, Tmax, dtype, use_ws)
    assert any_ws == path.endswith("_split")
    errs, bad = SR.measure(got, ref, allowed, B, T, H, Dh)
    g, r = errs["out"]
    print(f"ATTN-STREAM-ERR path={path} kind={kind} {case_id(case)} out={g:.3g}/{r:.3g} worst(b,i,h)={SR.worst_row(got, ref, allowed, B, T, H, Dh)}")
    fails = SR.failures(errs, bad, SR.TOL[(path, kind)])
    assert not fails, fails
    if shape == "split":      # no atomics anywhere: a second run from fresh caches gives the same bits
        again, _ = run_stream(capi, qkv, pkh, u, v, lens, scale, causal, pushes, Tmax, dtype, use_ws, check_cache=False)
        assert torch.equal(ibits(again), ibits(got))


def test_every_path_is_hit():
    hit = set()
    for dt, Dh, shape, causal, sched, ragged, kind, ws in CASES:
        s = UNSPLIT if shape == "unsplit" else SPLIT
        hit.add(path_name(dt, Dh, s["B"], s["Tmax"], SR.schedule(SCHED[sched], s["T"]), ws))
    assert hit == PATHS
    assert {p for p, _ in SR.TOL} == PATHS


def test_ops_wrapper_same_bits_and_argument_checks(capi):
    ops = importlib.import_module("ts-asr_amd.ops")
    B, T, Tmax, lens, Dh = SPLIT["B"], SPLIT["T"], SPLIT["Tmax"], SPLIT["lens"], 64
    (qkv, pkh, u, v, scale), pushes, allowed, ref = reference("split", Dh, 1, "MIX", True, "o1")
    direct, _ = run_stream(capi, qkv, pkh, u, v, lens, scale, 1, pushes, Tmax, BF16)
    qd, td, ud, vd = qkv.to(DEV).to(BF16), pkh.to(DEV).to(BF16), u.to(DEV), v.to(DEV)
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kc = torch.full((B, H, Tmax, Dh), float("nan"), dtype=BF16, device=DEV)
    vc = torch.full_like(kc, float("nan"))
    outs = []
    with torch.no_grad():
        for t0, Cn in pushes:
            ws = ops.relpos_attn_stream_workspace(B, Cn, H, Dh, Tmax, DEV)
            assert ws is not None
            outs.append(ops.relpos_attention_stream(qd[:, t0:t0 + Cn], kc, vc, td, ud, vd, kl, H, scale, 1, t0, ws))
        assert torch.equal(ibits(torch.cat(outs, 1).cpu()), ibits(direct))
        chunk = qd[:, :40]
        with pytest.raises(ValueError):
            ops.relpos_attention_stream(chunk, kc, vc, td, ud, vd, kl, H, scale, 1, Tmax - 39)          # t0 + C > Tmax
        with pytest.raises(ValueError):
            ops.relpos_attention_stream(chunk, kc.float(), vc.float(), td, ud, vd, kl, H, scale, 1, 0)  # cache dtype != qkv's
        with pytest.raises(ValueError):
            ops.relpos_attention_stream(chunk, kc, vc, td[:Tmax - 1], ud, vd, kl, H, scale, 1, 0)       # table shorter than the cache
        D72 = H * 72
        big = torch.zeros(B, 40, 3 * D72, dtype=BF16, device=DEV)
        c72 = torch.zeros(B, H, Tmax, 72, dtype=BF16, device=DEV)
        with pytest.raises(capi.TsasrHipError):                                                        # the ABI's shape check: Dh <= 64
            ops.relpos_attention_stream(big, c72, c72.clone(), torch.zeros(Tmax, D72, dtype=BF16, device=DEV), torch.zeros(D72, device=DEV),
                                        torch.zeros(D72, device=DEV), kl, H, scale, 1, 0)
        assert not bool(c72.any())
    with torch.enable_grad(), pytest.raises(RuntimeError):
        ops.relpos_attention_stream(qd[:, :40], kc, vc, td, ud, vd, kl, H, scale, 1, 0)
