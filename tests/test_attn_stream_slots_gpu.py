"""tsasr_relpos_attn_stream_slots_fwd (csrc/stream.hip) through the C-ABI: four slots at different offsets of their own sessions, one
idle, on every kernel path (attn_stream_ref.CEIL's names) unsplit, split and with a NULL workspace.

Per case: slot b's cache holds its own session's K / V in rows < t0s[b] and NaN everywhere else, `out` starts as NaN, the workspace as
0xFF. (1) For each distinct offset k the existing scalar entry point at t0 = k on cloned buffers (same B, C, Tmax: same split) gives the
bits of the slots at k, out rows and cache planes. (2) Against the float64 slot model (stream_slots_ref) within attn_stream_ref.CEIL,
globally, per row and structurally. (3) Cache rows t0s[b] .. t0s[b]+C-1 equal qkv's K / V bits, every other row of every slot keeps its
bits, the idle slot's planes are untouched and its out rows exact zeros. (4) A second launch that admits the idle slot at 0 and
advances the others by C continues against the float64 schedule; the slot whose offset reached Tmax is idled by the kernel's guard."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_stream_ref as SR  # noqa: E402
import stream_slots_ref as SS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
B, H = 4, 2
PATHS = {"f32": (F32, 16), "mfma64": (BF16, 64), "mfma32": (BF16, 32), "bf16s": (BF16, 16)}
CONFIGS = {"unsplit": (192, True), "split": (384, True), "nows": (384, False)}       # Tmax, pass the workspace
CHUNKS = [(1, 1), (7, 1), (40, 1), (70, 1), (40, 4)]                                   # (C, causal)
CASES = [(p, c, C, causal) for p in PATHS for c in CONFIGS for C, causal in CHUNKS]


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("ts-asr_amd._capi")


def ibits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def offsets(Tmax, C, causal):
    return [0, 37, Tmax - C, -1] if causal == 1 else [0, 36, (Tmax - C) // 4 * 4, -1]


_REF = {}


def reference(Dh, Tmax, C, causal):
    """The float64 schedule of a case, shared by the dtypes and by the split / NULL-workspace configurations of a shape:
    (inputs, [(t0s, key_lens, chunk [B,C,3D], ref out [B,C,D], live rows [B,C])] of the two launches)."""
    key = (Dh, Tmax, C, causal)
    if key not in _REF:
        qkv, pkh, u, v, scale = SR.inputs(B, Tmax, H, Dh, Tmax)
        m = SS.Slots(B, H, Dh, Tmax, pkh, u, v, scale, causal)
        t0s = offsets(Tmax, C, causal)
        q5 = qkv.double().view(B, Tmax, H, 3, Dh)
        for b, t0 in enumerate(t0s):                  # each slot's cache: its own session's rows < t0
            if t0 > 0:
                m.kc[b, :, :t0], m.vc[b, :, :t0] = q5[b, :t0, :, 1].transpose(0, 1), q5[b, :t0, :, 2].transpose(0, 1)
            m.t0[b] = max(t0, 0)
        launches = []
        # slot 0 shorter than its chunk end, slot 1 shorter than its own offset (an ended stream), slot 2 full; then slot 3 enters
        for lens, t0s_n in (([C - 1, 20, Tmax, 5], t0s), ([2 * C - 1, 20, Tmax, C], None)):
            if t0s_n is None:                         # the idle slot is admitted at 0, the others advance by C (slot 2 reaches Tmax)
                m.admit(3)
                t0s_n = [m.t0[0], m.t0[1], m.t0[2], 0]
            active = [0 <= t and t + C <= Tmax for t in t0s_n]
            chunk = torch.stack([qkv[b, max(t, 0):max(t, 0) + C] if active[b] else qkv[b, :C] for b, t in enumerate(t0s_n)])
            kmax = torch.tensor([min(ln, max(t, 0) + C) for ln, t in zip(lens, t0s_n)])[:, None]
            live = torch.tensor(active)[:, None] & (kmax > 0) & torch.ones(B, C, dtype=torch.bool)     # causal: key 0 is always in reach
            out, _ = m.push(chunk.double(), None, active, lens)
            launches.append((list(t0s_n), lens, chunk, out, live))
        assert launches[1][0][2] == Tmax and m.t0 == [2 * C, launches[0][0][1] + 2 * C, Tmax, C]
        _REF[key] = (qkv, pkh, u, v, scale), launches
    return _REF[key]


def call(capi, name, chunk, kc, vc, pkh, u, v, klen, out, C, Dh, Tmax, t0, causal, scale, ws):
    n = 0 if ws is None else ws.numel()
    t0_arg = capi.ptr(t0) if t0 is None or isinstance(t0, torch.Tensor) else int(t0)
    capi.check(getattr(capi.lib(), name)(capi.ptr(chunk), capi.ptr(kc), capi.ptr(vc), capi.ptr(pkh), capi.ptr(u), capi.ptr(v), capi.ptr(klen),
                                         capi.ptr(out), B, C, H, Dh, Tmax, t0_arg, causal, scale, capi.io_dtype(chunk), capi.ptr(ws), n,
                                         capi.stream_ptr()), name)


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c[:3])) + f"-c{c[3]}" for c in CASES])
def test_slots_launch(capi, case):
    path, config, C, causal = case
    dtype, Dh = PATHS[path]
    Tmax, use_ws = CONFIGS[config]
    D = H * Dh
    (qkv, pkh, u, v, scale), launches = reference(Dh, Tmax, C, causal)
    ns, _ = SR.stream_split(B, C, H, Tmax)
    need = capi.lib().tsasr_relpos_attn_stream_workspace_bytes(B, C, H, Dh, Tmax)
    assert (ns, need) == ((1, 0) if config == "unsplit" else (3, B * H * C * 3 * (Dh + 2) * 4)), (ns, need)
    nan = float("nan")
    qd, pd, ud, vd = qkv.to(DEV).to(dtype), pkh.to(DEV).to(dtype).contiguous(), u.to(DEV), v.to(DEV)
    q5 = qd.view(B, Tmax, H, 3, Dh)
    kc = torch.full((B, H, Tmax, Dh), nan, dtype=dtype, device=DEV)
    vc = torch.full_like(kc, nan)
    for b, t0 in enumerate(launches[0][0]):
        if t0 > 0:
            kc[b, :, :t0], vc[b, :, :t0] = q5[b, :t0, :, 1].transpose(0, 1), q5[b, :t0, :, 2].transpose(0, 1)
    for n, (t0s, lens, chunk, ref, live) in enumerate(launches):
        chunk = chunk.to(DEV).to(dtype).contiguous()
        klen = torch.tensor(lens, dtype=torch.int32, device=DEV)
        t0d = torch.tensor(t0s, dtype=torch.int32, device=DEV)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV) if need and use_ws else None
        out = torch.full((B, C, D), nan, dtype=dtype, device=DEV)
        kc0, vc0 = kc.clone(), vc.clone()
        call(capi, "tsasr_relpos_attn_stream_slots_fwd", chunk, kc, vc, pd, ud, vd, klen, out, C, Dh, Tmax, t0d, causal, scale, ws)
        torch.cuda.synchronize()
        active = [0 <= t and t + C <= Tmax for t in t0s]
        # (1) the scalar entry point at each distinct offset, on cloned buffers
        for k in sorted({t for t, a in zip(t0s, active) if a}):
            kc1, vc1 = kc0.clone(), vc0.clone()
            out1 = torch.full((B, C, D), nan, dtype=dtype, device=DEV)
            ws1 = None if ws is None else torch.full_like(ws, 0xFF)
            call(capi, "tsasr_relpos_attn_stream_fwd", chunk, kc1, vc1, pd, ud, vd, klen, out1, C, Dh, Tmax, k, causal, scale, ws1)
            for b in [b for b, t in enumerate(t0s) if t == k]:
                assert torch.equal(ibits(out[b]), ibits(out1[b])), f"launch {n} slot {b}: out bits differ from the scalar launch at {k}"
                assert torch.equal(ibits(kc[b]), ibits(kc1[b])) and torch.equal(ibits(vc[b]), ibits(vc1[b])), f"launch {n} slot {b}: cache"
        # (3) the caches
        cb = chunk.view(B, C, H, 3, Dh)
        for b, t0 in enumerate(t0s):
            if not active[b]:
                assert torch.equal(ibits(kc[b]), ibits(kc0[b])) and torch.equal(ibits(vc[b]), ibits(vc0[b])), f"launch {n}: idle slot {b}'s cache"
                assert bool((ibits(out[b]) == 0).all()), f"launch {n}: idle slot {b}'s out rows are not exact zeros"
                continue
            assert torch.equal(ibits(kc[b, :, t0:t0 + C]), ibits(cb[b, :, :, 1].transpose(0, 1).contiguous())), f"launch {n} slot {b}: K rows"
            assert torch.equal(ibits(vc[b, :, t0:t0 + C]), ibits(cb[b, :, :, 2].transpose(0, 1).contiguous())), f"launch {n} slot {b}: V rows"
            for pl, pl0 in ((kc, kc0), (vc, vc0)):
                assert torch.equal(ibits(pl[b, :, :t0]), ibits(pl0[b, :, :t0])) and torch.equal(ibits(pl[b, :, t0 + C:]), ibits(pl0[b, :, t0 + C:])), \
                    f"launch {n} slot {b}: a cache row outside the chunk moved"
        # (2) / (4) against the float64 schedule
        allowed = live[:, :, None]
        errs, bad = SR.measure(out.cpu(), ref, allowed, B, C, H, Dh)
        g, r = errs["out"]
        print(f"ATTN-SLOTS-ERR path={path} config={config} C={C} causal={causal} launch={n} t0s={t0s} out={g:.3g}/{r:.3g}")
        fails = SR.failures(errs, bad, {"out": SR.CEIL[path]})
        assert not fails, (n, fails)


def test_ops_wrapper_same_bits_and_argument_checks(capi):
    ops = importlib.import_module("ts-asr_amd.ops")
    Dh, Tmax, C = 32, 384, 40
    (qkv, pkh, u, v, scale), launches = reference(Dh, Tmax, C, 1)
    t0s, lens, chunk, _, _ = launches[0]
    qd, pd, ud, vd = qkv.to(DEV).to(BF16), pkh.to(DEV).to(BF16).contiguous(), u.to(DEV), v.to(DEV)
    q5 = qd.view(B, Tmax, H, 3, Dh)
    kc = torch.full((B, H, Tmax, Dh), float("nan"), dtype=BF16, device=DEV)
    vc = torch.full_like(kc, float("nan"))
    for b, t0 in enumerate(t0s):
        if t0 > 0:
            kc[b, :, :t0], vc[b, :, :t0] = q5[b, :t0, :, 1].transpose(0, 1), q5[b, :t0, :, 2].transpose(0, 1)
    kc1, vc1 = kc.clone(), vc.clone()
    chunk = chunk.to(DEV).to(BF16).contiguous()
    klen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    t0d = torch.tensor(t0s, dtype=torch.int32, device=DEV)
    need = capi.lib().tsasr_relpos_attn_stream_workspace_bytes(B, C, H, Dh, Tmax)
    direct = torch.full((B, C, H * Dh), float("nan"), dtype=BF16, device=DEV)
    call(capi, "tsasr_relpos_attn_stream_slots_fwd", chunk, kc1, vc1, pd, ud, vd, klen, direct, C, Dh, Tmax, t0d, 1, scale,
         torch.empty(need, dtype=torch.uint8, device=DEV))
    with torch.no_grad():
        ws = ops.relpos_attn_stream_workspace(B, C, H, Dh, Tmax, DEV)
        assert ws is not None and ws.numel() == need
        got = ops.relpos_attention_stream(chunk, kc, vc, pd, ud, vd, klen, H, scale, 1, t0d, ws)
        assert torch.equal(ibits(got), ibits(direct)) and torch.equal(ibits(kc), ibits(kc1)) and torch.equal(ibits(vc), ibits(vc1))
        with pytest.raises(ValueError):
            ops.relpos_attention_stream(chunk, kc, vc, pd, ud, vd, klen, H, scale, 1, t0d.long(), ws)          # offsets must be int32
        with pytest.raises(ValueError):
            ops.relpos_attention_stream(chunk, kc, vc, pd, ud, vd, klen, H, scale, 1, t0d[:3].contiguous(), ws)  # one per slot
        with pytest.raises(capi.TsasrHipError):                                                                 # the ABI refuses a null array
            call(capi, "tsasr_relpos_attn_stream_slots_fwd", chunk, kc, vc, pd, ud, vd, klen, got, C, Dh, Tmax, None, 1, scale, ws)
