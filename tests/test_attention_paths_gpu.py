"""The bf16 relative-position attention kernels (csrc/attention.hip, csrc/attention_short.hip), path by path, against the float64 reference
with dropout (tests/helpers/attn_ref.py). Every call goes through the C-ABI (tsasr_relpos_attn_fwd_ws + tsasr_relpos_attn_bwd, seed_dev =
NULL so that the dropout stream's seed is the argument); every output starts as NaN (both entries write all of theirs); every case checks
out, lse, dQ / dK / dV, d(pk) and d pos_bias u / v globally, per row and structurally.

The host picks the kernels by shape (launch rules mirrored by fwd_path / bwd_path below; the test asserts what the ABI shows of them: the
forward workspace of the split shapes):

    fwd short64       relpos_attn_fwd_short2_kernel<64>           bf16, Dh = 64, 2 <= T <= 128
    fwd short128      relpos_attn_fwd_short2_kernel<128>          bf16, Dh = 64, 129 <= T <= 256
    fwd stream        relpos_attn_fwd_kernel<T>                   otherwise, one key part
    fwd chunk         relpos_attn_fwd_chunk_kernel + relpos_attn_merge_kernel<bf16>      bf16, Dh = 64, key parts (T > 512, small B*H)
    fwd stream_split  relpos_attn_fwd_kernel<T> + relpos_attn_merge_kernel<T>            key parts otherwise
    bwd short         relpos_attn_bwd_q_short_kernel + relpos_attn_bwd_kv_short_kernel (attn_zero_kernel when causal)
    bwd stream        relpos_attn_bwd_q_kernel + relpos_attn_bwd_kv2_kernel (attn_zero_band_kernel when causal)
    bwd split         ... + relpos_attn_dq_merge_kernel           key parts
    bwd split_ks4     ... + relpos_attn_kv_merge_kernel           key parts and T > 3584 (the key-major pass in four parts)
    every bwd         relpos_dpk_kernel + dpk_reduce_kernel       (utterance groups when attn_bgroup > 1, query ranges when isplit > 1)

Bounds (attn_ref.TOL, per path, io dtype and dropout) come from the bf16 error budget - probabilities and dS rounded to bf16 into the
MFMAs, positional products crossing LDS as fp16 in the short and chunk kernels, q + u / q + v rounded to bf16, bf16 outputs - and were
confirmed on the MI355X: the measured worst value of each path stands next to its bound."""
import importlib
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SEED = 0x5EED1234


# ---------------------------------------------------------------------------------------------- the host's launch rules (csrc/attention.hip)
def cdiv(a, b):
    return -(-a // b)


def host_limit(i, causal):
    return i if causal <= 1 else (i // causal + 1) * causal - 1


def key_parts(B, T, H, causal, cus):
    """attn_key_parts: key parts of the streaming forward / query-major backward (1: unsplit)."""
    tiles, nqb = cdiv(T, 64), cdiv(T, 128)
    if tiles <= 8 or B * H * nqb >= cus:
        return 1
    per = 8
    while per < tiles:
        ends = [min(T, host_limit(qb * 128 + 127, causal) + 1) if causal else T for qb in range(nqb)]
        if sum(cdiv(cdiv(je, 64), per) for je in ends) * B * H <= cus:
            break
        per += 1
    return 1 if per >= tiles else cdiv(tiles, per)


def fwd_path(B, T, H, Dh, dtype, causal, cus):
    if dtype == BF16 and Dh == 64 and 2 <= T <= 256:
        return "short64" if T <= 128 else "short128"
    if key_parts(B, T, H, causal, cus) > 1:
        return "chunk" if dtype == BF16 and Dh == 64 else "stream_split"
    return "stream"


def bwd_path(B, T, H, Dh, dtype, causal, cus):
    np_ = key_parts(B, T, H, causal, cus)
    if dtype == BF16 and Dh == 64 and 2 <= T <= 256 and np_ == 1:
        return "short"
    if np_ > 1:
        return "split_ks4" if cdiv(cdiv(T, 64), 8) >= 8 else "split"
    return "stream"


def bgroup(B, T):
    want = max(1, 256 // (4 * cdiv(2 * T - 1, 64)))
    return max(1, cdiv(B, min(B, want)))


def dpk_isplit(B, T, H, causal):
    """attn_dpk_isplit capped by attn_dpk_max_isplit: query ranges of the d(pk) pass."""
    G, nib = cdiv(B, bgroup(B, T)), cdiv(T, 64)
    live = cdiv(T + max(causal, 1) if causal else 2 * T - 1, 64) * H * G
    return 1 if live >= 1024 or nib < 16 else min(cdiv(1024, live), nib // 8, 16)


# ---------------------------------------------------------------------------------------------- the matrix
def lens_pool(T, C):
    """Key lengths of one batch: full, 1, 2, on and one past every 32 / 64 / 128 / 256 boundary, C - 1 / C / C + 1 under a block-causal
    mask, and lengths that leave a whole trailing 64-key tile (and 128-key tile of the padded short kernels) masked."""
    c = {T, 1, 2}
    for b in (32, 64, 128, 256):
        c |= {b, b + 1}
    if C > 1:
        c |= {C - 1, C, C + 1}
    c |= {(cdiv(T, 64) - 1) * 64 - 5, (cdiv(T, 128) - 1) * 128 - 3}
    return tuple(sorted(x for x in c if 1 <= x <= T))


def short_cases():
    out = []
    for T in (2, 31, 33, 64, 65, 128, 129, 250, 255, 256):
        for C in sorted({0, 1, 40, 7, 64, T}):
            for p in (0.0, 0.1):
                out.append((len(lens_pool(T, C)), T, 2, 64, lens_pool(T, C), C, p, BF16))
    return out


def stream_cases():
    out = []
    for T, Dh in ((257, 64), (333, 64), (2, 36), (33, 36), (65, 36), (129, 36), (256, 36), (257, 36), (333, 36)):
        for C in (0, 1, 40):
            for p in (0.0, 0.1):
                out.append((len(lens_pool(T, C)), T, 2, Dh, lens_pool(T, C), C, p, BF16))
    return out


LONG = [  # (B, T, H, Dh, lens, causal, p, dtype)
    # forward in 256-key chunks + merge; backward key parts + dQ merge, d(pk) in 2 query ranges and 1 group of 2 utterances
    *[(2, 1100, 1, 64, (1100, 769), C, p, BF16) for C in (0, 1, 40) for p in (0.0, 0.1)],
    (2, 1100, 1, 64, (768, 513), 40, 0.1, BF16),
    # streaming forward in key parts + merge (Dh = 36); backward key parts + dQ merge
    *[(2, 777, 2, 36, (777, 513), C, p, BF16) for C in (0, 1, 40) for p in (0.0, 0.1)],
    # key-major pass in four parts + merge (T > 3584), d(pk) in 7 query ranges
    (1, 3600, 1, 64, (3600,), 0, 0.0, BF16), (1, 3600, 1, 64, (3600,), 1, 0.1, BF16), (1, 3600, 1, 64, (3329,), 40, 0.0, BF16),
    (1, 3600, 1, 36, (3600,), 40, 0.1, BF16),
    # d(pk) in utterance groups at the training length (attn_bgroup = 2; a last group of one)
    (9, 250, 2, 64, (250, 249, 200, 129, 128, 65, 64, 33, 1), 40, 0.1, BF16),
    (9, 250, 2, 64, (250, 249, 200, 129, 128, 65, 64, 33, 1), 0, 0.0, BF16),
    (9, 250, 1, 36, (250, 249, 200, 129, 128, 65, 64, 33, 1), 1, 0.1, BF16),
]

F32_CASES = [  # the float instantiation of the same MFMA kernels (io_dtype F32 with the exact-fp32 kernels bypassed)
    (3, 129, 2, 64, (129, 128, 33), 0, 0.1, F32), (3, 129, 2, 64, (129, 128, 33), 40, 0.0, F32),
    (4, 65, 2, 36, (65, 64, 7, 1), 7, 0.1, F32), (2, 333, 2, 64, (333, 257), 1, 0.0, F32),
    (2, 1100, 1, 64, (1100, 769), 1, 0.1, F32), (2, 1100, 1, 64, (1100, 769), 40, 0.0, F32),
]

CASES = short_cases() + stream_cases() + LONG + F32_CASES


def case_id(c):
    B, T, H, Dh, lens, C, p, dt = c
    return f"B{B}-T{T}-H{H}-Dh{Dh}-C{C}-p{p}-{'bf16' if dt == BF16 else 'f32'}" + ("" if lens == lens_pool(T, C) else "-L" + "_".join(map(str, lens)))


# ---------------------------------------------------------------------------------------------- inputs, kernel call, reference
@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("ts-asr_amd._capi")


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def inputs(B, T, H, Dh, dtype):
    """Scores of O(1) after scaling (the scale of a trained model's), pos_bias of 0.3, a random upstream gradient."""
    D = H * Dh
    g = torch.Generator().manual_seed(T * 131 + Dh * 7 + B * H)
    qkv = torch.randn(B, T, 3 * D, generator=g).to(dtype)
    pk = torch.randn(2 * T - 1, D, generator=g).to(dtype)
    u, v = torch.randn(D, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
    dout = torch.randn(B, T, D, generator=g).to(dtype)
    return qkv, pk, u, v, dout, 1.0 / math.sqrt(D)


def run_kernels(C, qkv, pk, u, v, dout, lens, H, scale, causal, p, seed):
    B, T, D3 = qkv.shape
    D = D3 // 3
    Dh = D // H
    qkv, pk, u, v, dout = (t.to(DEV) for t in (qkv, pk, u, v, dout))
    klen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    nan = float("nan")
    out = torch.full((B, T, D), nan, dtype=qkv.dtype, device=DEV)
    lse = torch.full((B, H, T), nan, dtype=torch.float32, device=DEV)
    nf = C.lib().tsasr_relpos_attn_fwd_workspace_bytes(B, T, H)
    wsf = torch.full((nf,), 0xFF, dtype=torch.uint8, device=DEV) if nf else None
    C.check(C.lib().tsasr_relpos_attn_fwd_ws(C.ptr(qkv), C.ptr(pk), C.ptr(u), C.ptr(v), C.ptr(klen), C.ptr(out), C.ptr(lse), B, T, H, Dh, scale,
                                             causal, p, seed, None, C.io_dtype(qkv), C.ptr(wsf), nf, C.stream_ptr()), "fwd")
    dqkv, dpk = torch.full_like(qkv, nan), torch.full_like(pk, nan)
    du, dv = torch.full_like(u, nan), torch.full_like(v, nan)
    nb = C.lib().tsasr_relpos_attn_bwd_workspace_bytes(B, T, H)
    wsb = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
    C.check(C.lib().tsasr_relpos_attn_bwd(C.ptr(qkv), C.ptr(pk), C.ptr(u), C.ptr(v), C.ptr(klen), C.ptr(out), C.ptr(dout), C.ptr(lse), C.ptr(dqkv),
                                          C.ptr(dpk), C.ptr(du), C.ptr(dv), B, T, H, Dh, scale, causal, p, seed, None, C.io_dtype(qkv), C.ptr(wsb), nb,
                                          C.stream_ptr()), "bwd")
    torch.cuda.synchronize()
    return nf, {k: t.cpu() for k, t in zip(("out", "lse", "dqkv", "dpk", "du", "dv"), (out, lse, dqkv, dpk, du, dv))}


_REF = {}


def reference(B, T, H, Dh, lens, causal, p, dtype):
    """Shared between the dtypes of a shape (the fp32 cases store the same bf16-representable values). C >= T masks nothing: the case is
    checked against the unmasked reference."""
    eff = 0 if causal >= T else causal
    key = (B, T, H, Dh, lens, eff, p)
    if key not in _REF:
        if len(_REF) > 8:
            _REF.clear()
        qkv, pk, u, v, dout, scale = inputs(B, T, H, Dh, BF16)
        allowed = AR.allowed_mask(T, lens, eff)
        _REF[key] = allowed, AR.reference(qkv, pk, u, v, dout, H, scale, allowed, AR.keep_mask(B, H, T, p, SEED), p)
    return _REF[key]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_attention_path_vs_float64(capi, cus, case):
    B, T, H, Dh, lens, causal, p, dtype = case
    fp, bp = fwd_path(B, T, H, Dh, dtype, causal, cus), bwd_path(B, T, H, Dh, dtype, causal, cus)
    qkv, pk, u, v, dout, scale = inputs(B, T, H, Dh, BF16)
    nf, got = run_kernels(capi, qkv.to(dtype), pk.to(dtype), u, v, dout.to(dtype), lens, H, scale, causal, p, SEED)
    if fp in ("chunk", "stream_split"):
        assert nf > 0, "a split shape without a forward workspace"
    elif fp.startswith("short"):
        assert capi.lib().tsasr_relpos_attn_keepbits_bytes(B, T, H) > 0
    allowed, ref = reference(B, T, H, Dh, lens, causal, p, dtype)
    errs, bad = AR.measure(got, ref, allowed, B, T, H, Dh)
    tag = "bf16" if dtype == BF16 else "f32"
    tol = {**AR.TOL[("fwd", fp, tag, p > 0)], **AR.TOL[("bwd", bp, tag, p > 0)]}
    print(f"ATTN-ERR fwd={fp} bwd={bp} {tag} bg={bgroup(B, T)} isplit={dpk_isplit(B, T, H, causal)} {case_id(case)} "
          + " ".join(f"{k}={g:.3g}/{r:.3g}" for k, (g, r) in errs.items()))
    fails = AR.failures(errs, bad, tol)
    assert not fails, fails
