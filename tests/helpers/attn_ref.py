"""float64 reference of the relative-position attention core (oracle/tsasr_ref.relpos_core) WITH the kernels' attention dropout, and the
strict checker that tests/test_attention_paths_gpu.py applies to every kernel path and tests/test_attention_ref_cpu.py proves able to fail.
Test infrastructure only.

Reference: the inputs as stored (bf16 or fp32 values, pos_bias u / v fp32) promoted to float64; the keep mask from the numpy twin of the
dropout stream (attn_mask.keep_mask) and kept probabilities scaled by 65536 / (65536 - thr16), the kernels' quantised 1 / (1 - p). None of
the kernels' internal roundings (q + u, P, dS, fp16 G tiles, bf16 outputs) is emulated: they are the error budget the bounds stand for.

Checker, per tensor: (a) relative L2 over the whole tensor; (b) relative L2 per row - out / dQ per (b, query, h), dK / dV per (b, key, h),
dpk per relative row r, du / dv per head - over max(|ref row|, ROW_FLOOR x the RMS row norm of the tensor), so that rows the reference
makes tiny are judged against the tensor's scale; lse as an absolute error per (b, h, i); (c) structure: every output finite, and what the
mask makes exactly zero in the reference (dK / dV rows of keys no query may attend, dpk rows of relative distances no (query, key) pair has)
exactly zero in the kernel's result."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_mask  # noqa: E402

ROW_FLOOR = 0.1
NAMES = ("out", "lse", "dQ", "dK", "dV", "dpk", "du", "dv")


def causal_limit(T, causal):
    """int64 [T]: the last key query i may attend. 0: none (T - 1); 1: the look-ahead mask (i); C > 1: block-causal (end of i's chunk)."""
    i = torch.arange(T)
    if not causal:
        return torch.full((T,), T - 1, dtype=torch.long)
    return i if int(causal) <= 1 else (i // int(causal) + 1) * int(causal) - 1


def allowed_mask(T, lens, causal=0, limit=None):
    """bool [B, T, T]: query i of utterance b may attend key j (j < lens[b] and j <= limit[i])."""
    lens = torch.as_tensor(lens, dtype=torch.long)
    lim = causal_limit(T, causal) if limit is None else limit
    j = torch.arange(T)
    return (j[None, None, :] < lens[:, None, None]) & (j[None, None, :] <= lim[None, :, None])


def keep_mask(B, H, T, p, seed):
    return torch.from_numpy(attn_mask.keep_mask(B, H, T, p, seed)) if p > 0 else None


def keep_scale(p):
    thr = attn_mask.thr16(p)
    return 65536.0 / (65536 - thr) if thr else 1.0


def reference(qkv, pk, u, v, dout, H, scale, allowed, keep=None, p=0.0):
    """qkv [B,T,3D] (per-head interleaved Q|K|V), pk [2T-1,D], u / v [H*Dh], dout [B,T,D]; allowed bool [B,T,T]; keep bool [B,H,T,T] or
    None. -> dict of float64 CPU tensors: out [B,T,D], lse [B,H,T] (natural log of the sum of exp(scaled score) over the attended keys,
    before dropout), dqkv, dpk, du, dv (the gradients of <out, dout>)."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    Dh = D // H
    x, pkx, ux, vx = (t.detach().cpu().to(torch.float64).requires_grad_() for t in (qkv, pk, u, v))
    q, k, vv = (t.transpose(1, 2) for t in x.view(B, T, H, 3 * Dh).split(Dh, dim=-1))   # [B,H,T,Dh]
    uu, vb = ux.view(1, H, 1, Dh), vx.view(1, H, 1, Dh)
    ac = (q + uu) @ k.transpose(-1, -2)
    bd_raw = (q + vb) @ pkx.view(2 * T - 1, H, Dh).permute(1, 2, 0)                  # [B,H,T,2T-1]
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1                  # BD[i, j] = BDraw[i, j - i + T - 1]
    s = (ac + torch.gather(bd_raw, 3, idx.expand(B, H, T, T))) * scale
    del ac, bd_raw
    s = s.masked_fill(~allowed.view(B, 1, T, T), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    if keep is not None:
        P = P * (keep.to(torch.float64) * keep_scale(p))
    o = (P @ vv).transpose(1, 2).reshape(B, T, D)
    o.backward(dout.detach().cpu().to(torch.float64))
    return {"out": o.detach(), "lse": lse.detach(), "dqkv": x.grad, "dpk": pkx.grad, "du": ux.grad, "dv": vx.grad}


def rows(name, t, B, T, H, Dh):
    """The row view the per-row check uses for tensor `name` (see the module docstring)."""
    if name == "out":
        return t.reshape(B * T * H, Dh)
    if name in ("dQ", "dK", "dV"):
        return t.reshape(B, T, H, 3, Dh)[:, :, :, "dQ dK dV".split().index(name)].reshape(B * T * H, Dh)
    if name == "dpk":
        return t.reshape(2 * T - 1, H * Dh)
    if name in ("du", "dv"):
        return t.reshape(H, Dh)
    return t.reshape(-1, 1)     # lse


def dead_rows(name, allowed, B, T, H):
    """bool over the rows of rows(name): rows the mask makes exactly zero in the reference (None: no such rule for `name`)."""
    if name in ("dK", "dV"):
        key_dead = ~allowed.any(dim=1)                                                  # [B, T]: no query attends key j
        return key_dead[:, :, None].expand(B, T, H).reshape(-1)
    if name == "dpk":
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1
        alive = torch.zeros(2 * T - 1, dtype=torch.bool)
        alive[idx[allowed.any(dim=0)]] = True
        return ~alive
    return None


def split(res, B, T, H, Dh):
    """{out, lse, dqkv, dpk, du, dv} -> {NAMES}: dqkv cut into its Q, K, V parts (full tensors, for the row views above)."""
    out = {k: res[k] for k in ("out", "lse", "dpk", "du", "dv") if k in res}
    if "dqkv" in res:
        for n in ("dQ", "dK", "dV"):
            out[n] = res["dqkv"]
    return out


def measure(got, ref, allowed, B, T, H, Dh):
    """-> ({name: (global rel L2, worst per-row error)}, [structural failures]). got / ref: {out, lse, dqkv, dpk, du, dv} (any subset)."""
    g, r = split(got, B, T, H, Dh), split(ref, B, T, H, Dh)
    errs, bad = {}, []
    for name in NAMES:
        if name not in g:
            continue
        a = rows(name, g[name].detach().cpu().to(torch.float64), B, T, H, Dh)
        b = rows(name, r[name].to(torch.float64), B, T, H, Dh)
        if not torch.isfinite(a).all():
            bad.append(f"{name}: {int((~torch.isfinite(a)).sum())} non-finite elements")
            a = torch.nan_to_num(a, nan=1e30, posinf=1e30, neginf=-1e30)
        if name == "lse":
            errs[name] = (float((a - b).abs().max()),) * 2
            continue
        dead = dead_rows(name, allowed, B, T, H)
        if dead is not None and dead.any():
            nz = int((a[dead] != 0).sum())
            if nz:
                bad.append(f"{name}: {nz} nonzero elements in rows the mask makes exactly zero")
        glob = float((a - b).norm() / max(float(b.norm()), 1e-300))
        rms_row = float(b.norm()) / b.shape[0] ** 0.5
        den = torch.clamp(b.norm(dim=1), min=ROW_FLOOR * rms_row + 1e-300)
        errs[name] = (glob, float(((a - b).norm(dim=1) / den).max()))
    return errs, bad


def failures(errs, bad, tol, global_only=False):
    """Failed checks of measure()'s result against tol {name: (global bound, per-row bound)} (lse: (abs bound, abs bound)).
    global_only: the relative L2 norms over whole tensors alone (out and the gradients), what the older bf16 tests check."""
    out = list(bad) if not global_only else []
    for name, (glob, row) in errs.items():
        if global_only and name == "lse":
            continue
        gt, rt = tol[name]
        if glob > gt:
            out.append(f"{name}: global {glob:.3g} > {gt:g}")
        if not global_only and name != "lse" and row > rt:
            out.append(f"{name}: per-row {row:.3g} > {rt:g}")
    return out


# ---------------------------------------------------------------------------------------------- bounds of the GPU path matrix
# TOL[(direction, path, io dtype, dropout on)] = {tensor: (global relative L2, worst per-row error)}; lse: (absolute, absolute). Paths:
# tests/test_attention_paths_gpu.py. Budget: bf16 P and dS into the MFMAs, fp16 positional products in the short and chunk kernels,
# bf16 q + u / q + v and bf16 outputs give ~2e-3 relative L2 per tensor and ~1e-2 per row; lse carries the bf16 rounding of the scores.
# Each bound is ~1.6x the worst value measured on the MI355X over the path's cases (written after it: global / per-row). The dQ and dK
# per-row bounds are wide where one key dominates a query row (length 1 or 2, the first rows under a causal mask), above all with
# dropout: the reference's dS = P (dP - D) cancels exactly there, the kernels' D = rowsum(dout * out) carries the bf16 rounding of out
# (of the 1 / (1 - p)-scaled value with dropout), ~2^-9 of |dout| |out|, against a row the reference makes near zero.
TOL = {
    ("bwd", "short", "bf16", False): {"dQ": (0.006, 0.36), "dK": (0.0071, 0.014), "dV": (0.0038, 0.012), "dpk": (0.008, 0.029), "du": (0.0088, 0.015), "dv": (0.0065, 0.012)},   # measured dQ 0.0037/0.23 dK 0.0044/0.0087 dV 0.0024/0.0069 dpk 0.005/0.018 du 0.0054/0.0088 dv 0.004/0.007
    ("bwd", "short", "bf16", True): {"dQ": (0.043, 0.9), "dK": (0.04, 2.9), "dV": (0.0043, 0.012), "dpk": (0.041, 0.074), "du": (0.056, 0.13), "dv": (0.031, 0.053)},   # measured dQ 0.026/0.56 dK 0.025/1.8 dV 0.0027/0.0073 dpk 0.025/0.046 du 0.035/0.077 dv 0.019/0.033
    ("bwd", "split", "bf16", False): {"dQ": (0.0054, 0.058), "dK": (0.006, 0.018), "dV": (0.0053, 0.013), "dpk": (0.006, 0.014), "du": (0.004, 0.0043), "dv": (0.0057, 0.0057)},   # measured dQ 0.0034/0.036 dK 0.0037/0.011 dV 0.0033/0.0078 dpk 0.0037/0.0084 du 0.0024/0.0027 dv 0.0036/0.0036
    ("bwd", "split", "bf16", True): {"dQ": (0.0054, 0.29), "dK": (0.006, 0.019), "dV": (0.0053, 0.016), "dpk": (0.006, 0.017), "du": (0.0045, 0.0045), "dv": (0.0053, 0.0053)},   # measured dQ 0.0034/0.18 dK 0.0037/0.011 dV 0.0033/0.0098 dpk 0.0037/0.01 du 0.0028/0.0028 dv 0.0033/0.0033
    ("bwd", "split", "f32", False): {"dQ": (0.0044, 0.011), "dK": (0.0051, 0.011), "dV": (0.0044, 0.012), "dpk": (0.0051, 0.012), "du": (0.0035, 0.0035), "dv": (0.0052, 0.0052)},   # measured dQ 0.0027/0.0069 dK 0.0032/0.0069 dV 0.0027/0.0072 dpk 0.0031/0.0073 du 0.0022/0.0022 dv 0.0032/0.0032
    ("bwd", "split", "f32", True): {"dQ": (0.0045, 0.25), "dK": (0.0052, 0.015), "dV": (0.0042, 0.016), "dpk": (0.0052, 0.012), "du": (0.0039, 0.0039), "dv": (0.0043, 0.0043)},   # measured dQ 0.0028/0.16 dK 0.0032/0.0091 dV 0.0026/0.0096 dpk 0.0032/0.0072 du 0.0024/0.0024 dv 0.0027/0.0027
    ("bwd", "split_ks4", "bf16", False): {"dQ": (0.0056, 0.031), "dK": (0.0061, 0.017), "dV": (0.0055, 0.014), "dpk": (0.0062, 0.017), "du": (0.0047, 0.0047), "dv": (0.0044, 0.0044)},   # measured dQ 0.0034/0.019 dK 0.0038/0.011 dV 0.0034/0.0086 dpk 0.0038/0.01 du 0.0029/0.0029 dv 0.0027/0.0027
    ("bwd", "split_ks4", "bf16", True): {"dQ": (0.0057, 0.11), "dK": (0.0062, 0.017), "dV": (0.0055, 0.016), "dpk": (0.0063, 0.018), "du": (0.0051, 0.0051), "dv": (0.0055, 0.0055)},   # measured dQ 0.0035/0.064 dK 0.0039/0.011 dV 0.0034/0.0094 dpk 0.0039/0.011 du 0.0032/0.0032 dv 0.0034/0.0034
    ("bwd", "stream", "bf16", False): {"dQ": (0.0059, 0.35), "dK": (0.0066, 0.016), "dV": (0.0037, 0.012), "dpk": (0.0065, 0.022), "du": (0.0058, 0.0073), "dv": (0.0059, 0.0082)},   # measured dQ 0.0036/0.21 dK 0.0041/0.0095 dV 0.0023/0.0073 dpk 0.004/0.014 du 0.0036/0.0045 dv 0.0036/0.0051
    ("bwd", "stream", "bf16", True): {"dQ": (0.015, 0.77), "dK": (0.017, 3.8), "dV": (0.0044, 0.015), "dpk": (0.017, 0.07), "du": (0.015, 0.03), "dv": (0.013, 0.03)},   # measured dQ 0.0091/0.48 dK 0.01/2.3 dV 0.0027/0.0093 dpk 0.01/0.044 du 0.0089/0.018 dv 0.0076/0.019
    ("bwd", "stream", "f32", False): {"dQ": (0.0038, 0.048), "dK": (0.0046, 0.0086), "dV": (0.0038, 0.0089), "dpk": (0.0046, 0.0074), "du": (0.0036, 0.004), "dv": (0.004, 0.0042)},   # measured dQ 0.0023/0.03 dK 0.0029/0.0053 dV 0.0023/0.0055 dpk 0.0029/0.0046 du 0.0022/0.0025 dv 0.0025/0.0026
    ("bwd", "stream", "f32", True): {"dQ": (0.0066, 0.34), "dK": (0.0073, 1.1), "dV": (0.0039, 0.0087), "dpk": (0.0071, 0.038), "du": (0.017, 0.026), "dv": (0.0056, 0.0058)},   # measured dQ 0.0041/0.21 dK 0.0045/0.68 dV 0.0024/0.0054 dpk 0.0044/0.023 du 0.01/0.016 dv 0.0034/0.0036
    ("fwd", "chunk", "bf16", False): {"out": (0.0054, 0.014), "lse": (0.0068, 0.0068)},   # measured out 0.0034/0.0086 lse 0.0043
    ("fwd", "chunk", "bf16", True): {"out": (0.0052, 0.015), "lse": (0.0068, 0.0068)},   # measured out 0.0032/0.0092 lse 0.0043
    ("fwd", "short128", "bf16", False): {"out": (0.0031, 0.011), "lse": (0.014, 0.014)},   # measured out 0.0019/0.0068 lse 0.0082
    ("fwd", "short128", "bf16", True): {"out": (0.0035, 0.012), "lse": (0.014, 0.014)},   # measured out 0.0021/0.0071 lse 0.0082
    ("fwd", "short64", "bf16", False): {"out": (0.003, 0.0094), "lse": (0.011, 0.011)},   # measured out 0.0018/0.0059 lse 0.0063
    ("fwd", "short64", "bf16", True): {"out": (0.0034, 0.013), "lse": (0.011, 0.011)},   # measured out 0.0021/0.008 lse 0.0063
    ("fwd", "stream", "bf16", False): {"out": (0.0029, 0.012), "lse": (0.012, 0.012)},   # measured out 0.0018/0.0069 lse 0.0074
    ("fwd", "stream", "bf16", True): {"out": (0.0044, 0.014), "lse": (0.012, 0.012)},   # measured out 0.0027/0.0083 lse 0.0074
    ("fwd", "stream", "f32", False): {"out": (0.0033, 0.0074), "lse": (0.0076, 0.0076)},   # measured out 0.002/0.0046 lse 0.0047
    ("fwd", "stream", "f32", True): {"out": (0.0037, 0.0088), "lse": (0.0075, 0.0075)},   # measured out 0.0023/0.0055 lse 0.0046
    ("fwd", "stream_split", "bf16", False): {"out": (0.0044, 0.009), "lse": (0.0036, 0.0036)},   # measured out 0.0027/0.0056 lse 0.0022
    ("fwd", "stream_split", "bf16", True): {"out": (0.0054, 0.014), "lse": (0.0077, 0.0077)},   # measured out 0.0033/0.0085 lse 0.0048
    ("fwd", "stream_split", "f32", False): {"out": (0.004, 0.011), "lse": (0.0063, 0.0063)},   # measured out 0.0024/0.0066 lse 0.0039
    ("fwd", "stream_split", "f32", True): {"out": (0.0041, 0.011), "lse": (0.0068, 0.0068)},   # measured out 0.0025/0.0068 lse 0.0042
}


def loosest():
    """The loosest bound of every tensor over all paths: what the CPU mutation tests hold the checker to."""
    out = {}
    for t in TOL.values():
        for k, (g, r) in t.items():
            og, orr = out.get(k, (0.0, 0.0))
            out[k] = (max(og, g), max(orr, r))
    return out
