"""float64 reference of the streaming relative-position attention (csrc/stream.hip: attn_stream_kernel, attn_stream_mfma_kernel,
attn_stream_merge_kernel), a push-by-push emulation of what those kernels do, and the strict checker that
tests/test_attn_stream_paths_gpu.py applies to every kernel path and tests/test_attn_stream_ref_cpu.py proves able to fail.
Test infrastructure only.

Contract (tsasr_relpos_attn_stream_fwd): an utterance arrives as pushes (t0, C) of C query frames at absolute offset t0. Query i of the
push (t0, C) may attend key j iff j < min(key_lens[b], t0 + C) - the kernel clamps key_lens to the keys pushed so far, so the growing
valid counts a stream passes equal the fixed final lengths - and, under a mask, j <= limit(i): i for causal = 1, the end of i's block of c
absolute frames for causal = c > 1. With a push that is no multiple of c a query cannot see the keys of its block that have not been
pushed yet; allowed() models exactly that. A row with no allowed key is dead: its output is exactly 0.

Reference: s(i, j) = scale * ((q_i + u).k_j + (q_i + v).pkh[|i - j|]) straight from the half table, inputs promoted to float64 as
stored; none of the kernels' internal roundings (bf16 q + u / q + v, bf16 P, bf16 outputs) is emulated: they are the error budget the
bounds stand for.

Checker: (a) relative L2 over the live rows; (b) the worst per-row error per (b, i, h) over max(|ref row|, ROW_FLOOR x the RMS row
norm); (c) structure: every element finite, dead rows exactly zero."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref  # noqa: E402

ROW_FLOOR = attn_ref.ROW_FLOOR
SKT, MQB = 64, 64       # csrc/stream.hip: keys per tile, queries per workgroup of the matrix-core kernel
DEFECTS = ("causal_late", "cache_dist", "drop_split", "stale_cache", "chunk_lens", "dead_nan", "one_element")


def cdiv(a, b):
    return -(-a // b)


def schedule(sizes, T):
    """Push sizes cycled and truncated to T frames -> ((t0, C), ...)."""
    out, t0, n = [], 0, 0
    while t0 < T:
        c = min(sizes[n % len(sizes)], T - t0)
        out.append((t0, c))
        t0, n = t0 + c, n + 1
    return tuple(out)


def limit(i, causal):
    """The last key query i (int64 tensor of absolute frames) may attend under causal >= 1."""
    return i.clone() if int(causal) <= 1 else (i // int(causal) + 1) * int(causal) - 1


def allowed(pushes, key_lens, causal, B):
    """bool [B, T, T] of the contract above; T = the frames pushed."""
    T = sum(c for _, c in pushes)
    j = torch.arange(T)
    out = torch.zeros(B, T, T, dtype=torch.bool)
    for t0, C in pushes:
        i = torch.arange(t0, t0 + C)
        cm = torch.ones(C, T, dtype=torch.bool) if not causal else j[None, :] <= limit(i, causal)[:, None]
        for b in range(B):
            kmax = t0 + C if key_lens is None else min(int(key_lens[b]), t0 + C)
            out[b, t0:t0 + C] = cm & (j[None, :] < kmax)
    return out


def reference(qkv, pkh, u, v, H, scale, allowed):
    """qkv [B,T,3D] (per-head interleaved Q|K|V), pkh [>= T, D] (row d = the positional row of distance d), u / v [H*Dh];
    allowed bool [B,T,T] -> float64 out [B,T,D]; dead rows exactly 0."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    Dh = D // H
    x, tab, ux, vx = (t.detach().cpu().to(torch.float64) for t in (qkv, pkh, u, v))
    q, k, vv = (t.transpose(1, 2) for t in x.view(B, T, H, 3 * Dh).split(Dh, dim=-1))   # [B,H,T,Dh]
    uu, vb = ux.view(1, H, 1, Dh), vx.view(1, H, 1, Dh)
    ac = (q + uu) @ k.transpose(-1, -2)
    bd_dist = (q + vb) @ tab[:T].view(T, H, Dh).permute(1, 2, 0)                         # [B,H,T,T]: (query, distance)
    dist = (torch.arange(T)[:, None] - torch.arange(T)[None, :]).abs()
    s = (ac + torch.gather(bd_dist, 3, dist.expand(B, H, T, T))) * scale
    live = allowed.any(dim=-1)                                                          # [B,T]
    s = s.masked_fill(~allowed.view(B, 1, T, T), float("-inf"))
    s = torch.where(live.view(B, 1, T, 1), s, torch.zeros_like(s))
    P = torch.softmax(s, dim=-1) * live.view(B, 1, T, 1)
    return (P @ vv).transpose(1, 2).reshape(B, T, D)


def stream_split(B, C, H, Tmax):
    """The host's stream_split (csrc/stream.hip): (nsplit, tiles per split) of a launch, a function of (B, C, H, Tmax) alone."""
    base, maxt = B * H * cdiv(C, MQB), cdiv(Tmax, SKT)
    n = 1
    if base < 256 and maxt > 4:
        n = min(cdiv(256, base), cdiv(maxt, 2))
    t = cdiv(maxt, n)
    return cdiv(maxt, t), t


def emulate(qkv, pkh, u, v, H, scale, pushes, key_lens, causal, Tmax, nsplit, tps, dtype=torch.float64, defect=None):
    """What the kernels do, push by push, in `dtype` arithmetic: an explicit K / V cache [B,H,Tmax,Dh] that starts as NaN and gets the
    chunk's rows at t0 after the push's attention; keys < t0 from the cache, keys >= t0 from the chunk; 64-key tiles with online softmax;
    key splits of `tps` tiles each merged by the m / l / o rule of attn_stream_merge_kernel. -> out [B,T,D] in `dtype`.
    defect: None, a name of DEFECTS, or (name, push index) to plant it in one push only:
      causal_late   the causal limit one frame late for the first query of a push
      cache_dist    the positional distance one short for keys read from the cache
      drop_split    the last non-empty split dropped in the merge (rows with two or more)
      stale_cache   the newest cache row (t0 - 1) read as zeros
      chunk_lens    key_lens ignored for keys of the current chunk
      dead_nan      a dead row left as NaN
      one_element   one element of one row (b 0, the middle frame, the last head) off by 2 % of the row's norm"""
    name, only = (defect, None) if defect is None or isinstance(defect, str) else defect
    assert name is None or name in DEFECTS, name
    B, T, D3 = qkv.shape
    D = D3 // 3
    Dh = D // H
    x = qkv.detach().cpu().to(dtype).view(B, T, H, 3, Dh)
    q, k, vv = x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2]                                # [B,T,H,Dh]
    tab = pkh.detach().cpu().to(dtype).view(-1, H, Dh)
    uu, vb = u.detach().cpu().to(dtype).view(H, Dh), v.detach().cpu().to(dtype).view(H, Dh)
    nan, ninf = float("nan"), float("-inf")
    kc = torch.full((B, H, Tmax, Dh), nan, dtype=dtype)
    vc = torch.full((B, H, Tmax, Dh), nan, dtype=dtype)
    out = torch.full((B, T, D), nan, dtype=dtype)
    for pi, (t0, C) in enumerate(pushes):
        on = name if only is None or only == pi else None
        kend = t0 + C
        assert kend <= Tmax
        i = torch.arange(t0, kend)
        lim = limit(i, causal) if causal else torch.full((C,), 2 ** 30)
        if on == "causal_late":
            lim[0] += 1
        for b in range(B):
            klen = kend if key_lens is None else max(0, min(int(key_lens[b]), kend))
            jend = kend if on == "chunk_lens" else klen
            if causal:
                jend = min(jend, kend, int(lim.max()) + 1)
            qu, qv = q[b, t0:kend] + uu, q[b, t0:kend] + vb                               # [C,H,Dh]
            ntiles = cdiv(jend, SKT)
            parts = []
            for sp in range(nsplit):
                m = torch.full((H, C), ninf, dtype=dtype)
                l = torch.zeros(H, C, dtype=dtype)
                o = torch.zeros(H, C, Dh, dtype=dtype)
                for jt in range(sp * tps, min(ntiles, (sp + 1) * tps)):
                    j = torch.arange(jt * SKT, (jt + 1) * SKT)
                    there = (j < jend) & ((j < klen) | ((j >= t0) if on == "chunk_lens" else torch.zeros_like(j, dtype=torch.bool)))
                    K, V = torch.zeros(SKT, H, Dh, dtype=dtype), torch.zeros(SKT, H, Dh, dtype=dtype)
                    old, new = there & (j < t0), there & (j >= t0)
                    K[old], V[old] = kc[b][:, j[old]].transpose(0, 1), vc[b][:, j[old]].transpose(0, 1)
                    K[new], V[new] = k[b, j[new]], vv[b, j[new]]
                    if on == "stale_cache":
                        K[j == t0 - 1], V[j == t0 - 1] = 0, 0
                    dist = (i[:, None] - j[None, :]).abs()                                # [C,64]
                    if on == "cache_dist":
                        dist = dist - (j < t0)[None, :].long()
                    Pb = tab[dist.clamp(max=tab.shape[0] - 1)] * (dist < Tmax)[:, :, None, None]     # [C,64,H,Dh]
                    s = (torch.einsum("chd,jhd->hcj", qu, K) + torch.einsum("chd,cjhd->hcj", qv, Pb)) * scale
                    masked = ~there[None, :] | (j[None, :] > lim[:, None])                # [C,64]
                    s = s.masked_fill(masked[None], ninf)
                    mn = torch.maximum(m, s.amax(dim=-1))
                    upd = mn > ninf                                                        # else: every key so far is masked
                    ms = torch.where(upd, mn, torch.zeros_like(mn))
                    alpha = torch.where(m == ninf, torch.zeros_like(m), torch.exp(m - ms))
                    p = torch.exp(s - ms[..., None])                                      # exp(-inf) = 0 for the masked keys
                    l = torch.where(upd, l * alpha + p.sum(-1), l)
                    o = torch.where(upd[..., None], o * alpha[..., None] + torch.einsum("hcj,jhd->hcd", p, V), o)
                    m = torch.where(upd, mn, m)
                parts.append((m, l, o))
            if nsplit == 1:
                m, L, O = parts[0]
            else:                                                                          # attn_stream_merge_kernel
                ms_ = torch.stack([p_[0] for p_ in parts])                                # [S,H,C]
                M = ms_.amax(dim=0)
                full = ms_ > ninf
                if on == "drop_split":
                    last = (nsplit - 1) - torch.flip(full, (0,)).to(torch.int8).argmax(dim=0)
                    full = full & ~((torch.arange(nsplit).view(-1, 1, 1) == last[None]) & (full.sum(0) >= 2)[None])
                L, O = torch.zeros(H, C, dtype=dtype), torch.zeros(H, C, Dh, dtype=dtype)
                for s_ in range(nsplit):
                    w = torch.where(full[s_], torch.exp(parts[s_][0] - torch.where(M > ninf, M, torch.zeros_like(M))), torch.zeros_like(M))
                    L = L + parts[s_][1] * w
                    O = O + parts[s_][2] * w[..., None]
            dead = nan if on == "dead_nan" else 0.0
            res = torch.where((L > 0)[..., None], O / torch.where(L > 0, L, torch.ones_like(L))[..., None], torch.full_like(O, dead))
            out[b, t0:kend] = res.transpose(0, 1).reshape(C, D)
        kc[:, :, t0:kend], vc[:, :, t0:kend] = k[:, t0:kend].transpose(1, 2), vv[:, t0:kend].transpose(1, 2)
    if name == "one_element":
        row = out.view(B, T, H, Dh)[0, T // 2, H - 1]
        row[3] += 0.02 * float(row.norm())
    return out


def _rows(got, ref, allowed, B, T, H, Dh):
    a = got.detach().cpu().to(torch.float64).reshape(B * T * H, Dh)
    b = ref.to(torch.float64).reshape(B * T * H, Dh)
    live = allowed.any(dim=-1)[:, :, None].expand(B, T, H).reshape(-1)
    return a, b, live


def measure(got, ref, allowed, B, T, H, Dh):
    """got / ref: out [B,T,D] -> ({"out": (global relative L2 over the live rows, worst per-row error)}, [structural failures])."""
    a, b, live = _rows(got, ref, allowed, B, T, H, Dh)
    bad = []
    if not torch.isfinite(a).all():
        bad.append(f"out: {int((~torch.isfinite(a)).sum())} non-finite elements")
        a = torch.nan_to_num(a, nan=1e30, posinf=1e30, neginf=-1e30)
    if (~live).any():
        nz = int((a[~live] != 0).sum())
        if nz:
            bad.append(f"out: {nz} nonzero elements in rows with no allowed key (exactly zero)")
    a, b = a[live], b[live]
    glob = float((a - b).norm() / max(float(b.norm()), 1e-300))
    rms_row = float(b.norm()) / max(b.shape[0], 1) ** 0.5
    den = torch.clamp(b.norm(dim=1), min=ROW_FLOOR * rms_row + 1e-300)
    row = float(((a - b).norm(dim=1) / den).max()) if b.shape[0] else 0.0
    return {"out": (glob, row)}, bad


def worst_row(got, ref, allowed, B, T, H, Dh):
    """(b, i, h) of the live row with the largest per-row error, for the line a GPU case prints."""
    a, b, live = _rows(got, ref, allowed, B, T, H, Dh)
    a = torch.nan_to_num(a, nan=1e30, posinf=1e30, neginf=-1e30)
    rms_row = float(b[live].norm()) / max(int(live.sum()), 1) ** 0.5
    e = (a - b).norm(dim=1) / torch.clamp(b.norm(dim=1), min=ROW_FLOOR * rms_row + 1e-300)
    n = int(torch.where(live, e, torch.full_like(e, -1.0)).argmax())
    return n // (T * H), n // H % T, n % H


def failures(errs, bad, tol, global_only=False):
    """Failed checks of measure()'s result against tol {"out": (global bound, per-row bound)}; global_only: the relative L2 over the
    whole output alone, what tests/test_streaming_gpu.py checks."""
    return attn_ref.failures(errs, bad, tol, global_only)


def inputs(B, T, H, Dh, Tmax, kind="o1"):
    """-> qkv [B,T,3D], pkh [Tmax+3, D] (a table longer than the cache, which the wrapper allows), u, v [D], scale; fp32 tensors of
    bf16-representable values, so that both io dtypes run the same numbers.
    o1: the draw of tests/test_attention_paths_gpu.py - scores of O(1) after scaling, pos_bias of 0.3.
    peaked: the same draw with the Q part x 4: single keys dominate rows, in different tiles for different rows."""
    assert kind in ("o1", "peaked"), kind
    D = H * Dh
    g = torch.Generator().manual_seed(T * 131 + Dh * 7 + B * H)
    qkv = torch.randn(B, T, 3 * D, generator=g).to(torch.bfloat16).float()
    pkh = torch.randn(Tmax + 3, D, generator=g).to(torch.bfloat16).float()
    u, v = torch.randn(D, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
    if kind == "peaked":
        qkv.view(B, T, H, 3, Dh)[:, :, :, 0] *= 4.0
    return qkv, pkh, u, v, 1.0 / math.sqrt(D)


# ---------------------------------------------------------------------------------------------- bounds of the GPU path matrix
# TOL[(path, kind)] = {"out": (global relative L2 over the live rows, worst per-row error)}. Paths: tests/test_attn_stream_paths_gpu.py.
# Each bound is 1.6x the worst value measured on the MI355X over the path's cases (written after it: global / per-row).
# CEIL, from what the project already holds these kernels to, which no bound exceeds but the exception below: global 1e-5 (fp32) / 8e-3
# (bf16) as tests/test_streaming_gpu.py; per-row 0.015 for the matrix-core kernels (the loosest forward per-row bound of attn_ref.TOL:
# bf16 q + u / q + v, P rounded to bf16, bf16 output); per-row 2^-8 for bf16s (fp32 arithmetic, only the store rounds, by half an ulp
# = 2^-8 relative per element at the most, so no row can be further off: the bf16s per-row bounds are that ceiling, 0.0039, where 1.6x
# the measured value would pass it); per-row 1e-5 for fp32 (the global figure: no row may be worse than the whole is allowed to be).
# OVER_CEILING: the per-row bound of the matrix-core kernels on the peaked draw. It is the format's budget, not the kernels': the Q part
# x 4 makes |q + u|, |q + v| ~ 4, their rounding to bf16 (2^-9 relative, the MFMA operand) moves a score by ~5e-3, and a row that one or
# two keys dominate moves by the same order. A float64 model that rounds only q + u and q + v to bf16 gives per-row 0.0148 / 0.0212
# (Dh 64, unsplit / split shape) and 0.0174 / 0.0182 (Dh 32) on these very cases, with P and the output rounded as well 0.0147 / 0.0209 /
# 0.0182 / 0.0195: what the kernels measure (0.014 / 0.0209 / 0.0184 / 0.0187). The fp32 and bf16s kernels, which keep q + u in fp32, stay
# at their o1 figures on the same cases. The global bounds of these entries are within the ceiling.
CEIL = {"f32": (1e-5, 1e-5), "mfma64": (8e-3, 0.015), "mfma32": (8e-3, 0.015), "bf16s": (8e-3, 2.0 ** -8)}
OVER_CEILING = {("mfma64", "peaked"), ("mfma64_split", "peaked"), ("mfma32", "peaked"), ("mfma32_split", "peaked")}
TOL = {
    ("bf16s", "o1"): {"out": (0.0027, 0.0039)},   # measured 0.00168/0.0031
    ("bf16s", "peaked"): {"out": (0.0026, 0.0039)},   # measured 0.00163/0.00274
    ("bf16s_nows", "o1"): {"out": (0.00065, 0.0039)},   # measured 0.000406/0.00266
    ("bf16s_split", "o1"): {"out": (0.0027, 0.0039)},   # measured 0.00167/0.00299
    ("bf16s_split", "peaked"): {"out": (0.0017, 0.0039)},   # measured 0.00108/0.00287
    ("f32", "o1"): {"out": (5.3e-07, 2.1e-06)},   # measured 3.31e-07/1.34e-06
    ("f32", "peaked"): {"out": (1.1e-06, 8.4e-06)},   # measured 7.1e-07/5.26e-06
    ("f32_nows", "o1"): {"out": (1.5e-07, 2.2e-06)},   # measured 9.66e-08/1.39e-06
    ("f32_split", "o1"): {"out": (6.6e-07, 2.4e-06)},   # measured 4.1e-07/1.49e-06
    ("f32_split", "peaked"): {"out": (8.4e-07, 6e-06)},   # measured 5.23e-07/3.75e-06
    ("mfma32", "o1"): {"out": (0.004, 0.0087)},   # measured 0.00253/0.00541
    ("mfma32", "peaked"): {"out": (0.0054, 0.029)},   # measured 0.00339/0.0184
    ("mfma32_nows", "o1"): {"out": (0.00094, 0.0086)},   # measured 0.000588/0.00539
    ("mfma32_split", "o1"): {"out": (0.0042, 0.0091)},   # measured 0.00265/0.00566
    ("mfma32_split", "peaked"): {"out": (0.0036, 0.03)},   # measured 0.00227/0.0187
    ("mfma64", "o1"): {"out": (0.004, 0.0075)},   # measured 0.00251/0.00471
    ("mfma64", "peaked"): {"out": (0.0057, 0.022)},   # measured 0.00358/0.014
    ("mfma64_nows", "o1"): {"out": (0.0011, 0.0088)},   # measured 0.000713/0.00547
    ("mfma64_split", "o1"): {"out": (0.0042, 0.0088)},   # measured 0.00265/0.00547
    ("mfma64_split", "peaked"): {"out": (0.0039, 0.033)},   # measured 0.00241/0.0209
}


def loosest(kind=None):
    """The loosest bound over all paths (of one kind of draw, or of every kind): what the CPU mutation tests hold the checker to."""
    out = {}
    for (_, kd), t in TOL.items():
        if kind is not None and kd != kind:
            continue
        for k, (g, r) in t.items():
            og, orr = out.get(k, (0.0, 0.0))
            out[k] = (max(og, g), max(orr, r))
    return out
