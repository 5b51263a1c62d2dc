"""float64 model of a slot schedule of the streaming encoder kernels (csrc/stream.hip: tsasr_relpos_attn_stream_slots_fwd,
tsasr_convmod_stream_slots_fwd), built on attn_stream_ref, and the checks tests/test_stream_slots_ref_cpu.py proves able to fail.
Test infrastructure only.

Contract: a batch of B slots. Per push the kernels get the offsets array t0s [B] (an idle slot: -1) - here the model's own offsets and
the push's active mask. An active slot b attends, for its queries at absolute frames t0s[b] .. t0s[b]+C-1 of its own session, the keys
< t0s[b] of its cache and the chunk's own keys, masked by its key length and the (block-)causal limit on its own absolute frames;
the chunk's K / V rows are appended at t0s[b]; its conv history advances. An idle slot: nothing of its cache or history is read or moves,
its rows of both outputs are exact zeros. admit(b) puts the slot's offset to 0 and clears its conv history; the K/V cache keeps its
bytes (rows at or past the offset are never read). The caches start as NaN, so a row read before it was written shows.

The conv part is the depthwise causal convolution over [history (K-1 rows) | chunk]: taps only, which is what the history feeds.

Checks, each named for the planted defect (DEFECTS) it rejects:
    check_idle_cache         idle_appends        an idle slot appends rows to its cache
    check_session_attention  slot0_offset        every slot runs at slot 0's offset
    check_session_conv       hist_not_cleared    admit() leaves the previous session's conv history
    check_idle_hist          idle_hist_moves     an idle slot's conv history advances
    check_poison             reads_past_offset   a cache row at or past the offset is read"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_stream_ref as SR  # noqa: E402

F64 = torch.float64
DEFECTS = {"idle_appends": "check_idle_cache", "slot0_offset": "check_session_attention", "hist_not_cleared": "check_session_conv",
           "idle_hist_moves": "check_idle_hist", "reads_past_offset": "check_poison"}


class Slots:
    """B slots of one layer: K/V cache [B,H,Tmax,Dh] (NaN to begin with), conv history [B,K-1,Dc], offsets t0 [B]."""

    def __init__(self, B, H, Dh, Tmax, pkh, u, v, scale, causal, conv_w=None, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.B, self.H, self.Dh, self.Tmax, self.scale, self.causal, self.defect = B, H, Dh, Tmax, float(scale), int(causal), defect
        self.tab = pkh.detach().cpu().to(F64).view(-1, H, Dh)
        self.u, self.v = u.detach().cpu().to(F64).view(H, Dh), v.detach().cpu().to(F64).view(H, Dh)
        self.kc = torch.full((B, H, Tmax, Dh), float("nan"), dtype=F64)
        self.vc = torch.full((B, H, Tmax, Dh), float("nan"), dtype=F64)
        self.w = None if conv_w is None else conv_w.detach().cpu().to(F64)          # [Dc, K]
        self.hist = None if conv_w is None else torch.zeros(B, self.w.shape[1] - 1, self.w.shape[0], dtype=F64)
        self.t0 = [0] * B
        self.trace = []          # per push: (active, cache and history of every slot before and after)

    def admit(self, b):
        self.t0[b] = 0
        if self.hist is not None and self.defect != "hist_not_cleared":
            self.hist[b] = 0

    def offsets(self, active):
        """The launch array of a push: the slot's offset, -1 for an idle slot."""
        return [t if a else -1 for t, a in zip(self.t0, active)]

    def _snapshot(self):
        return self.kc.clone(), self.vc.clone(), None if self.hist is None else self.hist.clone()

    def push(self, qkv, glu=None, active=None, key_lens=None):
        """qkv [B,C,3D] (per-head Q|K|V; an idle slot's rows are not looked at), glu [B,C,Dc] or None -> (out [B,C,D], z [B,C,Dc] or
        None); the active slots advance by C."""
        B, H, Dh = self.B, self.H, self.Dh
        C = qkv.shape[1]
        active = [True] * B if active is None else [bool(a) for a in active]
        t0s = self.offsets(active)
        if self.defect == "slot0_offset":
            t0s = [max(self.t0[0], 0) if a else -1 for a in active]
        before = self._snapshot()
        x = qkv.detach().cpu().to(F64).view(B, C, H, 3, Dh)
        out = torch.zeros(B, C, H * Dh, dtype=F64)
        z = None if glu is None else torch.zeros(B, C, self.w.shape[0], dtype=F64)
        for b in range(B):
            t0 = t0s[b]
            if t0 < 0 or t0 + C > self.Tmax:
                if self.defect == "idle_appends" and self.t0[b] + C <= self.Tmax:
                    self.kc[b, :, self.t0[b]:self.t0[b] + C] = x[b, :, :, 1].transpose(0, 1)
                    self.vc[b, :, self.t0[b]:self.t0[b] + C] = x[b, :, :, 2].transpose(0, 1)
                if self.defect == "idle_hist_moves" and glu is not None:
                    self.hist[b] = torch.cat([self.hist[b], glu[b].detach().cpu().to(F64)])[-self.hist.shape[1]:]
                continue
            q, k, v = x[b, :, :, 0], x[b, :, :, 1], x[b, :, :, 2]                      # [C,H,Dh]
            kend = t0 + C
            keys = torch.cat([self.kc[b, :, :t0].transpose(0, 1), k])                  # [kend,H,Dh]: cache rows < t0, then the chunk
            vals = torch.cat([self.vc[b, :, :t0].transpose(0, 1), v])
            j = torch.arange(kend)
            if self.defect == "reads_past_offset" and kend < self.Tmax:
                keys = torch.cat([keys, self.kc[b, :, kend:kend + 1].transpose(0, 1)])
                vals = torch.cat([vals, self.vc[b, :, kend:kend + 1].transpose(0, 1)])
                j = torch.cat([j, torch.tensor([t0])])                                  # (read as one more key at the chunk's first frame)
            i = torch.arange(t0, kend)
            klen = kend if key_lens is None else max(0, min(int(key_lens[b]), kend))
            ok = (j[None, :] < klen).expand(C, -1).clone()
            if self.causal:
                ok &= j[None, :] <= SR.limit(i, self.causal)[:, None]
            dist = (i[:, None] - j[None, :]).abs()
            s = (torch.einsum("chd,jhd->hcj", q + self.u, keys) + torch.einsum("chd,cjhd->hcj", q + self.v, self.tab[dist])) * self.scale
            live = ok.any(dim=-1)
            s = s.masked_fill(~ok[None], float("-inf"))
            s = torch.where(live[None, :, None], s, torch.zeros_like(s))
            p = torch.softmax(s, dim=-1) * live[None, :, None]
            # a masked key carries weight exactly 0, but 0 * NaN is NaN: only the keys some query may attend enter the sum
            used = ok.any(dim=0)
            o = torch.einsum("hcj,jhd->chd", p[:, :, used], vals[used])
            out[b] = o.reshape(C, H * Dh)
            self.kc[b, :, t0:kend], self.vc[b, :, t0:kend] = k.transpose(0, 1), v.transpose(0, 1)
            if glu is not None:
                ext = torch.cat([self.hist[b], glu[b].detach().cpu().to(F64)])          # [K-1+C, Dc]
                K = self.w.shape[1]
                z[b] = sum(ext[kk:kk + C] * self.w[:, kk] for kk in range(K))
                self.hist[b] = ext[-(K - 1):].clone()
        self.t0 = [t + C if a else t for t, a in zip(self.t0, active)]
        self.trace.append((active, before, self._snapshot()))
        return out, z


def run_schedule(model, sessions, ticks, C):
    """sessions: {name: dict(qkv [T,3D], glu [T,Dc] or absent, len = valid frames)}; ticks: a list of dicts with optional keys
    ``release`` [slots], ``admit`` {slot: session name} (after the releases) and ``pause`` [slots]; every occupied slot that is not
    paused pushes its session's next C frames. -> {name: (out [T,D], z [T,Dc] or None)} of the frames pushed, and the pushes of each
    session as attn_stream_ref wants them."""
    B = model.B
    owner, pos = [None] * B, {}
    outs = {n: ([], []) for n in sessions}
    for tick in ticks:
        for b in tick.get("release", ()):
            owner[b] = None
        for b, name in tick.get("admit", {}).items():
            assert owner[b] is None, f"slot {b} is occupied"
            model.admit(b)
            owner[b], pos[name] = name, 0
        active = [owner[b] is not None and b not in tick.get("pause", ()) and pos[owner[b]] < sessions[owner[b]]["qkv"].shape[0]
                  for b in range(B)]
        some = next(iter(sessions.values()))
        qkv = torch.zeros(B, C, some["qkv"].shape[1], dtype=F64)
        glu = None if "glu" not in some else torch.zeros(B, C, some["glu"].shape[1], dtype=F64)
        lens = [0] * B
        for b in range(B):
            if active[b]:
                s, p = sessions[owner[b]], pos[owner[b]]
                qkv[b] = s["qkv"][p:p + C]
                if glu is not None:
                    glu[b] = s["glu"][p:p + C]
                lens[b] = s["len"]
        out, z = model.push(qkv, glu, active, lens)
        for b in range(B):
            if active[b]:
                outs[owner[b]][0].append(out[b])
                if z is not None:
                    outs[owner[b]][1].append(z[b])
                pos[owner[b]] += C
    return {n: (torch.cat(o) if o else None, torch.cat(zz) if zz else None) for n, (o, zz) in outs.items()}


def session_reference(model, s, C):
    """What the session computes alone: attn_stream_ref.reference over its own pushes, and the causal depthwise conv with a zero pad."""
    T = s["qkv"].shape[0]
    pushes = SR.schedule((C,), T)
    allowed = SR.allowed(pushes, [s["len"]], model.causal, 1)
    out = SR.reference(s["qkv"][None], model.tab.reshape(model.tab.shape[0], -1), model.u.reshape(-1), model.v.reshape(-1), model.H,
                       model.scale, allowed)[0]
    z = None
    if "glu" in s:
        K = model.w.shape[1]
        ext = torch.cat([torch.zeros(K - 1, s["glu"].shape[1], dtype=F64), s["glu"].to(F64)])
        z = sum(ext[kk:kk + T] * model.w[:, kk] for kk in range(K))
    return out, z


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def check_session_attention(model, sessions, got, C, tol=1e-12):
    bad = []
    for n, s in sessions.items():
        ref, _ = session_reference(model, s, C)
        o = got[n][0]
        if o is None or not torch.isfinite(o).all() or float((o - ref[:o.shape[0]]).abs().max()) > tol:
            bad.append(f"session {n}: attention rows differ from the session alone")
    return bad


def check_session_conv(model, sessions, got, C, tol=1e-12):
    bad = []
    for n, s in sessions.items():
        _, ref = session_reference(model, s, C)
        z = got[n][1]
        if z is None or not torch.isfinite(z).all() or float((z - ref[:z.shape[0]]).abs().max()) > tol:
            bad.append(f"session {n}: conv rows differ from the session alone")
    return bad


def check_idle_cache(model):
    bad = []
    for n, (active, before, after) in enumerate(model.trace):
        for b in range(model.B):
            if not active[b] and not (_same(before[0][b], after[0][b]) and _same(before[1][b], after[1][b])):
                bad.append(f"push {n}: the K/V cache of idle slot {b} moved")
    return bad


def check_idle_hist(model):
    bad = []
    for n, (active, before, after) in enumerate(model.trace):
        for b in range(model.B):
            if not active[b] and before[2] is not None and not _same(before[2][b], after[2][b]):
                bad.append(f"push {n}: the conv history of idle slot {b} moved")
    return bad


def check_poison(got):
    return [f"session {n}: non-finite attention rows (a cache row read before it was written)" for n, (o, _) in got.items()
            if o is not None and not torch.isfinite(o).all()]


def run_checks(model, sessions, got, C):
    """{check name: [failures]} of every check."""
    return {"check_session_attention": check_session_attention(model, sessions, got, C),
            "check_session_conv": check_session_conv(model, sessions, got, C),
            "check_idle_cache": check_idle_cache(model), "check_idle_hist": check_idle_hist(model), "check_poison": check_poison(got)}
