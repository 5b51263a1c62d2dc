"""Float64 references, an fp32 restatement and the check matrix of the RNN-T loss lattice (csrc/rnnt.hip: rnnt_lp_kernel,
rnnt_alphabeta_kernel, rnnt_grad_kernel; the plane layout of csrc/rnnt_ws.h is read through tsasr_rnnt_loss_workspace_layout).

THE OPERATIONS
  rnnt_lp        lse = m + log(sum exp(x - m)) over the V valid columns of a row, lp(blank) = x[blank] - lse, lp(label) = x[y_u] - lse
                 (lpe_out(t, u), and the same value again as lpe_in(t, u + 1))
  rnnt_alphabeta alpha(t, u) = logaddexp(alpha(t-1, u) + lpb(t-1, u), alpha(t, u-1) + lpe_in(t, u)),   alpha(0, 0) = 0
                 beta(t, u)  = logaddexp(beta(t+1, u) + lpb(t, u),   beta(t, u+1) + lpe_out(t, u)),    beta(Tb-1, Ub) = lpb(Tb-1, Ub)
                 logp = alpha(Tb-1, Ub) + lpb(Tb-1, Ub), cost = -logp
  rnnt_grad      dlogits(t, u, v) = gscale * (exp(alpha + beta - logp - lse + x_v) - [v = blank] gblank - [v = y_u] gemit)
with Tb = clamp(tlen, 1, T), Ub = clamp(ulen, 0, U1 - 1) and labels clamped into [0, V) (include/tsasr_hip.h).

WHAT IS COMPARED WITH WHAT
  planes64   float64: lse / lpb / lpe from numpy, alpha / beta / costs from the C oracle (oracle/rnnt_ref.c), the gradient from its planes.
  planes32   an fp32 numpy restatement of each kernel's operation order (the lane tree of rnnt_lp's sums, logaddexp_f's
             m + log2(1 + exp2(d * log2e)) * ln2 with d clamped at -200, rnnt_grad's left-to-right sums). It is NOT a second reference: it
             measures what fp32 costs against float64 on the very inputs of a case, and the kernel gets 4 x that (the
             convention of the feature kernels). Floor: 2 fp32 ulp of the largest magnitude in the plane.
             MODELLING ASSUMPTION: nothing records how exact the hardware's exp2 / log2 are, so no figure is guessed. The restatement runs a
             second time with every transcendental result moved by one fp32 ulp (random direction, fixed seed); the tolerance is 4 x the
             larger of the two runs.
  LOCAL      each stage is judged from the kernel's OWN stored state (its lpb / lpe / alpha / beta / lse / logp), so that error carried along
             the perimeter does not blur the bound of a single step: one wrong cell anywhere in the lattice stands out by itself,
             whatever its occupancy. A lattice step is measured in fp32 ulps of ITS OWN cell (the largest of its operands, its result
             and 1), not of the plane: far off the likely paths a near-converged lattice holds magnitudes of thousands, and a bound
             taken from them would let a cell near the path be wrong by 1e-3.
  GLOBAL     planes, costs and gradient against planes64 within the restatement's carried error, and for every frame boundary the
             invariant logsumexp_u(alpha(t, u) + lpb(t, u) + beta(t + 1, u)) = logp.
The gradient is judged RELATIVE to the larger of its terms (the softmax term and what is subtracted): an absolute bound lets every entry of
a near-converged lattice (1e-3 .. 1e-6) pass whatever it is.
"""
import functools
import math

import numpy as np

from oracle import rnnt_ref as RR

F32 = np.float32
LOG2E = F32(1.44269504089)
LN2 = F32(0.69314718056)
PF = 8                     # the lattice kernel's prefetch window = steps per chunk
PLANES = ("lse", "lpb", "lpe_in", "lpe_out", "alpha", "beta")
REGIMES = ("normal", "peaked", "flat", "offset", "wide", "masked")
FACTOR = 4.0               # the kernel gets FACTOR x what the restatement loses against float64


# ---------------------------------------------------------------------------------------------------------------------------------
# lattice plans: a mirror of rnnt_plan (csrc/rnnt_ws.h)
# ---------------------------------------------------------------------------------------------------------------------------------
def lattice_K(U1):
    K = 1
    while 64 * K < U1:
        K *= 2
    return K


def instantiation(B, U1, plan=(-1, -1, -1)):
    """(KT, NW, NC, skew) of the lattice kernel that runs a [B, *, U1] batch under tsasr_rnnt_lattice_plan(*plan)."""
    skew_p, waves_p, mc_p = plan
    max_waves = waves_p if waves_p > 0 else 8
    skew_mode = skew_p if skew_p >= 0 else 1
    mc_cols = mc_p if mc_p >= 0 else 2
    mc_limit = 2048 if mc_p > 0 else 32
    K = lattice_K(U1)
    if K >= 8 and skew_mode != 0 and mc_cols in (1, 2, 4) and 2 * B * (K // mc_cols) <= mc_limit:
        return (mc_cols, 1, K // mc_cols, 1)
    nw = 1
    if K >= 8:
        nw = min(max_waves, K // 2)
        while nw & (nw - 1):
            nw &= nw - 1
    return (K // nw, nw, 1, 1 if (skew_mode == 2 or (skew_mode == 1 and nw > 1)) else 0)


# the dispatch table of launch_alphabeta: 15 (KT, NW) x (frame-major | skewed) + 3 split forms
AB_TABLE = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (4, 2), (8, 2), (16, 2), (2, 4), (4, 4), (8, 4), (2, 8), (4, 8), (2, 16)]
ALL_INSTANTIATIONS = sorted({(kt, nw, 0, s) for kt, nw in AB_TABLE for s in (0, 1)} | {(kt, 1, 1, 1) for kt in (1, 2, 4)})   # (KT, NW, split, skew)


def inst_key(inst):
    """An instantiation as the template arguments see it: (KT, NW, split?, skew)."""
    kt, nw, nc, skew = inst
    return (kt, nw, 1 if nc > 1 else 0, skew)


RAMP_U1 = (3, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)       # both ends of every K range
RAMP_PLANS = [(s, w, 0) for s in (0, 2) for w in (1, 2, 4, 8, 16)] + [(1, 8, mc) for mc in (1, 2, 4)]
RAMP_T, RAMP_TLEN = 11, (11, 4, 1)


def ramp_ulens(U1, inst, n):
    """n target lengths on the thread, wave and column-block boundaries of an instantiation: drawn from
    {0, KT g - 1, KT g, 64 KT k - 1, 64 KT k, U1 - 1} (as LAST live column Ub), deterministically."""
    kt, nw, nc, _ = inst
    rng = np.random.default_rng(U1 * 131 + kt * 17 + nw * 3 + nc)
    cand = {0, U1 - 1}
    G = (U1 + kt - 1) // kt
    if G > 1:
        g = int(rng.integers(1, G))
        cand |= {kt * g - 1, kt * g}
    nk = (U1 - 1) // (64 * kt)
    if nk >= 1:
        k = int(rng.integers(1, nk + 1))
        cand |= {64 * kt * k - 1, 64 * kt * k}
    cand = sorted(c for c in cand if 0 <= c <= U1 - 1)
    # the widest lattice first (every thread of the instantiation has live columns), then the boundaries in a fixed shuffle
    rest = [c for c in cand if c != U1 - 1]
    rng.shuffle(rest)
    return ([U1 - 1] + rest + [0, 0])[:n]


def ramp_cases():
    """[(B, U1, plan, instantiation)]: every instantiation the plans of the issue reach at every U1, once each."""
    seen, out = set(), []
    for U1 in RAMP_U1:
        for plan in RAMP_PLANS:
            B = 3
            if plan[2] > 0 and lattice_K(U1) >= 8:
                B = max(1, min(3, 32 // (lattice_K(U1) // plan[2])))      # split lattices: 2 B NC <= 64, every workgroup resident
            inst = instantiation(B, U1, plan)
            if (U1, inst_key(inst)) in seen:
                continue
            seen.add((U1, inst_key(inst)))
            out.append((B, U1, plan, inst))
    return out


STEADY_FORMS = [(nw, skew) for nw in (1, 2, 4, 8, 16) for skew in (0, 2)]


def steady_cases():
    """[(group, B, T, U1, tlen, plan)]: T = 64 NW + 29 and tlen = [T, 64 NW - 3] - one utterance reaches the unguarded chunk, one does not."""
    out = []
    for nw, skew in STEADY_FORMS:
        U1 = 257 if nw <= 4 else 513 if nw == 8 else 1025
        T = 64 * nw + 29
        out.append((f"nw{nw}", 2, T, U1, (T, 64 * nw - 3), (skew, nw, 0)))
    for kt in (1, 2, 4):
        out.append(("nw1", 2, 93, 257, (93, 61), (1, 8, kt)))
    return out


def is_steady(s, Tb, G):
    """Step s of a lattice walk runs in the unguarded chunk form (chunk(s0, false_type))."""
    s0 = ((s + PF) // PF) * PF - PF
    return s0 >= G - 1 and s0 + PF < Tb


def where(inst, Tb, t, u, direction):
    """Who computes cell (t, u): thread, wave, column block, step, ramp or steady - for a failure message."""
    kt, nw, nc, _ = inst
    g = u // kt
    G = 64 * nw
    cb, gl = (g // 64, g % 64) if nc > 1 else (0, g)
    s = t + gl if direction == "alpha" else (Tb - 1 - t) + (G - 1 - gl)
    return f"thread g={g} wave={gl // 64} block={cb} step s={s} ({'steady' if is_steady(s, Tb, G) else 'ramp'})"


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def clamp_args(targets, tlen, ulen, T, U1, V):
    """Lengths and labels as the header documents them: Tb = clamp(tlen, 1, T), Ub = clamp(ulen, 0, U1 - 1), labels into [0, V)."""
    Tb = np.clip(np.asarray(tlen, np.int64), 1, T).astype(np.int32)
    Ub = np.clip(np.asarray(ulen, np.int64), 0, U1 - 1).astype(np.int32)
    tg = np.clip(np.asarray(targets, np.int64), 0, V - 1).astype(np.int32)
    return tg, Tb, Ub


def make_targets(rng, B, U1, V, blank, allowed=None):
    labels = [v for v in (range(V) if allowed is None else allowed) if v != blank] or [blank]
    return np.asarray(labels, np.int32)[rng.integers(0, len(labels), size=(B, max(U1 - 1, 1)))]


def make_logits(regime, B, T, U1, V, targets, tlen, ulen, blank, seed):
    """[B, T, U1, V] float32 logits of one of the six regimes, deterministic in (regime, shape, seed)."""
    rng = np.random.default_rng([seed, REGIMES.index(regime), B, T, U1, V])
    tg, Tb, Ub = clamp_args(targets, tlen, ulen, T, U1, V)
    if regime == "flat":
        return np.full((B, T, U1, V), 0.625, np.float32)
    if regime == "wide":
        return (30.0 * rng.standard_normal((B, T, U1, V))).astype(np.float32)
    x = 2.0 * rng.standard_normal((B, T, U1, V))
    if regime == "offset":
        x += rng.uniform(-80.0, 80.0, size=(B, T, U1, 1))
    if regime == "peaked":      # a near-converged model: +12 on the label along a random monotone path and on blank elsewhere
        x = 0.5 * rng.standard_normal((B, T, U1, V))
        for b in range(B):
            moves = np.zeros(Tb[b] - 1 + Ub[b], bool)
            moves[rng.permutation(moves.size)[:Ub[b]]] = True          # True: emit a label
            peak = np.full((T, U1), blank)
            t = u = 0
            for mv in moves:
                if mv:
                    peak[t, u] = tg[b, u]
                    u += 1
                else:
                    t += 1
            x[b][np.arange(T)[:, None], np.arange(U1)[None, :], peak] += 12.0
    if regime == "masked":      # -inf in columns that are neither blank nor a label of that utterance
        for b in range(B):
            free = sorted(set(range(V)) - {blank} - set(tg[b, :Ub[b]].tolist()))
            for v in free[: max(1, len(free) // 2)] if len(free) else []:
                x[b, ..., v] = -np.inf
    return x.astype(np.float32)


def flat_cost(Tb, Ub, V):
    """All logits equal: every path has probability V^-(Tb+Ub) and there are C(Tb+Ub-1, Ub) of them."""
    return (Tb + Ub) * math.log(V) - (math.lgamma(Tb + Ub) - math.lgamma(Ub + 1) - math.lgamma(Tb))


# ---------------------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------------------
def _live(Tb, Ub, T, U1):
    t, u = np.arange(T)[None, :, None], np.arange(U1)[None, None, :]
    return (t < Tb[:, None, None]) & (u <= Ub[:, None, None])


def _take_v(x, idx):
    return np.take_along_axis(x, idx[..., None].astype(np.int64), axis=-1)[..., 0]


def _labels_plane(tg, T, U1):
    """label of the emit transition out of column u, [B, 1, U1] (the last column has none: 0)."""
    B = tg.shape[0]
    lab = np.zeros((B, U1), np.int32)
    n = min(U1 - 1, tg.shape[1])
    lab[:, :n] = tg[:, :n]
    return lab[:, None, :]


def grads64(x, lab, blank, Tb, Ub, gs, lse, lpb, lpe, alpha, beta, logp, want_scale=False):
    """The gradient formula in float64 on ANY set of planes (the oracle's, or a kernel's own), x = logits[..., :V].
    Returns dlogits [B, T, U1, V] (0 outside the lattice) and, on request, the magnitude of its larger term."""
    B, T, U1, V = x.shape
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    lse, lpb, lpe, alpha, beta = f(lse), f(lpb), f(lpe), f(alpha), f(beta)
    lp_ = f(logp)[:, None, None]
    live = _live(Tb, Ub, T, U1)
    t, u = np.arange(T)[None, :, None], np.arange(U1)[None, None, :]
    last_t, last_u = t == (Tb[:, None, None] - 1), u == Ub[:, None, None]
    with np.errstate(all="ignore"):
        bdn = np.concatenate([beta[:, 1:], np.zeros((B, 1, U1))], 1)          # beta(t + 1, u)
        brt = np.concatenate([beta[:, :, 1:], np.zeros((B, T, 1))], 2)        # beta(t, u + 1)
        gblank = np.where(~last_t, np.exp(alpha + lpb + bdn - lp_), np.where(last_u, np.exp(alpha + lpb - lp_), 0.0))
        gemit = np.where(u < Ub[:, None, None], np.exp(alpha + lpe + brt - lp_), 0.0)
        soft = np.exp((alpha + beta - lp_ - lse)[..., None] + f(x))
        v = np.arange(V)[None, None, None, :]
        sub = np.where(v == blank, gblank[..., None], 0.0) + np.where((v == lab[..., None]) & (u < Ub[:, None, None])[..., None], gemit[..., None], 0.0)
        g = np.where(live[..., None], (soft - sub) * f(gs)[:, None, None, None], 0.0)
        scale = np.where(live[..., None], np.maximum(soft, sub) * np.abs(f(gs))[:, None, None, None], 0.0)
    return (g, scale) if want_scale else g


def planes64(logits, targets, tlen, ulen, blank, V, gscale=None):
    """float64 planes of a batch: lse / lpb / lpe from numpy, alpha / beta / costs from the C oracle, the gradient from those planes."""
    lg = np.asarray(logits, np.float32)
    B, T, U1 = lg.shape[:3]
    tg, Tb, Ub = clamp_args(targets, tlen, ulen, T, U1, V)
    gs = np.ones(B) if gscale is None else np.asarray(gscale, np.float64)
    x = lg[..., :V].astype(np.float64)
    lab = _labels_plane(tg, T, U1)
    with np.errstate(all="ignore"):
        m = x.max(-1)
        lse = m + np.log(np.exp(x - m[..., None]).sum(-1))
    lpb = x[..., blank] - lse
    lpe = _take_v(x, np.broadcast_to(lab, (B, T, U1))) - lse
    costs, g32, alpha, beta = RR.rnnt_costs_grads(np.ascontiguousarray(lg), tg, Tb, Ub, blank, V=V, want_ab=True)
    logp = -costs
    g, scale = grads64(x, lab, blank, Tb, Ub, gs, lse, lpb, lpe, alpha, beta, logp, want_scale=True)
    return dict(lse=lse, lpb=lpb, lpe=lpe, alpha=alpha, beta=beta, logp=logp, costs=costs, grads=g, gscale_mag=scale,
                oracle_grads=g32[..., :V], Tb=Tb, Ub=Ub, targets=tg, lab=lab, live=_live(Tb, Ub, T, U1), x=x, gs=gs, blank=blank, V=V)


def brute_force_cost(logits, targets, T, U, blank=0):
    return RR.brute_force_cost(logits, targets, T, U, blank)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
class Fp32Model:
    """The transcendentals of the kernels as numpy sees them; perturb = seed: every result moved one ulp up or down at random."""

    def __init__(self, perturb=None, clamp=-200.0):
        self.rng = None if perturb is None else np.random.default_rng(perturb)
        self.clamp = F32(clamp)

    def _p(self, y):
        y = np.asarray(y, F32)
        if self.rng is None:
            return y
        up = self.rng.integers(0, 2, size=y.shape).astype(bool)
        with np.errstate(all="ignore"):
            return np.where(np.isfinite(y), np.nextafter(y, np.where(up, F32(np.inf), F32(-np.inf)).astype(F32)), y).astype(F32)

    def exp2(self, x):
        with np.errstate(all="ignore"):
            return self._p(np.exp2(np.asarray(x, F32)))

    def log2(self, x):
        with np.errstate(all="ignore"):
            return self._p(np.log2(np.asarray(x, F32)))

    def expf(self, x):          # __expf: v_exp_f32(x * log2e)
        with np.errstate(all="ignore"):
            return self.exp2(np.asarray(x, F32) * LOG2E)

    def logf(self, x):          # __logf: v_log_f32(x) * ln2
        return (self.log2(x) * LN2).astype(F32)

    def lae(self, a, b):
        """logaddexp_f of csrc/rnnt.hip: m = max, d = max(min - m, -200) (NaN from -inf - -inf gives the clamp), fma(log2(1 + exp2(d log2e)), ln2, m)."""
        a, b = np.asarray(a, F32), np.asarray(b, F32)
        with np.errstate(all="ignore"):
            m = np.fmax(a, b)
            d = np.fmax(np.fmin(a, b) - m, self.clamp)
            lg = self.log2(F32(1.0) + self.exp2(d * LOG2E))
            return (lg.astype(np.float64) * np.float64(LN2) + m.astype(np.float64)).astype(F32)      # fma: one rounding


def _lp32(x, lab, blank, M):
    """rnnt_lp's order: 8 lanes per row, lane s takes columns 4s .. 4s+3 of every 32-column chunk in order, then the three DPP steps
    (lane ^ 1, lane ^ 2, mirrored half row) - lane 0 ends with ((a0 + a1) + (a2 + a3)) + ((a7 + a6) + (a5 + a4))."""
    B, T, U1, V = x.shape
    nch = (V + 31) // 32
    xp = np.full((B, T, U1, nch * 32), -np.inf, F32)
    xp[..., :V] = x
    with np.errstate(all="ignore"):
        m = xp.max(-1)
        e = M.expf(xp - m[..., None]).reshape(B, T, U1, nch, 8, 4)
        lane = np.zeros((B, T, U1, 8), F32)
        for k in range(nch):
            for j in range(4):
                lane = lane + e[..., k, :, j]
        s = ((lane[..., 0] + lane[..., 1]) + (lane[..., 2] + lane[..., 3])) + ((lane[..., 7] + lane[..., 6]) + (lane[..., 5] + lane[..., 4]))
        lse = (m + M.logf(s)).astype(F32)
        lpb = (x[..., blank] - lse).astype(F32)
        lpe = (_take_v(x, np.broadcast_to(lab, (B, T, U1))) - lse).astype(F32)
    return lse, lpb, lpe


def _diagonals(Tb, Ub, T, U1):
    """live cells (b, t, u) grouped by anti-diagonal t + u, as index arrays."""
    b, t, u = np.nonzero(_live(Tb, Ub, T, U1))
    order = np.argsort(t + u, kind="stable")
    b, t, u = b[order], t[order], u[order]
    cuts = np.searchsorted(t + u, np.arange(T + U1 + 1))
    return b, t, u, cuts


def _alpha32(M, lpb, lpe_in, Tb, Ub, patches=()):
    B, T, U1 = lpb.shape
    A = np.full((B, T + 1, U1 + 1), -np.inf, F32)           # [b, t + 1, u + 1]: a border of -inf at t = -1 and u = -1
    LB = np.full((B, T + 1, U1), 0, F32)
    LB[:, 1:] = lpb
    bi, ti, ui, cuts = _diagonals(Tb, Ub, T, U1)
    byd = {}
    for p in patches:
        byd.setdefault(p["t"] + p["u"], []).append(p)
    with np.errstate(all="ignore"):
        for n in range(T + U1 - 1):
            lo, hi = cuts[n], cuts[n + 1]
            if lo == hi:
                continue
            b, t, u = bi[lo:hi], ti[lo:hi], ui[lo:hi]
            ne = np.where(t > 0, A[b, t, u + 1] + LB[b, t, u], np.where(u == 0, F32(0), F32(-np.inf))).astype(F32)
            qm = np.where(u > 0, lpe_in[b, t, u], F32(-np.inf)).astype(F32)
            A[b, t + 1, u + 1] = M.lae(ne, A[b, t + 1, u] + qm)
            for p in byd.get(n, ()):
                b0, t0, u0 = p["b"], p["t"], p["u"]
                left, ne0, qm0 = A[b0, t0 + 1, u0], A[b0, t0, u0 + 1] + LB[b0, t0, u0], lpe_in[b0, t0, u0]
                if p["kind"] == "left_inf":                 # the hand-off never arrived
                    left = F32(-np.inf)
                elif p["kind"] == "left_stale":             # the hand-off of the step before: alpha(t - 1, u - 1)
                    left = A[b0, t0, u0]
                elif p["kind"] == "stale_operands":         # the step reuses the operands of frame t - 1
                    ne0, qm0 = A[b0, t0, u0 + 1] + LB[b0, t0 - 1, u0], lpe_in[b0, t0 - 1, u0]
                A[b0, t0 + 1, u0 + 1] = M.lae(ne0, left + qm0)
    return A[:, 1:, 1:].copy()


def _beta32(M, lpb, lpe_out, Tb, Ub, seed_zero=False):
    B, T, U1 = lpb.shape
    Bt = np.full((B, T + 1, U1 + 1), -np.inf, F32)          # border of -inf at t = T and u = U1
    bi, ti, ui, cuts = _diagonals(Tb, Ub, T, U1)
    Tbb, Ubb = Tb[:, None], Ub[:, None]
    with np.errstate(all="ignore"):
        for n in range(T + U1 - 2, -1, -1):
            lo, hi = cuts[n], cuts[n + 1]
            if lo == hi:
                continue
            b, t, u = bi[lo:hi], ti[lo:hi], ui[lo:hi]
            lb = lpb[b, t, u]
            seed = F32(0) if seed_zero else lb
            ne = np.where(t < Tbb[b, 0] - 1, Bt[b, t + 1, u] + lb, np.where(u == Ubb[b, 0], seed, F32(-np.inf))).astype(F32)
            qm = np.where(u < Ubb[b, 0], lpe_out[b, t, u], F32(-np.inf)).astype(F32)
            # (columns beyond Ub are not live; the border at u = Ub + 1 may hold a live-looking value of a longer utterance: masked by qm)
            Bt[b, t, u] = M.lae(ne, np.where(u < Ubb[b, 0], Bt[b, t, u + 1], F32(-np.inf)) + qm)
    return Bt[:, :T, :U1].copy()


def grads32(M, x, lab, blank, Tb, Ub, gs, lse, lpb, lpe_out, alpha, beta, logp, miss_gemit_at=None):
    """rnnt_grad's order: c0 = ((a + be) - logp) - lse; val = expf(c0 + x) [- gblank] [- gemit]; * gscale."""
    B, T, U1, V = x.shape
    live = _live(Tb, Ub, T, U1)
    t, u = np.arange(T)[None, :, None], np.arange(U1)[None, None, :]
    last_t, last_u, emits = t == (Tb[:, None, None] - 1), u == Ub[:, None, None], u < Ub[:, None, None]
    lp_ = np.asarray(logp, F32)[:, None, None]
    with np.errstate(all="ignore"):
        bdn = np.concatenate([beta[:, 1:], np.zeros((B, 1, U1), F32)], 1)
        brt = np.concatenate([beta[:, :, 1:], np.zeros((B, T, 1), F32)], 2)
        c0 = (((alpha + beta) - lp_) - lse).astype(F32)
        gblank = np.where(~last_t, M.expf(((alpha + lpb) + bdn) - lp_), np.where(last_u, M.expf((alpha + lpb) - lp_), F32(0))).astype(F32)
        gemit = np.where(emits, M.expf(((alpha + lpe_out) + brt) - lp_), F32(0)).astype(F32)
        val = M.expf(c0[..., None] + x)
        v = np.arange(V)[None, None, None, :]
        val = np.where(v == blank, val - gblank[..., None], val).astype(F32)
        is_lab = (v == lab[..., None]) & emits[..., None]
        if miss_gemit_at is not None:
            is_lab = np.broadcast_to(is_lab, val.shape).copy()
            is_lab[miss_gemit_at] = False
        val = np.where(is_lab, val - gemit[..., None], val).astype(F32)
        g = (val * np.asarray(gs, F32)[:, None, None, None]).astype(F32)
    return np.where(live[..., None], g, F32(0))


def planes32(logits, targets, tlen, ulen, blank, V, gscale=None, perturb=None, clamp=-200.0, defect=None):
    """The kernels' outputs as an fp32 numpy restatement gives them (same keys as a kernel run: the six planes [B, T, U1], logp, costs,
    dlogits [B, T, U1, V]). defect: one planted fault, see DEFECTS."""
    lg = np.asarray(logits, np.float32)
    B, T, U1 = lg.shape[:3]
    tg, Tb, Ub = clamp_args(targets, tlen, ulen, T, U1, V)
    gs = np.ones(B, F32) if gscale is None else np.asarray(gscale, F32)
    M = Fp32Model(perturb, clamp)
    x = lg[..., :V]
    lab = _labels_plane(tg, T, U1)
    d = defect or {}
    kind = d.get("kind")
    lse, lpb, lpe_out = _lp32(x, lab, (blank + 1) % V if kind == "blank_neighbour" else blank, M)
    lpe_in = np.zeros_like(lpe_out)
    lpe_in[:, :, 1:] = lpe_out[:, :, :-1]
    if kind == "lpe_in_shift":                               # lpe_in(t, u) = lpe(t, u) instead of lpe(t, u - 1)
        lpe_in = lpe_out.copy()
    patches = [d] if kind in ("left_inf", "left_stale", "stale_operands") else ()
    alpha = _alpha32(M, lpb, lpe_in, Tb, Ub, patches)
    beta = _beta32(M, lpb, lpe_out, Tb, Ub, seed_zero=(kind == "beta_seed_zero"))
    if kind == "alpha_cell":
        alpha[d["b"], d["t"], d["u"]] += F32(d["by"])
    bb = np.arange(B)
    logp = (alpha[bb, Tb - 1, Ub] + lpb[bb, Tb - 1, Ub]).astype(F32)
    g = grads32(M, x, lab, blank, Tb, Ub, gs, lse, lpb, lpe_out, alpha, beta, logp,
                miss_gemit_at=(d["b"], d["t"], d["u"], int(tg[d["b"], d["u"]])) if kind == "miss_gemit" else None)
    return dict(lse=lse, lpb=lpb, lpe_in=lpe_in, lpe_out=lpe_out, alpha=alpha, beta=beta, logp=logp, costs=(-logp).astype(F32), dlogits=g)


# ---------------------------------------------------------------------------------------------------------------------------------
# the check matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def _ulp(x):
    return float(np.spacing(F32(max(abs(float(x)), 1e-30))))


def _abs_err(got, ref, mask):
    """|got - ref| where mask, inf where either is not finite and they differ."""
    with np.errstate(all="ignore"):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        e = np.abs(got - ref)
        e = np.where(np.isfinite(got) & np.isfinite(ref), e, np.where(got == ref, 0.0, np.inf))
    return np.where(mask, e, 0.0)


def _shift(a, axis, by, fill):
    """a shifted so that out[i] = a[i + by] along axis (fill outside)."""
    out = np.full_like(a, fill)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if by > 0:
        src[axis], dst[axis] = slice(by, None), slice(None, -by)
    else:
        src[axis], dst[axis] = slice(None, by), slice(-by, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def metrics(out, ref):
    """Every check of the matrix as an error array over ALL live cells (no cell left out): name -> (errors, the floor of the
    tolerance per utterance, the magnitude per utterance). alpha_local / beta_local are in fp32 ulps of the cell, grad_local / grad relative
    to the larger term of the entry, everything else absolute.
    out: a kernel's (or the restatement's) planes, logp, costs, dlogits; ref: planes64 of the same inputs."""
    Tb, Ub, live, x, lab, blank, gs = ref["Tb"], ref["Ub"], ref["live"], ref["x"], ref["lab"], ref["blank"], ref["gs"]
    B, T, U1, V = x.shape
    t, u = np.arange(T)[None, :, None], np.arange(U1)[None, None, :]
    Tb3, Ub3 = Tb[:, None, None], Ub[:, None, None]
    emits, enters = live & (u < Ub3), live & (u > 0)
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    k = {p: f(out[p]) for p in PLANES}
    logp_k, bb = f(out["logp"]), np.arange(B)
    NI = -np.inf
    mag = lambda a, m: np.array([np.max(np.abs(np.where(m[b] & np.isfinite(a[b]), a[b], 0.0)), initial=0.0) for b in range(B)])  # noqa: E731
    fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)  # noqa: E731
    # one lattice step is judged in fp32 ulps of ITS OWN cell: of the largest of its operands and its result, and of 1 (the log term is < 1)
    cell_ulp = lambda r, a, c: np.spacing(np.maximum(np.maximum(fin(r), fin(a)), np.maximum(fin(c), 1.0)).astype(F32)).astype(np.float64)  # noqa: E731
    res = {}

    def put(name, err, m_=None, floor=None):
        res[name] = (err, np.array([2.0 * _ulp(v) for v in m_]) if floor is None else np.full(B, floor), m_ if m_ is not None else np.ones(B))
    with np.errstate(all="ignore"):
        # --- rnnt_lp against float64 (its inputs are the logits: local and global are the same thing)
        put("lse", _abs_err(k["lse"], ref["lse"], live), mag(ref["lse"], live))
        put("lpb", _abs_err(k["lpb"], ref["lpb"], live), mag(ref["lpb"], live))
        put("lpe_out", _abs_err(k["lpe_out"], ref["lpe"], emits), mag(ref["lpe"], emits))
        put("lpe_in", _abs_err(k["lpe_in"], _shift(ref["lpe"], 2, -1, 0.0), enters), mag(ref["lpe"], emits))
        # --- one lattice step from the kernel's own state
        ne = np.where(t > 0, _shift(k["alpha"] + k["lpb"], 1, -1, NI), np.where(u == 0, 0.0, NI))
        em = np.where(u > 0, _shift(k["alpha"], 2, -1, NI) + k["lpe_in"], NI)
        put("alpha_local", _abs_err(k["alpha"], np.logaddexp(ne, em), live) / cell_ulp(k["alpha"], ne, em), floor=2.0)
        ne = np.where(t < Tb3 - 1, _shift(k["beta"], 1, 1, NI) + k["lpb"], np.where(u == Ub3, k["lpb"], NI))
        em = np.where(u < Ub3, _shift(k["beta"], 2, 1, NI) + k["lpe_out"], NI)
        put("beta_local", _abs_err(k["beta"], np.logaddexp(ne, em), live) / cell_ulp(k["beta"], ne, em), floor=2.0)
        lp_own = k["alpha"][bb, Tb - 1, Ub] + k["lpb"][bb, Tb - 1, Ub]
        put("logp_local", _abs_err(logp_k, lp_own, np.ones(B, bool)), np.abs(lp_own))
        put("cost_local", _abs_err(f(out["costs"]), -lp_own, np.ones(B, bool)), np.abs(lp_own))
        g_own, sc_own = grads64(x, lab, blank, Tb, Ub, gs, k["lse"], k["lpb"], k["lpe_out"], k["alpha"], k["beta"], logp_k, want_scale=True)
        dl = f(out["dlogits"])[..., :V]
        put("grad_local", _abs_err(dl, g_own, live[..., None]) / np.maximum(sc_own, 1e-30), floor=2.0 * 2.0 ** -23)
        # --- carried error: planes, costs, gradient against the oracle; the frame-boundary invariant
        put("alpha", _abs_err(k["alpha"], ref["alpha"], live), mag(ref["alpha"], live))
        put("beta", _abs_err(k["beta"], ref["beta"], live), mag(ref["beta"], live))
        put("cost", _abs_err(f(out["costs"]), ref["costs"], np.ones(B, bool)), np.abs(ref["costs"]))
        put("grad", _abs_err(dl, ref["grads"], live[..., None]) / np.maximum(ref["gscale_mag"], 1e-30), floor=2.0 * 2.0 ** -23)
        z = np.where(live & (t < Tb3 - 1), k["alpha"] + k["lpb"] + _shift(k["beta"], 1, 1, NI), NI)       # [B, T, U1]
        zm = z.max(-1)
        inv = np.where(np.isfinite(zm), zm + np.log(np.exp(z - np.where(np.isfinite(zm), zm, 0.0)[..., None]).sum(-1)), NI)
        bound = np.arange(T)[None, :] < (Tb[:, None] - 1)
        put("invariant", _abs_err(inv, np.broadcast_to(logp_k[:, None], (B, T)), bound), np.abs(logp_k))
    return res


def _per_b_max(err):
    return err.reshape(err.shape[0], -1).max(-1) if err.ndim > 1 else err


def tolerances(inputs, ref):
    """4 x what the fp32 restatement loses (the larger of the plain and the ulp-perturbed run), per check and utterance;
    floor 2 fp32 ulp of the largest magnitude in the plane (one lattice step: 2 ulp of its own cell, which is never more; gradients: relative
    to their larger term, so 2 ulp of 1)."""
    tol = {}
    for perturb in (None, 20260):
        m = metrics(planes32(*inputs[:6], gscale=inputs[6], perturb=perturb), ref)
        for name, (err, floor, _) in m.items():
            t_ = np.maximum(FACTOR * _per_b_max(err), floor)
            tol[name] = t_ if name not in tol else np.maximum(tol[name], t_)
    return tol


def judge(out, ref, tol, inst=None):
    """(failures, fractions): a message for the FIRST wrong cell of every check that misses its tolerance, and the worst fraction of the
    tolerance each check used."""
    fails, frac = [], {}
    Tb = ref["Tb"]
    for name, (err, _, _) in metrics(out, ref).items():
        t_ = tol[name].reshape((-1,) + (1,) * (err.ndim - 1))
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / t_)
        frac[name] = float(np.max(ratio))
        bad = np.argwhere(~(ratio <= 1.0))
        if len(bad):
            idx = tuple(int(i) for i in bad[0])
            msg = f"{name}: first wrong cell (b, t, u[, v]) = {idx}: error {err[idx]:.3e} > tolerance {float(t_.reshape(-1)[idx[0]]):.3e} ({len(bad)} cells)"
            if inst is not None and len(idx) >= 3:
                msg += "; " + where(inst, int(Tb[idx[0]]), idx[1], idx[2], "beta" if name.startswith("beta") else "alpha")
            fails.append(msg)
    return fails, frac


def old_tolerances_accept(out, ref):
    """What tests/test_rnnt_gpu.py asserts: rtol 2e-5 (atol 1e-4) on the costs, atol 3e-5 / rtol max(1e-3, 5e-5 (T + U1)) on the gradient."""
    B, T, U1, V = ref["x"].shape
    ok_c = np.allclose(np.asarray(out["costs"], np.float64), ref["costs"], rtol=2e-5, atol=1e-4)
    ok_g = np.allclose(np.asarray(out["dlogits"], np.float64)[..., :V], ref["grads"], atol=3e-5, rtol=max(1e-3, 5e-5 * (T + U1)))
    return bool(ok_c and ok_g)


@functools.lru_cache(maxsize=8)
def _case_cached(regime, B, T, U1, V, tlen, ulen, blank, seed, allowed):
    rng = np.random.default_rng([seed, B, T, U1, V, blank])
    tg = make_targets(rng, B, U1, V, blank, allowed)
    lg = make_logits(regime, B, T, U1, V, tg, tlen, ulen, blank, seed)
    gs = (0.75 + 0.5 * np.arange(B)).astype(np.float32) * np.where(np.arange(B) % 2, -1, 1).astype(np.float32)
    inputs = (lg, tg, np.asarray(tlen, np.int32), np.asarray(ulen, np.int32), blank, V, gs)
    ref = planes64(lg, tg, tlen, ulen, blank, V, gs)
    return inputs, ref, tolerances(inputs, ref)


def case(regime, B, T, U1, V, tlen, ulen, blank=0, seed=0, allowed=None):
    """(inputs, planes64, tolerances) of a deterministic case; computed once and shared (treat them as read-only)."""
    return _case_cached(regime, B, T, U1, V, tuple(int(v) for v in tlen), tuple(int(v) for v in ulen), blank, seed,
                        None if allowed is None else tuple(allowed))


# planted defects (tests/test_rnnt_lattice_ref_cpu.py): kind -> what it restates
DEFECTS = ("alpha_cell", "left_inf", "left_stale", "lpe_in_shift", "blank_neighbour", "beta_seed_zero", "stale_operands", "miss_gemit")
