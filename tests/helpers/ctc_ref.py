"""CTC in float64, written for this project's tests: the log-space lattice DP (costs, alpha, beta, posterior occupancy, gradient w.r.t. the
RAW per-frame scores) and a brute-force enumerator over all V^T frame labellings that the DP is checked against.

Conventions (include/tsasr_hip.h, "Auxiliary CTC loss"): x [B,T,V] raw scores, normalised per row here; T_b = clamp(tlen[b], 1, T),
U_b = clamp(ulen[b], 0, U); target ids clamped into [0, V-1]; extended states s = 0 .. 2 U_b: even = blank, odd s = label (s-1)/2;
alpha(t,s) and beta(t,s) BOTH include the emission of frame t, so occupancy(t,s) = exp(alpha + beta - lp(t,s) - log P). An infeasible
utterance (no path: T_b < U_b + adjacent repeats) has cost 0 and a zero gradient (torch's zero_infinity=True)."""
import itertools

import numpy as np

NEG = -np.inf


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _lse(*xs):
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.maximum.reduce(xs)
        ms = np.where(np.isfinite(m), m, 0.0)
        return np.where(np.isfinite(m), ms + np.log(sum(np.exp(x - ms) for x in xs)), NEG)


def lengths(tlen, ulen, T, U):
    return np.clip(np.asarray(tlen, np.int64), 1, T), np.clip(np.asarray(ulen, np.int64), 0, U)


def ctc_one(lp, y, blank):
    """lp [Tb,V] float64 log-probs, y [Ub] ids. Returns (cost, feasible, alpha [Tb,S], beta [Tb,S], occ [Tb,V])."""
    Tb, V = lp.shape
    Ub = len(y)
    S = 2 * Ub + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = y
    skip = np.zeros(S, bool)
    if Ub > 1:
        skip[3::2] = y[1:] != y[:-1]
    e = lp[:, ext]                                    # [Tb,S]
    alpha = np.full((Tb, S), NEG)
    alpha[0, 0] = e[0, 0]
    if S > 1:
        alpha[0, 1] = e[0, 1]
    pad = np.full(2, NEG)
    for t in range(1, Tb):
        a = np.concatenate([pad, alpha[t - 1]])
        alpha[t] = _lse(a[2:], a[1:-1], np.where(skip, a[:-2], NEG)) + e[t]
    beta = np.full((Tb, S), NEG)
    beta[Tb - 1, S - 1] = e[Tb - 1, S - 1]
    if S > 1:
        beta[Tb - 1, S - 2] = e[Tb - 1, S - 2]
    skipf = np.concatenate([skip[2:], np.zeros(2, bool)])[:S]  # s -> s + 2 allowed
    for t in range(Tb - 2, -1, -1):
        b = np.concatenate([beta[t + 1], pad])
        beta[t] = _lse(b[:-2], b[1:-1], np.where(skipf, b[2:], NEG)) + e[t]
    logp = _lse(alpha[Tb - 1, S - 1], alpha[Tb - 1, S - 2] if S > 1 else np.float64(NEG))
    occ = np.zeros((Tb, V))
    if not np.isfinite(logp):
        return 0.0, False, alpha, beta, occ
    with np.errstate(invalid="ignore"):
        post = np.exp(alpha + beta - e - logp)       # -inf - -inf never occurs where e is finite
    post = np.where(np.isfinite(alpha) & np.isfinite(beta), post, 0.0)
    for s in range(S):                               # fixed order, float64: the order does not matter at the tests' tolerances
        occ[:, ext[s]] += post[:, s]
    return float(-logp), True, alpha, beta, occ


def ctc_ref(x, targets, tlen, ulen, blank=0, gscale=None):
    """x [B,T,V] (any float dtype, upcast), targets [B,>=U]. Returns a dict: costs [B], feasible [B], grad [B,T,V] (= gscale * d cost / d x,
    zero on rows t >= T_b), occ [B,T,V], alpha / beta (lists of [T_b,S_b] arrays)."""
    x = np.asarray(x, np.float64)
    B, T, V = x.shape
    targets = np.asarray(targets, np.int64).reshape(B, -1)
    tl, ul = lengths(tlen, ulen, T, targets.shape[1])
    g = np.ones(B) if gscale is None else np.asarray(gscale, np.float64)
    out = dict(costs=np.zeros(B), feasible=np.zeros(B, bool), grad=np.zeros((B, T, V)), occ=np.zeros((B, T, V)), alpha=[], beta=[])
    for b in range(B):
        lp = log_softmax(x[b, :tl[b]])
        y = np.clip(targets[b, :ul[b]], 0, V - 1)
        cost, ok, al, be, occ = ctc_one(lp, y, blank)
        out["costs"][b], out["feasible"][b] = cost, ok
        out["alpha"].append(al)
        out["beta"].append(be)
        if ok:
            out["occ"][b, :tl[b]] = occ
            out["grad"][b, :tl[b]] = g[b] * (np.exp(lp) - occ)
    return out


def collapse(path, blank):
    """The CTC map: merge repeats, drop blanks."""
    return [k for k, _ in itertools.groupby(path) if k != blank]


def brute_force(x, y, blank=0):
    """-log of the total probability of all V^T frame labellings of x [T,V] that collapse to y (0.0 and False when there is none)."""
    lp = log_softmax(x)
    T, V = lp.shape
    y = list(int(k) for k in y)
    terms = [sum(lp[t, k] for t, k in enumerate(path)) for path in itertools.product(range(V), repeat=T) if collapse(path, blank) == y]
    if not terms:
        return 0.0, False
    m = max(terms)
    return float(-(m + np.log(sum(np.exp(v - m) for v in terms)))), True


def greedy_ref(x, tlen, blank=0):
    """speechbrain.decoders.ctc.ctc_greedy_decode on absolute lengths: argmax per frame (first maximum), collapse, drop blanks."""
    x = np.asarray(x, np.float64)
    return [collapse(list(np.argmax(x[b, :max(0, min(int(tlen[b]), x.shape[1]))], -1)), blank) for b in range(x.shape[0])]
