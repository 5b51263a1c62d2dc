"""float64 numpy restatement of forced alignment on the RNN-T lattice (csrc/rnnt.hip rnnt_viterbi_kernel), for the tests.

    delta(0,0) = 0,  delta(t,u) = max(delta(t-1,u) + lp[t-1,u,blank], delta(t,u-1) + lp[t,u-1,targets[u-1]])
    score = delta(T-1, U) + lp[T-1, U, blank]

Tie rule: equal candidates -> the blank predecessor (from t-1) wins. frames[u] = frame at which label u is emitted.
"""
import itertools

import numpy as np


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def viterbi(lp, targets, T, U, blank=0, return_gap=False):
    """lp [>=T, >=U+1, V] float64 log-probabilities of ONE utterance -> (frames int64 [U], score). With return_gap also the smallest
    |difference| between the two candidates over the nodes of the backtrace that have two predecessors (inf when there is none)."""
    targets = np.asarray(targets)
    lpb = np.asarray(lp[:T, :U + 1, blank], np.float64)
    lpl = np.asarray(lp[:T, np.arange(U), targets[:U]], np.float64) if U else np.zeros((T, 0))      # [T, U]: label u at (t, u)
    d = np.full((T, U + 1), -np.inf)
    lab = np.zeros((T, U + 1), bool)
    gapm = np.full((T, U + 1), np.inf)
    d[0, 0] = 0.0
    for n in range(1, T + U):            # anti-diagonal t + u = n: every cell depends on diagonal n - 1 only (the arithmetic of the cell loop)
        t = np.arange(max(0, n - U), min(T - 1, n) + 1)
        u = n - t
        tm, um = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
        ne = np.where(t > 0, d[tm, u] + lpb[tm, u], -np.inf)
        em = np.where(u > 0, d[t, um] + (lpl[t, um] if U else 0.0), -np.inf)
        lab[t, u] = em > ne
        d[t, u] = np.where(em > ne, em, ne)
        both = (t > 0) & (u > 0)
        gapm[t[both], u[both]] = np.abs(em[both] - ne[both])
    frames = np.zeros(U, np.int64)
    t, u, gap = T - 1, U, np.inf
    while t > 0 or u > 0:
        gap = min(gap, gapm[t, u])
        if lab[t, u]:
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    score = d[T - 1, U] + lp[T - 1, U, blank]
    return (frames, score, gap) if return_gap else (frames, score)


def path_score(lp, targets, frames, T, U, blank=0):
    """float64 score of the path that emits label u at frames[u]; asserts the path is valid (non-decreasing, 0 <= f < T)."""
    frames = np.asarray(frames[:U], np.int64)
    assert frames.shape == (U,)
    assert np.all(frames >= 0) and np.all(frames < T), frames
    assert np.all(np.diff(frames) >= 0), frames
    targets = np.asarray(targets)
    s = float(np.sum(lp[frames, np.arange(U), targets[:U]], dtype=np.float64)) if U else 0.0
    # blanks: frame t is left through column u(t) = number of labels emitted at frames <= t
    cols = np.searchsorted(frames, np.arange(T), side="right")
    s += float(np.sum(lp[np.arange(T), cols, blank], dtype=np.float64))
    return s


def brute_force(lp, targets, T, U, blank=0):
    """Every monotone path of a tiny lattice: (best frames, best score, sorted list of all (score, frames)). Equal scores: the path whose
    (f_{U-1}, ..., f_0) is lexicographically smallest, as the tie rule gives."""
    allp = []
    for fr in itertools.combinations_with_replacement(range(T), U):
        allp.append((path_score(lp, targets, np.array(fr, np.int64), T, U, blank), fr))
    best = max(s for s, _ in allp)
    cands = [fr for s, fr in allp if s == best]
    fr = min(cands, key=lambda f: tuple(reversed(f)))
    return np.array(fr, np.int64), best, sorted(allp, reverse=True)


def planted(rng, logits, targets, tlen, ulen, boost, blank=0):
    """Plants one path per utterance into `logits` [B,T,U1,V] (in place): fr = sort(rng.integers(0, T_b, U_b)); `boost` is added to the
    label logit at each (fr[u], u) and to the blank logit at the cell where the path leaves each frame. Returns the list of fr."""
    out = []
    for b in range(logits.shape[0]):
        Tb, Ub = int(tlen[b]), int(ulen[b])
        fr = np.sort(rng.integers(0, Tb, size=Ub)).astype(np.int64)
        for u in range(Ub):
            logits[b, fr[u], u, targets[b, u]] += boost
        cols = np.searchsorted(fr, np.arange(Tb), side="right")
        for t in range(Tb):
            logits[b, t, cols[t], blank] += boost
        out.append(fr)
    return out
