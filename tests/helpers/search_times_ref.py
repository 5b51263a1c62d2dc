"""Float64 reference for the emission frames a transducer search reports (numpy only).

A hypothesis y_1..y_n with frames f_1 <= ... <= f_n is ONE path through the RNN-T lattice: at frame t the tokens with f_i = t are
emitted, then the frame's single blank. Its log-probability is therefore a function of (tokens, frames) alone,

    path_logp = sum_i lp(f_i, i-1, y_i) + sum_{t<T} lp(t, #{i: f_i <= t}, blank),
    lp(t, u, .) = log_softmax(head(LeakyReLU(enc[t] + pn_u))),   pn_u = proj(LSTM(emb(blank, y_1..y_u)))[u],

and a beam search that never merges paths reports exactly this number as logp (score x (n + 1)); a frame list that is off by one frame
anywhere gives another number. ``weights``: float64 copies of whatever the kernel read, keys emb [n_emb, E], w_ih [4H, E], w_hh [4H, H],
b_ih, b_hh [4H] (or None), w_proj [J, H], b_proj [J] (or None), w_head [V, J], b_head [V] (or None); torch's LSTM gate order i, f, g, o.
"""
import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def predictor_outputs(tokens, weights, blank):
    """pn [n + 1, J] float64: row u = the projected predictor output after blank, y_1..y_u (row 0: primed with blank alone)."""
    w = {k: (None if v is None else np.asarray(v, np.float64)) for k, v in weights.items()}
    H = w["w_hh"].shape[1]
    h, c = np.zeros(H), np.zeros(H)
    rows = []
    for tok in [int(blank)] + [int(t) for t in tokens]:
        g = w["w_ih"] @ w["emb"][tok] + w["w_hh"] @ h
        for b in (w.get("b_ih"), w.get("b_hh")):
            if b is not None:
                g = g + b
        i, f, gg, o = _sigmoid(g[:H]), _sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sigmoid(g[3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        pn = w["w_proj"] @ h
        if w.get("b_proj") is not None:
            pn = pn + w["b_proj"]
        rows.append(pn)
    return np.stack(rows)


def joint_logits(enc_t, pn_u, weights, slope):
    """head(LeakyReLU(enc_t + pn_u)) [V] float64 (before the log-softmax)."""
    z = np.asarray(enc_t, np.float64) + pn_u
    z = np.where(z > 0, z, z * float(slope))
    out = np.asarray(weights["w_head"], np.float64) @ z
    if weights.get("b_head") is not None:
        out = out + np.asarray(weights["b_head"], np.float64)
    return out


def log_softmax(v):
    m = v.max()
    return v - m - np.log(np.exp(v - m).sum())


def lp_lattice(enc, tokens, weights, blank, slope):
    """lp [T, n + 1, V] float64: lp[t, u] = log_softmax over the symbols at frame t after u tokens."""
    pn = predictor_outputs(tokens, weights, blank)
    z = np.asarray(enc, np.float64)[:, None, :] + pn[None, :, :]
    z = np.where(z > 0, z, z * float(slope))
    lg = z @ np.asarray(weights["w_head"], np.float64).T
    if weights.get("b_head") is not None:
        lg = lg + np.asarray(weights["b_head"], np.float64)
    m = lg.max(-1, keepdims=True)
    return lg - m - np.log(np.exp(lg - m).sum(-1, keepdims=True))


def path_logp_from_lattice(lp, tokens, frames, blank):
    """(path_logp, label sum) of the path (tokens, frames) on a lattice lp [T, n + 1, V] (lp_lattice)."""
    T, n = lp.shape[0], len(tokens)
    fr = [int(f) for f in frames]
    if len(fr) != n or any(f < 0 or f >= T for f in fr) or any(b < a for a, b in zip(fr, fr[1:])):
        raise ValueError(f"frames {fr} are no non-decreasing list of {n} frames below {T}")
    labels = sum(lp[fr[i], i, int(tokens[i])] for i in range(n))
    emitted = np.searchsorted(np.asarray(fr, np.int64), np.arange(T), side="right")      # #{i: f_i <= t}
    blanks = sum(lp[t, int(emitted[t]), int(blank)] for t in range(T))
    return float(labels + blanks), float(labels)


def path_logp(enc, tokens, frames, weights, blank, slope):
    """(path_logp, label sum) in float64 of hypothesis ``tokens`` emitted at ``frames`` over enc [T, J]; see the module docstring."""
    return path_logp_from_lattice(lp_lattice(np.asarray(enc, np.float64), tokens, weights, blank, slope), tokens, frames, blank)
