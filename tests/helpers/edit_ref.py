"""The project's own host restatement of the edit-distance rule csrc/editdist.hip implements (NumPy, test infrastructure only): costs of
the whole lattice row by row, the operation of every cell from its three neighbouring costs with the reference's comparison order
(substitution / match only if strictly cheaper than both others, else the deletion if strictly cheaper than the insertion, else the
insertion; row 0 insertions, column 0 deletions), then the walk back from (n, m). tests/test_wer_cpu.py pins it to
tests/golden/wer_cases.npz (the reference's own results) before any GPU test relies on it for sizes the golden file does not hold."""
import numpy as np

EQ, SUB, DEL, INS = "=", "S", "D", "I"


def cost_table(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    n, m = len(a), len(b)
    cols = np.arange(m + 1, dtype=np.int64)
    D = np.empty((n + 1, m + 1), np.int64)
    D[0] = cols
    for i in range(1, n + 1):
        best = np.minimum(D[i - 1, :-1] + (b != a[i - 1]), D[i - 1, 1:] + 1)          # substitution / match or deletion, columns 1..m
        # the insertion chain: D[i, j] = min over k <= j of (candidate[k] + (j - k)), candidate[0] = i (column 0: deletions)
        D[i] = np.minimum.accumulate(np.concatenate([[i], best]) - cols) + cols
    return D


def op_codes(a, b, D=None):
    """uint8 [n+1, m+1] of ASCII operation codes; row 0 'I', column 0 'D', (0, 0) '='."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    D = cost_table(a, b) if D is None else D
    n, m = len(a), len(b)
    T = np.full((n + 1, m + 1), ord(EQ), np.uint8)
    T[0, :] = ord(INS)
    T[:, 0] = ord(DEL)
    T[0, 0] = ord(EQ)
    if n and m:
        ne = a[:, None] != b[None, :]
        sc, dc, ic = D[:-1, :-1] + ne, D[:-1, 1:] + 1, D[1:, :-1] + 1
        take_s = (sc < ic) & (sc < dc)
        take_d = ~take_s & (dc < ic)
        T[1:, 1:] = np.where(take_s, np.where(ne, ord(SUB), ord(EQ)), np.where(take_d, ord(DEL), ord(INS)))
    return T


def edit_ops(a, b):
    """-> ([edits, insertions, deletions, substitutions], alignment [(op, i or None, j or None), ...] in forward order)."""
    T = op_codes(a, b)
    i, j = len(a), len(b)
    out, cnt = [], {INS: 0, DEL: 0, SUB: 0, EQ: 0}
    while i or j:
        op = INS if i == 0 else DEL if j == 0 else chr(T[i, j])
        cnt[op] += 1
        if op == INS:
            j -= 1
            out.append((INS, None, j))
        elif op == DEL:
            i -= 1
            out.append((DEL, i, None))
        else:
            i, j = i - 1, j - 1
            out.append((op, i, j))
    out.reverse()
    return [cnt[INS] + cnt[DEL] + cnt[SUB], cnt[INS], cnt[DEL], cnt[SUB]], out


def error_rate(refs, hyps):
    """100 * edits / reference tokens over a list of pairs (the summary's WER)."""
    edits = sum(edit_ops(r, h)[0][0] for r, h in zip(refs, hyps))
    tokens = sum(len(r) for r in refs)
    return 100.0 * edits / tokens if tokens else 0.0


# ---- readers of tests/golden/wer_cases.npz (tools/gen_golden_wer.py) ----------------------------------------------------------
def _ragged(flat, off):
    return [flat[int(off[k]):int(off[k + 1])].tolist() for k in range(len(off) - 1)]


def golden_alignments(g, prefix=""):
    off = g[prefix + "align_off"]
    ops, ai, aj = g[prefix + "align_op"], g[prefix + "align_i"], g[prefix + "align_j"]
    return [[(chr(o), None if i < 0 else int(i), None if j < 0 else int(j)) for o, i, j in
             zip(ops[int(off[k]):int(off[k + 1])], ai[int(off[k]):int(off[k + 1])], aj[int(off[k]):int(off[k + 1])])] for k in range(len(off) - 1)]


def golden_pairs(g, prefix=""):
    """-> (refs, hyps, counts, alignments) of the pair set `prefix` ("" = all pairs, "wer_" / "cer_" = what the statistics objects scored)."""
    return (_ragged(g[prefix + "ref_sym"], g[prefix + "ref_off"]), _ragged(g[prefix + "hyp_sym"], g[prefix + "hyp_off"]),
            g[prefix + "counts"].tolist(), golden_alignments(g, prefix))


def golden_details(g, name):
    """The reference's per-utterance dicts of the statistics object `name` ("wer" / "cer"), rebuilt from the recorded arrays."""
    p = name + "_"
    vocab = [str(v) for v in g[p + "vocab"]]
    refs, hyps, counts, alis = golden_pairs(g, p)
    ids = [str(g["ids"][k]) for k in g[p + "pairs"]]
    return [{"key": key, "scored": True, "hyp_absent": False, "hyp_empty": bool(he), "num_edits": c[0], "num_ref_tokens": int(nref),
             "WER": float(w), "insertions": c[1], "deletions": c[2], "substitutions": c[3], "alignment": ali,
             "ref_tokens": [vocab[t] for t in r], "hyp_tokens": [vocab[t] for t in h]}
            for key, r, h, c, ali, nref, w, he in zip(ids, refs, hyps, counts, alis, g[p + "num_ref_tokens"], g[p + "utt_wer"], g[p + "hyp_empty"])]


def golden_summary(g, name):
    return {str(k): float(v) for k, v in zip(g[name + "_summary_keys"], g[name + "_summary_vals"])}


def golden_words(g, name="wer"):
    """(ids, hypothesis word lists, reference word lists) as the generator appended them to the statistics objects."""
    words = [str(w) for w in g["words"]]
    refs, hyps, _, _ = golden_pairs(g)
    use = [int(k) for k in g[name + "_pairs"]]
    return [str(g["ids"][k]) for k in use], [[words[t] for t in hyps[k]] for k in use], [[words[t] for t in refs[k]] for k in use]
