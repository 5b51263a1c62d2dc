#!/usr/bin/env python3
"""Golden WER / CER cases from the reference's own scorer (TEST INFRASTRUCTURE; runs ONLY where the reference is present).

Imports speechbrain's edit_distance / ErrorRateStats through the stubs of oracle/gen_golden.py and writes tests/golden/wer_cases.npz:
  pairs  - 300 seeded random pairs (alphabet 6, reference lengths 0-39, 40 % token noise: drop / replace / insert in equal parts) and
           five special ones ([""] against [""], an empty hypothesis, a single-token pair, two identical sequences, an empty reference),
           each with the counts and the alignment of op_table -> count_ops / alignment;
  stats  - the pairs with a non-empty reference through an ErrorRateStats() (word level) and an ErrorRateStats(split_tokens=True)
           (character level): per-utterance details, the summarize() dicts and the write_stats text;
  long   - one 1920-token pair (alphabet 28).
Only arrays and recorded text are stored. The generator refuses to write a file in which fewer than 50 random pairs get a different
insertion / deletion / substitution split under a "substitution wins ties" rule than under the reference's: the path choice must matter.

Run:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tools/gen_golden_wer.py
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import gen_golden as G  # noqa: E402

WORDS = ["", "a", "bb", "ccc", "dd", "e", "ffff"]      # index 0 (the empty word) appears only in the [""] / [""] pair
CODE = {"=": 0, "S": 1, "D": 2, "I": 3}


def random_pairs(n_pairs=300, alphabet=6, max_len=39, noise=0.4, seed=2024):
    rng = np.random.RandomState(seed)
    pairs = []
    for _ in range(n_pairs):
        ref = rng.randint(1, alphabet + 1, rng.randint(0, max_len + 1)).tolist()
        hyp = []
        for tok in ref:
            if rng.rand() >= noise:
                hyp.append(tok)
                continue
            kind = rng.randint(3)
            if kind == 1:
                hyp.append(int(rng.randint(1, alphabet + 1)))
            elif kind == 2:
                hyp += [tok, int(rng.randint(1, alphabet + 1))]
        pairs.append((ref, hyp))
    return pairs


def substitution_first_split(a, b):
    """(ins, del, sub) of the walk back when a tie goes to the substitution / match, then the deletion - NOT the reference's rule."""
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        D[i][0] = i
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    i, j, ins, dele, sub = n, m, 0, 0, 0
    while i or j:
        if i and j and D[i][j] == D[i - 1][j - 1] + (a[i - 1] != b[j - 1]):
            sub += a[i - 1] != b[j - 1]
            i, j = i - 1, j - 1
        elif i and D[i][j] == D[i - 1][j] + 1:
            dele, i = dele + 1, i - 1
        else:
            ins, j = ins + 1, j - 1
    return ins, dele, sub


def ragged(seqs, dtype=np.int32):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    flat = np.fromiter((x for s in seqs for x in s), dtype, int(off[-1]))
    return flat, off


def pack_alignments(alis):
    op, off = ragged([[ord(o) for o, _, _ in a] for a in alis], np.uint8)
    ai, _ = ragged([[-1 if i is None else i for _, i, _ in a] for a in alis])
    aj, _ = ragged([[-1 if j is None else j for _, _, j in a] for a in alis])
    return op, ai, aj, off


def main():
    G.import_reference()
    from speechbrain.utils import edit_distance as ED
    from speechbrain.utils.metric_stats import ErrorRateStats

    def score(a, b):
        table = ED.op_table(a, b)
        c = ED.count_ops(table)
        return [sum(c.values()), c["insertions"], c["deletions"], c["substitutions"]], ED.alignment(table)

    rnd = random_pairs()
    differ = 0
    for a, b in rnd:
        cnt, _ = score(a, b)
        alt = substitution_first_split(a, b)
        assert sum(alt) == cnt[0], "both rules give a shortest path"
        differ += tuple(cnt[1:]) != alt
    print(f"{differ} of {len(rnd)} random pairs split their edits differently under a substitution-first rule")
    assert differ >= 50, differ
    special = [([0], [0]), ([1, 2, 3, 2], []), ([5], [4]), ([1, 2, 3, 4, 5, 6, 1, 2], [1, 2, 3, 4, 5, 6, 1, 2]), ([], [3, 3, 1])]
    pairs = rnd + special
    ids = [f"utt{k:03d}" for k in range(len(rnd))] + ["both-empty-word", "empty-hyp", "single-token", "identical", "empty-ref"]
    out = {"words": np.array(WORDS), "ids": np.array(ids), "n_random": np.int64(len(rnd)), "n_path_choice_matters": np.int64(differ)}
    out["ref_sym"], out["ref_off"] = ragged([a for a, _ in pairs])
    out["hyp_sym"], out["hyp_off"] = ragged([b for _, b in pairs])
    scored = [score(a, b) for a, b in pairs]
    out["counts"] = np.array([c for c, _ in scored], np.int32)
    out["align_op"], out["align_i"], out["align_j"], out["align_off"] = pack_alignments([a for _, a in scored])

    # the statistics objects, over the pairs with a non-empty reference (the reference's scorer indexes ref_tokens[0])
    keep = [k for k, (a, _) in enumerate(pairs) if len(a)]
    for name, kwargs in (("wer", {}), ("cer", {"split_tokens": True})):
        use = [k for k in keep if not (name == "cer" and ids[k] == "both-empty-word")]      # split_word([""]) is an empty reference
        stats = ErrorRateStats(**kwargs)
        for lo in range(0, len(use), 32):
            part = use[lo:lo + 32]
            stats.append([ids[k] for k in part], [[WORDS[t] for t in pairs[k][1]] for k in part], [[WORDS[t] for t in pairs[k][0]] for k in part])
        summary = stats.summarize()
        text = io.StringIO()
        stats.write_stats(text)
        vocab = sorted({t for d in stats.scores for t in list(d["ref_tokens"]) + list(d["hyp_tokens"])})
        idx = {t: i for i, t in enumerate(vocab)}
        out[name + "_pairs"] = np.array(use, np.int64)
        out[name + "_vocab"] = np.array(vocab)
        out[name + "_ref_sym"], out[name + "_ref_off"] = ragged([[idx[t] for t in d["ref_tokens"]] for d in stats.scores])
        out[name + "_hyp_sym"], out[name + "_hyp_off"] = ragged([[idx[t] for t in d["hyp_tokens"]] for d in stats.scores])
        out[name + "_counts"] = np.array([[d["num_edits"], d["insertions"], d["deletions"], d["substitutions"]] for d in stats.scores], np.int32)
        out[name + "_num_ref_tokens"] = np.array([d["num_ref_tokens"] for d in stats.scores], np.int32)
        out[name + "_utt_wer"] = np.array([d["WER"] for d in stats.scores], np.float64)
        out[name + "_hyp_empty"] = np.array([d["hyp_empty"] for d in stats.scores], np.bool_)
        assert all(d["scored"] and d["hyp_absent"] is False for d in stats.scores)
        out[name + "_align_op"], out[name + "_align_i"], out[name + "_align_j"], out[name + "_align_off"] = pack_alignments(
            [d["alignment"] for d in stats.scores])
        keys = sorted(summary)
        out[name + "_summary_keys"] = np.array(keys)
        out[name + "_summary_vals"] = np.array([float(summary[k]) for k in keys], np.float64)
        out[name + "_text"] = np.frombuffer(text.getvalue().encode("utf-8"), np.uint8)
        print(name, {k: summary[k] for k in ("WER", "SER", "num_edits", "num_scored_tokens", "insertions", "deletions", "substitutions")})

    rng = np.random.RandomState(7)
    long_ref = rng.randint(1, 29, 1920).tolist()
    long_hyp = []
    for tok in long_ref:
        u = rng.rand()
        if u >= 0.25:
            long_hyp.append(tok)
        elif u < 0.08:
            long_hyp.append(int(rng.randint(1, 29)))
        elif u < 0.17:
            long_hyp += [tok, int(rng.randint(1, 29))]
    cnt, ali = score(long_ref, long_hyp)
    out["long_ref"], out["long_hyp"] = np.array(long_ref, np.int32), np.array(long_hyp, np.int32)
    out["long_counts"] = np.array(cnt, np.int32)
    out["long_align_op"], out["long_align_i"], out["long_align_j"], _ = pack_alignments([ali])
    print("long pair", len(long_ref), "x", len(long_hyp), "counts", cnt)
    path = os.path.join(ROOT, "tests", "golden", "wer_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
