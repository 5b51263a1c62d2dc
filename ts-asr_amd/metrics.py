"""WER / CER statistics with the reference's surface (SB/utils/metric_stats.py:196-358 ``ErrorRateStats``), scored on the device.

``append`` does the reference's token plumbing on the host (undo_padding, ind2lab, merge_char, split_word), interns the tokens to
int32, packs the batch into one pinned staging buffer, copies it without blocking and launches csrc/editdist.hip on the current
stream - it never synchronises. ``summarize`` reads the kernel's running totals once; ``scores`` (the reference's list of per-utterance
dicts, alignments included) is copied from the device when first asked for, and may be assigned (the recipe does after gathering the
ranks' lists): from then on ``summarize`` / ``write_stats`` work from the list alone, on the host. ``write_stats`` prints the
reference's text (SB/dataio/wer.py:15-198). There is no host scorer here: without a device ``append`` raises ``TsasrHipMissing``.
"""
import numpy as np
import torch

from . import _capi as C
from . import ops

OPS = {"eq": "=", "ins": "I", "del": "D", "sub": "S"}      # the reference's EDIT_SYMBOLS
_RING = 4                                                   # pinned staging buffers in flight per ErrorRateStats


# ---- the reference's token plumbing (SB/utils/data_utils.py:23-48, SB/dataio/dataio.py:1041-1138) -----------------------------
def undo_padding(batch, lengths):
    width = batch.shape[1]
    return [seq[:int(torch.round(rel * width))].tolist() for seq, rel in zip(batch, lengths)]


def merge_char(sequences, space="_"):
    return ["".join(seq).split(space) for seq in sequences]


def split_word(sequences, space="_"):
    return [list(space.join(seq)) for seq in sequences]


class CharTokenizer:
    """Stand-in with the call signature the recipe uses on its SentencePiece tokenizer, for a character vocabulary: piece i of
    ``pieces`` is a string, "▁" marks a word boundary. ``tokenizer(hyps, task="decode_from_list")`` -> one list of words per
    hypothesis (an empty hypothesis gives [""], as decoding to "" and splitting does). A test and demo aid, not a SentencePiece."""

    def __init__(self, pieces):
        self.pieces = list(pieces)

    def __call__(self, inputs, input_lens=None, task="decode_from_list"):
        if task != "decode_from_list":
            raise NotImplementedError(f"CharTokenizer: task {task!r}")
        texts = ("".join(self.pieces[int(i)] for i in seq).replace("▁", " ") for seq in inputs)
        return [t[1:].split(" ") if t.startswith(" ") else t.split(" ") for t in texts]


# ---- packing and the device call ----------------------------------------------------------------------------------------------
def pack_pairs(refs, hyps, ref_counts=None, out=None):
    """N pairs of int sequences -> (words int32 [3N + 2 + sum n + sum m] = ref_off | hyp_off | ref_count | ref_sym | hyp_sym,
    layout dict). ``out``: a callable n_words -> int32 numpy view to fill (the pinned buffer)."""
    N = len(refs)
    if N == 0 or len(hyps) != N:
        raise ValueError("pack_pairs: the reference and hypothesis batches must be non-empty and of the same size")
    n = np.fromiter((len(r) for r in refs), np.int64, N)
    m = np.fromiter((len(h) for h in hyps), np.int64, N)
    nr, nh = int(n.sum()), int(m.sum())
    words = 3 * N + 2 + nr + nh
    if words + 3 * N >= 2 ** 31:
        raise ValueError("pack_pairs: batch too large for int32 offsets")
    buf = out(words) if out is not None else np.empty(words, np.int32)
    o = 0
    buf[o] = 0
    np.cumsum(n, out=buf[o + 1:o + N + 1])
    o += N + 1
    buf[o] = 0
    np.cumsum(m, out=buf[o + 1:o + N + 1])
    o += N + 1
    buf[o:o + N] = n if ref_counts is None else np.asarray(ref_counts, np.int64)
    o += N
    if nr:
        buf[o:o + nr] = np.fromiter((s for r in refs for s in r), np.int64, nr)
    if nh:
        buf[o + nr:o + nr + nh] = np.fromiter((s for h in hyps for s in h), np.int64, nh)
    lay = dict(N=N, n=n, m=m, nr=nr, nh=nh, max_ref=int(n.max()), max_hyp=int(m.max()), cells=int(((n + 1) * (m + 1)).sum()))
    return buf, lay


def launch_packed(dev_words, lay, totals=None, workspace=None):
    """The kernel over a packed batch already on the device (pack_pairs layout). No synchronisation."""
    N, nr, nh = lay["N"], lay["nr"], lay["nh"]
    o = 2 * N + 2
    return ops.edit_distance(dev_words[o + N:o + N + nr], dev_words[0:N + 1], dev_words[o + N + nr:o + N + nr + nh], dev_words[N + 1:o],
                             dev_words[o:o + N], lay["max_ref"], lay["max_hyp"], lay["cells"], totals=totals, workspace=workspace)


def read_pairs(res, lay):
    """One batch's device results as host lists: per pair (counts [4], alignment [(op, i or None, j or None), ...])."""
    counts = res.counts.cpu().numpy()
    lens = res.align_len.cpu().numpy()
    aop, ai, aj = res.align_op.cpu().numpy(), res.align_i.cpu().numpy(), res.align_j.cpu().numpy()
    base = np.concatenate([[0], np.cumsum(lay["n"] + lay["m"])])
    out = []
    for k in range(lay["N"]):
        if counts[k, 0] < 0:
            raise C.TsasrHipError(f"edit distance: pair {k} was refused by the kernel (lengths {lay['n'][k]}, {lay['m'][k]})")
        s = slice(int(base[k]), int(base[k]) + int(lens[k]))
        ops_k = aop[s].tobytes().decode("ascii")
        out.append((counts[k].tolist(), [(c, None if i < 0 else i, None if j < 0 else j) for c, i, j in zip(ops_k, ai[s].tolist(), aj[s].tolist())]))
    return out


def score_pairs(refs, hyps, ref_counts=None, device=None, totals=None, workspace=None):
    """Convenience for tools and tests: pack on the host (pageable memory), copy, launch, read back. Synchronises."""
    if not torch.cuda.is_available():
        raise C.TsasrHipMissing("edit distance runs on an MI355X; there is no host scorer")
    buf, lay = pack_pairs(refs, hyps, ref_counts)
    dev = torch.from_numpy(buf).to(device or "cuda")
    res = launch_packed(dev, lay, totals=totals, workspace=workspace)
    return read_pairs(res, lay), res, lay


# ---- summary and text, from a list of per-utterance dicts (host) --------------------------------------------------------------
def wer_summary(details):
    s = dict.fromkeys(("num_edits", "num_scored_tokens", "num_erraneous_sents", "num_scored_sents", "num_absent_sents", "num_ref_sents",
                       "insertions", "deletions", "substitutions"), 0)
    for d in details:
        s["num_ref_sents"] += 1
        s["num_absent_sents"] += bool(d["hyp_absent"])
        if not d["scored"]:
            continue
        s["num_scored_sents"] += 1
        s["num_scored_tokens"] += d["num_ref_tokens"]
        s["num_erraneous_sents"] += d["num_edits"] > 0
        for key in ("num_edits", "insertions", "deletions", "substitutions"):
            s[key] += d[key]
    return _rates(s)


def _rates(s):
    wer = 100.0 * s["num_edits"] / s["num_scored_tokens"] if s["num_scored_tokens"] != 0 else 0.0
    ser = 100.0 * s["num_erraneous_sents"] / s["num_scored_sents"]      # no scored sentence: ZeroDivisionError, as the reference
    order = ("num_edits", "num_scored_tokens", "num_erraneous_sents", "num_scored_sents", "num_absent_sents", "num_ref_sents",
             "insertions", "deletions", "substitutions")
    return {"WER": wer, "SER": ser, **{k: int(s[k]) for k in order}}


def _alignment_lines(alignment, a, b, empty="<eps>", sep=" ; "):
    cols = []
    for op, i, j in alignment:
        cell = (empty if i is None else str(a[i]), str(op), empty if j is None else str(b[j]))
        width = max(len(c) for c in cell)
        cols.append([c.center(width) for c in cell])
    return [sep.join(c[row] for c in cols) for row in range(3)]


def write_wer_text(summary, details, out):
    """The reference's print_wer_summary + print_alignments (SB/dataio/wer.py) text."""
    bar = "=" * 80
    counts = "{insertions} ins, {deletions} del, {substitutions} sub ]"
    partial = " [PARTIAL]" if summary["num_scored_sents"] < summary["num_ref_sents"] else ""
    lines = [("%WER {WER:.2f} [ {num_edits} / {num_scored_tokens}, " + counts).format(**summary) + partial,
             "%SER {SER:.2f} [ {num_erraneous_sents} / {num_scored_sents} ]".format(**summary),
             "Scored {num_scored_sents} sentences, {num_absent_sents} not present in hyp.".format(**summary),
             bar, "ALIGNMENTS", "", "Format:", "<utterance-id>, WER DETAILS"]
    lines += _alignment_lines([("I", None, 0), ("S", 0, 1), ("=", 1, 2), ("=", 2, 3), ("S", 3, 4), ("D", 4, None)],
                              ["reference", "on", "the", "first", "line"], ["and", "hypothesis", "on", "the", "third"])
    for d in details:
        if d["scored"]:
            lines += [bar, ("{key}, %WER {WER:.2f} [ {num_edits} / {num_ref_tokens}, " + counts).format(**d)]
            lines += _alignment_lines(d["alignment"], d["ref_tokens"], d["hyp_tokens"])
    out.write("\n".join(lines) + "\n")


# ---- the statistics object ----------------------------------------------------------------------------------------------------
class ErrorRateStats:
    def __init__(self, merge_tokens=False, split_tokens=False, space_token="_", keep_values=True, extract_concepts_values=False,
                 tag_in="", tag_out=""):
        if extract_concepts_values:
            raise NotImplementedError("ErrorRateStats(extract_concepts_values=True) is outside the recipes (SURVEY.md section 2)")
        self.merge_tokens, self.split_tokens, self.space_token = merge_tokens, split_tokens, space_token
        self.keep_values, self.extract_concepts_values, self.tag_in, self.tag_out = keep_values, extract_concepts_values, tag_in, tag_out
        self._vocab = {}
        self._ring = [[None, None] for _ in range(_RING)]      # [pinned int32 tensor, event of its last copy]
        self._turn = 0
        self._workspace = None
        self.clear()

    def clear(self):
        self.ids, self.summary = [], {}
        self._scores, self._pending, self._assigned, self._totals = [], [], False, None

    # -- device side --
    def _staging(self, words):
        slot = self._ring[self._turn % _RING]
        self._turn += 1
        if slot[1] is not None:
            slot[1].synchronize()          # the copy out of this buffer has completed: it may be overwritten
        if slot[0] is None or slot[0].numel() < words:
            slot[0] = torch.empty(max(words, 2 * (slot[0].numel() if slot[0] is not None else 0)), dtype=torch.int32, pin_memory=True)
        return slot

    def _launch(self, ids, refs, hyps, ref_counts, ref_tokens, hyp_tokens):
        if not torch.cuda.is_available():
            raise C.TsasrHipMissing("ErrorRateStats scores on an MI355X (csrc/editdist.hip); there is no host scorer")
        C.lib()
        dev = torch.device("cuda", torch.cuda.current_device())
        slot = []

        def pinned(words):
            slot.append(self._staging(words))
            return slot[0][0].numpy()[:words]
        buf, lay = pack_pairs(refs, hyps, ref_counts, out=pinned)
        words = buf.shape[0]
        dev_words = torch.empty(words, dtype=torch.int32, device=dev)
        dev_words.copy_(slot[0][0][:words], non_blocking=True)
        slot[0][1] = torch.cuda.Event()
        slot[0][1].record()
        if self._totals is None:
            self._totals = torch.zeros(8, dtype=torch.int64, device=dev)
        need = ops.edit_distance_workspace_bytes(lay["N"], lay["cells"])
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)      # launches of one stream run in order: one workspace
        res = launch_packed(dev_words, lay, totals=self._totals, workspace=self._workspace)
        self._pending.append((list(ids), res, lay, dev_words, ref_tokens, hyp_tokens, list(ref_counts)))
        if self._assigned:
            self._materialise()

    def _materialise(self):
        for ids, res, lay, _, ref_tokens, hyp_tokens, ref_counts in self._pending:
            for key, (cnt, ali), ref, hyp, nref in zip(ids, read_pairs(res, lay), ref_tokens, hyp_tokens, ref_counts):
                wer = 100.0 * cnt[0] / len(ref) if len(ref) else (0.0 if cnt[0] == 0 else float("inf"))
                self._scores.append({"key": key, "scored": True, "hyp_absent": False, "hyp_empty": len(hyp) == 0, "num_edits": cnt[0],
                                     "num_ref_tokens": nref, "WER": wer, "insertions": cnt[1], "deletions": cnt[2],
                                     "substitutions": cnt[3], "alignment": ali, "ref_tokens": ref, "hyp_tokens": hyp})
        self._pending = []

    @property
    def scores(self):
        if self._pending:
            self._materialise()
        return self._scores

    @scores.setter
    def scores(self, value):
        self._scores, self._pending, self._assigned = list(value), [], True

    # -- the reference's surface --
    def append(self, ids, predict, target, predict_len=None, target_len=None, ind2lab=None):
        if predict_len is not None:
            predict = undo_padding(predict, predict_len)
        if target_len is not None:
            target = undo_padding(target, target_len)
        if ind2lab is not None:
            predict, target = ind2lab(predict), ind2lab(target)
        if self.merge_tokens:
            predict, target = merge_char(predict, space=self.space_token), merge_char(target, space=self.space_token)
        if self.split_tokens:
            predict, target = split_word(predict, space=self.space_token), split_word(target, space=self.space_token)
        if torch.is_tensor(predict):
            predict = predict.tolist()
        if torch.is_tensor(target):
            target = target.tolist()
        if len(ids) != len(predict) or len(ids) != len(target):
            raise ValueError("The reference and hypothesis batches are not of the same size")
        intern = self._vocab
        refs = [[intern.setdefault(tok, len(intern)) for tok in seq] for seq in target]
        hyps = [[intern.setdefault(tok, len(intern)) for tok in seq] for seq in predict]
        # the reference's `[""]` against `[""]` case: scored, but no reference token counted (SB/utils/edit_distance.py:483-486)
        counts = [0 if (len(r) and len(h) and r[0] == "" and h[0] == "") else len(r) for r, h in zip(target, predict)]
        self._launch(ids, refs, hyps, counts, list(target), list(predict))
        self.ids.extend(ids)

    def append_ids(self, ids, predict_ids, target_ids):
        """Lists of int lists (token ids): scored as they are, no interning; the tokens reported are the ids."""
        predict_ids, target_ids = [list(map(int, p)) for p in predict_ids], [list(map(int, t)) for t in target_ids]
        if len(ids) != len(predict_ids) or len(ids) != len(target_ids):
            raise ValueError("The reference and hypothesis batches are not of the same size")
        self._launch(ids, target_ids, predict_ids, [len(t) for t in target_ids], target_ids, predict_ids)
        self.ids.extend(ids)

    def summarize(self, field=None):
        if self._assigned or self._totals is None:
            self.summary = wer_summary(self.scores)
        else:
            t = self._totals.cpu().tolist()      # the stage's one read
            self.summary = _rates({"num_edits": t[0], "insertions": t[1], "deletions": t[2], "substitutions": t[3], "num_scored_tokens": t[4],
                                   "num_scored_sents": t[5], "num_erraneous_sents": t[6], "num_absent_sents": 0, "num_ref_sents": t[5]})
        self.summary["error_rate"] = self.summary["WER"]
        return self.summary if field is None else self.summary[field]

    def write_stats(self, filestream):
        if not self.summary:
            self.summarize()
        write_wer_text(self.summary, self.scores, filestream)


def merge_across_ranks(stats, group=None):
    """The reference recipe's gathering (train_librispeechmix_scratch.py:217-236): every rank's ``scores`` in rank order, then one entry
    per key - a later entry replaces an earlier one in the place of the first. Nothing happens on one rank."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return stats
    gathered = [None] * dist.get_world_size(group)
    dist.all_gather_object(gathered, stats.scores, group=group)
    stats.scores = list({d["key"]: d for part in gathered for d in part}.values())
    return stats
