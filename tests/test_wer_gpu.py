"""WER / CER scoring on the device (csrc/editdist.hip through ops.edit_distance / metrics.ErrorRateStats / the recipe) against the
reference's recorded results (tests/golden/wer_cases.npz) and, for sizes that file does not hold, against tests/helpers/edit_ref.py
(pinned to the same file by tests/test_wer_cpu.py). Everything compared is an integer or a string: equality, no tolerance."""
import importlib
import io
import os

import numpy as np
import pytest
import torch

from tests.helpers import edit_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
M = importlib.import_module("ts-asr_amd.metrics")
ops = importlib.import_module("ts-asr_amd.ops")


def _raw(res):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in (res.counts, res.align_len)]


def _same(got, counts, alis, tag):
    assert len(got) == len(counts)
    for k, (cnt, ali) in enumerate(got):
        assert cnt == counts[k], (tag, k, cnt, counts[k])
        assert len(ali) == len(alis[k]) and ali == alis[k], (tag, k)


@pytest.mark.parametrize("prefix", ["", "wer_", "cer_"])
def test_golden_pairs_in_one_batch_and_alone(golden, prefix):
    """Every pair of the golden file: counts, alignment length and alignment as the reference's op_table -> count_ops / alignment gave
    them, in one mixed-length batch and scored pair by pair."""
    refs, hyps, counts, alis = edit_ref.golden_pairs(golden["wer_cases"], prefix)
    got, res, lay = M.score_pairs(refs, hyps, device=DEV)
    _same(got, counts, alis, prefix + "batch")
    assert res.align_len.cpu().tolist() == [len(a) for a in alis]
    for k in range(len(refs)):
        one, _, _ = M.score_pairs([refs[k]], [hyps[k]], device=DEV)
        _same(one, [counts[k]], [alis[k]], f"{prefix}alone{k}")


LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1024]


def _random_pairs(alphabet, seed):
    rng = np.random.RandomState(seed)
    pairs = [(rng.randint(0, alphabet, n).tolist(), rng.randint(0, alphabet, m).tolist()) for n in LENGTHS for m in LENGTHS]
    # correlated pairs (a noisy copy: the path hugs the diagonal, as a hypothesis does) at the sizes where the kernel changes its layout
    for n in (64, 256, 257, 1024):
        ref = rng.randint(0, alphabet, n).tolist()
        hyp = [t if u >= 0.3 else int(rng.randint(alphabet)) for t, u in zip(ref, rng.rand(n)) if u >= 0.1]
        pairs.append((ref, hyp))
    # beyond 1024 columns the strips widen to 8 (the long pair below), 16 and 64 columns per thread
    pairs += [(rng.randint(0, alphabet, 70).tolist(), rng.randint(0, alphabet, 2100).tolist()),
              (rng.randint(0, alphabet, 40).tolist(), rng.randint(0, alphabet, 4200).tolist())]
    return pairs


@pytest.mark.parametrize("alphabet", [2, 28])
def test_sizes_against_edit_ref(golden, alphabet):
    """Lengths {0, 1, 63, 64, 65, 255, 256, 257, 1024} on either side in every combination (n = 0 and m = 0 among them), alphabet 2 (ties
    in almost every cell) and 28, plus the golden 1920-token pair: one mixed batch (256 threads per pair, tables in LDS and in the
    workspace), the pairs of at most 256 columns again as a batch of their own (one wave per pair), and a few pairs alone."""
    g = golden["wer_cases"]
    pairs = _random_pairs(alphabet, 100 + alphabet) + [(g["long_ref"].tolist(), g["long_hyp"].tolist())]
    want = [edit_ref.edit_ops(a, b) for a, b in pairs]
    assert want[-1][0] == g["long_counts"].tolist()
    counts, alis = [w[0] for w in want], [w[1] for w in want]
    got, _, lay = M.score_pairs([a for a, _ in pairs], [b for _, b in pairs], device=DEV)
    assert lay["max_hyp"] == 4200
    _same(got, counts, alis, "mixed")
    short = [k for k, (_, b) in enumerate(pairs) if len(b) <= 256]
    got, _, lay = M.score_pairs([pairs[k][0] for k in short], [pairs[k][1] for k in short], device=DEV)
    assert lay["max_hyp"] == 256 and len(short) >= 54
    _same(got, [counts[k] for k in short], [alis[k] for k in short], "one wave per pair")
    for k in (0, 1, 9, 40, 80, len(pairs) - 3, len(pairs) - 2, len(pairs) - 1):
        one, _, _ = M.score_pairs([pairs[k][0]], [pairs[k][1]], device=DEV)
        _same(one, [counts[k]], [alis[k]], f"alone{k}")


def test_totals_summary_repeatability_and_poisoned_workspace(golden):
    g = golden["wer_cases"]
    ids, hyp_words, ref_words = edit_ref.golden_words(g, "wer")
    stats = M.ErrorRateStats()
    cuts = [0, 7, 107, len(ids)]                             # three appends of different batch sizes
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        stats.append(ids[lo:hi], hyp_words[lo:hi], ref_words[lo:hi])
    totals = stats._totals.cpu().tolist()
    details = edit_ref.golden_details(g, "wer")
    assert totals[:4] == [sum(d[k] for d in details) for k in ("num_edits", "insertions", "deletions", "substitutions")]
    assert totals[4:8] == [sum(d["num_ref_tokens"] for d in details), len(details), sum(d["num_edits"] > 0 for d in details), 0]
    summary = stats.summarize()
    want = edit_ref.golden_summary(g, "wer")
    assert {k: float(v) for k, v in summary.items()} == want and summary["error_rate"] == summary["WER"]
    assert stats._pending and not stats._scores            # summarize read the totals: no per-utterance copy was made for it

    # two runs give identical buffers, whatever the workspace held: a batch with tables in LDS and tables in the workspace
    rng = np.random.RandomState(5)
    refs = [rng.randint(0, 3, n).tolist() for n in (30, 700, 0, 1024, 257, 12)]
    hyps = [rng.randint(0, 3, m).tolist() for m in (33, 650, 5, 1000, 1024, 0)]
    buf, lay = M.pack_pairs(refs, hyps)
    dev = torch.from_numpy(buf).to(DEV)
    need = ops.edit_distance_workspace_bytes(lay["N"], lay["cells"])
    runs = []
    for fill in (0, 255, 0x5A):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
        res = M.launch_packed(dev, lay, workspace=ws)
        torch.cuda.synchronize()
        lens = res.align_len.cpu().numpy()
        base = np.concatenate([[0], np.cumsum(lay["n"] + lay["m"])])
        used = np.concatenate([np.arange(base[k], base[k] + lens[k]) for k in range(lay["N"])]).astype(np.int64)
        runs.append([res.counts.cpu().numpy().tobytes(), lens.tobytes(), res.totals.cpu().numpy().tobytes()] +
                    [t.cpu().numpy()[used].tobytes() for t in (res.align_op, res.align_i, res.align_j)])
    assert runs[0] == runs[1] == runs[2]
    with pytest.raises(ValueError):
        M.launch_packed(dev, lay, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("name", ["wer", "cer"])
def test_error_rate_stats_end_to_end(golden, name):
    """ErrorRateStats on the device, word level and split_tokens=True, fed as the generator fed the reference's object: the per-utterance
    dicts, the summary and the write_stats text equal the recorded ones."""
    g = golden["wer_cases"]
    ids, hyp_words, ref_words = edit_ref.golden_words(g, name)
    stats = M.ErrorRateStats(split_tokens=name == "cer")
    for lo in range(0, len(ids), 32):
        stats.append(ids[lo:lo + 32], hyp_words[lo:lo + 32], ref_words[lo:lo + 32])
    out = io.StringIO()
    stats.write_stats(out)
    assert out.getvalue().encode("utf-8") == g[name + "_text"].tobytes()
    assert {k: float(v) for k, v in stats.summary.items()} == edit_ref.golden_summary(g, name)
    assert stats.scores == edit_ref.golden_details(g, name) and stats.ids == ids


PIECES = ["<blank>", "▁"] + list("abcdefghijklmnopqrstuvwxyz'")


def _intern(seqs_a, seqs_b):
    table = {}
    conv = lambda seqs: [[table.setdefault(t, len(table)) for t in s] for s in seqs]  # noqa: E731
    return conv(seqs_a), conv(seqs_b)


def test_recipe_scores_valid_and_test_stages(tmp_path):
    """train_tsasr.main on the scratch recipe (fp32, two synthetic batches): the TEST stage's token error rate, and with a tokenizer its
    WER and CER, equal edit_ref's over brain.last_hyps; --wer_file holds the write_stats text; the hypotheses are those of a run without
    the metric keys."""
    nnet = importlib.import_module("ts-asr_amd.nnet")
    mod = importlib.import_module("train_tsasr")
    wer_file = tmp_path / "wer_test.txt"
    argv = [os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml"), "--device", "cuda:0", "--synthetic", "2", "--number_of_epochs",
            "1", "--syn_batch", "4", "--syn_seconds", "2.0", "--syn_enroll_seconds", "1.0", "--syn_tokens", "12", "--hip_graph", "False",
            "--lr", "0.002", "--warmup_steps", "5", "--dropout", "0.0", "--beam_size", "3", "--d_model", "144", "--nhead", "4",
            "--encoder_num_layers", "2", "--speaker_num_layers", "2", "--d_ffn", "576", "--joint_dim", "160", "--decoder_neurons", "128",
            "--compute_dtype", "fp32"]
    opts = {"syn_batch": 4, "syn_seconds": 2.0, "syn_enroll_seconds": 1.0, "syn_tokens": 12}
    try:
        brain, result = mod.main(argv + ["--wer_file", str(wer_file)])
        test = mod.synthetic_loader(1, vars(brain.hparams), opts, 99, brain.device)      # what main() evaluated
        assert len(test) == 1
        targets = M.undo_padding(test[0].tokens.data.cpu(), test[0].tokens.lengths.cpu())
        hyps = brain.last_hyps
        assert len(hyps) == 4 and set(brain.test_stats) == {"loss", "TER"} and result["test_stats"] is brain.test_stats
        assert brain.test_stats["TER"] == edit_ref.error_rate(targets, hyps)
        assert set(brain.valid_stats) == {"loss", "TER"} and brain.valid_stats["loss"] == pytest.approx(brain.test_stats["loss"], rel=1e-5)
        assert [d["key"] for d in brain.wer_metric.scores] == test[0].id
        assert [d["num_edits"] for d in brain.wer_metric.scores] == [edit_ref.edit_ops(t, h)[0][0] for t, h in zip(targets, hyps)]
        text = io.StringIO()
        brain.wer_metric.write_stats(text)
        assert wer_file.read_text() == text.getvalue() and text.getvalue().startswith("%WER ")

        # with a tokenizer: words against batch.target_words, as the reference's recipe
        tok = M.CharTokenizer(PIECES)
        brain.tokenizer = tok
        test[0].target_words = tok(targets, task="decode_from_list")
        brain.evaluate(test)
        assert brain.last_hyps == hyps and set(brain.test_stats) == {"loss", "CER", "WER"}
        hyp_words = tok(hyps, task="decode_from_list")
        assert brain.test_stats["WER"] == edit_ref.error_rate(*_intern(test[0].target_words, hyp_words))
        assert brain.test_stats["CER"] == edit_ref.error_rate(*_intern(M.split_word(test[0].target_words), M.split_word(hyp_words)))
        assert brain.cer_metric.split_tokens is True and len(brain.cer_metric.scores) == 4

        plain, result2 = mod.main(argv + ["--wer_computer", "null", "--cer_computer", "null"])
        assert plain.last_hyps == hyps and set(plain.test_stats) == {"loss"} and plain.wer_metric is None
        assert result2["test_loss"] == result["test_loss"]
    finally:
        nnet.set_compute_dtype(torch.bfloat16)
