"""Host side of the WER / CER statistics (ts-asr_amd/metrics.py) against the reference's own results recorded in
tests/golden/wer_cases.npz (tools/gen_golden_wer.py), and the pin of tests/helpers/edit_ref.py - the restatement the GPU tests use for
sizes the golden file does not hold - to that file. All comparisons are between integers or strings: equality. No kernel runs here."""
import importlib
import io
import os
import sys

import pytest
import torch

from tests.helpers import edit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _metrics():
    return importlib.import_module("ts-asr_amd.metrics")


def _load(path, ov=None):
    hp = importlib.import_module("ts-asr_amd.hparams")
    with open(path) as f:
        return hp.load_hyperpyyaml(f, ov)


@pytest.mark.parametrize("name", ["conformer-t_scratch", "conformer-t_wavlm", "conformer-t_none"])
def test_recipe_yaml_builds_error_rate_stats(name):
    h = _load(os.path.join(ROOT, "hparams", f"{name}_mi355x.yaml"), dict(d_model=144, nhead=4, encoder_num_layers=2, speaker_num_layers=2,
                                                                          d_ffn=576, joint_dim=160, decoder_neurons=128))
    M = _metrics()
    cer, wer = h["cer_computer"](), h["wer_computer"]()
    assert type(cer) is M.ErrorRateStats and type(wer) is M.ErrorRateStats
    assert cer.split_tokens is True and wer.split_tokens is False and cer.space_token == "_"
    assert h["cer_computer"]() is not cer                  # !name: a factory, one object per stage


def test_reference_yaml_metric_keys_resolve():
    """The two keys as the reference's YAML writes them (conformer-t_scratch.yaml:297-300), beside a class path that has no mirror: the
    statistics class is re-pointed to metrics.ErrorRateStats, the logger stays a placeholder."""
    restated = ("cer_computer: !name:speechbrain.utils.metric_stats.ErrorRateStats\n    split_tokens: True\n\n"
                "wer_computer: !name:speechbrain.utils.metric_stats.ErrorRateStats\n")
    hp = importlib.import_module("ts-asr_amd.hparams")
    h = hp.load_hyperpyyaml(restated + "train_logger: !new:speechbrain.utils.train_logger.FileTrainLogger\n    save_file: x\n")
    M = _metrics()
    assert isinstance(h["cer_computer"](), M.ErrorRateStats) and h["cer_computer"]().split_tokens is True
    assert isinstance(h["wer_computer"](), M.ErrorRateStats)
    assert type(h["train_logger"]).__name__ == "Unavailable"
    with pytest.raises(NotImplementedError):
        M.ErrorRateStats(extract_concepts_values=True)


def test_edit_ref_reproduces_every_golden_pair(golden):
    g = golden["wer_cases"]
    assert int(g["n_path_choice_matters"]) >= 50           # the generator's condition: the tie rule decides the split in these
    ids = [str(i) for i in g["ids"]]
    assert {"both-empty-word", "empty-hyp", "single-token", "identical", "empty-ref"} <= set(ids)
    for prefix in ("", "wer_", "cer_"):
        refs, hyps, counts, alis = edit_ref.golden_pairs(g, prefix)
        assert len(refs) >= 290
        for k, (a, b) in enumerate(zip(refs, hyps)):
            cnt, ali = edit_ref.edit_ops(a, b)
            assert cnt == counts[k], (prefix, k, cnt, counts[k])
            assert ali == alis[k], (prefix, k)
    cnt, ali = edit_ref.edit_ops(g["long_ref"], g["long_hyp"])
    assert cnt == g["long_counts"].tolist()
    assert bytes(ord(o) for o, _, _ in ali) == g["long_align_op"].tobytes()
    assert [-1 if i is None else i for _, i, _ in ali] == g["long_align_i"].tolist()
    assert [-1 if j is None else j for _, _, j in ali] == g["long_align_j"].tolist()


def test_edit_ref_tie_rule_is_the_references():
    """Hand cases where the three rules part: equal costs go to the insertion, then the deletion; the substitution only when strictly cheaper."""
    # cell (2, 2) of [1, 2] against [2, 1]: all three candidates cost 2 -> insertion; then (2, 1) is a match and column 0 a deletion
    assert edit_ref.edit_ops([1, 2], [2, 1]) == ([2, 1, 1, 0], [("D", 0, None), ("=", 1, 0), ("I", None, 1)])
    assert edit_ref.edit_ops([1], [2]) == ([1, 0, 0, 1], [("S", 0, 0)])
    assert edit_ref.edit_ops([], [4, 4]) == ([2, 2, 0, 0], [("I", None, 0), ("I", None, 1)])
    assert edit_ref.edit_ops([4, 4], []) == ([2, 0, 2, 0], [("D", 0, None), ("D", 1, None)])
    assert edit_ref.edit_ops([], []) == ([0, 0, 0, 0], [])


@pytest.mark.parametrize("name", ["wer", "cer"])
def test_assigned_scores_give_the_golden_summary_and_text(golden, name):
    g = golden["wer_cases"]
    M = _metrics()
    stats = M.ErrorRateStats(split_tokens=name == "cer")
    stats.scores = edit_ref.golden_details(g, name)        # as the recipe assigns after gathering the ranks' lists
    summary = stats.summarize()
    want = edit_ref.golden_summary(g, name)
    assert set(summary) == set(want) and "error_rate" in summary
    for k, v in want.items():
        assert summary[k] == v and type(summary[k]) is (float if k in ("WER", "SER", "error_rate") else int), k
    assert stats.summarize("error_rate") == want["WER"]
    out = io.StringIO()
    stats.write_stats(out)
    assert out.getvalue().encode("utf-8") == g[name + "_text"].tobytes()
    stats.clear()
    assert stats.scores == [] and stats.ids == [] and stats.summary == {}


def test_token_plumbing_and_char_tokenizer():
    M = _metrics()
    assert M.undo_padding(torch.tensor([[1, 2, 3, 0], [4, 5, 6, 7]]), torch.tensor([0.75, 1.0])) == [[1, 2, 3], [4, 5, 6, 7]]
    assert M.merge_char([["a", "b", "_", "c", "_", "d", "e"], ["e", "f", "g", "_", "h", "i"]]) == [["ab", "c", "de"], ["efg", "hi"]]
    assert M.split_word([["ab", "c", "de"], ["efg", "hi"], [], [""]]) == [list("ab_c_de"), list("efg_hi"), [], []]
    tok = M.CharTokenizer(["<blank>", "▁", "a", "b", "c"])
    assert tok([[1, 2, 3, 1, 4], [2, 3], [], [1, 2, 1, 1, 3]], task="decode_from_list") == [["ab", "c"], ["ab"], [""], ["a", "", "b"]]
    buf, lay = M.pack_pairs([[5, 6], [], [7]], [[5], [8, 9], []], [2, 0, 1])
    assert buf.tolist() == [0, 2, 2, 3, 0, 1, 3, 3, 2, 0, 1, 5, 6, 7, 5, 8, 9]
    assert (lay["max_ref"], lay["max_hyp"], lay["cells"], lay["nr"], lay["nh"]) == (2, 2, 3 * 2 + 1 * 3 + 2 * 1, 3, 3)


def _merge_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    M = importlib.import_module("ts-asr_amd.metrics")
    stats = M.ErrorRateStats()
    # rank 0 holds a, b, c; rank 1 holds d, b (a duplicate the sampler padded in, with another value), e
    mine = [("a", 0), ("b", 0), ("c", 0)] if rank == 0 else [("d", 1), ("b", 1), ("e", 1)]
    stats.scores = [{"key": k, "scored": True, "hyp_absent": False, "hyp_empty": False, "num_edits": r, "num_ref_tokens": 2, "WER": 50.0 * r,
                     "insertions": r, "deletions": 0, "substitutions": 0, "alignment": [], "ref_tokens": ["x", "y"], "hyp_tokens": ["x", "y"]}
                    for k, r in mine]
    M.merge_across_ranks(stats)
    torch.save({"keys": [(d["key"], d["num_edits"]) for d in stats.scores], "summary": stats.summarize()}, os.path.join(out_dir, f"s{rank}.pt"))
    dist.destroy_process_group()


def test_merge_across_ranks_gloo_world2(tmp_path):
    """The reference recipe's gathering: rank order, then one entry per key - the later entry's value in the first one's place."""
    import torch.multiprocessing as mp
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    s0, s1 = torch.load(tmp_path / "s0.pt"), torch.load(tmp_path / "s1.pt")
    assert s0["keys"] == s1["keys"] == [("a", 0), ("b", 1), ("c", 0), ("d", 1), ("e", 1)]
    assert s0["summary"]["num_edits"] == 3 and s0["summary"]["num_scored_sents"] == 5 and s0["summary"]["WER"] == 30.0
    M = _metrics()
    alone = M.ErrorRateStats()
    assert M.merge_across_ranks(alone) is alone            # one process, no group: nothing happens


def test_append_needs_the_device(pkg):
    M = _metrics()
    capi = importlib.import_module("ts-asr_amd._capi")
    if not torch.cuda.is_available():                      # (with a device the same calls score: tests/test_wer_gpu.py)
        stats = M.ErrorRateStats()
        with pytest.raises(capi.TsasrHipMissing):
            stats.append(["u1"], [["a", "b"]], [["a", "c"]])
        with pytest.raises(capi.TsasrHipMissing):
            stats.append_ids(["u1"], [[1, 2]], [[1, 3]])
        with pytest.raises(capi.TsasrHipMissing):
            M.score_pairs([[1, 2]], [[1, 3]])
    with pytest.raises(capi.TsasrHipMissing):
        importlib.import_module("ts-asr_amd.ops").edit_distance(*[torch.zeros(2, dtype=torch.int32)] * 5, 1, 1, 4)
    assert {"tsasr_edit_distance", "tsasr_edit_distance_workspace_bytes"} <= set(capi.exported_symbols())
