#!/usr/bin/env python3
"""Recipe entry point on the MI355X runtime - the counterpart of the reference's train_librispeechmix_{scratch,pretrained,none}.py
`__main__` (train_librispeechmix_scratch.py:491-611): parse_arguments -> load_hyperpyyaml -> ddp_init_group -> TSASR -> fit -> evaluate.

    python train_tsasr.py hparams/conformer-t_scratch_mi355x.yaml [--key value ...]            (one GPU)
    python -m torch.distributed.run --nproc-per-node N train_tsasr.py <yaml> --distributed_launch   (one process per GPU, RCCL)

Run options and YAML overrides are those of speechbrain.core.parse_arguments (SB/core.py:134-393); extra keys understood here:
  --train_json / --valid_json / --test_json : LibriSpeechMix manifests written by the reference's librispeechmix_prepare.py
        (+ --data_folder). Audio decoding and the SentencePiece tokenizer are the caller's (dataio.py docstring): a manifest entry
        must carry `sig_path` tensors (torch .pt with mixed_sig / enroll_sig / tokens) - see ts-asr_amd/dataio.py.
  --synthetic N    : N synthetic LibriSpeechMix-shaped batches per epoch instead of manifests (no dataset on the GPU box); shapes from
        --syn_batch / --syn_seconds / --syn_enroll_seconds / --syn_tokens; lengths are length-bucketed like `sorting: ascending`.
  --hip_graph True : capture the step into hipGraphs (one per batch shape).
  --wer_file PATH  : the TEST stage writes the reference's WER report there (summary lines + one alignment per utterance).
  --align_file PATH : after the TEST stage the test batches are force-aligned to their reference transcripts (TSASR.align_batch: the best
        path through the RNN-T lattice) and a CTM is written there, "<utt> 1 <start> <dur> <word>" per word; without a tokenizer one
        line per token with the token id as the word. Works with --synthetic N.
  --hyp_ctm PATH : the TEST stage decodes with TransducerBeamSearcher.forward_timed (the same hypotheses, plus the encoder frame that
        emitted each token) and a CTM of the RECOGNISED words is written there after the stage, in the format and by the rules of
        --align_file. Like --align_file, rank 0 writes, and with several processes only what its own process decoded.
  --lm_ckpt FILE --lm_weight W : the TEST stage's beam search fuses a recurrent LM (decoders.py: LM fusion): FILE is a local state_dict
        of an RNNLM (the reference's keys; torch.save), its shape is read from the tensors; W > 0 is the LM's weight in the score. YAMLs
        that name lm_model / lm_weight themselves need neither option.
  --bias_file FILE --bias_weight W : contextual biasing of the TEST stage's beam search (ts-asr_amd/biasing.py: a prefix trie of phrases,
        W > 0 nats per matched token, given back if the phrase is left half-matched). Each line of FILE is one phrase: fields that are all
        integers are token ids; any other line is text, encoded with the tokenizer's pieces by greedy longest match (a space becomes the
        boundary piece); a line that cannot be encoded ends the run naming it. Needs a beam_searcher in the YAML; combines with --hyp_ctm
        and --lm_ckpt.
  --joint_logits lazy : subword vocabularies (32 < V <= 1024): loss and alignment run the fused joint + loss kernels, the [B,T',U+1,V]
        logits / dlogits tensors are never written (hparams key joint_logits: materialized | lazy; default materialized).
The pretrained-speaker variant is picked from the YAML (conformer-t_wavlm_mi355x.yaml); batches then carry `enroll_emb`."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "ts-asr_amd"
core = importlib.import_module(PKG + ".core")
dp = importlib.import_module(PKG + ".dp")
hp_mod = importlib.import_module(PKG + ".hparams")
batch_mod = importlib.import_module(PKG + ".batch")
tsasr = importlib.import_module(PKG + ".recipes.tsasr")

EXTRA = {"synthetic": 0, "syn_batch": 8, "syn_seconds": 4.0, "syn_enroll_seconds": 2.0, "syn_tokens": 24, "hip_graph": False,
         "number_of_epochs": 1, "train_json": None, "valid_json": None, "test_json": None, "data_folder": None, "wer_file": None,
         "align_file": None, "hyp_ctm": None, "lm_ckpt": None, "lm_weight": 0.0, "bias_file": None, "bias_weight": 0.0}


def load_lm(path, device):
    """An nnet.RNNLM (return_hidden=True, eval mode) built to fit the state_dict saved at ``path`` and loaded from it, strictly."""
    nnet = importlib.import_module(PKG + ".nnet")
    sd = torch.load(path, map_location="cpu")
    if not isinstance(sd, dict) or "embedding.Embedding.weight" not in sd or "rnn.rnn.weight_hh_l0" not in sd or "out.w.weight" not in sd:
        raise SystemExit(f"--lm_ckpt {path}: not the state_dict of an RNNLM with an LSTM")
    vocab, emb_dim = sd["embedding.Embedding.weight"].shape
    layers = sum(1 for k in sd if k.startswith("rnn.rnn.weight_hh_l"))
    blocks = sum(1 for k in sd if k.startswith("dnn.linear") and k.endswith(".w.weight"))
    lm = nnet.RNNLM(vocab, embedding_dim=emb_dim, rnn_layers=layers, rnn_neurons=sd["rnn.rnn.weight_hh_l0"].shape[1], return_hidden=True,
                    dnn_blocks=blocks, dnn_neurons=sd["out.w.weight"].shape[1])
    lm.load_state_dict(sd, strict=True)
    return lm.to(device).eval()


def load_bias(path, weight, pieces):
    """The biasing.ContextGraph of the phrase file ``path`` (module docstring); ``pieces``: the tokenizer's piece texts by id, or None."""
    biasing = importlib.import_module(PKG + ".biasing")
    with open(path, encoding="utf-8") as f:
        lines = f.read().splitlines()
    try:
        return biasing.ContextGraph.from_text(lines, pieces if pieces is not None else [], weight)
    except ValueError as e:
        raise SystemExit(f"--bias_file {path}: {e}")


def synthetic_loader(n_batches, hparams, opts, seed, device):
    """n_batches seeded LibriSpeechMix-shaped batches; three length buckets (x 1.0 / 0.75 / 0.5) visited in ascending order."""
    sr = hparams.get("sample_rate", 16000)
    feats = bool(hparams.get("input_is_feats", False))
    emb = int(hparams.get("speaker_embedding_dim", 0)) if "speaker_encoder_path" in hparams else 0
    out = []
    for i in range(n_batches):
        scale = (0.5, 0.75, 1.0)[min(2, i * 3 // max(n_batches, 1))]
        n_mix = int(opts["syn_seconds"] * scale * (100 if feats else sr))
        n_enr = int(opts["syn_enroll_seconds"] * (100 if feats else sr))
        if not feats:   # Fbank frames = 1 + L // 160: keep L = 160 * frames - 160 so that T' is a round number
            n_mix, n_enr = n_mix // 160 * 160 - 160, n_enr // 160 * 160 - 160
        b = batch_mod.synthetic_batch(opts["syn_batch"], n_mix, n_enr, max(1, int(opts["syn_tokens"] * scale)), vocab_size=hparams.get("vocab_size", 29),
                                      seed=seed + i, ragged=True, feats=feats, enroll_emb_dim=emb)
        out.append(b.to(device))
    return out


def write_alignments(brain, batches, hparams, path):
    """Force-aligns every batch to its reference transcript and writes one CTM; returns the number of lines. One device-to-host copy per batch."""
    align = importlib.import_module(PKG + ".align")
    fs = align.frame_seconds(hparams)
    pieces = getattr(getattr(brain, "tokenizer", None), "pieces", None)      # the tokenizer's piece texts by id (metrics.CharTokenizer has them)
    ids, spans = [], []
    for n, batch in enumerate(batches):
        frames, _ = align.fetch(*brain.align_batch(batch))
        refs = batch.tokens.data.tolist()      # whole rows: frames are -1 beyond an utterance's tokens, the spans stop there
        for utt, fr, ref in zip(_ctm_names(getattr(batch, "id", None), ids, n, len(refs)), frames, refs):
            ids.append(utt)
            spans.append(align.word_spans(fr, ref, pieces, fs) if pieces is not None else align.token_spans(fr, ref, fs))
    return align.write_ctm(path, ids, spans)


def _ctm_names(utts, ids, n, count):
    """Utterance names of batch ``n`` for a CTM: the batch's ids (numbered when it has none), kept apart from those already in ``ids``
    (synthetic batches reuse theirs)."""
    utts = utts or [f"utt{len(ids) + k}" for k in range(count)]
    return [f"{u}-{n}" for u in utts] if len(set(utts) & set(ids)) else list(utts)


def write_hyp_ctm(brain, hparams, path):
    """One CTM of the hypotheses the TEST stage recognised (brain.hyp_times, kept by compute_forward under hparams.hyp_ctm): word spans
    from the emission frame of each token; returns the number of lines."""
    align = importlib.import_module(PKG + ".align")
    fs = align.frame_seconds(hparams)
    pieces = getattr(getattr(brain, "tokenizer", None), "pieces", None)
    ids, spans = [], []
    for n, (utts, hyps, frames) in enumerate(getattr(brain, "hyp_times", [])):
        for utt, hyp, fr in zip(_ctm_names(utts, ids, n, len(hyps)), hyps, frames):
            ids.append(utt)
            spans.append(align.word_spans(fr, hyp, pieces, fs) if pieces is not None else align.token_spans(fr, hyp, fs))
    return align.write_ctm(path, ids, spans)


def main(argv=None):
    hparams_file, run_opts, overrides = core.parse_arguments(argv)
    opts = {k: overrides.pop(k, v) for k, v in EXTRA.items()}
    with open(hparams_file) as f:
        hparams = hp_mod.load_hyperpyyaml(f, overrides)
    if opts["wer_file"]:
        hparams["wer_file"] = str(opts["wer_file"])
    if opts["hyp_ctm"]:
        hparams["hyp_ctm"] = str(opts["hyp_ctm"])
    dp.ddp_init_group(run_opts)                                           # one process per GPU (SB/utils/distributed.py:123-201)
    brain = tsasr.TSASR(hparams["modules"], hparams["opt_class"], hparams, run_opts)
    if opts["hip_graph"]:
        brain.enable_hip_graph()
    if opts["lm_ckpt"]:
        searcher = hparams.get("beam_searcher")
        if searcher is None or float(opts["lm_weight"]) <= 0:
            raise SystemExit("--lm_ckpt needs a beam_searcher in the YAML and --lm_weight W with W > 0")
        searcher.lm, searcher.lm_weight = load_lm(str(opts["lm_ckpt"]), brain.device), float(opts["lm_weight"])
    if opts["bias_file"]:
        searcher = hparams.get("beam_searcher")
        if searcher is None or float(opts["bias_weight"]) <= 0:
            raise SystemExit("--bias_file needs a beam_searcher in the YAML and --bias_weight W with W > 0")
        try:
            searcher.bias = load_bias(str(opts["bias_file"]), float(opts["bias_weight"]), getattr(getattr(brain, "tokenizer", None), "pieces", None))
        except ValueError as e:                                           # a blank or a token outside the vocabulary
            raise SystemExit(f"--bias_file {opts['bias_file']}: {e}")
    rank = int(os.environ.get("RANK", 0))
    if opts["synthetic"]:
        train = synthetic_loader(int(opts["synthetic"]), hparams, opts, 1234 + 1000 * rank, brain.device)
        valid = synthetic_loader(max(1, int(opts["synthetic"]) // 4), hparams, opts, 99, brain.device)
        test = valid
    else:
        dataio = importlib.import_module(PKG + ".dataio")
        if not opts["train_json"]:
            raise SystemExit("give --train_json (a LibriSpeechMix manifest) or --synthetic N")
        load = lambda p: dataio.manifest_batches(p, hparams, opts["data_folder"], brain.device) if p else None  # noqa: E731
        train, valid, test = load(opts["train_json"]), load(opts["valid_json"]), load(opts["test_json"])
    hparams["epoch_counter"].limit = int(opts["number_of_epochs"])
    brain.fit(hparams["epoch_counter"], train, valid)
    result = {"train_loss": brain.avg_train_loss, "optimizer_steps": brain.optimizer_step, "nonfinite": brain.nonfinite_count}
    if test is not None:
        result["test_loss"] = brain.evaluate(test)
        result["test_hyps"] = getattr(brain, "last_hyps", None)
        result["test_stats"] = getattr(brain, "test_stats", None)
        if opts["align_file"] and rank == 0:
            result["align_lines"] = write_alignments(brain, test, hparams, str(opts["align_file"]))
        if opts["hyp_ctm"] and rank == 0:
            result["hyp_ctm_lines"] = write_hyp_ctm(brain, hparams, str(opts["hyp_ctm"]))
    if valid is not None:
        result["valid_stats"] = getattr(brain, "valid_stats", None)
    if rank == 0:
        print({k: (v if k != "test_hyps" else (v[:2] if v else v)) for k, v in result.items()})
    if dp.is_initialized():
        torch.distributed.destroy_process_group()
    return brain, result


if __name__ == "__main__":
    main()
