"""Host side of forced alignment: token frames (rnnt.rnnt_align / TSASR.align_batch) -> word time spans -> a CTM file.

The device work is one call per batch (csrc/rnnt.hip rnnt_viterbi_kernel); ``fetch`` brings its result to the host as ONE copy.
``frame_seconds`` is the duration of an encoder frame: 4 (the front-end's subsampling) x hop_length ms, 0.040 s with the shipped YAMLs.
"""
SUBSAMPLING = 4      # the two stride-2 convolutions of the front-end


def frame_seconds(hparams):
    """Seconds per encoder frame from the hparams (``hop_length`` in ms, 10 when the YAML does not say)."""
    get = hparams.get if hasattr(hparams, "get") else (lambda k, d=None: getattr(hparams, k, d))
    return SUBSAMPLING * float(get("hop_length", 10)) / 1000.0


def fetch(frames, scores):
    """(frames int32 [B, U], scores fp32 [B]) on the device -> (list of B lists of ints, list of B floats) with one device-to-host copy
    (the score travels as its bit pattern in an extra int32 column)."""
    import torch
    packed = torch.cat([frames.to(torch.int32), scores.to(torch.float32).view(torch.int32)[:, None]], dim=1).cpu()
    return packed[:, :-1].tolist(), packed[:, -1].contiguous().view(torch.float32).tolist()


def word_spans(frames, tokens, pieces, frame_seconds):
    """[(word, start_s, end_s), ...] of one utterance. ``frames[i]`` is the emission frame of ``tokens[i]`` (entries beyond the shorter of
    the two, and frames < 0, are padding); ``pieces[id]`` is the token's text. A piece beginning with "▁" starts a new word (a stand-alone
    "▁" as CharTokenizer has it, or a SentencePiece-style "▁the"); a word's text is its pieces joined with "▁" removed, empty words are
    dropped. start = frame(first token) * frame_seconds, end = (frame(last token) + 1) * frame_seconds."""
    spans, cur = [], None      # cur = [text, first frame, last frame]

    def close():
        if cur is not None and cur[0]:
            spans.append((cur[0], cur[1] * frame_seconds, (cur[2] + 1) * frame_seconds))

    for f, tok in zip(frames, tokens):
        f = int(f)
        if f < 0:
            break
        piece = pieces[int(tok)]
        if piece.startswith("▁") or cur is None:
            close()
            cur = ["", f, f]
        cur[0] += piece.replace("▁", "")
        cur[2] = f
    close()
    return spans


def token_spans(frames, tokens, frame_seconds):
    """Token-level spans for a run without a tokenizer: the token id is the word, each token lasts one frame."""
    return [(str(int(t)), int(f) * frame_seconds, (int(f) + 1) * frame_seconds) for f, t in zip(frames, tokens) if int(f) >= 0]


def write_ctm(path, ids, spans):
    """One line per word, "<utt> 1 <start> <dur> <word>" with three decimals; ``spans[i]`` are utterance ``ids[i]``'s (word, start, end)."""
    n = 0
    with open(path, "w", encoding="utf-8") as out:
        for utt, sp in zip(ids, spans):
            for word, start, end in sp:
                out.write(f"{utt} 1 {start:.3f} {end - start:.3f} {word}\n")
                n += 1
    return n
