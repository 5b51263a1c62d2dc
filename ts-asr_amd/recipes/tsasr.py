"""TS-ASR Brain: the reference recipes' ``TSASR(sb.Brain)`` on the MI355X runtime.

Mirrors train_librispeechmix_scratch.py:33-195 (and the ``pretrained`` / ``none`` variants, which differ only in
the speaker branch: train_librispeechmix_pretrained.py:45-63, train_librispeechmix_none.py): same module names in
``self.modules``, same call order, same return values (``compute_forward -> (logits [B,T',U+1,V], hyps or None)``,
``compute_objectives -> 0-dim loss with autograd``); with ``ctc_weight > 0`` the SpeechBrain transducer recipe's auxiliary CTC branch
(``proj_ctc`` on the projected encoder output, a third element ``ctc_scores`` in the forward's tuple). Differences: joiner + head run as ONE fused HIP kernel
(the [B,T',U+1,J] joint tensor is never built), lengths stay on the device, WER / CER are scored on the device
(metrics.py); plotting, logging and checkpoint selection are left to the caller (out of scope).
"""
import contextlib
import functools
import os

import torch

from .. import core, ctc, prof, rnnt
from ..hparams import Unavailable
from ..metrics import merge_across_ranks, undo_padding
from ..nnet import abs_lengths_round

Stage = core.Stage


# TSASR_OVERLAP: "1" (default) the speaker branch and, behind it, the predictor run on a second HIP stream; "2" only the speaker branch;
# "0" one stream. (Round 2's other placements - predictor on a third stream, issued after the encoder, its backward run re-entrantly,
# a high-priority side stream - were measured equal or slower and are gone: profiles/r02_notes.md section 5.)
_OVERLAP_MODE = os.environ.get("TSASR_OVERLAP", "1")
_OVERLAP_DEFAULT = _OVERLAP_MODE != "0"
# TSASR_CTC_STREAM: "main" (default) the auxiliary CTC branch (proj_ctc, loss) runs on the main stream between encoder_proj and the joint;
# "side" on a stream of its own, beside the joint and the transducer loss (profiles/ctc_notes.md section 4 has both timed)
_CTC_STREAM = os.environ.get("TSASR_CTC_STREAM", "main")
_PRED_STREAM_MIN_U = int(os.environ.get("TSASR_PRED_STREAM_MIN_U", "512"))      # tokens from which the predictor gets a stream of its own


class TSASR(core.Brain):
    """One class for the reference's three recipe scripts; ``variant`` says which speaker branch runs:
    "scratch" (train_librispeechmix_scratch.py), "pretrained" (train_librispeechmix_pretrained.py, frozen speaker encoder) or "none"
    (train_librispeechmix_none.py). Taken from hparams["variant"] / run_opts when given, else from what the YAML declares: the
    pretrained YAML has `speaker_encoder_path` and no speaker front-end (conformer-t_wavlm.yaml:121-123), the `none` YAML no speaker_proj."""

    def __init__(self, modules=None, opt_class=None, hparams=None, run_opts=None, checkpointer=None, profiler=None):
        super().__init__(modules, opt_class, hparams, run_opts, checkpointer, profiler)
        hp, ro = hparams or {}, run_opts or {}
        variant = ro.get("variant", hp.get("variant"))
        if variant is None:
            if "speaker_proj" not in self.modules:
                variant = "none"
            elif "speaker_encoder_path" in hp or "speaker_frontend" not in self.modules:
                variant = "pretrained"
            else:
                variant = "scratch"
        if variant not in ("scratch", "pretrained", "none"):
            raise ValueError(f"unknown TSASR variant {variant!r}")
        self.variant = variant
        # Auxiliary CTC head (SB recipes/LibriSpeech/ASR/transducer/hparams/conformer_transducer.yaml:198-200 `proj_ctc`): built here, before
        # the optimizer and the gradient arena exist, unless the YAML brought one; with ctc_weight == 0 there is none and nothing changes
        self.ctc_weight = float(hp.get("ctc_weight", 0.0) or 0.0)
        if not 0.0 <= self.ctc_weight <= 1.0:
            raise ValueError(f"ctc_weight must lie in [0, 1], got {self.ctc_weight}")
        if self.ctc_weight > 0 and "proj_ctc" not in self.modules:
            from ..nnet import Linear
            head = self.modules.transducer_head.w.weight
            self.modules["proj_ctc"] = Linear(input_size=head.shape[1], n_neurons=head.shape[0]).to(self.device)

    # ---- speaker branch (train_librispeechmix_scratch.py:44-80) ------------------------------------
    def _speaker_embedding(self, batch, epoch):
        hp = self.hparams
        if self.variant == "none":
            return None, None
        if self.variant == "pretrained":
            # train_librispeechmix_pretrained.py:45-63,80: the frozen speaker encoder's x-vector [B,1,E] (cross_attention: its last hidden
            # states [B,S,E]) goes through speaker_proj. The embedding arrives with the batch (`enroll_emb`, the synthetic / precomputed
            # form); a module registered as `speaker_encoder` (Hugging Face AutoModelForAudioXVector signature) is run as the reference does.
            if hasattr(batch, "enroll_emb"):
                embs, lens = batch.enroll_emb
            elif "speaker_encoder" in self.modules:
                enroll, lens = batch.enroll_sig
                with torch.no_grad():
                    self.modules.speaker_encoder.eval()
                    L = enroll.shape[-1]
                    n = (lens * L).ceil().clamp(max=L).int()
                    out = self.modules.speaker_encoder(input_values=enroll, attention_mask=(torch.arange(L, device=enroll.device)[None, :] < n[:, None]).long(),
                                                       output_attentions=False, output_hidden_states=hp.injection_mode == "cross_attention")
                embs = (out.hidden_states[-1][..., :hp.speaker_embedding_dim] if hp.injection_mode == "cross_attention"
                        else out.embeddings[:, None, :])
            else:
                raise ValueError("pretrained variant: the batch needs an `enroll_emb` field or modules['speaker_encoder'] must be set")
            return self.modules.speaker_proj(embs), lens
        enroll, enroll_lens = batch.enroll_sig
        if getattr(hp, "input_is_feats", False):
            feats = enroll
        else:
            feats = self.modules.speaker_feature_extractor(enroll)
            feats = self.modules.speaker_normalizer(feats, enroll_lens, epoch=epoch)
        feats = self.modules.speaker_frontend(feats)
        embs = self.modules.speaker_encoder(feats, enroll_lens)
        if hp.injection_mode != "cross_attention":     # masked mean-pool over the first ceil(len * T'e) frames (:52-64): one HIP launch
            from .. import ops
            embs = ops.mean_pool(embs, enroll_lens)
        return self.modules.speaker_proj(embs), enroll_lens

    def _predictor(self, tokens_bos, tokens_bos_lens):
        dec = self.modules.decoder
        if hasattr(dec, "forward_tokens"):       # embedding + decoder in one call: one-hot tokens never become a [B,U,V-1] tensor
            dec_out, _ = dec.forward_tokens(tokens_bos, self.modules.embedding, lengths=tokens_bos_lens)
        else:
            dec_out, _ = dec(self.modules.embedding(tokens_bos), lengths=tokens_bos_lens)
        return self.modules.decoder_proj(dec_out)

    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
            self._aux_streams.append(self._side)      # Brain joins it after backward
        return self._side

    def _ctc_stream(self):
        if getattr(self, "_ctc_side", None) is None:
            self._ctc_side = torch.cuda.Stream(device=self.device)
            self._aux_streams.append(self._ctc_side)
        return self._ctc_side

    def _pred_stream(self):
        if getattr(self, "_third", None) is None:
            self._third = torch.cuda.Stream(device=self.device)
            self._aux_streams.append(self._third)
        return self._third

    def _flush_main_wgrads(self, grad):
        """Tensor hook on the speaker embedding: fires (on the side stream) when the speaker branch's backward is about to start, i.e.
        when the mixture encoder's and front-end's backward have been enqueued on the main stream. Their queued weight gradients
        (three quarters of the step's) are launched there now, as one grouped kernel that runs beside the speaker branch's small,
        latency-bound backward kernels instead of after them; the rest follows in finish_backward. The gradient passes through."""
        prof.stamp("speaker backward starts [side]")
        arena = getattr(self, "arena", None)
        if arena is not None and arena.in_backward and getattr(arena, "_main_stream", None) is not None:
            with torch.cuda.stream(arena._main_stream):
                arena.flush_wgrads(hold=True)
                prof.stamp("early weight gradients done [main]")
        return None

    def _causal_features(self):
        """hparams ``causal_features: True``: the mixture's features are the causal ones (running floor, running normalisation) over the
        recipe's own Fbank tables; the enrolment keeps the sentence-level pair (it is whole before a stream starts)."""
        cf = getattr(self, "_causal_feats", None)
        if cf is None:
            from ..nnet import CausalFeatures
            cf = self._causal_feats = CausalFeatures(self.modules.feature_extractor)
        return cf

    def _ctc_train(self, epoch):
        """Does this TRAIN step carry the CTC term (train.py:111,153: ctc_weight > 0 and current_epoch <= number_of_ctc_epochs)?"""
        return self.ctc_weight > 0 and epoch <= int(getattr(self.hparams, "number_of_ctc_epochs", 0) or 0)

    def _host_draws(self):
        """Whether a step carries the CTC term is decided on the host, by the epoch: part of the captured graph's key, so the steps after
        the CTC epochs replay a graph of their own (nothing is added with ctc_weight == 0)."""
        draws = super()._host_draws()
        if self.ctc_weight > 0:
            hp = self.hparams
            draws += (("ctc", self._ctc_train(hp.epoch_counter.current if hasattr(hp, "epoch_counter") else 0)),)
        return draws

    def _forward_logits(self, batch, stage):
        """The forward up to the fused joint logits, shared by compute_forward and align_batch: (logits, enc_out, tlen, ulen, epoch).
        The CTC head's scores (or None) are left in ``self._ctc_scores``: TRAIN steps of the CTC epochs, and the VALID stage."""
        hp = self.hparams
        epoch = hp.epoch_counter.current if hasattr(hp, "epoch_counter") else 0
        batch = batch.to(self.device)
        mixed, mixed_lens = batch.mixed_sig
        tokens_bos, tokens_bos_lens = batch.tokens_bos
        tok = batch.tokens.data      # the loss's targets as the lattice kernels read them (int32): cast here, off the loss's own chain
        self._tokens32 = (tok, tok if tok.dtype == torch.int32 else tok.to(torch.int32).contiguous())
        # Two parts of the forward do not depend on the mixture encoder: the speaker branch (6 encoder layers over the enrollment,
        # half-filled grids; needed at the injection point) and the predictor (embedding -> LSTM -> projection; its persistent
        # recurrence kernels occupy 32 of 256 CUs for 0.4 + 0.7 ms; needed at the joint). Both run on a second HIP stream; the
        # encoder joins the first lazily at the injection, the joint waits for the second. Backward follows by itself (autograd
        # runs a node on the stream of its forward): the predictor's backward overlaps the last encoder layers', the speaker
        # branch's overlaps layer 0 / the front-end's. Works the same inside a captured hipGraph (fork / join become edges).
        overlap = (stage == Stage.TRAIN and self.variant != "none" and getattr(self, "overlap_branches", _OVERLAP_DEFAULT)
                   and torch.device(self.device).type == "cuda")
        dec_out = None
        if overlap:
            cur, side = torch.cuda.current_stream(), self._side_stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                spk, enroll_lens = self._speaker_embedding(batch, epoch)
                spk_ready = torch.cuda.Event()
                spk_ready.record(side)
                prof.stamp("speaker forward done [side]")
                if spk is not None and spk.requires_grad:
                    spk.register_hook(self._flush_main_wgrads)
                # The predictor follows the speaker branch on the forked stream, in eager and in captured steps alike (one autograd
                # topology: gradient buckets complete in the same order either way). Round 2 kept it on the main stream in eager steps
                # because runs with it forked deviated once in ~100; the cause was found in round 3 and is not a stream-ordering
                # matter: packed-fp32 instructions of one kernel returning wrong values while the per-step LSTM kernels ran beside it
                # (profiles/r03_notes.md section 1; the library no longer contains such instructions). "2" = speaker branch only.
                # Long targets (configs[4]: U = 1920, a 4.4 ms walk of 1920 dependent steps at B = 1): behind the speaker branch the
                # predictor ends 1.1 ms after the mixture encoder and the joint waits for it; on a stream of its own it starts with the
                # step. Short targets keep the one side stream: at configs[1] a third stream cost 0.1 ms (profiles/r04_notes.md section 4).
                own = _OVERLAP_MODE != "2" and tokens_bos.shape[1] >= _PRED_STREAM_MIN_U
                if _OVERLAP_MODE != "2" and not own:
                    dec_out = self._predictor(tokens_bos, tokens_bos_lens)
                    prof.stamp("predictor forward done [side]")
                    if prof.STAMPS and dec_out.requires_grad:
                        dec_out.register_hook(lambda g: prof.stamp("predictor backward starts [side]"))
            if own:
                third = self._pred_stream()
                third.wait_stream(cur)
                with torch.cuda.stream(third):
                    dec_out = self._predictor(tokens_bos, tokens_bos_lens)
                    prof.stamp("predictor forward done [third]")
                    if prof.STAMPS and dec_out.requires_grad:
                        dec_out.register_hook(lambda g: prof.stamp("predictor backward starts [third]"))

            def speaker_embs():
                prof.stamp("mixture reaches the injection [main]")
                cur.wait_event(spk_ready)
                spk.record_stream(cur)
                return spk
        else:
            speaker_embs, enroll_lens = self._speaker_embedding(batch, epoch)

        augment = bool(getattr(hp, "augment", False)) and stage == Stage.TRAIN
        if getattr(hp, "input_is_feats", False):
            feats = mixed
        else:
            if augment and "speed_perturb" in self.modules:      # train_librispeechmix_scratch.py:82-85
                mixed = self.modules.speed_perturb(mixed)
            if getattr(hp, "causal_features", False):            # BUILD EXTENSION: the features a live stream sees (nnet.CausalFeatures)
                feats = self._causal_features()(mixed, mixed_lens)
            else:
                feats = self.modules.feature_extractor(mixed)
                feats = self.modules.normalizer(feats, mixed_lens, epoch=epoch)
        if augment and "augmentation" in self.modules:           # train_librispeechmix_scratch.py:91-94
            feats = self.modules.augmentation(feats)
        feats = self.modules.frontend(feats)
        prof.stamp("mixture front-end forward done [main]")
        if prof.STAMPS and feats.requires_grad:
            feats.register_hook(lambda g: prof.stamp("mixture encoder backward done [main]"))
        enc_out = self.modules.encoder(feats, mixed_lens, speaker_embs, enroll_lens)
        enc_out = self.modules.encoder_proj(enc_out)
        prof.stamp("mixture encoder forward done [main]")
        if prof.STAMPS and enc_out.requires_grad:
            enc_out.register_hook(lambda g: prof.stamp("joint backward done [main]"))
        self._ctc_scores = None
        if "proj_ctc" in self.modules and ((stage == Stage.TRAIN and self._ctc_train(epoch)) or stage == Stage.VALID):
            fork = _CTC_STREAM == "side" and stage == Stage.TRAIN and torch.device(self.device).type == "cuda"
            if fork:
                cur, cs = torch.cuda.current_stream(), self._ctc_stream()
                cs.wait_stream(cur)
                enc_out.record_stream(cs)
            with (torch.cuda.stream(cs) if fork else contextlib.nullcontext()):
                self._ctc_scores = ctc.project(self.modules.proj_ctc, enc_out)      # raw scores [B,T',V]: the loss normalises the rows itself
            prof.stamp("ctc head forward done [main]")

        if dec_out is None:
            dec_out = self._predictor(tokens_bos, tokens_bos_lens)
        else:
            cur.wait_stream(side)
            if own:
                cur.wait_stream(third)
            dec_out.record_stream(cur)

        # joiner + transducer_head fused (train_librispeechmix_scratch.py:132-135)
        head = self.modules.transducer_head.w
        tlen = abs_lengths_round(mixed_lens, enc_out.shape[1])
        ulen = abs_lengths_round(batch.tokens.lengths.to(self.device), batch.tokens.data.shape[1])
        # hparams joint_logits: lazy -> a rnnt.JointLogits handle (the loss / alignment run the fused joint + loss kernels, no logits tensor)
        lazy = getattr(self.hparams, "joint_logits", "materialized") == "lazy"
        logits = rnnt.fused_joint_logits(enc_out, dec_out, head.weight, head.bias, self.modules.joiner.nonlinearity.negative_slope,
                                         tlen, ulen, materialize=not lazy)
        prof.stamp("joint forward done [main]")
        return logits, enc_out, tlen, ulen, epoch

    def compute_forward(self, batch, stage):
        hp = self.hparams
        logits, enc_out, _, _, epoch = self._forward_logits(batch, stage)
        hyps = None
        if stage == Stage.VALID:
            if epoch % getattr(hp, "valid_search_freq", 1) == 0 and hasattr(hp, "greedy_searcher"):
                hyps, _, _, _ = hp.greedy_searcher(enc_out)
        elif stage == Stage.TEST and hasattr(hp, "beam_searcher"):
            if getattr(hp, "hyp_ctm", None):      # timestamps of the recognised tokens: the same hypotheses, plus their emission frames
                hyps, _, _, _, frames, _ = hp.beam_searcher.forward_timed(enc_out)
                self.hyp_times.append((getattr(batch, "id", None), hyps, frames))
            else:
                hyps, _, _, _ = hp.beam_searcher(enc_out)
        if "proj_ctc" in self.modules:
            return logits, hyps, self._ctc_scores
        return logits, hyps

    def align_batch(self, batch):
        """Forced alignment of a batch's reference transcripts: ``(frames int32 [B, U], scores fp32 [B])`` on the device (rnnt.rnnt_align:
        frames[b, u] = encoder frame at which token u is emitted, -1 beyond the utterance's tokens). Eval mode, no gradients; the forward
        of compute_forward up to the joint logits with the same lengths - no searcher, no loss. The modules' training flag is restored."""
        was_training = self.modules.training
        self.modules.eval()
        try:
            with torch.no_grad():
                logits, _, tlen, ulen, _ = self._forward_logits(batch, Stage.TEST)
                return rnnt.rnnt_align(logits, self._tokens32[1], tlen, ulen, getattr(self.hparams, "blank_index", 0))
        finally:
            if was_training:
                self.modules.train()

    def compute_objectives(self, predictions, batch, stage):
        logits, hyps = predictions[:2]
        ctc_scores = predictions[2] if len(predictions) > 2 else None
        _, mixed_lens = batch.mixed_sig
        tokens, tokens_lens = batch.tokens
        t32 = getattr(self, "_tokens32", None)
        if t32 is not None and t32[0].data_ptr() == tokens.data_ptr() and t32[0].shape == tokens.shape:
            tokens = t32[1]
        loss = self.hparams.transducer_loss(logits, tokens, mixed_lens, tokens_lens)
        if stage == Stage.TRAIN and self.ctc_weight > 0:
            # train.py:153-160: ctc_weight * CTC + (1 - ctc_weight) * transducer during the CTC epochs; afterwards the CTC term is 0 and the
            # factor (1 - ctc_weight) stays
            loss = (1.0 - self.ctc_weight) * loss
            if ctc_scores is not None:
                cost = getattr(self.hparams, "ctc_cost", None)
                if cost is None or isinstance(cost, Unavailable):      # a YAML without the key: the recipe files' own setting
                    cost = functools.partial(ctc.ctc_loss, blank_index=getattr(self.hparams, "blank_index", 0), reduction="batchmean")
                fork = _CTC_STREAM == "side" and getattr(self, "_ctc_side", None) is not None
                if fork:     # (the scores were made on that stream; the term joins the main stream below)
                    cur, cs = torch.cuda.current_stream(), self._ctc_side
                    cs.wait_stream(cur)
                with (torch.cuda.stream(cs) if fork else contextlib.nullcontext()):
                    term = self.ctc_weight * cost(ctc_scores, tokens, mixed_lens, tokens_lens)
                if fork:
                    cur.wait_stream(cs)
                    term.record_stream(cur)
                loss = loss + term
        prof.stamp("loss forward done [main]")
        if hyps is not None:
            self.last_hyps = hyps
            self._score(hyps, batch)
        if stage == Stage.VALID and ctc_scores is not None:      # how far the CTC head has learnt: its greedy decoding, scored like the searcher's
            # (one device-to-host copy of the compacted tokens per VALID batch, as the searcher's own hypotheses make one: _score takes lists)
            self.last_ctc_hyps = ctc.ctc_greedy_decode(ctc_scores, mixed_lens, getattr(self.hparams, "blank_index", 0))
            cwer, ccer = getattr(self, "ctc_wer_metric", None), getattr(self, "ctc_cer_metric", None)
            if cwer is not None or ccer is not None:
                self._score(self.last_ctc_hyps, batch, cwer, ccer)
        return loss

    # ---- WER / CER statistics (train_librispeechmix_scratch.py:162-188, 197-262), scored on the device by metrics.ErrorRateStats ----
    def _metric(self, key):
        make = getattr(self.hparams, key, None)
        return make() if callable(make) and not isinstance(make, Unavailable) else None

    def _score(self, hyps, batch, wer=None, cer=None):
        """Appends a searched batch to the stage's statistics (the searcher's WER / CER objects, or the pair handed in): launches only, nothing is read back before the stage ends. With a
        tokenizer (the caller's, called as the reference calls its SentencePiece wrapper) words against batch.target_words into the
        CER and WER objects; without one the hypothesis token ids against batch.tokens cut to their lengths, into one token-level object."""
        if wer is None and cer is None:
            wer, cer = getattr(self, "wer_metric", None), getattr(self, "cer_metric", None)
        tokenizer = getattr(self, "tokenizer", None)
        if wer is None and (cer is None or tokenizer is None):
            return
        ids = getattr(batch, "id", None)
        if ids is None:      # a hand-made batch without utterance ids: number them through the stage
            ids = [f"utt{len((wer or cer).ids) + k}" for k in range(len(hyps))]
        if tokenizer is not None:
            words = tokenizer(hyps, task="decode_from_list")
            for m in (cer, wer):
                if m is not None:
                    m.append(ids, words, batch.target_words)
        else:
            tokens, rel = batch.tokens
            wer.append_ids(ids, hyps, undo_padding(tokens.cpu(), rel.cpu()))

    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        if stage != Stage.TRAIN:
            self.cer_metric, self.wer_metric = self._metric("cer_computer"), self._metric("wer_computer")
        if stage == Stage.VALID and "proj_ctc" in self.modules:
            self.ctc_cer_metric, self.ctc_wer_metric = self._metric("cer_computer"), self._metric("wer_computer")
        if stage == Stage.TEST:
            self.hyp_times = []      # (utterance ids, hypotheses, emission frames) per batch when hparams.hyp_ctm is set

    def on_stage_end(self, stage, stage_loss, epoch=None):
        super().on_stage_end(stage, stage_loss, epoch)
        hp = self.hparams
        stats = {"loss": stage_loss}
        if stage == Stage.TRAIN:
            self.train_stats = stats
            return
        wer, cer = getattr(self, "wer_metric", None), getattr(self, "cer_metric", None)
        current = hp.epoch_counter.current if hasattr(hp, "epoch_counter") else 0
        searched = wer is not None and (stage == Stage.TEST or current % getattr(hp, "valid_search_freq", 1) == 0)
        if searched and self.distributed:      # every rank takes part, also one that saw no batch
            for m in (cer, wer):
                if m is not None:
                    merge_across_ranks(m)
        searched = searched and (len(wer.ids) > 0 or len(wer.scores) > 0)      # (no searcher in the YAML: nothing was appended)
        if searched:
            if getattr(self, "tokenizer", None) is not None:
                if cer is not None:
                    stats["CER"] = cer.summarize("error_rate")
                stats["WER"] = wer.summarize("error_rate")
            else:
                stats["TER"] = wer.summarize("error_rate")
        cwer, ccer = getattr(self, "ctc_wer_metric", None), getattr(self, "ctc_cer_metric", None)
        if stage == Stage.VALID and "proj_ctc" in self.modules and cwer is not None:      # the CTC head's greedy decoding, every VALID stage
            if self.distributed:
                for m in (ccer, cwer):
                    if m is not None:
                        merge_across_ranks(m)
            if len(cwer.ids) > 0 or len(cwer.scores) > 0:
                if getattr(self, "tokenizer", None) is not None:
                    if ccer is not None:
                        stats["ctc_CER"] = ccer.summarize("error_rate")
                    stats["ctc_WER"] = cwer.summarize("error_rate")
                else:
                    stats["ctc_TER"] = cwer.summarize("error_rate")
        # (the reference logs through hparams.train_logger and keeps checkpoints by WER here: both are Unavailable, the caller's)
        if stage == Stage.VALID:
            self.valid_stats = stats
        else:
            self.test_stats = stats
            if searched and self.rank == 0 and getattr(hp, "wer_file", None):
                with open(hp.wer_file, "w") as w:
                    wer.write_stats(w)

    def on_fit_batch_end(self, batch, outputs, loss, should_step):
        if getattr(self.hparams, "enable_scheduler", False) and should_step:
            self.hparams.noam_scheduler(self.optimizer)
