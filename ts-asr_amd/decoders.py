"""Transducer search with the reference's constructor/return shape (speechbrain/decoders/transducer.py:14-373).

beam_size = 1 -> greedy (transducer.py:138-218): at most one symbol per encoder frame; the predictor state of an utterance
advances only when it emitted a non-blank. The per-frame decision stays on the device (argmax + masked state update, no
per-item Python loop as in transducer.py:187-194); only the final token table is read back.
beam_size > 1 -> the reference's per-utterance beam search with state_beam / expand_beam pruning (transducer.py:220-373).
For the recipes' networks one launch of csrc/search.hip decodes the batch (tsasr_beam_search: fp64 scores, the
reference's list order, one predictor step per hypothesis node); utterances that need more than ``cap`` hypotheses in a frame, and
every other network shape, run the host loop: host-side hypothesis bookkeeping exactly as specified there (SURVEY.md section 8f
row f1), device-side predictor / joint / head steps. Pinned to the reference's own hypotheses by tests/golden/c1_beam.npz.
Subword models (64 <= V <= 1024, or an embedding of up to 1024 columns; beam_size <= 64) run the same search in
beam_search_kernel's WIDE instantiations (tsasr_beam_search with wide set: offline, streams, timestamps and LM fusion alike).

LM fusion (lm_module, lm_weight > 0; transducer.py:95-110, 264-266, 311-351, 386-409): a hypothesis also carries the LM's state; each
expansion of a runs the LM on a's last token (blank doubles as its BOS) from a's LM state; a non-blank extension by sym takes the new
state and scores (logp(a) + logp_joint[sym]) + lm_weight * logp_lm[sym]; the top-k, the expand_beam test and the blank copies read
the joint alone. An nnet.RNNLM of the shapes _device_lm_ok lists is fused into the device search (tsasr_beam_search's lm: one LM step
per node, beside its predictor step); any other module with the reference's call form runs in the host loop. Greedy search never uses
the LM. Pinned to the reference's hypotheses by tests/golden/c1_beam_lm.npz.

Timestamps (forward_timed, greedy_stream / beam_stream with return_frames=True): frames[i] = index of the encoder frame whose joint
emitted token i, absolute from the start of the utterance or stream. Greedy emits at most one symbol per frame, so the frame is the
token's column in the kernel's ``preds``; the beam search never merges paths, so each hypothesis carries one frame list (the device
search records it per tree node, tsasr_beam_search's frames; the host loop carries it with the hypothesis). Seconds and word spans:
align.frame_seconds / align.word_spans.

Contextual biasing (``bias``: a biasing.ContextGraph for every utterance, or a list of B entries, each a graph or None; biasing.py
states the rule): a hypothesis also carries a trie state, 0 at the start; a blank copy keeps it; a non-blank extension by sym moves it
(graph.step) and adds the step's bonus d last, after the joint's and the LM's terms; the n-best is ranked and reported with
(logp - pending[state]) / len while the beam itself keeps logp. The host loop below is the definition; the device search carries the
state per tree node (tsasr_beam_search's bias). With no graph (None, an empty graph, a list of them) every call is today's.
"""
import os
import warnings

import torch
import torch.nn.functional as F

GREEDY_WIDE_MAX = 1024          # vocabulary and embedding columns the device greedy search takes (csrc/search.hip greedy_decode_kernel's WIDE instantiations)
BEAM_CAP = 512                  # hypotheses one frame of the device beam search may hold (its A list); past it: the host loop
BEAM_STREAM_FRAMES = 4096       # frames a beam_stream workspace is laid out for when the caller does not say
BEAM_HOST_REDECODES = {"utterances": 0}     # utterances the device beam search handed back to the host loop (status != 0)
_NO_GRAPH_YET = object()        # beam_stream: a stream of a biased state whose graph has not been named since its (re)start


class TransducerBeamSearcher(torch.nn.Module):
    def __init__(self, decode_network_lst, tjoint, classifier_network, blank_id, beam_size=4, nbest=5, lm_module=None,
                 lm_weight=0.0, state_beam=2.3, expand_beam=2.3, cap=BEAM_CAP, bias=None):
        super().__init__()
        self.decode_network_lst, self.tjoint, self.classifier_network = decode_network_lst, tjoint, classifier_network
        self.blank_id, self.beam_size, self.nbest = blank_id, beam_size, nbest
        self.state_beam, self.expand_beam = state_beam, expand_beam
        self.cap = int(cap)
        self.lm, self.lm_weight = lm_module, lm_weight
        if lm_module is None and lm_weight > 0:
            raise ValueError("Language model is not provided.")
        self.bias = bias

    @property
    def bias(self):
        """The phrase graphs of the beam search (biasing.py): None, one ContextGraph for every utterance, or a list with one entry
        (a graph or None) per utterance of the batches to come. Set like ``lm``; ``forward(..., bias=)`` overrides it for a call."""
        return self._bias

    @bias.setter
    def bias(self, value):
        self._check_bias(value)
        self._bias = value

    def _vocab(self):
        head = self.classifier_network[0] if len(self.classifier_network) else None
        lin = getattr(head, "w", head)
        return getattr(lin, "out_features", None)

    def _check_bias(self, bias):
        from .biasing import ContextGraph
        if bias is None:
            return
        for g in ([bias] if isinstance(bias, ContextGraph) else list(bias)):
            if g is not None:
                if not isinstance(g, ContextGraph):
                    raise ValueError("bias must be a biasing.ContextGraph or a list whose entries are ContextGraph or None")
                g.check(self.blank_id, self._vocab())

    def _bias_graphs(self, bias, B):
        """The call's graphs as a list of B entries (a graph or None), checked against the blank and the vocabulary; None if no utterance
        is biased."""
        from .biasing import as_list
        self._check_bias(bias)
        graphs = as_list(bias, B)
        return graphs if any(g is not None for g in graphs) else None

    def forward(self, tn_output, bias=None):
        bias = self.bias if bias is None else bias
        if self.beam_size <= 1:
            return self.transducer_greedy_decode(tn_output)           # (greedy search is not biased)
        if bias is None:
            return self.transducer_beam_search_decode(tn_output)
        return self.transducer_beam_search_decode(tn_output, bias=bias)

    def forward_timed(self, tn_output, bias=None):
        """forward's four values (the same lists, the same score bits) and then ``frames`` and ``nbest_frames``: frames[b][i] is the
        encoder frame that emitted hyps[b][i], nbest_frames[b][r][i] that of nbest_hyps[b][r][i] (None for greedy). Every frame of
        tn_output is decoded, padding included, so a frame may lie past an utterance's valid length."""
        bias = self.bias if bias is None else bias
        if self.beam_size <= 1:
            return self.transducer_greedy_decode(tn_output, timed=True)
        if bias is None:
            return self.transducer_beam_search_decode(tn_output, timed=True)
        return self.transducer_beam_search_decode(tn_output, timed=True, bias=bias)

    @staticmethod
    def _unpack_preds(preds, base=None):
        """preds [B,T] (symbol emitted at each frame or -1) -> (symbol lists, frame lists) with one device-to-host copy; ``base`` int
        [B] on the device = frames decoded before column 0 (travels as an extra column)."""
        if base is not None:
            preds = torch.cat([preds, base.to(preds.dtype)[:, None]], dim=1)
        rows = preds.cpu()
        off = [0] * rows.shape[0] if base is None else rows[:, -1].tolist()
        if base is not None:
            rows = rows[:, :-1]
        hyps = [[int(v) for v in row[row >= 0]] for row in rows]
        frames = [[int(t) + int(o) for t in torch.nonzero(row >= 0).flatten()] for row, o in zip(rows, off)]
        return hyps, frames

    def _pn(self, tok, hidden):
        emb, dec, proj = self.decode_network_lst
        out, hidden = dec(emb(tok), hx=hidden)
        return proj(out), hidden

    def _device_greedy_ok(self, tn_output):
        """The one-launch device decoder (csrc/search.hip) covers the recipes' networks: one-hot or learned embedding, one-layer
        unidirectional LSTM, Linear projection, joint = LeakyReLU(sum), one Linear classifier. Character models (V <= 63, embedding <= 64
        columns) run the narrow instantiation, subword models up to V = 1024 and 1024 embedding columns the wide one."""
        if os.environ.get("TSASR_GREEDY_KERNEL", "1") == "0":
            return False
        if not self._device_net_ok(tn_output, GREEDY_WIDE_MAX, GREEDY_WIDE_MAX):
            return False
        # the launchers' own limits (hidden size and joint dimension up to 1024; the kernel's LDS then always fits): a network past them
        # decodes through the host loop instead of meeting the entry point's argument check
        return bool(self.decode_network_lst[1].rnn.hidden_size <= 1024 and tn_output.shape[-1] <= 1024)

    def _greedy_is_wide(self):
        return self.decode_network_lst[0].embedding_dim > 64 or self.classifier_network[0].w.out_features > 63

    def _device_beam_ok(self, tn_output, bias=False):
        """The one-launch device beam search (csrc/search.hip) takes the networks the greedy decoder takes, with 2 <= beam_size <= V,
        nbest <= 64 and cap >= beam_size; subword models (_beam_is_wide) also need beam_size <= 64 and a shape whose search fits the
        kernel's LDS. TSASR_BEAM_KERNEL=0 sends every call to the host loop."""
        if os.environ.get("TSASR_BEAM_KERNEL", "1") == "0" or not self._device_net_ok(tn_output, GREEDY_WIDE_MAX, GREEDY_WIDE_MAX):
            return False
        rnn, V = self.decode_network_lst[1].rnn, self.classifier_network[0].w.out_features
        if self.lm_weight > 0 and not self._device_lm_ok(V):
            return False
        ok = bool(2 <= self.beam_size <= V and 1 <= self.nbest <= 64 and self.cap >= self.beam_size and rnn.hidden_size <= 1024
                  and tn_output.shape[-1] <= 1024 and tn_output.shape[0] > 0 and tn_output.shape[1] > 0)
        if ok and self._beam_is_wide():
            from . import ops
            lm_rnn = self.lm.rnn.rnn if self.lm_weight > 0 else None
            lm_dims = (self.lm.embedding.embedding_dim, lm_rnn.hidden_size, self.lm.out.w.in_features) if lm_rnn is not None else None
            ok = self.beam_size <= 64 and ops.beam_wide_lds_bytes(rnn.hidden_size, tn_output.shape[-1], self.decode_network_lst[0].embedding_dim,
                                                                  V, self.cap, lm_dims, bias=bool(bias)) <= ops.BEAM_WIDE_LDS_MAX
        return ok

    def _beam_is_wide(self):
        """Subword models (V > 63 or an embedding wider than 64 columns) run beam_search_kernel's WIDE instantiations, character models the narrow ones."""
        return self._greedy_is_wide()

    def _device_lm_ok(self, V):
        """The LMs the device search fuses: an nnet.RNNLM in eval mode over the same V symbols with 1-4 LSTM layers, 0-2 dnn blocks with
        LeakyReLU, and rnn_neurons, embedding_dim, dnn_neurons multiples of 4 up to 1024."""
        from . import nnet
        lm = self.lm
        if not isinstance(lm, nnet.RNNLM) or not isinstance(lm.rnn, nnet.LSTM) or lm.training:
            return False
        rnn, emb, blocks = lm.rnn.rnn, lm.embedding, lm.dnn_layers()
        size_ok = lambda n: 0 < n <= 1024 and n % 4 == 0  # noqa: E731
        ok = (1 <= rnn.num_layers <= 4 and not rnn.bidirectional and getattr(rnn, "proj_size", 0) == 0 and size_ok(rnn.hidden_size)
              and not emb.consider_as_one_hot and size_ok(emb.embedding_dim) and emb.num_embeddings == V and rnn.input_size == emb.embedding_dim
              and len(blocks) <= 2 and lm.out.w.out_features == V and size_ok(lm.out.w.in_features)
              and all(isinstance(b[0], nnet.Linear) and isinstance(b[1], nnet.LayerNorm) and isinstance(b[2], torch.nn.LeakyReLU)
                      and b[0].w.out_features == lm.out.w.in_features and b[2].negative_slope == blocks[0][2].negative_slope for b in blocks)
              and (blocks or lm.out.w.in_features == rnn.hidden_size))
        return bool(ok)

    def _device_lm_args(self, enc):
        """The fused LM's tensors as ops.beam_search(lm=) takes them: matrices in the predictor's weight dtype (the bf16 shadows with
        bf16 activations), the embedding table, biases and LayerNorm vectors fp32."""
        from .ops import _bf16_weight
        f = lambda t: None if t is None else t.detach().float().contiguous()  # noqa: E731
        w = (lambda t: _bf16_weight(t).contiguous()) if enc.dtype == torch.bfloat16 else f
        lm = self.lm
        rnn, blocks = lm.rnn.rnn, lm.dnn_layers()
        layers = range(rnn.num_layers)
        bias = lambda name: [f(getattr(rnn, f"{name}_l{l}")) if rnn.bias else None for l in layers]  # noqa: E731
        return dict(emb=f(lm.embedding.Embedding.weight), w_ih=[w(getattr(rnn, f"weight_ih_l{l}")) for l in layers],
                    w_hh=[w(getattr(rnn, f"weight_hh_l{l}")) for l in layers], b_ih=bias("bias_ih"), b_hh=bias("bias_hh"),
                    w_dnn=[w(b[0].w.weight) for b in blocks], b_dnn=[f(b[0].w.bias) for b in blocks],
                    ln_g=[f(b[1].norm.weight) for b in blocks], ln_b=[f(b[1].norm.bias) for b in blocks], ln_eps=[b[1].eps for b in blocks],
                    w_out=w(lm.out.w.weight), b_out=f(lm.out.w.bias), slope=blocks[0][2].negative_slope if blocks else 0.01,
                    weight=float(self.lm_weight))

    def _device_net_ok(self, tn_output, emb_max, vocab_max):
        """The network shape csrc/search.hip takes, with the caller's limits on the embedding width and the vocabulary: the greedy and
        the beam search (with LM fusion) both go to GREEDY_WIDE_MAX, in the WIDE instantiations past 64 columns / V = 63."""
        from . import nnet, rnnt
        if not tn_output.is_cuda or tn_output.dtype not in (torch.float32, torch.bfloat16):
            return False
        if len(self.decode_network_lst) != 3 or len(self.classifier_network) != 1:
            return False
        emb, dec, proj = self.decode_network_lst
        head = self.classifier_network[0]
        ok = (isinstance(emb, nnet.Embedding) and isinstance(dec, nnet.LSTM) and isinstance(proj, nnet.Linear) and isinstance(head, nnet.Linear)
              and isinstance(self.tjoint, rnnt.Transducer_joint) and isinstance(self.tjoint.nonlinearity, torch.nn.LeakyReLU)
              and dec.rnn.num_layers == 1 and not dec.rnn.bidirectional and emb.embedding_dim <= emb_max and head.w.out_features <= vocab_max
              and dec.rnn.hidden_size % 4 == 0 and proj.w.out_features % 4 == 0 and proj.w.out_features == tn_output.shape[-1])
        return bool(ok)

    @torch.no_grad()
    def _greedy_on_device(self, tn_output, timed=False):
        from . import ops
        enc = tn_output.contiguous()
        table, mats, b_ih, b_hh, b_proj, b_head, wdt = self._device_greedy_args(enc)   # (bf16 activations: the bf16 weight shadows)
        preds, logp = ops.greedy_decode(enc, table, mats, b_ih, b_hh, b_proj, b_head, self.blank_id,
                                        self.tjoint.nonlinearity.negative_slope, wdt)
        if timed:
            hyps, frames = self._unpack_preds(preds)
            return hyps, logp.exp().mean(), None, None, frames, None
        rows = preds.cpu()
        hyps = [[int(v) for v in row[row >= 0]] for row in rows]
        return hyps, logp.exp().mean(), None, None

    def _device_greedy_args(self, enc):
        """(embedding table, [W_ih, W_hh, W_proj, W_head], b_ih, b_hh, b_proj, b_head, weight dtype) as csrc/search.hip reads them."""
        from . import _capi as C
        emb, dec, proj = self.decode_network_lst
        head = self.classifier_network[0]
        f = lambda t: None if t is None else t.detach().float().contiguous()  # noqa: E731
        rnn = dec.rnn
        mats = [rnn.weight_ih_l0, rnn.weight_hh_l0, proj.w.weight, head.w.weight]
        if enc.dtype == torch.bfloat16:
            from .ops import _bf16_weight
            mats, wdt = [_bf16_weight(m).contiguous() for m in mats], C.BF16
        else:
            mats, wdt = [f(m) for m in mats], C.F32
        b_ih, b_hh = (f(rnn.bias_ih_l0), f(rnn.bias_hh_l0)) if rnn.bias else (None, None)
        return f(emb.Embedding.weight), mats, b_ih, b_hh, f(proj.w.bias), f(head.w.bias), wdt

    def greedy_stream(self, enc_chunk, state=None, n_valid=None, return_frames=False):
        """Greedy search over the next frames of a batch of streams: enc_chunk [B,C,J] (the encoder_proj output of one chunk), ``state``
        the value returned by the previous call (None: start of the streams, the predictor is primed with blank as in the one-call
        search), n_valid int32 [B] = frames of this chunk that belong to each stream (None: all C). Frames past a stream's count are not
        decoded and leave its state untouched. Returns (new symbols of each stream, state); state["logp_sum"] is the running sum of
        the emitted symbols' log-probabilities. Decoding a sequence in chunks gives the same symbols as one call over it: the
        device kernel (csrc/search.hip) carries the predictor state bit for bit, the step-wise loop carries it as tensors.
        return_frames=True (fixed at the first call of a stream; a later call with the other value raises ValueError): returns (new symbols, their frames, state); a frame is absolute in its stream,
        the token's column in this chunk plus state["frames_done"], the frames of the stream decoded by earlier calls."""
        if torch.is_grad_enabled():
            raise RuntimeError("greedy_stream is inference only: run it under torch.no_grad()")
        B, T, _ = enc_chunk.shape
        dev = enc_chunk.device
        nv = torch.full((B,), T, dtype=torch.int32, device=dev) if n_valid is None else n_valid.to(device=dev, dtype=torch.int32)
        if state is not None and ("frames_done" in state) != bool(return_frames):      # (an untimed call would not advance the count)
            raise ValueError(f"greedy_stream: this stream was started with return_frames={'frames_done' in state}")
        done = (torch.zeros(B, dtype=torch.int32, device=dev) if state is None else state["frames_done"]) if return_frames else None
        if self._device_greedy_ok(enc_chunk):
            from . import ops
            enc = enc_chunk.contiguous()
            table, mats, b_ih, b_hh, b_proj, b_head, wdt = self._device_greedy_args(enc)
            if state is None:
                S = ops.greedy_stream_state_size(mats[1].shape[1], enc.shape[-1])
                state = {"dev": torch.zeros(B, S, dtype=torch.float32, device=dev)}
            preds, logp = ops.greedy_decode_stream(enc, table, mats, b_ih, b_hh, b_proj, b_head, state["dev"], nv, self.blank_id,
                                                   self.tjoint.nonlinearity.negative_slope, wdt)
            state["logp_sum"] = logp
            if return_frames:
                state["frames_done"] = done + nv.clamp(0, T)
                return self._unpack_preds(preds, done) + (state,)
            rows = preds.cpu()
            return [[int(v) for v in row[row >= 0]] for row in rows], state
        if state is None:
            tok = torch.full((B, 1), self.blank_id, dtype=torch.long, device=dev)
            out_pn, hidden = self._pn(tok, None)
            state = {"tok": tok, "out_pn": out_pn, "hidden": hidden, "logp_sum": torch.zeros(B, device=dev)}
        tok, out_pn, hidden, logp_sum = state["tok"], state["out_pn"], state["hidden"], state["logp_sum"]
        preds = torch.full((B, T), -1, dtype=torch.long, device=dev)
        for t in range(T):
            live = t < nv
            j = self.tjoint(enc_chunk[:, t, :].unsqueeze(1).unsqueeze(1), out_pn.unsqueeze(1))
            for layer in self.classifier_network:
                j = layer(j)
            logp, pos = torch.max(F.log_softmax(j.float(), dim=-1).squeeze(1).squeeze(1), dim=1)
            upd = (pos != self.blank_id) & live
            preds[:, t] = torch.where(upd, pos, preds[:, t])
            logp_sum = logp_sum + torch.where(upd, logp, torch.zeros_like(logp))
            new_tok = torch.where(upd, pos, tok[:, 0]).unsqueeze(1)
            new_out, new_hidden = self._pn(new_tok, hidden)
            out_pn = torch.where(upd.view(B, 1, 1), new_out, out_pn)
            hidden = tuple(torch.where(upd.view(1, B, 1), nh, h) for nh, h in zip(new_hidden, hidden))
            tok = new_tok
        state = {"tok": tok, "out_pn": out_pn, "hidden": hidden, "logp_sum": logp_sum}
        if return_frames:
            state["frames_done"] = done + nv.clamp(0, T)
            return self._unpack_preds(preds, done) + (state,)
        rows = preds.cpu()
        return [[int(v) for v in row[row >= 0]] for row in rows], state

    @torch.no_grad()
    def transducer_greedy_decode(self, tn_output, timed=False):
        if self._device_greedy_ok(tn_output):
            return self._greedy_on_device(tn_output, timed)
        B, T, _ = tn_output.shape
        dev = tn_output.device
        tok = torch.full((B, 1), self.blank_id, dtype=torch.long, device=dev)
        out_pn, hidden = self._pn(tok, None)
        preds = torch.full((B, T), -1, dtype=torch.long, device=dev)
        logp_sum = torch.zeros(B, device=dev)
        for t in range(T):
            j = self.tjoint(tn_output[:, t, :].unsqueeze(1).unsqueeze(1), out_pn.unsqueeze(1))
            for layer in self.classifier_network:
                j = layer(j)
            logp, pos = torch.max(F.log_softmax(j.float(), dim=-1).squeeze(1).squeeze(1), dim=1)
            upd = pos != self.blank_id
            preds[:, t] = torch.where(upd, pos, preds[:, t])
            logp_sum = logp_sum + torch.where(upd, logp, torch.zeros_like(logp))
            new_tok = torch.where(upd, pos, tok[:, 0]).unsqueeze(1)
            new_out, new_hidden = self._pn(new_tok, hidden)
            m = upd.view(B, 1, 1)
            out_pn = torch.where(m, new_out, out_pn)
            hidden = tuple(torch.where(upd.view(1, B, 1), nh, h) for nh, h in zip(new_hidden, hidden))
            tok = new_tok
        if timed:
            hyps, frames = self._unpack_preds(preds)
            return hyps, logp_sum.exp().mean(), None, None, frames, None
        table = preds.cpu()
        hyps = [[int(x) for x in row[row >= 0]] for row in table]
        return hyps, logp_sum.exp().mean(), None, None

    @torch.no_grad()
    def transducer_beam_search_decode(self, tn_output, timed=False, bias=None):
        """Returns (best hyps, mean exp(normalised score), n-best hyps, n-best normalised log-scores) like the reference.
        A = hypotheses still to be extended at this frame, B = those that emitted blank here (the next frame's A). Until
        |B| >= beam: take the best a in A by logp / len(prediction); stop once the best b in B has logp >= state_beam + logp(a);
        run the predictor on a's last token, score the beam best symbols of the joint at this frame; blank closes a copy of
        a into B, a non-blank symbol within expand_beam of the best non-blank extends a (new predictor state) back into A.
        The recipes' networks run on the device (_device_beam_ok); an utterance the device search could not finish within ``cap``
        hypotheses per frame is decoded again by the host loop (counted in BEAM_HOST_REDECODES). ``timed`` (forward_timed): two more
        values, the best hypotheses' emission frames and the n-best's. ``bias``: the call's phrase graphs (biasing.py)."""
        graphs = self._bias_graphs(bias, tn_output.shape[0]) if bias is not None else None
        if graphs is not None:
            if self._device_beam_ok(tn_output, bias=True):
                return self._beam_on_device(tn_output, timed=timed, graphs=graphs)
            return self._beam_host_loop(tn_output, timed, graphs)
        if self._device_beam_ok(tn_output):
            # (the untimed call keeps its one-argument form: callers and tests wrap _beam_on_device(tn_output))
            return self._beam_on_device(tn_output, timed=True) if timed else self._beam_on_device(tn_output)
        return self._beam_host_loop(tn_output, timed)

    def _beam_host_loop(self, tn_output, timed=False, graphs=None):
        """``graphs``: None, or one entry per utterance (a ContextGraph or None); with it every hypothesis carries a trie state."""
        nbest_batch, nbest_scores, nbest_frames = [], [], []
        biased = graphs is not None
        for b in range(tn_output.shape[0]):
            # (prediction incl. the blank prefix, logp, predictor state); timed: + the emission frames of the prediction's tokens;
            # biased: + the trie state; LM fusion: + the LM's state, last
            g = graphs[b] if biased else None
            beam = [self._beam_start(timed, biased)]
            for t in range(tn_output.shape[1]):
                beam = self._beam_frame(beam, tn_output[b, t, :], t if timed else None, g, biased)
            ranked = self._beam_rank(beam, timed, g, biased)
            nbest_batch.append(ranked[0])
            nbest_scores.append(ranked[1])
            if timed:
                nbest_frames.append(ranked[2])
        best = [n[0] for n in nbest_batch]
        out = best, torch.tensor([s_[0] for s_ in nbest_scores]).exp().mean(), nbest_batch, nbest_scores
        return out + ([n[0] for n in nbest_frames], nbest_frames) if timed else out

    def _beam_start(self, timed=False, biased=False):
        """The hypothesis a search starts from: ([blank], 0.0, no predictor state) + ([] if timed) + (trie state 0 if biased) + (no LM
        state if the LM is used)."""
        return ([self.blank_id], 0.0, None) + (([],) if timed else ()) + ((0,) if biased else ()) + ((None,) if self.lm_weight > 0 else ())

    def _beam_frame(self, A, enc_t, t=None, graph=None, biased=False):
        """One frame of the host loop: the beam that leaves frame ``enc_t`` [J] when ``A`` enters it. ``t`` (not None: the hypotheses
        carry their frame lists at index 3) = absolute index of this frame, recorded for every token emitted here. ``biased``: the
        hypotheses carry a trie state behind the frames (index 3, timed: 4), moved by ``graph`` (None: this utterance has no graph, the
        state stays 0 and nothing is added). With the LM in use the last element of a hypothesis is its LM state."""
        key = lambda hyp: hyp[1] / len(hyp[0])  # noqa: E731
        use_lm = self.lm_weight > 0
        ci = 3 if t is None else 4
        dev = enc_t.device
        frame = enc_t.view(1, 1, 1, -1)
        beam = []
        while len(beam) < self.beam_size:
            a = max(A, key=key)
            if beam and max(beam, key=key)[1] >= self.state_beam + a[1]:
                break
            A.remove(a)
            tok = torch.full((1, 1), a[0][-1], dtype=torch.long, device=dev)
            out_pn, new_state = self._pn(tok, a[2])
            j = self.tjoint(frame, out_pn.unsqueeze(0))
            for layer in self.classifier_network:
                j = layer(j)
            logp, pos = torch.topk(F.log_softmax(j.float(), dim=-1).view(-1), k=self.beam_size)
            logp, pos = logp.tolist(), pos.tolist()      # one host read per expansion (the reference: one per symbol)
            if use_lm:                                   # transducer.py:311-314, 386-409: the LM on a's last token from a's LM state
                lm_logits, lm_state = self.lm(tok, hx=a[-1])
                lm_logp = F.log_softmax(lm_logits.float(), dim=-1).view(-1).tolist()
            best_nonblank = logp[0] if pos[0] != self.blank_id else logp[1]
            for lp, sym in zip(logp, pos):
                if sym == self.blank_id:                 # (a's frames and LM state travel in a[3:])
                    beam.append((a[0][:], a[1] + lp, a[2]) + a[3:])
                elif lp >= best_nonblank - self.expand_beam:
                    sc = (a[1] + lp) + self.lm_weight * lm_logp[sym] if use_lm else a[1] + lp
                    ctx = ()
                    if biased:
                        ctx = (0,)
                        if graph is not None:                # the trie step of a's state on sym; its bonus comes last
                            cs, d = graph.step(a[ci], sym)
                            sc, ctx = sc + d, (cs,)
                    A.append((a[0] + [sym], sc, new_state) + (() if t is None else (a[3] + [t],)) + ctx + ((lm_state,) if use_lm else ()))
        return beam

    def _beam_rank(self, beam, timed=False, graph=None, biased=False):
        """(n-best symbol lists, their logp / len) of a beam: sorted(beam, key, reverse=True)[:nbest] (stable, as the reference);
        ``timed``: and their frame lists. ``graph``: ranked and reported with (logp - pending[state]) / len, a phrase left half-matched
        earns nothing; the beam itself is left as it is."""
        ci = 4 if timed else 3
        key = (lambda hyp: (hyp[1] - float(graph.pending[hyp[ci]])) / len(hyp[0])) if biased and graph is not None else (
            lambda hyp: hyp[1] / len(hyp[0]))
        ranked = sorted(beam, key=key, reverse=True)[: self.nbest]
        out = [h[0][1:] for h in ranked], [key(h) for h in ranked]
        return out + ([list(h[3]) for h in ranked],) if timed else out

    def _device_beam_call(self, enc, fn, *extra, **kw):
        table, mats, b_ih, b_hh, b_proj, b_head, wdt = self._device_greedy_args(enc)   # (bf16 activations: the bf16 weight shadows)
        if self.lm_weight > 0:
            kw["lm"] = self._device_lm_args(enc)
        if self._beam_is_wide():
            kw["wide"] = True
        return fn(enc, table, mats, b_ih, b_hh, b_proj, b_head, self.blank_id, self.tjoint.nonlinearity.negative_slope, wdt, self.beam_size,
                  self.nbest, self.state_beam, self.expand_beam, self.cap, *extra, **kw)

    @staticmethod
    def _beam_kw(timed, graphs, device):
        """The keywords of a _device_beam_call: ``graphs`` (None: unbiased) packed for the device."""
        if graphs is None:
            return dict(frames=bool(timed))
        from .biasing import pack
        return dict(frames=bool(timed), bias=pack(graphs, device))

    @torch.no_grad()
    def _beam_on_device(self, tn_output, timed=False, graphs=None):
        from . import ops
        enc = tn_output.contiguous()
        out = self._device_beam_call(enc, ops.beam_search, **self._beam_kw(timed, graphs, enc.device))
        nbest_batch, nbest_scores, status = out[:3]
        nbest_frames = out[3] if timed else None
        bad = [b for b in range(enc.shape[0]) if int(status[b]) != 0]
        if bad:
            if BEAM_HOST_REDECODES["utterances"] == 0:
                warnings.warn(f"ts-asr_amd: the device beam search stopped {len(bad)} utterance(s) "
                              f"({sorted({ops.BEAM_STATUS[int(status[b])] for b in bad})}, cap={self.cap}); they are decoded by the host "
                              f"loop (counted in decoders.BEAM_HOST_REDECODES)", RuntimeWarning, stacklevel=3)
            BEAM_HOST_REDECODES["utterances"] += len(bad)
            for b in bad:
                redo = self._beam_host_loop(enc[b:b + 1], timed, None if graphs is None else [graphs[b]])
                nbest_batch[b], nbest_scores[b] = redo[2][0], redo[3][0]
                if timed:
                    nbest_frames[b] = redo[5][0]
        best = [n[0] for n in nbest_batch]
        out = best, torch.tensor([s_[0] for s_ in nbest_scores]).exp().mean(), nbest_batch, nbest_scores
        return out + ([n[0] for n in nbest_frames], nbest_frames) if timed else out

    @torch.no_grad()
    def reset_streams(self, state, slots):
        """Put the streams ``slots`` (indices into the batch) of a greedy_stream / beam_stream state back to the start of a stream, in
        place; every other stream keeps its bits. Device greedy: the slot's row of the [B, 2H+J+4] state and its frames_done are zeroed.
        Device beam: the slot's block of the workspace (B equal blocks, untimed, timed, LM, wide and biased layouts alike) is zeroed,
        which also clears a sticky status; a biased state also forgets the slot's graph. Host routes: the slot's predictor state / beam list starts afresh. ``state`` None (no call made
        yet: every stream is at its start) is returned as it is."""
        if state is None:
            return state
        slots = [int(b) for b in slots]
        if "graphs" in state:                                  # biased beam search: the streams' graphs are forgotten
            for b in slots:
                state["graphs"][b] = _NO_GRAPH_YET
        if "beams" in state:                                   # beam search, host route
            timed = "frames_done" in state
            for b in slots:
                state["beams"][b] = [self._beam_start(timed, "graphs" in state)]
                if timed:
                    state["frames_done"][b] = 0
        elif "tok" in state:                                   # greedy search, host route
            idx = torch.as_tensor(slots, dtype=torch.long, device=state["tok"].device)
            tok = torch.full((len(slots), 1), self.blank_id, dtype=torch.long, device=idx.device)
            out_pn, hidden = self._pn(tok, None)
            state["tok"][idx] = tok
            state["out_pn"][idx] = out_pn.to(state["out_pn"].dtype)
            for old, new in zip(state["hidden"], hidden):
                old[:, idx] = new.to(old.dtype)
            state["logp_sum"][idx] = 0
        elif "max_frames" in state:                            # beam search, device route: B equal blocks of the workspace
            per_utt = state["dev"].numel() // state["B"]
            for b in slots:
                state["dev"][b * per_utt:(b + 1) * per_utt].zero_()
        else:                                                  # greedy search, device route
            state["dev"][torch.as_tensor(slots, dtype=torch.long, device=state["dev"].device)] = 0
            if "logp_sum" in state:
                state["logp_sum"] = state["logp_sum"].clone()
                state["logp_sum"][slots] = 0
        if isinstance(state.get("frames_done"), torch.Tensor):
            state["frames_done"] = state["frames_done"].clone()
            state["frames_done"][slots] = 0
        for b in slots:                                        # the n-best lists of the last call describe the stream that left
            if "nbest" in state:
                state["nbest"][b], state["scores"][b] = [[]], [0.0]
            if "frames" in state:
                state["frames"][b] = [[]]
        return state

    def beam_stream(self, enc_chunk, state=None, n_valid=None, max_frames=None, return_frames=False, raise_stopped=True, bias=None):
        """Beam search over the next frames of a batch of streams, the counterpart of greedy_stream: enc_chunk [B,C,J], ``state`` the
        value returned by the previous call (None: start of the streams), n_valid int32 [B] = frames of this chunk that belong to each
        stream (None: all C); max_frames = frames a stream may reach (device route; default BEAM_STREAM_FRAMES), read at the first call.
        Returns (current best hypothesis of each stream, state); state["nbest"] / state["scores"] hold the n-best lists and their
        logp / len. Under beam search the best prefix can change, so the whole hypothesis is returned, not new symbols. Decoding a
        sequence in chunks gives the bits of one call over it: the device route resumes its workspace (csrc/search.hip), the host
        route carries the beam lists. A stream past ``cap`` hypotheses in a frame cannot be re-decoded chunk by chunk: RuntimeError.
        return_frames=True: the state also carries state["frames"], the n-best lists of emission frames (absolute in the stream) that
        match state["nbest"]. The flag is fixed at the first call of a stream (the timed device workspace has its own layout, the
        host hypotheses carry their frames): a later call with the other value raises ValueError.
        raise_stopped=False (device route): stopped streams do not raise; the state is stored for every stream and state["stopped"]
        lists them (a stopped stream stays stopped until reset_streams).
        bias (biasing.py; one ContextGraph or a list of B entries, each a graph or None): read at the first call of a state, where any
        value but None selects the biased layout for good (the device workspace holds a trie state per node, the host hypotheses carry
        theirs), also a list of None. The state remembers each stream's graph by identity: a later call names the same graphs or passes
        None (= as before); another graph for a stream that has not been reset raises ValueError. reset_streams forgets the graph of the
        streams it restarts, the next call names their new one (None again: no graph)."""
        if torch.is_grad_enabled():
            raise RuntimeError("beam_stream is inference only: run it under torch.no_grad()")
        B, T, _ = enc_chunk.shape
        dev = enc_chunk.device
        nv = torch.full((B,), T, dtype=torch.int32, device=dev) if n_valid is None else n_valid.to(device=dev, dtype=torch.int32)
        timed = bool(return_frames)
        if state is not None and ("frames" in state) != timed:
            raise ValueError(f"beam_stream: this stream was started with return_frames={'frames' in state}")
        if state is None and bias is None:
            bias = self.bias
        biased = bias is not None if state is None else "graphs" in state
        graphs = None
        if bias is not None and not biased:
            raise ValueError("beam_stream: this stream was started without bias")
        if biased:
            from .biasing import as_list
            self._check_bias(bias)
            named = as_list(bias, B) if bias is not None else None
            graphs = [_NO_GRAPH_YET] * B if state is None else state["graphs"]
            for b in range(B):
                if graphs[b] is _NO_GRAPH_YET:
                    graphs[b] = named[b] if named is not None else None
                elif named is not None and named[b] is not graphs[b]:
                    raise ValueError(f"beam_stream: stream {b} was started with another graph; reset_streams it before changing its graph")
        if self._device_beam_ok(enc_chunk, bias=biased):
            from . import ops
            enc = enc_chunk.contiguous()
            if state is None:
                mf = int(max_frames or BEAM_STREAM_FRAMES)
                lm_layers, lm_hidden = (self.lm.rnn.rnn.num_layers, self.lm.rnn.rnn.hidden_size) if self.lm_weight > 0 else (0, 0)
                nbytes = ops.beam_workspace_bytes(B, mf, self.decode_network_lst[1].rnn.hidden_size, enc.shape[-1],
                                                  self.classifier_network[0].w.out_features, self.beam_size, self.cap, lm_layers, lm_hidden,
                                                  timed, biased, self._beam_is_wide())
                state = {"dev": torch.zeros(nbytes, dtype=torch.uint8, device=dev), "max_frames": mf, "B": B}
                if biased:
                    state["graphs"] = graphs
            elif "dev" not in state:
                raise ValueError("beam_stream: this state was made by the host route")
            out = self._device_beam_call(enc, ops.beam_search_stream, state["dev"], nv, state["max_frames"],
                                         **self._beam_kw(timed, graphs, dev))
            nbest_batch, nbest_scores, status = out[:3]
            nbest_frames = out[3] if timed else None
            bad = [b for b in range(B) if int(status[b]) != 0]
            state["stopped"] = {b: ops.BEAM_STATUS[int(status[b])] for b in bad}
            if bad and raise_stopped:
                raise RuntimeError(f"beam_stream: stream(s) {bad} stopped ({sorted({ops.BEAM_STATUS[int(status[b])] for b in bad})}) with "
                                   f"cap={self.cap} hypotheses per frame and max_frames={state['max_frames']}; restart the stream with a "
                                   f"larger cap (TransducerBeamSearcher(cap=...)) or max_frames")
            for b in range(B):       # a stream that has not decoded a frame yet (a zeroed state and no valid frame) has no beam to list
                if not nbest_batch[b]:
                    nbest_batch[b], nbest_scores[b] = [[]], [0.0]
                    if timed:
                        nbest_frames[b] = [[]]
            state["nbest"], state["scores"] = nbest_batch, nbest_scores
            if timed:
                state["frames"] = nbest_frames
            return [n[0] for n in nbest_batch], state
        if state is None:
            state = {"beams": [[self._beam_start(timed, biased)] for _ in range(B)]}
            if timed:
                state["frames_done"] = [0] * B
            if biased:
                state["graphs"] = graphs
        elif "beams" not in state:
            raise ValueError("beam_stream: this state was made by the device route")
        counts = nv.cpu().tolist()
        for b in range(B):
            n = min(max(int(counts[b]), 0), T)
            for t in range(n):
                state["beams"][b] = self._beam_frame(state["beams"][b], enc_chunk[b, t, :], state["frames_done"][b] + t if timed else None,
                                                     graphs[b] if biased else None, biased)
            if timed:
                state["frames_done"][b] += n
        ranked = [self._beam_rank(beam, timed, graphs[b] if biased else None, biased) for b, beam in enumerate(state["beams"])]
        state["nbest"], state["scores"] = [r[0] for r in ranked], [r[1] for r in ranked]
        if timed:
            state["frames"] = [r[2] for r in ranked]
        return [n[0] for n in state["nbest"]], state
