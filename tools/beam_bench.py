#!/usr/bin/env python3
"""Device beam search (csrc/search.hip, tsasr_beam_search) against the host loop on a configs[1]-shaped TEST batch.

enc_proj [32, 250, 640] (seeded, the golden encoder output's scale), predictor 512 / joint 640 / 29 symbols with the deterministic golden
weights and the golden fixture's blank-bias shift (+3.0, so that the reference's loop ends); fp32 and bf16, beam 4 and 15. The device
search is timed over the whole batch (HIP events, median of --reps); the host loop (TSASR_BEAM_KERNEL=0) over --host-utts utterances and
reported per utterance. Expansions per frame and predictor steps computed come from a host restatement of the kernel's bookkeeping over
the device's own inputs (count only; the counts do not depend on which route ran).

    python tools/beam_bench.py [--reps 5] [--host-utts 2] [--frames 250]
    python tools/beam_bench.py --times [--reps 50] [--ab-lib OTHER.so]     # the timed launch (tsasr_beam_search with frames) beside the untimed one

--times: the launch alone, without the host read-back: the stream is pre-loaded, events sit around each launch, the two forms
alternate, median of --reps after warm-up (the method of profiles/align_notes.md); B = 32, T' = --frames, beam 15, bf16 and fp32.
--ab-lib: the untimed launch of another build of the library (e.g. the parent commit's) takes part in the same loop.

    python tools/beam_bench.py --lm [--reps 5] [--host-utts 1] [--lm-weight 0.3] [--ab-lib OTHER.so]

--lm: the LM-fused launch (tsasr_beam_search with lm, the reference-default RNNLM: 2 x 1024 LSTM, embedding 128, one 512 block; seeded initial
weights) beside the unfused launch in the same loop, by the method of --times; then the host loop with the same LM (TSASR_BEAM_KERNEL=0)
over --host-utts utterances, wall clock per utterance. LM steps per frame = hypothesis nodes expanded (one LM step each, as predictor steps).

    python tools/beam_bench.py --vocab 256 [--lm] [--times] [--blank-bias 3.0] [--reps 5] [--host-utts 1]

--vocab V: a subword model (beam_search_kernel's WIDE instantiations): predictor 512 / joint 640 / V symbols with the frozen one-hot table, weights seeded
like tests/helpers/joint_wide_ref.greedy_net (head scale 1.5, blank bias +3 and --blank-bias more, so that the search ends), enc_proj
[32, --frames, 640] seeded. The device search through the searcher's own call (launch and read-back of the n-best, median of --reps) beside
the host loop (TSASR_BEAM_KERNEL=0, --host-utts utterances, per utterance), beams --beams; --lm fuses the reference-default RNNLM over V
symbols into both, --times asks both for the emission frames.

    python tools/beam_bench.py --bias 16 [--lm] [--times] [--vocab 256] [--ab-lib OTHER.so] [--bias-weight 1.0] [--reps 5]

--bias N: contextual biasing (tsasr_beam_search with bias): one graph of N seeded phrases of 3-6 tokens for every utterance; the biased search
beside the unbiased one through the searcher's own call (launch and read-back of the n-best), the two forms alternating, median of --reps,
beams --beams; per-utterance time = batch time / 32. --lm fuses the reference-default RNNLM into both, --times asks both for the emission
frames, --vocab V takes the subword model; --ab-lib: the unbiased search of another build of the library takes part in the same loop.
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from oracle.golden_recipe import det_tensor  # noqa: E402


def counts(s, enc):
    """(expansions, predictor steps with memoisation, frames) of the host loop's bookkeeping on enc [1,T,J], counted as the kernel
    computes: one predictor step per hypothesis node (a blank copy keeps its node, an extension is a new node)."""
    import torch.nn.functional as F
    key = lambda h: h[1] / h[0]  # noqa: E731
    nodes = [(-1, s.blank_id)]                      # node -> (parent, token)
    beam, exp, memo = [(1, 0.0, 0)], 0, {}          # (len, logp, node)
    for t in range(enc.shape[1]):
        A, beam = beam, []
        while len(beam) < s.beam_size:
            a = max(A, key=key)
            if beam and max(beam, key=key)[1] >= s.state_beam + a[1]:
                break
            A.remove(a)
            exp += 1
            n = a[2]
            if n not in memo:
                par, tok = nodes[n]
                memo[n] = s._pn(torch.full((1, 1), tok, dtype=torch.long, device=enc.device), memo[par][1] if par >= 0 else None)
            j = s.tjoint(enc[0, t].view(1, 1, 1, -1), memo[n][0].unsqueeze(0))
            for layer in s.classifier_network:
                j = layer(j)
            logp, pos = torch.topk(F.log_softmax(j.float(), dim=-1).view(-1), k=s.beam_size)
            logp, pos = logp.tolist(), pos.tolist()
            bnb = logp[0] if pos[0] != s.blank_id else logp[1]
            for lp, sym in zip(logp, pos):
                if sym == s.blank_id:
                    beam.append((a[0], a[1] + lp, n))
                elif lp >= bnb - s.expand_beam:
                    nodes.append((n, sym))
                    A.append((a[0] + 1, a[1] + lp, len(nodes) - 1))
    return exp, len(memo), enc.shape[1]


def times_bench(args):
    """Timed against untimed launch on the TEST shape; prints one JSON line per dtype."""
    dec = importlib.import_module("ts-asr_amd.decoders")
    ops = importlib.import_module("ts-asr_amd.ops")
    capi = importlib.import_module("ts-asr_amd._capi")
    lib, P = capi.lib(), capi.ptr
    results = []
    for dtype in args.dtypes.split(","):
        brain, h = entry._config1_brain("cuda:0", dtype, joint_dim=640, decoder_neurons=512)
        brain._setup_dtype()
        m = brain.modules
        dt = torch.float32 if dtype == "fp32" else torch.bfloat16
        g = np.load(os.path.join(ROOT, "tests", "golden", "c1_chain_cat.npz"))["enc_proj"]
        B, T, beam, nbest, cap = 32, args.frames, 15, 5, dec.BEAM_CAP
        enc = torch.from_numpy(det_tensor("beam_bench.enc_proj", (B, T, 640), float(np.std(g)))).to("cuda:0", dt)
        with torch.no_grad():
            m.transducer_head.w.bias[0] += 3.0
            s = dec.TransducerBeamSearcher([m.embedding, m.decoder, m.decoder_proj], m.joiner, [m.transducer_head], blank_id=0,
                                           beam_size=beam, nbest=nbest, state_beam=2.3, expand_beam=2.3)
            table, mats, b_ih, b_hh, b_proj, b_head, wdt = s._device_greedy_args(enc)
        H, J, E, V, Lmax = mats[1].shape[1], 640, table.shape[1], mats[3].shape[0], 2 * T + 16
        ws = torch.zeros(ops.beam_workspace_bytes(B, T, H, J, V, beam, cap, times=True), dtype=torch.uint8, device="cuda:0")
        hyps, frames = (torch.empty(B, nbest, Lmax, dtype=torch.int32, device="cuda:0") for _ in range(2))
        lens = torch.empty(B, nbest, dtype=torch.int32, device="cuda:0")
        scores = torch.empty(B, nbest, dtype=torch.float64, device="cuda:0")
        status = torch.empty(B, dtype=torch.int32, device="cuda:0")
        # the offline narrow search: n_valid NULL, max_frames = T, then the frames, no LM, no graph, wide = 0
        head = (P(enc), P(table), P(mats[0]), P(mats[1]), P(b_ih), P(b_hh), P(mats[2]), P(b_proj), P(mats[3]), P(b_head), P(ws), ws.numel(),
                None, P(hyps), P(lens), P(scores), P(status), B, T, T, J, H, E, V, 0, beam, nbest, cap, Lmax, 2.3, 2.3, 0.01,
                capi.io_dtype(enc), wdt)
        launch = lambda fn, fr, what: capi.check(fn(*head, capi.stream_ptr(), P(fr), None, 0.0, None, 0), what)  # noqa: E731

        forms = {"untimed": lambda: launch(lib.tsasr_beam_search, None, "tsasr_beam_search"),
                 "timed": lambda: launch(lib.tsasr_beam_search, frames, "tsasr_beam_search (frames)")}
        if args.ab_lib:                                      # the untimed launch of another build of the library, in the same loop
            other = ctypes.CDLL(os.path.abspath(args.ab_lib)).tsasr_beam_search
            other.restype, other.argtypes = lib.tsasr_beam_search.restype, lib.tsasr_beam_search.argtypes
            forms["untimed_ab"] = lambda: launch(other, None, "tsasr_beam_search (--ab-lib)")
        names = list(forms)
        ms = {n: [] for n in names}
        fill = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0")
        for n in names * 2:                                  # warm-up
            forms[n]()
        torch.cuda.synchronize()
        for rep in range(args.reps):
            order = names[rep % len(names):] + names[:rep % len(names)]
            for n in (order if (rep // len(names)) % 2 == 0 else order[::-1]):      # no form always follows the same other one
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fill.fill_(rep % 200)                        # the stream is busy while the events and the launch are enqueued
                fill.fill_(rep % 200 + 1)
                e0.record()
                forms[n]()
                e1.record()
                torch.cuda.synchronize()
                ms[n].append(e0.elapsed_time(e1))
        with torch.no_grad():
            m.transducer_head.w.bias[0] -= 3.0
        med = {n: float(np.median(v)) for n, v in ms.items()}
        spread = lambda v: round(float(np.percentile(v, 90) - np.percentile(v, 10)), 3)  # noqa: E731
        r = dict(dtype=dtype, B=B, T=T, beam=beam, reps=args.reps, ratio=round(med["timed"] / med["untimed"], 4),
                 stopped_utts=int((status != 0).sum()))
        for n in names:
            r[n + "_ms"], r[n + "_p10_p90_ms"] = round(med[n], 3), spread(ms[n])
        print(json.dumps(r), flush=True)
        results.append(r)
    return results


def lm_bench(args):
    """Fused against unfused launch on the TEST shape, and the host loop with the same LM; prints one JSON line per dtype."""
    dec = importlib.import_module("ts-asr_amd.decoders")
    ops = importlib.import_module("ts-asr_amd.ops")
    nnet = importlib.import_module("ts-asr_amd.nnet")
    capi = importlib.import_module("ts-asr_amd._capi")
    lib, P = capi.lib(), capi.ptr
    results = []
    for dtype in args.dtypes.split(","):
        brain, h = entry._config1_brain("cuda:0", dtype, joint_dim=640, decoder_neurons=512)
        brain._setup_dtype()
        m = brain.modules
        dt = torch.float32 if dtype == "fp32" else torch.bfloat16
        g = np.load(os.path.join(ROOT, "tests", "golden", "c1_chain_cat.npz"))["enc_proj"]
        B, T, beam, nbest, cap = 32, args.frames, 15, 5, dec.BEAM_CAP
        enc = torch.from_numpy(det_tensor("beam_bench.enc_proj", (B, T, 640), float(np.std(g)))).to("cuda:0", dt)
        torch.manual_seed(0)
        lm = nnet.RNNLM(29, return_hidden=True).to("cuda:0").eval()
        with torch.no_grad():
            m.transducer_head.w.bias[0] += 3.0
            s = dec.TransducerBeamSearcher([m.embedding, m.decoder, m.decoder_proj], m.joiner, [m.transducer_head], blank_id=0,
                                           beam_size=beam, nbest=nbest, lm_module=lm, lm_weight=args.lm_weight, state_beam=2.3, expand_beam=2.3)
            assert s._device_beam_ok(enc)
            table, mats, b_ih, b_hh, b_proj, b_head, wdt = s._device_greedy_args(enc)
            lm_args = s._device_lm_args(enc)
        H, J, E, V, Lmax = mats[1].shape[1], 640, table.shape[1], mats[3].shape[0], 2 * T + 16
        desc, weight, lm_layers, lm_hidden = ops._beam_lm_desc(lm_args, V, wdt)
        ws = torch.zeros(ops.beam_workspace_bytes(B, T, H, J, V, beam, cap, lm_layers, lm_hidden), dtype=torch.uint8, device="cuda:0")
        hyps = torch.empty(B, nbest, Lmax, dtype=torch.int32, device="cuda:0")
        lens = torch.empty(B, nbest, dtype=torch.int32, device="cuda:0")
        scores = torch.empty(B, nbest, dtype=torch.float64, device="cuda:0")
        status, status_lm = (torch.empty(B, dtype=torch.int32, device="cuda:0") for _ in range(2))
        wptrs = (P(table), P(mats[0]), P(mats[1]), P(b_ih), P(b_hh), P(mats[2]), P(b_proj), P(mats[3]), P(b_head), P(ws), ws.numel())
        # the offline narrow search: n_valid NULL, max_frames = T, untimed, then the LM and its weight, no graph, wide = 0
        head = (P(enc),) + wptrs + (None, P(hyps), P(lens), P(scores), P(status), B, T, T, J, H, E, V, 0, beam, nbest, cap, Lmax, 2.3, 2.3, 0.01,
                                    capi.io_dtype(enc), wdt)
        outs_lm = (P(hyps), P(lens), P(scores), P(status_lm))
        unfused = lambda fn, what: capi.check(fn(*head, capi.stream_ptr(), None, None, 0.0, None, 0), what)  # noqa: E731
        forms = {"unfused": lambda: unfused(lib.tsasr_beam_search, "tsasr_beam_search"),
                 "fused": lambda: capi.check(ops._beam_launch(enc, wptrs, None, outs_lm, B, T, T, J, H, E, V, 0, beam, nbest, cap, Lmax, 2.3, 2.3,
                                                              0.01, wdt, None, desc, weight, None, False), "tsasr_beam_search (lm)")}
        if args.ab_lib:
            other = ctypes.CDLL(os.path.abspath(args.ab_lib)).tsasr_beam_search
            other.restype, other.argtypes = lib.tsasr_beam_search.restype, lib.tsasr_beam_search.argtypes
            forms["unfused_ab"] = lambda: unfused(other, "tsasr_beam_search (--ab-lib)")
        names = list(forms)
        ms = {n: [] for n in names}
        fill = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0")
        for n in names:                                      # warm-up
            forms[n]()
        torch.cuda.synchronize()
        for rep in range(args.reps):
            order = names[rep % len(names):] + names[:rep % len(names)]
            for n in (order if (rep // len(names)) % 2 == 0 else order[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fill.fill_(rep % 200)
                fill.fill_(rep % 200 + 1)
                e0.record()
                forms[n]()
                e1.record()
                torch.cuda.synchronize()
                ms[n].append(e0.elapsed_time(e1))
        med = {n: float(np.median(v)) for n, v in ms.items()}
        spread = lambda v: round(float(np.percentile(v, 90) - np.percentile(v, 10)), 3)  # noqa: E731
        r = dict(dtype=dtype, B=B, T=T, beam=beam, reps=args.reps, lm_weight=args.lm_weight, fused_over_unfused=round(med["fused"] / med["unfused"], 2),
                 stopped_utts=int((status != 0).sum()), stopped_utts_fused=int((status_lm != 0).sum()))
        for n in names:
            r[n + "_ms"], r[n + "_p10_p90_ms"] = round(med[n], 3), spread(ms[n])
        ok = [b for b in range(B) if int(status_lm[b]) == 0][: args.host_utts]
        if ok:
            os.environ["TSASR_BEAM_KERNEL"] = "0"
            try:
                with torch.no_grad():
                    steps = [0]
                    lm_forward = lm.forward

                    def counted(*a, **k):
                        steps[0] += 1
                        return lm_forward(*a, **k)
                    lm.forward = counted
                    t0 = time.perf_counter()
                    s(enc[ok])
                    torch.cuda.synchronize()
                    r["host_lm_ms_per_utt"] = round((time.perf_counter() - t0) * 1e3 / len(ok), 1)
                    r["host_lm_steps_per_frame"] = round(steps[0] / (len(ok) * T), 2)        # one per expansion on the host route
                    lm.forward = lm_forward
                    r["nodes_per_frame"] = round(counts(s, enc[ok[:1]])[1] / T, 2)             # (the unfused search's; one LM step each when fused)
                    r["fused_speedup_batch"] = round(r["host_lm_ms_per_utt"] * B / med["fused"], 1)
            finally:
                del os.environ["TSASR_BEAM_KERNEL"]
        with torch.no_grad():
            m.transducer_head.w.bias[0] -= 3.0
        print(json.dumps(r), flush=True)
        results.append(r)
    return results


def wide_bench(args):
    """--vocab V: device search per batch beside the host loop per utterance; prints one JSON line per dtype and beam."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import joint_wide_ref as JW
    dec = importlib.import_module("ts-asr_amd.decoders")
    ops = importlib.import_module("ts-asr_amd.ops")
    nnet = importlib.import_module("ts-asr_amd.nnet")
    rnnt = importlib.import_module("ts-asr_amd.rnnt")
    V, H, J, B, T = args.vocab, 512, 640, 32, args.frames
    net = {k: torch.from_numpy(v) for k, v in JW.greedy_net(f"beam_bench.v{V}", spec=(V, None, H, J, 1.5)).items()}
    net["b_head"][0] += args.blank_bias
    emb = nnet.Embedding(V, consider_as_one_hot=True, blank_id=0)
    lstm = nnet.LSTM(H, input_size=emb.embedding_dim)
    lstm.rnn.load_state_dict({"weight_ih_l0": net["w_ih"], "weight_hh_l0": net["w_hh"], "bias_ih_l0": net["b_ih"], "bias_hh_l0": net["b_hh"]})
    proj, head = nnet.Linear(J, input_size=H), nnet.Linear(V, input_size=J)
    proj.load_state_dict({"w.weight": net["w_proj"], "w.bias": net["b_proj"]})
    head.load_state_dict({"w.weight": net["w_head"], "w.bias": net["b_head"]})
    mods = [m.to("cuda:0").eval() for m in (emb, lstm, proj, head)]
    lm = None
    if args.lm:
        torch.manual_seed(0)
        lm = nnet.RNNLM(V, return_hidden=True).to("cuda:0").eval()
    results = []
    for dtype in args.dtypes.split(","):
        nnet.set_compute_dtype(torch.float32 if dtype == "fp32" else torch.bfloat16)       # the host loop's products
        enc = torch.from_numpy(det_tensor("beam_bench.enc_proj", (B, T, J), 1.0)).to("cuda:0", torch.float32 if dtype == "fp32" else torch.bfloat16)
        for beam in (int(b) for b in args.beams.split(",")):
            s = dec.TransducerBeamSearcher(mods[:3], rnnt.Transducer_joint(), [mods[3]], blank_id=0, beam_size=beam, nbest=5, lm_module=lm,
                                           lm_weight=args.lm_weight if lm is not None else 0.0, state_beam=2.3, expand_beam=2.3)
            kw = {"frames": True} if args.times else {}
            with torch.no_grad():
                assert s._device_beam_ok(enc) and s._beam_is_wide()
                status = s._device_beam_call(enc, ops.beam_search, **kw)[2]      # warm-up (no host re-decode: timed alone)
                ms = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    s._device_beam_call(enc, ops.beam_search, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                host_ms, exp, steps, frames = float("nan"), 0, 0, 1
                ok = [b for b in range(B) if int(status[b]) == 0][: args.host_utts]
                if ok:
                    os.environ["TSASR_BEAM_KERNEL"] = "0"
                    try:
                        t0 = time.perf_counter()
                        s.forward_timed(enc[ok]) if args.times else s(enc[ok])
                        torch.cuda.synchronize()
                        host_ms = (time.perf_counter() - t0) * 1e3 / len(ok)
                        if lm is None:
                            exp, steps, frames = counts(s, enc[ok[:1]])
                    finally:
                        del os.environ["TSASR_BEAM_KERNEL"]
            dev_ms = float(np.median(ms))
            r = dict(vocab=V, lm=bool(args.lm), times=bool(args.times), dtype=dtype, beam=beam, B=B, T=T, device_ms_per_batch=round(dev_ms, 2),
                     host_ms_per_utt=round(host_ms, 1), speedup_batch=round(host_ms * B / dev_ms, 1), device_stopped_utts=int((status != 0).sum()))
            if lm is None:
                r.update(expansions_per_frame=round(exp / frames, 2), predictor_steps_per_frame=round(steps / frames, 2))
            print(json.dumps(r), flush=True)
            results.append(r)
    return results


def bias_bench(args):
    """--bias N: biased beside unbiased search, device route, per batch; prints one JSON line per dtype and beam."""
    dec = importlib.import_module("ts-asr_amd.decoders")
    ops = importlib.import_module("ts-asr_amd.ops")
    nnet = importlib.import_module("ts-asr_amd.nnet")
    capi = importlib.import_module("ts-asr_amd._capi")
    biasing = importlib.import_module("ts-asr_amd.biasing")
    B, T = 32, args.frames
    V = args.vocab or 29
    rng = np.random.default_rng(args.bias)
    graph = biasing.ContextGraph([rng.integers(1, V, size=int(rng.integers(3, 7))).tolist() for _ in range(args.bias)], args.bias_weight)
    other = None
    if args.ab_lib:                                              # the unbiased search of another build, swapped in for its calls
        other = ctypes.CDLL(os.path.abspath(args.ab_lib))
        for name, (res, argt) in capi._PROTOS.items():
            if hasattr(other, name):
                getattr(other, name).restype, getattr(other, name).argtypes = res, argt
    results = []
    for dtype in args.dtypes.split(","):
        dt = torch.float32 if dtype == "fp32" else torch.bfloat16
        if args.vocab:
            sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
            import joint_wide_ref as JW
            rnnt = importlib.import_module("ts-asr_amd.rnnt")
            H, J = 512, 640
            net = {k: torch.from_numpy(v) for k, v in JW.greedy_net(f"beam_bench.v{V}", spec=(V, None, H, J, 1.5)).items()}
            net["b_head"][0] += args.blank_bias
            emb = nnet.Embedding(V, consider_as_one_hot=True, blank_id=0)
            lstm = nnet.LSTM(H, input_size=emb.embedding_dim)
            lstm.rnn.load_state_dict({"weight_ih_l0": net["w_ih"], "weight_hh_l0": net["w_hh"], "bias_ih_l0": net["b_ih"], "bias_hh_l0": net["b_hh"]})
            proj, head = nnet.Linear(J, input_size=H), nnet.Linear(V, input_size=J)
            proj.load_state_dict({"w.weight": net["w_proj"], "w.bias": net["b_proj"]})
            head.load_state_dict({"w.weight": net["w_head"], "w.bias": net["b_head"]})
            mods = [m.to("cuda:0").eval() for m in (emb, lstm, proj, head)]
            nets, joint = (mods[:3], [mods[3]]), rnnt.Transducer_joint()
            nnet.set_compute_dtype(dt)
            enc = torch.from_numpy(det_tensor("beam_bench.enc_proj", (B, T, J), 1.0)).to("cuda:0", dt)
        else:
            brain, h = entry._config1_brain("cuda:0", dtype, joint_dim=640, decoder_neurons=512)
            brain._setup_dtype()
            m = brain.modules
            g = np.load(os.path.join(ROOT, "tests", "golden", "c1_chain_cat.npz"))["enc_proj"]
            enc = torch.from_numpy(det_tensor("beam_bench.enc_proj", (B, T, 640), float(np.std(g)))).to("cuda:0", dt)
            with torch.no_grad():
                m.transducer_head.w.bias[0] += 3.0
            nets, joint = ([m.embedding, m.decoder, m.decoder_proj], [m.transducer_head]), m.joiner
        lm = None
        if args.lm:
            torch.manual_seed(0)
            lm = nnet.RNNLM(V, return_hidden=True).to("cuda:0").eval()
        for beam in (int(b) for b in args.beams.split(",")):
            s = dec.TransducerBeamSearcher(nets[0], joint, nets[1], blank_id=0, beam_size=beam, nbest=5, lm_module=lm,
                                           lm_weight=args.lm_weight if lm is not None else 0.0, state_beam=2.3, expand_beam=2.3)
            kw = {"frames": True} if args.times else {}
            with torch.no_grad():
                assert s._device_beam_ok(enc, bias=True)
                packed = biasing.pack([graph] * B, enc.device)
                status = {}

                def unbiased_ab():
                    mine, capi._lib = capi._lib, other
                    try:
                        return s._device_beam_call(enc, ops.beam_search, **kw)
                    finally:
                        capi._lib = mine
                forms = {"unbiased": lambda: s._device_beam_call(enc, ops.beam_search, **kw),
                         "biased": lambda: s._device_beam_call(enc, ops.beam_search, bias=packed, **kw)}
                if other is not None:
                    forms["unbiased_ab"] = unbiased_ab
                names = list(forms)
                ms = {n: [] for n in names}
                for n in names:                                  # warm-up
                    status[n] = forms[n]()[2]
                torch.cuda.synchronize()
                for rep in range(args.reps):
                    order = names[rep % len(names):] + names[:rep % len(names)]
                    for n in (order if (rep // len(names)) % 2 == 0 else order[::-1]):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        forms[n]()
                        e1.record()
                        torch.cuda.synchronize()
                        ms[n].append(e0.elapsed_time(e1))
            med = {n: float(np.median(v)) for n, v in ms.items()}
            r = dict(bias=args.bias, bias_weight=args.bias_weight, states=graph.num_states, vocab=V, lm=bool(args.lm), times=bool(args.times),
                     dtype=dtype, beam=beam, B=B, T=T, reps=args.reps, biased_over_unbiased=round(med["biased"] / med["unbiased"], 4),
                     biased_ms_per_utt=round(med["biased"] / B, 3), unbiased_ms_per_utt=round(med["unbiased"] / B, 3))
            for n in names:
                r[n + "_ms"], r[n + "_min_max_ms"] = round(med[n], 3), [round(min(ms[n]), 3), round(max(ms[n]), 3)]
                r[n + "_stopped_utts"] = int((status[n] != 0).sum())
            print(json.dumps(r), flush=True)
            results.append(r)
        if not args.vocab:
            with torch.no_grad():
                m.transducer_head.w.bias[0] -= 3.0
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=2)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--beams", default="4,15")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--times", action="store_true", help="time the timed launch beside the untimed one (launch only)")
    ap.add_argument("--ab-lib", default=None, help="--times: also time tsasr_beam_search of this other build of the library")
    ap.add_argument("--lm", action="store_true", help="time the LM-fused launch beside the unfused one, and the host loop with the same LM")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--vocab", type=int, default=0, help="a subword model of this many symbols (the wide search), with --lm / --times")
    ap.add_argument("--blank-bias", type=float, default=3.0, help="--vocab: added to the head's blank bias beside the seeded net's +3")
    ap.add_argument("--bias", type=int, default=0, help="time the biased search (this many seeded phrases) beside the unbiased one")
    ap.add_argument("--bias-weight", type=float, default=1.0)
    args = ap.parse_args()
    if args.bias:
        return bias_bench(args)
    if args.vocab:
        return wide_bench(args)
    if args.times:
        return times_bench(args)
    if args.lm:
        return lm_bench(args)
    dec = importlib.import_module("ts-asr_amd.decoders")
    ops = importlib.import_module("ts-asr_amd.ops")
    results = []
    for dtype in args.dtypes.split(","):
        brain, h = entry._config1_brain("cuda:0", dtype, joint_dim=640, decoder_neurons=512)
        brain._setup_dtype()
        m = brain.modules
        dt = torch.float32 if dtype == "fp32" else torch.bfloat16
        g = np.load(os.path.join(ROOT, "tests", "golden", "c1_chain_cat.npz"))["enc_proj"]
        enc = torch.from_numpy(det_tensor("beam_bench.enc_proj", (32, args.frames, 640), float(np.std(g)))).to("cuda:0", dt)
        with torch.no_grad():
            m.transducer_head.w.bias[0] += 3.0
        for beam in (int(b) for b in args.beams.split(",")):
            s = dec.TransducerBeamSearcher([m.embedding, m.decoder, m.decoder_proj], m.joiner, [m.transducer_head], blank_id=0,
                                           beam_size=beam, nbest=5, state_beam=2.3, expand_beam=2.3)
            with torch.no_grad():
                assert s._device_beam_ok(enc)
                _, _, status = s._device_beam_call(enc, ops.beam_search)          # warm-up (no host re-decode: timed alone)
                ms = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    s._device_beam_call(enc, ops.beam_search)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                stopped = int((status != 0).sum())
                host_ms, exp, steps, frames = float("nan"), 0, 0, 1
                ok = [b for b in range(32) if int(status[b]) == 0][: args.host_utts]
                if ok:                                               # (an utterance past cap would keep the host loop busy for long)
                    os.environ["TSASR_BEAM_KERNEL"] = "0"
                    try:
                        t0 = time.perf_counter()
                        s(enc[ok])
                        torch.cuda.synchronize()
                        host_ms = (time.perf_counter() - t0) * 1e3 / len(ok)
                        exp, steps, frames = counts(s, enc[ok[:1]])
                    finally:
                        del os.environ["TSASR_BEAM_KERNEL"]
            dev_ms = float(np.median(ms))
            r = dict(dtype=dtype, beam=beam, B=32, T=args.frames, device_ms_per_batch=round(dev_ms, 2), host_ms_per_utt=round(host_ms, 1),
                     speedup_batch=round(host_ms * 32 / dev_ms, 1), expansions_per_frame=round(exp / frames, 2),
                     predictor_steps_per_frame=round(steps / frames, 2), device_stopped_utts=stopped)
            print(json.dumps(r), flush=True)
            results.append(r)
        with torch.no_grad():
            m.transducer_head.w.bias[0] -= 3.0
    return results


if __name__ == "__main__":
    main()
