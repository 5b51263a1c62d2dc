"""Device greedy search for subword vocabularies (csrc/search.hip greedy_decode_kernel's WIDE instantiations through decoders.TransducerBeamSearcher) against
the float64 search of tests/helpers/joint_wide_ref.py and the reference searcher's hypotheses in tests/golden/c1_wide_vocab.npz.

Every case meets the helper's conditions (tests/test_joint_wide_ref_cpu.py: float64 top-2 logit margin >= 1e-4 at every decision, in fp32
and on the bf16-rounded weights), so the hypotheses are compared exactly; every utterance's logp_sum to 1e-4 absolute."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import joint_wide_ref as JW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
dec = importlib.import_module("ts-asr_amd.decoders")
nnet = importlib.import_module("ts-asr_amd.nnet")
rnnt = importlib.import_module("ts-asr_amd.rnnt")
DTYPES = [torch.float32, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def expected(name, dtype):
    net = JW.greedy_net(name)
    return JW.greedy(JW.greedy_net_bf16(net) if dtype == torch.bfloat16 else net)


def searcher(name, spec=None):
    V, E, H, J, _ = spec or JW.GREEDY_CASES[name]
    net = {k: torch.from_numpy(v) for k, v in JW.greedy_net(name, spec=spec).items()}
    emb = nnet.Embedding(V, consider_as_one_hot=True, blank_id=0) if E is None else nnet.Embedding(V, embedding_dim=E)
    if E is None:
        assert torch.equal(emb.Embedding.weight, net["emb"])
    else:
        emb.Embedding.load_state_dict({"weight": net["emb"]})
    lstm = nnet.LSTM(H, input_size=emb.embedding_dim)
    lstm.rnn.load_state_dict({"weight_ih_l0": net["w_ih"], "weight_hh_l0": net["w_hh"], "bias_ih_l0": net["b_ih"], "bias_hh_l0": net["b_hh"]})
    proj, head = nnet.Linear(J, input_size=H), nnet.Linear(V, input_size=J)
    proj.load_state_dict({"w.weight": net["w_proj"], "w.bias": net["b_proj"]})
    head.load_state_dict({"w.weight": net["w_head"], "w.bias": net["b_head"]})
    mods = [m.to(DEV).eval() for m in (emb, lstm, proj, head)]
    s = dec.TransducerBeamSearcher(mods[:3], rnnt.Transducer_joint(), [mods[3]], blank_id=0, beam_size=1)
    return s, net["enc"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(JW.GREEDY_CASES))
def test_device_greedy_matches_float64(golden, name, dtype):
    s, enc = searcher(name)
    enc = enc.to(DEV, dtype)
    assert s._device_greedy_ok(enc) and s._greedy_is_wide()
    assert not s._device_beam_ok(enc)                          # the beam search keeps its limits (V <= 63) and the host loop above them
    hyps, score, _, _, frames, _ = s.forward_timed(enc)
    want = expected(name, dtype)
    assert hyps == [r["tokens"] for r in want]
    assert frames == [r["frames"] for r in want]
    if dtype == torch.float32 and name in JW.FIXTURE_GREEDY:
        g = golden["c1_wide_vocab"]
        assert hyps == [list(map(int, row[:n])) for row, n in zip(g[f"greedy_{name}_hyps"], g[f"greedy_{name}_lens"])]
    # logp_sum of every utterance: the searcher only returns mean(exp(logp_sum)), so the one-call entry point is called for the sums themselves
    C = importlib.import_module("ts-asr_amd._capi")
    B, T, J = enc.shape
    table, mats, b_ih, b_hh, b_proj, b_head, wdt = s._device_greedy_args(enc)
    preds = torch.empty(B, T, dtype=torch.int32, device=DEV)
    logp = torch.empty(B, dtype=torch.float32, device=DEV)
    C.check(C.lib().tsasr_greedy_decode(C.ptr(enc), C.ptr(table), C.ptr(mats[0]), C.ptr(mats[1]), C.ptr(b_ih), C.ptr(b_hh), C.ptr(mats[2]),
                                        C.ptr(b_proj), C.ptr(mats[3]), C.ptr(b_head), None, None, C.ptr(preds), C.ptr(logp), B, T, J,
                                        mats[1].shape[1], table.shape[1], mats[3].shape[0], 0, 0.01, C.io_dtype(enc), wdt, C.stream_ptr(), 1),
            "tsasr_greedy_decode (wide)")
    sums = logp.cpu().numpy().astype(np.float64)
    assert float(score) == float(logp.exp().mean())
    for b in range(B):
        print(f"{name} {dtype} b={b}: logp_sum {sums[b]:.6f} helper {want[b]['logp_sum']:.6f} diff {abs(sums[b] - want[b]['logp_sum']):.2e}")
    for b in range(B):
        assert abs(sums[b] - want[b]["logp_sum"]) <= 1e-4, (b, sums[b], want[b]["logp_sum"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(JW.GREEDY_CASES))
def test_stream_form_gives_the_one_call_bits(name, dtype):
    """Chunks of 16 frames with ragged n_valid: the tokens, frames, log-probability sums and final predictor state of one call."""
    from importlib import import_module
    ops = import_module("ts-asr_amd.ops")
    s, enc = searcher(name)
    enc = enc.to(DEV, dtype)
    B, T, J = enc.shape
    want = expected(name, dtype)
    with torch.no_grad():
        whole, wf, st_whole = s.greedy_stream(enc, None, None, return_frames=True)
        lens = [T, T - 7, T - 19]                              # utterance b has lens[b] frames: the last chunks are ragged or empty
        toks, frs, state = [[] for _ in range(B)], [[] for _ in range(B)], None
        for c0 in range(0, T, 16):
            chunk = enc[:, c0:c0 + 16].contiguous()
            nv = torch.tensor([max(0, min(chunk.shape[1], n - c0)) for n in lens], dtype=torch.int32, device=DEV)
            new, nf, state = s.greedy_stream(chunk, state, nv, return_frames=True)
            for b in range(B):
                toks[b] += new[b]
                frs[b] += nf[b]
        ref_toks, ref_frs, st_ref = [], [], None
        for b in range(B):                                     # one call per utterance over exactly its frames
            t1, f1, st1 = s.greedy_stream(enc[b:b + 1, :lens[b]].contiguous(), None, None, return_frames=True)
            ref_toks.append(t1[0]); ref_frs.append(f1[0])
            assert torch.equal(st1["dev"][0], state["dev"][b]), f"final state of utterance {b}"
            assert torch.equal(st1["logp_sum"][0], state["logp_sum"][b])
    assert whole == [r["tokens"] for r in want] and wf == [r["frames"] for r in want]
    assert toks == ref_toks and frs == ref_frs
    assert toks[0] == whole[0] and frs[0] == wf[0]
    sums = st_whole["logp_sum"].cpu().numpy().astype(np.float64)
    for b in range(B):
        print(f"{name} {dtype} b={b}: logp_sum {sums[b]:.6f} helper {want[b]['logp_sum']:.6f}")
        assert abs(sums[b] - want[b]["logp_sum"]) <= 1e-4
    assert tuple(state["dev"].shape) == (B, ops.greedy_stream_state_size(JW.GREEDY_CASES[name][2], J))


def test_character_models_keep_the_narrow_kernel(monkeypatch):
    """V = 29 with the one-hot table: the searcher still calls tsasr_greedy_decode with wide = 0, and wide = 1, given the same network,
    emits the same preds - the narrow instantiation is what it was, the wide one agrees with it where both apply."""
    C = importlib.import_module("ts-asr_amd._capi")
    name, spec = JW.NARROW_CASE
    s, enc = searcher(name, spec)
    want = JW.greedy(JW.greedy_net(name, spec=spec))
    assert JW.greedy_case_ok(want)[0]
    enc = enc.to(DEV)
    assert s._device_greedy_ok(enc) and not s._greedy_is_wide()
    real, wides = C.lib().tsasr_greedy_decode, []
    monkeypatch.setattr(C.lib(), "tsasr_greedy_decode", lambda *a: (wides.append(a[-1]), real(*a))[1])
    hyps, _, _, _, frames, _ = s.forward_timed(enc)
    monkeypatch.undo()
    assert wides == [0]                                        # the searcher's own call
    assert hyps == [r["tokens"] for r in want] and frames == [r["frames"] for r in want]
    B, T, J = enc.shape
    table, mats, b_ih, b_hh, b_proj, b_head, wdt = s._device_greedy_args(enc)
    out = {}
    for wide in (0, 1):
        preds = torch.empty(B, T, dtype=torch.int32, device=DEV)
        logp = torch.empty(B, dtype=torch.float32, device=DEV)
        C.check(C.lib().tsasr_greedy_decode(C.ptr(enc), C.ptr(table), C.ptr(mats[0]), C.ptr(mats[1]), C.ptr(b_ih), C.ptr(b_hh), C.ptr(mats[2]),
                                            C.ptr(b_proj), C.ptr(mats[3]), C.ptr(b_head), None, None, C.ptr(preds), C.ptr(logp), B, T, J, 64,
                                            table.shape[1], 29, 0, 0.01, C.io_dtype(enc), wdt, C.stream_ptr(), wide), f"wide={wide}")
        out[wide] = (preds.cpu(), logp.cpu())
    assert torch.equal(out[0][0], out[1][0])
    torch.testing.assert_close(out[0][1], out[1][1], atol=1e-5, rtol=1e-5)
