"""Device beam search for subword vocabularies (csrc/search.hip beam_search_kernel's WIDE instantiations through decoders.TransducerBeamSearcher) against
the float64 search of tests/helpers/beam_wide_ref.py and the reference searcher's hypotheses in tests/golden/c1_beam_wide.npz.

Every case meets the helper's beam_case_ok (tests/test_beam_wide_ref_cpu.py: every comparison of the float64 search, in fp32 and on the
bf16-rounded weights, is at least 1e-4 from a tie), so n-best token lists are compared exactly; normalised scores to 1e-4 absolute, the
wide greedy search's bound on a sum of log-probabilities."""
import functools
import importlib
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import beam_wide_ref as BW  # noqa: E402
import joint_wide_ref as JW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
dec = importlib.import_module("ts-asr_amd.decoders")
ops = importlib.import_module("ts-asr_amd.ops")
nnet = importlib.import_module("ts-asr_amd.nnet")
rnnt = importlib.import_module("ts-asr_amd.rnnt")
capi = importlib.import_module("ts-asr_amd._capi")
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
RUNS = [(name, beam) for name, c in BW.CASES.items() for beam in c["runs"]]
SCORE_TOL = 1e-4


def bits(scores):
    return [np.array(x, np.float64).tobytes() for x in scores]


@functools.lru_cache(maxsize=None)
def modules(name, beam, run=None):
    """The predictor, projection and head of a case on the device (fp32 masters; a bf16 run reads their bf16 shadows) and its enc."""
    V, E, H, J, _ = JW.GREEDY_CASES[BW.CASES[name]["net"]]
    net = {k: torch.from_numpy(v) for k, v in BW.case_net(name, beam, False, run).items()}
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
    return [m.to(DEV).eval() for m in (emb, lstm, proj, head)], net["enc"]


@functools.lru_cache(maxsize=None)
def lm_module(lm_case):
    c = BW.LM_CASES[lm_case]
    cfg = BW.BL.LM_CONFIGS[c["lm"]]
    V = JW.GREEDY_CASES[BW.CASES[c["case"]]["net"]][0]
    lm = nnet.RNNLM(V, embedding_dim=cfg["emb"], dropout=0.0, rnn_layers=cfg["layers"], rnn_neurons=cfg["hidden"], return_hidden=True,
                    dnn_blocks=cfg["blocks"], dnn_neurons=cfg["dnn"])
    lm.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in BW.lm_weights(lm_case).items()}, strict=True)
    return lm.to(DEV).eval()


def searcher(name, beam, lm_case=None, nbest=BW.NBEST, cap=dec.BEAM_CAP, run=None, beam_size=None):
    run = BW.LM_CASES[lm_case]["run"] if lm_case else run
    mods, enc = modules(name, beam, run)
    s = dec.TransducerBeamSearcher(mods[:3], rnnt.Transducer_joint(), [mods[3]], blank_id=0, beam_size=beam_size or beam, nbest=nbest,
                                   lm_module=lm_module(lm_case) if lm_case else None,
                                   lm_weight=BW.LM_CASES[lm_case]["weight"] if lm_case else 0.0, state_beam=2.3, expand_beam=2.3, cap=cap)
    return s, enc


@pytest.fixture
def fp32_host():
    """The host loop runs the nnet modules: exact fp32 products for the test, the process's compute dtype put back after it."""
    prev = nnet.compute_dtype()
    nnet.set_compute_dtype(torch.float32)
    yield
    nnet.set_compute_dtype(prev)


def check_against_helper(tag, nb, sc, want, rows=None):
    """Exact n-best lists, scores within SCORE_TOL; prints and returns the worst score difference."""
    worst = 0.0
    for b in (range(len(want)) if rows is None else rows):
        assert nb[b] == want[b]["nbest"], (tag, b, nb[b], want[b]["nbest"])
        worst = max([worst] + [abs(x - y) for x, y in zip(sc[b], want[b]["scores"])])
    print(f"{tag}: worst |score - float64| {worst:.2e}")
    assert worst <= SCORE_TOL, (tag, worst)
    return worst


# ---- 1: device against the float64 helper (and the reference's fixture) ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,beam", RUNS)
def test_device_matches_float64(golden, name, beam, dtype):
    s, enc = searcher(name, beam)
    enc = enc.to(DEV, dtype)
    assert s._device_beam_ok(enc) and s._beam_is_wide()
    before = dec.BEAM_HOST_REDECODES["utterances"]
    best, _, nb, sc = s(enc)
    assert dec.BEAM_HOST_REDECODES["utterances"] == before
    want = BW.run_case(name, beam, dtype == torch.bfloat16)
    check_against_helper(f"{name} beam {beam} {dtype}", nb, sc, want)
    assert best == [r["nbest"][0] for r in want]
    if dtype == torch.float32 and name in BW.FIXTURE_CASES and beam == 4:
        g = golden["c1_beam_wide"]
        for b in range(len(nb)):
            lens = g[f"{name}_lens"][b]
            assert nb[b] == [g[f"{name}_hyps"][b, k, : int(lens[k])].tolist() for k in range(BW.NBEST) if lens[k] >= 0], (name, b)
            np.testing.assert_allclose(sc[b], g[f"{name}_scores"][b, : len(nb[b])], rtol=0, atol=SCORE_TOL)


# ---- 2: timed form ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,beam", RUNS)
def test_timed_form_same_bits_and_the_helpers_frames(name, beam, dtype):
    s, enc = searcher(name, beam)
    enc = enc.to(DEV, dtype)
    _, _, nb, sc = s(enc)
    best_t, _, nb_t, sc_t, fr_best, fr = s.forward_timed(enc)
    assert nb_t == nb and bits(sc_t) == bits(sc)
    want = BW.run_case(name, beam, dtype == torch.bfloat16)
    assert fr == [r["frames"] for r in want]
    assert fr_best == [r["frames"][0] for r in want] and best_t == [r["nbest"][0] for r in want]


# ---- 3: streams ---------------------------------------------------------------------------------------------------------------------------
def _beam_region(state, B, beam):
    """Per utterance the header words (primed, status, beam entries, tree size, frames) and the bytes of the live beam entries of its
    workspace block (an entry past the count keeps whatever an earlier call with a larger beam left there)."""
    per = state["dev"].numel() // B
    blocks = state["dev"].view(B, per)[:, : 64 + 24 * beam].cpu()
    out = []
    for blk in blocks:
        hdr = blk[:20].view(torch.int32).tolist()
        assert 1 <= hdr[2] <= beam
        out.append((hdr, blk[64: 64 + 24 * hdr[2]].tolist()))
    return out


def _stream(s, enc, lens, chunk, timed=True):
    B, T, _ = enc.shape
    state = None
    for c0 in list(range(0, T, chunk)) + [T]:                   # the call at T: an empty last chunk for every stream
        piece = enc[:, c0:c0 + chunk].contiguous() if c0 < T else enc[:, :1].contiguous()
        nv = torch.tensor([max(0, min(piece.shape[1], n - c0)) for n in lens], dtype=torch.int32, device=DEV)
        _, state = s.beam_stream(piece, state, nv, max_frames=T, return_frames=timed)
    return state


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["v100", "v100_e128"])
def test_stream_pieces_give_the_one_call_bits(name, dtype):
    """Chunks of 1, 7 and 16 frames, ragged n_valid, an empty last chunk: tokens, frames, score bits and the workspace's header and beam
    entries of one call over each stream's frames."""
    s, enc = searcher(name, 4)
    enc = enc.to(DEV, dtype)
    B, T, _ = enc.shape
    lens = [T, T - 7, 5]
    with torch.no_grad():
        whole = s.forward_timed(enc)
        one = _stream(s, enc, lens, T)
        ref = [s.forward_timed(enc[b:b + 1, : lens[b]].contiguous()) for b in range(B)]
        for b in range(B):
            assert one["nbest"][b] == ref[b][2][0] and one["frames"][b] == ref[b][5][0] and bits([one["scores"][b]]) == bits([ref[b][3][0]])
        assert one["nbest"][0] == whole[2][0] and one["frames"][0] == whole[5][0]
        for chunk in (1, 7, 16):
            st = _stream(s, enc, lens, chunk)
            assert st["nbest"] == one["nbest"] and st["frames"] == one["frames"], chunk
            assert bits(st["scores"]) == bits(one["scores"]), chunk
            assert _beam_region(st, B, 4) == _beam_region(one, B, 4), chunk
    want = BW.run_case(name, 4, dtype == torch.bfloat16)
    assert one["nbest"][0] == want[0]["nbest"] and one["frames"][0] == want[0]["frames"]


# ---- 4: LM fusion -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lm_case", list(BW.LM_CASES))
def test_lm_fusion_matches_float64(lm_case, dtype):
    c = BW.LM_CASES[lm_case]
    s, enc = searcher(c["case"], c["beam"], lm_case)
    plain, _ = searcher(c["case"], c["beam"], run=c["run"])
    enc = enc.to(DEV, dtype)
    assert s._device_beam_ok(enc) and s._beam_is_wide() and s.lm_weight > 0
    before = dec.BEAM_HOST_REDECODES["utterances"]
    with torch.no_grad():
        _, _, nb, sc, _, fr = s.forward_timed(enc)
        untimed = s(enc)
        unfused = plain(enc)[2]
        st = _stream(s, enc, [enc.shape[1]] * enc.shape[0], 7)
    assert dec.BEAM_HOST_REDECODES["utterances"] == before
    want = BW.run_case(c["case"], c["beam"], dtype == torch.bfloat16, lm_case)
    check_against_helper(f"{lm_case} {dtype}", nb, sc, want)
    assert fr == [r["frames"] for r in want]
    assert untimed[2] == nb and bits(untimed[3]) == bits(sc)
    assert st["nbest"] == nb and st["frames"] == fr and bits(st["scores"]) == bits(sc)
    assert any(a != b for a, b in zip(nb, unfused))


# ---- 5: device against the host loop ------------------------------------------------------------------------------------------------------
def test_device_equals_host_loop(monkeypatch, fp32_host):
    s, enc = searcher("v64", 4)
    enc = enc.to(DEV)
    _, _, nb, sc = s(enc)
    monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
    assert not s._device_beam_ok(enc)
    _, _, nb_h, sc_h = s(enc)
    assert nb == nb_h
    for a, b in zip(sc, sc_h):
        np.testing.assert_allclose(a, b, rtol=0, atol=SCORE_TOL)


# ---- 6: determinism -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v100", "v1024_big"])
def test_two_launches_give_the_same_bits(name):
    s, enc = searcher(name, 4)
    enc = enc.to(DEV, torch.bfloat16)
    a, b = s.forward_timed(enc), s.forward_timed(enc)
    assert a[2] == b[2] and a[5] == b[5] and bits(a[3]) == bits(b[3])


# ---- 7: overflow --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [16, 48])
def test_overflow_is_a_status_and_a_host_redecode(fp32_host, cap):
    """v64, beam 8, cap 16 and 48 (the float64 search's peaks are 45, 57 and 64: every utterance is past 16, the first fits 48): the
    utterances whose float64 search holds more than cap hypotheses in a frame stop with a status, the others are unaffected; the offline
    searcher re-decodes them on the host and counts them; a stream raises."""
    want = BW.run_case("v64", 8)
    over = [r["peak"] > cap for r in want]
    assert any(over) and (cap == 16 or not all(over))
    s, enc = searcher("v64", 8, cap=cap)
    enc = enc.to(DEV)
    assert s._device_beam_ok(enc) and s._beam_is_wide()
    with torch.no_grad():
        nb, sc, status = s._device_beam_call(enc.contiguous(), ops.beam_search)
        assert [int(x) != 0 for x in status] == over, (status, [r["peak"] for r in want])
        fine = [b for b in range(len(want)) if not over[b]]
        check_against_helper(f"v64 beam 8 cap {cap}", nb, sc, want, fine)
        before = dec.BEAM_HOST_REDECODES["utterances"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            _, _, nb_all, sc_all = s(enc)
        assert dec.BEAM_HOST_REDECODES["utterances"] == before + sum(over)
        check_against_helper(f"v64 beam 8 cap {cap}, re-decoded", nb_all, sc_all, want)
        with pytest.raises(RuntimeError, match="cap"):
            s.beam_stream(enc, None, None, max_frames=enc.shape[1])


# ---- 8: gates -----------------------------------------------------------------------------------------------------------------------------
def test_gates(monkeypatch):
    s65, enc = searcher("v100", 4, beam_size=65, nbest=3)
    enc = enc.to(DEV)
    assert s65._beam_is_wide() and not s65._device_beam_ok(enc)              # beam_size <= 64 on the wide route: the host loop
    s64, _ = searcher("v100", 4, beam_size=64)
    assert s64._device_beam_ok(enc)
    s1, _ = searcher("v100", 4, beam_size=1)
    assert not s1._device_beam_ok(enc)
    big, _ = searcher("v100", 4, cap=4000)                                   # a cap whose A arrays do not fit the LDS: the host loop
    assert not big._device_beam_ok(enc)
    table, mats, b_ih, b_hh, b_proj, b_head, wdt = big._device_greedy_args(enc)
    with torch.no_grad(), pytest.raises(capi.TsasrHipError, match="LDS"):    # and the entry point says so (no launch)
        ops.beam_search(enc, table, mats, b_ih, b_hh, b_proj, b_head, 0, 0.01, wdt, 4, 3, 2.3, 2.3, 4000, wide=True)
    with torch.no_grad(), pytest.raises(ValueError, match="E <= 64"):             # without the flag the wrapper keeps the narrow limits
        ops.beam_search(enc, table, mats, b_ih, b_hh, b_proj, b_head, 0, 0.01, wdt, 4, 3, 2.3, 2.3, 512)
    # a character model (V = 29, one-hot E = 28) still takes the narrow search: every launch has wide off and no LM
    name, spec = JW.NARROW_CASE
    V, _, H, J, _ = spec
    net = {k: torch.from_numpy(v) for k, v in JW.greedy_net(name, spec=spec).items()}
    emb = nnet.Embedding(V, consider_as_one_hot=True, blank_id=0)
    lstm = nnet.LSTM(H, input_size=emb.embedding_dim)
    lstm.rnn.load_state_dict({"weight_ih_l0": net["w_ih"], "weight_hh_l0": net["w_hh"], "bias_ih_l0": net["b_ih"], "bias_hh_l0": net["b_hh"]})
    proj, head = nnet.Linear(J, input_size=H), nnet.Linear(V, input_size=J)
    proj.load_state_dict({"w.weight": net["w_proj"], "w.bias": net["b_proj"]})
    net["b_head"][0] += 10.0                                                 # nearly every decision blank: the search ends at once
    head.load_state_dict({"w.weight": net["w_head"], "w.bias": net["b_head"]})
    mods = [m.to(DEV).eval() for m in (emb, lstm, proj, head)]
    narrow = dec.TransducerBeamSearcher(mods[:3], rnnt.Transducer_joint(), [mods[3]], blank_id=0, beam_size=4, nbest=3)
    enc29 = net["enc"][:, :4].contiguous().to(DEV)
    assert narrow._device_beam_ok(enc29) and not narrow._beam_is_wide()

    real, launches = ops._beam_launch, []

    def spy(*a):                                                             # (..., fr, lm_desc, lm_weight, bias_desc, wide)
        assert a[-4] is None and not a[-1], "a character model reached the LM / wide search"
        launches.append(a[-1])
        return real(*a)
    monkeypatch.setattr(ops, "_beam_launch", spy)
    before = dec.BEAM_HOST_REDECODES["utterances"]
    _, _, nb, _ = narrow(enc29)
    assert launches and len(nb) == enc29.shape[0] and dec.BEAM_HOST_REDECODES["utterances"] == before


# ---- 9: workspace -------------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_and_guard_region():
    fn = lambda *a: capi.lib().tsasr_beam_search_workspace_bytes(*a, 0, 1)   # noqa: E731  (no graph, wide)
    a16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for B, T, H, J, V, beam, cap, Ll, Hl, times in ((3, 24, 64, 64, 100, 4, 512, 0, 0, 0), (2, 12, 512, 640, 1022, 15, 77, 2, 1024, 1)):
        nodes = 1 + (T + 1) * beam + cap
        lmw = (V + 3) // 4 * 4 + 2 * Ll * Hl if Ll else 0
        want = B * (a16(64 + 24 * beam) + a16(8 * nodes) + 4 * (cap + beam) * (J + 2 * H + lmw) + (a16(4 * nodes) if times else 0))
        assert fn(B, T, H, J, V, beam, cap, Ll, Hl, times) == want == ops.beam_workspace_bytes(B, T, H, J, V, beam, cap, Ll, Hl, bool(times), wide=True)
    assert fn(0, 24, 64, 64, 100, 4, 512, 0, 0, 0) == 0
    s, enc = searcher("v1024_big", 4)
    enc = enc.to(DEV)
    B, T, J = enc.shape
    need = ops.beam_workspace_bytes(B, T, 512, J, 1024, 4, s.cap, times=True, wide=True)
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        nb, sc, status, fr = s._device_beam_call(enc.contiguous(), ops.beam_search, workspace=buf[:need], frames=True)
    assert [int(x) for x in status] == [0] * B
    assert bool((buf[need:] == 0xA5).all()), "the search wrote past its workspace"
    want = BW.run_case("v1024_big", 4)
    assert nb == [r["nbest"] for r in want] and fr == [r["frames"] for r in want]


# ---- 10: a character model through the wide entry point ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _narrow_searcher(with_lm):
    """JW.NARROW_CASE (V = 29, one-hot E = 28, H = J = 64) at B = 3, T = 24, beam 4, nbest 3; blank bias +2 (the float64 search then ends
    every frame below 32 hypotheses and emits 16 to 30 tokens per utterance, with and without the LM); ``with_lm``: BL's l1b0 over V = 29."""
    name, spec = JW.NARROW_CASE
    V, _, H, J, _ = spec
    net = {k: torch.from_numpy(v.copy()) for k, v in JW.greedy_net(name, spec=spec).items()}
    net["b_head"][0] += 2.0
    emb = nnet.Embedding(V, consider_as_one_hot=True, blank_id=0)
    lstm = nnet.LSTM(H, input_size=emb.embedding_dim)
    lstm.rnn.load_state_dict({"weight_ih_l0": net["w_ih"], "weight_hh_l0": net["w_hh"], "bias_ih_l0": net["b_ih"], "bias_hh_l0": net["b_hh"]})
    proj, head = nnet.Linear(J, input_size=H), nnet.Linear(V, input_size=J)
    proj.load_state_dict({"w.weight": net["w_proj"], "w.bias": net["b_proj"]})
    head.load_state_dict({"w.weight": net["w_head"], "w.bias": net["b_head"]})
    mods = [m.to(DEV).eval() for m in (emb, lstm, proj, head)]
    lm = None
    if with_lm:
        cfg = BW.BL.LM_CONFIGS["l1b0"]
        lm = nnet.RNNLM(V, embedding_dim=cfg["emb"], dropout=0.0, rnn_layers=cfg["layers"], rnn_neurons=cfg["hidden"], return_hidden=True,
                        dnn_blocks=cfg["blocks"], dnn_neurons=cfg["dnn"])
        lm.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in BW.BL.lm_weights("l1b0", V=V).items()}, strict=True)
        lm = lm.to(DEV).eval()
    s = dec.TransducerBeamSearcher(mods[:3], rnnt.Transducer_joint(), [mods[3]], blank_id=0, beam_size=4, nbest=3, lm_module=lm,
                                   lm_weight=cfg["weight"] if with_lm else 0.0, state_beam=2.3, expand_beam=2.3)
    return s, net["enc"][:3, :24].contiguous()


@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "l1b0"])
@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_character_model_same_bits_through_the_wide_entry_point(dtype, timed, with_lm):
    """WIDE switches widths, the embedding's route, the log-softmax / top-k and who appends; at V = 29, E = 28 none of them changes a
    bit: wave 0 holds the whole vocabulary (the other waves add a maximum of -inf and a sum of +0), both top-k orders are (value
    descending, index ascending), and E <= 64 takes the side operand. So tsasr_beam_search with wide = 1 gives the hypotheses of wide = 0,
    lengths, status, fp64 scores and frames."""
    s, enc = _narrow_searcher(with_lm)
    enc = enc.to(DEV, dtype)
    assert s._device_beam_ok(enc) and not s._beam_is_wide()
    with torch.no_grad():
        narrow = s._device_beam_call(enc, ops.beam_search, frames=timed)
        wide = s._device_beam_call(enc, ops.beam_search, frames=timed, wide=True)
    assert [int(x) for x in narrow[2]] == [0] * enc.shape[0] == [int(x) for x in wide[2]]
    assert all(1 <= len(h) <= 3 and len(h[0]) > 0 for h in narrow[0])
    assert wide[0] == narrow[0]                                              # token lists: hyps and lens
    assert bits(wide[1]) == bits(narrow[1])
    if timed:
        assert wide[3] == narrow[3]
