"""Forced alignment on the RNN-T lattice (csrc/rnnt.hip rnnt_viterbi_kernel through tsasr_rnnt_align) against the float64 reference
of tests/helpers/align_ref.py: valid paths, scores, optimality, planted paths recovered exactly, the tie rule, the Python and recipe
entry points, graph capture."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import rnnt_ref as RR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import align_ref as AR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [
    # B, T, U1, V, tlen, ulen      (the loss tests' lattices: the smallest that cross each code path)
    (4, 50, 21, 29, [50, 45, 40, 35], [20, 18, 15, 10]),
    (3, 6, 5, 7, [6, 4, 1], [4, 2, 0]),          # ragged incl. T=1 and empty target
    (2, 9, 65, 11, [9, 3], [64, 63]),            # 2 columns per lane, lattice wider than it is long
    (2, 40, 130, 29, [40, 17], [129, 100]),      # 4 columns per lane
    (1, 300, 300, 29, [300], [299]),             # 4 waves, skewed planes
    (2, 33, 600, 6, [33, 20], [599, 1]),         # 8 waves
    (1, 400, 1921, 29, [400], [1920]),           # the long-form width: 8 waves x 4 columns per thread
]
IDS = [f"B{c[0]}-T{c[1]}-U{c[2]}" for c in CASES]
BOOST = [10.0] * len(CASES)      # (the T=400, U1=1921 case holds its precondition at 10 as well: smallest on-path gap 4.5)
KAT_LOGITS = [[[[0.1, 0.6, 0.1, 0.1, 0.1], [0.1, 0.1, 0.6, 0.1, 0.1], [0.1, 0.1, 0.2, 0.8, 0.1]],
               [[0.1, 0.6, 0.1, 0.1, 0.1], [0.1, 0.1, 0.2, 0.1, 0.1], [0.7, 0.1, 0.2, 0.1, 0.1]]]]


@pytest.fixture(scope="module")
def rn():
    return importlib.import_module("ts-asr_amd.rnnt")


def tol(ref):
    """The project's budget for a (T+U)-term fp32 lattice sum (tests/test_rnnt_gpu.py: rtol 2e-5, atol 1e-4)."""
    return 1e-4 + 2e-5 * abs(ref)


def dev_i32(x):
    return torch.tensor(np.asarray(x), device=DEV, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def random_case(i):
    """Inputs of case i and their float64 references, computed once: (lg, tg, [lp_b], [(frames_b, optimum_b)], costs)."""
    B, T, U1, V, tlen, ulen = CASES[i]
    rng = np.random.default_rng(B * 1000 + T)
    lg = (rng.standard_normal((B, T, U1, V)) * 2).astype(np.float32)
    tg = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32) if U1 > 1 else np.zeros((B, 1), np.int32)
    lps = [AR.log_softmax(lg[b]) for b in range(B)]
    best = [AR.viterbi(lps[b], tg[b], tlen[b], ulen[b]) for b in range(B)]
    costs, _ = RR.rnnt_costs_grads(lg, tg, tlen, ulen, 0)
    for a in (lg, tg):
        a.setflags(write=False)
    return lg, tg, lps, best, np.asarray(costs, np.float64)


@functools.lru_cache(maxsize=None)
def planted_case(i):
    """Case i with a planted path per utterance (the generator continues behind the random case's draws)."""
    B, T, U1, V, tlen, ulen = CASES[i]
    rng = np.random.default_rng(B * 1000 + T)
    lg = (rng.standard_normal((B, T, U1, V)) * 2).astype(np.float32)
    tg = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32) if U1 > 1 else np.zeros((B, 1), np.int32)
    fr = AR.planted(rng, lg, tg, tlen, ulen, BOOST[i])
    lg.setflags(write=False)
    return lg, tg, fr


def run(rn, lg, tg, tlen, ulen, blank=0):
    frames, scores = rn.rnnt_align(torch.tensor(lg, device=DEV), torch.tensor(tg, device=DEV), dev_i32(tlen), dev_i32(ulen), blank)
    return frames.cpu().numpy(), scores.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_random_logits(rn, i):
    B, T, U1, V, tlen, ulen = CASES[i]
    lg, tg, lps, best, costs = random_case(i)
    frames, scores = run(rn, lg, tg, tlen, ulen)
    assert frames.shape == (B, U1 - 1) and frames.dtype == np.int32 and scores.shape == (B,)
    for b in range(B):
        Tb, Ub = tlen[b], ulen[b]
        assert np.all(frames[b, Ub:] == -1)                                        # (i) ... and path_score asserts the path is valid
        own = AR.path_score(lps[b], tg[b], frames[b], Tb, Ub)
        opt = best[b][1]
        t = tol(opt)
        print(f"case {i} b={b}: score {scores[b]:.6f} own path {own:.6f} optimum {opt:.6f} -cost {-costs[b]:.6f} tol {t:.2e}")
        assert abs(scores[b] - own) <= t                                           # (ii) the score is that of the returned path
        assert own >= opt - 2 * t                                                  # (iii) and the path is optimal
        assert scores[b] <= -costs[b] + t                                          # (iv) the best path cannot exceed the total probability


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_planted_path_is_recovered_exactly(rn, i):
    B, T, U1, V, tlen, ulen = CASES[i]
    lg, tg, planted = planted_case(i)
    for b in range(B):      # the test's own precondition, on the CPU: float64 finds the planted path, no decision on it is closer than 1.0
        fr, _, gap = AR.viterbi(AR.log_softmax(lg[b]), tg[b], tlen[b], ulen[b], return_gap=True)
        assert np.array_equal(fr, planted[b]), (i, b)
        assert gap >= 1.0, (i, b, gap)
    frames, _ = run(rn, lg, tg, tlen, ulen)
    for b in range(B):
        assert np.array_equal(frames[b, :ulen[b]], planted[b]), (i, b)
        assert np.all(frames[b, ulen[b]:] == -1)


def test_reference_known_answer_on_gpu(rn):
    """vendor/speechbrain/tests/unittests/test_losses.py:120-134, targets [1, 2]: best path frames [0, 0], log-probability -5.45381."""
    lg = torch.tensor(KAT_LOGITS, device=DEV)
    frames, scores = rn.rnnt_align(lg, dev_i32([[1, 2]]), dev_i32([2]), dev_i32([2]), 0)
    assert frames.cpu().tolist() == [[0, 0]]
    assert scores.item() == pytest.approx(-5.45381, abs=2e-4)


def test_tie_rule_blank_wins(rn):
    """Identical logits in every cell: all paths are equally probable and every label is emitted in frame 0."""
    B, T, U1, V, tlen, ulen = 2, 7, 5, 6, [7, 3], [4, 2]
    tg = np.random.default_rng(0).integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    frames, scores = run(rn, np.zeros((B, T, U1, V), np.float32), tg, tlen, ulen)
    assert frames.tolist() == [[0, 0, 0, 0], [0, 0, -1, -1]]
    np.testing.assert_allclose(scores, [-(7 + 4) * np.log(6.0), -(3 + 2) * np.log(6.0)], rtol=1e-6)


def test_transducer_align_rounds_relative_lengths(rn):
    nnet = importlib.import_module("ts-asr_amd.nnet")
    B, T, U1, V, _, _ = CASES[0]
    lg, tg, _ = planted_case(0)
    x, y = torch.tensor(lg, device=DEV), torch.tensor(tg, device=DEV)
    rel_t = torch.tensor([1.0, 0.9, 0.8, 0.7], device=DEV)           # the lengths the path was planted under
    rel_u = torch.tensor([1.0, 0.9, 0.76, 0.5], device=DEV)
    f_rel, s_rel = rn.transducer_align(x, y, rel_t, rel_u, 0)
    tl, ul = nnet.abs_lengths_round(rel_t, T), nnet.abs_lengths_round(rel_u, U1 - 1)
    assert tl.cpu().tolist() == [50, 45, 40, 35] and ul.cpu().tolist() == [20, 18, 15, 10]
    f_abs, s_abs = rn.rnnt_align(x, y, tl, ul, 0)
    assert torch.equal(f_rel, f_abs) and torch.equal(s_rel, s_abs)


def test_bf16_and_unpadded_logits(rn):
    """Non-fp32 logits and rows of V floats (ldl = V, here 29: not a multiple of 4) go through _as_padded_rows as the loss's do: the same
    bits as the fp32 call on 128-byte rows, and the planted path."""
    B, T, U1, V, tlen, ulen = CASES[0]
    lg, tg, planted = planted_case(0)
    y, tl, ul = torch.tensor(tg, device=DEV), dev_i32(tlen), dev_i32(ulen)
    x = torch.tensor(lg, device=DEV)                                   # [B,T,U1,29] contiguous: unpadded
    padded = torch.zeros(B, T, U1, 32, device=DEV)
    padded[..., :V] = x
    f_pad, s_pad = rn.rnnt_align(padded[..., :V], y, tl, ul, 0)
    f_unp, s_unp = rn.rnnt_align(x, y, tl, ul, 0)
    assert torch.equal(f_pad, f_unp) and torch.equal(s_pad, s_unp)
    xb = x.to(torch.bfloat16)
    padded[..., :V] = xb.float()
    f_b, s_b = rn.rnnt_align(xb, y, tl, ul, 0)
    f_bf, s_bf = rn.rnnt_align(padded[..., :V], y, tl, ul, 0)
    assert torch.equal(f_b, f_bf) and torch.equal(s_b, s_bf)
    for b in range(B):
        assert np.array_equal(f_unp[b, :ulen[b]].cpu().numpy(), planted[b])
        assert np.array_equal(f_b[b, :ulen[b]].cpu().numpy(), planted[b])     # a decision gap >= 7 against bf16 rounding of ~70 logits of size <= 16
    # scores: each of the <= 70 terms of a path moves by at most two roundings (the logit, the row's lse) of 2^-9 relative on |x| <= 16
    torch.testing.assert_close(s_b, s_pad, rtol=0, atol=70 * 2 * 16 * 2.0 ** -9)


def test_rejects_bad_arguments_and_launches_nothing(rn):
    C = importlib.import_module("ts-asr_amd._capi")
    lib = C.lib()
    B, T, U1, V = 2, 5, 4, 5
    lg = torch.zeros(B, T, U1, 8, device=DEV)
    tg = torch.ones(B, U1 - 1, device=DEV, dtype=torch.int32)
    tl, ul = dev_i32([5, 4]), dev_i32([3, 2])
    frames = torch.full((B, U1 - 1), 77, device=DEV, dtype=torch.int32)
    scores = torch.full((B,), 77.0, device=DEV)
    need = lib.tsasr_rnnt_align_workspace_bytes(B, T, U1)
    assert need > 0 and lib.tsasr_rnnt_align_workspace_bytes(0, T, U1) == 0
    ws = torch.full((need,), 0x5A, device=DEV, dtype=torch.uint8)

    def call(ws_bytes, ldf=U1 - 1, blank=0, u1=U1):
        return lib.tsasr_rnnt_align(C.ptr(lg), C.ptr(tg), tg.stride(0), C.ptr(tl), C.ptr(ul), C.ptr(frames), ldf, C.ptr(scores), B, T, u1, V, 8,
                                    blank, C.ptr(ws), ws_bytes, C.stream_ptr())
    assert call(need - 1) != 0 and b"workspace too small" in lib.tsasr_last_error()
    assert call(need, ldf=U1 - 2) != 0 and b"ldf" in lib.tsasr_last_error()
    assert call(need, blank=V) != 0 and b"blank" in lib.tsasr_last_error()
    assert call(need, u1=2049) != 0
    torch.cuda.synchronize()
    assert torch.all(frames == 77) and torch.all(scores == 77.0) and torch.all(ws == 0x5A)      # nothing ran
    assert call(need) == 0
    torch.cuda.synchronize()
    assert frames.cpu().tolist() == [[0, 0, 0], [0, 0, -1]]
    with pytest.raises(ValueError):
        rn.rnnt_align(lg[..., :V], tg[:, :1], tl, ul, 0)            # targets too short
    with pytest.raises(C.TsasrHipMissing):
        rn.rnnt_align(lg[..., :V].cpu(), tg.cpu(), tl.cpu(), ul.cpu(), 0)


def test_captured_in_a_graph_gives_the_same_bits(rn):
    """rnnt_align captured on one stream and replayed twice (workspace and outputs scribbled over in between) == the eager call."""
    C = importlib.import_module("ts-asr_amd._capi")
    lib = C.lib()
    i = 4                                                             # T = 300, U1 = 300: four waves, LDS edge words, barriers
    B, T, U1, V, tlen, ulen = CASES[i]
    lg, tg, _, _, _ = random_case(i)
    x = torch.zeros(B, T, U1, 32, device=DEV)
    x[..., :V] = torch.tensor(lg, device=DEV)
    y, tl, ul = torch.tensor(tg, device=DEV), dev_i32(tlen), dev_i32(ulen)
    f_eager, s_eager = rn.rnnt_align(x[..., :V], y, tl, ul, 0)
    frames = torch.empty(B, U1 - 1, device=DEV, dtype=torch.int32)
    scores = torch.empty(B, device=DEV)
    ws = torch.empty(lib.tsasr_rnnt_align_workspace_bytes(B, T, U1), device=DEV, dtype=torch.uint8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        C.check(lib.tsasr_rnnt_align(C.ptr(x), C.ptr(y), y.stride(0), C.ptr(tl), C.ptr(ul), C.ptr(frames), frames.stride(0), C.ptr(scores),
                                     B, T, U1, V, 32, 0, C.ptr(ws), ws.numel(), C.stream_ptr()), "tsasr_rnnt_align")
    for _ in range(2):
        ws.fill_(0xFF)
        frames.fill_(-7)
        scores.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(frames, f_eager) and torch.equal(scores, s_eager)


# ---- recipe ---------------------------------------------------------------------------------------------------------------------
SMALL = ["--d_model", "144", "--nhead", "4", "--encoder_num_layers", "2", "--speaker_num_layers", "2", "--d_ffn", "576", "--joint_dim", "160",
         "--decoder_neurons", "128", "--compute_dtype", "bf16"]
SYN = {"syn_batch": 4, "syn_seconds": 2.0, "syn_enroll_seconds": 1.0, "syn_tokens": 12}


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """train_tsasr.main on two synthetic batches with --align_file: (module, brain, result, path of the CTM)."""
    tt = importlib.import_module("train_tsasr")
    path = str(tmp_path_factory.mktemp("align") / "test.ctm")
    argv = [os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml"), "--device", "cuda:0", "--synthetic", "2", "--number_of_epochs", "1",
            "--dropout", "0.0", "--beam_size", "2", "--align_file", path]
    for k, v in SYN.items():
        argv += ["--" + k, str(v)]
    brain, result = tt.main(argv + SMALL)
    return tt, brain, result, path


def test_recipe_align_batch(trained, rn):
    tt, brain, _, _ = trained
    core = importlib.import_module("ts-asr_amd.core")
    nnet = importlib.import_module("ts-asr_amd.nnet")
    batch = tt.synthetic_loader(1, vars(brain.hparams), dict(tt.EXTRA, **SYN), 99, brain.device)[0]
    brain.modules.train()
    frames, scores = brain.align_batch(batch)
    assert brain.modules.training                                      # the training flag is restored
    tokens, rel = batch.tokens
    B, U = tokens.shape
    assert frames.shape == (B, U) and frames.dtype == torch.int32 and scores.shape == (B,)
    brain.modules.eval()
    with torch.no_grad():
        logits, _ = brain.compute_forward(batch, core.Stage.VALID)
        f_ref, s_ref = rn.transducer_align(logits, tokens, batch.mixed_sig.lengths, rel, 0)
    assert torch.equal(frames, f_ref) and torch.equal(scores, s_ref)
    tl = nnet.abs_lengths_round(batch.mixed_sig.lengths, logits.shape[1]).cpu().tolist()
    ul = nnet.abs_lengths_round(rel, U).cpu().tolist()
    fr = frames.cpu().numpy()
    assert len(set(ul)) > 1                                            # a ragged batch
    for b in range(B):
        f = fr[b, :ul[b]]
        assert np.all(f >= 0) and np.all(f < tl[b]) and np.all(np.diff(f) >= 0) and np.all(fr[b, ul[b]:] == -1)
    assert torch.isfinite(scores).all() and (scores < 0).all()


def test_train_script_writes_a_ctm(trained):
    tt, brain, result, path = trained
    nnet = importlib.import_module("ts-asr_amd.nnet")
    test = tt.synthetic_loader(1, vars(brain.hparams), dict(tt.EXTRA, **SYN), 99, brain.device)       # the script's test loader for --synthetic 2
    n_tokens = sum(int(nnet.abs_lengths_round(b.tokens.lengths, b.tokens.data.shape[1]).sum()) for b in test)
    with open(path, encoding="utf-8") as f:
        lines = [l.split() for l in f.read().splitlines()]
    assert len(lines) == n_tokens == result["align_lines"] and n_tokens > 0     # no tokenizer: one line per aligned token
    ids = [i for b in test for i in b.id]
    assert sorted(set(l[0] for l in lines)) == sorted(ids)
    last = {}
    for utt, chan, start, dur, word in lines:
        assert chan == "1" and len(start.split(".")[1]) == 3 and len(dur.split(".")[1]) == 3
        assert float(start) >= last.get(utt, 0.0) and float(dur) == pytest.approx(0.040)
        assert 0 < int(word) < 29
        last[utt] = float(start)
