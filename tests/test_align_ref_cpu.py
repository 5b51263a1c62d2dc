"""The float64 alignment reference of tests/helpers/align_ref.py against a brute force over all paths and the reference's known-answer
logits, and the host side of forced alignment (ts-asr_amd/align.py: word spans and the CTM writer). No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import align_ref as AR  # noqa: E402

# vendor/speechbrain/tests/unittests/test_losses.py:120-134 (targets [1, 2], blank 0)
KAT_LOGITS = np.array([[[0.1, 0.6, 0.1, 0.1, 0.1], [0.1, 0.1, 0.6, 0.1, 0.1], [0.1, 0.1, 0.2, 0.8, 0.1]],
                       [[0.1, 0.6, 0.1, 0.1, 0.1], [0.1, 0.1, 0.2, 0.1, 0.1], [0.7, 0.1, 0.2, 0.1, 0.1]]])


@pytest.fixture(scope="module")
def AL():
    return importlib.import_module("ts-asr_amd.align")


@pytest.fixture(scope="module")
def M():
    return importlib.import_module("ts-asr_amd.metrics")


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("U", [0, 1, 2, 3])
def test_viterbi_equals_brute_force(T, U):
    rng = np.random.default_rng(100 * T + U)
    for _ in range(5):
        lp = AR.log_softmax(rng.standard_normal((T, U + 1, 5)) * 2)
        tg = rng.integers(1, 5, size=max(U, 1))
        fr, sc = AR.viterbi(lp, tg, T, U)
        bf, bs, allp = AR.brute_force(lp, tg, T, U)
        assert np.array_equal(fr, bf)
        assert sc == pytest.approx(bs, abs=1e-12)
        assert AR.path_score(lp, tg, fr, T, U) == pytest.approx(sc, abs=1e-12)
        assert all(s <= sc + 1e-12 for s, _ in allp)


def test_tie_rule_of_the_reference():
    """Identical logits in every cell: every path has the same score; blank wins ties, so every label is emitted in frame 0 - which is also
    what the brute force picks as the path with the lexicographically smallest (f_{U-1}, ..., f_0)."""
    lp = AR.log_softmax(np.zeros((4, 4, 5)))
    fr, _ = AR.viterbi(lp, [1, 2, 3], 4, 3)
    bf, _, _ = AR.brute_force(lp, [1, 2, 3], 4, 3)
    assert np.array_equal(fr, [0, 0, 0]) and np.array_equal(bf, [0, 0, 0])


def test_known_answer():
    lp = AR.log_softmax(KAT_LOGITS)
    fr, sc, gap = AR.viterbi(lp, [1, 2], 2, 2, return_gap=True)
    assert np.array_equal(fr, [0, 0])
    assert sc == pytest.approx(-5.45381, abs=1e-5)
    _, _, allp = AR.brute_force(lp, [1, 2], 2, 2)
    assert [fr for _, fr in allp][0] == (0, 0) and len(allp) == 3
    assert allp[1][0] == pytest.approx(-5.67268, abs=1e-5) and allp[2][0] == pytest.approx(-5.67268, abs=1e-5)
    assert gap == pytest.approx(5.67268 - 5.45381, abs=2e-5)


def test_path_score_rejects_invalid_paths():
    lp = AR.log_softmax(KAT_LOGITS)
    with pytest.raises(AssertionError):
        AR.path_score(lp, [1, 2], [1, 0], 2, 2)      # decreasing
    with pytest.raises(AssertionError):
        AR.path_score(lp, [1, 2], [0, 2], 2, 2)      # frame outside the utterance
    with pytest.raises(AssertionError):
        AR.path_score(lp, [1, 2], [-1, 0], 2, 2)


def test_planted_path_is_the_best_path():
    rng = np.random.default_rng(3)
    lg = (rng.standard_normal((2, 12, 6, 7)) * 2).astype(np.float32)
    tg = rng.integers(1, 7, size=(2, 5)).astype(np.int32)
    fr = AR.planted(rng, lg, tg, [12, 7], [5, 3], 10.0)
    for b, (T, U) in enumerate(((12, 5), (7, 3))):
        got, _, gap = AR.viterbi(AR.log_softmax(lg[b]), tg[b], T, U, return_gap=True)
        assert np.array_equal(got, fr[b]) and gap >= 1.0


# ---- host side: word spans and CTM ------------------------------------------------------------------------------------------------
PIECES = ["<blank>", "▁", "a", "b", "c", "▁the"]
FS = 0.040


def test_word_spans_char_pieces(AL, M):
    tok = M.CharTokenizer(PIECES)
    tokens = [2, 3, 1, 4, 2]                     # "ab ca"
    frames = [3, 5, 9, 9, 20]
    spans = AL.word_spans(frames, tokens, PIECES, FS)
    assert [w for w, _, _ in spans] == tok([tokens])[0] == ["ab", "ca"]
    assert spans[0][1:] == pytest.approx((3 * FS, 6 * FS))
    assert spans[1][1:] == pytest.approx((9 * FS, 21 * FS))      # the word starts with its first token, the boundary piece


def test_word_spans_leading_and_consecutive_boundaries(AL):
    spans = AL.word_spans([0, 1, 2, 4, 4, 7], [1, 2, 1, 1, 3, 1], PIECES, FS)      # "▁a▁▁b▁": empty words are dropped
    assert [w for w, _, _ in spans] == ["a", "b"]
    assert spans[0][1:] == pytest.approx((0.0, 2 * FS))
    assert spans[1][1:] == pytest.approx((4 * FS, 5 * FS))


def test_word_spans_empty_target_and_padding(AL):
    assert AL.word_spans([], [], PIECES, FS) == []
    assert AL.word_spans([-1, -1], [], PIECES, FS) == []
    spans = AL.word_spans([2, 3, -1, -1], [2, 3, 0, 0], PIECES, FS)                 # frames of padded columns are -1
    assert [w for w, _, _ in spans] == ["ab"] and spans[0][1:] == pytest.approx((2 * FS, 4 * FS))


def test_word_spans_multi_character_piece(AL):
    spans = AL.word_spans([1, 6, 7, 11], [5, 5, 2, 4], PIECES, FS)                  # "▁the" "▁the" "a" "c" -> the, theac
    assert [w for w, _, _ in spans] == ["the", "theac"]
    assert spans[0][1:] == pytest.approx((1 * FS, 2 * FS))
    assert spans[1][1:] == pytest.approx((6 * FS, 12 * FS))


def test_token_spans_and_frame_seconds(AL):
    assert AL.token_spans([0, 2, -1], [7, 9, 0], FS) == [("7", 0.0, pytest.approx(FS)), ("9", pytest.approx(2 * FS), pytest.approx(3 * FS))]
    assert AL.frame_seconds({"hop_length": 10}) == pytest.approx(0.040)
    hp = importlib.import_module("ts-asr_amd.hparams")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "hparams", "conformer-t_scratch_mi355x.yaml")) as f:
        assert AL.frame_seconds(hp.load_hyperpyyaml(f, {})) == pytest.approx(0.040)


def test_write_ctm(AL, tmp_path):
    path = tmp_path / "a.ctm"
    n = AL.write_ctm(str(path), ["u1", "u2", "u3"], [[("ab", 0.12, 0.24), ("ca", 0.36, 0.84)], [], [("the", 1.0, 1.04)]])
    assert n == 3
    assert path.read_text(encoding="utf-8").splitlines() == ["u1 1 0.120 0.120 ab", "u1 1 0.360 0.480 ca", "u3 1 1.000 0.040 the"]
