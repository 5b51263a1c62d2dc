"""The float64 reference of the causal features (tests/helpers/stream_feats_ref.py) checked on its own: chunk invariance, the prior,
the first frame, frozen statistics after a stream's end, a known answer - and that the audio the GPU test uses is well conditioned."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import stream_feats_ref as SR  # noqa: E402
from tests.helpers.stream_feats_audio import noise_audio  # noqa: E402


def _db(B=2, L=8000, seed=3):
    return SR.raw_frames(noise_audio(B, L, seed))


def test_raw_frames_are_the_oracle_fbank_before_its_floor():
    import torch
    from oracle import tsasr_ref as R
    wav = noise_audio(2, 4000, 5)
    db = SR.raw_frames(wav)
    assert db.shape == (2, 26, 80)
    floor = db.max(axis=(1, 2), keepdims=True) - np.float32(80.0)
    assert np.array_equal(np.maximum(db, floor), R.fbank(torch.from_numpy(wav)).numpy())
    assert np.all(SR.raw_frames(np.zeros((1, 320), np.float32)) == -100.0)


def test_chunk_invariance_bit_for_bit():
    db = _db()
    whole, r0 = SR.causal_features_ref(db)
    for splits in ([1], [4, 8, 12], list(range(1, db.shape[1])), [7, 8, 30]):
        y, r = SR.causal_features_ref(db, splits=splits)
        assert np.array_equal(whole, y)
        assert np.array_equal(r0.s1, r.s1) and np.array_equal(r0.s2, r.s2) and np.array_equal(r0.n, r.n) and np.array_equal(r0.rmax, r.rmax)


def test_causal_a_frame_does_not_depend_on_later_frames():
    db = _db()
    whole, _ = SR.causal_features_ref(db)
    head, _ = SR.causal_features_ref(db[:, :17])
    assert np.array_equal(whole[:, :17], head)


def test_floor_is_the_running_maximum_and_never_revisited():
    db = np.full((1, 4, 2), -100.0, np.float32)
    db[0, 2, 0] = 10.0                                   # the maximum arrives at frame 2: frames 2, 3 are floored at -70, frames 0, 1 were not
    ref = SR.RunningNormRef(1, 2, prior=(np.zeros(2), np.ones(2), 1e12))     # (a prior that leaves x itself visible: y ~ x)
    y = ref.push(db)
    assert np.allclose(y[0, :, 1], [-100.0, -100.0, -70.0, -70.0], atol=1e-6)
    assert np.allclose(y[0, :, 0], [-100.0, -100.0, 10.0, -70.0], atol=1e-6)


def test_prior_none_equals_zero_count_and_large_count_pins_the_statistics():
    db = _db(1, 4000)
    a, _ = SR.causal_features_ref(db)
    b, _ = SR.causal_features_ref(db, prior=(np.full(80, 3.0), np.full(80, 2.0), 0.0))
    assert np.array_equal(a, b)
    mu, sd = np.linspace(-5, 5, 80), np.linspace(1, 3, 80)
    y, ref = SR.causal_features_ref(db, prior=(mu, sd, 1e12))
    x = np.maximum(db, np.maximum.accumulate(db.max(axis=2), axis=1)[..., None] - np.float32(80.0)).astype(np.float64)
    assert np.allclose(y, (x - mu) / sd, rtol=1e-4, atol=1e-4)


def test_first_frame_has_unit_deviation():
    db = _db(1, 320)
    y, _ = SR.causal_features_ref(db)
    assert np.array_equal(y[0, 0], np.zeros(80, np.float32))          # (x - x) / 1
    y, _ = SR.causal_features_ref(db, prior=(np.full(80, 1.0), np.full(80, 9.0), 0.5))     # N = 1.5 < 2: deviation 1, mean (0.5 + x) / 1.5
    x = db[0, 0].astype(np.float64)
    assert np.allclose(y[0, 0], x - (0.5 + x) / 1.5, rtol=1e-6, atol=1e-6)


def test_statistics_freeze_at_the_end_of_a_stream():
    db = _db(2, 8000)
    F = db.shape[1]
    ref = SR.RunningNormRef(2)
    y1 = ref.push(db[:, :20], [20, 13])
    s = (ref.s1.copy(), ref.s2.copy(), ref.n.copy(), ref.rmax.copy())
    y2 = ref.push(db[:, 20:], [F - 20, 0])
    assert np.array_equal(ref.s1[1], s[0][1]) and np.array_equal(ref.s2[1], s[1][1]) and ref.n[1] == 13 and ref.rmax[1] == s[3][1]
    assert ref.n[0] == F
    alone = SR.RunningNormRef(1)
    ya = alone.push(db[1:2, :13])
    assert np.array_equal(y1[1, :13], ya[0])
    # past the end: the frozen mean / deviation and the frozen maximum
    n = 13.0
    mean = ref.s1[1] / n
    std = np.sqrt((ref.s2[1] - ref.s1[1] ** 2 / n) / (n - 1))
    for k, yk in ((15, y1[1, 15]), (30, y2[1, 10])):
        x = np.maximum(db[1, k], np.float32(ref.rmax[1] - np.float32(80.0))).astype(np.float64)
        assert np.array_equal(yk, ((x - mean) / std).astype(np.float32))
    # a stream with no valid frame at all and no prior: x itself (mean 0, deviation 1)
    ref0 = SR.RunningNormRef(1)
    assert np.array_equal(ref0.push(db[:1, :3], [0]), db[:1, :3])


def test_known_answer_one_bin():
    y, _ = SR.causal_features_ref(np.array([[[1.0], [2.0], [3.0]]], np.float32))
    assert np.allclose(y[0, :, 0], [0.0, 0.5 / np.sqrt(0.5), 1.0], rtol=1e-7, atol=0)
    assert abs(y[0, 1, 0] - 0.70710678) < 1e-7


def test_gpu_test_audio_is_well_conditioned():
    """tests/test_stream_feats_gpu.py asserts var / (var + mean^2) >= 1e-3 in every bin at every valid frame for its audio; the seeds
    it uses meet that here, on the oracle's raw frames."""
    from tests.helpers.stream_feats_audio import GPU_CASES
    for B, L, seed in GPU_CASES:
        _, ref = SR.causal_features_ref(SR.raw_frames(noise_audio(B, L, seed)))
        assert ref.min_cond >= 4e-3, (B, L, seed, ref.min_cond)
