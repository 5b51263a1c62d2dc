"""The planner of audio-fed slot sessions (ts-asr_amd/streaming.py: audio_frames_available, plan_audio_steps, audio_ring_capacity) on
the CPU: frame counts and the step schedule against a brute-force simulation that walks frame by frame and group by group, for random
sample counts, random ends and groups of 4 and 32 frames; every frame of a session goes out exactly once and in order, an ended session
emits exactly 1 + P//160 frames, and no packet sequence with N <= max_audio_samples needs more of a ring than audio_ring_capacity gives."""
import importlib
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP, PAD = 160, 256


@pytest.fixture(scope="module")
def S():
    return importlib.import_module("ts-asr_amd.streaming")


def brute_available(P, ended):
    """Frames whose samples exist: frame k reads samples [k*HOP - PAD, k*HOP + PAD); a live session must hold the last of them, an ended
    one (zeros follow) only the window's centre k*HOP <= P."""
    k = 0
    while (k * HOP <= P) if ended else (k * HOP + PAD - 1 < P):
        k += 1
    return k


def brute_steps(P, done, ended, g):
    """The issue's step rule, walked one group at a time."""
    B, done, steps = len(P), list(done), []
    while True:
        groups = {}
        for b in range(B):
            if P[b] is None:
                continue
            rem, n = brute_available(P[b], ended[b]) - done[b], 0
            while rem >= g:
                rem, n = rem - g, n + 1
            if ended[b] and rem > 0:
                n += 1                                   # the padded tail group
            if n:
                groups[b] = n
        if not groups:
            return steps, done
        k = min(groups.values())
        F = g * k
        lens = [0] * B
        for b in groups:
            lens[b] = min(brute_available(P[b], ended[b]) - done[b], F)
            assert lens[b] == F or ended[b]
        steps.append((F, [b in groups for b in range(B)], lens))
        done = [d + n for d, n in zip(done, lens)]


def test_frames_available_against_brute_force(S):
    for P in list(range(0, 1300)) + [31840, 28656, 25472, 22288]:
        for ended in (False, True):
            assert S.audio_frames_available(P, ended) == brute_available(P, ended), (P, ended)
    assert S.audio_frames_available(255, False) == 0 and S.audio_frames_available(256, False) == 1
    assert S.audio_frames_available(0, True) == 1 and S.audio_frames_available(31840, True) == 200


@pytest.mark.parametrize("g", [4, 32])
def test_plan_equals_brute_force_on_random_counts(S, g):
    rng = random.Random(100 + g)
    for _ in range(300):
        B = rng.randint(1, 5)
        P = [None if rng.random() < 0.2 else rng.choice([0, 1, 255, 256, 257, rng.randint(0, 3000), rng.randint(0, 40000)]) for _ in range(B)]
        ended = [rng.random() < 0.4 for _ in range(B)]
        done = [0 if p is None else rng.randint(0, S.audio_frames_available(p, False)) // g * g for p in P]
        got, after = S.plan_audio_steps(P, done, ended, g)
        want, after_w = brute_steps(P, done, ended, g)
        assert got == want and after == after_w, (P, done, ended)
        for F, on, lens in got:
            assert F % g == 0 and F > 0 and any(on)
            assert all((n == 0) == (not a) for a, n in zip(on, lens))
        for b in range(B):
            if P[b] is None:
                assert after[b] == done[b]
            elif ended[b]:
                assert after[b] == 1 + P[b] // HOP
            else:
                assert 0 <= S.audio_frames_available(P[b], False) - after[b] < g


@pytest.mark.parametrize("g", [4, 32])
@pytest.mark.parametrize("max_audio", [1, 160, 2000, 32000])
def test_sessions_emit_every_frame_once_and_the_ring_suffices(S, g, max_audio):
    """Random packet sequences into three slots whose sessions start, pause and end on their own: per session the emitted frame indices
    are 0, 1, 2, ... without gap or repeat, an ended session has exactly 1 + P//160, and before every append the samples a slot still
    needs plus the packet fit the ring."""
    rng = random.Random(7 * g + max_audio)
    cap = S.audio_ring_capacity(max_audio, g)
    assert cap == max_audio + (g - 1) * HOP + 2 * PAD
    B = 3
    have, done, ended, frames = [None] * B, [0] * B, [False] * B, [[] for _ in range(B)]
    finished = 0
    for _ in range(400 if max_audio > 1 else 3000):
        for b in range(B):
            if have[b] is None and rng.random() < 0.3:
                have[b], done[b], ended[b], frames[b] = 0, 0, False, []      # a session is admitted
        act = [have[b] is not None and not ended[b] and rng.random() < 0.8 for b in range(B)]
        lens = [rng.choice([0, 1, max_audio, rng.randint(0, max_audio)]) if act[b] else 0 for b in range(B)]
        stop = [act[b] and rng.random() < 0.05 for b in range(B)]
        for b in range(B):
            if act[b]:
                assert have[b] + lens[b] - max(done[b] * HOP - PAD, 0) <= cap, (have[b], lens[b], done[b], cap)
                have[b] += lens[b]
                ended[b] = stop[b]
        steps, after = S.plan_audio_steps([have[b] if act[b] else None for b in range(B)], done, ended, g)
        for F, on, ml in steps:
            for b in range(B):
                assert on[b] <= act[b]
                frames[b].extend(range(done[b], done[b] + ml[b]))
                done[b] += ml[b]
        assert done == after
        for b in range(B):
            if have[b] is None:
                continue
            assert frames[b] == list(range(len(frames[b])))
            if act[b] and not ended[b]:                  # drained: fewer than one group plus one window of samples is still needed
                assert have[b] - max(done[b] * HOP - PAD, 0) < (g - 1) * HOP + 2 * PAD
            if ended[b]:
                assert len(frames[b]) == 1 + have[b] // HOP
                have[b], finished = None, finished + 1   # released
    assert finished > 5


def test_plan_examples(S):
    # nothing before 256 samples; one group of 4 at 256 + 3*160 samples
    assert S.plan_audio_steps([255], [0], [False], 4) == ([], [0])
    assert S.plan_audio_steps([735], [0], [False], 4) == ([], [0])
    assert S.plan_audio_steps([736], [0], [False], 4) == ([(4, [True], [4])], [4])
    # an ended session's tail is a padded group with a short mel_lens; the live slot beside it sets the step's size
    steps, after = S.plan_audio_steps([2000, None, 31840], [0, 0, 190], [False, False, True], 4)
    assert steps == [(8, [True, False, True], [8, 0, 8]), (4, [False, False, True], [0, 0, 2])] and after == [8, 0, 200]
    # an ended session with no sample still has its one frame
    assert S.plan_audio_steps([0], [0], [True], 32) == ([(32, [True], [1])], [1])
    with pytest.raises(ValueError):
        S.plan_audio_steps([0], [0], [False], 0)
