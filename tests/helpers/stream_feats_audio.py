"""The audio of the causal-feature tests: white noise whose level changes every 10 ms (so that every mel bin has a healthy variance
from the second frame on) around 0 dB in the mel domain (so that the mean does not dwarf the deviation), with one stretch of exact
silence in the middle of longer signals - its frames sit 80 dB below the running maximum and are floored."""
import numpy as np

GPU_CASES = [(2, 16000 + 77, 48), (3, 3 * 160 + 100, 284), (1, 159, 13), (4, 32000, 185)]     # (B, L, seed) of tests/test_stream_feats_gpu.py


def noise_audio(B, L, seed):
    rng = np.random.default_rng(seed)
    wav = rng.standard_normal((B, L)).astype(np.float32)
    gain = 0.05 * 10.0 ** rng.uniform(-0.75, 0.75, size=(B, L // 160 + 1))
    wav *= np.repeat(gain, 160, axis=1)[:, :L].astype(np.float32)
    if L >= 8000:       # (seeds are chosen with this layout: tests/test_stream_feats_ref_cpu.py checks their conditioning)
        wav[:, L // 2:L // 2 + 1600] = 0.0
    return wav
