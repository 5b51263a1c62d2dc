"""The CTC case list shared by tests/test_ctc_ref_cpu.py (helper vs torch's CPU float64 function) and tests/test_ctc_gpu.py (kernels vs helper):
the smallest shapes that reach each path of csrc/ctc.hip. Its lattice kernel gives a thread 4 consecutive states and a workgroup
64 .. 1024 threads, so S = 2 U + 1 crosses an ownership boundary at every multiple of 4, a wave boundary at 256 and workgroup-size steps
at every 256 states: U = 31 / 32 (S = 63 / 65), 63 / 64 (127 / 129), 127 / 128 (255 / 257: one wave / two), 511 / 512 (256 / 320 threads), 2047
(4095 states, 1024 threads). Everything is drawn from a seeded generator; scores are float32 values (bf16 cases round them on the way in)."""
import functools

import numpy as np

GSCALE = np.array([1.0, 0.0, -2.5, 1e3, 0.37, 1.0])      # 0, a negative value and 1e3 among them
GRID_U = (0, 1, 31, 32, 63, 64, 127, 128, 511, 512, 2047)


def _case(name, x, targets, tlen, ulen, blank=0, dtype="fp32", skip=()):
    B = x.shape[0]
    return dict(name=name, x=x.astype(np.float32), targets=np.asarray(targets, np.int64).reshape(B, np.size(targets) // B), tlen=np.asarray(tlen, np.int64),
                ulen=np.asarray(ulen, np.int64), blank=blank, dtype=dtype, gscale=GSCALE[np.arange(B) % len(GSCALE)].copy(),
                infeasible=tuple(skip))


def _labels(rng, B, U, V, blank):
    ids = np.array([v for v in range(V) if v != blank] or [0])
    return ids[rng.integers(0, len(ids), (B, max(U, 0)))].reshape(B, U)


def grid(U):
    """B = 6 utterances of U labels with T_b = 1, 2, 3, U, 2 U + 1, 250 frames (0 is clamped to 1). The T_b = U utterance has no adjacent
    equal labels: exactly at the feasibility limit, a single path."""
    rng = np.random.default_rng(1000 + U)
    tlen = np.array([1, 2, 3, U, 2 * U + 1, 250])
    T, V = int(max(tlen.max(), 1)), 5
    y = _labels(rng, 6, U, V, 0)
    y[3] = 1 + (np.arange(U) % 2)
    return _case(f"grid_U{U}", rng.standard_normal((6, T, V)), y, tlen, np.full(6, U))


def limit():
    """y = 1 1 2 2 2 3: three adjacent repeats, so 9 frames carry exactly one path (1 _ 1 2 _ 2 _ 2 3); 8 frames none; 12 many."""
    rng = np.random.default_rng(7)
    y = np.tile(np.array([1, 1, 2, 2, 2, 3]), (3, 1))
    return _case("limit", rng.standard_normal((3, 12, 4)) * 2, y, [9, 8, 12], [6, 6, 6], skip=(1,))


LIMIT_PATH = (1, 0, 1, 2, 0, 2, 0, 2, 3)


def repeats():
    """aab, aaa, abab and 64 equal labels (127 frames at least) in one batch."""
    rng = np.random.default_rng(8)
    y = np.zeros((4, 64), np.int64)
    y[0, :3], y[1, :3], y[2, :4], y[3] = (1, 1, 2), (1, 1, 1), (1, 2, 1, 2), 3
    return _case("repeats", rng.standard_normal((4, 140, 6)), y, [7, 5, 9, 140], [3, 3, 4, 64])


def ragged(dtype="fp32", scale=1.0):
    """Five utterances of different T_b and U_b; the target columns beyond U_b hold ids far outside the vocabulary, and so do a few inside
    (clamped into [0, V-1] like the RNN-T loss clamps them). Utterance 3 has more labels than frames."""
    rng = np.random.default_rng(9)
    B, T, U, V = 5, 37, 11, 29
    ulen = np.array([11, 4, 0, 9, 7])
    y = _labels(rng, B, U, V, 0)
    y[0, 5], y[4, 2] = 10 ** 6, -7
    for b in range(B):
        y[b, ulen[b]:] = 2 ** 31 - 1 if b % 2 else -(2 ** 31)
    return _case(f"ragged_{dtype}_s{scale:g}", rng.standard_normal((B, T, V)) * scale, y, [37, 20, 5, 6, 31], ulen, dtype=dtype, skip=(3,))


def vocab(V, blank, dtype):
    rng = np.random.default_rng(100 + V + blank)
    B, T, U = 3, 20, 6
    return _case(f"V{V}_blank{blank}_{dtype}", rng.standard_normal((B, T, V)), _labels(rng, B, U, V, blank), [20, 13, 11], [6, 3, 6], blank=blank,
                 dtype=dtype)


def longform():
    rng = np.random.default_rng(11)
    return _case("longform", rng.standard_normal((1, 4000, 29)), _labels(rng, 1, 1920, 29, 0), [4000], [1920])


@functools.lru_cache(maxsize=None)
def build():
    cases = [grid(U) for U in GRID_U]
    cases += [limit(), repeats(), longform()]
    cases += [ragged(d, s) for d in ("fp32", "bf16") for s in (1.0, 30.0)]       # scale 30: linear-space sums would underflow
    cases += [vocab(V, b, d) for V in (2, 5, 29, 33, 256, 1024) for b in (0, V - 1) for d in ("fp32", "bf16")]
    return tuple(cases)


NAMES = [c["name"] for c in build()]


@functools.lru_cache(maxsize=None)
def get(name):
    """A case by name, built once (drawn deterministically); callers must not modify its arrays."""
    return next(c for c in build() if c["name"] == name)


def ld_of(V):
    return (V + 7) // 8 * 8


def seen(case):
    """The float64 values of the scores as the kernel sees them (bf16 cases: rounded to bf16 first)."""
    import torch
    x = torch.from_numpy(case["x"])
    if case["dtype"] == "bf16":
        x = x.to(torch.bfloat16)
    return x.double().numpy()
