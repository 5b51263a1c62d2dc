#!/usr/bin/env python3
"""Lab bench of the device WER / CER scorer (csrc/editdist.hip) - what profiles/wer_bench.md was measured with. Needs an MI355X.

    python tools/wer_bench.py [--out FILE.md] [--reps N]      time the host baseline and the device route, and the TEST stage
    python tools/wer_bench.py --kernel-only                   only launch the three shapes (for `rocprofv3 --kernel-trace --stats -- ...`)

Shapes: (a) a validation-shaped batch of 32 pairs, character level (about 180 symbols a side) and word level (about 30); (b) one
1920-token pair. Host baseline: the reference's algorithm (one interpreted loop iteration per lattice cell, the table of operations,
the walk back) restated below in plain Python, on this machine's CPU. Device route: ErrorRateStats.append_ids (intern-free packing into
the pinned buffer, copy, launch) followed by a synchronise; kernel alone: device events around the launch over data already on the device.
TEST stage: train_tsasr.main on the scratch recipe's small fp32 model at B = 32, then brain.evaluate with the metric keys on and off,
alternating."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = importlib.import_module("ts-asr_amd.metrics")


def host_score(a, b):
    """Pure-Python scorer: operation table row by row with the reference's comparison order, then the walk back. -> [edits, I, D, S]."""
    n, m = len(a), len(b)
    ops = [bytearray(m + 1) for _ in range(n + 1)]      # 0 match, 1 substitution, 2 deletion, 3 insertion
    prev = list(range(m + 1))
    for i in range(1, n + 1):
        cur = [i] * (m + 1)
        row, ai = ops[i], a[i - 1]
        for j in range(1, m + 1):
            ne = ai != b[j - 1]
            sc, dc, ic = prev[j - 1] + ne, prev[j] + 1, cur[j - 1] + 1
            if sc < ic and sc < dc:
                cur[j], row[j] = sc, ne
            elif dc < ic:
                cur[j], row[j] = dc, 2
            else:
                cur[j], row[j] = ic, 3
        prev = cur
    i, j, cnt = n, m, [0, 0, 0, 0]
    while i or j:
        op = 3 if i == 0 else 2 if j == 0 else ops[i][j]
        cnt[op] += 1
        i, j = i - (op != 3), j - (op != 2)
    return [cnt[1] + cnt[2] + cnt[3], cnt[3], cnt[2], cnt[1]]


def noisy_pairs(n_pairs, length, alphabet, seed, noise=0.1, jitter=True):
    rng = np.random.RandomState(seed)
    pairs = []
    for _ in range(n_pairs):
        ref = rng.randint(1, alphabet, max(1, int(length * (0.8 + 0.4 * rng.rand()))) if jitter else length).tolist()
        hyp = []
        for t in ref:
            u = rng.rand()
            if u >= noise:
                hyp.append(t)
            elif u < noise / 3:
                hyp.append(int(rng.randint(1, alphabet)))
            elif u < 2 * noise / 3:
                hyp += [t, int(rng.randint(1, alphabet))]
        pairs.append((ref, hyp))
    return pairs


SHAPES = {"32 pairs, character level (~180)": lambda: noisy_pairs(32, 180, 29, 1),
          "32 pairs, word level (~30)": lambda: noisy_pairs(32, 30, 1000, 2),
          "1 pair of 1920 tokens": lambda: noisy_pairs(1, 1920, 29, 3, noise=0.2, jitter=False)}


def device_route(pairs, reps):
    refs, hyps = [a for a, _ in pairs], [b for _, b in pairs]
    ids = [str(k) for k in range(len(pairs))]
    stats = M.ErrorRateStats()
    times = []
    for r in range(reps + 3):
        stats.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats.append_ids(ids, hyps, refs)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    counts = stats._pending[-1][1].counts.cpu().tolist()
    return statistics.median(times[3:]), counts


def kernel_alone(pairs, reps):
    buf, lay = M.pack_pairs([a for a, _ in pairs], [b for _, b in pairs])
    dev = torch.from_numpy(buf).to("cuda")
    need = M.ops.edit_distance_workspace_bytes(lay["N"], lay["cells"])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    totals = torch.zeros(8, dtype=torch.int64, device="cuda")
    times = []
    for r in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        M.launch_packed(dev, lay, totals=totals, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times[3:])


def test_stage(reps):
    mod = importlib.import_module("train_tsasr")
    argv = [os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml"), "--device", "cuda:0", "--synthetic", "2", "--number_of_epochs", "1",
            "--syn_batch", "32", "--syn_seconds", "4.0", "--syn_enroll_seconds", "2.0", "--syn_tokens", "24", "--hip_graph", "False", "--lr", "0.002",
            "--warmup_steps", "5", "--dropout", "0.0", "--beam_size", "3", "--d_model", "144", "--nhead", "4", "--encoder_num_layers", "2",
            "--speaker_num_layers", "2", "--d_ffn", "576", "--joint_dim", "160", "--decoder_neurons", "128", "--compute_dtype", "fp32"]
    brain, _ = mod.main(argv)
    opts = {"syn_batch": 32, "syn_seconds": 4.0, "syn_enroll_seconds": 2.0, "syn_tokens": 24}
    test = mod.synthetic_loader(1, vars(brain.hparams), opts, 99, brain.device)
    makers = (brain.hparams.cer_computer, brain.hparams.wer_computer)
    on, off, stats = [], [], None
    for r in range(2 * (reps + 2)):
        with_metrics = r % 2 == 0
        brain.hparams.cer_computer, brain.hparams.wer_computer = makers if with_metrics else (None, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        brain.evaluate(test)
        torch.cuda.synchronize()
        (on if with_metrics else off).append(time.perf_counter() - t0)
        if with_metrics:
            stats = dict(brain.test_stats)
    brain.hparams.cer_computer, brain.hparams.wer_computer = makers
    importlib.import_module("ts-asr_amd.nnet").set_compute_dtype(torch.bfloat16)
    return statistics.median(on[2:]), statistics.median(off[2:]), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/wer_bench.py measures on an MI355X"
    if args.kernel_only:
        for name, make in SHAPES.items():
            kernel_alone(make(), 10)
        return
    lines = ["| shape | lattice cells | host baseline (pure Python, this CPU) | device route (pack + copy + kernel + sync) | kernel alone (events) | host / device |",
             "|---|---|---|---|---|---|"]
    ok = True
    for name, make in SHAPES.items():
        pairs = make()
        cells = sum((len(a) + 1) * (len(b) + 1) for a, b in pairs)
        host_times, host_counts = [], None
        for _ in range(3 if cells < 2e6 else 2):
            t0 = time.perf_counter()
            host_counts = [host_score(a, b) for a, b in pairs]
            host_times.append(time.perf_counter() - t0)
        host = min(host_times)
        dev, counts = device_route(pairs, args.reps)
        assert counts == host_counts, "device and host counts differ"
        kern = kernel_alone(pairs, args.reps)
        ok &= dev < host
        lines.append(f"| {name} | {cells} | {host * 1e3:.2f} ms | {dev * 1e3:.3f} ms | {kern * 1e3:.3f} ms | {host / dev:.0f} x |")
        print(lines[-1], flush=True)
    t_on, t_off, stats = test_stage(max(3, args.reps // 4))
    share = (t_on - t_off) / t_on
    lines += ["", f"TEST stage of the small fp32 recipe run (one batch of 32, beam 3): {t_on * 1e3:.2f} ms with the metric keys, {t_off * 1e3:.2f} ms with them "
              f"overridden away: scoring adds {100 * share:.1f} % of the stage (token error rate {stats.get('TER')!r})."]
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        raise SystemExit("the device route is not faster than the host baseline")


if __name__ == "__main__":
    main()
