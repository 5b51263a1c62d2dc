"""Lab bench of forced alignment (tsasr_rnnt_align: rnnt_lp + rnnt_viterbi) beside the loss forward (tsasr_rnnt_loss_fwd: rnnt_lp +
rnnt_alphabeta) at the same lattice, in the same run - the lattices of tools/rnnt_bench.py.

    python tools/align_bench.py [--long] [--reps 50] [--json PATH]

Both go through the C-ABI on preallocated buffers (no allocation in the timed window). Per repetition the stream is pre-loaded with
two 256 MB fills (~0.1 ms of device time), then [event, align, event, loss forward, event] are enqueued behind it, so the launches are
queued before the device reaches them and the events time the device, not the enqueue; the order of the two alternates between
repetitions. Reported: the median over the repetitions after 5 warm-up rounds, and the ratio align / loss forward.
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
C = importlib.import_module("ts-asr_amd._capi")


def run(B, T, U, V, reps, ragged):
    dev, lib = "cuda", C.lib()
    U1 = U + 1
    g = torch.Generator(device="cpu").manual_seed(5)
    logits = torch.zeros(B, T, U1, 32)
    logits[..., :V] = torch.randn(B, T, U1, V, generator=g)
    logits = logits.to(dev)
    targets = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
    tl = torch.full((B,), T, dtype=torch.int32)
    ul = torch.full((B,), U, dtype=torch.int32)
    if ragged and B > 1:
        tl = torch.randint(T // 2, T + 1, (B,), generator=g, dtype=torch.int32); tl[0] = T
        ul = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32); ul[0] = U
    tl, ul = tl.to(dev), ul.to(dev)
    frames = torch.empty(B, U, dtype=torch.int32, device=dev)
    scores = torch.empty(B, device=dev)
    costs = torch.empty(B, device=dev)
    ws_a = torch.empty(lib.tsasr_rnnt_align_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    ws_l = torch.empty(lib.tsasr_rnnt_loss_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    filler = torch.empty(64 << 20, device=dev)      # 256 MB fill: ~100 us of device time ahead of the timed launches

    def align():
        C.check(lib.tsasr_rnnt_align(C.ptr(logits), C.ptr(targets), targets.stride(0), C.ptr(tl), C.ptr(ul), C.ptr(frames), frames.stride(0),
                                     C.ptr(scores), B, T, U1, V, 32, 0, C.ptr(ws_a), ws_a.numel(), C.stream_ptr()), "tsasr_rnnt_align")

    def loss():
        C.check(lib.tsasr_rnnt_loss_fwd(C.ptr(logits), C.ptr(targets), targets.stride(0), C.ptr(tl), C.ptr(ul), C.ptr(costs), B, T, U1, V, 32, 0,
                                        C.ptr(ws_l), ws_l.numel(), C.stream_ptr()), "tsasr_rnnt_loss_fwd")

    ta, tf = [], []
    for r in range(reps + 5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        first, second = (align, loss) if r % 2 == 0 else (loss, align)
        filler.zero_()
        filler.zero_()
        ev[0].record()
        first()
        ev[1].record()
        second()
        ev[2].record()
        torch.cuda.synchronize()
        if r >= 5:
            a, b = ev[0].elapsed_time(ev[1]) * 1e3, ev[1].elapsed_time(ev[2]) * 1e3
            ta.append(a if first is align else b)
            tf.append(b if first is align else a)
    ta.sort(); tf.sort()
    med_a, med_f = ta[len(ta) // 2], tf[len(tf) // 2]
    res = {"B": B, "T": T, "U1": U1, "V": V, "ragged": bool(ragged), "reps": reps, "align_us": round(med_a, 1), "loss_fwd_us": round(med_f, 1),
           "align_over_loss_fwd": round(med_a / med_f, 3), "align_us_min_max": [round(ta[0], 1), round(ta[-1], 1)],
           "loss_fwd_us_min_max": [round(tf[0], 1), round(tf[-1], 1)], "score_sum": scores.double().sum().item(),
           "cost_sum": costs.double().sum().item(), "workspace_bytes": {"align": ws_a.numel(), "loss": ws_l.numel()}}
    print(f"[{B},{T},{U1},{V}] ragged={ragged}: rnnt_align {med_a:9.1f} us   tsasr_rnnt_loss_fwd {med_f:9.1f} us   ratio {med_a / med_f:.3f}   "
          f"(sum of best-path scores {res['score_sum']:.4f} <= -sum of costs {-res['cost_sum']:.4f})")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true", help="B=1, T'=4000, U1=1921 (default: B=32, T'=250, U1=121)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None, help="also write the results there")
    a = ap.parse_args()
    out = [run(1, 4000, 1920, 29, a.reps, False)] if a.long else [run(32, 250, 120, 29, a.reps, False), run(32, 250, 120, 29, a.reps, True)]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
