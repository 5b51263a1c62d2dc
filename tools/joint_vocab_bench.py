"""Lab bench of the joint -> loss -> backward chain per vocabulary size: joint forward, loss forward, loss backward and joint backward on
their own at the benchmark batch (B=32, T'=250, U1=121, J=640) for V = 29 (the narrow kernels of csrc/rnnt.hip), 256 and 1024 (the
vocabulary-tiled kernels of csrc/joint_wide.hip).

    python tools/joint_vocab_bench.py [--vocab 29 256 1024] [--reps 5] [--dtype bf16] [--longform]

Per phase: median microseconds, achieved TFLOP/s against 2*B*T*U1*J*V per GEMM-equivalent pass (joint forward: one pass, the logits; joint
backward: two, dh and dW; the loss kernels have none) and GB/s against the bytes the phase has to move at least (the [B,T,U1,ldl] fp32
logits and / or their gradient once each; the activations and the head matrix are noise beside them).

Beside the phases: the whole chain (forward + loss + backward, one pair of HIP events around it, median of the same number of runs) on the
materialised route and on the lazy one (fused_joint_logits(..., materialize=False): the fused joint + loss kernels, no logits tensor; for
V <= 32 the handle is materialised, so the row says so), and both routes' peak allocated bytes (torch.cuda.max_memory_allocated above what
was allocated before the chain). --longform runs the chains alone at B = 1, T' = 4000, U1 = 1921, J = 640 for V = 256 and 1024; a route
whose logits + dlogits would not fit the device's free memory is skipped, and the tool says so.
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rnnt = importlib.import_module("ts-asr_amd.rnnt")


def make_inputs(B, T, U1, J, V, dtype):
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(5)
    enc = torch.randn(B, T, J, generator=g).to(dev, dtype).requires_grad_(True)
    dec = torch.randn(B, U1, J, generator=g).to(dev, dtype).requires_grad_(True)
    W = (torch.randn(V, J, generator=g) / J ** 0.5).to(dev).requires_grad_(True)
    b = (0.1 * torch.randn(V, generator=g)).to(dev).requires_grad_(True)
    targets = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32).to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul = torch.full((B,), U1 - 1, dtype=torch.int32, device=dev)
    return enc, dec, W, b, targets, tl, ul


def chain(B, T, U1, J, V, reps, dtype, lazy):
    """Forward + loss + backward of one route: (median microseconds, peak allocated bytes above the inputs, loss) or None when skipped."""
    ldl = 32 if V <= 32 else (V + 31) // 32 * 32
    need = 2 * B * T * U1 * ldl * 4
    if not lazy or V <= 32:
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            print(f"    chain {'lazy (narrow: materialised)' if lazy else 'materialised':12s} skipped: logits + dlogits need {need / 1e9:.1f} GB, "
                  f"{free / 1e9:.1f} GB free")
            return None
    enc, dec, W, b, targets, tl, ul = make_inputs(B, T, U1, J, V, dtype)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, peak, loss = [], 0, None
    for r in range(reps + 2):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0.record()
        logits = rnnt.fused_joint_logits(enc, dec, W, b, 0.01, tl, ul, materialize=not lazy)
        loss = rnnt.rnnt_costs(logits, targets, tl, ul, 0).sum()
        grads = torch.autograd.grad(loss, (enc, dec, W, b))
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            times.append(e0.elapsed_time(e1) * 1e3)
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del logits, grads
    times.sort()
    return times[len(times) // 2], peak, float(loss.detach())


def chains(B, T, U1, J, V, reps, dtype):
    rows = {}
    for lazy in (False, True):
        res = chain(B, T, U1, J, V, reps, dtype, lazy)
        name = "materialised" if not lazy else ("lazy" if V > 32 else "lazy (narrow: materialised)")
        rows[name] = res
        if res is not None:
            print(f"    chain {name:12s} {res[0]:11.1f} us   peak {res[1] / 1e6:10.1f} MB   loss {res[2]:.3f}   (median of {reps})")
    return rows


def run(B, T, U1, J, V, reps, dtype):
    enc, dec, W, b, targets, tl, ul = make_inputs(B, T, U1, J, V, dtype)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    t = {k: [] for k in ("joint fwd", "loss fwd", "loss bwd", "joint bwd")}
    for r in range(reps + 2):
        ev[0].record()
        logits = rnnt.fused_joint_logits(enc, dec, W, b, 0.01, tl, ul)
        ev[1].record()
        costs = rnnt.rnnt_costs(logits, targets, tl, ul, 0)
        ev[2].record()
        (dlogits,) = torch.autograd.grad(costs.sum(), logits, retain_graph=True)
        ev[3].record()
        grads = torch.autograd.grad(logits, (enc, dec, W, b), dlogits)
        ev[4].record()
        torch.cuda.synchronize()
        if r >= 2:
            for i, k in enumerate(t):
                t[k].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
        del logits, costs, dlogits
    ldl = 32 if V <= 32 else (V + 31) // 32 * 32
    cells = B * T * U1
    row_bytes = cells * ldl * 4
    passes = {"joint fwd": 1, "loss fwd": 0, "loss bwd": 0, "joint bwd": 2}
    moved = {"joint fwd": row_bytes, "loss fwd": row_bytes, "loss bwd": 2 * row_bytes, "joint bwd": row_bytes}
    print(f"V={V} (rows of {ldl} floats, {row_bytes / 1e9:.2f} GB per tensor), {dtype}, sum |dbias| = {float(grads[3].abs().sum()):.4f}")
    for k, v in t.items():
        v.sort()
        us = v[len(v) // 2]
        tf = passes[k] * 2.0 * cells * J * V / us / 1e6
        print(f"    {k:9s} {us:11.1f} us   {tf:8.2f} TFLOP/s   {moved[k] / us / 1e3:8.1f} GB/s")
    del enc, dec, W, b, grads
    chains(B, T, U1, J, V, reps, dtype)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, nargs="+", default=[29, 256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--longform", action="store_true", help="the chains alone at B=1, T'=4000, U1=1921, J=640 for V = 256 and 1024")
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    if a.longform:
        for V in (256, 1024):
            print(f"long form B=1 T'=4000 U1=1921 J=640 V={V}, {dt}")
            chains(1, 4000, 1921, 640, V, a.reps, dt)
    else:
        for V in a.vocab:
            run(32, 250, 121, 640, V, a.reps, dt)
