"""Lab bench of the joint -> loss -> backward chain per vocabulary size: joint forward, loss forward, loss backward and joint backward on
their own at the benchmark batch (B=32, T'=250, U1=121, J=640) for V = 29 (the narrow kernels of csrc/rnnt.hip), 256 and 1024 (the
vocabulary-tiled kernels of csrc/joint_wide.hip).

    python tools/joint_vocab_bench.py [--vocab 29 256 1024] [--reps 5] [--dtype bf16]

Per phase: median microseconds, achieved TFLOP/s against 2*B*T*U1*J*V per GEMM-equivalent pass (joint forward: one pass, the logits; joint
backward: two, dh and dW; the loss kernels have none) and GB/s against the bytes the phase has to move at least (the [B,T,U1,ldl] fp32
logits and / or their gradient once each; the activations and the head matrix are noise beside them).
"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rnnt = importlib.import_module("ts-asr_amd.rnnt")


def run(B, T, U1, J, V, reps, dtype):
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(5)
    enc = torch.randn(B, T, J, generator=g).to(dev, dtype).requires_grad_(True)
    dec = torch.randn(B, U1, J, generator=g).to(dev, dtype).requires_grad_(True)
    W = (torch.randn(V, J, generator=g) / J ** 0.5).to(dev).requires_grad_(True)
    b = (0.1 * torch.randn(V, generator=g)).to(dev).requires_grad_(True)
    targets = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32).to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul = torch.full((B,), U1 - 1, dtype=torch.int32, device=dev)
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, nargs="+", default=[29, 256, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    a = ap.parse_args()
    for V in a.vocab:
        run(32, 250, 121, 640, V, a.reps, torch.bfloat16 if a.dtype == "bf16" else torch.float32)
