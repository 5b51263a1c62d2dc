"""Bench of the auxiliary CTC branch: proj_ctc + loss forward + backward on the hand-written kernels (ctc.project, csrc/ctc.hip) beside
the library route on the same inputs, F.ctc_loss(F.log_softmax(proj(x), -1).transpose(0, 1), ...) on the GPU - the yardstick, which
writes a log-prob tensor that ours does not. Both chains are timed with device events around a whole forward + backward (the library
route's host synchronisation inside F.ctc_loss is part of what a step with it would pay), alternated in one process after a warm-up;
medians and the min - max spread are printed, and a split of our chain into head forward / loss forward / loss backward / head backward.

    python tools/ctc_bench.py [--reps 30] [--dtype bf16|fp32] [--only bench|v1024|long]

Shapes: the benchmark batch (bench.py: B = 32, T' = 250, V = 29, its token lengths U = 120), the same with V = 1024, and the long form
B = 1, T' = 4000, U = 1920. One JSON line per shape at the end."""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ctc = importlib.import_module("ts-asr_amd.ctc")
nnet = importlib.import_module("ts-asr_amd.nnet")

SHAPES = {"bench": dict(B=32, T=250, U=120, V=29), "v1024": dict(B=32, T=250, U=120, V=1024), "long": dict(B=1, T=4000, U=1920, V=29)}
J = 640


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def run(name, B, T, U, V, reps, dtype):
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(5)
    nnet.set_compute_dtype(dtype)
    x = (torch.randn(B, T, J, generator=g) * 0.5).to(dtype).to(dev).requires_grad_(True)
    head = nnet.Linear(input_size=J, n_neurons=V).to(dev)
    targets = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
    tl = torch.randint(T * 3 // 4, T + 1, (B,), generator=g, dtype=torch.int32)
    ul = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32)
    tl[0], ul[0] = T, U
    tl, ul = tl.to(dev), ul.to(dev)
    tg64, tl64, ul64 = targets.long(), tl.long(), ul.long()
    w16, b32 = head.w.weight.detach().to(dtype), head.w.bias.detach().to(dtype)
    w16.requires_grad_(True)

    def ours(ev=None):
        x.grad = None
        head.w.weight.grad = head.w.bias.grad = None
        if ev:
            ev[0].record()
        s = ctc.project(head, x)
        if ev:
            ev[1].record()
        c = ctc.ctc_costs(s, targets, tl, ul, 0)
        if ev:
            ev[2].record()
        gs = torch.autograd.grad(c.sum(), s, retain_graph=True)[0] if ev else None
        if ev:
            ev[3].record()
            s.backward(gs)
            ev[4].record()
        else:
            c.sum().backward()
        return c

    def library():
        x.grad = w16.grad = None
        s = F.linear(x, w16, b32)
        c = F.ctc_loss(F.log_softmax(s.float(), -1).transpose(0, 1), tg64, tl64, ul64, 0, reduction="none", zero_infinity=True)
        c.sum().backward()
        return c

    for _ in range(5):
        co, cl = ours(), library()
    torch.cuda.synchronize()
    close = torch.allclose(co.detach(), cl.detach(), rtol=2e-2, atol=1e-1)
    t_ours, t_lib, split = [], [], []
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    for r in range(reps):
        for which in ((ours, library) if r % 2 == 0 else (library, ours)):      # alternated
            e[0].record()
            which()
            e[1].record()
            torch.cuda.synchronize()
            (t_ours if which is ours else t_lib).append(e[0].elapsed_time(e[1]) * 1e3)
    for r in range(max(reps // 2, 5)):
        ours(ev)
        torch.cuda.synchronize()
        split.append([ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(4)])
    parts = [med([s[k] for s in split]) for k in range(4)]
    out = dict(shape=name, B=B, T=T, U=U, V=V, dtype=str(dtype).split(".")[-1], reps=reps, ours_us=round(med(t_ours), 1),
               ours_min_max_us=[round(min(t_ours), 1), round(max(t_ours), 1)], library_us=round(med(t_lib), 1),
               library_min_max_us=[round(min(t_lib), 1), round(max(t_lib), 1)],
               split_us=dict(head_fwd=round(parts[0], 1), loss_fwd=round(parts[1], 1), loss_bwd=round(parts[2], 1), head_bwd=round(parts[3], 1)),
               costs_agree=bool(close), cost0=round(float(co[0]), 4), library_cost0=round(float(cl[0]), 4))
    print(f"{name}: B={B} T'={T} U={U} V={V} {out['dtype']}: ours {out['ours_us']:.1f} us [{out['ours_min_max_us'][0]:.1f} .. {out['ours_min_max_us'][1]:.1f}]   "
          f"library {out['library_us']:.1f} us [{out['library_min_max_us'][0]:.1f} .. {out['library_min_max_us'][1]:.1f}]   split {out['split_us']}   "
          f"costs[0] {out['cost0']} / {out['library_cost0']}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--only", default=None, choices=list(SHAPES))
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    res = [run(n, reps=a.reps, dtype=dt, **s) for n, s in SHAPES.items() if a.only in (None, n)]
    for r in res:
        print(json.dumps(r))
