#!/usr/bin/env python3
"""How long does each launch of the speaker branch's backward take INSIDE the replayed step, beside the main stream's work, and how long
when the same chain runs with nothing beside it? Like tools/step_stamps.py (TSASR_STAMPS=1: one-thread kernels that store the device
clock, captured with the step), with one more stamp in front of every library call made on the side stream between "speaker backward
starts" and "backward done"; a launch's time is the distance to the next stamp (the chain is serial in its stream), net of the distance
between two stamps with nothing in between. `--alone`: the side stream first waits for everything the main stream has enqueued and the
early weight-gradient launch is not forked, so the chain has the chip to itself (a change of this tool's run only).
usage: python tools/chain_stamps.py [--alone] [--replays N]   -> one line per library function: calls, mean microseconds per call"""
import collections
import ctypes
import importlib
import os
import sys

os.environ["TSASR_STAMPS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

bench = importlib.import_module("bench")
prof = importlib.import_module(bench.PKG + ".prof")
capi = importlib.import_module(bench.PKG + "._capi")
alone = "--alone" in sys.argv
replays = int(sys.argv[sys.argv.index("--replays") + 1]) if "--replays" in sys.argv else 8
wl = bench.WORKLOADS["scratch"]
dev = "cuda:0"
torch.cuda.set_device(0)
batch_mod = importlib.import_module(bench.PKG + ".batch")
brain, h, _ = bench.build_brain(dev, "bf16", 1, wl["overrides"], wl["yaml"])
batch = batch_mod.synthetic_batch(wl["B"], wl["T"], wl["Te"], wl["U"], feats=True, seed=1234, enroll_emb_dim=wl["emb"]).to(dev)

START, END = "speaker backward starts [side]", "backward done [side]"


def armed():
    names = prof._stamp_names
    side = getattr(brain, "_side", None)
    return (side is not None and START in names and END not in names and "backward done [main]" not in names
            and torch.cuda.current_stream().cuda_stream == side.cuda_stream)


L = capi.lib()
for name, (res, args) in capi._PROTOS.items():
    if res is not ctypes.c_int or not args or "bytes" in name:
        continue
    real = getattr(L, name)

    def wrapper(*a, _real=real, _name=name):
        if armed():
            prof.stamp("call " + _name)
        return _real(*a)
    setattr(L, name, wrapper)

if alone:
    def hook(grad):
        prof.stamp(START)
        arena = getattr(brain, "arena", None)
        main = getattr(arena, "_main_stream", None) if arena is not None else None
        if main is not None:
            ev = torch.cuda.Event()
            ev.record(main)
            torch.cuda.current_stream().wait_event(ev)
        prof.stamp("call (two stamps, nothing between)")
        prof.stamp("call (chain begins)")
        return None
    brain._flush_main_wgrads = hook
else:
    real_hook = brain._flush_main_wgrads

    def hook(grad):
        r = real_hook(grad)
        prof.stamp("call (two stamps, nothing between)")
        prof.stamp("call (chain begins)")
        return r
    brain._flush_main_wgrads = hook

brain.enable_hip_graph(warmup_steps=3)
for _ in range(6):
    brain.fit_batch(batch)
    torch.cuda.synchronize()
assert brain._graph is not None
for _ in range(10):
    brain.fit_batch(batch)
torch.cuda.synchronize()
runs = []
for _ in range(replays):
    brain.fit_batch(batch)
    torch.cuda.synchronize()
    runs.append(prof.stamps_us())
names = [n for n, _ in runs[0]]
print(f"{len(names)} stamps ({'alone' if alone else 'in step'}), {replays} replays")
idx = [i for i, n in enumerate(names) if n.startswith("call ") or n == END]
idx.sort(key=lambda i: runs[-1][i][1])
per = collections.defaultdict(list)
for r in runs:
    for a, b in zip(idx[:-1], idx[1:]):
        per[names[a]].append(r[b][1] - r[a][1])
empty = per.get("call (two stamps, nothing between)", [0.0])
e = sum(empty) / len(empty)
print(f"stamp to stamp with nothing between: {e:.2f} us (subtracted below)")
for r in runs[-3:]:
    t = dict((n, v) for n, v in r)
    print(f"  speaker backward starts -> backward done [side]: {t[END] - t[START]:.1f} us")
for n, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
    calls = len(v) // len(runs)
    print(f"{n[5:]:44s} calls {calls:4d}  mean {sum(v) / len(v) - e:8.2f} us  total {(sum(v) / len(runs)) - calls * e:8.1f} us")
