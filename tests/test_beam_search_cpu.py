"""Host side of the device beam search: the ops wrappers refuse bad arguments with ValueError before any device call, the streaming
transcriber refuses an unknown search, and the workspace size follows the formula include/tsasr_hip.h documents."""
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module("ts-asr_amd.ops")
capi = importlib.import_module("ts-asr_amd._capi")
streaming = importlib.import_module("ts-asr_amd.streaming")


def _net(H=128, J=160, E=29, V=29, wdt=torch.float32):
    mats = [torch.zeros(4 * H, E, dtype=wdt), torch.zeros(4 * H, H, dtype=wdt), torch.zeros(J, H, dtype=wdt), torch.zeros(V, J, dtype=wdt)]
    return torch.eye(V, E), mats, torch.zeros(4 * H), torch.zeros(4 * H), torch.zeros(J), torch.zeros(V)


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library or the device fails the test: validation has to come first. The one library function the checks
    themselves read is the workspace's size, a function of the shape alone that touches no device."""
    def boom(*a, **k):
        raise AssertionError("reached the device before the arguments were checked")

    class SizeOnly:
        tsasr_beam_search_workspace_bytes = capi.lib().tsasr_beam_search_workspace_bytes

        def __getattr__(self, name):
            boom()
    monkeypatch.setattr(capi, "lib", SizeOnly)
    monkeypatch.setattr(capi, "require_gpu", boom)


CASES = {
    "enc 2-D": dict(enc=torch.zeros(10, 160)),
    "enc fp16": dict(enc=torch.zeros(2, 10, 160, dtype=torch.float16)),
    "empty enc": dict(enc=torch.zeros(2, 0, 160)),
    "J mismatch": dict(enc=torch.zeros(2, 10, 96)),
    "beam 1": dict(beam_size=1),
    "beam > V": dict(beam_size=30),
    "nbest 0": dict(nbest=0),
    "nbest 65": dict(nbest=65),
    "cap < beam": dict(cap=3),
    "blank outside": dict(blank=29),
    "bf16 weights with the fp32 flag": dict(net=_net(wdt=torch.bfloat16)),
    "H not a multiple of 4": dict(net=_net(H=130)),
    "V 64": dict(net=_net(V=64, E=29)),
    "embedding wider than 64": dict(net=_net(E=65)),
    "bias of the wrong size": dict(net=_net()[:5] + (torch.zeros(30),)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_beam_search_wrapper_checks(no_device, case):
    kw = dict(enc=torch.zeros(2, 10, 160), net=_net(), beam_size=4, nbest=2, cap=64, blank=0)
    kw.update(CASES[case])
    table, mats, b_ih, b_hh, b_proj, b_head = kw["net"]
    with torch.no_grad():
        with pytest.raises(ValueError):
            ops.beam_search(kw["enc"], table, mats, b_ih, b_hh, b_proj, b_head, kw["blank"], 0.01, capi.F32, kw["beam_size"], kw["nbest"], 2.3,
                            2.3, kw["cap"])


def test_beam_search_stream_wrapper_checks(no_device):
    table, mats, b_ih, b_hh, b_proj, b_head = _net()
    enc = torch.zeros(2, 8, 160)
    need = ops.beam_workspace_bytes(2, 100, 128, 160, 29, 4, 64)
    args = (table, mats, b_ih, b_hh, b_proj, b_head, 0, 0.01, capi.F32, 4, 2, 2.3, 2.3, 64)
    with torch.no_grad():
        with pytest.raises(ValueError, match="workspace"):
            ops.beam_search_stream(enc, *args, torch.zeros(need - 1, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), 100)
        with pytest.raises(ValueError, match="workspace"):
            ops.beam_search_stream(enc, *args, torch.zeros(need, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), 200)
        with pytest.raises(ValueError, match="n_valid"):
            ops.beam_search_stream(enc, *args, torch.zeros(need, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), 100)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.beam_search(enc, *args)


def test_streaming_transcriber_refuses_unknown_search():
    with pytest.raises(ValueError, match="search"):
        streaming.StreamingTranscriber(object(), search="nope")


def _formula(B, T, H, J, beam, cap):
    a16 = lambda v: -(-v // 16) * 16  # noqa: E731
    return B * (a16(64 + 24 * beam) + a16(8 * (1 + (T + 1) * beam + cap)) + 4 * (cap + beam) * (J + 2 * H))


def test_workspace_bytes_formula_and_monotone():
    lib = capi.lib()
    base = dict(B=32, T=250, H=512, J=640, beam=15, cap=512)
    for kw in (base, dict(base, T=4000), dict(base, B=1, T=1, H=4, J=4, beam=2, cap=2), dict(base, beam=4, cap=37)):
        args = [kw[k] for k in ("B", "T", "H", "J", "beam", "cap")]
        plain = args[:4] + [29] + args[4:]                   # the plain narrow search: no LM, untimed, no graph (V sizes nothing)
        assert lib.tsasr_beam_search_workspace_bytes(*plain, 0, 0, 0, 0, 0) == ops.beam_workspace_bytes(*plain) == _formula(*args)
    for k in base:
        prev = 0
        for f in (1, 2, 3, 5, 8):
            kw = dict(base, **{k: base[k] * f})
            n = ops.beam_workspace_bytes(*[kw[x] for x in ("B", "T", "H", "J")], 29, kw["beam"], kw["cap"])
            assert n > prev, k
            prev = n
    # configs[1] (B = 32, T' = 250, beam 15, default cap 512) and configs[4] (T' = 4000): the sizes DESIGN.md quotes
    assert _formula(32, 250, 512, 640, 15, 512) == 113_355_776
    assert _formula(32, 4000, 512, 640, 15, 512) == 127_755_776
    assert ops.beam_workspace_bytes(0, 250, 512, 640, 29, 15, 512) == 0


def test_workspace_bytes_every_form():
    """times x lm x bias x wide at three shapes against the one formula of include/tsasr_hip.h, written out here. lm on: the shape's own
    LM, or one layer of 32 where it names none."""
    lib = capi.lib()
    a16 = lambda v: -(-v // 16) * 16  # noqa: E731
    for B, T, H, J, V, beam, cap, Ll, Hl in ((3, 24, 64, 64, 100, 4, 512, 0, 0), (2, 12, 512, 640, 1024, 4, 512, 2, 1024),
                                             (1, 4096, 64, 64, 101, 15, 33, 1, 32)):
        for times in (0, 1):
            for lm in (0, 1):
                for bias in (0, 1):
                    for wide in (0, 1):
                        L, Hh = ((Ll or 1), (Hl or 32)) if lm else (0, 0)
                        nodes = 1 + (T + 1) * beam + cap
                        lmw = (-(-V // 4) * 4 if wide else 64) + 2 * L * Hh if L > 0 else 0
                        want = B * (a16(64 + 24 * beam) + a16(8 * nodes) + 4 * (cap + beam) * (J + 2 * H + lmw) + (times + bias) * a16(4 * nodes))
                        assert lib.tsasr_beam_search_workspace_bytes(B, T, H, J, V, beam, cap, L, Hh, times, bias, wide) == want
                        assert ops.beam_workspace_bytes(B, T, H, J, V, beam, cap, L, Hh, bool(times), bool(bias), bool(wide)) == want
