"""Chunk-by-chunk inference of the causal encoder on the MI355X: the three streaming kernels (csrc/stream.hip attention on a K/V cache
and convolution core with carried history, csrc/search.hip resumable greedy search) against the CPU oracle on whole sequences, and the
whole stream (ts-asr_amd/streaming.py) against the reference's causal goldens and the offline causal encoder."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from oracle import tsasr_ref as R  # noqa: E402
from oracle.golden_recipe import CFG1, det_tensor, golden_inputs, load_det_weights  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def rel_l2(a, b):
    return float((a.detach().float().cpu() - b.detach().float().cpu()).norm() / (b.detach().float().cpu().norm() + 1e-30))


def close(a, b, atol, rtol=0.0):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).float().cpu()
    assert torch.allclose(a, b, atol=atol, rtol=rtol), float((a - b).abs().max())


@pytest.fixture(scope="module")
def mods():
    return (importlib.import_module("ts-asr_amd.ops"), importlib.import_module("ts-asr_amd.nnet"),
            importlib.import_module("ts-asr_amd.streaming"))


# ---------------------------------------------------------------------------------------------- a) attention on a K/V cache
def _attn_stream_case(ops, B, Tp, H, Dh, causal, chunk, dtype, key_lens, tag):
    D = H * Dh
    qkv = T(det_tensor(f"{tag}.qkv", (B, Tp, 3 * D), 1.0))
    w = T(det_tensor(f"{tag}.wpos", (D, D), 1.0 / math.sqrt(D)))
    bu = T(det_tensor(f"{tag}.bu", (Dh, H), 0.1))
    bv = T(det_tensor(f"{tag}.bv", (Dh, H), 0.1))
    pk = R.relpos_table(Tp, D)[0] @ w.t()                  # [2T'-1, D]; row T'-1+d = linear_pos(PE(d))
    qkv, pk = qkv.to(dtype).float(), pk.to(dtype).float()  # the oracle sees the operands the kernel reads
    kl = torch.tensor(key_lens, dtype=torch.int32) if key_lens is not None else None
    kpm = None if kl is None else torch.arange(Tp)[None, :] >= kl[:, None].long()
    ref, _ = R.relpos_core(qkv, pk, bu, bv, H, 1.0 / math.sqrt(D), kpm, causal)
    qd, pkh = qkv.to(DEV).to(dtype), pk[Tp - 1:].contiguous().to(DEV).to(dtype)
    kc = torch.zeros(B, H, Tp, Dh, dtype=dtype, device=DEV)
    vc = torch.zeros_like(kc)
    kld = None if kl is None else kl.to(DEV)
    outs = []
    with torch.no_grad():
        for t0 in range(0, Tp, chunk):
            c = min(chunk, Tp - t0)
            ws = ops.relpos_attn_stream_workspace(B, c, H, Dh, Tp, DEV)
            outs.append(ops.relpos_attention_stream(qd[:, t0:t0 + c], kc, vc, pkh, bu.to(DEV), bv.to(DEV), kld, H, 1.0 / math.sqrt(D),
                                                    causal, t0, ws))
    out = torch.cat(outs, 1)
    torch.cuda.synchronize()
    # the cache holds the K, V rows of every frame pushed
    q4 = qd.view(B, Tp, H, 3 * Dh)
    assert torch.equal(kc, q4[..., Dh:2 * Dh].transpose(1, 2)) and torch.equal(vc, q4[..., 2 * Dh:].transpose(1, 2))
    return out, ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("causal", [1, 8])
def test_attn_stream_small_ragged_vs_oracle(mods, dtype, causal):
    ops = mods[0]
    out, ref = _attn_stream_case(ops, 4, 50, 4, 36 if dtype == torch.float32 else 32, causal, 8, dtype, [50, 37, 23, 9], "s.a")
    e = rel_l2(out, ref)
    print(f"attn stream T'=50 causal={causal} {dtype}: {e:.2e}")
    assert e < (1e-5 if dtype == torch.float32 else 8e-3), e


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("causal", [1, 40])
def test_attn_stream_d256_vs_oracle(mods, dtype, causal):
    ops = mods[0]
    out, ref = _attn_stream_case(ops, 2, 250, 4, 64, causal, 40, dtype, [250, 181], "s.b")
    e = rel_l2(out, ref)
    print(f"attn stream T'=250 causal={causal} {dtype}: {e:.2e}")
    assert e < (1e-5 if dtype == torch.float32 else 8e-3), e


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attn_stream_T4000_chunk40_vs_oracle(mods, dtype):
    """100 pushes of 40 frames at B = 1 (the key split across workgroups and its merge launch are on this path)."""
    ops = mods[0]
    assert ops.relpos_attn_stream_workspace(1, 40, 4, 64, 4000, DEV) is not None
    out, ref = _attn_stream_case(ops, 1, 4000, 4, 64, 40, 40, dtype, None, "s.c")
    e = rel_l2(out, ref)
    print(f"attn stream T'=4000 chunk 40 {dtype}: {e:.2e}")
    assert e < (1e-5 if dtype == torch.float32 else 1.5e-2), e


# ---------------------------------------------------------------------------------------------- b) convolution core with history
def _conv_stream(ops, conv, x, chunks):
    B, Tn, D = x.shape
    K = conv.kernel_size
    hist = [torch.zeros(B, K - 1, D, device=DEV), torch.zeros(B, K - 1, D, device=DEV)]
    outs, t0, i = [], 0, 0
    with torch.no_grad():
        while t0 < Tn:
            c = min(chunks[i % len(chunks)], Tn - t0)
            y = ops.layer_norm(x[:, t0:t0 + c], conv.layer_norm.weight, conv.layer_norm.bias, 1e-5)
            y2 = ops.matmul_nt(y, conv.bottleneck[0].weight)
            z = ops.convmod_stream(y2, conv.bottleneck[0].bias, conv.conv.weight, conv.conv.bias, conv.after_conv[0].weight,
                                   conv.after_conv[0].bias, hist[0], hist[1], 1e-5, conv.slope)
            hist = hist[::-1]
            outs.append(ops.linear(z, conv.after_conv[2].weight, conv.after_conv[2].bias))
            t0, i = t0 + c, i + 1
    return torch.cat(outs, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Tn,D,chunks", [(4, 50, 144, (8,)), (4, 50, 144, (7,)), (1, 4000, 256, (40,))])
def test_convmod_stream_vs_oracle(mods, dtype, B, Tn, D, chunks):
    ops, nn_ = mods[0], mods[1]
    nn_.set_compute_dtype(dtype)
    try:
        conv = load_det_weights(nn_.ConvolutionModule(D, 31, True, torch.nn.LeakyReLU, 0.0, causal=True), "blk.conv.").to(DEV).eval()
        x = T(det_tensor("stream.conv.x", (B, Tn, D), 1.0))
        out = _conv_stream(ops, conv, x.to(DEV).to(dtype), chunks)
        sd = {"c." + k: v.detach().float().cpu() for k, v in conv.state_dict().items()}
        ref = R.conv_module(x.to(dtype).float(), sd, "c.", None, True)
    finally:
        nn_.set_compute_dtype(torch.bfloat16)
    e = rel_l2(out, ref)
    print(f"conv stream {B}x{Tn}x{D} chunks {chunks} {dtype}: {e:.2e}")
    assert e < (1e-5 if dtype == torch.float32 else 1.2e-2), e


# ---------------------------------------------------------------------------------------------- c) resumable greedy search
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_greedy_stream_pieces_bit_identical(mods, dtype):
    ops = mods[0]
    C = importlib.import_module("ts-asr_amd._capi")
    brain, h = entry._config1_brain(DEV, dtype)
    brain.modules.eval()
    srch = h["greedy_searcher"]
    B, Tn, J = 4, 57, h["modules"]["encoder_proj"].w.out_features
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    enc = (T(det_tensor("stream.greedy.enc", (B, Tn, J), 3.0))).to(DEV).to(tdt).contiguous()
    assert srch._device_greedy_ok(enc)
    table, mats, b_ih, b_hh, b_proj, b_head, wdt = srch._device_greedy_args(enc)
    slope = float(srch.tjoint.nonlinearity.negative_slope)
    Hd = mats[1].shape[1]
    preds = torch.empty(B, Tn, dtype=torch.int32, device=DEV)
    logp = torch.empty(B, dtype=torch.float32, device=DEV)
    C.check(C.lib().tsasr_greedy_decode(C.ptr(enc), C.ptr(table), C.ptr(mats[0]), C.ptr(mats[1]), C.ptr(b_ih), C.ptr(b_hh), C.ptr(mats[2]),
                                        C.ptr(b_proj), C.ptr(mats[3]), C.ptr(b_head), None, None, C.ptr(preds), C.ptr(logp), B, Tn, J, Hd,
                                        table.shape[1], mats[3].shape[0], int(srch.blank_id), slope, C.io_dtype(enc), wdt, C.stream_ptr(), 0),
            "tsasr_greedy_decode")
    assert int((preds >= 0).sum()) > 0
    with torch.no_grad():
        for step in (1, 7, 40):
            state = torch.zeros(B, ops.greedy_stream_state_size(Hd, J), device=DEV)
            got, lp = [], None
            for t0 in range(0, Tn, step):
                c = min(step, Tn - t0)
                nv = torch.full((B,), c, dtype=torch.int32, device=DEV)
                p, lp = ops.greedy_decode_stream(enc[:, t0:t0 + c].contiguous(), table, mats, b_ih, b_hh, b_proj, b_head, state, nv,
                                                 srch.blank_id, slope, wdt)
                got.append(p)
            assert torch.equal(torch.cat(got, 1), preds), step
            assert torch.equal(lp, logp), step
            # a chunk with no valid frame leaves the state bit for bit as it was
            before = state.clone()
            p, lp2 = ops.greedy_decode_stream(enc[:, :5].contiguous(), table, mats, b_ih, b_hh, b_proj, b_head, state,
                                              torch.zeros(B, dtype=torch.int32, device=DEV), srch.blank_id, slope, wdt)
            assert torch.equal(state, before) and bool((p == -1).all()) and torch.equal(lp2, logp)
        # the searcher's API: hypotheses of the pieces = hypotheses of one call
        full, _, _, _ = srch(enc)
        hyps, st = [[] for _ in range(B)], None
        for t0 in range(0, Tn, 7):
            new, st = srch.greedy_stream(enc[:, t0:t0 + 7], st)
            for b in range(B):
                hyps[b] += new[b]
        assert hyps == full


# ---------------------------------------------------------------------------------------------- the whole stream
def _spk(mode, golden):
    inp = golden_inputs()
    if mode != "cross_attention":
        return T(golden["c1_chain_cat"]["spk_emb"]).to(DEV)
    from tests.test_oracle_golden import full_state_dict
    cc = {}
    R.compute_forward({k: T(v) for k, v in inp.items()}, full_state_dict(CFG1, mode), CFG1, mode, True, "causal", collect=cc)
    return cc["spk_emb"].to(DEV)


def _stream(streaming, brain, feats, enc_lens, spk, spk_len, push):
    st = streaming.StreamingTranscriber(brain)
    with torch.no_grad():
        st.start(feats.shape[0], max_frames=(feats.shape[1] + 3) // 4, speaker_embs=spk, speaker_embs_length=spk_len, keep_encoder_out=True)
        F = feats.shape[1]
        for f0 in range(0, F, push):
            st.push(feats[:, f0:f0 + push], enc_lens=enc_lens, last=f0 + push >= F)
    return st


@pytest.mark.parametrize("mode", ["cat", "sum", "prod", "cross_attention"])
def test_stream_encoder_vs_reference_causal_golden(mods, golden, mode):
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "fp32", causal_encoder=True, frontend_padding="causal", injection_mode=mode)
    try:
        inp = golden_inputs()
        feats = T(golden["c1_features"]["norm"]).to(DEV)
        ml = T(inp["mixed_lens"]).to(DEV)
        valid = nn_.abs_lengths_round(ml, 50).to(torch.int32)
        st = _stream(streaming, brain, feats, valid, _spk(mode, golden), T(inp["enroll_lens"]).to(DEV), 32)
        out = st.encoder_out()
        assert out.shape[1] == 50
        ref = T(golden["c1_encoder_variants"][f"enc:{mode}_causal"])
        rows = [(b, int(valid[b])) for b in range(4)]
        got = torch.cat([out[b, :n].cpu() for b, n in rows])
        exp = torch.cat([ref[b, :n] for b, n in rows])
        assert rel_l2(got, exp) < 2e-5
        close(got, exp, atol=1e-4, rtol=1e-4)
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def _offline_block_causal(nn_, golden, dtype):
    """Offline causal encoder (attention chunks of 8) on the golden batch and greedy search on each utterance cut to its valid frames."""
    brain, h = entry._config1_brain(DEV, dtype, causal_encoder=True, frontend_padding="causal", attention_chunk_size=8)
    brain._setup_dtype()
    m = brain.modules
    m.eval()
    inp = golden_inputs()
    feats = T(golden["c1_features"]["norm"]).to(DEV)
    ml, el = T(inp["mixed_lens"]).to(DEV), T(inp["enroll_lens"]).to(DEV)
    spk = _spk("cat", golden)
    with torch.no_grad():
        off = m.encoder(m.frontend(feats), ml, spk, el)
        off_proj = m.encoder_proj(off)
        valid = nn_.abs_lengths_round(ml, off.shape[1]).to(torch.int32)
        hyps = [h["greedy_searcher"](off_proj[b:b + 1, :int(valid[b])])[0][0] for b in range(4)]
    return brain, off, valid, hyps, (feats, spk, el)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stream_block_causal_vs_offline(mods, golden, dtype):
    """attention_chunk_size 8 (block-causal on absolute frames): streamed encoder = offline causal encoder on the valid rows, and the
    streamed greedy hypotheses = offline greedy search on each utterance cut to its valid frames (fp32: all of them; bf16: the
    untrained deterministic weights give near-tie logits, so - as for the offline bf16 path in test_variants_gpu.py - the count of
    utterances whose hypothesis equals the fp32 one must be at least the offline bf16 path's count)."""
    ops, nn_, streaming = mods
    try:
        ref_brain, ref_off, valid, ref_hyps, _ = _offline_block_causal(nn_, golden, "fp32")
        brain, off, valid, off_hyps, (feats, spk, el) = _offline_block_causal(nn_, golden, dtype) if dtype != "fp32" else \
            (ref_brain, ref_off, valid, ref_hyps, _offline_block_causal(nn_, golden, "fp32")[4])
        st = _stream(streaming, brain, feats, valid, spk, el, 32)    # 8 encoder frames per push: one attention block
        out = st.encoder_out()
        rows = [(b, int(valid[b])) for b in range(4)]
        got = torch.cat([out[b, :n] for b, n in rows])
        exp = torch.cat([off[b, :n] for b, n in rows])
        e = rel_l2(got, exp)
        hyps = st.finish()
        print(f"block-causal stream vs offline {dtype}: {e:.2e}; equal to fp32 hyps: stream {[a == r for a, r in zip(hyps, ref_hyps)]}, "
              f"offline {[a == r for a, r in zip(off_hyps, ref_hyps)]}")
        if dtype == "fp32":
            assert e < 1e-5, e
            assert hyps == off_hyps
        else:
            assert e < 2e-2, e
            assert sum(a == r for a, r in zip(hyps, ref_hyps)) >= sum(a == r for a, r in zip(off_hyps, ref_hyps))
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_stream_strict_hip_no_library_route(mods, golden, monkeypatch):
    ops, nn_, streaming = mods
    monkeypatch.setattr(ops, "STRICT_HIP", True)
    ops.LIB_FALLBACKS.clear()
    brain, h = entry._config1_brain(DEV, "bf16", causal_encoder=True, frontend_padding="causal", attention_chunk_size=8)
    try:
        feats = T(golden["c1_features"]["norm"]).to(DEV)
        st = _stream(streaming, brain, feats, None, _spk("cat", golden), T(golden_inputs()["enroll_lens"]).to(DEV), 32)
        assert len(st.finish()) == 4
        assert ops.LIB_FALLBACKS == {}
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_stream_refuses_grad_mode(mods, golden):
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "bf16", causal_encoder=True, frontend_padding="causal")
    st = streaming.StreamingTranscriber(brain)
    with pytest.raises(RuntimeError):
        st.start(4, 50)
    with torch.no_grad():
        st.start(4, 50)
    with pytest.raises(RuntimeError):
        st.push(T(golden["c1_features"]["norm"][:, :32]).to(DEV))
    nn_.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("chunk", [64, 100])
def test_attn_stream_bf16_query_groups_vs_oracle(mods, chunk):
    """bf16 matrix-core kernel with a full 64-query group and with two groups per chunk (C = 100: 64 + 36), ragged key lengths."""
    ops = mods[0]
    out, ref = _attn_stream_case(ops, 2, 250, 4, 64, 1, chunk, torch.bfloat16, [250, 181], "s.d")
    e = rel_l2(out, ref)
    print(f"attn stream bf16 T'=250 chunk {chunk}: {e:.2e}")
    assert e < 8e-3, e


def test_greedy_stream_python_loop_pieces_equal_one_call(mods, monkeypatch):
    """The step-wise loop of greedy_stream (taken where the device decoder does not apply) in pieces = the one-call search; frames past a
    stream's valid count are not decoded."""
    monkeypatch.setenv("TSASR_GREEDY_KERNEL", "0")
    brain, h = entry._config1_brain(DEV, "fp32")
    brain._setup_dtype()
    brain.modules.eval()
    srch = h["greedy_searcher"]
    B, Tn, J = 3, 23, h["modules"]["encoder_proj"].w.out_features
    enc = T(det_tensor("stream.greedy.py", (B, Tn, J), 3.0)).to(DEV)
    assert not srch._device_greedy_ok(enc)
    with torch.no_grad():
        full, _, _, _ = srch(enc)
        short, _, _, _ = srch(enc[:, :11])
        hyps, st = [[] for _ in range(B)], None
        for t0 in range(0, Tn, 5):
            c = min(5, Tn - t0)
            nv = torch.tensor([c, c, max(0, min(c, 11 - t0))], dtype=torch.int32)    # stream 2 ends after 11 frames
            new, st = srch.greedy_stream(enc[:, t0:t0 + c], st, nv)
            for b in range(B):
                hyps[b] += new[b]
    assert hyps[:2] == full[:2] and hyps[2] == short[2]
    assert sum(len(x) for x in full) > 0


def test_stream_start_with_enrollment_runs_the_speaker_branch(mods, golden):
    """start(enroll=(signals, lengths)) computes the speaker embedding through the recipe's own speaker branch (fbank, sentence
    normalisation, speaker front-end and encoder, pooling, speaker_proj): it equals the reference's, and the stream runs with it."""
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "fp32", causal_encoder=True, frontend_padding="causal")
    try:
        inp = golden_inputs()
        st = streaming.StreamingTranscriber(brain)
        with torch.no_grad():
            st.start(4, 50, enroll=(T(inp["enroll_sig"]).to(DEV), T(inp["enroll_lens"]).to(DEV)))
            e = rel_l2(st.spk, T(golden["c1_chain_cat"]["spk_emb"]))
            print(f"speaker embedding through start(enroll=...) vs reference: {e:.2e}")
            assert e < 1e-3, e
            st.push(T(golden["c1_features"]["norm"][:, :32]).to(DEV))
            assert st.encoder_frames == 8
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_stream_overflowing_push_leaves_state_unchanged(mods, golden):
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "bf16", causal_encoder=True, frontend_padding="causal")
    feats = T(golden["c1_features"]["norm"]).to(DEV)
    st = streaming.StreamingTranscriber(brain)
    with torch.no_grad():
        st.start(4, 12)
        st.push(feats[:, :32])
        mel, fe = st.mel.clone(), [c.clone() for c in st.fe_state]
        with pytest.raises(ValueError, match="max_frames"):
            st.push(feats[:, 32:64])                   # 8 + 8 > 12 encoder frames
        assert st.encoder_frames == 8 and torch.equal(st.mel, mel) and all(torch.equal(a, b) for a, b in zip(st.fe_state, fe))
        st.push(feats[:, 32:48])                       # 8 + 4 fits
        assert st.encoder_frames == 12
        enc = brain.modules.encoder
        assert any(getattr(p, "_bf16", None) is not None for p in enc.parameters())
        st.finish()
        assert all(getattr(p, "_bf16", None) is None for p in enc.parameters())    # the weights' bf16 copies are gone again
    nn_.set_compute_dtype(torch.bfloat16)
