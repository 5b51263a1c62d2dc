"""Streaming math on the CPU: the causal encoder restated chunk by chunk from oracle.tsasr_ref pieces (half positional table, K/V cache,
carried convolution and front-end history) equals the offline oracle; and the streaming API refuses what cannot stream before it
touches a device."""
import importlib
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import tsasr_ref as R  # noqa: E402
from oracle.golden_recipe import CFG1  # noqa: E402
from tests.test_oracle_golden import full_state_dict  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _ln(x, sd, p, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), sd[p + "weight"], sd[p + "bias"], eps)


def _attn_chunk(y, st, sd, p, H, t0, causal):
    """RelPosMHAXL on a chunk at offset t0 against the K/V cache: score = ((q+u).k_j + (q+v).pk_half[|i-j|]) * scale."""
    B, C, D = y.shape
    Dh = D // H
    qkv = (y @ sd[p + "in_proj_weight"].t()).view(B, C, H, 3 * Dh)
    q, k, v = qkv[..., :Dh], qkv[..., Dh:2 * Dh], qkv[..., 2 * Dh:]
    st["k"] = torch.cat([st["k"], k], 1)
    st["v"] = torch.cat([st["v"], v], 1)
    K, V = st["k"], st["v"]                                       # [B, t0 + C, H, Dh]
    n = K.shape[1]
    i = torch.arange(t0, t0 + C)
    j = torch.arange(n)
    pk = st["pk_half"][(i[:, None] - j[None, :]).abs()].view(C, n, H, Dh)
    u = sd[p + "pos_bias_u"].reshape(-1).view(H, Dh)
    vb = sd[p + "pos_bias_v"].reshape(-1).view(H, Dh)
    ac = torch.einsum("bihd,bjhd->bhij", q + u, K)
    bd = torch.einsum("bihd,ijhd->bhij", q + vb, pk)
    s = (ac + bd) / math.sqrt(D)
    lim = i if causal <= 1 else (i // causal + 1) * causal - 1
    s = s.masked_fill(j[None, :] > lim[:, None], float("-inf"))
    o = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, -1), V).reshape(B, C, D)
    return o @ sd[p + "out_proj.weight"].t() + sd[p + "out_proj.bias"]


def _conv_chunk(x, st, sd, p):
    D = x.shape[-1]
    w = sd[p + "conv.weight"]
    K = w.shape[-1]
    y = _ln(x, sd, p + "layer_norm.")
    y = y @ sd[p + "bottleneck.0.weight"].squeeze(-1).t() + sd[p + "bottleneck.0.bias"]
    g = y[..., :D] * torch.sigmoid(y[..., D:])
    ext = torch.cat([st["hist"], g], 1)                           # [B, K-1 + C, D]: history in place of the zero pad
    st["hist"] = ext[:, -(K - 1):]
    c = F.conv1d(ext.transpose(1, 2), w, sd[p + "conv.bias"], groups=D).transpose(1, 2)
    c = F.leaky_relu(_ln(c, sd, p + "after_conv.0."), R.LRELU_SLOPE)
    return c @ sd[p + "after_conv.2.weight"].t() + sd[p + "after_conv.2.bias"]


def _stream_encoder(feats, sd, H, L, push, causal, spk):
    B, Fm, _ = feats.shape
    D = sd["encoder.norm.norm.weight"].shape[0]
    Tmax = (Fm + 3) // 4
    pe_half = R.relpos_table(Tmax, D)[0, Tmax - 1:]               # PE(d), d = 0 .. Tmax-1: the non-negative half of the symmetric table
    K = sd["encoder.layers.0.convolution_module.conv.weight"].shape[-1]
    layers = [{"k": torch.zeros(B, 0, H, D // H), "v": torch.zeros(B, 0, H, D // H), "hist": torch.zeros(B, K - 1, D),
               "pk_half": pe_half @ sd[f"encoder.layers.{i}.mha_layer.linear_pos.weight"].t()} for i in range(L)]
    carries = [torch.zeros(B, 2, 80, 1), torch.zeros(B, 2, 40, 128)]
    fe = {k[len("frontend."):]: v for k, v in sd.items() if k.startswith("frontend.")}
    outs, t0 = [], 0
    for f0 in range(0, Fm, push):
        x = feats[:, f0:f0 + push].unsqueeze(-1)
        for bi in range(2):                                       # front-end: [carry | chunk], first output row dropped
            xe = torch.cat([carries[bi], x], 1)
            carries[bi] = xe[:, -2:]
            x = R.conv_block(xe, fe, f"convblock_{bi}.", "causal")[:, 1:]
        x = x.reshape(B, x.shape[1], -1)
        x = x @ sd["encoder.custom_src_module.layers.0.w.weight"].t() + sd["encoder.custom_src_module.layers.0.w.bias"]
        C = x.shape[1]
        for li in range(L):
            p = f"encoder.layers.{li}."
            x = x + 0.5 * R.ffn_module(x, sd, p + "ffn_module1.")
            y = _ln(x, sd, p + "norm1.norm.")
            x = x + _attn_chunk(y, layers[li], sd, p + "mha_layer.", H, t0, causal)
            x = x + _conv_chunk(x, layers[li], sd, p + "convolution_module.")
            x = x + 0.5 * R.ffn_module(x, sd, p + "ffn_module2.")
            x = _ln(x, sd, p + "norm2.norm.")
            if li == 0:
                x = x + spk                                       # injection_mode "sum" after layer 0
        outs.append(F.layer_norm(x, (D,), sd["encoder.norm.norm.weight"], sd["encoder.norm.norm.bias"], 1e-6))
        t0 += C
    return torch.cat(outs, 1)


@pytest.mark.parametrize("push,causal", [(32, 1), (28, 1), (32, 8)])
def test_chunked_causal_encoder_restatement_equals_offline_oracle(push, causal):
    sd = full_state_dict(CFG1, "sum")
    feats = torch.from_numpy(np.load(os.path.join(GOLDEN, "c1_features.npz"))["norm"])
    spk = torch.from_numpy(np.random.default_rng(3).standard_normal((4, 1, CFG1["d_model"])).astype(np.float32))
    H, L = CFG1["nhead"], CFG1["encoder_num_layers"]
    with torch.no_grad():
        f = R.frontend(feats, {k[len("frontend."):]: v for k, v in sd.items() if k.startswith("frontend.")}, "causal")
        ref = R.conformer_encoder(f, None, sd, "encoder.", H, L, spk, None, "sum", (0,), causal)
        got = _stream_encoder(feats, sd, H, L, push, causal, spk)
    assert got.shape == ref.shape
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 1e-6, rel


# ---------------------------------------------------------------------------------------------- refusals before any device call
def _fake_brain(causal, padding):
    nn_ = importlib.import_module("ts-asr_amd.nnet")
    cf = importlib.import_module("ts-asr_amd.conformer")
    fe = nn_.ConvolutionFrontEnd(input_shape=[None, None, 80], num_blocks=2, num_layers_per_block=1, out_channels=(128, 128),
                                 kernel_sizes=(3, 3), strides=(2, 2), residuals=(True, True), dropout=0.0, padding=padding)
    enc = cf.ConformerEncoder(2560, d_model=32, nhead=2, num_layers=1, d_ffn=64, dropout=0.0, activation=torch.nn.LeakyReLU,
                              kernel_size=7, causal=causal, injection_mode="sum", injection_after=0)
    mods = {"frontend": fe, "encoder": enc, "encoder_proj": nn_.Linear(input_size=32, n_neurons=16)}
    return types.SimpleNamespace(modules=mods, hparams={"greedy_searcher": torch.nn.Module()})


def test_streaming_refuses_models_that_cannot_stream():
    streaming = importlib.import_module("ts-asr_amd.streaming")
    with pytest.raises(ValueError, match="causal encoder"):
        streaming.StreamingTranscriber(_fake_brain(False, "causal"))
    with pytest.raises(ValueError, match="frontend_padding"):
        streaming.StreamingTranscriber(_fake_brain(True, "same"))
    cf = importlib.import_module("ts-asr_amd.conformer")
    enc = _fake_brain(False, "causal").modules["encoder"]
    assert isinstance(enc, cf.ConformerEncoder)
    with pytest.raises(ValueError):
        enc.init_stream(1, 8)


def test_streaming_refuses_bad_pushes_before_device_calls():
    streaming = importlib.import_module("ts-asr_amd.streaming")
    capi = importlib.import_module("ts-asr_amd._capi")
    st = streaming.StreamingTranscriber(_fake_brain(True, "causal"))
    with pytest.raises(RuntimeError):
        st.start(2, 16)                                       # grad mode on
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            st.push(torch.zeros(2, 8, 80))                    # before start()
        st.start(2, 16)
        with pytest.raises(ValueError, match="multiple of 4"):
            st.push(torch.zeros(2, 6, 80))
        with pytest.raises(ValueError):
            st.push(torch.zeros(3, 8, 80))                    # wrong batch
        assert st.enc_state is None                           # nothing was allocated
        with pytest.raises(capi.TsasrHipMissing):             # a well-formed push is a device call: refused on CPU tensors
            st.push(torch.zeros(2, 8, 80))
