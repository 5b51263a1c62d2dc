"""Float64 restatement of the joint + head (forward and analytic backward) for the wide-vocabulary kernels (csrc/joint_wide.hip).

    logits[b,t,u,v] = bias[v] + sum_k W[v,k] * lrelu(enc[b,t,k] + dec[b,u,k])

``rounded=True`` rounds the operands where the kernels round them and nowhere else:
  forward : x = enc + dec and h = lrelu(x) are formed in float32 (as the kernel forms them from the stored activations), h and W are rounded
            to bf16, the products and sums are float64 (the kernel: fp32 MFMA accumulation), the bias is added un-rounded.
  backward: dlogits, W and h are rounded to bf16 for the three products (dh = lrelu'(x) * dlogits.W, dW = dlogits^T.h), dbias sums the
            UN-rounded dlogits (the kernel adds them in fp32 while it stages the tile), lrelu' is taken from the float32 x.
``rounded=False`` is the plain function in float64 (what oracle/tsasr_ref.joint_logits computes).
"""
import numpy as np
import torch

from oracle.golden_recipe import det_tensor

SLOPE = 0.01
FIXTURE_SHAPE = (2, 7, 5, 64)      # B, T, U1, J of tests/golden/c1_wide_vocab.npz (tools/gen_golden_wide_vocab.py)
FIXTURE_VOCABS = (33, 100)


def fixture_inputs(V):
    """(enc [B,T,J], dec [B,U1,J], W [V,J], bias [V]) float32 numpy of the reference-pin fixture, seeded by name."""
    B, T, U1, J = FIXTURE_SHAPE
    return (det_tensor("wide.enc", (B, T, J), 1.0), det_tensor("wide.dec", (B, U1, J), 1.0),
            det_tensor(f"wide.W{V}", (V, J), 1.0 / np.sqrt(J)), det_tensor(f"wide.b{V}", (V,), 0.1))


def bf16(x):
    """Round to bf16 (nearest even), returned as float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _hidden(enc, dec, slope, rounded):
    if rounded:
        x = enc.to(torch.float32)[:, :, None, :] + dec.to(torch.float32)[:, None, :, :]
        h = torch.where(x > 0, x, x * torch.tensor(slope, dtype=torch.float32))
        return x.to(torch.float64), bf16(h)
    x = enc.to(torch.float64)[:, :, None, :] + dec.to(torch.float64)[:, None, :, :]
    return x, torch.where(x > 0, x, x * slope)


def forward(enc, dec, W, bias, slope=SLOPE, rounded=True):
    """[B,T,J], [B,U1,J], [V,J], [V] -> float64 logits [B,T,U1,V]."""
    _, h = _hidden(enc, dec, slope, rounded)
    Wd = bf16(W) if rounded else W.to(torch.float64)
    return h @ Wd.t() + bias.to(torch.float64)


def backward(enc, dec, W, dlogits, slope=SLOPE, rounded=True):
    """Gradients of sum(logits * dlogits): (denc [B,T,J], ddec [B,U1,J], dW [V,J], dbias [V]) in float64."""
    x, h = _hidden(enc, dec, slope, rounded)
    g = bf16(dlogits) if rounded else dlogits.to(torch.float64)
    Wd = bf16(W) if rounded else W.to(torch.float64)
    dh = (g @ Wd) * torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))
    dW = torch.einsum("btuv,btuj->vj", g, h)
    return dh.sum(2), dh.sum(1), dW, dlogits.to(torch.float64).sum((0, 1, 2))


# ---- greedy transducer search in float64 (speechbrain/decoders/transducer.py:138-218; csrc/search.hip greedy_decode_kernel's WIDE instantiations) ----
GREEDY_BLANK_BIAS = 3.0          # added to the head's blank bias, as oracle/gen_golden_beam.py does (random heads rarely choose blank)
GREEDY_B, GREEDY_T = 3, 40
GREEDY_CASES = {                 # name -> V, learned embedding width (None: the frozen one-hot table, E = V - 1), H, J, head scale
    "v64": (64, None, 64, 64, 3.0),                # (the head scale is chosen per case so that a quarter of the decisions at least are
    "v100": (100, None, 64, 64, 1.0),              # blank and a quarter emit: greedy_case_ok)
    "v100_e128": (100, 128, 64, 64, 1.5),
    "v100_big": (100, None, 512, 640, 1.5),
    "v1024_big": (1024, None, 512, 640, 1.5),
}
FIXTURE_GREEDY = ("v64", "v100")   # the cases whose hypotheses tests/golden/c1_wide_vocab.npz pins to the reference's searcher


NARROW_CASE = ("v29", (29, None, 64, 64, 2.0))      # a character model: the narrow kernel's ground, for the test that it is untouched


def greedy_net(name, blank=0, spec=None):
    """Seeded float32 numpy weights and encoder output of a search case: emb [V,E], w_ih [4H,E], w_hh [4H,H], b_ih, b_hh [4H], w_proj [J,H],
    b_proj [J], w_head [V,J], b_head [V] (blank bias raised), enc [B,T,J]."""
    V, E, H, J, head_scale = spec or GREEDY_CASES[name]
    if E is None:
        E = V - 1
        emb = np.zeros((V, E), np.float32)
        emb[blank + 1:] = np.eye(E, dtype=np.float32)[blank:]
        emb[:blank] = np.eye(E, dtype=np.float32)[:blank]
    else:
        emb = det_tensor(f"gw.{name}.emb", (V, E), 1.0)
    d = lambda key, shape, scale: det_tensor(f"gw.{name}.{key}", shape, scale)  # noqa: E731
    net = dict(emb=emb, w_ih=d("w_ih", (4 * H, E), 1.0), w_hh=d("w_hh", (4 * H, H), 1.0 / np.sqrt(H)), b_ih=d("b_ih", (4 * H,), 0.1),
               b_hh=d("b_hh", (4 * H,), 0.1), w_proj=d("w_proj", (J, H), 2.0 / np.sqrt(H)), b_proj=d("b_proj", (J,), 0.1),
               w_head=d("w_head", (V, J), head_scale / np.sqrt(J)), b_head=d("b_head", (V,), 0.1), enc=d("enc", (GREEDY_B, GREEDY_T, J), 1.0))
    net["b_head"] = net["b_head"].copy()
    net["b_head"][blank] += GREEDY_BLANK_BIAS
    return net


def greedy(net, blank=0, slope=SLOPE):
    """Float64 greedy search over net["enc"] [B,T,J] with the predictor embedding -> LSTM step (torch gate order i, f, g, o) -> projection,
    the joint LeakyReLU(enc + pn) and the head; every tensor of ``net`` is taken as given (round them first to follow a bf16 run).
    Returns per utterance a dict: tokens, frames, logp_sum (sum of the emitted symbols' log-probabilities), margins (top-1 minus top-2
    logit at every decision), n_blank, n_emit."""
    w = {k: torch.as_tensor(v).to(torch.float64) for k, v in net.items()}
    H = w["w_hh"].shape[1]
    out = []

    def predictor(tok, h, c):
        g = w["w_ih"] @ w["emb"][tok] + w["b_ih"] + w["w_hh"] @ h + w["b_hh"]
        i, f, gg, o = torch.sigmoid(g[:H]), torch.sigmoid(g[H:2 * H]), torch.tanh(g[2 * H:3 * H]), torch.sigmoid(g[3 * H:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        return w["w_proj"] @ h + w["b_proj"], h, c

    for enc in w["enc"]:
        h = c = torch.zeros(H, dtype=torch.float64)
        pn, h, c = predictor(blank, h, c)
        res = dict(tokens=[], frames=[], logp_sum=0.0, margins=[], n_blank=0, n_emit=0)
        for t in range(enc.shape[0]):
            x = enc[t] + pn
            logits = w["w_head"] @ torch.where(x > 0, x, x * slope) + w["b_head"]
            top = torch.topk(logits, 2)
            pos = int(top.indices[0])
            res["margins"].append(float(top.values[0] - top.values[1]))
            if pos == blank:
                res["n_blank"] += 1
                continue
            res["n_emit"] += 1
            res["tokens"].append(pos)
            res["frames"].append(t)
            res["logp_sum"] += float(logits[pos] - torch.logsumexp(logits, 0))
            pn, h, c = predictor(pos, h, c)
        out.append(res)
    return out


def greedy_case_ok(results):
    """The conditions a stored / tested search case meets: at least a quarter blank and a quarter emitting decisions, and a float64
    top-2 logit margin of at least 1e-4 at every decision. Returns (ok, blank fraction, emit fraction, smallest margin)."""
    n = sum(r["n_blank"] + r["n_emit"] for r in results)
    fb, fe = sum(r["n_blank"] for r in results) / n, sum(r["n_emit"] for r in results) / n
    mm = min(min(r["margins"]) for r in results)
    return fb >= 0.25 and fe >= 0.25 and mm >= 1e-4, fb, fe, mm


def greedy_net_bf16(net):
    """The case as a bf16 device run reads it: the four matrices (the training step's bf16 shadow copies) and the encoder output rounded to
    bf16, the embedding table and the biases fp32."""
    r = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()  # noqa: E731
    return {k: (r(v) if k in ("w_ih", "w_hh", "w_proj", "w_head", "enc") else v) for k, v in net.items()}
