"""A language model that is no nnet.RNNLM, with the call form the transducer searcher asks of an LM: (tokens [1,1], hx) -> (logits
[1,1,V], hidden). One tanh recurrent cell between an embedding and a Linear; ``numpy_step`` restates it in float64 for
beam_lm_ref.beam_search_lm(step=)."""
import numpy as np
import torch


class TinyLM(torch.nn.Module):
    def __init__(self, V, E=6, H=10, seed=5, scale=0.8):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g) * scale)  # noqa: E731
        self.emb, self.w_x, self.w_h, self.b, self.w_o, self.b_o = mk(V, E), mk(H, E), mk(H, H), mk(H), mk(V, H), mk(V)

    def forward(self, tokens, hx=None):
        x = self.emb[tokens.long().view(-1)]                                   # [1, E]
        h = torch.zeros(1, self.w_h.shape[0], dtype=x.dtype, device=x.device) if hx is None else hx
        h = torch.tanh(x @ self.w_x.t() + h @ self.w_h.t() + self.b)
        return (h @ self.w_o.t() + self.b_o).unsqueeze(1), h

    def numpy_step(self):
        p = {k: v.detach().double().cpu().numpy() for k, v in self.named_parameters()}

        def step(tok, state):
            h = np.zeros(p["w_h"].shape[0]) if state is None else state
            h = np.tanh(p["w_x"] @ p["emb"][tok] + p["w_h"] @ h + p["b"])
            lg = p["w_o"] @ h + p["b_o"]
            m = lg.max()
            return lg - m - np.log(np.exp(lg - m).sum()), h
        return step
