"""Float64 statement of the causal features (nnet.CausalFeatures, csrc/features_stream.hip): running floor, running per-bin statistics,
a prior, frozen statistics after a stream's end. Input: the raw dB frames as fp32 (the kernel's own, or - for the CPU checks -
raw_frames() from the oracle's Fbank pieces). The floor subtraction is fp32, as the offline floor kernel does it; everything after is fp64
and the result is rounded once to fp32."""
import numpy as np
import torch

HOP, NFFT, NMELS, TOP_DB, AMIN, EPS = 160, 512, 80, 80.0, 1e-10, 1e-10


def raw_frames(wav, n_mels=NMELS):
    """wav [B,L] float32 -> raw dB [B, 1 + L//160, n_mels] float32, no floor: oracle.tsasr_ref.fbank's own steps without its last two lines."""
    from oracle import tsasr_ref as R
    wav = torch.as_tensor(wav, dtype=torch.float32)
    window = torch.hamming_window(NFFT)
    st = torch.stft(wav, NFFT, HOP, NFFT, window, center=True, pad_mode="constant", normalized=False, onesided=True, return_complex=True)
    power = (st.real ** 2 + st.imag ** 2).transpose(1, 2)
    mel = power @ R.mel_filterbank(n_mels, NFFT, 16000)
    return (10.0 * torch.log10(torch.clamp(mel, min=AMIN))).numpy().astype(np.float32)


class RunningNormRef:
    """State of B streams over n_mels bins; push(db, n_valid) returns y float32 [B,F,n_mels] and advances stream b by its first n_valid[b]
    frames. ``stats`` collects, per push, (mean, var) of every valid frame for the conditioning check of the GPU test."""

    def __init__(self, B, n_mels=NMELS, prior=None, top_db=TOP_DB, eps=EPS):
        self.B, self.M, self.top_db, self.eps = B, n_mels, np.float32(top_db), float(eps)
        self.s1 = np.zeros((B, n_mels), np.float64)
        self.s2 = np.zeros((B, n_mels), np.float64)
        self.n = np.zeros(B, np.float64)
        self.rmax = np.full(B, -np.inf, np.float32)
        if prior is not None and float(prior[2]) > 0:
            mu, sd, n0 = np.asarray(prior[0], np.float64), np.asarray(prior[1], np.float64), float(prior[2])
            self.s1[:] = n0 * mu
            self.s2[:] = n0 * (sd * sd + mu * mu)
            self.n[:] = n0
        self.min_cond = np.inf      # min over valid frames with n >= 2 and bins of var / (var + mean^2)

    def push(self, db, n_valid=None):
        db = np.asarray(db)
        assert db.dtype == np.float32 and db.shape[0] == self.B and db.shape[2] == self.M
        F = db.shape[1]
        n_valid = [F] * self.B if n_valid is None else [int(v) for v in n_valid]
        y = np.empty(db.shape, np.float32)
        for b in range(self.B):
            nv = min(max(n_valid[b], 0), F)
            for k in range(F):
                valid = k < nv
                if valid:
                    self.rmax[b] = max(self.rmax[b], db[b, k].max())
                with np.errstate(invalid="ignore"):
                    x = np.maximum(db[b, k], np.float32(self.rmax[b] - self.top_db)).astype(np.float64)   # fp32 subtraction, fp32 max
                if valid:
                    self.s1[b] += x
                    self.s2[b] += x * x
                    self.n[b] += 1.0
                n = self.n[b]
                mean = self.s1[b] / n if n > 0 else np.zeros(self.M)
                if n >= 2:
                    var = np.maximum(0.0, (self.s2[b] - self.s1[b] * self.s1[b] / n) / (n - 1.0))
                    std = np.maximum(np.sqrt(var), self.eps)
                    if valid:
                        self.min_cond = min(self.min_cond, float((var / (var + mean * mean)).min()))
                else:
                    std = np.ones(self.M)
                y[b, k] = ((x - mean) / std).astype(np.float32)
        return y


def causal_features_ref(db, n_valid=None, prior=None, splits=None):
    """Whole rows at once, or cut at the frame indices ``splits``: (y, RunningNormRef)."""
    db = np.asarray(db, np.float32)
    ref = RunningNormRef(db.shape[0], db.shape[2], prior)
    cuts = [0] + sorted(splits or []) + [db.shape[1]]
    nv = [db.shape[1]] * db.shape[0] if n_valid is None else [int(v) for v in n_valid]
    parts = [ref.push(db[:, a:b], [min(max(v - a, 0), b - a) for v in nv]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    return np.concatenate(parts, axis=1), ref
