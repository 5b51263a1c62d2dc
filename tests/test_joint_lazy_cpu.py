"""Host side of the lazy joint logits (rnnt.JointLogits, the hparams key joint_logits): what needs no GPU."""
import importlib
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rn():
    return importlib.import_module("ts-asr_amd.rnnt")


def cpu_handle(rn, B=2, T=7, U1=4, J=64, V=100, **kw):
    return rn.fused_joint_logits(torch.zeros(B, T, J), torch.zeros(B, U1, J), torch.zeros(V, J), torch.zeros(V), materialize=False, **kw)


def test_a_handle_from_cpu_tensors_launches_nothing(rn, monkeypatch):
    C = importlib.import_module("ts-asr_amd._capi")
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("building a handle must not touch the library"))
    h = cpu_handle(rn, slope=0.02, enc_abs_lens=torch.tensor([7, 5]), tok_abs_lens=torch.tensor([3, 1]))
    assert isinstance(h, rn.JointLogits)
    assert h.shape == (2, 7, 4, 100) and tuple(h.size()) == (2, 7, 4, 100) and h.size(3) == 100 and h.dim() == 4
    assert h.dtype == torch.float32 and h.device == torch.device("cpu")
    assert h.slope == 0.02 and h.enc_abs_lens.tolist() == [7, 5] and h.tok_abs_lens.tolist() == [3, 1]
    assert h.wide and not cpu_handle(rn, V=29).wide


def test_indexing_and_arithmetic_name_materialize(rn):
    h = cpu_handle(rn)
    for use in (lambda: h[0], lambda: h[..., :5], lambda: h + 1, lambda: 2 * h, lambda: h - h, lambda: h / 2, lambda: -h, lambda: len(h),
                lambda: list(h), lambda: h @ torch.zeros(100, 1)):
        with pytest.raises(TypeError, match=r"\.materialize\(\)"):
            use()


def test_materialize_is_the_default(rn):
    assert inspect.signature(rn.fused_joint_logits).parameters["materialize"].default is True
    C = importlib.import_module("ts-asr_amd._capi")
    with pytest.raises(C.TsasrHipMissing):                # the eager call computes: no CPU path
        rn.fused_joint_logits(torch.zeros(1, 2, 64), torch.zeros(1, 3, 64), torch.zeros(100, 64), torch.zeros(100))
    with pytest.raises(C.TsasrHipMissing):                # and so does the loss on a CPU handle
        rn.rnnt_costs(cpu_handle(rn), torch.ones(2, 3, dtype=torch.int32), torch.tensor([7, 5]), torch.tensor([3, 1]), 0)


def test_handle_shapes_are_checked(rn):
    with pytest.raises(ValueError):
        rn.fused_joint_logits(torch.zeros(2, 7, 64), torch.zeros(2, 4, 32), torch.zeros(100, 64), torch.zeros(100), materialize=False)
    with pytest.raises(ValueError):
        rn.fused_joint_logits(torch.zeros(2, 7, 64), torch.zeros(2, 4, 64), torch.zeros(100, 32), torch.zeros(100), materialize=False)


def test_hparams_joint_logits_key():
    hp = importlib.import_module("ts-asr_amd.hparams")
    tiny = dict(d_model=64, nhead=4, encoder_num_layers=1, speaker_num_layers=1, d_ffn=128, joint_dim=64, decoder_neurons=64)

    def load(**over):
        with open(os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml")) as f:
            return hp.load_hyperpyyaml(f, dict(tiny, **over))

    assert "joint_logits" not in load()                    # absent: today's behaviour
    assert load(joint_logits="materialized")["joint_logits"] == "materialized"
    assert load(joint_logits="lazy")["joint_logits"] == "lazy"
    with pytest.raises(ValueError, match="joint_logits.*materialized.*lazy"):
        load(joint_logits="sometimes")
