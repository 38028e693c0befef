"""GPU: the T = 1 branch of process_output_2d -- the Softmax model's step -- reduces its B images with ONE batched
1 - max softmax call, bit-equal to calculate_one_minus_msr per image."""
import numpy as np
import pytest
import torch

from tests.formula import formula_tensor

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [3, 1])
def test_one_prediction_step_is_one_batched_call(monkeypatch, B):
    from values_amd import uncertainty
    from values_amd.predict2d import process_output_2d
    from values_amd.uncertainty import calculate_one_minus_msr
    C, H, W = 19, 5, 7
    z = formula_tensor((B, 1, C, H, W), 77 + B, scale=4.0)
    e = np.exp(z - z.max(axis=2, keepdims=True))
    probs = torch.from_numpy((e / e.sum(axis=2, keepdims=True)).astype(np.float32)).cuda()
    calls = []
    real = uncertainty.one_minus_msr_batch
    monkeypatch.setattr(uncertainty, "one_minus_msr_batch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = process_output_2d(None, probs=probs)
    assert len(calls) == 1
    pe = out["pred_entropy"]
    assert pe.shape == (B, H, W) and pe.dtype == torch.float32 and pe.is_contiguous()
    assert "aleatoric_uncertainty" not in out
    for b in range(B):
        want = calculate_one_minus_msr(probs[b, 0])["pred_entropy"]
        assert torch.equal(pe[b].view(torch.int32), want.view(torch.int32)), b
        assert (pe[b].cpu().numpy() == 1 - probs[b, 0].cpu().numpy().max(0)).all()
