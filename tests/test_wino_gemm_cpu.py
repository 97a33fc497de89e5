"""The batched-GEMM Winograd route restated in torch fp32 on the CPU: V [16, C, T], U [16, K, C], bmm, output transform, epilogue
(wino_gemm_cases.wg_flow_f32).  It checks the index maps of csrc/conv_winograd_gemm.hip without a GPU, and that the bounds the
kernel tests assert (test_gpu_wino_gemm_bounds.py) are ones this data flow meets: every shape, every input family, the integer
family bit-exact."""
import pytest

import conv_bounds as cb
import wino_gemm_cases as wc


@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_flow_meets_the_bounds(shape, kind):
    x, w, b, bounds = wc.forward_case(shape, kind)
    for epi in ("none", "relu", "mfm"):
        bounds[epi].check(wc.wg_flow_f32(x, w, None if epi == "none" else b, epi))


@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_data_gradient_flow_meets_the_bounds(shape, kind):
    go, w, y, bounds = wc.dgrad_case(shape, kind)
    bounds[False].check(wc.wg_flow_f32(go, w, data_gradient=True))
    bounds[True].check(wc.wg_flow_f32(go, w, data_gradient=True, mask=y))


def test_flow_equals_the_existing_winograd_restatement():
    """Same arithmetic as conv_bounds.winograd_forward_f32 up to the order of the sum over C: integer inputs agree exactly."""
    import torch
    x, w, b, _ = wc.forward_case(wc.SHAPES[0], "integers")
    assert torch.equal(wc.wg_flow_f32(x, w, b, "bias"), cb.winograd_forward_f32(x, w, b))
    go, w, _, _ = wc.dgrad_case(wc.SHAPES[1], "integers")
    assert torch.equal(wc.wg_flow_f32(go, w, data_gradient=True), cb.winograd_dgrad_f32(go, w))
