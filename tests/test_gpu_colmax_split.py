"""ffwm_correlation_colmax_split (csrc/correlation.hip) on the GPU against tests/colmax_split_bounds.py: the float64 bound for every
element, the exact family bit for bit, the non-finite contract, determinism, and the wiring of the precision keyword through
PerceptualCorrectness, checked exactly.  The shapes are the smallest at which the kernel can go wrong: ragged row and column tiles,
two column tiles, N below one column tile, one row past a row tile, every C."""
import pytest
import torch

import colmax_split_bounds as cs
import step_bounds as sb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = ["B%d-N%d-C%d" % s for s in cs.SPLIT_SHAPES]


def split_call(s, t):
    """The C entry on s [B, N, C], t [B, C, N]; out sits in a NaN-prefilled buffer with guard cells behind it."""
    from ffwm_amd import _lib as L
    B, N, C = s.shape
    ds, dt = s.to(DEV).contiguous(), t.to(DEV).contiguous()
    out = sb.guarded_nan(B * N, torch.float32, DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    L.check(L.load().ffwm_correlation_colmax_split(ds.data_ptr(), dt.data_ptr(), out.data_ptr(), B, N, C, L.F32, stream),
            "ffwm_correlation_colmax_split")
    torch.cuda.synchronize()
    return out.cpu()


# ================================================================================================ (a) bound
@pytest.mark.parametrize("family", cs.SPLIT_FAMILIES)
@pytest.mark.parametrize("shape", cs.SPLIT_SHAPES, ids=IDS)
def test_split_colmax_meets_the_bound_everywhere(shape, family):
    s, t = cs.split_inputs(*shape, family=family)
    ck = sb.Checks("colmax split %s %s" % (shape, family))
    cs.SplitRef(s, t).check(ck, split_call(s, t), family=family)
    ck.finish()


# ================================================================================================ (b) exact family
@pytest.mark.parametrize("shape", cs.SPLIT_SHAPES, ids=IDS)
def test_split_colmax_is_the_three_term_value_bit_for_bit(shape):
    _, N, C = shape
    s, t, planted = cs.split_exact_inputs(N, C)
    three, full = cs.split_exact_reference(s, t, planted)
    assert bool((three != full).any())
    out = split_call(s, t)
    sb.check_guards(out, N, "out")
    ck = sb.Checks("colmax split exact N=%d C=%d" % (N, C))
    ck.equal("colmax_split", "exact", out[:N].view(1, N), three.float())
    ck.finish()


# ================================================================================================ (c) non-finite contract
@pytest.mark.parametrize("N,C", [(33, 64), (160, 128)])
@pytest.mark.parametrize("case", cs.NONFINITE_CASES)
def test_split_colmax_nonfinite_contract(case, N, C):
    s, t = cs.split_nonfinite_inputs(case, N, C)
    ck = sb.Checks("colmax split %s N=%d C=%d" % (case, N, C))
    cs.split_nonfinite_check(ck, case, s, t, split_call(s, t))           # the untouched sample keeps its bound
    ck.finish()


# ================================================================================================ (d) determinism
@pytest.mark.parametrize("shape", cs.SPLIT_SHAPES, ids=IDS)
def test_two_calls_agree_bit_for_bit(shape):
    s, t = cs.split_inputs(*shape, seed=3)
    a, b = split_call(s, t), split_call(s, t)
    n = shape[0] * shape[1]
    assert torch.equal(sb.bits(a[:n]), sb.bits(b[:n])) and bool(torch.isfinite(a[:n]).all())


def test_ops_takes_the_split_entry_for_bf16x3():
    """ops.correlation_colmax(precision="bf16x3") is the split entry, bit for bit; the default is the fp32 entry."""
    from ffwm_amd import ops
    s, t = cs.split_inputs(2, 200, 64)
    n = 2 * 200
    got = ops.correlation_colmax(s.to(DEV), t.to(DEV), precision="bf16x3").cpu().reshape(-1)
    assert torch.equal(sb.bits(got), sb.bits(split_call(s, t)[:n]))
    fp32 = ops.correlation_colmax(s.to(DEV), t.to(DEV)).cpu().reshape(-1)
    assert torch.equal(sb.bits(fp32), sb.bits(ops.correlation_colmax(s.to(DEV), t.to(DEV), precision="fp32").cpu().reshape(-1)))
    assert not torch.equal(sb.bits(fp32), sb.bits(got))                  # two kernels, two roundings


# ================================================================================================ (e) wiring, exactly
def _wiring_case():
    gen = torch.Generator().manual_seed(11)
    tgt = (torch.rand(6, 64, 64, 64, generator=gen) + 0.1).to(DEV)
    src = (torch.rand(6, 64, 64, 64, generator=gen) + 0.1).to(DEV)
    flow = (torch.rand(6, 2, 64, 64, generator=gen) * 2.2 - 1.1).to(DEV)
    mask = (torch.rand(6, 1, 64, 64, generator=gen) < 0.6).float().to(DEV)
    return tgt, src, flow, mask


def _by_hand(tgt, src, flow, mask, eps, **kw):
    """What calculate_loss computes on its MFMA + fused branch, from the ops themselves."""
    import torch.nn.functional as F
    from ffwm_amd import ops
    b, c, h, w = tgt.shape
    fl = F.interpolate(flow, [h, w]).contiguous()
    source_all = src.reshape(b, c, -1).transpose(1, 2)
    target_all = tgt.reshape(b, c, -1)
    source_norm = source_all / (source_all.norm(dim=2, keepdim=True) + eps)
    target_norm = target_all / (target_all.norm(dim=1, keepdim=True) + eps)
    corr_max = ops.correlation_colmax(source_norm, target_norm, **kw)
    m = F.interpolate(mask, size=(h, w)).reshape(-1, h * w).to(fl.dtype).contiguous()
    out, grad, _ = ops.sampling_correctness(src.contiguous(), tgt.contiguous(), fl, corr_max.contiguous(), m, eps, want_grad=True)
    return out[0], grad * (1.0 / out[1])


def _through_the_module(tgt, src, flow, mask, **kw):
    from ffwm_amd.external_function import WarpNet
    from ffwm_amd.losses import PerceptualCorrectness
    pc = PerceptualCorrectness(None, WarpNet(), fused=True, **kw)
    pc.target_vgg, pc.source_vgg = {"x": tgt}, {"x": src}
    fl = flow.clone().requires_grad_(True)
    loss = pc.calculate_loss(fl, "x", mask, use_bilinear_sampling=True)
    loss.backward()
    return pc, loss.detach(), fl.grad


def test_perceptual_correctness_hands_the_precision_to_the_kernel(monkeypatch):
    from ffwm_amd import ops
    tgt, src, flow, mask = _wiring_case()
    assert 6 * ((64 * 64 + 127) // 128) >= 192                          # the MFMA branch of calculate_loss
    seen = []
    real = ops.correlation_colmax

    def spy(source, target, *args, **kw):
        seen.append((args, dict(kw)))
        return real(source, target, *args, **kw)
    monkeypatch.setattr(ops, "correlation_colmax", spy)
    pc, loss, grad = _through_the_module(tgt, src, flow, mask, corr_precision="bf16x3")
    assert seen == [((), {"precision": "bf16x3"})], seen
    monkeypatch.setattr(ops, "correlation_colmax", real)
    want_loss, want_grad = _by_hand(tgt, src, flow, mask, pc.eps, precision="bf16x3")
    assert torch.equal(sb.bits(loss.reshape(1)), sb.bits(want_loss.reshape(1)))
    assert torch.equal(sb.bits(grad), sb.bits(want_grad)) and float(grad.abs().max()) > 0
    # fp32 asked: today's result (the call without the keyword), and a different number than the split route's
    pc32, loss32, grad32 = _through_the_module(tgt, src, flow, mask, corr_precision="fp32")
    today_loss, today_grad = _by_hand(tgt, src, flow, mask, pc32.eps)
    assert torch.equal(sb.bits(loss32.reshape(1)), sb.bits(today_loss.reshape(1))) and torch.equal(sb.bits(grad32), sb.bits(today_grad))
    pcd, lossd, gradd = _through_the_module(tgt, src, flow, mask)       # the default
    assert pcd.corr_precision == "fp32" and torch.equal(sb.bits(lossd.reshape(1)), sb.bits(loss32.reshape(1)))
    assert torch.equal(sb.bits(gradd), sb.bits(grad32))
    assert not torch.equal(sb.bits(grad), sb.bits(grad32))
