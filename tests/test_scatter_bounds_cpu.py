"""The per-cell yardstick of tests/scatter_bounds.py, checked on the CPU: the float32 oracle -- the reference's own arithmetic,
float atomics in index order -- meets it with rho / 4 and eta = 0 on every input family, and it rejects an output whose cells
carry the fixed-point noise of a scale taken from another channel or another tile, which the suite's global-max bound accepts."""
import pytest
import torch

import scatter_bounds as sb

FAMILIES_RS = sb.FAMILIES + ("small_sigma",)


def _rs_case(kind, ks=4):
    B, C, H, W = 1, 8, 60, 72
    in2 = sb.rs_small_sigma(B, H, W, 5) if kind == "small_sigma" else sb.rs_flow(B, H, W, 3)
    go = sb.family_grad("signed" if kind == "small_sigma" else kind, (B, C, H, W), 11)
    return (B, C, H, W), in2, go, ks


@pytest.mark.parametrize("ks", [2, 4])
@pytest.mark.parametrize("kind", FAMILIES_RS)
def test_resample2d_reference_meets_the_bound(oracle, kind, ks):
    shape, in2, go, ks = _rs_case(kind, ks)
    bound = sb.resample2d_bound(shape, in2, go, ks)
    got = sb.resample2d_bwd1_oracle(shape, in2.float(), go.float(), ks, dtype=torch.float32)
    rho, _ = sb.rho_eta(torch.float32)
    bound.check(got, rho=rho / 4, eta=0.0, what="fp32 oracle, %s ks %d" % (kind, ks))


def test_resample2d_small_sigma_has_pixels_whose_products_underflow(oracle):
    """(f) reaches what it is for: pixels whose 16 float products all underflow while both per-axis sums stay positive, and the
    float32 replica of the reference's weight sum agrees with the oracle's forward (a pixel with sum 0 samples 0 from ones)."""
    shape, in2, go, ks = _rs_case("small_sigma")
    s = sb.resample2d_weight_sum_f32(in2, ks)
    dead = s == 0
    assert int(dead.sum()) > 100 and int((~dead).sum()) > 100
    ones = torch.ones(1, 1, shape[2], shape[3])
    out = oracle.resample2d_forward(ones, in2.float().contiguous(), ks, 1)[:, 0]
    assert torch.equal(out == 0, dead)


@pytest.mark.parametrize("kind", sb.FAMILIES)
def test_block_extractor_reference_meets_the_bound(oracle, kind):
    B, C, H, W, k = 1, 8, 40, 70, 3
    flow = sb.block_flow(B, H, W, 4)
    go = sb.family_grad(kind, (B, C, k * H, k * W), 12)
    bound = sb.block_extractor_bound((B, C, H, W), flow, go, k)
    got, _ = oracle.block_extractor_backward(torch.zeros(B, C, H, W), flow, go, k)
    rho, _ = sb.rho_eta(torch.float32)
    bound.check(got, rho=rho / 4, eta=0.0, what="fp32 oracle, %s" % kind)


@pytest.mark.parametrize("kind", sb.FAMILIES)
def test_block_attention_reference_meets_the_bound(oracle, kind):
    B, C, H, W, k = 1, 8, 40, 70, 3
    flow = sb.block_flow(B, H, W, 6)
    w = torch.randn(B, k * k, H, W, generator=torch.Generator().manual_seed(7))
    go = sb.family_grad(kind, (B, C, H, W), 13)
    bound = sb.block_attention_bound((B, C, H, W), flow, w, go, k)
    ext = sb.attention_extractor_grad(w, go, k).float()
    got, _ = oracle.block_extractor_backward(torch.zeros(B, C, H, W), flow, ext, k)
    rho, _ = sb.rho_eta(torch.float32)
    bound.check(got, rho=rho / 4, eta=0.0, what="fp32 oracle, %s" % kind)


@pytest.mark.parametrize("kind", sb.FAMILIES)
def test_warp_reference_meets_the_bound(oracle, kind):
    B, C, H, W = 1, 8, 64, 128
    flow = sb.warp_grid(B, H, W, 8)
    go = sb.family_grad(kind, (B, C, H, W), 14)
    bound = sb.warp_bound((B, C, H, W), flow, go)
    got, _ = oracle.warp_backward(torch.zeros(B, C, H, W), flow, go)
    rho, _ = sb.rho_eta(torch.float32)
    bound.check(got, rho=rho / 4, eta=0.0, what="fp32 oracle, %s" % kind)


def _fake_kernel(bound, scale, seed):
    """ref + the rounding noise of a fixed-point cell whose unit is 2^-22 x `scale` (one unit per cell, random sign)."""
    gen = torch.Generator().manual_seed(seed)
    noise = (torch.rand(bound.ref.shape, generator=gen, dtype=torch.float64) * 2 - 1) * scale * 2.0 ** -22
    return (bound.ref + noise).float()


def test_the_bound_rejects_a_scale_from_another_channel(oracle):
    """group_mags: channel 1 (1e-5) scaled as if it were channel 2 (1e3) of its 4-channel group -- what one scale per group does."""
    shape, in2, go, ks = _rs_case("group_mags")
    bound = sb.resample2d_bound(shape, in2, go, ks)
    fake = bound.ref.float().clone()
    wrong = _fake_kernel(bound, float(go[:, 2].abs().max()), 21)
    fake[:, 1] = wrong[:, 1]
    assert sb.global_close(fake, bound.ref, 1e-5)                  # today's bound: tol (1 + max|ref|) lets it through
    ratio, _ = bound.ratio(fake)
    assert ratio > 100, ratio
    fair = _fake_kernel(bound, float(go[:, 1].abs().max()), 22)     # the channel's own scale: accepted
    fake[:, 1] = fair[:, 1]
    assert bound.ratio(fake)[0] <= 1.0


def test_the_bound_rejects_a_scale_from_another_tile(oracle):
    """masked: the zero region's cells rounded to the unit of a tile of the log-normal part (the largest gradient elsewhere)."""
    B, C, H, W, k = 1, 2, 256, 384, 3                # the zero region (128 x 192 pixels) is wider than the reach R
    flow = sb.block_flow(B, H, W, 9)
    go = sb.family_grad("masked", (B, C, k * H, k * W), 15)
    bound = sb.block_extractor_bound((B, C, H, W), flow, go, k)
    fake = _fake_kernel(bound, float(go.abs().max()), 23)
    assert sb.global_close(fake, bound.ref, 1e-5)
    assert bound.ratio(fake)[0] > 100
    # the same noise confined to the cells whose own neighbourhood holds that gradient is accepted
    near = bound.L >= float(go.abs().max()) / 2
    assert bound.ratio(torch.where(near, fake, bound.ref.float()))[0] <= 1.0
