"""tests/conv_bounds.py judged without a GPU: fp32 stand-ins of the kernels' arithmetic (ATen's fp32 CPU convolutions, a torch
emulation of Winograd F(2x2, 3x3), a chunked sum in reversed order) meet the per-element bounds with rho / 4 on every family and
the integer family bit for bit; the yardstick rejects by > 100 x what the old global tolerance accepts; the integer guard raises."""
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb

B, C, K, H, W = 2, 67, 22, 10, 12          # 67 = 64 + 3: a thin remainder; 22 output channels: scales differ inside a chunk


def _case(kind, seed=0, C=C, K=K, H=H, W=W):
    x = cb.activations(kind, (B, C, H, W), 100 + seed)
    w, b = cb.weights(kind, (K, C, 3, 3), 200 + seed)
    return x, w, b


@pytest.mark.parametrize("kind", cb.FAMILIES)
def test_aten_fp32_forward_and_data_gradient_meet_the_bound(kind):
    x, w, b = _case(kind)
    exact = kind == "integers"
    act = "relu" if exact else "lrelu"
    bound = cb.forward_bound(x, w, b, 1, 1, 0, act, 0.2, cb.rho_conv_fwd(C, 9), exact=exact, what="aten fwd " + kind)
    bound.check(F.leaky_relu(F.conv2d(x, w, b, 1, 1), 0.0 if exact else 0.2), rho=bound.rho / 4)
    go = cb.grad_outputs(kind, (B, K, H, W), 300)
    dbound = cb.forward_bound(go, w, None, 1, 1, 3, rho=cb.rho_conv_fwd(K, 9), exact=exact, what="aten dgrad " + kind)
    dbound.check(torch.nn.grad.conv2d_input((B, C, H, W), w, go, 1, 1), rho=dbound.rho / 4)
    # stride 2: Conv2d(3, 2, 1), its data gradient (mode 2) and ConvTranspose2d(4, 2, 1) (mode 1)
    s2 = cb.forward_bound(x, w, b, 2, 1, 0, None, 0.2, cb.rho_conv_fwd(C, 9), exact=exact, what="aten s2 " + kind)
    s2.check(F.conv2d(x, w, b, 2, 1), rho=s2.rho / 4)
    g2 = cb.grad_outputs(kind, (B, K, H // 2, W // 2), 301)
    m2 = cb.forward_bound(g2, w, None, 2, 1, 2, rho=cb.rho_conv_fwd(K, 4), exact=exact, what="aten mode 2 " + kind)
    m2.check(torch.nn.grad.conv2d_input((B, C, H, W), w, g2, 2, 1), rho=m2.rho / 4)
    wt, bt = cb.weights(kind, (C, K, 4, 4), 201, out_dim=1)
    m1 = cb.forward_bound(x, wt, bt, 2, 1, 1, None, 0.2, cb.rho_conv_fwd(C, 4), exact=exact, what="aten mode 1 " + kind)
    m1.check(F.conv_transpose2d(x, wt, bt, 2, 1), rho=m1.rho / 4)


@pytest.mark.parametrize("kind", cb.FAMILIES)
def test_aten_fp32_weight_gradient_meets_the_bound(kind):
    x = cb.activations(kind, (B, C, H, W), 110)
    go = cb.grad_outputs(kind, (B, K, H, W), 310)
    exact = kind == "integers"
    n = B * H * W
    wb, bb = cb.wgrad_bounds(x, go, 3, 1, 1, rho=cb.rho_any_order(n), exact=exact, what="aten wgrad " + kind)
    _, gw, gb = torch.ops.aten.convolution_backward(go, x, torch.zeros(K, C, 3, 3), [K], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, True])
    wb.check(gw, rho=wb.rho / 4)
    bb.check(gb, rho=bb.rho / 4)


@pytest.mark.parametrize("kind", cb.FAMILIES)
def test_winograd_emulation_meets_the_bound(kind):
    """fp32 F(2x2, 3x3) in torch -- forward, data gradient and the Winograd-domain weight gradient -- against mag_patch."""
    x, w, b = _case(kind, 1)
    exact = kind == "integers"
    fb = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, cb.rho_winograd(C), winograd=True, exact=exact, what="wino fwd " + kind)
    fb.check(cb.winograd_forward_f32(x, w, b), rho=fb.rho / 4)
    go = cb.grad_outputs(kind, (B, K, H, W), 320)
    db = cb.forward_bound(go, w, None, 1, 1, 3, rho=cb.rho_winograd(K), winograd=True, exact=exact, what="wino dgrad " + kind)
    db.check(cb.winograd_dgrad_f32(go, w), rho=db.rho / 4)
    tiles = B * (H // 2) * (W // 2)
    wb, _ = cb.wgrad_bounds(x, go, 3, 1, 1, rho=cb.SAFETY * 16 * (tiles + 10) * cb.U32, winograd=True, exact=exact, what="wino wgrad " + kind)
    wb.check(cb.winograd_wgrad_f32(x, go), rho=wb.rho / 4)


def test_winograd_emulation_in_float64_is_the_convolution():
    x, w, b = _case("iid", 2)
    ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    assert (cb.winograd_forward_f32(x.double(), w.double(), b.double()) - ref).abs().max() < 1e-12
    go = cb.grad_outputs("iid", (B, K, H, W), 5).double()
    dref = torch.nn.grad.conv2d_input((B, C, H, W), w.double(), go, 1, 1)
    assert (cb.winograd_dgrad_f32(go, w.double()) - dref).abs().max() < 1e-12
    wref = cb.wgrad_bounds(x, go, 3, 1, 1, rho=1.0)[0].ref
    assert (cb.winograd_wgrad_f32(x.double(), go) - wref).abs().max() < 1e-11


@pytest.mark.parametrize("kind", cb.FAMILIES)
def test_chunked_sum_in_reversed_order_meets_the_bound(kind):
    """The reduction cut into 8-channel chunks added last chunk first (a split launch whose slices meet in another order)."""
    x, w, b = _case(kind, 3)
    exact = kind == "integers"
    acc = torch.zeros(B, K, H, W)
    chunks = list(range(0, C, 8))
    for c0 in reversed(chunks):
        acc = acc + F.conv2d(x[:, c0:c0 + 8], w[:, c0:c0 + 8], None, 1, 1)
    bound = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, cb.rho_conv_fwd(C, 9, len(chunks)), exact=exact, what="chunked " + kind)
    bound.check(acc + b.view(1, -1, 1, 1), rho=bound.rho / 4)


# ------------------------------------------------------------------------------------------------ what the old yardstick accepts
def _rejects(bound, got, tol=2e-5):
    assert cb.global_close(got, bound.ref, tol), "the old global tolerance was expected to accept this"
    ratio, wrong, idx = bound.measure(got)
    assert ratio > 100, (ratio, idx)
    return idx


def test_rejects_a_zeroed_small_scale_output_channel():
    x, w, b = _case("out_scales")
    bound = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, cb.rho_conv_fwd(C, 9))
    k = int(cb.channel_exponents(K).argmin())
    got = bound.ref.float()
    got[:, k] = 0
    assert _rejects(bound, got)[1] == k


def test_rejects_a_lost_tap_on_the_border_row_of_a_small_scale_channel():
    x, w, b = _case("out_scales")
    bound = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, cb.rho_conv_fwd(C, 9))
    k = int(cb.channel_exponents(K).argmin())
    w2 = w.clone()
    w2[k, :, 2, 1] = 0                                        # the tap below the pixel, lost on the first row only
    got = bound.ref.float()
    got[:, k, 0] = F.conv2d(x.double(), w2.double(), b.double(), 1, 1)[:, k, 0].float()
    idx = _rejects(bound, got)
    assert idx[1] == k and idx[2] == 0


def test_rejects_a_bias_lost_on_the_ragged_last_tile():
    Kr = 70                                                   # channels 64..69: the ragged last 64-tile
    x = cb.activations("iid", (B, 16, H, W), 120)
    w, b = cb.weights("iid", (Kr, 16, 3, 3), 220)
    s = torch.ones(Kr)
    s[64:] = 2.0 ** -10
    w, b = w * s.view(-1, 1, 1, 1) * 4, b * s
    w[:64] *= 64
    bound = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, cb.rho_conv_fwd(16, 9))
    got = bound.ref.float()
    got[:, 64:] -= b[64:].view(1, -1, 1, 1)
    assert _rejects(bound, got)[1] >= 64


@pytest.mark.parametrize("winograd", [False, True])
def test_rejects_a_spike_rounding_noise_leaked_into_the_neighbouring_tile(winograd):
    Cs = 8
    x = cb.activations("spike", (B, Cs, 16, 16), 130)
    w, b = cb.weights("iid", (K, Cs, 3, 3), 230)
    b = b * 1e-3
    rho = cb.rho_winograd(Cs) if winograd else cb.rho_conv_fwd(Cs, 9)
    bound = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, rho, winograd=winograd)
    sy, sx = 8, 7                                             # activations(): the spike at (H // 2, W // 2 - 1)
    amp = float(x[:, :, sy, sx].abs().max())
    assert amp == 1e4
    got = bound.ref.float()
    # one rounding of the spike's product (|w| ~ 0.1; the Winograd input transform carries 4 x the spike), two tiles to the right:
    # outside the 4 x 4 patch of the spike's tile
    got[:, :, sy, sx + 5] += amp * cb.U32 * (0.4 if winograd else 0.1)
    idx = _rejects(bound, got)
    assert idx[2:] == (sy, sx + 5)


def test_rejects_an_unrotated_weight_in_one_parity_class():
    go = cb.grad_outputs("integers", (B, K, H, W), 340)
    w, _ = cb.weights("integers", (K, C, 3, 3), 240)
    bound = cb.forward_bound(go, w, None, 1, 1, 3, rho=cb.rho_conv_fwd(K, 9), exact=True)
    got = bound.ref.float()
    bound.check(got)
    wrong = torch.nn.grad.conv2d_input((B, C, H, W), w.flip(2, 3).double(), go.double(), 1, 1).float()
    got[:, :, 1::2, 0::2] = wrong[:, :, 1::2, 0::2]
    with pytest.raises(AssertionError):
        bound.check(got)
    assert not torch.equal(got, bound.ref.float())
    # and on real-valued inputs the same mistake fails the bound by orders of magnitude
    go = cb.grad_outputs("iid", (B, K, H, W), 341)
    w, _ = cb.weights("iid", (K, C, 3, 3), 241)
    bound = cb.forward_bound(go, w, None, 1, 1, 3, rho=cb.rho_conv_fwd(K, 9))
    got = bound.ref.float()
    got[:, :, 1::2, 0::2] = torch.nn.grad.conv2d_input((B, C, H, W), w.flip(2, 3).double(), go.double(), 1, 1).float()[:, :, 1::2, 0::2]
    assert bound.measure(got)[0] > 100


def test_non_finite_elements_must_sit_where_the_reference_has_them():
    x, w, b = _case("nonfinite")
    bound = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, cb.rho_conv_fwd(C, 9))
    got = bound.ref.float()
    assert bound.measure(got)[1] == 0
    got2 = got.clone()
    got2[0, 0, 0, 0] = float("nan")                           # far from both pixels
    assert bound.measure(got2)[1] == 1
    got3 = torch.nan_to_num(got, nan=0.0, posinf=0.0, neginf=0.0)
    assert bound.measure(got3)[1] > 0
    # the Winograd yardstick frees the rest of the 4 x 4 patch's tiles, nothing else
    wb = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.2, cb.rho_winograd(C), winograd=True)
    free = torch.isfinite(wb.ref) & ~torch.isfinite(wb.mag)
    assert 0 < int(free[0, 0].sum()) <= 16 and bool(torch.isfinite(wb.mag[0, 0, 0, 0]))
    ratio, wrong, _ = wb.measure(cb.winograd_forward_f32(x, w, b), wb.rho / 4)
    assert wrong == 0 and ratio <= 1


def test_integer_guard_raises_on_a_case_that_is_too_large():
    x = cb.activations("integers", (16, 8, 64, 64), 1)
    go = cb.grad_outputs("integers", (16, 8, 64, 64), 2)
    with pytest.raises(ValueError):
        cb.wgrad_bounds(x, go, 3, 1, 1, rho=1.0, winograd=True, exact=True)          # -3..3 over 16384 tiles: 64 mag_patch >= 2^24
    xs, gs = cb.activations("integers", (16, 8, 64, 64), 1, small=True), cb.grad_outputs("integers", (16, 8, 64, 64), 2, small=True)
    cb.wgrad_bounds(xs, gs, 3, 1, 1, rho=1.0, winograd=True, exact=True)             # -1..1 is well-formed
    with pytest.raises(ValueError):
        cb.require_exact(torch.tensor([2.0 ** 24]))


def test_structure_formulas_follow_the_launch_code():
    """Spot values of the (chain, partial sums) mirrors, computed by hand from the launch code."""
    assert cb.wgrad3x3_structure(8, 192, 192, 128, 128) == (64 * 74, 28)          # 9 tiles -> 28 slices of ceil(2048 / 28) = 74 row steps
    assert cb.wgrad_wino_structure(8, 64, 64, 64, 64) == (8 * 16, 64)             # 1024 chunks, 1 tile: 64 slices of 16 chunks
    assert cb.rho_conv_fwd(1026, 9, 8) == cb.SAFETY * (1026 * 9 + 8 + 1) * cb.U32
