"""tests/small_kernel_bounds.py judged without a GPU.  Every bound and every input family of tests/test_gpu_small_kernel_bounds.py is
met by an fp32 torch stand-in on the CPU with rho / SAFETY (the exact kernels: bit for bit) -- ATen's fp32 CPU composition, a
sequential fp32 restatement of the affine gradient, chain-ordered fp32 restatements of the two backward convolutions -- so the bounds
and the inputs are satisfiable by the reference alone; no case excludes an element other than those a non-finite input reaches
(Bound.measure excludes nothing else).  Seven mutants, each the restatement of a real slip, miss their bound.  The route rules resolve
every GPU shape to the route its test names, and the C entry points answer bad arguments before any launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import small_kernel_bounds as sk


# ------------------------------------------------------------------------------------------------ routes
def test_flow_head_shapes_reach_every_tile_width():
    tiles = sk.flow_head_tiles(sk.FLOW_HEAD_SHAPES)
    assert set(tiles.values()) == {4, 16, 64}
    assert tiles[(6, 128, 16, 16)] == 16 and tiles[(4, 70, 19, 23)] == 16 and (19 * 23) % 16 != 0          # the second ends in a partial tile
    assert tiles[(8, 256, 8, 8)] == 4 and tiles[(8, 1024, 2, 2)] == 4 and tiles[(8, 32, 64, 64)] == 64
    assert sk.flow_head_tile(8, 256) == 16                                                                  # the training batch at 16 x 16
    assert set(sk.flow_head_tiles(sk.FLOW_HEAD_BWD_SHAPES).values()) == {4, 16, 64}
    import test_gpu_conv_bounds as g
    assert set(sk.flow_head_tiles(g.FLOW_HEADS).values()) == {4, 16, 64} and set(g.FLOW_HEADS) == set(sk.FLOW_HEAD_SHAPES)


def test_element_wise_shapes_resolve_to_the_routes_their_tests_name():
    g = sk
    for shape, offset, route, past in g.MFM_SHAPES:
        assert sk.mfm_route(shape, offset)[::2] == (route, past), shape
        assert sk.bias_relu_route((shape[0], shape[1] // 2) + tuple(shape[2:]), offset)[0] == route
    assert sk.mfm_route((1, 66, 255, 257))[1] > 2097152 and sk.mfm_route((1, 130, 256, 512))[1] * 4 > 8388608
    for shape, offset, route, past in g.RELU_SHAPES:
        assert sk.bias_relu_route(shape, offset)[::2] == (route, past), shape
    for n_shape in sk.RESIDUAL_SIZES:
        n = int(torch.Size(n_shape).numel())
        n4, tail, past = sk.residual_route(n)
        assert (tail, past) == g.RESIDUAL_EXPECT[n_shape], (n_shape, tail, past)
    assert {sk.residual_route(int(torch.Size(s).numel()))[1] for s in sk.RESIDUAL_SIZES} == {0, 1, 2, 3}
    for shape, route in g.GATE_STRIDED_SHAPES:
        stride = (shape[1] + 5) * shape[2] * shape[3]
        assert sk.gate_strided_route(shape, stride, 2 * shape[2] * shape[3])[::2] == (route, True), shape
    for name, case in g.BIAS_ACT_CASES.items():
        assert sk.bias_act_case_route(name)[::2] == case[4:], name
    assert {c[4:] for c in g.BIAS_ACT_CASES.values()} == {("vector", False), ("scalar", False), ("vector", True), ("scalar", True)}
    # tests/test_gpu_frontalizer.py: one shape per route past 524 288 threads, each into a guarded view (2 channels before, 3 after)
    for h_shape, route in (((1, 132, 256, 256), "vector"), ((1, 36, 241, 243), "scalar")):
        B, C4, H, W = h_shape
        assert sk.shuffle_route(h_shape, (C4 // 4 + 5) * 4 * H * W, 2 * 4 * H * W) == (route, sk.shuffle_route(h_shape, 0)[1], True)
        assert sk.shuffle_route(h_shape, 0)[1] > 524288
    for x_shape, route in (((1, 3, 512, 360), "vector"), ((1, 3, 211, 209), "scalar")):
        B, C, H, W = x_shape
        r = sk.upsample_route(x_shape, (C + 5) * 4 * H * W, 2 * 4 * H * W)
        assert r[0] == route and r[1] > 524288 and r[2]
    # below the caps: the shapes the older tests use fit one sweep
    assert not sk.mfm_route((8, 192, 32, 32))[2] and not sk.residual_route(2 * 3 * 4 * 6)[2]


# ------------------------------------------------------------------------------------------------ exact kernels: the reference and its mutants
def _mfm_standin(x, bias, go, maximum=torch.max, tie_full=False):
    """The kernel's formulas in fp32 torch: y = max(a, b), dx = g [a > b] + g/2 [a == b] (mfm.hip mfm_grad)."""
    C = x.shape[1] // 2
    h = x if bias is None else x + bias.view(1, -1, 1, 1)
    a, b = h[:, :C], h[:, C:]
    y = maximum(a, b)
    hg = torch.where(a == b, go if tie_full else 0.5 * go, go)
    da = torch.where(a < b, torch.zeros_like(go), hg)
    db = torch.where(b < a, torch.zeros_like(go), hg)
    return y, torch.cat((da, db), 1)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("kind", sk.MFM_KINDS)
@pytest.mark.parametrize("shape", [(3, 10, 7, 9), (2, 6, 2, 2)])
def test_mfm_formulas_equal_the_reference_bit_for_bit(shape, kind, with_bias):
    x, bias, go = sk.mfm_inputs(kind, shape, 11, with_bias)
    y_ref, dx_ref, _ = sk.mfm_reference(x, bias, go)
    y, dx = _mfm_standin(x, bias, go)
    sk.assert_same(y, y_ref, "mfm y")
    sk.assert_same(dx, dx_ref, "mfm dx")
    if kind in sk.MFM_NONFINITE and (with_bias or kind != "nan_by_bias"):
        assert not bool(torch.isfinite(y_ref).all())
    if kind in ("ties", "bias_ties"):
        C = shape[1] // 2
        h = x if bias is None else x + bias.view(1, -1, 1, 1)
        assert int((h[:, :C] == h[:, C:]).sum()) >= y.numel() // 4


def test_mutant_maximum_that_drops_nan_misses():
    for kind in ("nan_first", "nan_second", "nan_both", "nan_by_bias"):
        x, bias, go = sk.mfm_inputs(kind, (3, 10, 7, 9), 11, True)
        y_ref, _, _ = sk.mfm_reference(x, bias, go)
        y, _ = _mfm_standin(x, bias, go, maximum=torch.fmax)
        with pytest.raises(AssertionError, match="NaN positions"):
            sk.assert_same(y, y_ref, kind)
    h, bias, go = sk.relu_inputs("nan", (2, 5, 7, 9), 12)
    with pytest.raises(AssertionError, match="NaN positions"):
        sk.assert_same(torch.fmax(h + bias.view(1, -1, 1, 1), torch.zeros(())), sk.relu_reference(h, bias, go)[0], "relu")


def test_mutant_tie_with_the_full_gradient_on_both_halves_misses():
    for kind in ("ties", "bias_ties"):
        x, bias, go = sk.mfm_inputs(kind, (3, 10, 7, 9), 11, True)
        _, dx_ref, _ = sk.mfm_reference(x, bias, go)
        _, dx = _mfm_standin(x, bias, go, tie_full=True)
        with pytest.raises(AssertionError, match="differ"):
            sk.assert_same(dx, dx_ref, kind)


@pytest.mark.parametrize("kind", sk.RELU_KINDS)
def test_bias_relu_reference_families(kind):
    h, bias, go = sk.relu_inputs(kind, (2, 5, 7, 9), 12)
    y_ref, dh_ref, _ = sk.relu_reference(h, bias, go)
    z = h + bias.view(1, -1, 1, 1)
    y = torch.where(z != z, z, torch.clamp_min(z, 0))
    sk.assert_same(y, y_ref, "relu y")
    sk.assert_same(torch.ops.aten.threshold_backward(go, y, 0), dh_ref, "relu dh")          # BiasReLUFunction.backward, from y
    if kind in sk.RELU_NONFINITE:
        assert bool(torch.isnan(y_ref).any()) or kind == "inf"
        assert not bool(torch.isfinite(y_ref).all())


def test_mutant_sweep_that_stops_at_the_cap_misses():
    """A grid-stride loop without its stride covers one sweep of the capped grid: the rest of a NaN-filled destination stays NaN."""
    shape = (1, 33, 256, 256)
    n = int(torch.Size(shape).numel())
    n4, tail, past = sk.residual_route(n)
    assert past
    a, b = sk.sweep_z(n, 3)
    a, b = a.clamp(-50, 50).nan_to_num(0.0), b.nan_to_num(0.0).clamp(-50, 50)
    ref = F.leaky_relu(a + b, 0.2)
    got = torch.full_like(ref, float("nan"))
    covered = 4 * 2048 * sk.KBLOCK
    got[:covered] = ref[:covered]
    with pytest.raises(AssertionError, match="NaN positions"):
        sk.assert_same(got, ref, "one sweep")


# ------------------------------------------------------------------------------------------------ sigmoid and the products behind it
def test_sigmoid_yardstick_on_aten_cpu_and_its_mutant():
    a, b = sk.sweep_z(40000, 5)
    aten = torch.sigmoid(a + b)
    e_got, e_aten = sk.check_sigmoid(aten, aten, a, b, "ATen CPU against itself")
    assert e_got == e_aten and e_aten < 8.0            # a + b is exact: what is left is expf and the division
    z = a + b
    assert bool(((z > 87) & torch.isfinite(z)).any()) and bool((z < -87).any()) and bool(torch.isnan(z).any()) and bool(torch.isinf(z).any())
    # saturated for certain once exp(|z|) has overflowed (|z| >= 89); between 87 and 88.7 the negative side is still a subnormal
    vals = set(aten[(z.abs() >= 89) & ~torch.isnan(z)].tolist())
    assert vals == {0.0, 1.0}, vals
    i = int(((a == -20.0) & (b == 0.0)).nonzero()[0])
    bad = aten.clone()
    bad[i] = bad[i] * (1 + 2.0 ** -10)
    assert abs(float(bad[i]) - 2.06e-9) < 1e-10          # an absolute 2e-7 tolerance cannot see it
    with pytest.raises(AssertionError, match="worst relative error"):
        sk.check_sigmoid(bad, aten, a, b, "wrong by 2^-10 at z = -20")


def test_gate_products_meet_their_bounds_in_fp32():
    n = 40000
    a, b = sk.sweep_z(n, 6)
    x, g = sk.mixed_scale(n, 7), sk.mixed_scale(n, 8)
    att = torch.sigmoid(a + b)
    sk.check_product(x * att, x.double() * att.double(), 1, "y = x att")
    dz_ref, dx_ref = sk.gate_backward_refs(x, att, g)
    sk.check_product(((g * x) * (1 - att)) * att, dz_ref, 4, "gate dz")
    sk.check_product(g * att, dx_ref, 1, "gate dx")
    sk.check_product((g * (1 - att)) * att, sk.sigmoid_backward_ref(att, g), 3, "sigmoid dz")
    with pytest.raises(AssertionError):
        sk.check_product((g * x) * ((1 - att) * att) * (1 + 2.0 ** -20), dz_ref, 4, "a dz off by 16 u")


def test_leaky_relu_kink_inputs():
    a, b = sk.sweep_z(4000, 9)
    go = sk.mixed_scale(4000, 10)
    y, dz = sk.leaky_reference(a, b, go, 0.2)
    z = a + b
    for v in (0.0, sk.SMALLEST_NORMAL, -sk.SMALLEST_NORMAL):
        assert bool((z == v).any())
    # add_act_bwd_kernel reads the sign of y, ATen that of z: the same selection on every finite input, the kink included
    fin = ~torch.isnan(z)
    sk.assert_same(torch.where(y > 0, go, go * 0.2)[fin], dz[fin], "backward from y")


# ------------------------------------------------------------------------------------------------ bias_act
@pytest.mark.parametrize("act", [0, 1, 2])
def test_bias_act_reference(act):
    h = sk.activations("iid", (2, 5, 7, 9), 13) * 3
    bias = torch.randn(5, generator=torch.Generator().manual_seed(14))
    ref = sk.bias_act_reference(h, bias, act)
    pre = h + bias.view(1, -1, 1, 1)
    if act == 2:
        ref.check(torch.tanh(pre), "tanh stand-in")
        with pytest.raises(AssertionError):
            ref.check(torch.tanh(pre) * (1 + 2.0 ** -20), "tanh off by 16 ulps")
    else:
        assert torch.equal(ref, pre if act == 0 else torch.where(pre > 0, pre, pre * 0.2))
    assert torch.equal(sk.bias_act_reference(h, None, 0), h)


# ------------------------------------------------------------------------------------------------ flow head / upsampler backward
HEAD_CPU_SHAPES = [(3, 70, 9, 11), (4, 70, 19, 23), (8, 1024, 2, 2)]


def _head_case(shape, kind, ykind):
    B, C, H, W = shape
    go = sk.grad_outputs(kind, (B, 2, H, W), 40 + C)
    w, _ = sk.weights(kind, (2, C, 3, 3), 41 + C)
    y = sk.head_outputs("zero" if kind == "integers" else ykind, (B, 2, H, W), 42 + C)
    return y, go, w


@pytest.mark.parametrize("ykind", sk.HEAD_Y_KINDS)
@pytest.mark.parametrize("kind", sk.cb.FAMILIES)
@pytest.mark.parametrize("shape", HEAD_CPU_SHAPES[:2])
def test_flow_head_backward_standin_meets_the_bound_without_the_safety_factor(shape, kind, ykind):
    if kind == "integers" and ykind != "moderate":
        return
    y, go, w = _head_case(shape, kind, ykind)
    zb, xb = sk.flow_head_backward_bounds(y, go, w, exact=kind == "integers", safety=1.0, what="head bwd %s %s %s" % (shape, kind, ykind))
    gz, gx = sk.flow_head_backward_f32(y, go, w)
    zb.check(gz)
    xb.check(gx)
    if ykind == "ones":
        fin = torch.isfinite(go)
        assert bool((gz[fin] == 0).all())


@pytest.mark.parametrize("flipped,masked", [(False, True), (True, False)])
def test_mutant_flow_head_backward_misses(flipped, masked):
    """Un-flipped taps, and neighbours read across the border instead of masked: on the spike family -- large gradients on border
    pixels in a small-gradient plane, where max|d| <= 1e-5 (1 + max|ref|) sees nothing of the plane's other pixels."""
    for shape in HEAD_CPU_SHAPES:
        y, go, w = _head_case(shape, "iid", "moderate")
        _, xb = sk.flow_head_backward_bounds(y, go, w, what="mutant")
        gz, gx = sk.flow_head_backward_f32(y, go, w, flipped=flipped, masked=masked)
        ratio, _, _ = xb.measure(gx)
        assert ratio > 1.0, (shape, ratio)
    y, go, w = _head_case((3, 70, 9, 11), "iid", "moderate")
    go = go * 1e-4
    go[0, 0, 4, 5] = 50.0                                     # one large interior gradient: the old whole-tensor yardstick's scale
    _, xb = sk.flow_head_backward_bounds(y, go, w, what="mutant")
    _, gx = sk.flow_head_backward_f32(y, go, w, flipped=True, masked=masked)
    if not masked:                                            # the border slip hides below 1e-5 (1 + max|ref|) and not below the bound
        assert sk.cb.global_close(gx, xb.ref, 1e-5) and xb.measure(gx)[0] > 1.0


@pytest.mark.parametrize("kind", sk.cb.FAMILIES)
@pytest.mark.parametrize("shape", [(8, 2, 2), (3, 7, 9), (8, 16, 16), (1, 1, 1)])
def test_flow_up_backward_standin_meets_the_bound_without_the_safety_factor(shape, kind):
    B, H, W = shape
    go = sk.grad_outputs(kind, (B, 2, 2 * H, 2 * W), 50 + H)
    w, _ = sk.weights(kind, (2, 2, 4, 4), 51 + H, out_dim=1)
    bound = sk.flow_up_backward_bound(go, w, exact=kind == "integers", safety=1.0, what="flow_up bwd %s %s" % (shape, kind))
    bound.check(sk.flow_up_backward_f32(go, w))


# ------------------------------------------------------------------------------------------------ affine regulariser
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", sk.AFFINE_FLOWS)
@pytest.mark.parametrize("shape", sk.AFFINE_SHAPES)
def test_affine_sequential_standin_meets_the_bounds_without_the_safety_factor(shape, kind, dtype):
    B, h, w, kz = shape
    flow = sk.affine_flow(kind, B, h, w, 60 + h).to(dtype)
    M = sk.affine_matrix(kz)
    lb, gb = sk.affine_bounds(flow, M, kz, dtype, safety=1.0, what="affine %s %s" % (shape, kind))
    loss, grad = sk.affine_f32(flow, M, kz)
    gb.check(grad)
    lb.check(loss)
    if kind == "nan_cell":
        nan = torch.isnan(grad)
        yy, xx = h // 2, w - 2
        expect = torch.zeros_like(nan)
        expect[B - 1, 1, max(yy - kz + 1, 0):yy + kz, max(xx - kz + 1, 0):xx + kz] = True
        assert torch.equal(nan, expect) and bool(torch.isnan(loss))
    else:
        assert bool(torch.isfinite(grad).all())


def test_affine_shapes_hold_a_single_window_and_one_window_tiles():
    for (B, h, w, kz), (cols_last, rows_last) in zip(sk.AFFINE_SHAPES, [(1, 1), (1, None), (1, 1), (None, None), (None, None)]):
        hw, ww = h - kz + 1, w - kz + 1
        if cols_last is not None:
            assert ww % sk.AR_TILE_X == cols_last, (h, w, kz)
        if rows_last is not None:
            assert hw % sk.AR_TILE_Y == rows_last, (h, w, kz)
    assert sk.AFFINE_SHAPES[0][1] == sk.AFFINE_SHAPES[0][3]


def test_mutant_affine_gradient_missing_a_seam_window_column_misses():
    B, h, w, kz = 2, 6, 67, 3
    M = sk.affine_matrix(kz)
    for kind in ("uniform", "extremes"):
        flow = sk.affine_flow(kind, B, h, w, 66)
        _, gb = sk.affine_bounds(flow, M, kz, what="mutant")
        for col in (sk.AR_TILE_X - 1, sk.AR_TILE_X):               # the last window column of the first tile, the only one of the second
            _, grad = sk.affine_f32(flow, M, kz, skip_window_column=col)
            assert gb.measure(grad)[0] > 1.0


# ------------------------------------------------------------------------------------------------ argument errors, before any launch
@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


def _aligned_buffer(n=64):
    raw = (ctypes.c_float * (n + 8))()
    base = ctypes.addressof(raw)
    skip = (-base) % 16
    return raw, base + skip


def test_residual_entries_refuse_misaligned_pointers(hiplib):
    raw, p = _aligned_buffer()
    for bad in ((p + 4, p, p), (p, p + 4, p), (p, p, p + 8)):
        assert hiplib.ffwm_add_act_forward(*bad, 16, 1, 0.2, 0, None) == -1 and b"16-byte aligned" in hiplib.ffwm_last_error()
        assert hiplib.ffwm_add_act_backward(*bad, 16, 3, 0.0, 0, None) == -1 and b"16-byte aligned" in hiplib.ffwm_last_error()
    assert hiplib.ffwm_sigmoid_gate_forward(p, p, p, p + 4, p, 16, 0, None) == -1 and b"16-byte aligned" in hiplib.ffwm_last_error()
    assert hiplib.ffwm_sigmoid_gate_backward(p, p, p, p, p + 12, 16, 0, None) == -1 and b"16-byte aligned" in hiplib.ffwm_last_error()


def test_act_out_of_range_and_short_strides_are_refused(hiplib):
    raw, p = _aligned_buffer()
    for act in (0, 2, 4, -1):
        assert hiplib.ffwm_add_act_forward(p, p, p, 16, act, 0.2, 0, None) == -1 and b"act must be" in hiplib.ffwm_last_error()
        assert hiplib.ffwm_add_act_backward(p, p, p, 16, act, 0.2, 0, None) == -1 and b"act must be" in hiplib.ffwm_last_error()
    assert hiplib.ffwm_add_act_forward(p, p, p, 16, 1, 0.0, 0, None) == -1 and b"negative_slope" in hiplib.ffwm_last_error()
    for act in (3, -1):
        assert hiplib.ffwm_bias_act_forward(p, None, p, None, 1, 2, 8, 16, 0, act, 0.2, 0, None) == -1 and b"activation" in hiplib.ffwm_last_error()
    # C HW = 16: a destination whose batch stride is shorter would overlap the next sample
    assert hiplib.ffwm_bias_act_forward(p, None, p, None, 2, 2, 8, 15, 0, 1, 0.2, 0, None) == -1 and b"batch stride" in hiplib.ffwm_last_error()
    assert hiplib.ffwm_bias_act_forward(p, None, p, p, 2, 2, 8, 16, 12, 1, 0.2, 0, None) == -1 and b"batch stride" in hiplib.ffwm_last_error()
    assert hiplib.ffwm_bias_act_forward(p, None, None, None, 2, 2, 8, 0, 0, 1, 0.2, 0, None) == -1 and b"NULL" in hiplib.ffwm_last_error()
    assert hiplib.ffwm_sigmoid_gate_forward_strided(p, p, p, None, p, 2, 2, 8, 15, 0, None) == -1 and b"batch stride" in hiplib.ffwm_last_error()
