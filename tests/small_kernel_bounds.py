"""Per-element yardsticks for the one-pass kernels between the reduction-heavy ones (a plain helper module, not a conftest):
csrc/mfm.hip, csrc/residual.hip, the element-wise and two-channel-backward parts of csrc/flownet_ops.hip, csrc/affine_reg.hip and the
grid-stride kernels of csrc/netg_eval.hip.  Bound, rho_any_order, SAFETY, U32 and the activations / weights / grad_outputs families
are those of tests/conv_bounds.py; u = U32 = 2^-24 is the unit roundoff of fp32 (2^-53 where a kernel runs in float64).

Exact kernels (no bound, bit for bit; tensors that may hold NaN: the same NaN positions and equal elsewhere, `assert_same`)
  * mfm / bias + ReLU: one add (x + bias, rounded once, as ATen adds it first) and a selection.  The reference is the fp32 torch
    composition on the CPU and its autograd: torch.max(*split(x + bias)), relu(h + bias).  IEEE addition and comparison are the same
    on both machines, ATen's maximum and relu propagate NaN, and maximum's derivative gives a tie half the gradient to each side.
  * LeakyReLU tails of residual.hip: a + b rounded once, z > 0 ? z : z * slope -- one add and one multiply, nothing to reassociate.
  * bias_act, act none / LeakyReLU: one add, one multiply.

tanh (bias_act act 2): conv_bounds' post = 4 ulps of tanhf against float64 tanh(fl(h + b)), rho = 0 (the add is part of the reference).

Sigmoid (residual.hip act 3, the gate, gate_strided_kernel): 1 / (1 + expf(-z)), z = fl(a + b).  No document gives the accuracy of the
device's expf, so no constant is fixed here: `sigmoid_rel_error` measures the worst |got - s| / (u s) over -87 <= z <= 87 against
s = sigmoid(a + b) in float64 from the fp32 inputs, the test measures ATen's own fp32 composition on the same device with it, and the
kernel may exceed that figure by at most SIGMOID_MARGIN = 2 u (one last-bit difference in expf, one in the division).  The inputs
(`sweep_z`) are built so that a + b is exact in fp32: a rounding of z would put up to 64 u (|z| near 87) into both figures and hide
a wrong expf behind it.  Outside the range (and for +-inf, NaN) expf has over- or underflowed to inf / 0 / NaN and nothing is left to
round: the kernel equals ATen bit for bit there (0, 1, NaN).
  Products behind a sigmoid (each fp32 product is one rounding, (1 + u)^k - 1 <= k u / (1 - k u) =: gamma_k):
    y  = x att                        from the kernel's own att (compared separately): gamma_1 |x att|
    dx = g att                        gamma_1 |g att|
    dz = ((g x) (1 - att)) att        g x, 1 - att (at most one rounding, relative to 1 - att itself; exact for att >= 1/2), two
                                      more products: gamma_4 |g x (1 - att) att|
    dz = (g (1 - y)) y                (add_act backward, sigmoid)  gamma_3 |g (1 - y) y|
  each against the float64 value of the same expression of the fp32 operands the kernel read, plus k 2^-149 (a product that lands in the
  subnormal range rounds to a multiple of 2^-149, not relatively).  `product_bound` returns these.

Flow head backward (flow_head_bwd_kernel), from a given fp32 y:  gz_ref = go (1 - y^2), gx_ref = conv2d_input(gz_ref, w) in float64.
  fl(y y) errs by u y^2 <= u, 1 - fl(y^2) by another u: an ABSOLUTE error of 2 u on a factor in [0, 1], then one product: |gz - gz_ref|
  <= 3 u |go|.  gx: 18 fma steps over gz values that each carry 3 u |go|, + 1: (18 + 4) u mag, mag = conv2d_input(|go|, |w|).
  rho_gz = SAFETY 3 u (mag = |go|), rho_gx = SAFETY 22 u.  y = +-1 gives gz = 0 exactly; integers with y = 0 are exact.
Flow upsampler backward (flow_up_bwd_kernel): 2 channels x 16 taps of fma in one chain, rho_any_order(32), mag = conv2d(|go|, |w|).

Fused affine regulariser (affine_reg_kernel), u of the tensor's dtype.  p = the float64 grid window of the fp32 / float64 flow,
M = K^T K as the kernel received it, scale = 1 / (B h' w'):
  gradient  ref = scatter over windows of 2 64 scale (M p), mag = the same scatter of 2 64 scale (|M| |p|);
            |got - ref| <= SAFETY (2 kz^2 + 4) u mag: the kz^2-term chain of r (kz^2), flow2grid's one rounding (f + 1; / 2 and * 128
            are exact) (1), the products of the chain (1), r * grad_scale and the rounding of grad_scale (2), and up to kz^2 atomics into
            one cell in any order (kz^2).
  loss      a (B)-style bound from the launch geometry (`affine_loss_terms`): a thread's q is a chain of kz^2 products p_a r_a, r_a as
            above (2 kz^2 + 2), the wave tree (6 levels), four waves added in order (4), one atomic per block (P = B 2 tiles_x tiles_y
            partial sums), the final * scale (1); mag = scale sum_windows sum_a |p_a| sum_c |M_ac| |p_c|.
A NaN in one flow cell reaches exactly the cells of the windows that hold it (within kz - 1 of it, same sample and grid) and the loss.

Route rules restated (the source line each restates is named at the function): flow_head_tile, the vector / scalar predicates and the
grid caps.  tests/test_small_kernel_bounds_cpu.py resolves every GPU shape through them and meets every bound above with fp32 stand-ins
and rho / SAFETY.
"""
import math

import torch
import torch.nn.functional as F

import conv_bounds as cb
from conv_bounds import Bound, SAFETY, U32, rho_any_order, activations, weights, grad_outputs  # noqa: F401  (re-exported)

U64 = 2.0 ** -53
KBLOCK = 256                      # common.hpp:13
SUBNORMAL = 2.0 ** -149
SIGMOID_MARGIN = 2.0              # u: one last-bit difference in expf, one in the division
SIGMOID_RANGE = 87.0

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ route rules, restated
def flow_head_tile(B, HW):
    """flownet_ops.hip:322 `flow_head_tile`: the widest of 64 / 16 / 4 pixels per block that still gives 96 blocks."""
    def blocks(P):
        return B * (-(-HW // P))
    return 64 if HW >= 64 and blocks(64) >= 96 else (16 if HW >= 16 and blocks(16) >= 96 else 4)


def _grid(n, cap):
    return max(min(-(-n // KBLOCK), cap), 1)


def _route(vec, n_elems, cap):
    """-> (route, work items, True when the items exceed one sweep of the capped grid)."""
    items = n_elems // 4 if vec else n_elems
    return ("vector" if vec else "scalar"), items, items > _grid(items, cap) * KBLOCK


def mfm_route(shape, offset=0):
    """mfm.hip:148 (`vec = HW % 4 == 0 && pointers % 16 == 0`) and mfm.hip:114 `mfm_grid` (8192 blocks); shape = x [B, 2C, ...],
    offset = the element offset of x in a 16-byte aligned buffer.  Items are outputs (B C HW)."""
    B, C2 = shape[0], shape[1]
    HW = int(math.prod(shape[2:]))
    return _route(HW % 4 == 0 and offset % 4 == 0, B * (C2 // 2) * HW, 256 * 32)


def bias_relu_route(shape, offset=0):
    """mfm.hip:132 and mfm_grid."""
    HW = int(math.prod(shape[2:]))
    return _route(HW % 4 == 0 and offset % 4 == 0, int(math.prod(shape)), 256 * 32)


def bias_act_route(shape, y_stride=None, y2_stride=None, offsets=(0, 0, 0)):
    """flownet_ops.hip:304 (`vec`: HW % 4 == 0, h aligned, every destination aligned with a batch stride % 4 == 0) and :218 `ew_grid`
    (8192 blocks).  y_stride / y2_stride: None = destination absent; offsets = element offsets of (h, y, y2)."""
    B, C, H, W = shape
    vec = (H * W) % 4 == 0 and offsets[0] % 4 == 0
    for s, o in ((y_stride, offsets[1]), (y2_stride, offsets[2])):
        if s is not None:
            vec = vec and o % 4 == 0 and s % 4 == 0
    return _route(vec, B * C * H * W, 256 * 32)


def residual_route(n):
    """residual.hip:110 `vec_grid` (kVecBlocks = 2048 blocks of float4 lanes) and the tail lane (residual.hip:48).
    -> (float4 items, tail elements, past the cap)."""
    n4 = n // 4
    return n4, n - 4 * n4, n4 > _grid((n + 3) // 4, 256 * 8) * KBLOCK


def gate_strided_route(shape, y_stride, offset=0):
    """netg_eval.hip:337 (`vec`: C HW % 4 == 0, batch stride % 4 == 0, all pointers aligned) and :23 `ew_grid` (kEwBlocks = 2048)."""
    B, C, H, W = shape
    return _route((C * H * W) % 4 == 0 and y_stride % 4 == 0 and offset % 4 == 0, B * C * H * W, 256 * 8)


def shuffle_route(h_shape, y_stride, offset=0):
    """netg_eval.hip:269-270: vec when W % 4 == 0 (aligned, stride % 4 == 0); items = B K H W / (4 | 1), K = C / 4."""
    B, C4, H, W = h_shape
    return _route(W % 4 == 0 and y_stride % 4 == 0 and offset % 4 == 0, B * (C4 // 4) * H * W, 256 * 8)


def upsample_route(x_shape, y_stride, offset=0):
    """netg_eval.hip:315-316: vec when W % 2 == 0 (four OUTPUT pixels per lane); items = B C 2H 2W / (4 | 1)."""
    B, C, H, W = x_shape
    return _route(W % 2 == 0 and y_stride % 4 == 0 and offset % 4 == 0, B * C * 4 * H * W, 256 * 8)


# ---- the GPU matrix of tests/test_gpu_small_kernel_bounds.py: (shape, element offset of the tensor in its buffer, route, past the cap)
MFM_SHAPES = [((3, 10, 7, 9), 0, "scalar", False), ((2, 6, 2, 2), 0, "vector", False), ((2, 6, 4, 6), 1, "scalar", False),
              ((1, 66, 255, 257), 0, "scalar", True), ((1, 130, 256, 512), 0, "vector", True)]
RELU_SHAPES = [((3, 5, 7, 9), 0, "scalar", False), ((2, 3, 2, 2), 0, "vector", False), ((2, 3, 4, 6), 1, "scalar", False),
               ((1, 33, 255, 257), 0, "scalar", True), ((1, 65, 256, 512), 0, "vector", True)]
# shape -> (tail elements, past the cap) of residual.hip
RESIDUAL_EXPECT = {(1, 1, 1, 5): (1, False), (1, 1, 2, 3): (2, False), (1, 1, 1, 7): (3, False), (2, 3, 4, 6): (0, False),
                   (1, 33, 256, 256): (0, True), (1, 3, 839, 841): (1, True)}
GATE_STRIDED_SHAPES = [((1, 33, 256, 256), "vector"), ((1, 3, 419, 421), "scalar")]
# name -> (shape, y (batch stride, element offset) | "inplace" | None, y2 (batch stride, element offset) | None, bias, route, past the cap)
BIAS_ACT_CASES = {
    "inplace": ((2, 6, 4, 6), "inplace", None, True, "vector", False),
    "no_bias": ((2, 6, 4, 6), "inplace", None, False, "vector", False),
    "y_slice": ((2, 6, 4, 6), (11 * 24, 2 * 24), None, True, "vector", False),
    "y_and_y2": ((2, 6, 4, 6), (11 * 24, 2 * 24), (9 * 24, 24), True, "vector", False),
    "y2_only": ((2, 6, 4, 6), None, (9 * 24, 24), True, "vector", False),
    "odd_plane": ((2, 5, 7, 9), (10 * 63, 2 * 63), (8 * 63, 63), True, "scalar", False),
    "odd_stride": ((2, 6, 4, 6), (6 * 24 + 6, 0), None, True, "scalar", False),
    "misaligned_slice": ((2, 6, 4, 6), (6 * 24 + 8, 2), None, True, "scalar", False),
    "past_scalar": ((1, 33, 255, 257), (33 * 255 * 257, 0), None, True, "scalar", True),
    "past_vector": ((1, 130, 256, 256), (130 * 65536, 0), None, True, "vector", True),
}


def bias_act_case_route(name):
    shape, y, y2, _, _, _ = BIAS_ACT_CASES[name]
    B, C, H, W = shape
    if y == "inplace":
        y = (C * H * W, 0)
    return bias_act_route(shape, None if y is None else y[0], None if y2 is None else y2[0],
                          (0, 0 if y is None else y[1], 0 if y2 is None else y2[1]))


# the new flow-head shapes of tests/test_gpu_conv_bounds.FLOW_HEADS and the backward matrix below
FLOW_HEAD_SHAPES = [(8, 1024, 2, 2), (8, 256, 8, 8), (3, 70, 9, 11), (8, 32, 64, 64), (2, 16, 128, 128), (6, 128, 16, 16), (4, 70, 19, 23)]
FLOW_HEAD_BWD_SHAPES = [(8, 1024, 2, 2), (3, 70, 9, 11), (6, 128, 16, 16), (4, 70, 19, 23), (8, 32, 64, 64)]


def flow_head_tiles(shapes):
    return {s: flow_head_tile(s[0], s[2] * s[3]) for s in shapes}


# ------------------------------------------------------------------------------------------------ comparisons
def assert_same(got, ref, what=""):
    """Same NaN positions, equal elsewhere (torch.equal alone fails on a correct NaN)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    gn, rn = torch.isnan(got), torch.isnan(ref)
    if not torch.equal(gn, rn):
        bad = (gn != rn).nonzero()
        raise AssertionError("%s: NaN positions differ at %d elements, first %s (got %r, reference %r)" % (
            what, bad.shape[0], tuple(int(i) for i in bad[0]), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])])))
    eq = (got == ref) | rn
    if not bool(eq.all()):
        bad = (~eq).nonzero()
        raise AssertionError("%s: %d elements differ, first %s (got %r, reference %r)" % (
            what, bad.shape[0], tuple(int(i) for i in bad[0]), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])])))


def offset_view(t, offset=1):
    """A contiguous copy of t that starts `offset` elements into its (16-byte aligned) buffer, on t's device."""
    buf = torch.empty(t.numel() + offset + 3, dtype=t.dtype, device=t.device)
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() - buf.data_ptr()) == offset * t.element_size()
    return v


# ------------------------------------------------------------------------------------------------ mfm / bias + ReLU
MFM_KINDS = ("iid", "ties", "bias_ties", "zeros", "nan_first", "nan_second", "nan_both", "inf", "nan_by_bias")
MFM_NONFINITE = ("nan_first", "nan_second", "nan_both", "inf", "nan_by_bias")
RELU_KINDS = ("iid", "zeros", "nan", "inf", "nan_by_bias")
RELU_NONFINITE = ("nan", "inf", "nan_by_bias")


def mfm_inputs(kind, shape, seed, with_bias):
    """-> (x [B, 2C, ...], bias [2C] or None, grad_output [B, C, ...]) float32."""
    gen = torch.Generator().manual_seed(seed)
    B, C2 = shape[0], shape[1]
    C = C2 // 2
    x = torch.randn(shape, generator=gen)
    bias = torch.randn(C2, generator=gen) if with_bias else None
    go = torch.randn((B, C) + tuple(shape[2:]), generator=gen)
    halves = x.view(B, 2, -1)
    n = halves.shape[2]
    if kind == "ties":                                    # exact ties between the halves (of x + bias when there is one)
        if bias is not None:
            bias[C:] = bias[:C]
        halves[:, 1, ::3] = halves[:, 0, ::3]
    elif kind == "bias_ties":                             # halves that differ by exactly what the bias takes back
        if bias is None:
            halves[:, 1, ::3] = halves[:, 0, ::3]
        else:
            bias.copy_(torch.randint(-4, 5, (C2,), generator=gen).float())
            x.copy_(torch.randint(-8, 9, shape, generator=gen).float())
            xa = x.view(B, 2, C, -1)
            xa[:, 1, :, ::2] = xa[:, 0, :, ::2] + (bias[:C] - bias[C:]).view(1, C, 1)
    elif kind == "zeros":
        halves[:, :, ::2] = 0
        halves[:, 0, 1::4] = -0.0
    elif kind == "nan_first":
        halves[:, 0, 1::5] = NAN
    elif kind == "nan_second":
        halves[:, 1, 2::5] = NAN
    elif kind == "nan_both":
        halves[:, 0, 1::5] = NAN
        halves[:, 1, 1::7] = NAN
    elif kind == "inf":
        halves[:, 0, 0::7] = INF
        halves[:, 1, 0::5] = -INF
        halves[:, 1, 3::11] = INF
        halves[:, 0, 4::13] = -INF
    elif kind == "nan_by_bias":                           # inf + (-inf bias) = NaN, made by the kernel's own add
        if bias is None:
            halves[:, 0, 1::5] = NAN
        else:
            bias[0] = -INF
            bias[C2 - 1] = INF
            xa = x.view(B, 2, C, -1)
            xa[:, 0, 0, ::2] = INF
            xa[:, 1, C - 1, 1::3] = -INF
    elif kind != "iid":
        raise ValueError(kind)
    assert n > 0
    return x.contiguous(), bias, go.contiguous()


def mfm_reference(x, bias, go):
    """torch.max(*split(x + bias)) and its autograd in fp32 on the CPU -> (y, d(x), d(bias) or None)."""
    xr = x.detach().cpu().clone().requires_grad_(True)
    br = None if bias is None else bias.detach().cpu().clone().requires_grad_(True)
    h = xr if br is None else xr + br.view(1, -1, *([1] * (x.dim() - 2)))
    a, b = torch.split(h, x.shape[1] // 2, 1)
    y = torch.max(a, b)
    y.backward(go.detach().cpu())
    return y.detach(), xr.grad, (None if br is None else br.grad)


def relu_inputs(kind, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    C = shape[1]
    h, bias, go = torch.randn(shape, generator=gen), torch.randn(C, generator=gen), torch.randn(shape, generator=gen)
    flat = h.view(-1)
    if kind == "zeros":
        bias.copy_(torch.randint(-2, 3, (C,), generator=gen).float())
        h.copy_(torch.randint(-2, 3, shape, generator=gen).float())          # h + bias = +-0 often
        flat[1::4] = -0.0
    elif kind == "nan":                                    # NaN against the 0 of ReLU
        flat[1::5] = NAN
    elif kind == "inf":
        flat[0::7] = INF
        flat[3::5] = -INF
    elif kind == "nan_by_bias":
        bias[0] = -INF
        bias[C - 1] = INF
        hv = h.view(shape[0], C, -1)
        hv[:, 0, ::2] = INF
        hv[:, C - 1, 1::3] = -INF
    elif kind != "iid":
        raise ValueError(kind)
    return h.contiguous(), bias, go.contiguous()


def relu_reference(h, bias, go):
    hr, br = h.detach().cpu().clone().requires_grad_(True), bias.detach().cpu().clone().requires_grad_(True)
    y = torch.relu(hr + br.view(1, -1, *([1] * (h.dim() - 2))))
    y.backward(go.detach().cpu())
    return y.detach(), hr.grad, br.grad


# ------------------------------------------------------------------------------------------------ residual tails and gate
RESIDUAL_SIZES = [(1, 1, 1, 5), (1, 1, 2, 3), (1, 1, 1, 7), (2, 3, 4, 6), (1, 33, 256, 256), (1, 3, 839, 841)]       # tails 1, 2, 3, 0; past the cap with tail 0 and 1
SMALLEST_NORMAL = 2.0 ** -126


def sweep_z(n, seed):
    """(a, b) float32 [n] with z = a + b swept over [-100, 100], the saturation edges, the kink, +-inf and NaN at fixed places.  a, b and
    z are multiples of 2^-10 below 2^8, so the fp32 sum is EXACT (asserted): the float64 reference sigmoid(a + b) is then the sigmoid
    of the very z the kernel forms, and the measured error is that of expf and the division alone."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.round(torch.linspace(-100.0, 100.0, n) * 1024) / 1024
    z = z[torch.randperm(n, generator=gen)]
    b = (torch.round(torch.randn(n, generator=gen) * 1024) / 1024).clamp(-4, 4)
    a = z - b
    special = [0.0, -0.0, SMALLEST_NORMAL, -SMALLEST_NORMAL, 2.0 ** -149, -2.0 ** -149, -20.0, 20.0, -87.0, 87.0, -87.5, 87.5, -88.75, 88.75,
               -100.0, 100.0, -104.0, 104.0, INF, -INF, NAN]
    k = min(len(special), n)
    pos = torch.arange(k) * max(n // k, 1)
    a[pos] = torch.tensor(special[:k])
    b[pos] = 0.0
    if n > 2 * k:
        a[1], b[1] = INF, -INF                             # NaN made by the add
    fin = torch.isfinite(a) & torch.isfinite(b)
    assert torch.equal((a + b)[fin].double(), a[fin].double() + b[fin].double())
    return a.contiguous(), b.contiguous()


def mixed_scale(n, seed):
    """x / g of mixed scale: normal values times powers of two over 2^-12 .. 2^12."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=gen) * torch.exp2(torch.randint(-12, 13, (n,), generator=gen).float())).contiguous()


def leaky_reference(a, b, go, slope):
    """ATen's fp32 composition on the CPU -> (y, dz)."""
    ar, br = a.detach().cpu().clone().requires_grad_(True), b.detach().cpu().clone()
    y = F.leaky_relu(ar + br, slope)
    y.backward(go.detach().cpu())
    return y.detach(), ar.grad


def sigmoid_in_range(a, b):
    z = a.detach().cpu().double() + b.detach().cpu().double()
    return (z >= -SIGMOID_RANGE) & (z <= SIGMOID_RANGE)


def sigmoid_rel_error(got, a, b):
    """Worst |got - s| / (u s) over the elements with -87 <= a + b <= 87, s = sigmoid(a + b) in float64 from the fp32 inputs."""
    z = a.detach().cpu().double() + b.detach().cpu().double()
    m = sigmoid_in_range(a, b)
    s = torch.sigmoid(z[m])
    e = (got.detach().cpu().double()[m] - s).abs() / (U32 * s)
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    return float(e.max()) if e.numel() else 0.0


def check_sigmoid(got, aten, a, b, what, need_outside=True):
    """The kernel's sigmoid against ATen's on the same inputs: within SIGMOID_MARGIN u of ATen's worst relative error inside the range,
    bit for bit outside it.  Prints and returns both figures."""
    e_aten, e_got = sigmoid_rel_error(aten, a, b), sigmoid_rel_error(got, a, b)
    print("SMALLBOUND %s: sigmoid worst relative error %.3f u, ATen %.3f u, allowed %.3f u" % (what, e_got, e_aten, e_aten + SIGMOID_MARGIN))
    out = ~sigmoid_in_range(a, b)
    assert bool(out.any()) or not need_outside
    g, r = got.detach().cpu(), aten.detach().cpu()
    assert_same(g[out], r[out], what + " outside [-87, 87]")
    assert not bool(torch.isnan(g[~out]).any()), what
    assert e_got <= e_aten + SIGMOID_MARGIN, "%s: sigmoid worst relative error %.3f u, ATen's %.3f u + %g u" % (what, e_got, e_aten, SIGMOID_MARGIN)
    return e_got, e_aten


def product_bound(ref64, roundings):
    """gamma_k |ref| + k 2^-149 for a value formed by k fp32 roundings, each relative to its own result."""
    k = float(roundings)
    return (k * U32 / (1.0 - k * U32)) * ref64.abs() + k * SUBNORMAL


def check_product(got, ref64, roundings, what):
    """-> error / bound; non-finite references must be matched in kind (NaN with NaN, an infinity with the same infinity)."""
    got = got.detach().cpu().double()
    fin = torch.isfinite(ref64)
    assert_same(torch.where(fin, torch.zeros_like(got), got), torch.where(fin, torch.zeros_like(ref64), ref64), what + " non-finite")
    q = torch.where(fin, (got - ref64).abs() / product_bound(ref64, roundings), torch.zeros_like(got))
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
    ratio = float(q.max())
    print("SMALLBOUND %s: error/bound %.3g (%d roundings)" % (what, ratio, roundings))
    assert ratio <= 1.0, "%s: error / bound = %.3g at %d" % (what, ratio, int(q.argmax()))
    return ratio


def gate_backward_refs(x, att, g):
    """float64 of exactly what the kernel read -> (dz_ref (4 roundings), dx_ref (1 rounding))."""
    xd, sd, gd = x.detach().cpu().double(), att.detach().cpu().double(), g.detach().cpu().double()
    return gd * xd * (1.0 - sd) * sd, gd * sd


def sigmoid_backward_ref(y, g):
    yd, gd = y.detach().cpu().double(), g.detach().cpu().double()
    return gd * (1.0 - yd) * yd                            # 3 roundings


# ------------------------------------------------------------------------------------------------ bias_act
def bias_act_reference(h, bias, act, slope=0.2):
    """act 0 / 1: the fp32 CPU composition (bit for bit).  act 2: Bound(ref = float64 tanh(fl(h + b)), rho 0, post 4)."""
    h = h.detach().cpu()
    pre = h if bias is None else h + bias.detach().cpu().view(1, -1, 1, 1)
    if act == 0:
        return pre
    if act == 1:
        return F.leaky_relu(pre, slope)
    return Bound(torch.tanh(pre.double()), torch.zeros(pre.shape, dtype=torch.float64), 0.0, 4.0, what="bias_act tanh")


# ------------------------------------------------------------------------------------------------ flow head / upsampler backward
HEAD_Y_KINDS = ("moderate", "saturated", "ones")


def head_outputs(kind, shape, seed):
    """The forward's y [B, 2, H, W] handed to the backward: tanh of a normal, saturated up to 1 - 2^-24, or exactly +-1."""
    gen = torch.Generator().manual_seed(seed)
    n = int(math.prod(shape))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    if kind == "moderate":
        y = torch.tanh(torch.randn(n, generator=gen))
    elif kind == "saturated":
        y = sign * (1.0 - torch.exp2(-(torch.arange(n) % 24 + 1).float()))
        assert float(y.abs().max()) == 1.0 - 2.0 ** -24
    elif kind == "ones":
        y = sign
    elif kind == "zero":
        y = torch.zeros(n)
    else:
        raise ValueError(kind)
    return y.view(shape).contiguous()


def flow_head_backward_bounds(y, go, w, exact=False, safety=SAFETY, what=""):
    """-> (Bound of grad_z, Bound of grad_x); w = the head's weight [2, C, 3, 3]."""
    yd, gd, wd = y.detach().cpu().double(), go.detach().cpu().double(), w.detach().cpu().double()
    B, _, H, W = yd.shape
    shape = (B, wd.shape[1], H, W)
    gz = gd * (1.0 - yd * yd)
    gx = torch.nn.grad.conv2d_input(shape, wd, gz, 1, 1)
    mag = torch.nn.grad.conv2d_input(shape, wd.abs(), gd.abs(), 1, 1)
    if exact:
        cb.require_exact(mag, 1.0, what)
    return (Bound(gz, gd.abs(), safety * 3 * U32, 0.0, exact, what + " grad_z"),
            Bound(gx, mag, safety * (18 + 4) * U32, 0.0, exact, what + " grad_x"))


def flow_up_backward_bound(go, w, exact=False, safety=SAFETY, what=""):
    """d(input) of ConvTranspose2d(2, 2, 4, 2, 1): conv2d(go, w, stride 2, pad 1) with w [Ci, Co, 4, 4] read as [out, in, 4, 4]."""
    gd, wd = go.detach().cpu().double(), w.detach().cpu().double()
    ref = F.conv2d(gd, wd, None, 2, 1)
    mag = F.conv2d(gd.abs(), wd.abs(), None, 2, 1)
    if exact:
        cb.require_exact(mag, 1.0, what)
    return Bound(ref, mag, rho_any_order(2 * 16) * safety / SAFETY, 0.0, exact, what + " grad_x")


def _shift(t, dy, dx, wrap=False):
    """t[..., y + dy, x + dx] with zeros (or, wrap: the rolled neighbour) outside."""
    if wrap:
        return torch.roll(t, (-dy, -dx), (2, 3))
    H, W = t.shape[2:]
    p = F.pad(t, (1, 1, 1, 1))
    return p[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def flow_head_backward_f32(y, go, w, flipped=True, masked=True):
    """The kernel's arithmetic restated in fp32 torch, in its chain order (tap k = 0 .. 8, channel 0 then 1 of grad_z).  flipped=False
    and masked=False are the two slips the mutants restate: taps read at p + (r - 1, s - 1), and neighbours read across the border."""
    gz = go * (1.0 - y * y)
    C = w.shape[1]
    gx = torch.zeros((y.shape[0], C) + tuple(y.shape[2:]), dtype=y.dtype)
    for k in range(9):
        dy, dx = 1 - k // 3, 1 - k % 3
        if not flipped:
            dy, dx = -dy, -dx
        z = _shift(gz, dy, dx, wrap=not masked)
        for ch in range(2):
            gx = gx + z[:, ch:ch + 1] * w[ch, :, k // 3, k % 3].view(1, C, 1, 1)
    return gz, gx


def flow_up_backward_f32(go, w):
    """flow_up_bwd_kernel's chain in fp32 torch: taps ky, kx in order, output channel 0 then 1."""
    B, _, Ho, Wo = go.shape
    H, W = Ho // 2, Wo // 2
    gp = F.pad(go, (1, 1, 1, 1))
    gx = torch.zeros(B, 2, H, W, dtype=go.dtype)
    for ky in range(4):
        for kx in range(4):
            tap = gp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2]              # go[2 iy - 1 + ky, 2 ix - 1 + kx]
            for co in range(2):
                gx = gx + tap[:, co:co + 1] * w[:, co, ky, kx].view(1, 2, 1, 1)
    return gx


# ------------------------------------------------------------------------------------------------ fused affine regulariser
AFFINE_SHAPES = [(1, 3, 3, 3), (2, 6, 67, 3), (2, 9, 69, 5), (1, 12, 71, 7), (3, 37, 41, 5)]
AFFINE_FLOWS = ("uniform", "smooth", "constant", "extremes", "nan_cell")
AR_TILE_X, AR_TILE_Y = 64, 4      # affine_reg.hip:25


def affine_matrix(kz):
    """K^T K [kz^2, kz^2] in float64, as ffwm_amd.losses builds it."""
    from ffwm_amd.losses import affine_residual_kernels
    return affine_residual_kernels(kz).reshape(kz * kz, kz * kz).double()


def affine_flow(kind, B, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind in ("uniform", "nan_cell"):
        f = torch.rand(B, 2, h, w, generator=gen) * 2 - 1
        if kind == "nan_cell":
            f[B - 1, 1, h // 2, w - 2] = NAN
    elif kind == "smooth":
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
        import fill
        f = fill.flow_field(B, h, w, "affine_%d" % seed).clamp(-1, 1)
    elif kind == "constant":
        f = torch.full((B, 2, h, w), 0.3)
    elif kind == "extremes":
        f = torch.where(torch.rand(B, 2, h, w, generator=gen) < 0.5, -1.0, 1.0)
    else:
        raise ValueError(kind)
    return f.float().contiguous()


def affine_loss_terms(B, h, w, kz):
    """(L, P) of the loss: a thread's chain (r: kz^2 adds + products + flow2grid = kz^2 + 2; q: kz^2), the wave tree (6), the four waves
    in order (4), the final scale (1); P = one atomic per block, blocks as affine_reg.hip:95-97 `launch` counts them."""
    hw, ww = h - kz + 1, w - kz + 1
    blocks = B * 2 * (-(-ww // AR_TILE_X)) * (-(-hw // AR_TILE_Y))
    return 2 * kz * kz + 2 + 6 + 4 + 1, blocks


def affine_bounds(flow, M, kz, dtype=torch.float32, safety=SAFETY, what=""):
    """-> (Bound of the loss (0-d), Bound of grad_flow).  flow in the dtype the kernel gets, M float64 [kz^2, kz^2] rounded to it."""
    u = U32 if dtype == torch.float32 else U64
    B, _, h, w = flow.shape
    hw, ww = h - kz + 1, w - kz + 1
    scale = 1.0 / (B * hw * ww)
    Md = M.to(dtype).double()
    grid = (flow.detach().cpu().to(dtype).double() + 1.0) / 2.0 * 128.0
    p = F.unfold(grid.reshape(B * 2, 1, h, w), kz)                             # [B 2, kz^2, windows]
    r, rm = Md @ p, Md.abs() @ p.abs()
    g = 2.0 * 64.0 * scale
    ref = F.fold(r * g, (h, w), kz).reshape(B, 2, h, w)
    mag = F.fold(rm * g, (h, w), kz).reshape(B, 2, h, w)
    L, P = affine_loss_terms(B, h, w, kz)
    loss = Bound((p * r).sum() * scale, (p.abs() * rm).sum() * scale, safety * (L + P) * u, what=what + " loss")
    # Bound's roundoff of `post` and its floor are fp32's; neither is used here (post = 0; the floor 1e-38 is far below both)
    return loss, Bound(ref, mag, safety * (2 * kz * kz + 4) * u, what=what + " grad_flow")


def affine_f32(flow, M, kz, want_grad=True, skip_window_column=None):
    """The kernel's arithmetic restated sequentially in flow's dtype: r = sum_c M[a, c] p[c] as a chain, q += p[a] r, the gradient added
    window cell by window cell (a = 0 .. kz^2 - 1).  skip_window_column: the mutant that loses that window column's contributions."""
    dt = flow.dtype
    B, _, h, w = flow.shape
    hw, ww = h - kz + 1, w - kz + 1
    scale = 1.0 / (B * hw * ww)
    Mt = M.to(dt)
    grid = ((flow + 1) / 2) * 128
    win = [grid[:, :, i:i + hw, j:j + ww] for i in range(kz) for j in range(kz)]
    gs = torch.tensor(2.0 * 64.0 * scale, dtype=dt)
    grad = torch.zeros_like(flow)
    q = torch.zeros_like(win[0])
    for a in range(kz * kz):
        r = torch.zeros_like(win[0])
        for c in range(kz * kz):
            r = r + Mt[a, c] * win[c]
        q = q + win[a] * r
        contrib = r * gs
        if skip_window_column is not None:
            contrib = contrib.clone()
            contrib[..., skip_window_column] = 0
        i, j = a // kz, a % kz
        grad[:, :, i:i + hw, j:j + ww] += contrib
    return q.sum() * scale, (grad if want_grad else None)
