"""Float64 error bounds, exact family, non-finite contract and torch restatement of the split batched-GEMM Winograd route as the
FROZEN loss networks of the train step use it (ffwm_conv3x3_wg_split_apply, ffwm_conv3x3_wg_split_weights_dgrad,
csrc/conv_winograd_gemm_split.hip): the data gradient with its ReLU mask and the `relu` / `mfm` epilogues.  A plain helper module, not
a conftest.  It builds on wino_split_cases.py (the split route's derivation: rho_split, SplitBound, the exact family) and on
wino_gemm_cases.py (the fp32 route's data-gradient cases and epilogue bounds); no constant is fitted.

Data gradient.  d(input) of Conv2d(C, K, 3, 1, 1) is the convolution of grad_output [B, K, H, W] with the layer's weight transposed
  and rotated by 180 degrees: the same kernels with the roles swapped, C output rows and a reduction over K.  The derivation of
  wino_split_cases.py holds word for word with K in the place of C:
      |got - ref| <= rho_split(K) mag_patch + SAFETY u |ref| + eta
  ref and mag_patch = sum_k (max |go_k| over the 4 x 4 patch) (sum of |w_kc| over the taps) from cb.forward_bound(go, w, None, mode=3,
  winograd=True); eta = 2^-126 x 16 (3 sum_k (4 X_k + G_kc) + 6 K) from the patch magnitudes of go and the tap sums over K.
  The ReLU mask is an exact selection of grad_output elements made BEFORE the transform (`mask <= 0 ? 0 : x`, aten::threshold_backward:
  a NaN in the mask lets the value pass, a masked-out infinity or NaN is a zero): the masked case is the same bound of
  aten.threshold_backward(go, y, 0).
Epilogues.  `none` and `bias` are wino_split_cases.split_bounds.  `relu` is wino_gemm_cases.relu_bound of the split bias bound (ReLU
  is 1-Lipschitz and exact).  `mfm` takes max(a, b) of two output channels; max is 1-Lipschitz in each argument, so the bound is the
  maximum of the halves' references and magnitudes under rho_split(C), as wino_gemm_cases.forward_case has it for the fp32 route.
Exact family.  wino_split_cases.split_exact_inputs gives x and a weight w' whose convolution is exact in the three-term arithmetic.
  The layer whose data gradient IS that convolution has the weight w'.transpose(0, 1).flip(2, 3): its data gradient of x must be the
  three-term value bit for bit.
Restatement.  split_flow_f32 below is wino_split_cases.split_flow_f32 with `data_gradient` and `mask`, the epilogues of the fp32
  route, and the mutants not_rotated, not_transposed (the weight's memory read as [C, K, 3, 3] without the transposition),
  mask_on_output (the mask applied position by position to the transformed patches instead of to the input) and mask_lt (`< 0`
  instead of `<= 0`: a ReLU output is never negative, so nothing is masked)."""
import functools

import torch

import conv_bounds as cb
import wino_gemm_cases as wc
import wino_split_cases as ws
from colmax_split_bounds import TINY, split_terms
from conv_bounds import SAFETY

SHAPES = ws.SHAPES
# the data gradient also with a reduction (K = 19) shorter than one 32-channel stage and a ragged output-row tile (C = 70)
DGRAD_SHAPES = ws.SHAPES + [(2, 70, 7, 9, 19)]
TILES = ws.TILES
EPILOGUES = ("none", "bias", "relu", "mfm")
MUTANTS = ("not_rotated", "not_transposed", "mask_on_output", "mask_lt")
MUTANT_SHAPE = (2, 19, 7, 9, 70)


def split_dgrad_bound(go, w, safety=SAFETY, exact=False, what=""):
    """The bound of d(input) [B, C, H, W] for float32 go [B, K, H, W] and the layer's own w [K, C, 3, 3]: split_bounds, roles swapped."""
    ws.check_contract(go, w)
    K = w.shape[0]
    rho = ws.rho_split(K, safety)
    base = cb.forward_bound(go, w, None, mode=3, rho=rho, winograd=True, exact=exact, what=what)
    g = w.double().abs().sum((2, 3)).t()                                       # [C, K]: output row, reduction
    sum_x = cb.patch_mag_forward(go.double(), torch.ones_like(g))
    eta = TINY * 16.0 * (3.0 * (4.0 * sum_x + g.sum(1).view(1, -1, 1, 1)) + 6.0 * K)
    eta = torch.where(torch.isfinite(eta), eta, torch.zeros_like(eta))
    return ws.SplitBound(base.ref, base.mag, rho, safety + base.post, exact, what, eta)


def split_dgrad_bounds(go, w, y, safety=SAFETY, exact=False, what=""):
    """-> {False: plain, True: behind the ReLU whose output is y}."""
    masked_go = torch.ops.aten.threshold_backward(go, y, 0)
    return {False: split_dgrad_bound(go, w, safety, exact, what),
            True: split_dgrad_bound(masked_go, w, safety, exact, what + " relu mask")}


@functools.lru_cache(maxsize=None)
def split_dgrad_case(shape, kind):
    """-> go [B, K, H, W], the layer's w [K, C, 3, 3], a ReLU output y of go's shape (zeros, positives, one NaN that lets the gradient
    pass: wino_gemm_cases.dgrad_case), and the bounds {False: plain, True: masked} of d(input) [B, C, H, W]."""
    B, C, H, W, K = shape
    small = K > 64
    s = 2000 * DGRAD_SHAPES.index(shape) + 17 * cb.FAMILIES.index(kind) + 507
    go = cb.grad_outputs(kind, (B, K, H, W), s, small)
    w, _ = cb.weights(kind, (K, C, 3, 3), s + 1, out_dim=1, small=small)
    y = torch.relu(torch.randn((B, K, H, W), generator=torch.Generator().manual_seed(s + 2)))
    y[0, 0, 0, 0] = float("nan")
    return go, w, y, split_dgrad_bounds(go, w, y, exact=kind == "integers", what="wg split dgrad %s %s" % (shape, kind))


def split_epilogue_bounds(x, w, b, safety=SAFETY, exact=False, what=""):
    """-> {"none", "bias", "relu", "mfm"} for float32 x [B, C, H, W], w [K, C, 3, 3] (K even), b [K]."""
    base = ws.split_bounds(x, w, b, safety=safety, exact=exact, what=what)
    pre = base["bias"]
    h = w.shape[0] // 2
    mfm = cb.Bound(torch.maximum(pre.ref[:, :h], pre.ref[:, h:]), torch.maximum(pre.mag[:, :h], pre.mag[:, h:]), pre.rho, 0.0, exact,
                   what + " bias+mfm")
    return {"none": base["none"], "bias": pre, "relu": wc.relu_bound(pre, what + " bias+relu"), "mfm": mfm}


@functools.lru_cache(maxsize=None)
def split_forward_case(shape, kind):
    """-> x, w, b of wino_split_cases.split_case and the bounds of the four epilogues of the loss networks' entry."""
    x, w, b, _ = ws.split_case(shape, kind)
    return x, w, b, split_epilogue_bounds(x, w, b, exact=kind == "integers", what="wg split train %s %s" % (shape, kind))


def with_safety_one(bound, C):
    """-> (rho, post) of `bound` with SAFETY = 1 on every count of roundings, for a reduction over C."""
    return ws.rho_split(C, safety=1.0), (bound.post - SAFETY + 1.0 if isinstance(bound, ws.SplitBound) else bound.post)


# ------------------------------------------------------------------------------------------------ the data flow in torch fp32
def split_flow_f32(x, w, b=None, epilogue="none", data_gradient=False, mask=None, mutant=None):
    """wino_split_cases.split_flow_f32 as the loss networks call it: the kernels' data flow, every step in fp32.  data_gradient: w is
    the layer's own [K, C, 3, 3] and x its grad_output [B, K, H, W]; mask: a tensor of x's shape, x is read as `mask <= 0 ? 0 : x`."""
    if mask is not None and mutant != "mask_on_output":
        drop = (mask < 0) if mutant == "mask_lt" else (mask <= 0)
        x = torch.where(drop, torch.zeros_like(x), x)
    if data_gradient:
        if mutant == "not_rotated":
            w = w.transpose(0, 1).contiguous()
        elif mutant == "not_transposed":
            w = w.contiguous().view(w.shape[1], w.shape[0], 3, 3).flip(2, 3).contiguous()
        else:
            w = w.transpose(0, 1).flip(2, 3).contiguous()
    B, C, H, W = x.shape
    K = w.shape[0]
    bt, g, at = cb._BT.to(x.dtype), cb._G.to(x.dtype), cb._AT.to(x.dtype)
    P = cb._patches(x)
    TH, TW = P.shape[2], P.shape[3]
    T = B * TH * TW
    Vp = bt @ P @ bt.t()
    if mask is not None and mutant == "mask_on_output":
        Vp = torch.where(cb._patches(mask) <= 0, torch.zeros_like(Vp), Vp)
    V = Vp.permute(4, 5, 1, 0, 2, 3).reshape(16, C, T)
    U = (g @ w @ g.t()).permute(2, 3, 0, 1).reshape(16, K, C)
    uh, ul = (t.to(x.dtype) for t in split_terms(U))
    vh, vl = (t.to(x.dtype) for t in split_terms(V))
    M = (torch.bmm(ul, vh) + torch.bmm(uh, vl)) + torch.bmm(uh, vh)
    M = M.reshape(4, 4, K, B, TH, TW).permute(3, 2, 4, 5, 0, 1)
    Y = at @ M @ at.t()
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, K, 2 * TH, 2 * TW)[:, :, :H, :W]
    if epilogue != "none":
        y = y + b.view(1, -1, 1, 1)
    if epilogue == "relu":
        y = torch.relu(y)
    elif epilogue == "mfm":
        y = torch.maximum(y[:, :K // 2], y[:, K // 2:])
    return y.contiguous()


@functools.lru_cache(maxsize=None)
def mutant_case():
    """-> go, w, y, bounds of MUTANT_SHAPE, iid, with a mask that holds exact zeros (about half of it) and one NaN."""
    go, w, y, bounds = split_dgrad_case(MUTANT_SHAPE, "iid")
    assert bool((y == 0).any()) and bool(torch.isnan(y).any()) and bool((y > 0).any())
    return go, w, y, bounds


# ------------------------------------------------------------------------------------------------ exact family
@functools.lru_cache(maxsize=None)
def exact_dgrad_inputs():
    """-> go, the layer's weight w, and the three-term / full / hi-hi values (float64) its data gradient of go must be / must differ
    from: go and w' are wino_split_cases.split_exact_inputs, w = w'.transpose(0, 1).flip(2, 3)."""
    x, wp = ws.split_exact_inputs()
    three, full, hh = ws.split_exact_reference(x, wp)
    return x, wp.transpose(0, 1).flip(2, 3).contiguous(), three, full, hh


# ------------------------------------------------------------------------------------------------ non-finite contract
def nonfinite_masked_case(case):
    """-> x, w, b of wino_split_cases.split_nonfinite_case(case) (an input defect), a mask that is zero at the defect and one
    elsewhere, and the bound of the `none` epilogue on the masked input: a NaN or an infinity behind a zero of the mask does not reach
    the result."""
    assert case in ("nan_input", "inf_input")
    x, w, b, _, _ = ws.split_nonfinite_case(case)
    mask = torch.ones_like(x)
    mask[~torch.isfinite(x)] = 0.0
    clean = torch.ops.aten.threshold_backward(x, mask, 0)
    assert bool(torch.isfinite(clean).all()) and not bool(torch.isfinite(x).all())
    return x, w, b, mask, ws.split_bounds(clean, w, b, what="wg split masked " + case)["none"]


# ------------------------------------------------------------------------------------------------ the route through a network
def route_bound(x, w, bias, epilogue, mask, data_gradient, what=""):
    """The bound of ONE recorded call of ops.conv3x3_wg_split_frozen through the layer whose own weight is w [K, C, 3, 3]."""
    x, w = x.cpu(), w.cpu()
    if data_gradient:
        if mask is not None:
            x = torch.ops.aten.threshold_backward(x, mask.cpu(), 0)
        return split_dgrad_bound(x, w, what=what)
    b = torch.zeros(w.shape[0]) if bias is None else bias.cpu()
    if epilogue in ("none", "bias") or w.shape[0] % 2:
        return ws.split_bounds(x, w, b, what=what)[epilogue]
    return split_epilogue_bounds(x, w, b, what=what)[epilogue]


# ------------------------------------------------------------------------------------------------ sizes
def weights_bytes(rows, reduction):
    """ffwm_conv3x3_wg_split_weights_bytes(rows, reduction): a hi and a lo bf16 per entry, the reduction rounded up to 32."""
    return 16 * ((reduction + 31) // 32 * 32) * rows * 4


def workspace_bytes(B, C, H, W, K):
    """ffwm_conv3x3_wg_split_workspace_bytes: V (4 bytes per entry) and fp32 M, both with the 128 tile's padding."""
    T = (B * ((H + 1) // 2) * ((W + 1) // 2) + 127) // 128 * 128
    return 16 * T * ((C + 31) // 32 * 32 + (K + 127) // 128 * 128) * 4
