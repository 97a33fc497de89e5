"""Cases and per-element bounds for the batched-GEMM Winograd route (csrc/conv_winograd_gemm.hip), shared by the CPU restatement
(test_wino_gemm_cpu.py) and the kernel tests (test_gpu_wino_gemm_bounds.py).  A plain helper module, not a conftest.

The data flow -- V = B^T d B [16, C, T], U = G w G^T [16, K, C], 16 GEMMs M_p = U_p V_p, y = A^T M A, the epilogue -- has the
roundings conv_bounds.py derives for conv_winograd.hip with splits = 1: two in V, four in U, one fma chain over C in any order, four
in the output transform.  So: forward rho_winograd(C) on mag_patch, data gradient rho_winograd(K) (mode 3).  The max-feature-map
epilogue takes max(a, b) of two output channels; max is 1-Lipschitz in each argument, so |max(a', b') - max(a, b)| <=
max(|a' - a|, |b' - b|) <= rho max(mag_a, mag_b).  ReLU is 1-Lipschitz and exact.  The ReLU mask of the data gradient is an exact
selection of grad_output elements (aten::threshold_backward), applied to the reference's input."""
import functools

import torch

import conv_bounds as cb

# (B, C, H, W, K): odd planes and a tile tail; the C and K tails of both GEMM tiles (64, 128) and of the 16-channel stage; a one-tile
# plane; more than one GEMM tile per axis; more than one stage of the reduction.
SHAPES = [(2, 19, 7, 9, 70), (3, 40, 5, 6, 36), (1, 8, 2, 2, 64), (1, 64, 32, 32, 64), (2, 130, 12, 12, 200)]
TILES = (64, 128)


def _seed(shape, kind):
    return 1000 * SHAPES.index(shape) + 17 * cb.FAMILIES.index(kind) + 5


def relu_bound(pre, what):
    """ReLU behind the bound `pre` of conv + bias: 1-Lipschitz and exact.  torch.relu, as csrc/mfm.hip's bias + ReLU has it: NaN stays
    NaN and -inf becomes 0 (conv_bounds' "relu" is LeakyReLU with slope 0, whose -inf x 0 is NaN: the rule of conv_winograd.hip's
    fused activation, not of the launch this epilogue replaces)."""
    return cb.Bound(torch.relu(pre.ref), pre.mag, pre.rho, 0.0, pre.exact, what)


@functools.lru_cache(maxsize=None)
def forward_case(shape, kind):
    """-> x, w, b (float32 CPU) and the bounds of the three epilogues {"none", "relu", "mfm"}."""
    B, C, H, W, K = shape
    small = C > 64
    exact = kind == "integers"
    s = _seed(shape, kind)
    x = cb.activations(kind, (B, C, H, W), s, small)
    w, b = cb.weights(kind, (K, C, 3, 3), s + 1, small=small)
    rho = cb.rho_winograd(C)
    what = "wg fwd %s %s" % (shape, kind)
    none = cb.forward_bound(x, w, None, rho=rho, winograd=True, exact=exact, what=what + " none")
    pre = cb.forward_bound(x, w, b, rho=rho, winograd=True, exact=exact, what=what + " bias")
    relu = relu_bound(pre, what + " bias+relu")
    h = K // 2
    mfm = cb.Bound(torch.maximum(pre.ref[:, :h], pre.ref[:, h:]), torch.maximum(pre.mag[:, :h], pre.mag[:, h:]), rho, 0.0, exact,
                   what + " bias+mfm")
    return x, w, b, {"none": none, "relu": relu, "mfm": mfm}


@functools.lru_cache(maxsize=None)
def dgrad_case(shape, kind):
    """-> go [B, K, H, W], the layer's w [K, C, 3, 3], a ReLU output y of go's shape (zeros, positives, one NaN that lets the
    gradient pass), and the bounds {False: plain, True: masked} of d(input) [B, C, H, W]."""
    B, C, H, W, K = shape
    small = K > 64
    exact = kind == "integers"
    s = _seed(shape, kind) + 500
    go = cb.grad_outputs(kind, (B, K, H, W), s, small)
    w, _ = cb.weights(kind, (K, C, 3, 3), s + 1, out_dim=1, small=small)
    y = torch.relu(torch.randn((B, K, H, W), generator=torch.Generator().manual_seed(s + 2)))
    y[0, 0, 0, 0] = float("nan")
    rho = cb.rho_winograd(K)
    what = "wg dgrad %s %s" % (shape, kind)
    plain = cb.forward_bound(go, w, None, mode=3, rho=rho, winograd=True, exact=exact, what=what)
    masked_go = torch.ops.aten.threshold_backward(go, y, 0)
    masked = cb.forward_bound(masked_go, w, None, mode=3, rho=rho, winograd=True, exact=exact, what=what + " relu mask")
    return go, w, y, {False: plain, True: masked}


# ------------------------------------------------------------------------------------------------ the data flow in torch fp32
def wg_flow_f32(x, w, b=None, epilogue="none", data_gradient=False, mask=None):
    """Exactly the kernels' data flow and index maps, every step in x.dtype: tile t = (b, ty, tx) row-major, position p = 4 i + j."""
    if mask is not None:
        x = torch.where(mask <= 0, torch.zeros_like(x), x)
    if data_gradient:
        w = w.transpose(0, 1).flip(2, 3).contiguous()
    B, C, H, W = x.shape
    K = w.shape[0]
    bt, g, at = cb._BT.to(x.dtype), cb._G.to(x.dtype), cb._AT.to(x.dtype)
    P = cb._patches(x)                                              # [B, C, TH, TW, 4, 4]
    TH, TW = P.shape[2], P.shape[3]
    T = B * TH * TW
    V = (bt @ P @ bt.t()).permute(4, 5, 1, 0, 2, 3).reshape(16, C, T)
    U = (g @ w @ g.t()).permute(2, 3, 0, 1).reshape(16, K, C)
    M = torch.bmm(U, V)                                             # [16, K, T]
    M = M.reshape(4, 4, K, B, TH, TW).permute(3, 2, 4, 5, 0, 1)     # [B, K, TH, TW, 4, 4]
    Y = at @ M @ at.t()                                             # [B, K, TH, TW, 2, 2]
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, K, 2 * TH, 2 * TW)[:, :, :H, :W]
    if epilogue != "none" and b is not None:
        y = y + b.view(1, -1, 1, 1)
    if epilogue == "relu":
        y = torch.relu(y)
    elif epilogue == "mfm":
        y = torch.maximum(y[:, :K // 2], y[:, K // 2:])
    return y.contiguous()
