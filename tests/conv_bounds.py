"""Per-element float64 error bounds and exact-integer cases for the convolution kernels (a plain helper module, not a conftest).

One convolution output -- forward, data gradient, weight gradient, bias gradient -- is a sum of products per element.  For every
element, with u = 2^-24:

  ref  ATen's float64 result (F.conv2d, F.conv_transpose2d, torch.nn.grad.conv2d_input, aten.convolution_backward) plus bias,
       then the activation;
  mag  the same operation on |x|, |w|, |grad_output| with |bias| added: sum_i |a_i b_i|, the condition number of the element's sum;

and the assertion, on every element whose mag is finite:

    |got - ref| <= rho mag + post u |ref| + 1e-38,

elements with a non-finite reference non-finite in the result too.  (An element whose reference is finite and whose mag is not
lies inside the reach of a non-finite input of a transform-domain kernel -- the 4 x 4 patch of a Winograd tile -- and is free.)
LeakyReLU / ReLU / tanh are 1-Lipschitz, so the bound of the pre-activation passes through them; `post` is the rounding of the
activation itself (LeakyReLU: one product, 1; tanhf: 4 ulps of a value below 1).

Which mag a kernel gets
  * direct kernels (conv_fwd.hip modes 0-3, conv_wgrad.hip, conv_bwd.hip, the thin kernels of flownet_ops.hip): the plain mag.
    Taps that fall into the padding, and the structural zeros of a parity class, contribute exact zeros.
  * conv_winograd.hip (F(2x2, 3x3), forward and data gradient): the input transform B^T d B mixes the 4 x 4 patch of a 2 x 2 output
    tile, so the products of one element are not bounded by its own 9 taps' inputs:
        mag_patch[b, k, y, x] = sum_c (max |x_c| over the 4 x 4 patch of the element's tile) * (sum of |w_kc| over the 9 taps) + |bias_k|,
    which is >= the plain mag everywhere (so "the larger of the two" is mag_patch itself).  The thin-tail and image-head kernels of
    the same file are direct; they are held to the same bound (their rho below is smaller than the Winograd one).
  * conv_wgrad_wino.hip (Winograd-domain weight gradient): per (k, c) and for all 9 taps
        mag_patch[k, c] = sum_{b, tile} (max |x_c| over the tile's 4 x 4 patch) * (sum of |grad_output_k| over the tile's 2 x 2 pixels).

Where rho comes from.  Every kernel here uses fp32 fma only: products are exact inside the fma, each accumulation step rounds once
relative to the partial sum, and every partial sum of terms a_i b_i is at most sum |a_i b_i| = mag.  Hence
  (S) a sum of n terms in ANY order (chain, tree, MFMA k-pairs, lanes of a wave) errs by at most n u mag;
  (B) a sum cut into P partial sums whose longest sequential chain has L terms, the partial sums meeting by atomics or a reduce pass
      in any order, errs by at most (L + P) u mag.
These are worst cases (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), not fits: typical errors are ~sqrt(n) u.  Nothing
sharper that holds for every input can be argued for a chain, so n u it is.  One safety factor, SAFETY = 4, multiplies all of them.
  * conv_fwd.hip, every mode: the reduction is C x taps (9, 16, or the 4 taps of a parity class for modes 1 / 2; mode 3: 9), walked
    as ONE fma chain per slice (v_mfma_f32_32x32x2f32 over chunks of 32-36 steps), `splitk` slices added in slot order, then bias:
    (S) with n = C taps + splitk + 1.                                                             rho = 4 (C taps + splitk + 1) u
  * thin kernels (flow_head: C x 9 terms + bias, tanh; flow_up: 2 x 4 + bias; conv_thin: C x 9 + bias): (S).  rho = 4 (n + 1) u
  * conv_winograd.hip: V = B^T d B has entries sum of 4 inputs (|V| <= 4 X_c, 2 roundings), U = G w G^T entries 0, +-1, +-1/2
    (|U_ij| <= sum |w| =: G_kc, 4 roundings), M_ij = sum_c U_ij V_ij one fma chain over C (8-channel MFMA chunks) cut into `splits`
    atomically added pieces: |dM_ij| <= (C + splits + 6) u sum_c 4 X_c |U_ij|; the output transform A^T M A adds 9 of the 16 M_ij with
    4 roundings, and sum over those 9 positions of |U_ij| <= 4 G_kc.  Together |dY| <= 16 (C + splits + 10) u mag_patch, + 1 for the bias.
                                                                                      rho = 4 x 16 (C + splits + 11) u
  * conv_wgrad.hip (direct, packed, swapped-packed): a workgroup walks ceil(steps / nsplit) row steps of 64 pixels with one chain per
    accumulator (steps = B (W / 64) H, nsplit = min(256 / tiles, steps / 4) as launch_wgrad computes it) and adds its tile by atomics;
    the bias gradient is summed by the same workgroups: (B) with L = 64 ceil(steps / nsplit), P = nsplit, + 1 for `+=`.
  * conv_bwd.hip generic / tiled: chunks of 32 pixels, `chunks` per slice as the entry points compute them, slices meet by atomics
    (tiled, unsliced: one chain over all pixels): (B) with L = 32 chunks, P = slices.  The tile-shape search of the tiled entry only
    changes P between 1 and its maximum; the bound takes the worst of the candidates.
  * conv_wgrad_wino.hip: V as above (|V| <= 4 X), Z = A dY A^T (|Z| <= S, 2 roundings), M_ij one chain over the slice's tiles
    (chunks of 8 tiles, nsplit = min(256 / tiles, chunks / 16) slices by atomics), dW = G^T M G with sum |coefficient| <= 4 per side
    and 4 roundings: |d dW| <= 16 (L + P + 8) u mag_patch with L = 8 ceil(chunks / nsplit).            rho = 4 x 16 (L + P + 9) u

Exact cases (family `integers`).  With integer inputs all of the above is exact as long as every partial sum is representable:
direct kernels need mag < 2^24; the Winograd kernels hold quarter-integers up to 16 mag_patch (x 4 input transform x 4 for the 9
summed positions / the two-sided G), i.e. numerators up to 64 mag_patch < 2^24.  `require_exact` proves that in float64 or raises;
then the assertion is torch.equal(got, ref.float()).

The fp32 stand-ins of tests/test_conv_bounds_cpu.py (ATen's fp32 CPU kernels, a torch emulation of F(2x2, 3x3), a chunked sum in
reversed order) meet every bound with rho / 4 and the integer family exactly.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
SAFETY = 4.0
FLOOR = 1e-38
EXACT_LIMIT = 2.0 ** 24


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ rho per kernel
def rho_any_order(n_terms, extra=1):
    """(S): n terms in any order, + extra roundings (bias, +=)."""
    return SAFETY * (n_terms + extra) * U32


def rho_blocked(chain, partials, extra=1):
    """(B): longest chain + number of partial sums, + extra roundings."""
    return SAFETY * (chain + partials + extra) * U32


def rho_conv_fwd(C, taps, splitk=1):
    return rho_any_order(C * taps + splitk, 1)


def rho_winograd(C, splits=1):
    return SAFETY * 16 * (C + splits + 11) * U32


def wgrad3x3_structure(B, C, K, H, W):
    """(L, P) of conv_wgrad.hip: the worst of its three launches (full 64-tiles, packed remainder columns, swapped packed rows)."""
    def thin(n):
        r = n % 64
        return n if n <= 3 else (r if (n > 64 and 0 < r <= 3) else 0)
    km, cm = K - thin(K), C - thin(C)
    steps = B * (W // 64) * H
    worst = (0, 0)
    launches = []
    if km > 0 and cm > 0:
        launches.append(_ceil_div(km, 64) * _ceil_div(cm, 64))
    if cm < C:
        launches.append(_ceil_div(K, 128))
    if km < K and cm > 0:
        launches.append(_ceil_div(cm, 128))
    for tiles in launches:
        nsplit = 1 if tiles >= 256 else 256 // tiles
        if nsplit > steps // 4:
            nsplit = max(steps // 4, 1)
        L, P = 64 * _ceil_div(steps, nsplit), nsplit
        if L + P > sum(worst):
            worst = (L, P)
    return worst


def rho_wgrad3x3(B, C, K, H, W, accumulate=False):
    L, P = wgrad3x3_structure(B, C, K, H, W)
    return rho_blocked(L, P, 2 if accumulate else 1)


def wgrad_wino_structure(B, C, K, H, W):
    """(L in tiles, P) of conv_wgrad_wino.hip (launch_wgrad_wino)."""
    tiles = _ceil_div(K, 64) * _ceil_div(C, 64)
    chunks = B * (H // 2) * (W // 16)
    nsplit = 1 if tiles >= 256 else 256 // tiles
    nsplit = max(min(nsplit, chunks // 16), 1)
    return 8 * _ceil_div(chunks, nsplit), nsplit


def rho_wgrad_wino(B, C, K, H, W, accumulate=False):
    L, P = wgrad_wino_structure(B, C, K, H, W)
    return SAFETY * 16 * (L + P + 9 + (1 if accumulate else 0)) * U32


def rho_wgrad_generic(B, K, P_out, N_cols):
    """conv_bwd.hip generic: every image's plane padded to chunks of 32 pixels; slices of >= 4 chunks towards 1024 workgroups."""
    total = B * _ceil_div(P_out, 32)
    tiles = _ceil_div(N_cols, 64) * _ceil_div(K, 64)
    slices = max(min(_ceil_div(1024, tiles), total // 4), 1)
    per = _ceil_div(total, slices)
    return rho_blocked(32 * per, _ceil_div(total, per), 1)


def rho_wgrad_tiled(B, K, P_out, N_cols, unsliced=False, target=512):
    """conv_bwd.hip tiled: pixels linearised over the batch; the worst (L + P) over the four tile shapes the entry chooses from."""
    total = _ceil_div(B * P_out, 32)
    worst = 0
    for cm in (1, 2):
        for cn in (1, 2):
            tiles = _ceil_div(K, 64 * cm) * _ceil_div(N_cols, 64 * cn)
            sl = 1 if (tiles >= target or unsliced) else max(min(target // tiles, total // 4), 1)
            per = _ceil_div(total, sl)
            worst = max(worst, 32 * per + _ceil_div(total, per))
    return SAFETY * (worst + 1) * U32


# ------------------------------------------------------------------------------------------------ the yardstick
class Bound:
    """ref / mag of one output (float64 CPU tensors of its shape), its rho, and the activation's own ulps."""

    def __init__(self, ref, mag, rho, post=0.0, exact=False, what=""):
        self.ref, self.mag, self.rho, self.post, self.exact, self.what = ref, mag, rho, post, exact, what

    def measure(self, got, rho=None):
        """-> (max error / bound over the elements with finite mag, number of wrongly (non-)finite elements, index of the worst)."""
        rho = self.rho if rho is None else rho
        got = got.detach().to("cpu", torch.float64)
        assert got.shape == self.ref.shape, (tuple(got.shape), tuple(self.ref.shape))
        fin_ref = torch.isfinite(self.ref)
        strict = torch.isfinite(self.mag) & fin_ref
        wrong = int((~torch.isfinite(got) & strict).sum()) + int((torch.isfinite(got) & ~fin_ref).sum())
        err = (got - self.ref).abs()
        bound = rho * self.mag + self.post * U32 * self.ref.abs() + FLOOR
        q = torch.where(strict, err / bound, torch.zeros_like(err))
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        if q.numel() == 0:
            return 0.0, wrong, ()
        flat = int(q.argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), q.shape))
        return float(q.max()), wrong, idx

    def describe(self, idx):
        """Where the worst element sits: channel, 64-channel tile, 8-channel chunk, 2 x 2 tile and parity class."""
        if len(idx) != 4:
            return "index %s" % (idx,)
        a, ch, y, x = idx
        return "index %s: channel %d (64-tile %d, chunk %d), 2x2 tile (%d, %d), parity (%d, %d)" % (idx, ch, ch // 64, ch // 8, y // 2, x // 2, y & 1, x & 1)

    def check(self, got, what="", rho=None):
        ratio, wrong, idx = self.measure(got, rho)
        what = what or self.what
        print("CONVBOUND %s: error/bound %.3g wrong_nonfinite %d at %s" % (what, ratio, wrong, self.describe(idx)))
        assert wrong == 0, "%s: %d elements non-finite where the reference is not, or the other way round" % (what, wrong)
        assert ratio <= 1.0, "%s: per-element error / bound = %.3g at %s (got %r, ref %r)" % (
            what, ratio, self.describe(idx), float(got.detach().cpu()[idx]), float(self.ref[idx]))
        if self.exact:
            g = got.detach().cpu()
            same = torch.equal(g, self.ref.float())
            if not same:
                bad = (g != self.ref.float()).nonzero()
                raise AssertionError("%s: integer case not bit-exact: %d elements differ, first at %s" % (what, bad.shape[0], tuple(int(i) for i in bad[0])))
        return ratio


def global_close(got, ref, tol, scale=1.0):
    """The old yardstick of tests/test_gpu_parity.py: max|got - ref| <= tol (1 + max|ref|) scale."""
    got = got.detach().to("cpu", torch.float64)
    return float((got - ref).abs().max()) <= tol * (1 + float(ref.abs().max())) * scale


def require_exact(mag, amplification=1.0, what=""):
    """Prove an integer case well-formed: the largest possible partial sum (x amplification) stays below 2^24."""
    m = float(mag.max()) * amplification
    if not (m < EXACT_LIMIT):
        raise ValueError("%s: integer case too large to be exact in fp32: %g x %g >= 2^24" % (what, float(mag.max()), amplification))


# ------------------------------------------------------------------------------------------------ Winograd magnitudes
def tile_max(a):
    """[B, C, H, W] -> the max of a (non-negative) over the 4 x 4 patch of every 2 x 2 tile, [B, C, ceil(H/2), ceil(W/2)]."""
    return F.max_pool2d(F.pad(a, (1, 2, 1, 2)), 4, 2)[:, :, :(a.shape[2] + 1) // 2, :(a.shape[3] + 1) // 2]


def tile_sum(a):
    H, W = a.shape[2], a.shape[3]
    return F.avg_pool2d(F.pad(a, (0, W & 1, 0, H & 1)), 2, 2) * 4


def patch_mag_forward(x, g_kc, bias=None):
    """sum_c tile_max(|x_c|) G_kc (+ |bias|) at every pixel; g_kc [K_out, C_in] = the taps' sum of |w|."""
    B, C, H, W = x.shape
    X = tile_max(x.abs().double())
    m = torch.einsum("bchw,kc->bkhw", X, g_kc.double())
    m = m.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :H, :W]
    if bias is not None:
        m = m + bias.abs().double().view(1, -1, 1, 1)
    return m.contiguous()


def patch_mag_wgrad(x, go):
    X = tile_max(x.abs().double())
    S = tile_sum(go.abs().double())
    return torch.einsum("bkhw,bchw->kc", S, X)[:, :, None, None].expand(-1, -1, 3, 3).contiguous()


# ------------------------------------------------------------------------------------------------ references
def _act(t, act, slope):
    if act in (None, 0, "none"):
        return t, 0.0
    if act in (1, "lrelu", "relu"):
        s = 0.0 if act == "relu" else slope
        return F.leaky_relu(t, s), (0.0 if s == 0.0 else 1.0)
    if act in (2, "tanh"):
        return torch.tanh(t), 4.0
    raise ValueError(act)


def _forward64(x, w, b, stride, pad, mode, out_hw=None):
    if mode == 0:
        return F.conv2d(x, w, b, stride, pad)
    if mode == 1:
        return F.conv_transpose2d(x, w, b, stride, pad)
    B, _, H, W = x.shape
    shape = (B, w.shape[1]) + ((2 * H, 2 * W) if mode == 2 else (H, W))
    y = torch.nn.grad.conv2d_input(shape, w, x, stride, pad)
    return y if b is None else y + b.view(1, -1, 1, 1)


def forward_bound(x, w, b=None, stride=1, pad=1, mode=0, act=None, slope=0.2, rho=None, winograd=False, exact=False, what=""):
    """Forward / data gradient as conv_fwd.hip's modes name them: 0 Conv2d, 1 ConvTranspose2d(4, 2, 1) (w [C, K, 4, 4]),
    2 / 3 d(input) of Conv2d(3, 2, 1) / Conv2d(3, 1, 1) (x = grad_output, w = the layer's own [K_layer, C_layer, 3, 3]).
    winograd: mag_patch (modes 0 and 3 at 3x3 / stride 1 only)."""
    xd, wd = x.double().cpu(), w.double().cpu()
    bd = None if b is None else b.double().cpu()
    pre = _forward64(xd, wd, bd, stride, pad, mode)
    ref, post = _act(pre, act, slope)
    if winograd:
        g = wd.abs().sum((2, 3))
        mag = patch_mag_forward(xd, g if mode == 0 else g.t(), bd)
    else:
        mag = _forward64(xd.abs(), wd.abs(), None if bd is None else bd.abs(), stride, pad, mode)
    if exact:
        require_exact(mag[torch.isfinite(mag)], 64.0 if winograd else 1.0, what)
    return Bound(ref, mag, rho, post, exact, what)


def wgrad_bounds(x, go, kernel, stride, pad, transposed=False, rho=None, rho_bias=None, winograd=False, exact=False, what="", init=None):
    """-> (Bound of grad_weight, Bound of grad_bias) of Conv2d (weight [K, C, k, k]) or ConvTranspose2d (weight [Ci, Co, 4, 4]; x =
    the layer's input, go = its grad_output).  init: what grad_weight held before an accumulating (+=) call."""
    xd, gd = x.double().cpu(), go.double().cpu()
    wshape = (xd.shape[1], gd.shape[1], kernel, kernel) if transposed else (gd.shape[1], xd.shape[1], kernel, kernel)

    def run(a, g):
        return torch.ops.aten.convolution_backward(g, a, torch.zeros(wshape, dtype=torch.float64), None, [stride, stride], [pad, pad], [1, 1],
                                                   transposed, [0, 0], 1, [False, True, False])[1]
    ref, mag = run(xd, gd), run(xd.abs(), gd.abs())
    if winograd:
        mag = patch_mag_wgrad(xd, gd)
    if init is not None:
        ref, mag = ref + init.double().cpu(), mag + init.double().cpu().abs()
    bref, bmag = gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3))
    if exact:
        require_exact(mag[torch.isfinite(mag)], 64.0 if winograd else 1.0, what)
        require_exact(bmag[torch.isfinite(bmag)], 1.0, what)
    return (Bound(ref, mag, rho, 0.0, exact, what + " grad_weight"),
            Bound(bref, bmag, rho if rho_bias is None else rho_bias, 0.0, exact, what + " grad_bias"))


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("iid", "in_scales", "out_scales", "concat", "mean", "spike", "zero_channels", "nonfinite", "integers")
SOME_FAMILIES = tuple(f for f in FAMILIES if f not in ("iid", "integers"))


def channel_exponents(n):
    """Powers of two over 2^-12 .. 2^12 that differ inside every 8-channel chunk, 64-channel tile and in a thin remainder."""
    return ((torch.arange(n) * 5) % 25 - 12).double()


def _spike_positions(H, W):
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (min(1, H - 1), min(2, W - 1)), (H // 2, max(W // 2 - 1, 0)),
           (max(H // 2 - 1, 0), W // 2), (H - 1, W // 2)]
    return pos


def activations(kind, shape, seed, small=False):
    """The activation-like operand of a family (an input, or a grad_output), float32 [B, C, H, W]."""
    gen = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    x = torch.randn(shape, generator=gen)
    if kind in ("iid", "out_scales"):
        pass
    elif kind == "in_scales":
        x = x * torch.exp2(channel_exponents(C)).float().view(1, C, 1, 1)
    elif kind == "concat":
        s = torch.ones(C)
        s[C // 3:(2 * C) // 3] = 1e-3
        s[(2 * C) // 3:] = 30.0
        s[-2:] = 1e3                                  # the two flow channels at the end of FlowNet's concatenations
        x = x * s.view(1, C, 1, 1)
    elif kind == "mean":
        x = 64.0 + x * 2.0 ** -6
    elif kind == "spike":
        x = x * 1e-3
        for i, (py, px) in enumerate(_spike_positions(H, W)):
            x[i % B, (7 * i + 1) % C, py, px] = 1e4 * (-1) ** i
    elif kind == "zero_channels":
        x[:, 1::5] = 0
    elif kind == "nonfinite":
        x[0, 1 % C, H // 2, W // 2] = float("nan")
        x[B - 1, (C - 1), min(1, H - 1), W - 1] = float("inf")
    elif kind == "integers":
        r = 1 if small else 3
        x = torch.randint(-r, r + 1, shape, generator=gen).float()
    else:
        raise ValueError(kind)
    return x.contiguous()


def weights(kind, shape, seed, out_dim=0, small=False):
    """The weight of a family, float32 [K, C, k, k] (out_dim 0) or [C, K, k, k] (out_dim 1: ConvTranspose2d / data gradients), with
    its bias [K]."""
    gen = torch.Generator().manual_seed(seed)
    K = shape[out_dim]
    fan = shape[1 - out_dim] * shape[2] * shape[3]
    w = torch.randn(shape, generator=gen) / fan ** 0.5
    b = torch.randn(K, generator=gen)
    view = [1, 1, 1, 1]
    view[out_dim] = K
    if kind == "out_scales":
        s = torch.exp2(channel_exponents(K)).float()
        w, b = w * s.view(view), b * s
    elif kind == "zero_channels":
        z = torch.zeros(K, dtype=torch.bool)
        z[2::7] = True
        w = torch.where(z.view(view), torch.zeros_like(w), w)
        b = torch.where(z, torch.zeros_like(b), b)
        w[:, :, 0, shape[3] - 1] = 0                  # a whole tap
    elif kind == "integers":
        r = 1 if small else 3
        w = torch.randint(-r, r + 1, shape, generator=gen).float()
        b = torch.randint(-3, 4, (K,), generator=gen).float()
    elif kind not in FAMILIES:
        raise ValueError(kind)
    return w.contiguous(), b.contiguous()


def grad_outputs(kind, shape, seed, small=False):
    """The grad_output of a weight-gradient case: the family's output-channel structure on an activation-like tensor."""
    B, K, H, W = shape
    if kind == "out_scales":
        return (activations("iid", shape, seed) * torch.exp2(channel_exponents(K)).float().view(1, K, 1, 1)).contiguous()
    if kind == "zero_channels":
        g = activations("iid", shape, seed)
        g[:, 2::7] = 0
        return g
    if kind == "integers":
        return activations("integers", shape, seed, small)
    if kind in ("spike", "mean", "concat"):
        return activations(kind, shape, seed)
    return activations("iid", shape, seed) * 0.1


# ------------------------------------------------------------------------------------------------ fp32 Winograd F(2x2, 3x3) in torch
_BT = torch.tensor([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
_G = torch.tensor([[1., 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
_AT = torch.tensor([[1., 1, 1, 0], [0, 1, -1, -1]])


def _patches(x):
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1 + (W & 1), 1, 1 + (H & 1)))
    return xp.unfold(2, 4, 2).unfold(3, 4, 2)              # [B, C, TH, TW, 4, 4]


def winograd_forward_f32(x, w, b=None):
    """Conv2d(C, K, 3, 1, 1) by F(2x2, 3x3), every step in `x.dtype` arithmetic."""
    B, C, H, W = x.shape
    bt, g, at = _BT.to(x.dtype), _G.to(x.dtype), _AT.to(x.dtype)
    V = bt @ _patches(x) @ bt.t()
    Uw = g @ w @ g.t()
    M = torch.einsum("bcthij,kcij->bkthij", V, Uw)
    Y = at @ M @ at.t()                                     # [B, K, TH, TW, 2, 2]
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, w.shape[0], Y.shape[2] * 2, Y.shape[3] * 2)[:, :, :H, :W]
    return (y if b is None else y + b.view(1, -1, 1, 1)).contiguous()


def winograd_dgrad_f32(go, w):
    """d(input) of Conv2d(C, K, 3, 1, 1): the same transform with the weight transposed and rotated."""
    return winograd_forward_f32(go, w.transpose(0, 1).flip(2, 3).contiguous())


def winograd_wgrad_f32(x, go):
    """grad_weight [K, C, 3, 3] in the Winograd domain: G^T [sum (B^T d B) . (A dY A^T)] G (even H, W)."""
    B, K, H, W = go.shape
    bt, g, at = _BT.to(x.dtype), _G.to(x.dtype), _AT.to(x.dtype)
    V = bt @ _patches(x) @ bt.t()
    T = go.unfold(2, 2, 2).unfold(3, 2, 2)                  # [B, K, TH, TW, 2, 2]
    Z = at.t() @ T @ at
    M = torch.einsum("bkthij,bcthij->kcij", Z, V)
    return (g.t() @ M @ g).contiguous()
