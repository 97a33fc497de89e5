"""Float64 error bound, exact family, non-finite contract and torch restatement of the split batched-GEMM Winograd route
(ffwm_conv3x3_wg_split_forward, csrc/conv_winograd_gemm_split.hip): a plain helper module, not a conftest.

Conventions of conv_bounds.py / colmax_split_bounds.py: every reference is float64 ATen on the CPU, computed from what the kernel is
GIVEN (F.conv2d of the float32 input, weight and bias); u = 2^-24; SAFETY = 4 multiplies every count of roundings; no constant is
fitted.

The kernel.  V = B^T d B [16, C, T] and U = G w G^T [16, K, C] are computed in fp32 exactly as the fp32 route computes them
(wino_gemm_cases.wg_flow_f32).  Every entry x of U and V is then split in two bf16 terms, hi = bf16_rn(x), lo = bf16_rn(x - hi), and
M_p[k, t] = sum_c (Ul Vh + Uh Vl + Uh Vh) is formed on v_mfma_f32_32x32x16_bf16 in one fp32 accumulator.  y = A^T M A in fp32, then
bias and LeakyReLU.

Derivation, per output element, with X_c = max |x_c| over the 4 x 4 patch of the element's tile, G_kc = sum of |w_kc| over the taps:
  * U and V carry the roundings of the fp32 route (conv_bounds.py): |U| <= G_kc with four roundings, |V| <= 4 X_c with two.  To
    first order that is 6 u |U V| per product.
  * The split (colmax_split_bounds.py): |x - hi - lo| <= 2^-18 |x|, |hi| <= (1 + 2^-9) |x|, |lo| <= 2^-9 (1 + 2^-9) |x|; the terms the
    kernel never forms, Ul Vl + eU V + (U - eU) eV, are at most 3 x 2^-18 (1 + 2^-8) |U V| <= TRUNC |U V|, TRUNC = 2^-16, per product.
  * The 3 C partial products of one M entry are exact in fp32 (8 x 8 significand bits).  The ISA documents neither the order nor the
    internal width in which the instruction adds its 16 products to the accumulator: they are charged as 3 C roundings in any order
    (rule (S)) on sum |terms| <= MAG sum |U V|, MAG = 1 + 2^-6 (which also covers the (1 + 6 u) of the computed U, V under TRUNC).
  * The output transform adds 9 of the 16 M_p with four roundings, and the bias one.
  * The products of one output element: sum over its 9 positions of |U_p| <= 4 G_kc, |V_p| <= 4 X_c: 16 mag_patch, as rho_winograd.
  Counting: (3 C) + 6 + 4 + 1 = 3 C + 11 roundings.  The final result is one fp32 number: its own
  representation and the LeakyReLU product are charged on |ref|, (SAFETY + post) u |ref|.
Underflow, stated, not silent (ETA of colmax_split_bounds.py, per position): a bf16 term, a product or a partial sum below 2^-126 may
  be flushed to zero; per channel and position at most the four operand terms, each costing 2^-126 times the other operand's
  magnitude with (1 + 2^-9) <= 1.5 folded in, and 3 C products and 3 C partial sums of 2^-126 each, 16 positions at most:
      eta = 2^-126 x 16 (3 sum_c (4 X_c + G_kc) + 6 C)
Together
      |got - ref| <= 16 (TRUNC MAG + SAFETY (3 C + 11) u MAG) mag_patch + (SAFETY + post) u |ref| + eta.
  At C = 64: 1.0e-3 mag_patch (SAFETY = 1: 4.4e-4), against 2.9e-4 of the fp32 route.  LeakyReLU is 1-Lipschitz.

Non-finite contract.  An infinite entry of U or V has hi = inf, lo = bf16(inf - inf) = NaN: an infinity in the input or a weight
  behaves as a NaN over the reach of its 4 x 4 patch / in its output channel.  conv_bounds.Bound already frees the elements inside
  the reach of a non-finite input (mag_patch is not finite there) and wants them non-finite where the reference is; a NaN result is
  that.  Finite |x| >= 2^125 is outside the contract (V sums four inputs, hi may round to infinity): split_case raises.

Exact family.  The bound alone cannot see a dropped lo term on random data (a single-bf16 product errs by ~2^-9 / sqrt(n) of the
  magnitude, below 16 x 2^-16).  Sparse inputs and weights whose non-zeros are +-(1 + q 2^-10) 2^e (q = 1..3, e = -1..1), so that hi
  = +-2^e and lo = +-q 2^(e-10) are exact and non-zero:
    input: pixels on a grid of pitch 4 (no 4 x 4 patch holds two of them), at each of them at most four non-zero channels -- every
      entry of V is then 0 or +- one input value, without a rounding, and an output element sums at most four products;
    weight: one non-zero tap per (k, c): every entry of U is the tap times 1, 1/2 or 1/4, without a rounding.
  The hi terms of V are multiples of 2^-1 and its lo terms of 2^-11, those of U of 2^-3 and 2^-13; the kernel never forms lo lo, so
  every product it forms (Ul Vh, Uh Vl, Uh Vh), every partial sum in any order, M and the sums of the output transform are multiples of
  Q = 2^-14, and split_exact_reference shows the sum of the magnitudes of ALL terms of one output element below 2^24 Q: every partial
  sum is exact, so the kernel's value is EXACTLY the three-term value.  (The full product holds multiples of 2^-24: it need not be a
  float32 number at all.)  The
  grid starts at pixel (0, 0) of the first image and is shifted to reach pixel (H - 1, W - 1) of the last; every output channel
  carries weights (both halves of the MFMA C/D layout, the ragged last GEMM tile), channel C - 1 (the tail of the last stage) is
  among the non-zero ones at every grid pixel and has its tap in the centre, so a product lands on every grid pixel.  The helper also shows that the value differs from the full product (lo lo included)
  and from hi hi alone.

tests/test_wino_split_cpu.py: the restatement split_flow_f32 meets the bound with SAFETY = 1 and the exact family bit for bit, and
each mutant misses an assertion of the exact family.
"""
import functools

import torch
import torch.nn.functional as F

import conv_bounds as cb
import step_bounds as sb
import wino_gemm_cases as wc
from colmax_split_bounds import MAG, TINY, TRUNC, split_terms
from conv_bounds import SAFETY, U32

# (B, C, H, W, K): odd planes, C below one 32-channel stage, K tail of the 64 tile; C tail past one stage; one tile per image and C =
# one stage exactly; several GEMM tiles along T; several stages, K tail of the 128 tile, more than one K tile.
SHAPES = [(2, 19, 7, 9, 70), (3, 40, 5, 6, 36), (1, 32, 2, 2, 64), (1, 64, 32, 32, 64), (2, 130, 12, 12, 200)]
TILES = (64, 128)
EPILOGUES = ("none", "bias", "lrelu")
SLOPE = 0.2
MUTANTS = ("lo_hi_dropped", "hi_lo_dropped", "single_bf16", "lo_lo_added")
EXACT_SHAPE = (2, 40, 17, 17, 70)          # T = 162: three 64-tiles / two 128-tiles, the last ragged; C = 32 + 8; K = 64 + 6


def rho_split(C, safety=SAFETY):
    return 16.0 * (TRUNC * MAG + safety * (3 * C + 11) * U32 * MAG)


class SplitBound(cb.Bound):
    """conv_bounds.Bound with the underflow term eta added to every element's bound."""

    def __init__(self, ref, mag, rho, post, exact, what, eta):
        cb.Bound.__init__(self, ref, mag, rho, post, exact, what)
        self.eta = eta

    def measure(self, got, rho=None):
        rho = self.rho if rho is None else rho
        got = got.detach().to("cpu", torch.float64)
        assert got.shape == self.ref.shape, (tuple(got.shape), tuple(self.ref.shape))
        fin_ref = torch.isfinite(self.ref)
        strict = torch.isfinite(self.mag) & fin_ref
        wrong = int((~torch.isfinite(got) & strict).sum()) + int((torch.isfinite(got) & ~fin_ref).sum())
        err = (got - self.ref).abs()
        bound = rho * self.mag + self.post * U32 * self.ref.abs() + self.eta + cb.FLOOR
        q = torch.where(strict, err / bound, torch.zeros_like(err))
        q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
        flat = int(q.argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), q.shape))
        return float(q.max()), wrong, idx


def check_contract(x, w):
    for t, what in ((x, "input"), (w, "weight")):
        fin = torch.isfinite(t)
        if bool((t[fin].abs() >= 2.0 ** 125).any()):
            raise ValueError("split Winograd route: a finite %s value of 2^125 or more is outside the contract" % what)


def split_bounds(x, w, b, slope=SLOPE, safety=SAFETY, exact=False, what=""):
    """-> {"none", "bias", "lrelu"}: the bounds of the three epilogues for float32 x [B, C, H, W], w [K, C, 3, 3], b [K]."""
    check_contract(x, w)
    C = x.shape[1]
    rho = rho_split(C, safety)
    xd, wd = x.double(), w.double()
    g = wd.abs().sum((2, 3))
    sum_x = cb.patch_mag_forward(xd, torch.ones_like(g))
    eta = TINY * 16.0 * (3.0 * (4.0 * sum_x + g.sum(1).view(1, -1, 1, 1)) + 6.0 * C)
    eta = torch.where(torch.isfinite(eta), eta, torch.zeros_like(eta))
    out = {}
    for epi in EPILOGUES:
        base = cb.forward_bound(x, w, None if epi == "none" else b, act="lrelu" if epi == "lrelu" else None, slope=slope, rho=rho,
                                winograd=True, exact=exact, what="%s %s" % (what, epi))
        # the LeakyReLU product is a rounding of its own (fl32(y fl32(slope)) is not fl32(y slope)): the integer case is exact before it
        out[epi] = SplitBound(base.ref, base.mag, rho, safety + base.post, exact and epi != "lrelu", base.what, eta)
    return out


@functools.lru_cache(maxsize=None)
def split_case(shape, kind):
    """-> x, w, b (float32 CPU) of the family `kind` of conv_bounds.FAMILIES and the bounds of the three epilogues.  Every family
    stays inside the contract: "nonfinite" holds a NaN and an infinity, which the kernel turns into NaNs over their patches."""
    B, C, H, W, K = shape
    small = C > 64
    s = 2000 * SHAPES.index(shape) + 17 * cb.FAMILIES.index(kind) + 7
    x = cb.activations(kind, (B, C, H, W), s, small)
    w, b = cb.weights(kind, (K, C, 3, 3), s + 1, small=small)
    return x, w, b, split_bounds(x, w, b, exact=kind == "integers", what="wg split %s %s" % (shape, kind))


# ------------------------------------------------------------------------------------------------ the data flow in torch fp32
def split_flow_f32(x, w, b=None, epilogue="none", slope=SLOPE, mutant=None):
    """wino_gemm_cases.wg_flow_f32 with split_terms applied to U and V and three bmm's added in fp32: the kernels' data flow."""
    B, C, H, W = x.shape
    K = w.shape[0]
    bt, g, at = cb._BT.to(x.dtype), cb._G.to(x.dtype), cb._AT.to(x.dtype)
    P = cb._patches(x)
    TH, TW = P.shape[2], P.shape[3]
    T = B * TH * TW
    V = (bt @ P @ bt.t()).permute(4, 5, 1, 0, 2, 3).reshape(16, C, T)
    U = (g @ w @ g.t()).permute(2, 3, 0, 1).reshape(16, K, C)
    uh, ul = split_terms(U)
    vh, vl = split_terms(V)
    uh, ul, vh, vl = uh.to(x.dtype), ul.to(x.dtype), vh.to(x.dtype), vl.to(x.dtype)
    lo_hi, hi_lo, hi_hi = torch.bmm(ul, vh), torch.bmm(uh, vl), torch.bmm(uh, vh)
    if mutant == "single_bf16":
        M = hi_hi
    elif mutant == "lo_hi_dropped":
        M = hi_lo + hi_hi
    elif mutant == "hi_lo_dropped":
        M = lo_hi + hi_hi
    elif mutant == "lo_lo_added":
        M = ((torch.bmm(ul, vl) + lo_hi) + hi_lo) + hi_hi
    else:
        M = (lo_hi + hi_lo) + hi_hi
    M = M.reshape(4, 4, K, B, TH, TW).permute(3, 2, 4, 5, 0, 1)
    Y = at @ M @ at.t()
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, K, 2 * TH, 2 * TW)[:, :, :H, :W]
    if epilogue != "none":
        y = y + b.view(1, -1, 1, 1)
    if epilogue == "lrelu":
        y = torch.where(y > 0, y, y * slope)
    return y.contiguous()


# ------------------------------------------------------------------------------------------------ exact family
def _values(n, gen):
    """n values +-(1 + q 2^-10) 2^e, q in 1..3, e in -1..1: hi = +-2^e, lo = +-q 2^(e - 10), both exact and non-zero."""
    q = torch.randint(1, 4, (n,), generator=gen).double()
    e = torch.randint(-1, 2, (n,), generator=gen).double()
    sign = torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    return (sign * (1 + q * 2.0 ** -10) * torch.exp2(e)).float()


@functools.lru_cache(maxsize=None)
def split_exact_inputs(shape=EXACT_SHAPE, seed=0):
    """-> x [B, C, H, W], w [K, C, 3, 3] of the exact family (module docstring)."""
    B, C, H, W, K = shape
    gen = torch.Generator().manual_seed(9300 + seed)
    x = torch.zeros(B, C, H, W)
    for b in range(B):
        y0, x0 = ((H - 1) % 4, (W - 1) % 4) if b == B - 1 else (0, 0)          # the last image's grid reaches pixel (H - 1, W - 1)
        for py in range(y0, H, 4):
            for px in range(x0, W, 4):
                ch = torch.cat((torch.tensor([C - 1]), torch.randperm(C - 1, generator=gen)[:3]))
                x[b, ch, py, px] = _values(4, gen)
    assert x[0, :, 0, 0].ne(0).sum() == 4 and x[B - 1, :, H - 1, W - 1].ne(0).sum() == 4
    w = torch.zeros(K * C, 9)
    tap = torch.randint(0, 9, (K, C), generator=gen)
    tap[:, C - 1] = 4                                                          # the centre: a product lands on every grid pixel
    w[torch.arange(K * C), tap.reshape(-1)] = _values(K * C, gen)
    return x.contiguous(), w.view(K, C, 3, 3).contiguous()


def split_exact_reference(x, w):
    """-> (three-term value, full product, hi hi alone), float64 [B, K, H, W], the first and the last proven exact in float32; raises unless U and V are
    hi + lo exactly, every partial sum of the kernel is exact, and the three values differ from one another."""
    xd, wd = x.double(), w.double()
    K, C = w.shape[0], w.shape[1]
    B, _, H, W = x.shape
    bt, g, at = cb._BT.double(), cb._G.double(), cb._AT.double()
    P = cb._patches(xd)
    TH, TW = P.shape[2], P.shape[3]
    T = B * TH * TW
    V = (bt @ P @ bt.t()).permute(4, 5, 1, 0, 2, 3).reshape(16, C, T)
    U = (g @ wd @ g.t()).permute(2, 3, 0, 1).reshape(16, K, C)
    sb.require_exact(U, "split exact family: U")
    sb.require_exact(V, "split exact family: V")
    # no rounding on the way to U and V: every entry of V is 0 or +- one input, every entry of U a tap times 1, 1/2 or 1/4
    if not (set((V.abs() * 2048).unique().tolist()) <= set((xd.abs() * 2048).unique().tolist())):
        raise ValueError("split exact family: an entry of V is not a single input value")
    uh, ul = (t.double() for t in split_terms(U.float()))
    vh, vl = (t.double() for t in split_terms(V.float()))
    if not (torch.equal(uh + ul, U) and torch.equal(vh + vl, V)):
        raise ValueError("split exact family: an operand is not hi + lo exactly")
    if not (bool((ul != 0).any()) and bool((vl != 0).any())):
        raise ValueError("split exact family: no lo term")
    # every operand term is a multiple of its quantum, so every product the kernel forms (never lo lo) and every sum of them is a
    # multiple of Q; the magnitudes of ALL terms of one output element (three products per channel, 16 positions) stay below 2^24 Q:
    # any partial sum in any order is exact
    quh, qul, qvh, qvl = 2.0 ** -3, 2.0 ** -13, 2.0 ** -1, 2.0 ** -11
    for t, q in ((uh, quh), (ul, qul), (vh, qvh), (vl, qvl)):
        if not torch.equal(t / q, (t / q).round()):
            raise ValueError("split exact family: an operand term is not a multiple of its quantum")
    Q = min(qul * qvh, quh * qvl, quh * qvh)
    mag = torch.bmm(ul.abs(), vh.abs()) + torch.bmm(uh.abs(), vl.abs()) + torch.bmm(uh.abs(), vh.abs())
    if not float(mag.reshape(16, -1).sum(0).max()) / Q < 2.0 ** 24:
        raise ValueError("split exact family: a partial sum may leave the exact range of float32")
    if int((V != 0).sum(1).max()) > 4:
        raise ValueError("split exact family: more than four products in a sum")

    def out(M):
        M = M.reshape(4, 4, K, B, TH, TW).permute(3, 2, 4, 5, 0, 1)
        Y = at @ M @ at.t()
        return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, K, 2 * TH, 2 * TW)[:, :, :H, :W].contiguous()
    three = out(torch.bmm(ul, vh) + torch.bmm(uh, vl) + torch.bmm(uh, vh))
    hh = out(torch.bmm(uh, vh))
    full = F.conv2d(xd, wd, None, 1, 1)
    if not torch.equal(out(torch.bmm(U, V)), full):
        raise ValueError("split exact family: the Winograd form of the full product is not the convolution")
    for t, what in ((three, "three terms"), (hh, "hi hi")):
        sb.require_exact(t, "split exact family (%s)" % what)
    # the three values differ wherever a product lands: at the first and the last pixel, in both halves of the C/D layout (rows 0-3
    # and 4-7 of a 32-row block), in the last (ragged) tile of K, and behind the channel tail
    for k in (0, 5, K - 1):
        for (b, py, px) in ((0, 0, 0), (B - 1, H - 1, W - 1)):
            patch = (slice(b, b + 1), slice(k, k + 1), slice(max(py - 1, 0), py + 2), slice(max(px - 1, 0), px + 2))
            if not (bool((three[patch] != full[patch]).any()) and bool((three[patch] != hh[patch]).any())):
                raise ValueError("split exact family: the three-term value cannot be told apart at channel %d, pixel %s" % (k, (b, py, px)))
    return three, full, hh


# ------------------------------------------------------------------------------------------------ non-finite contract
NONFINITE_CASES = ("nan_input", "inf_input", "nan_weight")
NONFINITE_SHAPE = (2, 40, 9, 10, 36)


def split_nonfinite_case(case):
    """-> x, w, b, the bounds, and (must, may) [B, K, H, W]: where the result must be NaN and where it may be.  Image 0 carries the
    defect, image 1 is untouched (but for a weight's NaN, which makes output channel 3 NaN everywhere).  An input defect at pixel
    (4, 5) of channel 7 must reach the outputs the convolution itself lets it reach, rows 3..5, columns 4..6, and may reach the
    whole tiles whose 4 x 4 patches hold it, tiles (1..2, 2..3): rows 2..5, columns 4..7.  (The kernel adds and subtracts the patch,
    so its NaNs are the first set; the restatement multiplies by B's zeros, so its NaNs are the second.)"""
    B, C, H, W, K = NONFINITE_SHAPE
    x = cb.activations("iid", (B, C, H, W), 4411)
    w, b = cb.weights("iid", (K, C, 3, 3), 4412)
    must, may = torch.zeros(B, K, H, W, dtype=torch.bool), torch.zeros(B, K, H, W, dtype=torch.bool)
    if case == "nan_weight":
        w[3, 11, 1, 2] = float("nan")
        must[:, 3] = may[:, 3] = True
    else:
        x[0, 7, 4, 5] = float("nan") if case == "nan_input" else float("-inf")
        must[0, :, 3:6, 4:7] = True
        may[0, :, 2:6, 4:8] = True
    return x, w, b, split_bounds(x, w, b, what="wg split " + case), (must, may)


def split_nonfinite_check(case, bounds, want, outs):
    """outs {"none", "bias", "lrelu"}: NaN (never an infinity) over the stated reach, inside the bound elsewhere."""
    must, may = want
    for epi, got in outs.items():
        got = got.detach().cpu()
        assert bool(torch.isnan(got)[must].all()), "%s %s: a result inside the defect's reach is not NaN" % (case, epi)
        assert bool(torch.isfinite(got)[~may].all()), "%s %s: a non-finite result outside the stated reach" % (case, epi)
        bounds[epi].check(got)


assert wc.SHAPES[0] == SHAPES[0]          # the fp32 route's cases, with C = 8 replaced by one full stage
