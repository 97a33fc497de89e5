"""Per-pixel float64 error bounds for the gather backward outputs (a plain helper module, not a conftest).

The four sampling operators have two kinds of backward output.  The scatter outputs have their bounds in tests/scatter_bounds.py;
the GATHER outputs -- resample2d d_input2 (d/dx, d/dy, d/dsigma), block-extractor d_flow, block-attention d_flow and d_weights,
warp d_flow -- are signed sums over taps and channels, one per pixel.  Their largest value on a plane is hundreds of times a
border pixel's or a quiet channel group's, so ``tol * (1 + max|ref|)`` passes a 0.1 % error there.  For one output element:

  ref    the float64 oracle's value;
  mag    the sum of the absolute values of every product the reference adds into the element, from a plain float64 torch
         restatement of the operator's taps (``gather`` on the flattened planes) -- the condition number of the element's sum;
  kappa  the input conditioning every fp32 implementation shares with the reference (below), 0 where the inputs make it 0;

and the assertion, on every element where ref is finite,

    |got - ref| <= rho mag + kappa + 1e-38,

non-finite elements sitting exactly where the reference has them.

mag, per output (x component; y is symmetric):
  * warp            (Wi/2) sum_c |g_c| ((|s0| + |s1|)(1 - ay) + (|s2| + |s3|) ay), invalid corners 0; with flipcat g is the direct
                    half plus the mirrored flipped half.
  * block extractor d_flow: the same form per window tap, summed over the k x k taps, corners clamped to the border.
  * block attention d_flow: the extractor's form on the windows (g / k^2) w_ij.
  * block attention d_weights: every term is (g_c / k^2) x a bilinear weight x a source value, the weights non-negative:
                    the oracle's forward extraction of |src| contracted with |g| / k^2.
  * resample2d      component j: sum_k |coef_jk| w_k a_k / sum + |sumgrad_j| sum_k w_k a_k / sum^2, a_k = sum_c |g_c| |in1_c[tap k]|,
                    coef as in the reference (resample2d_kernel.cu:272-293): +-x_ / (-sigma^2), +-y_ / (-sigma^2),
                    (y_^2 + x_^2) / sigma^3.  The two halves of the quotient rule are bounded separately because every
                    implementation forms them separately.

rho (why it is a function of the case): the longest fp32 chain among the implementations is the REFERENCE's -- one running sum
over n = taps x C terms (warp 4 C; extractor / attention d_flow 4 k^2 C; attention d_weights 4 C; resample2d 4 (ks/2)^2 C).  A
float sum of n terms in any order errs by at most (n - 1) u sum|terms|; the kernels' own orders (slabs, groups of four, atomics,
a double accumulator) are covered by the same figure.  Each term carries the roundings of its own factors and the result those
of its final scaling, TERM_OPS of them:
  * warp 6: the corner weight (1), two products (2), the flipcat sum of g (1), the scale Wi/2 (1), one slab combination (1);
  * extractor 8: the weight 1 - (dx - fdx) (2), four products summed (4), the product with g (1), the flow pixel's own sum (1);
    attention d_flow 10: (g / k^2) w_ij adds 2;
  * attention d_weights 6: two weights and their product (3), the product with the source (1), g / k^2 and its product (2);
  * resample2d 16: the tap distance (1), five factors (4), SAFE_DIV (1), sumgrad / C (1), the channel product of the second half
    (3), sum^2, two divisions, the difference (4); the Gaussian weights themselves are kappa's.
So the derivation gives (n + TERM_OPS) u, and rho = SAFETY x that with SAFETY = 4, as in scatter_bounds; u = 2^-24, or 2^-53 for
a float64 kernel.  The float32 oracle must meet every bound at rho / SAFETY (tests/test_gather_bounds_cpu.py).

kappa:
  * resample2d: 4 A u mag, A = min((ks/2 dilation + 1)^2 / (2 sigma^2), cap) per pixel as in scatter_bounds.resample2d_bound (the
    exponent of a Gaussian weight is a float quotient, 3 u relative, A u absolute).  The sigma range keeps A <= 40, so no product
    underflows; the small-sigma regime stays with d_input1's tests.
  * warp: ix = ((g + 1) W - 1) / 2 is three fp32 operations: fl(g + 1), fl(. W), fl(. - 1), the halving exact:
    |d ix| <= (2 |g + 1| W + |(g + 1) W - 1|) u / 2 <= (1.5 max|g + 1| W + 0.5) u.  On a binary grid with power-of-two sizes all three
    are exact and kappa is 0; otherwise d/dx moves by |d iy|_max (Wi/2) sum_c |g_c| (|s0| + |s1| + |s2| + |s3|), and d/dy likewise
    with |d ix|_max.
  * block extractor / attention: pixel + flow + tap offset is exact in float32 for the flows used here: kappa = 0.

Inputs: d_flow is discontinuous across cell edges, so fp32 and float64 must pick the same cell: every flow offset is an odd
multiple of 2^-9 (`odd`), never within 2^-10 of an edge (the warp's fp32 coordinate error is below 2^-14 at these sizes).  The
gradient families are scatter_bounds' (signed, ramp, group_mags, masked, tiny, huge; under `tiny` a term below the normal range errs
by at most 2^-149, which the floor of 1e-38 covers); features and sources are randn, or randn times the per-channel pattern 1, 1e-5,
1e3, 1e-2 (`feat_mags`: the resample2d kernels walk channels in fours).
"""
import functools
import math

import torch

import scatter_bounds as sb

SAFETY = 4
FLOOR = 1e-38
TERM_OPS = {"warp": 6, "block_extractor": 8, "block_attention_flow": 10, "block_attention_weights": 6, "resample2d": 16}
GRAD_FAMILIES = sb.FAMILIES
FAMILIES = GRAD_FAMILIES + ("feat_mags",)
WARP_GRIDS = ("interior", "border", "outside")


def rho_units(op, C, taps):
    """rho in units of u for a case with C channels and `taps` taps per channel: SAFETY (taps C + TERM_OPS)."""
    return SAFETY * (taps * C + TERM_OPS[op])


class Bound:
    """ref / mag / kappa of one gather output (float64 CPU tensors of the output's shape) and the case's rho in units of u."""

    def __init__(self, ref, mag, kappa, units, dtype=torch.float32, signed=None):
        self.ref, self.mag = ref, mag
        self.kappa = kappa if kappa is not None else torch.zeros_like(ref)
        self.units, self.dtype, self.signed = units, dtype, signed

    def ratio(self, got, units=None):
        """max over the finite elements of |got - ref| / bound, and the number of elements whose finiteness differs."""
        rho = (self.units if units is None else units) * sb.unit_roundoff(self.dtype)
        got = got.detach().to("cpu", torch.float64)
        fin = torch.isfinite(self.ref)
        wrong = int((torch.isfinite(got) != fin).sum())
        err = (got - self.ref).abs()[fin]
        if err.numel() == 0:
            return 0.0, wrong
        q = err / ((rho * self.mag + self.kappa)[fin] + FLOOR)
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        return float(q.max()), wrong

    def check(self, got, units=None, what=""):
        ratio, wrong = self.ratio(got, units)
        assert wrong == 0, "%s: %d elements non-finite where the reference is not, or the other way round" % (what, wrong)
        assert ratio <= 1.0, "%s: per-pixel error / bound = %.3g" % (what, ratio)
        return ratio


def same_nonfinite(got, ref):
    """Number of elements whose finiteness differs (the cases whose inputs are non-finite are judged by placement alone)."""
    return int((torch.isfinite(got.detach().to("cpu", torch.float64)) != torch.isfinite(ref)).sum())


def _gather(planes, row, col, W):
    """planes [B, C, Hp * Wp], row / col [B, N] (long, in range) -> [B, C, N]."""
    idx = (row * W + col).unsqueeze(1).expand(-1, planes.shape[1], -1)
    return planes.gather(2, idx)


def _cell(v, n):
    return v.long().clamp(0, n - 1)


# ------------------------------------------------------------------------------------------------ inputs
def odd(t):
    """Odd multiples of 2^-9: at least 2^-9 from every cell edge."""
    return sb.quantize(t, 8) + 2.0 ** -9


def features(kind, shape, seed):
    """randn; `feat_mags`: times the per-channel pattern 1, 1e-5, 1e3, 1e-2 inside each 4-channel group."""
    return sb.family_grad("group_mags" if kind == "feat_mags" else "signed", shape, seed)


def grads(kind, shape, seed):
    return sb.family_grad("signed" if kind == "feat_mags" else kind, shape, seed)


def rs_flow(B, H, W, seed, reach=3.0, sigma=(0.5, 2.5)):
    in2 = sb.rs_flow(B, H, W, seed, reach, sigma)
    in2[:, :2] = odd(in2[:, :2])
    return in2.contiguous()


def block_flow(B, H, W, seed, reach=2.0):
    return odd(sb.block_flow(B, H, W, seed, reach)).contiguous()


def warp_grid(kind, B, in_hw, out_hw, seed):
    """grid_sample coordinates [B, 2, H, W] (float32) for an input of in_hw sampled on out_hw pixels.
    interior: zoom 0.8 about the centre plus jitter, no pixel leaves the image; border: identity +- 2 px; outside: zoom 1.3 (bands
    of pixels with all four corners invalid); zoom18 / zoom25: zoom 1.8 / 2.5 (at 2.5 the sampling positions of a 64 x 16 pixel tile span more than 32 source rows: see
    warp_lds_boxes).  The layout
    is sb.warp_grid's; the samples are odd multiples of 2^-9 and the input may differ in size from the grid."""
    Hi, Wi = in_hw
    H, W = out_hw
    gen = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ux, uy = (xs + 0.5) * Wi / W - 0.5, (ys + 0.5) * Hi / H - 0.5          # the identity, in input pixels
    zoom, amp = {"interior": (0.8, min(1.0, 0.04 * (min(Hi, Wi) - 1))), "border": (1.0, 2.0), "outside": (1.3, 0.5), "zoom18": (1.8, 0.5), "zoom25": (2.5, 0.5)}[kind]
    cx, cy = (Wi - 1) / 2.0, (Hi - 1) / 2.0
    jx = (torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 2 - 1) * amp
    jy = (torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 2 - 1) * amp
    ix, iy = odd(cx + zoom * (ux - cx) + jx), odd(cy + zoom * (uy - cy) + jy)
    if kind == "interior":
        ix, iy = ix.clamp(2.0 ** -9, Wi - 1 - 2.0 ** -9), iy.clamp(2.0 ** -9, Hi - 1 - 2.0 ** -9)
    return torch.stack(((2 * ix + 1) / Wi - 1, (2 * iy + 1) / Hi - 1), 1).float().contiguous()


# ------------------------------------------------------------------------------------------------ warp d_flow
def warp_pixel_slab(B, C, H, W, cs_default=32, min_blocks=4096):
    """Channels per block of the pixel-major warp kernels (csrc/runtime.hip plan(): 64 x 4 pixel tiles, the slab halved, rounding up,
    while the launch has fewer than 4096 blocks).  warp_bwd_body walks its slab four channels per trip and the rest one by one, so
    only a slab of >= 4 channels runs the four-channel loops (the pair loads among them)."""
    spatial = B * ((W + 63) // 64) * ((H + 3) // 4)
    cs = min(cs_default, C)
    while cs > 1 and spatial * ((C + cs - 1) // cs) < min_blocks:
        cs = (cs + 1) // 2
    return cs


def warp_lds_boxes(grid, in_hw):
    """(bw, bh) of every 64 x 16 pixel tile of warp_bwd_flow_lds_kernel: the bounding box, in source cells, of the corners of the
    tile's pixels that have a valid corner, its left edge aligned down to 4 cells, in the kernel's float32 arithmetic.  A tile whose
    box exceeds 128 x 32 cells takes the kernel's direct-gather arm instead of LDS."""
    Hi, Wi = in_hw
    g = grid.float()
    B, _, H, W = g.shape
    x0 = torch.floor(((g[:, 0] + 1) * float(Wi) - 1) / 2)
    y0 = torch.floor(((g[:, 1] + 1) * float(Hi) - 1) / 2)
    live = (x0 >= -1) & (x0 <= Wi - 1) & (y0 >= -1) & (y0 <= Hi - 1)
    boxes = []
    for b in range(B):
        for ty in range(0, H, 16):
            for tx in range(0, W, 64):
                m = live[b, ty:ty + 16, tx:tx + 64]
                if not bool(m.any()):
                    boxes.append((0, 0))
                    continue
                xs, ys = x0[b, ty:ty + 16, tx:tx + 64][m].long(), y0[b, ty:ty + 16, tx:tx + 64][m].long()
                bx0 = (int(xs.min()) // 4) * 4
                boxes.append((int(xs.max()) + 1 - bx0 + 1, int(ys.max()) + 1 - int(ys.min()) + 1))
    return boxes


def warp_restatement(feat, grid, go, flipcat=False, flip_padded=False):
    """(signed, mag, tot): the float64 restatement's d_flow, its sum of |terms|, and (Wi/2, Hi/2) sum_c |g_c| sum_q |s_q| (kappa's
    factor), all [B, 2, H, W].  flip_padded (a mutant for the CPU tests): the first corner's sign is flipped on the pixels that
    have a zero-padded corner."""
    feat, grid, go = feat.double(), grid.double(), go.double()
    B, C, Hi, Wi = feat.shape
    _, _, H, W = grid.shape
    signed, mag, tot = (torch.empty(B, 2, H * W, dtype=torch.float64) for _ in range(3))
    for b in range(B):                                     # (one image at a time: the large case's temporaries stay small)
        g = (go[b:b + 1, :C] + go[b:b + 1, C:].flip(3)) if flipcat else go[b:b + 1]
        g = g.reshape(1, C, H * W)
        ag = g.abs()
        ix = (((grid[b:b + 1, 0] + 1) * Wi - 1) / 2).reshape(1, H * W)
        iy = (((grid[b:b + 1, 1] + 1) * Hi - 1) / 2).reshape(1, H * W)
        fx, fy = torch.floor(ix), torch.floor(iy)
        ax, ay = (ix - fx).unsqueeze(1), (iy - fy).unsqueeze(1)
        x0, y0 = fx.clamp(-2.0 ** 40, 2.0 ** 40).long(), fy.clamp(-2.0 ** 40, 2.0 ** 40).long()
        planes = feat[b:b + 1].reshape(1, C, Hi * Wi)

        def corner(yy, xx):
            valid = (yy >= 0) & (yy < Hi) & (xx >= 0) & (xx < Wi)
            v = _gather(planes, yy.clamp(0, Hi - 1), xx.clamp(0, Wi - 1), Wi)
            return torch.where(valid.unsqueeze(1), v, torch.zeros_like(v))       # (not v * valid: a padded corner is 0 even beside a NaN cell)

        s0, s1, s2, s3 = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
        a0, a1, a2, a3 = s0.abs(), s1.abs(), s2.abs(), s3.abs()
        if flip_padded:
            padded = (y0 < 0) | (y0 + 1 >= Hi) | (x0 < 0) | (x0 + 1 >= Wi)
            s0 = torch.where(padded.unsqueeze(1), -s0, s0)
        signed[b, 0] = (Wi / 2.0) * (g * ((s1 - s0) * (1 - ay) + (s3 - s2) * ay)).sum(1)[0]
        signed[b, 1] = (Hi / 2.0) * (g * ((s2 - s0) * (1 - ax) + (s3 - s1) * ax)).sum(1)[0]
        mag[b, 0] = (Wi / 2.0) * (ag * ((a0 + a1) * (1 - ay) + (a2 + a3) * ay)).sum(1)[0]
        mag[b, 1] = (Hi / 2.0) * (ag * ((a0 + a2) * (1 - ax) + (a1 + a3) * ax)).sum(1)[0]
        t = (ag * (a0 + a1 + a2 + a3)).sum(1)[0]
        tot[b, 0], tot[b, 1] = (Wi / 2.0) * t, (Hi / 2.0) * t
    return signed.view(B, 2, H, W), mag.view(B, 2, H, W), tot.view(B, 2, H, W)


def _pow2(n):
    return n & (n - 1) == 0


def warp_coordinate_error(grid, n, u):
    """|d ix|_max of ix = ((g + 1) n - 1) / 2 in arithmetic of unit roundoff u; 0 for a power-of-two n (binary grids: exact)."""
    if _pow2(n):
        return 0.0
    gmax = float((grid.double() + 1).abs().max())
    return (1.5 * gmax * n + 0.5) * u


def warp_flow_bound(feat, grid, go, flipcat=False, dtype=torch.float32):
    import oracle
    B, C, Hi, Wi = feat.shape
    _, ref = oracle.warp_backward(feat.double().contiguous(), grid.double().contiguous(), go.double().contiguous(), flipcat)
    signed, mag, tot = warp_restatement(feat, grid, go, flipcat)
    u = sb.unit_roundoff(dtype)
    kappa = torch.stack((warp_coordinate_error(grid[:, 1], Hi, u) * tot[:, 0], warp_coordinate_error(grid[:, 0], Wi, u) * tot[:, 1]), 1)
    return Bound(ref, mag, kappa, rho_units("warp", C, 4), dtype, signed)


# ------------------------------------------------------------------------------------------------ block extractor / attention
def block_extractor_restatement(src, flow, go, k, flip_clamped=False):
    """(signed, mag) of the extractor's d_flow [B, 2, Hf, Wf] for the k x k windows `go` [B, C, k Hf, k Wf].  flip_clamped (a
    mutant for the CPU tests): the top-left corner's sign is flipped on the taps that were clamped to the border."""
    src, flow, go = src.double(), flow.double(), go.double()
    B, C, Hs, Ws = src.shape
    _, _, Hf, Wf = flow.shape
    ys, xs = torch.meshgrid(torch.arange(Hf, dtype=torch.float64), torch.arange(Wf, dtype=torch.float64), indexing="ij")
    planes = src.reshape(B, C, Hs * Ws)
    win = go.reshape(B, C, Hf, k, Wf, k)
    signed = torch.zeros(B, 2, Hf * Wf, dtype=torch.float64)
    mag = torch.zeros(B, 2, Hf * Wf, dtype=torch.float64)
    for i in range(k):
        for j in range(k):
            dy = ((flow[:, 1] + (i - k // 2)) + ys).reshape(B, -1)
            dx = ((flow[:, 0] + (j - k // 2)) + xs).reshape(B, -1)
            fdx, fdy = torch.floor(dx), torch.floor(dy)
            xL, xR, yT, yB = _cell(fdx, Ws), _cell(fdx + 1, Ws), _cell(fdy, Hs), _cell(fdy + 1, Hs)
            xRP, yBP = (dx - fdx).unsqueeze(1), (dy - fdy).unsqueeze(1)
            xLP, yTP = 1 - xRP, 1 - yBP
            sTL, sTR = _gather(planes, yT, xL, Ws), _gather(planes, yT, xR, Ws)
            sBL, sBR = _gather(planes, yB, xL, Ws), _gather(planes, yB, xR, Ws)
            if flip_clamped:
                sTL = torch.where(((xL == xR) | (yT == yB)).unsqueeze(1), -sTL, sTL)
            g = win[:, :, :, i, :, j].reshape(B, C, -1)
            ag = g.abs()
            signed[:, 0] += (g * (-yTP * sTL - yBP * sBL + yTP * sTR + yBP * sBR)).sum(1)
            signed[:, 1] += (g * (-xLP * sTL - xRP * sTR + xLP * sBL + xRP * sBR)).sum(1)
            mag[:, 0] += (ag * (yTP * (sTL.abs() + sTR.abs()) + yBP * (sBL.abs() + sBR.abs()))).sum(1)
            mag[:, 1] += (ag * (xLP * (sTL.abs() + sBL.abs()) + xRP * (sTR.abs() + sBR.abs()))).sum(1)
    return signed.view(B, 2, Hf, Wf), mag.view(B, 2, Hf, Wf)


def block_extractor_flow_bound(src, flow, go, k, dtype=torch.float32):
    import oracle
    C = src.shape[1]
    _, ref = oracle.block_extractor_backward(src.double().contiguous(), flow.double().contiguous(), go.double().contiguous(), k)
    signed, mag = block_extractor_restatement(src, flow, go, k)
    return Bound(ref, mag, None, rho_units("block_extractor", C, 4 * k * k), dtype, signed)


def block_attention_bounds(src, flow, w, go, k, dtype=torch.float32):
    """(d_flow bound, d_weights bound) against the composition avg_pool2d(extractor(src, flow) x reshape(w), k)."""
    import oracle
    C = src.shape[1]
    s64, f64 = src.double().contiguous(), flow.double().contiguous()
    ext_go = sb.attention_extractor_grad(w, go, k)                       # (g / k^2) w_ij
    _, ref_f = oracle.block_extractor_backward(s64, f64, ext_go, k)
    signed, mag_f = block_extractor_restatement(src, flow, ext_go, k)
    flow_bound = Bound(ref_f, mag_f, None, rho_units("block_attention_flow", C, 4 * k * k), dtype, signed)
    gpool = (go.double() / (k * k)).repeat_interleave(k, 2).repeat_interleave(k, 3)
    ext = oracle.block_extractor_forward(s64, f64, k)
    ext_abs = oracle.block_extractor_forward(s64.abs().contiguous(), f64, k)
    ref_w = oracle.local_attn_reshape_backward((gpool * ext).sum(1, keepdim=True).contiguous(), k)
    mag_w = oracle.local_attn_reshape_backward((gpool.abs() * ext_abs).sum(1, keepdim=True).contiguous(), k)
    return flow_bound, Bound(ref_w, mag_w, None, rho_units("block_attention_weights", C, 4), dtype)


# ------------------------------------------------------------------------------------------------ resample2d d_input2
def resample2d_restatement(in1, in2, go, ks, dilation=1, halves=False):
    """(signed, mag) of d_input2 [B, 3, H, W] (d/dx, d/dy, d/dsigma), resample2d_kernel.cu:204-330 in float64; with `halves` the
    two halves of the quotient rule instead (signed = first - second)."""
    in1, in2, go = in1.double(), in2.double(), go.double()
    B, _, H, W = in2.shape
    _, C, Hi, Wi = in1.shape
    N = H * W
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    xf, yf, sig = (xs + in2[:, 0]).reshape(B, N), (ys + in2[:, 1]).reshape(B, N), in2[:, 2].reshape(B, N)
    fx0, fy0 = torch.floor(xf), torch.floor(yf)
    alpha, beta = xf - fx0, yf - fy0
    planes = in1[:B].reshape(B, C, Hi * Wi)
    g = go.reshape(B, C, N)
    ag = g.abs()
    ns2, s3 = -sig * sig, sig * sig * sig

    def gauss(v):
        return torch.exp(-v * v / (2 * sig * sig))

    total = torch.zeros(B, N, dtype=torch.float64)
    WS, WA = torch.zeros_like(total), torch.zeros_like(total)
    grad1, sumgrad, mag1 = (torch.zeros(B, 3, N, dtype=torch.float64) for _ in range(3))
    for fy in range(ks // 2):
        for fx in range(ks // 2):
            rows = ((fy * dilation + beta, _cell(fy0 - fy * dilation, Hi), 1.0), ((1 + fy) * dilation - beta, _cell(fy0 + (fy + 1) * dilation, Hi), -1.0))
            cols = ((fx * dilation + alpha, _cell(fx0 - fx * dilation, Wi), 1.0), ((1 + fx) * dilation - alpha, _cell(fx0 + (fx + 1) * dilation, Wi), -1.0))
            for y_, row, sy in rows:
                for x_, col, sx in cols:
                    wk = gauss(y_) * gauss(x_)
                    v = _gather(planes, row, col, Wi)
                    S, a = (g * v).sum(1), (ag * v.abs()).sum(1)
                    coef = torch.stack((sx * x_ / ns2, sy * y_ / ns2, (y_ * y_ + x_ * x_) / s3), 1)
                    total += wk
                    WS += wk * S
                    WA += wk * a
                    grad1 += coef * (wk * S).unsqueeze(1)
                    sumgrad += coef * wk.unsqueeze(1)
                    mag1 += coef.abs() * (wk * a).unsqueeze(1)
    tot = total.unsqueeze(1)
    if halves:
        return (grad1 / tot).view(B, 3, H, W), (sumgrad * WS.unsqueeze(1) / (tot * tot)).view(B, 3, H, W)
    signed = grad1 / tot - sumgrad * WS.unsqueeze(1) / (tot * tot)
    mag = mag1 / tot + sumgrad.abs() * WA.unsqueeze(1) / (tot * tot)
    return signed.view(B, 3, H, W), mag.view(B, 3, H, W)


def resample2d_input2_bound(in1, in2, go, ks, dilation=1, dtype=torch.float32):
    import oracle
    C = in1.shape[1]
    _, ref = oracle.resample2d_backward(in1.double().contiguous(), in2.double().contiguous(), go.double().contiguous(), ks, dilation)
    signed, mag = resample2d_restatement(in1, in2, go, ks, dilation)
    u = sb.unit_roundoff(dtype)
    sig = in2[:, 2:3].double()
    vmax = (ks // 2) * dilation + 1
    A = ((vmax * vmax / 2.0) / (sig * sig)).clamp(max=104.0 if dtype == torch.float32 else 745.0)
    assert float(A.max()) <= 40.0, "sigma range: a Gaussian product would underflow"
    return Bound(ref, mag, 4 * u * A * mag, rho_units("resample2d", C, 4 * (ks // 2) ** 2), dtype, signed)


# ------------------------------------------------------------------------------------------------ the cases of the GPU matrix
# Shared by tests/test_gpu_gather_bounds.py (the kernels) and tests/test_gather_bounds_cpu.py (the float32 oracle at the same
# shapes).  Every builder is cached per (case, family): the float64 reference is computed once and never modified.

# name: (in1 shape, flow grid or None (= in1's), kernel_size, dilation, flow reach, sigma range, dtype)
RS_CASES = {
    "lds_slabs": ((1, 20, 37, 70), None, 4, 1, 3.0, (0.5, 2.5), torch.float32),       # W % 64, H % 4 != 0; channel slabs + atomics
    "lds_store": ((1, 4, 37, 70), None, 4, 1, 3.0, (0.5, 2.5), torch.float32),        # one slab: plain stores
    "lds_c6": ((1, 6, 37, 70), None, 4, 1, 3.0, (0.5, 2.5), torch.float32),           # ragged 4-channel group
    "lds_c5_ks2": ((1, 5, 37, 70), None, 2, 1, 3.0, (0.5, 2.5), torch.float32),
    "lds_c7_ks6": ((1, 7, 37, 70), None, 6, 1, 3.0, (0.5, 2.5), torch.float32),
    "lds_grids": ((1, 8, 24, 30), (17, 40), 4, 1, 3.0, (0.5, 2.5), torch.float32),    # input grid != output grid
    "lds_fallback": ((1, 6, 37, 70), None, 4, 1, 40.0, (0.5, 2.5), torch.float32),    # the box exceeds LDS: direct gathers
    "pixels_dil2": ((1, 6, 37, 70), None, 4, 2, 3.0, (0.6, 2.5), torch.float32),
    "pixels_sv2": ((1, 6, 37, 70), None, 4, 1, 3.0, (0.5, 2.5), torch.float32),       # (scatter_variant = 2)
    "pixels_f64": ((1, 6, 37, 70), None, 4, 1, 3.0, (0.5, 2.5), torch.float64),
    "pixels_f64_dil2": ((1, 6, 37, 70), None, 4, 2, 3.0, (0.6, 2.5), torch.float64),
    "generic_ks8": ((1, 3, 14, 14), None, 8, 1, 3.0, (0.6, 2.5), torch.float32),
}


@functools.lru_cache(maxsize=None)
def rs_case(name, kind):
    shape, grid, ks, dil, reach, sigma, dtype = RS_CASES[name]
    B, C, Hi, Wi = shape
    H, W = grid or (Hi, Wi)
    in1 = features(kind, shape, 130)
    in2 = rs_flow(B, H, W, 131, reach, sigma)
    go = grads(kind, (B, C, H, W), 132)
    return in1, in2, go, resample2d_input2_bound(in1, in2, go, ks, dil, dtype)


# name: (source shape, flow grid or None, k, flow reach, dtype)
BE_CASES = {
    "pixels": ((1, 8, 60, 70), None, 3, 2.0, torch.float32),
    "pixels_f64": ((1, 8, 60, 70), None, 3, 2.0, torch.float64),
    "pixels_k2": ((1, 3, 20, 33), None, 2, 2.0, torch.float32),
    "pixels_k4": ((1, 3, 20, 33), None, 4, 2.0, torch.float32),
    "pixels_k5": ((1, 3, 20, 33), None, 5, 2.0, torch.float32),
    "pixels_k5_f64": ((1, 3, 20, 33), None, 5, 2.0, torch.float64),
    "grids": ((1, 2, 16, 16), (9, 21), 3, 2.0, torch.float32),
    "generic_k9": ((1, 2, 9, 9), (4, 4), 9, 2.0, torch.float32),
    "tiles": ((1, 8, 150, 200), None, 3, 2.0, torch.float32),
    "tiles_far": ((1, 8, 150, 200), None, 3, 24.0, torch.float32),       # most pixels leave the tile's box: the far kernel's pixels
}


@functools.lru_cache(maxsize=None)
def be_case(name, kind):
    shape, grid, k, reach, dtype = BE_CASES[name]
    B, C, Hs, Ws = shape
    Hf, Wf = grid or (Hs, Ws)
    src = features(kind, shape, 140)
    flow = block_flow(B, Hf, Wf, 141, reach)
    go = grads(kind, (B, C, k * Hf, k * Wf), 142)
    return src, flow, go, k, block_extractor_flow_bound(src, flow, go, k, dtype)


BA_CASES = {"c8": ((1, 8, 100, 140), torch.float32), "c6": ((1, 6, 100, 140), torch.float32), "c6_f64": ((1, 6, 40, 70), torch.float64)}


@functools.lru_cache(maxsize=None)
def ba_case(name, kind):
    shape, dtype = BA_CASES[name]
    B, C, H, W = shape
    src = features(kind, shape, 150)
    flow = block_flow(B, H, W, 151)
    w = torch.randn(B, 9, H, W, generator=torch.Generator().manual_seed(152))
    go = grads(kind, shape, 153)
    return (src, flow, w, go) + block_attention_bounds(src, flow, w, go, 3, dtype)


# name: (feature shape, grid size or None, dtype)
WARP_CASES = {
    "b2c5_64": ((2, 5, 64, 64), None, torch.float32),
    "ragged_w": ((1, 6, 70, 67), None, torch.float32),                   # W % 4 != 0: the scalar grad_output loads
    "grids": ((1, 3, 96, 130), (80, 129), torch.float32),
    "slabs": ((1, 40, 64, 64), None, torch.float32),                     # channel slabs combine by atomics
    "c2_66": ((1, 2, 66, 66), None, torch.float32),                      # zoom18: stays in LDS; zoom25: boxes of > 32 rows, direct gathers
    "small": ((2, 5, 12, 10), None, torch.float32),
    "ragged": ((1, 7, 33, 70), None, torch.float32),
    "crop": ((1, 3, 128, 128), (32, 32), torch.float32),
    "small_f64": ((2, 5, 12, 10), None, torch.float64),
    "ragged_f64": ((1, 7, 33, 70), None, torch.float64),
    "natural": ((4, 64, 256, 256), None, torch.float32),                 # exactly 2^24: the LDS kernel's own route
    "multi_wide": ((2, 8, 64, 192), None, torch.float32),
    "multi_crop": ((2, 3, 64, 64), (16, 16), torch.float32),
    "slab5": ((4, 20, 256, 256), None, torch.float32),                   # the pixel kernels keep 5 channels per block (warp_pixel_slab)
}


@functools.lru_cache(maxsize=None)
def warp_case(name, grid_kind, kind, flipcat):
    shape, grid_hw, dtype = WARP_CASES[name]
    B, C, Hi, Wi = shape
    H, W = grid_hw or (Hi, Wi)
    feat = features(kind, shape, 160)
    grid = warp_grid(grid_kind, B, (Hi, Wi), (H, W), 161)
    go = grads(kind, (B, 2 * C if flipcat else C, H, W), 162)
    return feat, grid, go, warp_flow_bound(feat, grid, go, flipcat, dtype)


# The matrix: which (grid family, gradient / feature family, flipcat) combinations a warp case runs, and which families the others.
def warp_matrix(name):
    if name == "natural":              # one family: the float64 reference of 2^24 elements takes seconds
        return [("border", "group_mags", False)]
    if name.startswith("multi") or name == "slab5":        # (slab5: 5.2 M elements, about a second per reference)
        return [(g, k, f) for g in ("interior", "border") for k, f in (("signed", False), ("group_mags", True))]
    rows = [(g, "signed", f) for g in WARP_GRIDS for f in (False, True)]
    if name.endswith("f64"):
        return rows + [("border", "group_mags", True), ("border", "feat_mags", False)]
    if name == "c2_66":
        return [(g, k, f) for g in ("zoom18", "zoom25") for k, f in (("signed", False), ("group_mags", True), ("feat_mags", False))]
    rows += [("border", k, i % 2 == 1) for i, k in enumerate(FAMILIES[1:])]
    if name in ("ragged_w", "grids"):  # tiles that leave LDS, with the scalar grad_output loads / unequal grids
        rows += [("zoom25", "signed", False), ("zoom25", "group_mags", True)]
    return rows
