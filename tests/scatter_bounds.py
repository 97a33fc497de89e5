"""Per-cell float64 error bounds for the scatter backward outputs (a plain helper module, not a conftest).

The four scatter backward operators -- resample2d d_input1, block_extractor d_source, block attention d_source and warp d_feat --
add many weighted gradient terms into each cell of their output.  Several of their fp32 kernels accumulate in 32-bit fixed-point
LDS cells whose scale is a power of two taken from the largest gradient of a CHANNEL near the cell (per block and channel, or per
block and 4-channel group for resample2d's owned tiles); float atomics, which the reference uses, round each partial sum relative
to the cell's own terms instead.  A global bound such as ``tol * (1 + max|ref|)`` cannot tell the two apart wherever magnitudes
differ between tiles or channels, so these bounds are per cell.  For one output, with every cell's contributions w_i g_i:

  ref  the exact sum, from the float64 oracle;
  mag  sum_i |w_i g_i|: the same oracle backward run with |grad_output| (and |weights| for block attention).  The interpolation
       weights are non-negative (bilinear, normalised Gaussian), so this is the condition number of the cell's sum;
  L    the per-CHANNEL local maximum of |g| over the grad_output pixels within R = (R_y, R_x) pixels of the cell (max_pool2d of
       |g|; for the extractor and attention each flow pixel's k x k window is reduced first).

and the assertion, on every cell where ref is finite:

    |got - ref| <= rho mag + eta L + kappa + 1e-38,

non-finite cells sitting exactly where the reference has them.  kappa is the fp32 conditioning of the resample2d WEIGHTS
(below); it is 0 for the other operators.

Where R comes from (the reach of a fixed-point scale): a block's scale is a maximum over the pixels it visits, and the cell it
writes lies inside that pixel region, so every such pixel is within the region's extent of the cell.
  * resample2d owned tiles (rs_bwd1_owned_kernel): a block visits a 64 x 48 pixel REGION (its 54 x 38 own tile at ks = 4 grown by
    the margin M = 3 + ks/2 on each side): R = (47, 63).  The shared-cell tile kernel (rs_bwd1_tile_kernel) visits 64 x 16 pixels
    whose box reaches 6 cells further: inside the same R.
  * block extractor / block attention (be_bwd_tile2_kernel, ba_bwd_src_kernel): a tile of 64 x 32 flow pixels, a box grown by a
    halo of at most 8 cells plus the k x k window and the bilinear neighbour: R = (32 + 12, 64 + 12) = (44, 76).
  * warp (warp_bwd_feat_tile_kernel): tiles of at most 64 x 32 pixels with their halo: the extractor's R covers them.

Where rho and eta come from (the kernels' own contracts, include/ffwm_hip.h), for fp32 (u = 2^-24):
  * rho = 2^8 u = 2^-16: float rounding of about n terms -- each product w_i g_i rounds once (u), each weight carries a few ulps of
    its own arithmetic (normalisation, products: <= 4 u), and a float sum of n terms in any order errs by <= (n - 1) u sum|terms|.
    A cell takes <= 16 pixel-taps (ks = 4) to ~40 of them for flows that do not contract: (40 + 5) u < 2^6 u; x 4 margin.
  * eta = 2^12 u = 2^-12: one fixed-point unit per contribution.  The unit of a cell is at most 2^3 x 2 max|g_c| / 2^22 over the
    block's pixels (resample2d owned tiles: the channel's maximum within 2^3 of the scale, 22 bits; the tile kernel 2^-19 with its
    per-channel scale; the extractor / attention <= 2^-20 x 4 of the sampled maximum), <= 2^-18 L; rounding to it errs by half a
    unit per contribution, and ~40 contributions give 20 x 2^-18 L < 2^-13.7 L.
  For fp64 outputs the same multiples of u = 2^-53 apply.
  * kappa (resample2d only): the reference forms each Gaussian weight as exp of a FLOAT quotient -v^2 / (2 sigma^2), whose relative
    error (<= 3 u) becomes an absolute error of A u in the exponent: a relative error of <= 4 A u of the weight, A <= min((ks/2 + 1)^2 / (2
    sigma^2), 104) the largest exponent a non-zero float weight can have.  Every fp32 implementation (kernels and reference) shares
    it: kappa is the backward of |g| 4 A u.  A tap whose float product is below the normal range has no relative precision left:
    its normalised weight is below 2^-126 / sum either way, and kappa adds that times |g| to the tap's cell.  A pixel whose float
    sum itself is tiny (< 2^-100) gets its whole contribution |w g| as slack, and a pixel whose 16 float products all UNDERFLOW contributes
    nothing in the reference (SAFE_DIV(0, 0) = 0): its gradient is zeroed in ref and mag (not in L), so a kernel that adds O(g)
    for it fails by orders of magnitude.

A flow that CONTRACTS many pixels onto one cell has a fixed-point resolution that scales with the counted population by design;
those cases keep their own tests (tests/test_gpu_parity.py) and are not measured here.

The float32 oracle itself meets these bounds with rho / 4 and eta = 0 (tests/test_scatter_bounds_cpu.py).
"""
import math

import torch
import torch.nn.functional as F

RHO_UNITS, ETA_UNITS = 2.0 ** 8, 2.0 ** 12
FLOOR = 1e-38
R_RESAMPLE = (47, 63)
R_BLOCK = (44, 76)
R_WARP = R_BLOCK
SUBNORMAL_SUM = 2.0 ** -100


def unit_roundoff(dtype):
    return 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53


def rho_eta(dtype):
    u = unit_roundoff(dtype)
    return RHO_UNITS * u, ETA_UNITS * u


class Bound:
    """ref / mag / L / kappa of one scatter output, all float64 CPU tensors of the output's shape."""

    def __init__(self, ref, mag, L, kappa=None, dtype=torch.float32):
        self.ref, self.mag, self.L = ref, mag, L
        self.kappa = kappa if kappa is not None else torch.zeros_like(ref)
        self.dtype = dtype

    def ratio(self, got, rho=None, eta=None):
        """max over the finite cells of |got - ref| / bound, and the non-finite cells that differ (count)."""
        r0, e0 = rho_eta(self.dtype)
        rho = r0 if rho is None else rho
        eta = e0 if eta is None else eta
        got = got.detach().to("cpu", torch.float64)
        fin = torch.isfinite(self.ref)
        wrong_nonfinite = int((torch.isfinite(got) != fin).sum())
        err = (got - self.ref).abs()[fin]
        bound = (rho * self.mag + eta * self.L + self.kappa)[fin] + FLOOR
        if err.numel() == 0:
            return 0.0, wrong_nonfinite
        q = err / bound
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        return float(q.max()), wrong_nonfinite

    def check(self, got, rho=None, eta=None, what=""):
        ratio, wrong = self.ratio(got, rho, eta)
        assert wrong == 0, "%s: %d cells non-finite where the reference is not, or the other way round" % (what, wrong)
        assert ratio <= 1.0, "%s: per-cell error / bound = %.3g" % (what, ratio)
        return ratio


def global_close(got, ref, tol):
    """The suite's old yardstick (test_gpu_parity._close, relative): max|got - ref| <= tol (1 + max|ref|)."""
    got = got.detach().to("cpu", torch.float64)
    return float((got - ref).abs().max()) <= tol * (1 + float(ref.abs().max()))


def local_max(absg, R, out_hw):
    """Per-channel max of |g| over the pixels within R = (R_y, R_x) of each cell, on a cell grid of out_hw (clamped indices
    where the cell grid is larger than the pixel grid).  Non-finite gradients do not count (their cells are compared for
    non-finiteness instead)."""
    a = torch.where(torch.isfinite(absg), absg, torch.zeros_like(absg)).to(torch.float64)
    B, C, H, W = a.shape
    ry, rx = min(R[0], H - 1), min(R[1], W - 1)
    m = F.max_pool2d(a, (2 * ry + 1, 2 * rx + 1), stride=1, padding=(ry, rx)) if (ry or rx) else a
    Ho, Wo = out_hw
    iy = torch.arange(Ho).clamp(max=H - 1)
    ix = torch.arange(Wo).clamp(max=W - 1)
    return m[:, :, iy][:, :, :, ix].contiguous()


# ------------------------------------------------------------------------------------------------ resample2d d_input1
def _gauss_f32(v, sigma):
    """The reference's exp(SAFE_DIV(-v*v, 2*sigma*sigma)) in float32 arithmetic (resample2d_kernel.cu:72-75)."""
    num = -v * v
    den = 2 * sigma * sigma
    q = torch.where(den == 0, num.double() / 1e-8, (num / torch.where(den == 0, torch.ones_like(den), den)).double())
    return torch.exp(q).float()


def _rs_taps_f32(in2, ks, quirk=True, Hi=None, Wi=None):
    """The reference's float32 weight products of every tap of every pixel, with the (clamped) cell each lands on, and their
    float32 sum in the reference's order (resample2d_kernel.cu:140-200): ([(product, row, col)], sum), all [B, H, W]."""
    in2 = in2.float()
    B, _, H, W = in2.shape
    Hi, Wi = Hi or H, Wi or W
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    xf, yf = xs + in2[:, 0], ys + in2[:, 1]
    sig = in2[:, 2]
    if quirk:
        alpha, beta = xf - torch.trunc(xf), yf - torch.trunc(yf)
    else:
        alpha, beta = xf - torch.floor(xf), yf - torch.floor(yf)
    fx0, fy0 = torch.floor(xf), torch.floor(yf)

    def cell(v, n):
        return torch.nan_to_num(v, nan=0.0).clamp(-2.0 ** 31, 2.0 ** 31 - 1).long().clamp(0, n - 1)

    taps, s = [], torch.zeros(B, H, W, dtype=torch.float32)
    for fy in range(ks // 2):
        for fx in range(ks // 2):
            xL = _gauss_f32(fx + alpha, sig)
            xR = _gauss_f32(torch.tensor(1.0 + fx, dtype=torch.float32) - alpha, sig)
            yT = _gauss_f32(fy + beta, sig)
            yB = _gauss_f32(torch.tensor(1.0 + fy, dtype=torch.float32) - beta, sig)
            s = s + (yT * xL + yT * xR + yB * xL + yB * xR)
            rT, rB = cell(fy0 - fy, Hi), cell(fy0 + (fy + 1), Hi)
            cL, cR = cell(fx0 - fx, Wi), cell(fx0 + (fx + 1), Wi)
            taps += [(yT * xL, rT, cL), (yT * xR, rT, cR), (yB * xL, rB, cL), (yB * xR, rB, cR)]
    return taps, s


def resample2d_weight_sum_f32(in2, ks, quirk=True):
    """The reference's float32 sum of a pixel's (ks/2 x 2)^2 weight products, [B, H, W] (resample2d_kernel.cu:140-162)."""
    return _rs_taps_f32(in2, ks, quirk)[1]


def resample2d_bwd1_oracle(in1_shape, in2, go, ks, quirk=True, dtype=torch.float64):
    """The oracle's d_input1 alone (dilation 1), computed in `dtype`."""
    import oracle
    _, C, Hi, Wi = in1_shape
    B, _, H, W = in2.shape
    in2 = in2.to(dtype).contiguous()
    go = go.to(dtype).contiguous()
    g1 = torch.zeros(B, C, Hi, Wi, dtype=dtype)
    oracle._call("oracle_resample2d_backward_input1", g1, oracle._p(in2), oracle._p(go), oracle._p(g1), oracle._i64(B),
                 oracle._i64(C), oracle._i64(Hi), oracle._i64(Wi), oracle._i64(H), oracle._i64(W), oracle._i32(ks), oracle._i32(1),
                 oracle._i32(1 if quirk else 0))
    return g1


def resample2d_bound(in1_shape, in2, go, ks, quirk=True, dtype=torch.float32, R=R_RESAMPLE):
    """Bound of resample2d's d_input1 (dilation 1) for an implementation computing in `dtype`."""
    B, C, H, W = go.shape
    Hi, Wi = in1_shape[2], in1_shape[3]
    absg = go.double().abs()
    u = unit_roundoff(dtype)
    sig = in2[:, 2:3].double()
    vmax = ks // 2 + 1                                  # the farthest tap (quirk: alpha in (-1, 1))
    A = torch.where(sig != 0, (vmax * vmax / 2.0) / (sig * sig), torch.full_like(sig, math.inf))
    A = A.clamp(max=104.0 if dtype == torch.float32 else 745.0)
    cond = 4 * u * A
    g = go.double()
    under = torch.zeros(B, C, Hi * Wi, dtype=torch.float64)
    if float(A.max()) <= 40.0:
        # every float product is >= exp(-2 A) > 2^-126: nothing underflows, and kappa <= 4 u max(A) mag (one oracle pass less)
        ref = resample2d_bwd1_oracle(in1_shape, in2, g, ks, quirk)
        mag = resample2d_bwd1_oracle(in1_shape, in2, absg, ks, quirk)
        return Bound(ref, mag, local_max(absg, R, (Hi, Wi)), 4 * u * float(A.max()) * mag, dtype)
    if dtype == torch.float32:
        taps, s = _rs_taps_f32(in2, ks, quirk, Hi, Wi)
        s = s[:, None]
        dead = s == 0                                   # every product underflowed: the reference adds nothing
        cond = torch.where((s > 0) & (s < SUBNORMAL_SUM), torch.ones_like(cond), cond)
        g = torch.where(dead, torch.zeros_like(g), g)
        absg_live = torch.where(dead, torch.zeros_like(absg), absg)
        # a single product below the normal range has no relative precision: its normalised weight, true or float, is below
        # 2^-126 / sum -- the absolute slack of that tap
        d = torch.where(s > 0, 2.0 ** -126 / s.double(), torch.zeros_like(s, dtype=torch.float64)) * absg_live
        for prod, row, col in taps:
            small = (prod < 2.0 ** -126)[:, None]
            idx = (row * Wi + col).view(B, 1, H * W).expand(B, C, H * W)
            under.scatter_add_(2, idx, torch.where(small, d, torch.zeros_like(d)).reshape(B, C, H * W))
    else:
        absg_live = absg
    ref = resample2d_bwd1_oracle(in1_shape, in2, g, ks, quirk)
    mag = resample2d_bwd1_oracle(in1_shape, in2, absg_live, ks, quirk)
    kappa = resample2d_bwd1_oracle(in1_shape, in2, absg_live * cond, ks, quirk) + under.view(B, C, Hi, Wi)
    return Bound(ref, mag, local_max(absg, R, (Hi, Wi)), kappa, dtype)


# ------------------------------------------------------------------------------------------------ block extractor d_source
def _window_max(absgo, k):
    return F.max_pool2d(torch.where(torch.isfinite(absgo), absgo, torch.zeros_like(absgo)).double(), k, k)


def block_extractor_bound(src_shape, flow, go, k, dtype=torch.float32, R=R_BLOCK):
    import oracle
    Hs, Ws = src_shape[2], src_shape[3]
    fl = flow.double().contiguous()
    src0 = torch.zeros(src_shape, dtype=torch.float64)
    ref, _ = oracle.block_extractor_backward(src0, fl, go.double().contiguous(), k)
    mag, _ = oracle.block_extractor_backward(src0, fl, go.double().abs().contiguous(), k)
    return Bound(ref, mag, local_max(_window_max(go.double().abs(), k), R, (Hs, Ws)), None, dtype)


def attention_extractor_grad(w, go, k):
    """The k x k grad_output windows the block attention backward hands the extractor: (g / k^2) w_ij (avg_pool2d and the
    product's backward, formed in float64)."""
    import oracle
    gpool = (go.double() / (k * k)).repeat_interleave(k, 2).repeat_interleave(k, 3)
    wr = oracle.local_attn_reshape_forward(w.double().contiguous(), k)
    return (gpool * wr).contiguous()


def block_attention_bound(src_shape, flow, w, go, k, dtype=torch.float32, R=R_BLOCK):
    """d_source of BlockAttention: the extractor's bound on the windows (g / k^2) w_ij; mag with |g| and |w|."""
    import oracle
    Hs, Ws = src_shape[2], src_shape[3]
    fl = flow.double().contiguous()
    src0 = torch.zeros(src_shape, dtype=torch.float64)
    ref, _ = oracle.block_extractor_backward(src0, fl, attention_extractor_grad(w, go, k), k)
    gabs = attention_extractor_grad(w.double().abs(), go.double().abs(), k)
    mag, _ = oracle.block_extractor_backward(src0, fl, gabs, k)
    return Bound(ref, mag, local_max(_window_max(gabs, k), R, (Hs, Ws)), None, dtype)


# ------------------------------------------------------------------------------------------------ warp d_feat
def warp_bound(feat_shape, flow, go, dtype=torch.float32, R=R_WARP):
    import oracle
    Hi, Wi = feat_shape[2], feat_shape[3]
    fl = flow.double().contiguous()
    f0 = torch.zeros(feat_shape, dtype=torch.float64)
    ref, _ = oracle.warp_backward(f0, fl, go.double().contiguous())
    mag, _ = oracle.warp_backward(f0, fl, go.double().abs().contiguous())
    return Bound(ref, mag, local_max(go.double().abs(), R, (Hi, Wi)), None, dtype)


# ------------------------------------------------------------------------------------------------ input families
# (a) signed: randn, contributions cancel; (b) ramp: magnitudes exp(alpha x) from 1e-4 to 1 across the width, so the local maximum
# differs from the global one; (c) group_mags: channel magnitudes 1, 1e-5, 1e3, 1e-2 repeated -- inside one 4-channel group;
# (d) masked: one region zero, the rest log-normal; (e) tiny / huge: 1e-30 / 1e30.  (f) small sigma is resample2d's own (rs_small_sigma).
FAMILIES = ("signed", "ramp", "group_mags", "masked", "tiny", "huge")
GROUP_MAGS = (1.0, 1e-5, 1e3, 1e-2)


def family_grad(kind, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    g = torch.randn(shape, generator=gen)
    if kind == "ramp":
        g = g * torch.exp(math.log(1e-4) * (1 - torch.linspace(0, 1, W))).view(1, 1, 1, W)
    elif kind == "group_mags":
        g = g * torch.tensor(GROUP_MAGS * ((C + 3) // 4))[:C].view(1, C, 1, 1)
    elif kind == "masked":
        g = g.sign() * torch.exp(2 * torch.randn(shape, generator=gen))
        g[:, :, H // 8:(5 * H) // 8, W // 6:(4 * W) // 6] = 0
    elif kind == "tiny":
        g = g * 1e-30
    elif kind == "huge":
        g = g * 1e30
    elif kind != "signed":
        raise ValueError(kind)
    return g.contiguous()


def quantize(t, bits=10):
    """Values on a 2^-bits grid: pixel coordinates x + dx are then exact in float32 (|x + dx| < 2^(23 - bits)), so the fp32
    implementations and the float64 reference sample at the same points."""
    return torch.round(t * 2.0 ** bits) / 2.0 ** bits


def rs_flow(B, H, W, seed, reach=3.0, sigma=(0.5, 2.5)):
    """resample2d input2 = (dx, dy, sigma): flows U[-reach, reach) on the 2^-10 grid, sigma U[sigma)."""
    gen = torch.Generator().manual_seed(seed)
    fl = quantize((torch.rand(B, 2, H, W, generator=gen) * 2 - 1) * reach)
    sg = quantize(torch.rand(B, 1, H, W, generator=gen) * (sigma[1] - sigma[0]) + sigma[0])
    return torch.cat((fl, sg), 1).contiguous()


def rs_small_sigma(B, H, W, seed):
    """(f): sigma in {0.03, 0.04, 0.05, 0.1}, pixels near half-integers (|flow| < 3: the owned tiles) and, in the same call, every
    7th row / 5th column far beyond +-3 (the far kernel), so that both kernels meet the pixels whose float weight products
    underflow while the per-axis sums do not."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.randint(-2, 2, (B, 2, H, W), generator=gen).float()
    jitter = torch.randint(-160, 161, (B, 2, H, W), generator=gen).float() / 1024
    fl = base + 0.5 + jitter
    far = torch.zeros(B, 2, H, W, dtype=torch.bool)
    far[:, :, ::7] = True
    far[:, :, :, ::5] = True
    fl = torch.where(far, fl + torch.randint(4, 12, (B, 2, H, W), generator=gen).float() * (torch.randint(0, 2, (B, 2, H, W), generator=gen) * 2 - 1), fl)
    sg = torch.tensor([0.03, 0.04, 0.05, 0.1])[torch.randint(0, 4, (B, 1, H, W), generator=gen)]
    return torch.cat((fl, sg), 1).contiguous()


def block_flow(B, H, W, seed, reach=2.0):
    gen = torch.Generator().manual_seed(seed)
    return quantize((torch.rand(B, 2, H, W, generator=gen) * 2 - 1) * reach).contiguous()


def warp_grid(B, H, W, seed, reach=2.0):
    """grid_sample coordinates (normalised, align_corners=False) of the identity plus U[-reach, reach) pixels on the 2^-8 grid;
    with power-of-two H, W the unnormalisation ((x + 1) W - 1) / 2 is exact in float32."""
    gen = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ix = xs + quantize((torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 2 - 1) * reach, 8)
    iy = ys + quantize((torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 2 - 1) * reach, 8)
    return torch.stack(((2 * ix + 1) / W - 1, (2 * iy + 1) / H - 1), 1).float().contiguous()
