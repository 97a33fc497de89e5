"""Per-element float64 error bounds for the FORWARD outputs of the sampling operators (a plain helper module, not a conftest).

The warp, resample2d, the block extractor and block attention have per-element bounds on their backward outputs
(tests/scatter_bounds.py, tests/gather_bounds.py).  Their forward outputs -- the values the network consumes -- were held to one
global ``max|diff| <= 2e-6`` on ``torch.rand`` inputs, which passes a wrong tap, a dropped weight or a wrong normalisation wherever
the element's own terms are small: a zero-padded band, a quiet channel next to a loud one, a masked region, data of scale 1e-30.
For one forward output element:

  ref    the float64 oracle's forward (block attention: the composition avg_pool2d(extract x reshape(w), k, k) that
         test_gpu_parity._attention_reference uses, in float64);
  mag    the same forward of |source| (and |weights| for attention).  Every interpolation weight is non-negative (bilinear,
         normalised Gaussian), so this is the sum of the absolute values of the element's terms: its condition number;
  kappa  the conditioning every fp32 implementation shares with the reference (below);

and the assertion, on every element where ref is finite,

    |got - ref| <= rho mag + kappa + 1e-38,

finiteness matching the reference at EVERY element (NaN and +-Inf of a source plane reach exactly the outputs whose taps touch
them, taps of weight 0 included: the reference multiplies; a corner the warp zero-pads is not a tap).

rho = SAFETY (n + TERM_OPS) u, SAFETY = 4 as in gather_bounds, u = 2^-24 (2^-53 for a float64 kernel).  n is the taps per element
-- warp and extractor 4, attention 4 k^2, resample2d 4 (ks/2)^2: a float sum of n terms in any order errs by at most (n - 1) u
sum|terms|.  TERM_OPS counts the roundings each term and the result carry besides, from the operator's own arithmetic:
  * warp 4: the two weight factors x1 - ix, y1 - iy (2; ix, iy themselves are kappa's), their product (1), the product with the
    sample (1).
  * block extractor 6: the factors 1 - (dx - fdx) round twice each (4; dx = pixel + flow + tap offset is exact for the flows used
    here), their product (1), the product with the sample (1).
  * block attention 8: the extractor's 6, the product with the attention weight (1), the scaling by 1 / k^2 (1); the pooling sum
    is inside n = 4 k^2.  (ba_fwd_pix_kernel contracts Wy^T (w / k^2) Wx first: the same factors in another order.)
  * resample2d 10 + n: per term the tap distance (1), the exp of each Gaussian factor (2; its EXPONENT is kappa's), their product
    (1), the product with the sample (1); the normalising sum adds its own n-term chain over products that carry 4 roundings each
    (n - 1 + 4, relative to the sum, hence to mag), and the division rounds once (1): n + 10 beside the numerator's n.
The float32 oracle must meet every bound at rho / SAFETY (tests/test_sample_forward_bounds_cpu.py) -- a derivation, not a
measurement.

kappa:
  * warp: ix = ((g + 1) W - 1) / 2 is three fp32 operations whose error |d ix| gather_bounds.warp_coordinate_error bounds (0 on
    power-of-two sizes with binary grids); the output moves by |d ix| S_x + |d iy| S_y with the float64 slopes of the bilinear
    patch per channel, S_x = (1 - ay) |s1 - s0| + ay |s3 - s2| and its transpose, invalid corners counting 0.
  * resample2d: 4 A u mag, A = min((ks/2 dilation + 1)^2 / (2 sigma^2), 104) as in scatter_bounds (the exponent of a Gaussian
    weight is a float quotient); and, for float32, n 2^-149 / sum: a term below the normal range rounds to a multiple of 2^-149 and
    the division by a small weight sum scales that up (under `tiny` with sigma about 0.1 every term is subnormal while the sum is a
    normal 1e-9: flushing them gives 0 where the reference gives 1e-30).
    Small sigma (A > 40) needs scatter_bounds.resample2d_bound's classification, from the reference's float32 weight products:
    a pixel whose products ALL underflow is `dead` -- SAFE_DIV(0, 0) = 0: ref = mag = 0, the kernel must write 0; a pixel whose
    float sum is below SUBNORMAL_SUM = 2^-100 gets its whole mag as slack (at most 5 % of the elements of a case may be judged so:
    SLACK_SHARE_CAP, asserted on the CPU); a single product below the normal range adds 2^-126 / sum times its |sample|.
    A float64 kernel has neither (its products stay normal) and is judged with u64 and A <= 745.
  * block extractor / attention: 0.

Inputs.  Flows are gather_bounds' `odd` multiples of 2^-9, so fp32 and float64 pick the same cell.  Source families: signed, ramp,
masked, tiny, huge (scatter_bounds.family_grad), feat_mags (the per-channel pattern 1, 1e-5, 1e3, 1e-2 inside each 4-channel group:
rs_fwd_lds_kernel and ba_fwd_pix_kernel keep four channels in one LDS cell, warp_fwd_body walks four per trip) and `nonfinite`:
signed, with NaN / +Inf / -Inf cells on a plane border, in the interior, in the last channel (the last of its slab) and in the
last channel of the first group of four; three rows of flow pixels around the interior cell sit on exact integers there, so
that cell is also touched with weight 0 (the warp: on power-of-two sizes only, where the fp32 coordinate is exact).  For the
warp's LDS tiles the family adds a NaN at the first cell of the staged box of every tile that has pixels WITHOUT a valid corner
next to pixels with one (warp_lds_dead_origins): such a pixel's output is 0 in the reference whatever the box holds.
`exact` (warp on power-of-two sizes, extractor): integer sources below 32 in magnitude, flows on multiples of 2^-9 with every
third row on exact integers: every weight is a multiple of 2^-18, every product and partial sum exact in fp32 in any order:
equality with the float64 reference, and on the integer rows (weights 0 and 1) the output equals the source value.
"""
import functools
import math

import torch
import torch.nn.functional as F

import gather_bounds as gb
import scatter_bounds as sb

SAFETY = gb.SAFETY
FLOOR = gb.FLOOR
TERM_OPS = {"warp": 4, "block_extractor": 6, "block_attention": 8, "resample2d": 10}
SOURCE_FAMILIES = ("signed", "feat_mags", "ramp", "masked", "tiny", "huge", "nonfinite")
OLD_YARDSTICK = 2e-6
SLACK_SHARE_CAP = 0.05
SMALL_SIGMAS = (0.02, 0.03, 0.08, 0.09, 0.1, 0.1)
Bound = gb.Bound
NAN, INF = float("nan"), float("inf")


def taps(op, k=None):
    return {"warp": 4, "block_extractor": 4, "block_attention": 4 * (k or 0) ** 2, "resample2d": 4 * ((k or 0) // 2) ** 2}[op]


def rho_units(op, k=None):
    """rho in units of u: SAFETY (n + TERM_OPS), resample2d's normalising sum adding its own n."""
    n = taps(op, k)
    return SAFETY * (n + TERM_OPS[op] + (n if op == "resample2d" else 0))


def old_yardstick(got, ref, tol=OLD_YARDSTICK):
    """The forward tests' former assertion, max|got - ref| <= 2e-6, over the elements where the reference is finite."""
    got = got.detach().to("cpu", torch.float64)
    fin = torch.isfinite(ref)
    d = (got - ref).abs()[fin]
    return bool(torch.isfinite(d).all()) and float(d.max()) <= tol


# ------------------------------------------------------------------------------------------------ inputs
def nonfinite_cells(shape):
    B, C, H, W = shape
    cells = [((0, 0, 0, W // 3), NAN), ((0, min(1, C - 1), H // 2, W // 2), INF), ((B - 1, C - 1, H // 3, (2 * W) // 3), -INF),
             ((0, C - 1, H - 1, W - 1), NAN)]
    if C > 4:
        cells.append(((0, 3, (2 * H) // 3, W // 4), NAN))
    return cells


def source(kind, shape, seed, extra_cells=()):
    """A source tensor of the family (float32); `nonfinite`: signed with nonfinite_cells and `extra_cells` [(b, c, y, x)] as NaN."""
    fam = {"feat_mags": "group_mags", "nonfinite": "signed"}.get(kind, kind)
    s = sb.family_grad(fam, shape, seed)
    if kind == "nonfinite":
        for at, v in nonfinite_cells(shape):
            s[at] = v
        for at in extra_cells:
            s[at] = NAN
    return s.contiguous()


def attention_weights(kind, shape, seed):
    """Signed randn; `feat_mags`: times the pattern 1, 1e-5, 1e3, 1e-2 over the nine taps."""
    w = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    if kind == "feat_mags":
        w = w * torch.tensor(sb.GROUP_MAGS * 3)[:shape[1]].view(1, -1, 1, 1)
    return w.contiguous()


def integer_rows(Hs, Hf):
    """The rows of flow pixels put on exact integers under `nonfinite`: around the source's interior cell (Hs // 2)."""
    return slice(max(Hs // 2 - 1, 0), min(Hs // 2 + 2, Hf))


def block_flow(kind, B, Hs, Hf, Wf, seed, reach):
    flow = gb.block_flow(B, Hf, Wf, seed, reach)
    if kind == "nonfinite":
        flow[:, :, integer_rows(Hs, Hf)] = 0
    return flow.contiguous()


def rs_flow(kind, B, Hi, H, W, seed, reach, sigma):
    in2 = gb.rs_flow(B, H, W, seed, reach, sigma)
    if kind == "nonfinite":
        in2[:, :2, integer_rows(Hi, H)] = 0
    return in2.contiguous()


def rs_small_sigma(B, H, W, seed):
    """scatter_bounds.rs_small_sigma's flows (half-integers +- 0.16, a far row / column every 7th / 5th) with the sigma set
    SMALL_SIGMAS: 0.02 and 0.03 underflow every product (dead pixels); 0.08 .. 0.1 underflow the far products and keep the sum
    above 2^-100, at dilation 2 as well.  sb's own set {0.03, 0.04, 0.05, 0.1} puts 45 % of the pixels into the slack arm, and the
    mixed regime (0.045; 0.07 at dilation 2) is left out altogether: where ONE product survives as a multiple of 2^-149 the float32
    reference returns that single sample, up to max|sample| + |ref| from the float64 value -- it missed `mag` itself by a factor
    1.07 on [1, 6, 37, 70] -- so no input can keep the reference inside the slack arm, and the arm stays empty on these inputs
    (asserted on the CPU: the share is within the cap of 5 %)."""
    in2 = sb.rs_small_sigma(B, H, W, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    in2[:, 2:] = torch.tensor(SMALL_SIGMAS)[torch.randint(0, len(SMALL_SIGMAS), (B, 1, H, W), generator=gen)]
    return in2.contiguous()


def rs_sigma_zero(B, H, W, seed):
    """sigma = 0 (SAFE_DIV's EPS arm: the exponent is -v^2 / 1e-8): odd flows give weight 0 everywhere (output 0), the pixels of
    every other row sit on exact integers, where the one tap at distance 0 has weight 1 and the output is the source value."""
    in2 = gb.rs_flow(B, H, W, seed, 3.0, (0.5, 2.5))
    in2[:, :2, ::2] = torch.round(in2[:, :2, ::2])
    in2[:, 2] = 0
    return in2.contiguous()


def rs_sigma_tenth(B, H, W, seed):
    """sigma = 0.1 on sb.rs_small_sigma's flows: weight sums of about 1e-9, normal; under `tiny` every term is subnormal."""
    in2 = sb.rs_small_sigma(B, H, W, seed)
    in2[:, 2] = 0.1
    return in2.contiguous()


def warp_grid(kind, grid_kind, B, in_hw, out_hw, seed):
    grid = gb.warp_grid(grid_kind, B, in_hw, out_hw, seed)
    Hi, Wi = in_hw
    if kind == "nonfinite" and in_hw == out_hw and gb._pow2(Hi) and gb._pow2(Wi):
        rows = integer_rows(Hi, Hi)
        xs = torch.arange(Wi, dtype=torch.float64)
        ys = torch.arange(Hi, dtype=torch.float64)[rows]
        grid[:, 0, rows] = ((2 * xs + 1) / Wi - 1).float().view(1, 1, Wi)
        grid[:, 1, rows] = ((2 * ys + 1) / Hi - 1).float().view(1, -1, 1)
    return grid.contiguous()


def warp_lds_dead_origins(grid, in_hw, limit=3):
    """[(b, 0, y, x)]: the first cell of the staged box of the 64 x 16 pixel tiles of the warp's LDS kernels (box as in
    gather_bounds.warp_lds_boxes, the kernel's float32 arithmetic) that hold a pixel without a valid corner beside pixels with
    one, where that cell lies inside the image and the box fits 128 x 32 cells."""
    Hi, Wi = in_hw
    g = grid.float()
    B, _, H, W = g.shape
    x0 = torch.floor(((g[:, 0] + 1) * float(Wi) - 1) / 2)
    y0 = torch.floor(((g[:, 1] + 1) * float(Hi) - 1) / 2)
    live = (x0 >= -1) & (x0 <= Wi - 1) & (y0 >= -1) & (y0 <= Hi - 1)
    cells = []
    for b in range(B):
        for ty in range(0, H, 16):
            for tx in range(0, W, 64):
                m = live[b, ty:ty + 16, tx:tx + 64]
                if bool(m.all()) or not bool(m.any()):
                    continue
                xs, ys = x0[b, ty:ty + 16, tx:tx + 64][m].long(), y0[b, ty:ty + 16, tx:tx + 64][m].long()
                bx0, by0 = (int(xs.min()) // 4) * 4, int(ys.min())
                fits = int(xs.max()) + 2 - bx0 <= 128 and int(ys.max()) + 2 - by0 <= 32
                if fits and 0 <= bx0 < Wi and 0 <= by0 < Hi and len(cells) < limit:
                    cells.append((b, 0, by0, bx0))
    return cells


def warp_sampled_cells(grid, in_hw):
    """[(0, 0, y, x)]: the north-west corner cells of two pixels of image 0, where they lie inside the image (a zooming grid skips
    cells, so a fixed cell may have no pixel that samples it)."""
    Hi, Wi = in_hw
    g = grid.float()
    H, W = g.shape[2:]
    cells = []
    for y, x in ((H // 2, W // 2), (H // 4, (3 * W) // 4)):
        x0 = int(torch.floor(((g[0, 0, y, x] + 1) * float(Wi) - 1) / 2))
        y0 = int(torch.floor(((g[0, 1, y, x] + 1) * float(Hi) - 1) / 2))
        if 0 <= x0 < Wi and 0 <= y0 < Hi:
            cells.append((0, 0, y0, x0))
    return cells


def exact_source(shape, seed):
    return torch.randint(-31, 32, shape, generator=torch.Generator().manual_seed(seed)).float().contiguous()


def exact_offsets(B, H, W, seed, reach):
    """[B, 2, H, W] multiples of 2^-9 in [-reach, reach], every third row on exact integers."""
    gen = torch.Generator().manual_seed(seed)
    off = sb.quantize((torch.rand(B, 2, H, W, generator=gen, dtype=torch.float64) * 2 - 1) * reach, 9)
    off[:, :, ::3] = torch.round(off[:, :, ::3])
    return off


def exact_warp_grid(B, H, W, seed, reach=3.0):
    """Identity + exact_offsets on a power-of-two size: grid, ((g + 1) W - 1) / 2 and every weight are exact in fp32."""
    assert gb._pow2(H) and gb._pow2(W)
    off = exact_offsets(B, H, W, seed, reach)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ix, iy = xs + off[:, 0], ys + off[:, 1]
    grid = torch.stack(((2 * ix + 1) / W - 1, (2 * iy + 1) / H - 1), 1)
    assert bool((grid.float().double() == grid).all())
    return grid.float().contiguous()


# ------------------------------------------------------------------------------------------------ warp
def warp_parts(feat, grid):
    """The float64 restatement's pieces: (s, w, valid) -- four corner samples [B, C, N] (gathered at the clamped index), four
    weights [B, 1, N] and four validity masks [B, 1, N], corner order nw, ne, sw, se -- and (ax, ay) [B, 1, N]."""
    feat, grid = feat.double(), grid.double()
    B, C, Hi, Wi = feat.shape
    N = grid.shape[2] * grid.shape[3]
    ix = (((grid[:, 0] + 1) * Wi - 1) / 2).reshape(B, N)
    iy = (((grid[:, 1] + 1) * Hi - 1) / 2).reshape(B, N)
    fx, fy = torch.floor(ix), torch.floor(iy)
    ax, ay = (ix - fx).unsqueeze(1), (iy - fy).unsqueeze(1)
    x0, y0 = fx.clamp(-2.0 ** 40, 2.0 ** 40).long(), fy.clamp(-2.0 ** 40, 2.0 ** 40).long()
    planes = feat.reshape(B, C, Hi * Wi)
    s, valid = [], []
    for yy, xx in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
        valid.append(((yy >= 0) & (yy < Hi) & (xx >= 0) & (xx < Wi)).unsqueeze(1))
        s.append(gb._gather(planes, yy.clamp(0, Hi - 1), xx.clamp(0, Wi - 1), Wi))
    w = [(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay]
    return s, w, valid, ax, ay


def warp_compose(s, w, valid, shape, flipcat=False):
    """sum over the valid corners of s w (an invalid corner is no tap: it adds nothing, whatever it holds) -> [B, C or 2C, H, W]."""
    out = sum(torch.where(v, sq * wq, torch.zeros_like(sq)) for sq, wq, v in zip(s, w, valid))
    out = out.view(out.shape[0], out.shape[1], shape[0], shape[1])
    return torch.cat((out, out.flip(3)), 1) if flipcat else out


def warp_bound(feat, grid, flipcat=False, dtype=torch.float32):
    import oracle
    B, C, Hi, Wi = feat.shape
    H, W = grid.shape[2:]
    f64, g64 = feat.double().contiguous(), grid.double().contiguous()
    ref = oracle.warp_forward(f64, g64, flipcat)
    mag = oracle.warp_forward(f64.abs(), g64, flipcat)
    u = sb.unit_roundoff(dtype)
    dix, diy = gb.warp_coordinate_error(grid[:, 0], Wi, u), gb.warp_coordinate_error(grid[:, 1], Hi, u)
    kappa = None
    if dix or diy:
        s, _, valid, ax, ay = warp_parts(feat, grid)
        z = [torch.where(v, sq, torch.zeros_like(sq)) for sq, v in zip(s, valid)]
        sx = (1 - ay) * (z[1] - z[0]).abs() + ay * (z[3] - z[2]).abs()
        sy = (1 - ax) * (z[2] - z[0]).abs() + ax * (z[3] - z[1]).abs()
        kappa = (dix * sx + diy * sy).view(B, C, H, W)
        if flipcat:
            kappa = torch.cat((kappa, kappa.flip(3)), 1)
    return Bound(ref, mag, kappa, rho_units("warp"), dtype)


# ------------------------------------------------------------------------------------------------ block extractor / attention
def block_extractor_bound(src, flow, k, dtype=torch.float32):
    import oracle
    s64, f64 = src.double().contiguous(), flow.double().contiguous()
    return Bound(oracle.block_extractor_forward(s64, f64, k), oracle.block_extractor_forward(s64.abs(), f64, k), None,
                 rho_units("block_extractor"), dtype)


def attention_composition(oracle, src, flow, w, k):
    """test_gpu_parity._attention_reference's forward, in the dtype of its arguments."""
    return F.avg_pool2d(oracle.block_extractor_forward(src, flow, k) * oracle.local_attn_reshape_forward(w, k), k, k)


def block_attention_bound(src, flow, w, k, dtype=torch.float32):
    import oracle
    s64, f64, w64 = src.double().contiguous(), flow.double().contiguous(), w.double().contiguous()
    return Bound(attention_composition(oracle, s64, f64, w64, k), attention_composition(oracle, s64.abs(), f64, w64.abs(), k), None,
                 rho_units("block_attention", k), dtype)


# ------------------------------------------------------------------------------------------------ resample2d
def _gauss(v, sigma):
    if v.dtype == torch.float32:
        return sb._gauss_f32(v, sigma)
    num, den = -v * v, 2 * sigma * sigma
    return torch.exp(torch.where(den == 0, num / 1e-8, num / torch.where(den == 0, torch.ones_like(den), den)))


def rs_taps(in2, ks, dil, Hi, Wi, dtype):
    """The reference's forward taps (resample2d_kernel.cu:52-91) in `dtype` arithmetic: ([(wy, wx, row, col)] in the reference's
    order, their sum in the reference's order, (sum of the x factors, sum of the y factors) per axis), all [B, H, W]."""
    in2 = in2.to(dtype)
    B, _, H, W = in2.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    xf, yf, sig = xs + in2[:, 0], ys + in2[:, 1], in2[:, 2]
    fx0, fy0 = torch.floor(xf), torch.floor(yf)
    alpha, beta = xf - fx0, yf - fy0

    def cell(v, n):
        return torch.nan_to_num(v, nan=0.0).clamp(-2.0 ** 31, 2.0 ** 31 - 1).long().clamp(0, n - 1)

    out, s = [], torch.zeros(B, H, W, dtype=dtype)
    sx, sy = torch.zeros_like(s), torch.zeros_like(s)
    for fy in range(ks // 2):
        yT, yB = _gauss(fy * dil + beta, sig), _gauss(torch.tensor(float((1 + fy) * dil), dtype=dtype) - beta, sig)
        rT, rB = cell(fy0 - fy * dil, Hi), cell(fy0 + (fy + 1) * dil, Hi)
        sy = sy + (yT + yB)
        for fx in range(ks // 2):
            xL, xR = _gauss(fx * dil + alpha, sig), _gauss(torch.tensor(float((1 + fx) * dil), dtype=dtype) - alpha, sig)
            cL, cR = cell(fx0 - fx * dil, Wi), cell(fx0 + (fx + 1) * dil, Wi)
            if fy == 0:
                sx = sx + (xL + xR)
            s = s + (yT * xL + yT * xR + yB * xL + yB * xR)
            out += [(yT, xL, rT, cL), (yT, xR, rT, cR), (yB, xL, rB, cL), (yB, xR, rB, cR)]
    return out, s, (sx, sy)


def _safe_div(a, b):
    return torch.where(b == 0, a / 1e-8, a / torch.where(b == 0, torch.ones_like(b), b))


def _flush(t):
    return torch.where(t.abs() < 2.0 ** -126, torch.zeros_like(t), t)


def rs_forward_torch(in1, in2, ks, dil=1, dtype=torch.float32, mode=None):
    """A stand-in of the forward in `dtype` torch arithmetic, tap by tap in the reference's order.  mode (the mutants of the CPU
    tests): "per_axis" normalises each axis by its own sum instead of the 2-D sum; "flush" flushes every product below the normal
    range to zero."""
    B, _, H, W = in2.shape
    _, C, Hi, Wi = in1.shape
    tp, s, (sx, sy) = rs_taps(in2, ks, dil, Hi, Wi, dtype)
    planes = in1[:B].to(dtype).reshape(B, C, Hi * Wi)
    val = torch.zeros(B, C, H * W, dtype=dtype)
    for wy, wx, row, col in tp:
        v = gb._gather(planes, row.reshape(B, -1), col.reshape(B, -1), Wi)
        if mode == "per_axis":
            p = (_safe_div(wy, sy) * _safe_div(wx, sx)).reshape(B, 1, -1) * v
        elif mode == "flush":
            p = _flush(_flush(wy * wx).reshape(B, 1, -1) * v)
        else:
            p = (wy * wx).reshape(B, 1, -1) * v
        val = val + p
    out = val if mode == "per_axis" else _safe_div(val, s.reshape(B, 1, -1).expand_as(val))
    return out.view(B, C, H, W)


class RsBound(Bound):
    """A resample2d bound with its classification: `dead` and `slack` [B, 1, H, W] masks (all False outside the small-sigma arm)."""

    def slack_share(self):
        return float(self.slack.double().mean())


def resample2d_bound(in1, in2, ks, dil=1, dtype=torch.float32):
    import oracle
    B, _, H, W = in2.shape
    _, C, Hi, Wi = in1.shape
    i64, f64 = in1.double().contiguous(), in2.double().contiguous()
    ref = oracle.resample2d_forward(i64, f64, ks, dil)
    mag = oracle.resample2d_forward(i64.abs(), f64, ks, dil)
    u = sb.unit_roundoff(dtype)
    n = taps("resample2d", ks)
    sig = in2[:, 2:3].double()
    vmax = (ks // 2) * dil + 1
    A = torch.where(sig != 0, (vmax * vmax / 2.0) / (sig * sig), torch.full_like(sig, math.inf))
    A = A.clamp(max=104.0 if dtype == torch.float32 else 745.0)
    kappa = 4 * u * A * mag
    dead = torch.zeros(B, 1, H, W, dtype=torch.bool)
    slack = dead.clone()
    if dtype == torch.float32:
        tp, s, _ = rs_taps(in2, ks, dil, Hi, Wi, torch.float32)
        s = s[:, None].double()
        live = s > 0
        inv = torch.where(live, 1.0 / torch.where(live, s, torch.ones_like(s)), torch.zeros_like(s))
        kappa = kappa + n * 2.0 ** -149 * inv
        if float(A.max()) > 40.0:
            dead, slack = ~live, live & (s < sb.SUBNORMAL_SUM)
            planes = i64[:B].abs().reshape(B, C, Hi * Wi)
            under = torch.zeros(B, C, H * W, dtype=torch.float64)
            for wy, wx, row, col in tp:
                small = ((wy * wx) < 2.0 ** -126).reshape(B, 1, -1)
                v = gb._gather(planes, row.reshape(B, -1), col.reshape(B, -1), Wi)
                under += torch.where(small, (2.0 ** -126 * inv).reshape(B, 1, -1) * v, torch.zeros_like(v))
            kappa = torch.where(slack, mag, kappa + under.view(B, C, H, W))
            zero = dead & torch.isfinite(ref)             # (a non-finite sample times a weight of 0 stays NaN in the reference)
            ref = torch.where(zero, torch.zeros_like(ref), ref)
            mag = torch.where(zero, torch.zeros_like(mag), mag)
            kappa = torch.where(dead, torch.zeros_like(kappa), kappa)
    bound = RsBound(ref, mag, kappa, rho_units("resample2d", ks), dtype)
    bound.dead, bound.slack = dead, slack
    return bound


# ------------------------------------------------------------------------------------------------ the cases of the GPU matrix
# Shared by tests/test_gpu_sample_forward_bounds.py (the kernels) and tests/test_sample_forward_bounds_cpu.py (the float32 oracle at
# the same shapes and families).  Every builder is cached: the float64 reference is computed once and never modified.

# name: (feature shape, grid size or None (= the feature's), dtype).  Shapes are gather_bounds.WARP_CASES' where they serve.
WARP_CASES = {
    "c5_64": ((2, 5, 64, 64), None, torch.float32),
    "c7": ((1, 7, 33, 70), None, torch.float32),
    "small": ((2, 5, 12, 10), None, torch.float32),
    "grids": ((1, 3, 96, 130), (80, 129), torch.float32),
    "trip5": ((4, 5, 512, 512), None, torch.float32),       # 4096 tiles: plan() keeps the whole slab -- one four-channel trip + 1
    "trip7": ((4, 7, 512, 512), None, torch.float32),       # ... + 3
    "slabs": ((2, 8, 512, 512), None, torch.float32),       # 2048 tiles: two slabs of 4 channels
    "small_f64": ((2, 5, 12, 10), None, torch.float64),
    "c7_f64": ((1, 7, 33, 70), None, torch.float64),
    "ragged_w": ((1, 6, 70, 67), None, torch.float32),
    "c2_66": ((1, 2, 66, 66), None, torch.float32),
    "natural": ((4, 64, 256, 256), None, torch.float32),    # exactly 2^24 elements: the default route's LDS kernel
    "m_lds32": ((1, 32, 32, 32), None, torch.float32),      # >= 32 channels on >= 32 x 32 pixels: the multi launch's LDS arm
    "m_lds40": ((1, 33, 40, 36), None, torch.float32),
    "m_lds64": ((1, 40, 64, 32), None, torch.float32),
}


def warp_forward_slab(B, C, H, W, cs_default=16):
    """Channels per block of warp_fwd_kernel (csrc/runtime.hip plan() with the forward's default of 16)."""
    return gb.warp_pixel_slab(B, C, H, W, cs_default)


@functools.lru_cache(maxsize=None)
def warp_case(name, grid_kind, kind, flipcat):
    shape, grid_hw, dtype = WARP_CASES[name]
    B, C, Hi, Wi = shape
    H, W = grid_hw or (Hi, Wi)
    grid = warp_grid(kind, grid_kind, B, (Hi, Wi), (H, W), 261)
    extra = warp_lds_dead_origins(grid, (Hi, Wi)) + warp_sampled_cells(grid, (Hi, Wi)) if kind == "nonfinite" else ()
    feat = source(kind, shape, 260, extra)
    return feat, grid, warp_bound(feat, grid, flipcat, dtype)


@functools.lru_cache(maxsize=None)
def warp_exact_case(shape, flipcat):
    """(feat, grid, float64 reference) of the exact family."""
    import oracle
    B, C, H, W = shape
    feat, grid = exact_source(shape, 262), exact_warp_grid(B, H, W, 263)
    return feat, grid, oracle.warp_forward(feat.double(), grid.double(), flipcat)


# name: (source shape, flow grid or None, k, flow reach, dtype)
BE_CASES = {
    "k1": ((1, 3, 20, 33), None, 1, 2.0, torch.float32),
    "k2": ((1, 3, 20, 33), None, 2, 2.0, torch.float32),
    "k3": ((1, 5, 37, 70), None, 3, 2.0, torch.float32),
    "k4": ((1, 3, 20, 33), None, 4, 2.0, torch.float32),
    "k3_f64": ((1, 5, 37, 70), None, 3, 2.0, torch.float64),
    "rows4": ((1, 8, 150, 200), None, 3, 2.0, torch.float32),            # Hf >= 64: four pixel rows per thread
    "rows4_far": ((1, 8, 150, 200), None, 3, 24.0, torch.float32),
    "k5": ((1, 3, 20, 33), None, 5, 2.0, torch.float32),
    "k6": ((1, 2, 10, 10), None, 6, 2.0, torch.float32),
    "k7": ((1, 2, 20, 33), None, 7, 2.0, torch.float32),
    "k9": ((1, 2, 9, 9), (4, 4), 9, 2.0, torch.float32),
    "grids": ((1, 2, 16, 16), (9, 21), 3, 2.0, torch.float32),
}


@functools.lru_cache(maxsize=None)
def be_case(name, kind):
    shape, grid, k, reach, dtype = BE_CASES[name]
    B, C, Hs, Ws = shape
    Hf, Wf = grid or (Hs, Ws)
    src = source(kind, shape, 240)
    flow = block_flow(kind, B, Hs, Hf, Wf, 241, reach)
    return src, flow, k, block_extractor_bound(src, flow, k, dtype)


@functools.lru_cache(maxsize=None)
def be_exact_case(name):
    import oracle
    shape, grid, k, reach, _ = BE_CASES[name]
    B, C, Hs, Ws = shape
    Hf, Wf = grid or (Hs, Ws)
    src, flow = exact_source(shape, 242), exact_offsets(B, Hf, Wf, 243, reach).float().contiguous()
    return src, flow, k, oracle.block_extractor_forward(src.double(), flow.double(), k)


# name: (source shape, k, dtype)
BA_CASES = {
    "c8": ((1, 8, 100, 140), 3, torch.float32),
    "c6": ((1, 6, 100, 140), 3, torch.float32),
    "low": ((1, 6, 40, 70), 3, torch.float32),                           # Hf < 64
    "k2": ((1, 3, 20, 33), 2, torch.float32),                            # the generic kernel
    "c6_f64": ((1, 6, 40, 70), 3, torch.float64),
}


@functools.lru_cache(maxsize=None)
def ba_case(name, kind, wkind):
    shape, k, dtype = BA_CASES[name]
    B, C, H, W = shape
    src = source(kind, shape, 250)
    flow = block_flow(kind, B, H, H, W, 251, 2.0)
    w = attention_weights(wkind, (B, k * k, H, W), 252)
    return src, flow, w, k, block_attention_bound(src, flow, w, k, dtype)


# name: (in1 shape, flow grid or None, kernel_size, dilation, flow: reach or a generator's name, sigma range, dtype)
RS_CASES = {
    "lds_c6": ((1, 6, 37, 70), None, 4, 1, 3.0, (0.5, 2.5), torch.float32),
    "lds_c5_ks2": ((1, 5, 37, 70), None, 2, 1, 3.0, (0.5, 2.5), torch.float32),
    "lds_c7_ks6": ((1, 7, 37, 70), None, 6, 1, 3.0, (0.5, 2.5), torch.float32),
    "lds_c5_ks5": ((1, 5, 37, 70), None, 5, 1, 3.0, (0.5, 2.5), torch.float32),      # odd kernel_size: ks / 2 = 2
    "lds_grids": ((1, 8, 24, 30), (17, 40), 4, 1, 3.0, (0.5, 2.5), torch.float32),
    "lds_fallback": ((1, 6, 37, 70), None, 4, 1, 40.0, (0.5, 2.5), torch.float32),   # every block's box exceeds LDS
    "lds_rpt2": ((4, 5, 512, 512), None, 4, 1, 3.0, (0.5, 2.5), torch.float32),      # 4 x 8 x 64 = 2048 tiles: two rows per thread
    "lds_small_sigma": ((1, 6, 37, 70), None, 4, 1, "small_sigma", None, torch.float32),
    "lds_sigma_zero": ((1, 6, 37, 70), None, 4, 1, "sigma_zero", None, torch.float32),
    "lds_sigma_tenth": ((1, 6, 37, 70), None, 4, 1, "sigma_tenth", None, torch.float32),
    "direct_dil2": ((1, 6, 37, 70), None, 4, 2, 3.0, (0.6, 2.5), torch.float32),
    "direct_f64": ((1, 6, 37, 70), None, 4, 1, 3.0, (0.5, 2.5), torch.float64),
    "direct_small_sigma": ((1, 6, 37, 70), None, 4, 2, "small_sigma", None, torch.float32),
    "direct_sigma_zero": ((1, 6, 37, 70), None, 4, 2, "sigma_zero", None, torch.float32),
    "direct_sigma_tenth": ((1, 6, 37, 70), None, 4, 2, "sigma_tenth", None, torch.float32),
    "direct_small_sigma_f64": ((1, 6, 37, 70), None, 4, 1, "small_sigma", None, torch.float64),
    "generic_ks8": ((1, 3, 14, 14), None, 8, 1, 3.0, (0.6, 2.5), torch.float32),
}
RS_SPECIAL = {"small_sigma": rs_small_sigma, "sigma_zero": rs_sigma_zero, "sigma_tenth": rs_sigma_tenth}


def rs_families(name):
    """The source families a resample2d case runs: the large route one, the special sigma inputs two or three, the rest all."""
    flow = RS_CASES[name][4]
    if name == "lds_rpt2":
        return ("feat_mags",)
    if flow == "sigma_tenth":
        return ("signed", "tiny")
    if isinstance(flow, str):
        return ("signed", "feat_mags")
    return SOURCE_FAMILIES


@functools.lru_cache(maxsize=None)
def rs_case(name, kind):
    shape, grid, ks, dil, reach, sigma, dtype = RS_CASES[name]
    B, C, Hi, Wi = shape
    H, W = grid or (Hi, Wi)
    in1 = source(kind, shape, 230)
    in2 = RS_SPECIAL[reach](B, H, W, 231) if isinstance(reach, str) else rs_flow(kind, B, Hi, H, W, 231, reach, sigma)
    return in1, in2, ks, dil, resample2d_bound(in1, in2, ks, dil, dtype)


def rs_irregular(in2):
    """A copy of `in2` with one flow pixel non-finite and one beyond 2^20: their blocks leave the LDS box for direct gathers, the
    other blocks of the call stay staged."""
    bad = in2.clone()
    bad[0, 0, 5, 7] = 3e6
    bad[0, 1, 20, 11] = NAN
    return bad


# ------------------------------------------------------------------------------------------------ the matrices
def _alternate(kinds, start=0):
    return [(k, (i + start) % 2 == 1) for i, k in enumerate(kinds)]


# (path, case, grid family, source family, flipcat).  path: `direct` forces warp_fwd_kernel (warp_fwd_variant = 1), `lds`
# warp_fwd_lds_kernel (2), `natural` leaves the route to the shape.  The small direct cases are planned down to ONE channel per
# block (the remainder loop alone); trip5 / trip7 / slabs keep the four-channel trip (warp_forward_slab, proven on the CPU).
WARP_ROWS = (
    [("direct", "c5_64", "border", k, f) for k, f in _alternate(SOURCE_FAMILIES)] +
    [("direct", "c5_64", g, "signed", f) for g, f in (("interior", True), ("outside", False))] +
    [("direct", "c7", "border", k, f) for k, f in _alternate(("signed", "feat_mags", "tiny", "nonfinite"), 1)] +
    [("direct", "small", "border", k, f) for k, f in _alternate(("signed", "nonfinite"))] +
    [("direct", "grids", "border", k, f) for k, f in _alternate(("signed", "feat_mags", "masked", "nonfinite"))] +
    [("direct", "grids", "outside", "signed", True)] +
    [("direct", "trip5", "border", "feat_mags", False), ("direct", "trip7", "border", "nonfinite", True),
     ("direct", "slabs", "border", "feat_mags", True)] +
    [("direct", n, "border", k, f) for n in ("small_f64", "c7_f64") for k, f in _alternate(("signed", "feat_mags", "nonfinite"))] +
    [("lds", "ragged_w", "border", k, f) for k, f in _alternate(SOURCE_FAMILIES, 1)] +
    [("lds", "ragged_w", "outside", k, f) for k, f in _alternate(("signed", "feat_mags", "nonfinite"))] +
    [("lds", "c2_66", g, k, f) for g in ("zoom18", "zoom25") for k, f in _alternate(("signed", "feat_mags", "nonfinite"))] +
    [("lds", "grids", "outside", k, f) for k in ("signed", "nonfinite") for f in (False, True)] +
    [("lds", "c5_64", "border", k, f) for k, f in _alternate(("nonfinite", "tiny"))] +
    [("natural", "natural", "border", "feat_mags", False)])

# warp_multi_forward: nine small problems -- the table flushes at kMaxWarpProblems = 8 and again for the ninth --, three of them on
# the LDS arm of multi_wants_lds, six on direct gathers; without flipcat `natural` joins them, which fwd_wants_lds sends out alone.
MULTI = (("m_lds32", "feat_mags"), ("small", "nonfinite"), ("m_lds40", "nonfinite"), ("c7", "feat_mags"), ("grids", "signed"),
         ("m_lds64", "tiny"), ("c5_64", "nonfinite"), ("ragged_w", "masked"), ("c2_66", "huge"))
MULTI_ALONE = ("natural", "feat_mags")
WARP_ROWS += [("multi", n, "border", k, f) for n, k in MULTI for f in (False, True)]

# path: (case, options, profiler scope).  be_fwd_variant: 1 = direct gathers, 9 = the per-element kernel.
BE_PATHS = {
    "lds_k1": ("k1", {}, "block_extractor_fwd_lds"), "lds_k2": ("k2", {}, "block_extractor_fwd_lds"),
    "lds_k3": ("k3", {}, "block_extractor_fwd_lds"), "lds_k4": ("k4", {}, "block_extractor_fwd_lds"),
    "lds_k3_f64": ("k3_f64", {}, "block_extractor_fwd_lds"), "lds_grids": ("grids", {}, "block_extractor_fwd_lds"),
    "lds_rows4": ("rows4", {}, "block_extractor_fwd_lds"), "lds_rows4_far": ("rows4_far", {}, "block_extractor_fwd_lds"),
    "direct_k1": ("k1", {"be_fwd_variant": 1}, "block_extractor_fwd"), "direct_k2": ("k2", {"be_fwd_variant": 1}, "block_extractor_fwd"),
    "direct_k3": ("k3", {"be_fwd_variant": 1}, "block_extractor_fwd"), "direct_k4": ("k4", {"be_fwd_variant": 1}, "block_extractor_fwd"),
    "direct_k5": ("k5", {}, "block_extractor_fwd"), "direct_k6": ("k6", {}, "block_extractor_fwd"),
    "direct_k7": ("k7", {}, "block_extractor_fwd"),
    "generic_k9": ("k9", {}, "block_extractor_fwd_generic"), "generic_k3": ("k3", {"be_fwd_variant": 9}, "block_extractor_fwd_generic"),
}
BE_SCOPES = ("block_extractor_fwd_lds", "block_extractor_fwd", "block_extractor_fwd_generic")


def be_families(path):
    return ("signed", "feat_mags", "nonfinite") if "rows4" in path else SOURCE_FAMILIES


BE_ROWS = [(path, kind) for path in BE_PATHS for kind in be_families(path)]

# (case, ba_fwd_pix, source family, weight family).  ba_fwd_pix 1 .. 4: ba_fwd_pix_kernel's configurations; 0: be_fwd_lds_kernel's
# attention mode (one row per thread below 64 rows, four from there).  Both run under the scope block_attention_fwd_lds: the
# option is what tells them apart.  k = 2 and float64 take ba_fwd_generic.
BA_ROWS = ([("c8", pix, k, k) for pix in range(5) for k in ("signed", "feat_mags")] +
           [("c8", 1, k, "signed") for k in ("ramp", "masked", "tiny", "huge", "nonfinite")] +
           [("c6", pix, k, w) for pix in range(1, 5) for k, w in (("nonfinite", "signed"), ("feat_mags", "feat_mags"))] +
           [("low", pix, k, w) for pix in (0, 1) for k, w in (("signed", "signed"), ("feat_mags", "feat_mags"), ("nonfinite", "signed"))] +
           [(n, 1, k, w) for n in ("k2", "c6_f64") for k, w in (("signed", "signed"), ("feat_mags", "feat_mags"), ("nonfinite", "signed"))])

RS_ROWS = [(name, kind) for name in RS_CASES for kind in rs_families(name)]
EXACT_WARP = ((2, 5, 64, 64), (1, 6, 128, 64))
EXACT_BE = ("k1", "k2", "k3", "k4", "k5", "k9", "grids", "rows4")
