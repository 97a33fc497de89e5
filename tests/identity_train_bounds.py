"""Yardsticks of the training half of --crop (ffwm_identity_input_backward in csrc/lightcnn_eval.hip, external_function.
IdentityInputFunction, losses.IdentityLoss, FFWMTrainer(crop=True)); a plain helper module, not a conftest.  SAFETY, U32 and
rho_any_order are those of tests/conv_bounds.py; the coordinates, COORD_ROUNDINGS and `crop_reference` those of tests/identity_bounds.py.

The crop is a fixed linear map, separable over the two axes of the plane:
    out = A_y gray A_x^T,   A = R S per axis (`axis_matrix`)
  S [98, 128]: row r is the two-tap grid_sample at source coordinate c_r = origin + 98 r / 97 (origin 27.5 for rows, 14.5 for columns):
    S[r, floor(c_r)] = 1 - frac(c_r), S[r, floor(c_r) + 1] = frac(c_r).  Every tap is inside the image (identity_bounds.crop_taps_inside).
  R [128, 98]: row o is the two-tap half-pixel resize at 0.765625 (o + 0.5) - 0.5, clamped at 0, the upper tap clamped at 97.
  All weights are >= 0 and every row of A sums to 1.
The adjoint (`crop_adjoint_reference`):  grad_gray = A_y^T g A_x,  grad_img[b, c] = grad_gray / Cin  for every channel c, in float64.

`crop_adjoint_bound`, per element of grad_img.  T = (A != 0) marks the outputs that touch an input index; N_y, N_x = the largest column
counts of T_y, T_x (4 and 4, counted from the matrices: an input index lies under at most two sample rows r, each of which serves
two or three outputs, some of them shared).  Two terms, as in identity_bounds.crop_bound:
  * the weighted sum.  A cell is the sum of at most n = N_y N_x products A_y[oy, Y] A_x[ox, X] g[oy, ox] (all weights >= 0), in any order
    and any grouping: a separable evaluation (N_y terms, then N_x) rounds fewer times than the flat sum the count allows.  Extra
    roundings on a term's path: an axis weight is a sum of at most three products l w of a resize weight and a sample weight (the
    differences that give l and w from the coordinates are exact): 3 per axis; the product with g in either pass: 2; the division by
    Cin: 1.  EXTRA = 3 + 3 + 2 + 1 = 9.
        magnitude = rho_any_order(n, EXTRA) (A_y^T |g| A_x) / Cin
  * coordinates.  The resize coordinate is exact in fp32; a source coordinate formed in fp32 is off by at most COORD_ROUNDINGS 128 u
    (identity_bounds: ATen's linspace / normalise / un-normalise chain; one rounding of a double for the kernel).  A shift d of c_r
    moves the two weights of row r of S by d each (one up, one down), so A[o, i] moves by at most d sum_r R[o, r] <= d for every
    output o that touches i and not at all for the others -- as long as no c_r crosses an integer, which would move a tap to a
    neighbouring cell: the c_r keep a distance of at least 1 / 194 from every integer (98 r / 97 + 1 / 2 is never an integer: 196 r =
    97 (2 k - 1) has no solution, the left side being even), 6e4 times the shift.  With the other axis' weights at most 1:
        coord = 2 axes x COORD_ROUNDINGS 128 u (T_y^T |g| T_x) / Cin         (the sum of |g| over the outputs that touch the cell)
  |got - ref| <= SAFETY coord + magnitude.
  Where no output touches a cell -- rows 0 .. 26 and 127, columns 0 .. 13 and 114 .. 127 -- both terms are 0: the kernel owes an exact 0.
  The CPU test shows that ATen's own fp32 autograd of the composition meets the bound on random and one-hot g, and that the adjoints
  of the two wrong variants of `crop_reference` (row centre 64, align_corners=True) miss it by a wide factor.

The sum rule.  Every row of A sums to 1, whatever the coordinates (the two weights of a sample are 1 - f and f), so
  sum(grad_img) = sum(g) up to the magnitude term summed over the cells: `sum_rule_tolerance`.

The stand-in identity network (`StandIn`): a seeded linear map from the [B, 1, 128, 128] input to (None, fc [B, 16], pool [B, 8]) -- 8 x 8
  average pooling, then a [24, 256] matrix -- used where the test is about the input stage and the loss around it; LightCNN-29 as
  tests/golden/fill.py fills it turns an ulp of its input into percent of its feature (tests/identity_bounds.py).  Two short sums
  (64 and 256 terms) keep the worst-case rounding of the features themselves small.  `loss_tolerance` pushes the input stage's
  per-element bound e (identity_bounds.crop_bound / gray_bound) through the loss:
      pooled cell:  mean of e over the cell + rho_any_order(64) mean |input|
      feature:      |W| (that) + rho_any_order(256) |W| pooled |input|                         (`_feature_deviation`)
      loss:         mean over the features of (deviation of f(out) + deviation of f(gt)) per L1 term + rho_any_order(16 B, 2) loss
  The reference forms its grid in float32 and casts it (`type_as`), so its float64 run -- the fixture -- carries the float32 grid's
  coordinate error, which e covers: a float32 evaluation and the fixture both lie within the tolerance of the exact map, and within
  twice the tolerance of each other.
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import identity_bounds as ib  # noqa: E402
from conv_bounds import SAFETY, U32, rho_any_order  # noqa: E402,F401

EXTRA = 9
FACE, PLANE = ib.FACE, ib.PLANE


def axis_matrix(coords, align_corners=False):
    """A = R S [128, 128] (float64) of one axis from its 98 source coordinates."""
    S = torch.zeros(PLANE, FACE, dtype=torch.float64)
    i0 = coords.floor().long()
    f = coords - i0.double()
    r = torch.arange(PLANE)
    S[r, i0] += 1.0 - f
    S[r, i0 + 1] += f
    rc = ib._resize_coordinates(align_corners)
    R = torch.zeros(FACE, PLANE, dtype=torch.float64)
    j0 = rc.floor().long().clamp(max=PLANE - 1)
    j1 = (j0 + 1).clamp(max=PLANE - 1)
    w1 = rc - j0.double()
    o = torch.arange(FACE)
    R[o, j0] += 1.0 - w1
    R.index_put_((o, j1), w1, accumulate=True)
    return R @ S


def crop_matrices(row_origin=ib.ROW_ORIGIN, align_corners=False):
    """-> (A_y, A_x); row_origin / align_corners: the wrong variants of identity_bounds.crop_reference."""
    ys, xs = ib.crop_coordinates()
    return axis_matrix(ys - ib.ROW_ORIGIN + row_origin, align_corners), axis_matrix(xs, align_corners)


A_Y, A_X = crop_matrices()
T_Y, T_X = (A_Y != 0).double(), (A_X != 0).double()
N_Y, N_X = int(T_Y.sum(0).max()), int(T_X.sum(0).max())
N_TOUCH = N_Y * N_X
ROWS_INSIDE = (T_Y.sum(0) > 0)          # input rows some output touches: 27 .. 126
COLS_INSIDE = (T_X.sum(0) > 0)          # input columns: 14 .. 113


def _sandwich(g, my, mx):
    """my^T g mx on the last two axes of g [B, 1, 128, 128] (float64)."""
    return torch.einsum("oy,bcop,px->bcyx", my, g, mx)


def crop_adjoint_reference(g, cin, matrices=None):
    """-> float64 [B, cin, 128, 128]: A_y^T g A_x / cin in every channel."""
    ay, ax = matrices if matrices is not None else (A_Y, A_X)
    gg = g.detach().cpu().double()
    return (_sandwich(gg, ay, ax) / cin).expand(-1, cin, -1, -1).contiguous()


def magnitude_term(g, cin):
    return rho_any_order(N_TOUCH, EXTRA) * (_sandwich(g.detach().cpu().double().abs(), A_Y, A_X) / cin).expand(-1, cin, -1, -1)


def crop_adjoint_bound(g, cin):
    """-> (float64 reference [B, cin, 128, 128], per-element bound); see the module docstring."""
    ga = g.detach().cpu().double().abs()
    coord = 2.0 * ib.COORD_ROUNDINGS * 128.0 * U32 * (_sandwich(ga, T_Y, T_X) / cin).expand(-1, cin, -1, -1)
    return crop_adjoint_reference(g, cin), SAFETY * coord + magnitude_term(g, cin)


def sum_rule_tolerance(g, cin):
    return float(magnitude_term(g, cin).sum())


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; a cell whose bound is 0 must be exactly right (0 / 0 counts as 0, anything / 0 as inf)."""
    err = (got.detach().cpu().double() - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max())


# ---- the g families of the CPU and GPU tests
ONE_HOT = {"corner00": (0, 0), "corner0w": (0, 127), "cornerh0": (127, 0), "cornerhw": (127, 127), "centre": (64, 64),
           "clamped": (0, 127)}          # "clamped": row 0's resize coordinate clamps at 0, column 127's upper tap at 97


def one_hot(name, B=1):
    g = torch.zeros(B, 1, FACE, FACE)
    oy, ox = ONE_HOT[name]
    g[B - 1, 0, oy, ox] = 1.0
    return g


def random_g(B, seed=7):
    return torch.randn(B, 1, FACE, FACE, generator=torch.Generator().manual_seed(seed))


# ---- the stand-in identity network
POOL = 8


class StandIn(torch.nn.Module):
    """(None, fc [B, 16], pool [B, 8]) = a fixed seeded linear map of the [B, 1, 128, 128] input: 8 x 8 average pooling, then a
    [24, 256] matrix; defined identically in tests/golden/make_identity_loss_golden.py, which feeds it to the reference's IdentityLoss.
    The seed is one at which every feature difference of `loss_inputs` is at least ten times its fp32 error away from zero
    (`signs_are_safe`, asserted by the CPU test), so that the gradient does not hang on the sign of a rounding error."""

    def __init__(self, dtype=torch.float64, device="cpu"):
        super().__init__()
        gen = torch.Generator().manual_seed(29)
        w = (torch.rand(24, 256, generator=gen, dtype=torch.float64) * 2.0 - 1.0) / 16.0
        self.register_buffer("w", w.to(dtype=dtype, device=device))

    def forward(self, x):
        f = (F.avg_pool2d(x, POOL).reshape(x.shape[0], 1, -1) * self.w.unsqueeze(0)).sum(-1)          # (products and a plain sum: no BLAS call)
        return None, f[:, :16], f[:, 16:]


def loss_fixture():
    """tests/golden/reference_identity_loss.pt: the reference's IdentityLoss around StandIn on `loss_inputs` -- loss_plain / loss_crop,
    grad_plain / grad_crop [2, 1, 128, 128] (d loss / d out, the same plane in each of the three channels) and grad_spread_* (the
    largest difference between the channels in the reference's own run)."""
    return torch.load(os.path.join(ib.golden_dir(), "reference_identity_loss.pt"))


def loss_inputs():
    """-> (out, gt) float64 [2, 3, 128, 128] holding float32 values: two seeded images (tests/golden/fill.py) under opposite diagonal
    brightness ramps, so that their pooled planes -- and with them the stand-in's features -- differ by far more than fp32 rounding."""
    fill = ib.fill_module()
    ramp = torch.linspace(0, 1, FACE).view(1, 1, FACE, 1) * torch.linspace(0, 1, FACE).view(1, 1, 1, FACE)
    out = fill.image(2, 3, FACE, FACE, "idloss_out") * (0.25 + 0.75 * ramp)
    gt = fill.image(2, 3, FACE, FACE, "idloss_gt") * (1.0 - 0.75 * ramp)
    return out.double(), gt.double()


def reference_loss(out, gt, crop):
    """float64 restatement of IdentityLoss(StandIn, crop) from the matrices: -> loss (float64 scalar tensor; differentiable in out)."""
    net = StandIn()

    def feat(x):
        gray = x.double().mean(1, keepdim=True)
        if crop:
            gray = torch.einsum("oy,bcyx,px->bcop", A_Y, gray, A_X)
        return net(gray)
    _, fo, po = feat(out)
    with torch.no_grad():
        _, fg, pg = feat(gt)
    return (fo - fg).abs().mean() + (po - pg).abs().mean()


def _feature_deviation(x, crop):
    """-> (float64 features [B, 24] of the exact input stage, how far an fp32 evaluation of them can be off [B, 24])."""
    w = StandIn().w
    x = x.detach().cpu().float()
    ref, e = ib.crop_bound(x) if crop else ib.gray_bound(x)
    B = ref.shape[0]
    pooled, pooled_abs = F.avg_pool2d(ref, POOL).reshape(B, -1), F.avg_pool2d(ref.abs(), POOL).reshape(B, -1)
    e_pool = F.avg_pool2d(e, POOL).reshape(B, -1) + rho_any_order(POOL * POOL) * pooled_abs
    return pooled @ w.t(), e_pool @ w.abs().t() + rho_any_order(256) * (pooled_abs @ w.abs().t())


def loss_tolerance(out, gt, crop):
    """The input stage's per-element bound pushed through the stand-in and the two L1 means (module docstring) -> float."""
    (_, d_out), (_, d_gt) = _feature_deviation(out, crop), _feature_deviation(gt, crop)
    dev = d_out + d_gt                                          # [B, 24]: how far f(out) - f(gt) can be off
    loss = float(reference_loss(out, gt, crop))
    return float(dev[:, :16].mean() + dev[:, 16:].mean()) + rho_any_order(16 * out.shape[0], 2) * abs(loss)


def signs_are_safe(out, gt, crop):
    """No feature difference of the exact evaluation is within the fp32 path's error of zero: both take the same branch of every |.|."""
    (f_out, d_out), (f_gt, d_gt) = _feature_deviation(out, crop), _feature_deviation(gt, crop)
    return bool(((f_out - f_gt).abs() > d_out + d_gt).all())


def grad_tolerance(out, crop):
    """d loss / d out when `signs_are_safe`: the sign pattern s of the feature differences is then the exact evaluation's, and the
    gradient is the input stage's adjoint applied to the FIXED g = unpool(sum_j s_j W[j] / (B F_j)) / 64 -- a 24-term fp32 sum, one
    division by 64 (exact) and the scale 1 / (B F_j) (one rounding, one more for the product): |g| <= g_abs, its own error
    rho_any_order(24, 2) g_abs.  -> per-element bound [B, Cin, 128, 128]: the adjoint's bound at g_abs plus the adjoint of g's error."""
    B, cin = out.shape[0], out.shape[1]
    w = StandIn().w.abs()
    cell = (w[:16].sum(0) / (16 * B) + w[16:].sum(0) / (8 * B)).view(1, 1, FACE // POOL, FACE // POOL) / (POOL * POOL)
    g_abs = F.interpolate(cell, scale_factor=POOL, mode="nearest").expand(B, -1, -1, -1)
    g_err = rho_any_order(24, 2) * g_abs
    if crop:
        _, bound = crop_adjoint_bound(g_abs, cin)
        return bound + (_sandwich(g_err, A_Y, A_X) / cin).expand(-1, cin, -1, -1)
    return ((SAFETY * U32 * g_abs + g_err) / cin).expand(-1, cin, -1, -1)
