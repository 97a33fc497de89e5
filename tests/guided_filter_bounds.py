"""Per-element float64 error bounds, exact windows and fp32 stand-ins for the guided-filter kernels of csrc/guided_filter.hip (a plain
helper module, not a conftest): ffwm_guided_filter_forward / _backward (the four-launch "fast" kernels, gf_*) and
ffwm_guided_filter_forward_general / _backward_general (the sliding-window "general" kernels, gfg_*).

Conventions are the project's: every reference is float64 torch on the CPU, computed from the kernel's ACTUAL inputs; u = 2^-24,
u64 = 2^-53; one SAFETY = 4 multiplies every count of roundings; FLOOR = 1e-38 keeps a bound of exactly zero from dividing; no
constant here is fitted.  Tensors are handled plane-flat: x [Px, H, W], y / grad_output [Py, H, W], Py = Px cdiv; y plane p is guided
by x plane p // cdiv.

The route (route / col_rows, RESTATED from gfg_fast / gfg_col_rows of the .hip file -- the values are not observable from outside
the library, so the cases are chosen BY these functions and the GPU test checks the launch names)
  fast     Px == Py, H <= 128, W <= 128 and no grad_y: a wave of WAVE = 64 lanes holds a line as FAST_PER_LANE = 2 elements per lane.
  general  everything else: the column pass walks chunks of rc = col_rows(Py, H, W) rows (128, halved down to 32 while the two-quantity
           launch 2 Py ceil(W / 64) ceil(H / rc) has fewer than 2048 waves); the row pass chunks of ROW_CHUNK = 256 outputs in
           ROW_SEGS = 4 segments of 64.

Box-sum primitives.  A box is a pass down the columns and a pass along the rows of the column sums.  Every pass bounds the error of
one line's window sum by  count u M  with a count of roundings and a magnitude M that both follow the algorithm (any rounding errs
by u times the magnitude of its result, and an error once made is carried on unamplified: every later operation is an addition):
  fast (line_box): inclusive cumsum by the pair add b += a (1), six shuffle levels (6), excl = incl - b (1), ca / cb = a + excl (1)
    = 9 roundings in each of cumsum[hi] and cumsum[lo - 1], each on a value of magnitude <= P(hi), the prefix sum of |v| up to the
    window's upper end hi -- the prefix, not the window, because the algorithm is a cumsum difference -- and the difference itself
    (1):  C_FAST = 19,  M = P(hi).
  general columns (gfg_cols_kernel): the seed adds seed_len <= 2r + 1 values one after the other (the window of the row above the
    chunk; r values for the first chunk); step t = 1, 2, ... of the chunk computes fl(add - sub), of magnitude <= |add| + |sub| <=
    W_abs(t) + W_abs(t - 1), and accumulates it into a sum of magnitude <= W_abs(t):  count = seed_len + 3 t,  M = max over s in
    [0, t] of W_abs(s), the window sum of |v|; s = 0 is the seed's window, and the maximum restarts with every chunk.  (Two
    roundings per step as the code reads, the first on a magnitude of up to 2 M: hence 3 and not 2.)  Outside the support of a
    locally supported input M is zero from the first chunk that does not see the support: the drift of a running sum that is
    never reseeded is what this term does not allow.
  general rows (gfg_row_boxes): the seed is a lane-strided partial sum of ceil(seed_len / 64) terms and six levels of the wave
    reduction; a segment computes fl(add - sub) per lane -- the errors of the lanes up to k add up to u sum (|add| + |sub|), and the
    adds (the subs) of a segment are 64 consecutive values, covered by ceil(64 / (2r + 1)) windows centred in the chunk, 2 ceil(64 /
    (2r + 1)) M in all --, scans them in six levels whose every intermediate is a difference of two window sums, <= 2 M (12), and adds
    the carry (1):  count = ceil(seed_len / 64) + 6 + (13 + 2 ceil(64 / (2r + 1))) (segment + 1),  M as for the columns, over the
    row chunk.
  The row pass works on the column sums, whose magnitude is bounded by the column box of |v| plus the column pass's own bound; the
  error of the column pass and the error `din` that the pointwise input brings along (a rounded product or quotient: x y, x x, g / N,
  g x / N add their roundings times |v|) go through the exact box.  The float64 reference sums a window directly (pad, unfold, sum):
  2r + 1 terms per pass in whatever order, so it is itself within 2 (2r + 1) u64 box|v|, which every bound includes unscaled.

Forward.  First-order error bounds (not magnitudes) are propagated through the stages, d q = the bound of q:
    mean = S / N:                      d mean = d S / N + u |mean|
    cov = E[xy] - mx my:               d cov = d E[xy] + |my| d mx + |mx| d my + u |mx my| + u |cov|
    ve = (E[xx] - mx^2) + eps:         d ve = d E[xx] + 2 |mx| d mx + u mx^2 + u |var| + u |ve|
    A = cov / ve:                      d A = d cov / ve + |A| d ve / ve + u |A|
    b = my - A mx:                     d b = d my + |mx| d A + |A| d mx + u |A mx| + u |b|
    mean_A, mean_b: the box primitive with din = d A, d b, then / N as above
    out = mean_A x + mean_b:           d out = |x| d mean_A + d mean_b + u |mean_A x| + u |out|
  The bounds of cov and ve are sums over the cancelling terms, so the conditioning is carried.  First order is valid only while
  d ve << ve: that is a CONDITION, d ve (at SAFETY = 4) <= ve / 8 on every element, computed from the float64 reference alone
  (ValueError otherwise).  eps enters as the kernel holds it: float32(eps) for the float kernels.

Backward.  The reference is a function of what the kernel is GIVEN -- x, y, g and the kernel's own `saved` planes, all converted
to float64 -- in closed form (box = the clipped box sum):
    q1 = box(g x / N), q2 = box(g / N);  gA = q1 - q2 mx, gcov = gA / ve, gvar = -gA A / ve
    gmx = -q2 A - gcov my - 2 gvar mx,  gmy = q2 - gcov mx
    grad_x = box(gmx / N) + g mean_A + y box(gcov / N) + 2 x box(gvar / N),  grad_y = x box(gcov / N) + box(gmy / N)
  (one-channel guide: gmx, gvar and the pointwise terms of grad_x summed over the cdiv channels, channel 0 first).  The bound is the
  same propagation, two box stages with the quotient-rule terms between them; every sum of products carries the sum of the
  magnitudes of its terms, and the count of roundings on its longest path: gA 2, gcov 1, gvar 2, gmx 3 (+ cdiv - 1 for the sum over
  the channels, as gvar), gmy 2, the quotients by N 1 each, grad_x 2 + 2 cdiv, grad_y 2.
  tests/test_guided_filter_bounds_cpu.py ties the closed form to autograd of ffwm_amd.nets.GuidedFilter.

Float64 instantiation: the same formulas with u64 on the `double` kernels; a structural error exceeds them by many orders.

Exact windows.  Integer inputs make every box sum of x, y, x y, x x exact in float32 on both routes (the fast path takes differences
of cumsums of integers, the general path adds and subtracts integers) as long as every sum the algorithm forms stays below 2^24:
require_exact computes the largest box sum of the four quantities -- and for the fast route the largest whole-line sum of column
sums, the cumsum's last value -- in float64 and raises otherwise.  Then mean_x, mean_y == float32(S) / float32(N) bit for bit.

Input families (amplitudes found on the CPU against the ve condition, on every case of CASES):
  uniform   i.i.d. [0, 1), as the existing tests.
  planes    uniform, x plane p scaled by 2^(p % 7 - 3), y by 2^((3 p + 1) % 5 - 2), grad_output by 2^((5 p + 2) % 9 - 4).
  image     0.5 + 0.3 sin(low-frequency phase, different per plane) + IMAGE_NOISE (uniform - 0.5), IMAGE_NOISE = 0.25; y = 0.8 x +
            0.1 + 0.05 (uniform - 0.5): A near 0.8.  The noise gives a window of a smooth plane its variance: with 0.125 the ve
            condition stands at 1.85 on the rc = 128 case (it fails), with 0.25 at 0.55.
  offset    x = OFFSET_C + (uniform - 0.5), OFFSET_C = 3.5: the cancellation of E[xx] - mean_x^2 at the largest multiple of 1/2 for
            which the ve condition holds on every case: it stands at 0.86 on the rc = 128 case (column chunks of 128 steps have the
            largest count), and at 1.12 -- a failure -- with OFFSET_C = 4.
  integers  x, y in 0 .. hi - (p % 4) with hi = 15 (7 for the r = 140 case), a different range per plane.

The fp32 stand-ins of tests/test_guided_filter_bounds_cpu.py (emulate_forward / emulate_backward below: the kernels' order of
operations restated in torch, with the sliding-window and the cumsum-difference box) meet every bound with SAFETY = 1 and the
integer family exactly; the mutants of the same restatement each miss an assertion.

GPU ratios (MI355X, SAFETY = 4, worst error / bound over all cases and families): forward 0.049 on the fast route (mean_x), 0.017 /
0.025 / 0.027 on the general route with rc = 32 / 64 / 128; backward 0.0023 (fast) and 0.0036-0.0040 (general, grad_y); the float64
kernels 0.031 forward and 0.0040 backward at most.  GPU_RATIOS of tests/test_gpu_guided_filter_bounds.py has the table.  The counts
are worst cases of chains of up to 400 roundings whose errors largely cancel, hence the distance; the emulation with a
window off by one element misses the same bounds by a factor above 10^4 on the mean planes, with a seed one element short by 500 or
more on every plane.
"""
import functools
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 4.0
FLOOR = 1e-38
WAVE = 64
FAST_PER_LANE = 2
FAST_MAX = WAVE * FAST_PER_LANE          # kGfMaxDim
ROW_SEGS = 4
ROW_CHUNK = ROW_SEGS * WAVE              # kGfgRowChunk
C_FAST = 19
VE_CONDITION = 8.0
IMAGE_NOISE = 0.25
OFFSET_C = 3.5
EPS = 1e-8
FAMILIES = ("uniform", "planes", "image", "offset")


def _ceil_div(a, b):
    return -(-a // b)


def unit(dtype):
    return U32 if dtype == torch.float32 else U64


# ------------------------------------------------------------------------------------------------ the route (a restatement)
def route(Px, Py, H, W, want_y):
    """gfg_fast of csrc/guided_filter.hip, restated: "fast" (the four-launch kernels) or "general"."""
    return "fast" if (Px == Py and H <= FAST_MAX and W <= FAST_MAX and not want_y) else "general"


def col_rows(Py, H, W):
    """gfg_col_rows of csrc/guided_filter.hip, restated: rows per work unit of the general column pass."""
    rc = 128
    while rc > 32 and 2 * Py * _ceil_div(W, WAVE) * _ceil_div(H, rc) < 2048:
        rc //= 2
    return rc


class Plan:
    """How one direction of one call computes its boxes."""

    def __init__(self, kind, r, rc=None):
        self.kind, self.r, self.rc = kind, r, rc

    def __repr__(self):
        return self.kind if self.kind == "fast" else "general/rc=%d" % self.rc


# (B, Cx, Cy, H, W, r, want_y) -> forward route, backward route, rc
CASES = {
    "fast_minimal": ((1, 1, 1, 9, 12, 3, False), "fast", "fast", 32),
    "fast_ragged": ((1, 2, 2, 37, 61, 5, False), "fast", "fast", 32),
    "fast_odd_strip": ((1, 2, 2, 127, 33, 7, False), "fast", "fast", 32),
    "fast_full_line": ((1, 1, 1, 128, 128, 32, False), "fast", "fast", 32),
    "general_grad_y_on_fast": ((1, 2, 2, 64, 48, 8, True), "fast", "general", 32),
    "general_many_chunks": ((1, 2, 2, 200, 136, 66, True), "general", "general", 32),
    "general_long_window": ((1, 1, 1, 290, 300, 140, True), "general", "general", 32),
    "general_rc64_guide1": ((24, 1, 8, 130, 65, 5, True), "general", "general", 64),
    "general_rc64": ((24, 8, 8, 130, 65, 5, True), "general", "general", 64),
    "general_rc128_guide1": ((32, 1, 8, 130, 65, 5, True), "general", "general", 128),
    "general_rc128": ((32, 8, 8, 130, 65, 5, True), "general", "general", 128),
    "guide1_long_lines": ((2, 1, 3, 40, 260, 4, True), "general", "general", 32),
}


def plans(case):
    """-> (forward Plan, backward Plan) of a case tuple."""
    B, Cx, Cy, H, W, r, want_y = case
    rc = col_rows(B * Cy, H, W)
    return (Plan(route(B * Cx, B * Cy, H, W, False), r, rc), Plan(route(B * Cx, B * Cy, H, W, want_y), r, rc))


def integer_hi(case):
    return 7 if case[5] >= 100 else 15


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(case, family):
    """-> x [B, Cx, H, W], y, grad_output [B, Cy, H, W]: float32 CPU tensors (the float64 kernels get the same values)."""
    B, Cx, Cy, H, W, r, _ = case
    gen = torch.Generator().manual_seed(977 + 13 * H + 7 * W + 3 * r + Cx + 5 * B + 101 * (FAMILIES + ("integers",)).index(family))
    Px, Py = B * Cx, B * Cy
    px, py = torch.arange(Px), torch.arange(Py)
    x = torch.rand(Px, H, W, generator=gen, dtype=torch.float64)
    y = torch.rand(Py, H, W, generator=gen, dtype=torch.float64)
    g = torch.rand(Py, H, W, generator=gen, dtype=torch.float64)

    def per(t, e):
        return t * torch.exp2(e.double()).view(-1, 1, 1)
    if family == "planes":
        x, y, g = per(x, px % 7 - 3), per(y, (3 * py + 1) % 5 - 2), per(g, (5 * py + 2) % 9 - 4)
    elif family == "image":
        i = torch.arange(H, dtype=torch.float64).view(1, H, 1) / H
        j = torch.arange(W, dtype=torch.float64).view(1, 1, W) / W
        fi, fj, ph = (1 + px % 3).view(-1, 1, 1), (1 + (px // 3) % 3).view(-1, 1, 1), (0.7 * px).view(-1, 1, 1)
        x = 0.5 + 0.3 * torch.sin(2 * math.pi * (fi * i + fj * j) + ph) + IMAGE_NOISE * (x - 0.5)
        y = 0.8 * x.repeat_interleave(Cy // Cx, 0) + 0.1 + 0.05 * (y - 0.5)
        g = per(g - 0.5, (5 * py + 2) % 9 - 4)
    elif family == "offset":
        x = OFFSET_C + (x - 0.5)
        g = g - 0.5
    elif family == "integers":
        hi = integer_hi(case)
        x = torch.floor(x * (hi + 1 - px % 4).view(-1, 1, 1).double())
        y = torch.floor(y * (hi + 1 - (py + 1) % 4).view(-1, 1, 1).double())
        g = torch.floor(g * 5) - 2
    return x.float().view(B, Cx, H, W), y.float().view(B, Cy, H, W), g.float().view(B, Cy, H, W)


# ------------------------------------------------------------------------------------------------ boxes in float64
def _along(t, dim, fn):
    """fn on the lines of `dim` ([..., L] -> [..., L])."""
    if dim == t.dim() - 1:
        return fn(t)
    return fn(t.transpose(dim, -1)).transpose(dim, -1)


def _win_direct(v, r):
    """Window sums of the lines [..., L], every window summed on its own (the reference: no cumsum)."""
    return F.pad(v, (r, r)).unfold(-1, 2 * r + 1, 1).sum(-1)


def _win_cumsum(a, r, ext=False):
    """Window sums of non-negative magnitudes by a cumsum difference; ext: L + 1 positions, the first the window of position -1."""
    L = a.size(-1)
    c = F.pad(a.cumsum(-1), (1, 0))
    p = torch.arange(-1 if ext else 0, L)
    return c.index_select(-1, (p + r).clamp(max=L - 1) + 1) - c.index_select(-1, (p - r).clamp(min=0))


def box64(v, r):
    """The clipped box sum of [P, H, W] planes, columns then rows, in the tensor's own dtype (float64 for a reference)."""
    return _along(_along(v, 1, lambda t: _win_direct(t, r)), 2, lambda t: _win_direct(t, r))


def _abox(a, r):
    return _along(_along(a, 1, lambda t: _win_cumsum(t, r)), 2, lambda t: _win_cumsum(t, r))


def box_count(H, W, r, dtype=torch.float64, clipped=True):
    """N = box(1) in closed form, [1, H, W]."""
    if not clipped:
        return torch.full((1, H, W), float((2 * r + 1) ** 2), dtype=dtype)
    i, j = torch.arange(H), torch.arange(W)
    h = (i + r).clamp(max=H - 1) - (i - r).clamp(min=0) + 1
    w = (j + r).clamp(max=W - 1) - (j - r).clamp(min=0) + 1
    return (h.view(H, 1) * w.view(1, W)).to(dtype).view(1, H, W)


# ------------------------------------------------------------------------------------------------ the box primitives' bounds
def _line_term(a, r, kind, chunk):
    """count x M of one pass along the lines [..., L] of magnitudes a (module docstring); kind: fast / cols / rows."""
    L = a.size(-1)
    k = torch.arange(L)
    if kind == "fast":
        return C_FAST * a.cumsum(-1).index_select(-1, (k + r).clamp(max=L - 1))
    wext = _win_cumsum(a, r, ext=True)                     # positions -1 .. L - 1
    out = torch.empty_like(a)
    per_seg = 13 + 2 * _ceil_div(WAVE, 2 * r + 1)
    for s in range(0, L, chunk):
        e = min(s + chunk, L)
        m = wext[..., s:e + 1].cummax(-1).values[..., 1:]
        seed_len = min(s - 1 + r, L - 1) - max(s - 1 - r, 0) + 1
        t = torch.arange(1, e - s + 1, dtype=a.dtype)
        if kind == "cols":
            count = seed_len + 3 * t
        else:
            count = _ceil_div(seed_len, WAVE) + 6 + per_seg * (torch.div(t - 1, WAVE, rounding_mode="floor") + 1)
        out[..., s:e] = count * m
    return out


def box_err(plan, absv, din, U):
    """Bound of |the kernel's box - the exact box| for an input of magnitude absv that arrives with the error din; U = SAFETY u."""
    r = plan.r
    fast = plan.kind == "fast"
    col = _along(absv, 1, lambda a: _line_term(a, r, "fast" if fast else "cols", plan.rc))
    colabs = _along(absv, 1, lambda a: _win_cumsum(a, r))
    row = _along(colabs + U * col, 2, lambda a: _line_term(a, r, "fast" if fast else "rows", ROW_CHUNK))
    inner = U * col + (_along(din, 1, lambda a: _win_cumsum(a, r)) if torch.is_tensor(din) else 0.0)
    return (_along(inner, 2, lambda a: _win_cumsum(a, r)) + U * row
            + 2 * (2 * r + 1) * U64 * _along(colabs, 2, lambda a: _win_cumsum(a, r)))


# ------------------------------------------------------------------------------------------------ the formulas, any dtype, any box
MUTANTS = ("hi_off_by_one", "seed_short", "unclipped_n", "eps_dropped", "guide_plane_mod", "gvar_sign", "no_reseed")


def _expander(Px, cdiv, mutant=None):
    if cdiv == 1:
        return lambda t: t
    if mutant == "guide_plane_mod":
        idx = torch.arange(Px * cdiv) % Px
        return lambda t: t.index_select(0, idx)
    return lambda t: t.repeat_interleave(cdiv, 0)


def forward_formulas(box, x, y, r, eps, mutant=None):
    """x [Px, H, W], y [Py, H, W] -> dict of mean_x, mean_y, A, ve, mean_A, out (+ b) in the tensors' dtype; box(v) = the box sum."""
    Px, H, W = x.shape
    cdiv = y.size(0) // Px
    ex = _expander(Px, cdiv, mutant)
    n = box_count(H, W, r, x.dtype, clipped=mutant != "unclipped_n")
    mx = box(x) / n
    var = box(x * x) / n - mx * mx
    ve = var if mutant == "eps_dropped" else var + torch.tensor(eps, dtype=x.dtype)
    xe, mxe = ex(x), ex(mx)
    my = box(y) / n
    A = (box(xe * y) / n - mxe * my) / ex(ve)
    b = my - A * mxe
    mA = box(A) / n
    out = mA * xe + box(b) / n
    return {"mean_x": mx, "mean_y": my, "A": A, "ve": ve, "mean_A": mA, "out": out, "b": b}


def backward_formulas(box, x, y, g, saved, r, mutant=None):
    """-> dict of grad_x [Px, H, W], grad_y [Py, H, W]; saved: dict of mean_x, mean_y, A, ve, mean_A in the same dtype."""
    Px, H, W = x.shape
    Py = y.size(0)
    cdiv = Py // Px
    ex = _expander(Px, cdiv, mutant)
    n = box_count(H, W, r, x.dtype, clipped=mutant != "unclipped_n")
    xe, mx, ve = ex(x), ex(saved["mean_x"]), ex(saved["ve"])
    my, A, mA = saved["mean_y"], saved["A"], saved["mean_A"]
    q1, q2 = box(g * xe / n), box(g / n)
    gA = q1 - q2 * mx
    gcov = gA / ve
    gvar = -gA * A / ve
    if mutant == "gvar_sign":
        gvar = -gvar
    gmx = -q2 * A + (-gcov * my - 2 * gvar * mx)
    gmy = q2 - gcov * mx

    def over_channels(t):                                  # channel 0 first
        t = t.view(Px, cdiv, H, W)
        acc = t[:, 0]
        for c in range(1, cdiv):
            acc = acc + t[:, c]
        return acc
    r1, r2, r3, r4 = box(over_channels(gmx) / n), box(gcov / n), box(over_channels(gvar) / n), box(gmy / n)
    gx = r1 + 2 * x * r3
    pw = (g * mA + y * r2).view(Px, cdiv, H, W)
    for c in range(cdiv):
        gx = gx + pw[:, c]
    return {"grad_x": gx, "grad_y": xe * r2 + r4}


# ------------------------------------------------------------------------------------------------ exact windows
def require_exact(x, y, r, fast):
    """Every sum the kernels form of the integer planes x [Px, H, W], y [Py, H, W] stays below 2^24, or ValueError.  -> the box sums
    of x and of y in float64."""
    x, y = x.double(), y.double()
    for t, w in ((x, "x"), (y, "y")):
        if not torch.equal(t, t.round()):
            raise ValueError("require_exact: %s is not integer-valued" % w)
    xe = x.repeat_interleave(y.size(0) // x.size(0), 0)
    worst = 0.0
    for q, w in ((x, "x"), (y, "y"), (xe * y, "x y"), (x * x, "x x")):
        a = q.abs()
        top = float(_abox(a, r).max())
        if fast:                                           # the cumsum's last value: a whole line of column sums
            top = max(top, float(_along(a, 1, lambda t: _win_cumsum(t, r)).sum(2).max()), float(a.sum(1).max()))
        if top >= 2.0 ** 24:
            raise ValueError("require_exact: a sum of %s reaches %.0f >= 2^24" % (w, top))
        worst = max(worst, top)
    return box64(x, r), box64(y, r)


def exact_means(x, y, r, fast):
    """-> mean_x, mean_y as float32(S) / float32(N), float32 tensors."""
    sx, sy = require_exact(x, y, r, fast)
    n = box_count(x.size(1), x.size(2), r, torch.float32)
    return sx.float() / n, sy.float() / n


# ------------------------------------------------------------------------------------------------ the bounds
def worst_ratio(got, ref, bound):
    """max |got - ref| / (bound + FLOOR); inf where got is not finite."""
    got = got.detach().to("cpu", torch.float64).reshape(ref.shape)
    q = (got - ref).abs() / (bound + FLOOR)
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, math.inf))
    return float(q.max())


class ForwardBound:
    """ref[name], bound[name] for mean_x, mean_y, A, ve, mean_A, out; x, y float32 or float64 [Px, H, W] / [Py, H, W]."""
    NAMES = ("mean_x", "mean_y", "A", "ve", "mean_A", "out")

    def __init__(self, plan, x, y, eps=EPS, safety=SAFETY):
        u0 = unit(x.dtype)
        U = safety * u0
        r = plan.r
        eps_k = float(torch.tensor(eps, dtype=x.dtype))
        x, y = x.double(), y.double()
        Px, H, W = x.shape
        cdiv = y.size(0) // Px
        ex = _expander(Px, cdiv)
        n = box_count(H, W, r)
        ref = forward_formulas(lambda v: box64(v, r), x, y, r, eps_k)
        mx, my, A, ve, mA, out, b = (ref[k] for k in ("mean_x", "mean_y", "A", "ve", "mean_A", "out", "b"))
        xe, mxe = ex(x), ex(mx)
        dmx = box_err(plan, x.abs(), 0.0, U) / n + U * mx.abs()
        xx = x * x
        Exx = ve - eps_k + mx * mx
        dExx = box_err(plan, xx, U * xx, U) / n + U * Exx
        dve = dExx + 2 * mx.abs() * dmx + U * mx * mx + U * (ve - eps_k).abs() + U * ve.abs()
        self.ve_condition = float((dve * (SAFETY / safety) * VE_CONDITION / ve).max())
        if not self.ve_condition <= 1.0:
            raise ValueError("guided filter: the bound of var_x + eps reaches %.3g of var_x + eps / %g: the first-order propagation "
                             "does not hold for these inputs" % (self.ve_condition, VE_CONDITION))
        dmy = box_err(plan, y.abs(), 0.0, U) / n + U * my.abs()
        xy = (xe * y).abs()
        cov = A * ex(ve)
        Exy = cov + mxe * my
        dExy = box_err(plan, xy, U * xy, U) / n + U * Exy.abs()
        dmxe, dvee, vee = ex(dmx), ex(dve), ex(ve)
        dcov = dExy + my.abs() * dmxe + mxe.abs() * dmy + U * (mxe * my).abs() + U * cov.abs()
        dA = dcov / vee + A.abs() * dvee / vee + U * A.abs()
        db = dmy + mxe.abs() * dA + A.abs() * dmxe + U * (A * mxe).abs() + U * b.abs()
        dmA = box_err(plan, A.abs(), dA, U) / n + U * mA.abs()
        mb = out - mA * xe
        dmb = box_err(plan, b.abs(), db, U) / n + U * mb.abs()
        dout = xe.abs() * dmA + dmb + U * (mA * xe).abs() + U * out.abs()
        self.ref = ref
        self.bound = {"mean_x": dmx, "mean_y": dmy, "A": dA, "ve": dve, "mean_A": dmA, "out": dout}

    def ratios(self, got):
        """got: dict name -> tensor.  -> {name: worst error / bound}."""
        return {k: worst_ratio(got[k], self.ref[k], self.bound[k]) for k in self.NAMES if k in got}


class BackwardBound:
    """ref / bound for grad_x, grad_y from x, y, g and the kernel's own saved planes (dict of tensors of the kernel's dtype)."""

    def __init__(self, plan, x, y, g, saved, safety=SAFETY):
        U = safety * unit(x.dtype)
        r = plan.r
        x, y, g = x.double(), y.double(), g.double()
        sv = {k: v.detach().to("cpu", torch.float64) for k, v in saved.items()}
        Px, H, W = x.shape
        Py = y.size(0)
        cdiv = Py // Px
        ex = _expander(Px, cdiv)
        n = box_count(H, W, r)
        self.ref = backward_formulas(lambda v: box64(v, r), x, y, g, sv, r)
        box = lambda v: box64(v, r)
        xe, mx, ve = ex(x), ex(sv["mean_x"]), ex(sv["ve"])
        my, A, mA = sv["mean_y"], sv["A"], sv["mean_A"]
        in1, in2 = g * xe / n, g / n
        q1, q2 = box(in1), box(in2)
        dq1 = box_err(plan, in1.abs(), 2 * U * in1.abs(), U)
        dq2 = box_err(plan, in2.abs(), U * in2.abs(), U)
        gA = q1 - q2 * mx
        dgA = dq1 + mx.abs() * dq2 + U * (q2 * mx).abs() + U * (q1.abs() + (q2 * mx).abs())
        gcov = gA / ve
        dgcov = dgA / ve.abs() + U * gcov.abs()
        gvar = -gA * A / ve
        dgvar = dgA * A.abs() / ve.abs() + 2 * U * gvar.abs()
        mag_gmx = (q2 * A).abs() + (gcov * my).abs() + 2 * (gvar * mx).abs()
        gmx = -q2 * A - gcov * my - 2 * gvar * mx
        dgmx = A.abs() * dq2 + my.abs() * dgcov + 2 * mx.abs() * dgvar + 3 * U * mag_gmx
        gmy = q2 - gcov * mx
        dgmy = dq2 + mx.abs() * dgcov + 2 * U * (q2.abs() + (gcov * mx).abs())

        def ch(t):
            return t.view(Px, cdiv, H, W).sum(1)
        sgmx, sgvar = ch(gmx), ch(gvar)
        dsgmx = ch(dgmx) + (cdiv - 1) * U * ch(mag_gmx)
        dsgvar = ch(dgvar) + (cdiv - 1) * U * ch(gvar.abs())
        mag_sgmx = ch(mag_gmx)

        def stage(v, mag, dv):                              # v / N, then the box
            w = v / n
            return box(w), box_err(plan, mag / n, dv / n + U * mag / n, U), _abox(mag / n, r)
        r1, dr1, a1 = stage(sgmx, mag_sgmx, dsgmx)
        r2, dr2, a2 = stage(gcov, gcov.abs(), dgcov)
        r3, dr3, a3 = stage(sgvar, ch(gvar.abs()), dsgvar)
        r4, dr4, a4 = stage(gmy, q2.abs() + (gcov * mx).abs(), dgmy)
        mag_gx = a1 + ch((g * mA).abs() + y.abs() * a2) + 2 * x.abs() * a3
        dgx = dr1 + ch(y.abs() * dr2) + 2 * x.abs() * dr3 + (2 + 2 * cdiv) * U * mag_gx
        dgy = xe.abs() * dr2 + dr4 + 2 * U * (xe.abs() * a2 + a4)
        self.bound = {"grad_x": dgx, "grad_y": dgy}

    def ratios(self, got):
        return {k: worst_ratio(got[k], self.ref[k], self.bound[k]) for k in ("grad_x", "grad_y") if got.get(k) is not None}


# ------------------------------------------------------------------------------------------------ the kernels' order in torch
def _scan64(d):
    """Inclusive scan of [..., 64] in six shuffle levels (gfg_wave_scan / line_box)."""
    o = 1
    while o < d.size(-1):
        d = torch.cat((d[..., :o], d[..., o:] + d[..., :-o]), -1)
        o *= 2
    return d


def _tree64(a):
    """Wave reduction of [..., 64] in six levels."""
    while a.size(-1) > 1:
        h = a.size(-1) // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def emu_line_fast(t, r, mutant=None):
    """line_box on the lines [..., L <= 128]."""
    L = t.size(-1)
    p = F.pad(t, (0, FAST_MAX - L)).view(*t.shape[:-1], WAVE, 2)
    a, b = p[..., 0], p[..., 1]
    b = b + a
    incl = _scan64(b)
    excl = incl - b
    c = torch.stack((a + excl, b + excl), -1).view(*t.shape[:-1], FAST_MAX)
    k = torch.arange(L)
    hi = (k + r + (1 if mutant == "hi_off_by_one" else 0)).clamp(max=L - 1)
    lo = k - r - 1
    h, l = c.index_select(-1, hi), c.index_select(-1, lo.clamp(min=0))
    return torch.where(lo >= 0, h - l, h)


def emu_line_cols(t, r, rc, mutant=None):
    """gfg_cols_kernel along the lines [..., L]: a sliding sum, seeded afresh every rc steps."""
    L = t.size(-1)
    up = 1 if mutant == "hi_off_by_one" else 0
    if mutant == "no_reseed":
        rc = L
    out = torch.empty_like(t)
    zero = torch.zeros_like(t[..., 0])
    for s in range(0, L, rc):
        lo, hi = max(s - 1 - r, 0), min(s - 1 + r + up, L - 1)
        if mutant == "seed_short" and s > 0:
            lo += 1
        acc = zero
        for i in range(lo, hi + 1):
            acc = acc + t[..., i]
        for i in range(s, min(s + rc, L)):
            ia, isub = i + r + up, i - r - 1
            add = t[..., ia] if ia < L else zero
            sub = t[..., isub] if isub >= 0 else zero
            acc = acc + (add - sub)
            out[..., i] = acc
    return out


def emu_line_rows(t, r, mutant=None):
    """gfg_row_boxes along the lines [..., L]: chunks of 256 outputs, a wave-reduced seed, four scanned segments."""
    L = t.size(-1)
    up = 1 if mutant == "hi_off_by_one" else 0
    out = torch.empty_like(t)
    lanes = torch.arange(WAVE)
    for s in range(0, L, ROW_CHUNK):
        e = min(s + ROW_CHUNK, L)
        lo, hi = max(s - 1 - r, 0), min(s - 1 + r + up, L - 1)
        if mutant == "seed_short" and s > 0:
            lo += 1
        acc = torch.zeros(*t.shape[:-1], WAVE, dtype=t.dtype)
        for m0 in range(lo, hi + 1, WAVE):
            seg = t[..., m0:min(m0 + WAVE, hi + 1)]
            acc = acc + F.pad(seg, (0, WAVE - seg.size(-1)))
        carry = _tree64(acc)
        for k0 in range(s, e, WAVE):
            k = k0 + lanes
            ia, isub = k + r + up, k - r - 1
            add = torch.where(ia < L, t.index_select(-1, ia.clamp(max=L - 1)), torch.zeros((), dtype=t.dtype))
            sub = torch.where((isub >= 0) & (isub < L), t.index_select(-1, isub.clamp(0, L - 1)), torch.zeros((), dtype=t.dtype))
            S = carry.unsqueeze(-1) + _scan64(add - sub)
            carry = S[..., WAVE - 1]
            out[..., k0:min(k0 + WAVE, e)] = S[..., :min(k0 + WAVE, e) - k0]
    return out


def emu_box(plan, v, mutant=None):
    """The kernels' box of [P, H, W] planes in v's dtype: columns, then rows."""
    r = plan.r
    if plan.kind == "fast":
        cols = _along(v, 1, lambda t: emu_line_fast(t, r, mutant))
        return _along(cols, 2, lambda t: emu_line_fast(t, r, mutant))
    cols = _along(v, 1, lambda t: emu_line_cols(t, r, plan.rc, mutant))
    return _along(cols, 2, lambda t: emu_line_rows(t, r, mutant))


def emulate_forward(plan, x, y, eps=EPS, mutant=None):
    return forward_formulas(lambda v: emu_box(plan, v, mutant), x, y, plan.r, eps, mutant)


def emulate_backward(plan, x, y, g, saved, mutant=None):
    return backward_formulas(lambda v: emu_box(plan, v, mutant), x, y, g, saved, plan.r, mutant)


# ------------------------------------------------------------------------------------------------ shared by the test files
def flat(case, tensors):
    B, Cx, Cy, H, W = case[:5]
    return [t.reshape(-1, H, W) for t in tensors]


def split_saved(saved, Px, Py, H, W):
    """The documented layout of `saved`: mean_x [Px], mean_y [Py], A [Py], var_x + eps [Px], mean_A [Py], flat."""
    s = saved.reshape(-1)
    out, at = {}, 0
    for name, planes in (("mean_x", Px), ("mean_y", Py), ("A", Py), ("ve", Px), ("mean_A", Py)):
        out[name] = s[at:at + planes * H * W].view(planes, H, W)
        at += planes * H * W
    assert at == s.numel(), (at, s.numel())
    return out


@functools.lru_cache(maxsize=None)
def inputs(name, family):
    """Cached, never modified: the flat float32 x, y, g of a case of CASES."""
    case = CASES[name][0]
    return tuple(flat(case, make_inputs(case, family)))


@functools.lru_cache(maxsize=None)
def forward_bound(name, family, dtype):
    x, y, _ = inputs(name, family)
    return ForwardBound(plans(CASES[name][0])[0], x.to(dtype), y.to(dtype))
