"""Per-element float64 error bounds, input families and a float32 emulation for the fused landmark loss
(csrc/landmark_loss.hip, ffwm_landmark_loss) -- a plain helper module, not a conftest.  The convention is that of
tests/correctness_bounds.py.

The reference is float64 torch on the CPU, computed from the call's ACTUAL inputs (the float values it is handed, widened; the
integer landmarks as they are).  u = 2^-24 (2^-53 for a float64 call), one SAFETY = 4 multiplies every count of roundings
(U = SAFETY u below), FLOOR = 1e-38 keeps a bound of exactly zero from dividing.  No constant is fitted to the kernel's output:
each is a count of roundings read off the kernel's arithmetic, which is (per scale: side s, divisor q, weight; the library is
built without FMA contraction)
    in range     0 <= lm_F[b,l,0] < s q and 0 <= lm_F[b,l,1] < s q           (else the landmark is skipped by this scale)
    cell         (X, Y) = (lm_F[b,l,0] div q, lm_F[b,l,1] div q)              exact integers
    w_c          = T(lm_S[b,l,c] div q) * T(2 / s) - 1                        the conversion is exact below 2^24 (2^53): a CONDITION
    d_c          = flow[b,c,Y,X] - w_c                                        1 rounding
    acc_c       += (gate_c * gate_c) * d_c     in landmark order              2 roundings per term, 1 per addition
    grad[b,c,Y,X] = T(weight / (B L)) * acc_c                                 1 rounding of the coefficient, 1 of the product
    e_c          = d_c * gate_c                                               1 rounding
    sum          += double(e_c) * double(e_c)  in double, fixed order         1 double rounding per product and per addition
    out[1 + i]   = T(sum / (2 B L)),   out[0] = T(sum_i weight_i (sum_i / (2 B L)))   in double, then one rounding to T

The target.  When 2 / s is a power of two (s = 1, 2, 4, ...: 128, 64, 32) the product only changes the exponent and
n 2^-k - 1 = (n - 2^k) 2^-k has an integer numerator below 2^24: w_c is EXACT.  Otherwise T(2 / s) is rounded, the product is
rounded and the subtraction is rounded, each on a value of at most |w_c| + 1: 3 u (|w_c| + 1), priced as
    ew = 2 U (|w_c| + 1)                                 (0 when 2 / s is a power of two)
an ABSOLUTE error of the target that moves d_c, and with it every term, by as much.

A gradient element with n >= 1 contributing landmarks, terms t_l = coef gate^2 (flow - w_c), coef = weight / (B L):
    d_c, gate^2, their product, the coefficient, the last product: k = 5 roundings, the n - 1 additions fewer than n more, every
    one relative to at most sum |t_l|:
    bound = U (5 + n) sum_l |t_l| + coef sum_l gate^2 ew
An element with no contributing landmark is written as 0 and asserted == 0 (so is everything under an all-zero gate).

The loss of a scale.  All terms e^2 are non-negative, so the bound is relative to S = sum e^2, except for the target's error:
    e_c carries 2 roundings and |gate| ew:    de = 2 U |e| + |gate| ew,    d(e^2) = 2 |e| de  =  4 U e^2 + 2 |e| |gate| ew
    the N = 2 B L products and the additions of the double accumulation (per thread, xor butterfly, wave order, slots in index
    order, tree: any order has fewer than 2 N additions on partial sums of at most S):  3 N SAFETY 2^-53 S
    the division in double, then the rounding to T:  U mse
    bound_i = (4 U S + 2 sum |e| |gate| ew + 3 N SAFETY 2^-53 S) / (2 B L) + U mse_i
    out[0]:  sum_i |weight_i| bound_i + U |out[0]|       (the weighted sum in double: inside the SAFETY of the terms above)
A module-level result multiplies the stored gradient by grad_output: 2 U |ref| more per element.
For a float64 call the reference rounds as often as the kernel does: the assertions take twice the bound.

Input families (FAMILIES), R = s q the range of the coordinates (the same for every scale of a case):
    random       landmarks in [R / 8, 7 R / 8) (that is [16, 112) for R = 128), gates uniform in [0.5, 1.5)
    clustered    every landmark of a sample on one of three points: (0, 0), (R - 1, R - 1) and one more -- at most three cells per
                 scale, among them (0, 0) and (s - 1, s - 1); binary gates
    half_gated   random, half the landmarks gated off (both channels)
    gated_off    random, all gates 0: out and every gradient element must be == 0
    outside      random, a quarter of the lm_F ENTRIES (components) replaced in turn by -1, R and 2^40; `skipped` is the number of
                 landmarks with such a component, and they contribute nothing
    negative_S   random, lm_S in [-R, R): the floor division of negative numerators
"""
import math

import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 4.0
FLOOR = 1e-38
GUARD = 64                   # NaN cells before and behind every gradient destination
FAMILIES = ("random", "clustered", "half_gated", "gated_off", "outside", "negative_S")
# (B, L): one landmark; fewer than a chunk of 256; an odd count; exactly four chunks, more than one sample; a ragged sixth chunk
SHAPES = ((1, 1), (2, 40), (3, 67), (2, 1024), (1, 1500))
# ((side, divisor), ...): the three scales of MultiScaleLDLoss in one call; a side whose 400 cells end inside the second tile
# with 2 / s rounded; a divisor that is no power of two with 2 / s rounded
SCALES = (((128, 1), (64, 2), (32, 4)), ((20, 1),), ((24, 5),))
LD_WEIGHTS = (1000.0, 1000.0, 1500.0)


def unit(dtype):
    return U32 if dtype == torch.float32 else U64


class Case:
    """One call's inputs: flows (CPU tensors of the call's dtype), lm_S, lm_F (int64), gate, sides, divisors, weights."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def dtype(self):
        return self.flows[0].dtype

    def __repr__(self):
        B, L, _ = self.lm_S.shape
        return "%s B%d L%d %s %s" % (self.family, B, L, "/".join("%dq%d" % sq for sq in zip(self.sides, self.divisors)),
                                     str(self.dtype).replace("torch.", ""))


def make_case(B, L, scales, family, dtype=torch.float32, seed=0, weights=None):
    assert family in FAMILIES
    sides, divisors = [s for s, _ in scales], [q for _, q in scales]
    R = sides[0] * divisors[0]
    assert all(s * q == R for s, q in scales), "one coordinate range per case"
    gen = torch.Generator().manual_seed(7919 * seed + 131 * FAMILIES.index(family) + 17 * B + L + 3 * R + len(scales))
    lo, hi = R // 8, 7 * R // 8
    lm_F = torch.randint(lo, hi, (B, L, 2), generator=gen)
    lm_S = torch.randint(lo, hi, (B, L, 2), generator=gen)
    gate = 0.5 + torch.rand(B, L, 2, generator=gen, dtype=torch.float64)
    if family == "clustered":
        third = torch.randint(1, R - 1, (B, 1, 2), generator=gen)
        points = torch.cat((torch.zeros(B, 1, 2, dtype=torch.int64), torch.full((B, 1, 2), R - 1), third), 1)       # [B, 3, 2]
        pick = torch.randint(0, 3, (B, L), generator=gen)
        pick[:, 0] = 0
        pick[:, -1] = 1
        lm_F = points.gather(1, pick.unsqueeze(2).expand(B, L, 2))
        gate = (torch.rand(B, L, 1, generator=gen) > 0.2).double().expand(B, L, 2).clone()
    elif family == "half_gated":
        on = torch.rand(B, L, 1, generator=gen) < 0.5
        gate = gate * on
    elif family == "gated_off":
        gate = torch.zeros(B, L, 2, dtype=torch.float64)
    elif family == "outside":
        bad = torch.rand(B, L, 2, generator=gen) < 0.25
        bad.view(-1)[0] = True
        values = torch.tensor([-1, R, 2 ** 40])[torch.arange(B * L * 2) % 3].view(B, L, 2)
        lm_F = torch.where(bad, values, lm_F)
    elif family == "negative_S":
        lm_S = torch.randint(-R, R, (B, L, 2), generator=gen)
        lm_S.view(-1)[0] = -1
    flows = [(torch.rand(B, 2, s, s, generator=gen, dtype=torch.float64) * 2 - 1).to(dtype).contiguous() for s in sides]
    if weights is None:
        weights = LD_WEIGHTS[:len(scales)] if len(scales) > 1 else (1.0,)
    return Case(flows=flows, lm_S=lm_S.contiguous(), lm_F=lm_F.contiguous(), gate=gate.to(dtype).contiguous(), sides=sides,
                divisors=divisors, weights=[float(w) for w in weights], family=family)


def _floor_div(t, q):
    return torch.div(t, q, rounding_mode="floor")


def _power_of_two(x):
    return math.frexp(x)[0] == 0.5


class Scale:
    """The float64 reference and the bounds of one scale."""

    def __init__(self, case, i, U):
        B, L, _ = case.lm_S.shape
        s, q, weight = case.sides[i], case.divisors[i], case.weights[i]
        flow = case.flows[i].double()
        limit = (2.0 ** 24 if case.dtype == torch.float32 else 2.0 ** 53)
        if int(_floor_div(case.lm_S, q).abs().max()) >= limit:
            raise ValueError("%r: lm_S div q does not convert exactly" % case)
        inside = ((case.lm_F >= 0) & (case.lm_F < s * q)).all(2)                                   # [B, L]
        self.inside = inside
        cell_xy = _floor_div(case.lm_F.clamp(0, s * q - 1), q)
        cell = cell_xy[..., 1] * s + cell_xy[..., 0]                                              # [B, L]
        index = cell.unsqueeze(1).expand(B, 2, L)
        w = (_floor_div(case.lm_S, q).double() * (2.0 / s) - 1).transpose(1, 2)                    # [B, 2, L]
        g = case.gate.double().transpose(1, 2) * inside.unsqueeze(1)                              # a skipped landmark: gate 0
        d = flow.flatten(2).gather(2, index) - w
        e = d * g
        N = 2 * B * L
        S = float((e * e).sum())
        self.mse = S / N
        coef = weight / (B * L)
        terms = coef * g * g * d
        self.grad = torch.zeros(B, 2, s * s, dtype=torch.float64).scatter_add_(2, index, terms).view(B, 2, s, s)
        ew = torch.zeros_like(w) if _power_of_two(2.0 / s) else 2 * U * (w.abs() + 1)
        live = (inside.unsqueeze(1).expand(B, 2, L)).double()
        count = torch.zeros(B, 2, s * s, dtype=torch.float64).scatter_add_(2, index, live)
        mag = torch.zeros(B, 2, s * s, dtype=torch.float64).scatter_add_(2, index, terms.abs())
        shift = torch.zeros(B, 2, s * s, dtype=torch.float64).scatter_add_(2, index, coef * g * g * ew)
        self.touched = (count > 0).view(B, 2, s, s)
        self.grad_bound = (U * (5 + count) * mag + shift).view(B, 2, s, s)
        self.loss_bound_unrounded = (4 * U * S + 2 * float((e.abs() * g.abs() * ew).sum()) + 3 * N * SAFETY * U64 * S) / N
        self.loss_bound = self.loss_bound_unrounded + U * self.mse


class Bound:
    def __init__(self, case, safety=SAFETY):
        self.case = case
        self.U = U = safety * unit(case.dtype)
        self.twice = 2.0 if case.dtype == torch.float64 else 1.0
        self.scales = [Scale(case, i, U) for i in range(len(case.sides))]
        self.out0 = sum(w * sc.mse for w, sc in zip(case.weights, self.scales))
        self.out0_bound = sum(abs(w) * sc.loss_bound_unrounded for w, sc in zip(case.weights, self.scales)) + U * abs(self.out0)
        bad = ~self.scales[0].inside
        for sc in self.scales[1:]:
            bad = bad | ~sc.inside
        self.skipped = int(bad.sum())

    def _ratio(self, got, ref, bound):
        got = got.detach().to("cpu", torch.float64).reshape(ref.shape)
        r = (got - ref).abs() / (bound + FLOOR)
        r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
        return float(r.max()) if r.numel() else 0.0

    def check(self, out=None, grads=None, skipped=None, what="", factor=1.0, verbose=True):
        """The entry point's outputs (any may be None; grads[i] may be None) against the bounds; untouched cells exactly 0."""
        rows, fails = {}, []
        f = factor * self.twice
        if out is not None:
            o = out.detach().cpu().double()
            rows["out0"] = abs(float(o[0]) - self.out0) / (f * self.out0_bound + FLOOR)
            for i, sc in enumerate(self.scales):
                rows["mse%d" % i] = abs(float(o[1 + i]) - sc.mse) / (f * sc.loss_bound + FLOOR)
            if self.case.family == "gated_off" and not bool((o == 0).all()):
                fails.append("out != 0 under an all-zero gate")
        for i, g in enumerate(grads or []):
            if g is None:
                continue
            sc = self.scales[i]
            gc = g.detach().cpu()
            rows["grad%d" % i] = self._ratio(gc, sc.grad, f * sc.grad_bound)
            if not bool((gc[~sc.touched] == 0).all()):
                fails.append("grad%d != 0 on %d cells without a landmark" % (i, int((gc[~sc.touched] != 0).sum())))
            if self.case.family == "gated_off" and not bool((gc == 0).all()):
                fails.append("grad%d != 0 under an all-zero gate" % i)
        if skipped is not None and int(skipped) != self.skipped:
            fails.append("skipped = %d, expected %d" % (int(skipped), self.skipped))
        return self._finish(rows, fails, what, verbose)

    def check_module(self, loss, flow_grads, grad_output=1.0, what="", factor=1.0, verbose=True):
        """A module-level result: the loss and d(grad_output * loss)/d(flow_i) = grad_output * the stored gradient."""
        f = factor * self.twice
        rows = {"loss": abs(float(loss) - self.out0) / (f * self.out0_bound + FLOOR)}
        for i, (g, sc) in enumerate(zip(flow_grads, self.scales)):
            ref = grad_output * sc.grad
            rows["flow%d.grad" % i] = self._ratio(g, ref, f * (abs(grad_output) * sc.grad_bound + 2 * self.U * ref.abs()))
        return self._finish(rows, [], what, verbose)

    def _finish(self, rows, fails, what, verbose):
        if verbose:
            print("LMBOUND %s %r: %s" % (what, self.case, " ".join("%s %.3g" % kv for kv in sorted(rows.items()))))
        fails += ["%s: error / bound = %.3g" % kv for kv in sorted(rows.items()) if not kv[1] <= 1.0]
        assert not fails, "%s %r: %s" % (what, self.case, "; ".join(fails))
        return rows


def emulate(case, chunk=37):
    """The kernel's arithmetic in torch on the CPU, in the case's dtype: the same operations in the same order PER TERM, the terms of
    a cell added chunk by chunk from the LAST chunk to the first (another order than the kernel's, which a bound on any order must
    cover), the squares in double.  -> (out [n + 1], grads, skipped)."""
    T = case.dtype
    B, L, _ = case.lm_S.shape
    out, grads = torch.zeros(len(case.sides) + 1, dtype=torch.float64), []
    bad = torch.zeros(B, L, dtype=torch.bool)
    for i, (s, q, weight) in enumerate(zip(case.sides, case.divisors, case.weights)):
        flow = case.flows[i]
        inside = ((case.lm_F >= 0) & (case.lm_F < s * q)).all(2)
        bad |= ~inside
        cell_xy = _floor_div(case.lm_F.clamp(0, s * q - 1), q)
        index = (cell_xy[..., 1] * s + cell_xy[..., 0]).unsqueeze(1).expand(B, 2, L)
        two_over_s = torch.tensor(2.0 / s, dtype=T)
        w = (_floor_div(case.lm_S, q).to(T) * two_over_s - 1).transpose(1, 2)
        g = (case.gate * inside.unsqueeze(2)).transpose(1, 2)
        d = flow.flatten(2).gather(2, index) - w
        terms = (g * g) * d
        e = d * g
        acc = torch.zeros(B, 2, s * s, dtype=T)
        for l0 in reversed(range(0, L, chunk)):
            part = torch.zeros(B, 2, s * s, dtype=T).scatter_add_(2, index[..., l0:l0 + chunk], terms[..., l0:l0 + chunk].contiguous())
            acc = acc + part
        coef = torch.tensor(weight / (B * L), dtype=T)
        grads.append((coef * acc).view(B, 2, s, s))
        mse = float((e.double() * e.double()).sum()) / (2 * B * L)
        out[1 + i] = mse
        out[0] += weight * mse
    return out.to(T), grads, int(bad.sum())
