"""Per-pixel float64 error bounds, input families and their conditions for the fused sampling-correctness loss
(csrc/sampling_correctness.hip, ffwm_sampling_correctness) -- a plain helper module, not a conftest.

The reference is float64 torch on the CPU, computed from the kernel's ACTUAL inputs (the float values it is handed, widened):
F.grid_sample (bilinear / zeros / align_corners=False), F.cosine_similarity, exp, and autograd for the gradient of
sum(mask loss_map) with respect to the flow -- every loss_map pixel depends on its own flow vector alone, so that gradient IS
mask d(loss_map)/d(flow), what the kernel stores.  u = 2^-24 (2^-53 for a float64 call), one SAFETY = 4 multiplies every count
of roundings (U = SAFETY u below), FLOOR = 1e-38 keeps a bound of exactly zero from dividing.  No constant is fitted to the
kernel's output.  For a float64 call the reference rounds as often as the kernel does: the assertions take twice the bound.

Notation, per pixel and channel c: v00, v01, v10, v11 the four taps (0 when out of range), tx, ty the fractional coordinates,
    s  = sum_q w_q v_q                                   A  = sum_q w_q |v_q|
    dx = (1 - ty)(v01 - v00) + ty (v11 - v10)            Gx = (1 - ty)|v01 - v00| + ty |v11 - v10|        Rx = |v01 - v00| + |v11 - v10|
    dy = (1 - tx)(v10 - v00) + tx (v11 - v01)            Gy, Ry likewise
Magnitudes are formed on absolute values throughout (Dabs = sum |s||t|, Pxabs = sum |t| Gx, Qxabs = sum |s| Gx, ...): the
cancellation inside D, Px, Qx and in cos' = Px / (ns nt) - cos Qx / S is priced, not hidden.

The sampling position.  px = ((f + 1) Wi - 1) / 2 rounds three times (the addition, the product, the subtraction; halving is
exact) and tx = px - floor(px) once more, each on a value of at most |f + 1| Wi + 2:
    etx = 3 U (|fx + 1| Wi + 2),     ety likewise with Hi.
A position error moves the sample by its derivative, which is only meaningful while float and double agree on the taps: the
CONDITION (checked in float64 AND in the float arithmetic of the kernel, ValueError otherwise) is that every pixel with a tap in
range has both fractional coordinates in [1/16, 15/16] and the same floor in both arithmetics.
    es  = Gx etx + Gy ety + 7 U A          (1 - tx, the four weight products... : 2 per weight, 1 per product, 3 additions <= 7)
    edx = Rx ety + 4 U Gx                  (the differences, 1 - ty, the products, the addition; d(dx)/d(ty) <= Rx)
    edy = Ry etx + 4 U Gy
The channel sums, n = C terms in ANY order ((n - 1) additions + the product: (n + 1) U times the sum of magnitudes):
    eD  = sum es |t| + (n + 1) U Dabs            eS = 2 sum es |s| + (n + 1) U S            eT = (n + 1) U T
    ePx = sum edx |t| + (n + 1) U Pxabs          eQx = sum (edx |s| + es Gx) + (n + 1) U Qxabs             (y likewise)
Norms and cosine: rel_ns = eS / (2 S) + 2 U (the square root), rel_nt = eT / (2 T) + 2 U, inv = 1 / (ns nt), cosabs = Dabs inv,
    ecos = eD inv + cosabs (rel_ns + rel_nt + 3 U)                        (ns nt, the reciprocal, the product)
The CONDITION that makes rel_ns meaningful and keeps [sqrt S > 1e-8] the same in every arithmetic: a pixel is either WHOLLY
OUTSIDE (all four taps out of range: s = 0 exactly, and then loss_map == 1 and grad_flow == 0 EXACTLY, asserted with ==) or has
sqrt S >= 1e-4; the count of pixels between the two states must be exactly 0 (features are rand + 0.1).  corr_max lies in
[0.25, 1], so the exponent stays in [-4, 4].
    cme = corr_max + eps,    earg = ecos / cme + 3 U cosabs / cme         (the addition, the division, float(eps) against eps)
    em  = m expm1(earg) + K_EXP u m
The exponential: the kernel calls the device library's expf / exp, whose accuracy no document available to this project states.
As tests/bn_bounds.py did for the sigmoid, float32 torch.exp was measured against float64 on the CPU over the range the cases
produce and beyond: 2^24 uniform samples x 4 and a 2^24-point grid in [-4.1, 4.1], and 2^24 arguments +-2^-k r (k < 40, r
uniform); the worst |exp_f32 - exp_f64| / (u exp_f64) seen was 1.032 (at 2.794): EXP_WORST = 1.05, K_EXP = SAFETY x 1.05.
The gradient, cos'_x = t1 - t2 with t1 = Px inv, t2 = cos Qx / S (t1abs = Pxabs inv, t2abs = cosabs Qxabs / S, cpabs = t1abs + t2abs):
    et1 = ePx inv + t1abs (rel_ns + rel_nt + 3 U)
    et2 = ecos Qxabs / S + cosabs eQx / S + t2abs (2 rel_ns + 3 U)
    ecp = et1 + et2 + U cpabs
    grad_x = -mask m / cme cos'_x Wi / 2:   eg = |mask| (Wi / 2) / cme (em cpabs + m ecp) + 6 U gabs,  gabs = |mask| m / cme cpabs Wi / 2
out[0], with N pixels: the kernel adds mask m in double (N u64 per unit of sum |mask| m, + U for the product), a float
composition in any order N U (float_sums=True, for the stand-in only):
    masked:   [sum |mask| em + rho_sum sum |mask| m] / den + 4 U (sum |mask| m + e1) / den,   den = sum mask + eps
    unmasked: [sum em + rho_sum sum m] / N + 3 U (sum m / N + e1)
An all-zero mask gives the reference's (0 - e1) / (0 + eps) within 4 U e1 / eps.
A module-level result (loss, flow.grad) divides the stored gradient by out[1] and multiplies by grad_output: 2 U more.

Input families (FAMILIES): `smooth` interior flow, `random` in-range flow, `left` / `right` / `top` / `bottom` straddling one
border (half the pixels have their outer taps out of range), `mixed` (random with a quarter of the pixels wholly outside),
`outside` (every pixel has |f| > 1 + 3 / size on an axis).  Masks (MASKS): `none`, `binary` (zeros and ones, rows 0 and H // 2
entirely zero), `zero`.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 4.0
FLOOR = 1e-38
EXP_WORST = 1.05             # measured, see the docstring
TINY = 1e-8                  # F.cosine_similarity's eps
EPS = 1e-8                   # PerceptualCorrectness.eps
FAMILIES = ("smooth", "random", "left", "right", "top", "bottom", "mixed", "outside")
MASKS = ("none", "binary", "zero")
GUARD = 64                   # NaN cells behind every output of a C-ABI call


def unit(dtype):
    return U32 if dtype == torch.float32 else U64


def exp_minus_one(dtype):
    return float(torch.exp(torch.tensor(-1.0, dtype=dtype)))


class Case:
    """One call's inputs (CPU tensors of the call's dtype; mask None = a NULL pointer) and scalars."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def dims(self):
        B, C, Hi, Wi = self.source.shape
        return B, C, Hi, Wi, self.target.shape[2], self.target.shape[3]

    def __repr__(self):
        return "%s/%s %s %s" % (self.family, self.mask_kind, self.dims, str(self.source.dtype).replace("torch.", ""))


# ------------------------------------------------------------------------------------------------ inputs
def _positions(family, B, H, W, size, axis, gen):
    """Sampling positions in source pixels along one axis (float64 [B, H, W]) with fractional parts in [1/8, 7/8]."""
    frac = 0.125 + 0.75 * torch.rand(B, H, W, generator=gen, dtype=torch.float64)
    cell = torch.randint(0, max(size - 1, 1), (B, H, W), generator=gen).double()          # 0 .. size - 2: both taps in range
    if family == "smooth":
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        along, across = (xs, ys) if axis == 0 else (ys, xs)
        n_along = W if axis == 0 else H
        p = 0.5 + along * (size - 2.0) / max(n_along - 1, 1) + 0.4 * torch.sin(0.7 * across + 0.3 * along + axis)
        p = p.clamp(0.0, size - 1.125).unsqueeze(0).repeat(B, 1, 1)
        cell = torch.floor(p)
        frac = (p - cell).clamp(0.125, 0.875)
    side = {"left": (0, -1.0), "right": (0, size - 1.0), "top": (1, -1.0), "bottom": (1, size - 1.0)}.get(family)
    if side is not None and side[0] == axis:
        straddle = torch.rand(B, H, W, generator=gen) < 0.5
        straddle.view(-1)[0] = True
        cell = torch.where(straddle, torch.full_like(cell, side[1]), cell)
    return cell + frac


def make_case(shape, family, mask_kind="none", dtype=torch.float32, seed=0):
    """shape = (B, C, Hi, Wi, H, W)."""
    B, C, Hi, Wi, H, W = shape
    assert family in FAMILIES and mask_kind in MASKS
    gen = torch.Generator().manual_seed(977 * seed + 31 * FAMILIES.index(family) + 7 * MASKS.index(mask_kind) + C + Hi * Wi + 3 * H * W)
    source = (torch.rand(B, C, Hi, Wi, generator=gen, dtype=torch.float64) + 0.1).to(dtype)
    target = (torch.rand(B, C, H, W, generator=gen, dtype=torch.float64) + 0.1).to(dtype)
    fam = "random" if family in ("mixed", "outside") else family
    px = _positions(fam, B, H, W, Wi, 0, gen)
    py = _positions(fam, B, H, W, Hi, 1, gen)
    fx = (2 * px + 1) / Wi - 1
    fy = (2 * py + 1) / Hi - 1
    if family in ("mixed", "outside"):
        out = torch.ones(B, H, W, dtype=torch.bool) if family == "outside" else torch.rand(B, H, W, generator=gen) < 0.25
        if family == "mixed":
            out.view(-1)[1] = True
        which = torch.randint(0, 3, (B, H, W), generator=gen)                       # x, y, both
        sign = torch.where(torch.rand(B, H, W, generator=gen) < 0.5, -1.0, 1.0).double()
        far = torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 0.5 + 1e-3
        fx = torch.where(out & (which != 1), sign * (1 + 3.0 / Wi + far), fx)
        fy = torch.where(out & (which != 0), -sign * (1 + 3.0 / Hi + far), fy)
    flow = torch.stack((fx, fy), 1).to(dtype).contiguous()
    mask = None
    if mask_kind == "binary":
        mask = (torch.rand(B, H, W, generator=gen) < 0.6).to(dtype)
        mask[:, 0] = 0
        mask[:, H // 2] = 0
        mask = mask.reshape(B, H * W).contiguous()
    elif mask_kind == "zero":
        mask = torch.zeros(B, H * W, dtype=dtype)
    case = Case(source=source.contiguous(), target=target.contiguous(), flow=flow, mask=mask, corr_max=None, family=family,
                mask_kind=mask_kind, eps=EPS, e1=exp_minus_one(dtype))
    case.corr_max = correlation_max(case.source, case.target, EPS)
    return case


def correlation_max(source, target, eps=EPS):
    """The correlation maximum exactly as PerceptualCorrectness.calculate_loss forms it (ffwm_amd/losses.py, the bmm + max route)."""
    b, c = target.shape[:2]
    with torch.no_grad():
        target_all = target.reshape(b, c, -1)
        source_all = source.reshape(b, c, -1).transpose(1, 2)
        source_norm = source_all / (source_all.norm(dim=2, keepdim=True) + eps)
        target_norm = target_all / (target_all.norm(dim=1, keepdim=True) + eps)
        return torch.bmm(source_norm, target_norm).max(dim=1)[0].contiguous()


# ------------------------------------------------------------------------------------------------ the taps and the conditions
def _coords(flow, size, axis, dtype):
    """px (or py) as `dtype` arithmetic forms it, widened: ((f + 1) size - 1) / 2, [B, H W]."""
    f = flow[:, axis].reshape(flow.shape[0], -1).to(dtype)
    return (((f + 1) * size - 1) / 2).double()


class Taps:
    """floor, fraction and validity of the four taps of every pixel, from the flow the kernel is given, in float64."""

    def __init__(self, case):
        B, C, Hi, Wi, H, W = case.dims
        dt = case.flow.dtype
        self.px, self.py = _coords(case.flow, Wi, 0, torch.float64), _coords(case.flow, Hi, 1, torch.float64)
        self.x0, self.y0 = torch.floor(self.px), torch.floor(self.py)
        self.tx, self.ty = self.px - self.x0, self.py - self.y0
        xs = (self.x0, self.x0 + 1, self.x0, self.x0 + 1)
        ys = (self.y0, self.y0, self.y0 + 1, self.y0 + 1)
        self.valid = [(x >= 0) & (x < Wi) & (y >= 0) & (y < Hi) for x, y in zip(xs, ys)]
        self.index = [(y.clamp(0, Hi - 1) * Wi + x.clamp(0, Wi - 1)).long() for x, y in zip(xs, ys)]
        self.outside = ~(self.valid[0] | self.valid[1] | self.valid[2] | self.valid[3])
        # the same in the call's own arithmetic: the floors must agree and the fractions stay off the kink
        lx, ly = _coords(case.flow, Wi, 0, dt), _coords(case.flow, Hi, 1, dt)
        live = ~self.outside
        bad = live & ((torch.floor(lx) != self.x0) | (torch.floor(ly) != self.y0))
        for t in (self.tx, self.ty, lx - torch.floor(lx), ly - torch.floor(ly)):
            bad |= live & ((t < 1.0 / 16) | (t > 15.0 / 16))
        # a pixel the call's arithmetic sees outside must be outside here too (and the other way round)
        lxs = (torch.floor(lx), torch.floor(lx) + 1)
        lys = (torch.floor(ly), torch.floor(ly) + 1)
        l_any = torch.zeros_like(live)
        for x in lxs:
            for y in lys:
                l_any |= (x >= 0) & (x < Wi) & (y >= 0) & (y < Hi)
        bad |= l_any != live
        if bool(bad.any()):
            raise ValueError("%r: %d pixels whose taps differ between float64 and the call's arithmetic, or whose fractional "
                             "coordinates leave [1/16, 15/16]" % (case, int(bad.sum())))


def check_conditions(case, taps, S):
    between = ~taps.outside & (torch.sqrt(S) < 1e-4)
    if int(between.sum()) != 0:
        raise ValueError("%r: %d pixels are neither wholly outside nor have sqrt(S) >= 1e-4" % (case, int(between.sum())))
    cm = case.corr_max.double()
    if not bool(((cm >= 0.25) & (cm <= 1.0)).all()):
        raise ValueError("%r: corr_max leaves [0.25, 1] (%.3g .. %.3g)" % (case, float(cm.min()), float(cm.max())))


# ------------------------------------------------------------------------------------------------ the reference and the bounds
def reference(case):
    """float64: loss_map [B, H W], mask d(loss_map)/d(flow) [B, 2, H, W], out[0], out[1]."""
    B, C, Hi, Wi, H, W = case.dims
    flow = case.flow.detach().double().clone().requires_grad_(True)
    sample = F.grid_sample(case.source.double(), flow.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=False)
    cos = F.cosine_similarity(sample.reshape(B, C, -1), case.target.double().reshape(B, C, -1))
    m = torch.exp(-cos / (case.corr_max.double() + case.eps))
    mask = None if case.mask is None else case.mask.double()
    weighted = m if mask is None else mask * m
    (grad,) = torch.autograd.grad(weighted.sum(), flow)
    if mask is None:
        out1 = float(B * H * W)
        out0 = float(m.detach().sum()) / out1 - case.e1
    else:
        out1 = float(mask.sum()) + case.eps
        out0 = (float(weighted.detach().sum()) - case.e1) / out1
    return m.detach(), grad.detach(), out0, out1


class Bound:
    def __init__(self, case, safety=SAFETY, float_sums=False):
        """float_sums: for a stand-in that adds the pixels in float (the torch composition); never for the kernel."""
        self.case, self.safety = case, safety
        B, C, Hi, Wi, H, W = case.dims
        N = B * H * W
        u = unit(case.source.dtype)
        U = safety * u
        self.U = U
        self.twice = 2.0 if case.source.dtype == torch.float64 else 1.0
        tp = Taps(case)
        self.outside = tp.outside
        src = case.source.double().reshape(B, C, Hi * Wi)
        t = case.target.double().reshape(B, C, H * W)
        v = [src.gather(2, i.unsqueeze(1).expand(B, C, H * W)) * ok.unsqueeze(1) for i, ok in zip(tp.index, tp.valid)]
        tx, ty = tp.tx.unsqueeze(1), tp.ty.unsqueeze(1)
        w = ((1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty)
        s = sum(wq * vq for wq, vq in zip(w, v))
        A = sum(wq * vq.abs() for wq, vq in zip(w, v))
        d01, d23, d02, d13 = v[1] - v[0], v[3] - v[2], v[2] - v[0], v[3] - v[1]
        Gx, Rx = (1 - ty) * d01.abs() + ty * d23.abs(), d01.abs() + d23.abs()
        Gy, Ry = (1 - tx) * d02.abs() + tx * d13.abs(), d02.abs() + d13.abs()
        fx = case.flow[:, 0].double().reshape(B, 1, H * W)
        fy = case.flow[:, 1].double().reshape(B, 1, H * W)
        etx, ety = 3 * U * ((fx + 1).abs() * Wi + 2), 3 * U * ((fy + 1).abs() * Hi + 2)
        es = Gx * etx + Gy * ety + 7 * U * A
        edx, edy = Rx * ety + 4 * U * Gx, Ry * etx + 4 * U * Gy
        nU = (C + 1) * U
        sa, ta = s.abs(), t.abs()
        Dabs, S, T = (sa * ta).sum(1), (s * s).sum(1), (t * t).sum(1)
        check_conditions(case, tp, S)
        eD = (es * ta).sum(1) + nU * Dabs
        eS = 2 * (es * sa).sum(1) + nU * S
        eT = nU * T
        ns, nt = torch.sqrt(S).clamp_min(TINY), torch.sqrt(T).clamp_min(TINY)
        live = ~tp.outside
        Ssafe = torch.where(live, S, torch.ones_like(S))
        rel_ns = torch.where(live, eS / (2 * Ssafe), torch.zeros_like(S)) + 2 * U
        rel_nt = eT / (2 * T) + 2 * U
        inv = 1.0 / (ns * nt)
        cosabs = Dabs * inv
        ecos = eD * inv + cosabs * (rel_ns + rel_nt + 3 * U)
        cme = case.corr_max.double() + case.eps
        earg = ecos / cme + 3 * U * cosabs / cme
        self.ref_map, self.ref_grad, self.ref_out0, self.ref_out1 = reference(case)
        m = self.ref_map
        em = m * torch.expm1(earg) + safety * EXP_WORST * u * m
        self.map_bound = self.twice * em
        mk = torch.ones_like(m) if case.mask is None else case.mask.double().abs()
        bounds = []
        for Gd, ed, size in ((Gx, edx, Wi), (Gy, edy, Hi)):
            Pabs, Qabs = (ta * Gd).sum(1), (sa * Gd).sum(1)
            eP = (ed * ta).sum(1) + nU * Pabs
            eQ = (ed * sa + es * Gd).sum(1) + nU * Qabs
            t1abs, t2abs = Pabs * inv, torch.where(live, cosabs * Qabs / Ssafe, torch.zeros_like(S))
            et1 = eP * inv + t1abs * (rel_ns + rel_nt + 3 * U)
            et2 = torch.where(live, (ecos * Qabs + cosabs * eQ) / Ssafe, torch.zeros_like(S)) + t2abs * (2 * rel_ns + 3 * U)
            cpabs = t1abs + t2abs
            ecp = et1 + et2 + U * cpabs
            gabs = mk * m / cme * cpabs * size / 2
            bounds.append(mk * (size / 2.0) / cme * (em * cpabs + m * ecp) + 6 * U * gabs)
        self.grad_bound = self.twice * torch.stack(bounds, 1).reshape(B, 2, H, W)
        rho_sum = (N * U if float_sums else N * safety * U64) + U
        wm = float((mk * m).sum())
        if case.mask is None:
            self.out_bound = self.twice * ((float(em.sum()) + rho_sum * wm) / N + 3 * U * (wm / N + case.e1))
        else:
            self.out_bound = self.twice * ((float((mk * em).sum()) + rho_sum * wm) / self.ref_out1 + 4 * U * (wm + case.e1) / self.ref_out1)

    # ---- assertions
    def _ratio(self, got, ref, bound):
        got = got.detach().to("cpu", torch.float64).reshape(ref.shape)
        q = (got - ref).abs() / (bound + FLOOR)
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        return float(q.max()) if q.numel() else 0.0

    def check(self, out=None, loss_map=None, grad_flow=None, what="", factor=1.0, verbose=True):
        """The entry point's outputs (any may be None) against the bounds; wholly-outside pixels exactly."""
        rows, fails = {}, []
        B, C, Hi, Wi, H, W = self.case.dims
        if loss_map is not None:
            lm = loss_map.detach().cpu().reshape(B, H * W)
            rows["loss_map"] = self._ratio(lm, self.ref_map, factor * self.map_bound)
            if not bool((lm[self.outside] == 1).all()):
                fails.append("loss_map != 1 on %d wholly-outside pixels" % int((lm[self.outside] != 1).sum()))
        if grad_flow is not None:
            gf = grad_flow.detach().cpu().reshape(B, 2, H * W)
            rows["grad_flow"] = self._ratio(gf, self.ref_grad.reshape(B, 2, H * W), factor * self.grad_bound.reshape(B, 2, H * W))
            o = self.outside.unsqueeze(1).expand(B, 2, H * W)
            if not bool((gf[o] == 0).all()):
                fails.append("grad_flow != 0 on wholly-outside pixels")
            if self.case.mask is not None:
                z = (self.case.mask == 0).unsqueeze(1).expand(B, 2, H * W)
                if not bool((gf[z] == 0).all()):
                    fails.append("grad_flow != 0 under a zero of the mask")
        if out is not None:
            o = out.detach().cpu().double()
            rows["out0"] = abs(float(o[0]) - self.ref_out0) / (factor * self.out_bound + FLOOR)
            rows["out1"] = abs(float(o[1]) - self.ref_out1) / (factor * self.twice * 2 * self.U * abs(self.ref_out1) + FLOOR)
        return self._finish(rows, fails, what, verbose)

    def check_module(self, loss, flow_grad, what="", factor=1.0, verbose=True):
        """A module-level result: the loss and d(loss)/d(flow) = stored gradient / out[1]."""
        rows = {"loss": abs(float(loss) - self.ref_out0) / (factor * self.out_bound + FLOOR)}
        ref = self.ref_grad / self.ref_out1
        rows["flow.grad"] = self._ratio(flow_grad, ref, factor * (self.grad_bound / self.ref_out1 + self.twice * 2 * self.U * ref.abs()))
        return self._finish(rows, [], what, verbose)

    def _finish(self, rows, fails, what, verbose):
        if verbose:
            print("SCBOUND %s %r: %s" % (what, self.case, " ".join("%s %.3g" % kv for kv in sorted(rows.items()))))
        fails += ["%s: error / bound = %.3g" % kv for kv in sorted(rows.items()) if not kv[1] <= 1.0]
        assert not fails, "%s %r: %s" % (what, self.case, "; ".join(fails))
        return rows


# ------------------------------------------------------------------------------------------------ the matrix
# (B, C, Hi, Wi, H, W): the issue's five, then the sizes at which the host takes another decomposition -- 16 slices of the channels
# for C >= 32 on fewer than 1024 blocks of 64 pixels, else 4 -- and a slice long enough for the four-channel trips
SHAPES = {
    "c3": (2, 3, 9, 6, 5, 7),
    "c64": (2, 64, 16, 16, 16, 16),
    "c70_ragged": (1, 70, 20, 33, 20, 33),
    "c256": (2, 256, 32, 32, 32, 32),
    "c5_f64": (1, 5, 8, 8, 12, 10),
    "c20_trips": (1, 20, 7, 9, 9, 13),
    "c31": (1, 31, 6, 5, 7, 11),
    "c32": (1, 32, 6, 5, 7, 11),
    "c32_1024_blocks": (4, 32, 4, 4, 128, 128),
}
F64 = ("c5_f64",)


def lane_slices(shape):
    """4: 16 channel slices on 16-pixel blocks; 1: 4 slices on 64-pixel blocks (sc_lane_slices of the .hip file)."""
    B, C, Hi, Wi, H, W = shape
    return 4 if (C >= 32 and B * ((H * W + 63) // 64) < 1024) else 1


def cases():
    """(shape name, family, mask): every family and every mask at least once, rotated over the shapes; the large shape once."""
    out = []
    small = [n for n in SHAPES if n != "c32_1024_blocks"]
    for i, name in enumerate(small):
        for j in range(3):
            k = 3 * i + j
            out.append((name, FAMILIES[k % len(FAMILIES)], MASKS[(i + j) % len(MASKS)]))
    out.append(("c32_1024_blocks", "mixed", "binary"))
    return out


def case_id(spec):
    return "-".join(spec)


def build(spec, seed=0):
    name, family, mask_kind = spec
    return make_case(SHAPES[name], family, mask_kind, torch.float64 if name in F64 else torch.float32, seed)
