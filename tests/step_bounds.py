"""Float64 error bounds and exact cases for three kernels of every train step (a plain helper module, not a conftest): the flat Adam
step (csrc/adam.hip), the fused L1 terms (csrc/l1_loss.hip) and the correlation column maximum (csrc/correlation.hip).  The batched
spectral norm has its own module, tests/step_bounds_sn.py, which takes the yardstick (Checks) and the reductions from here.

Conventions of bn_bounds.py: every reference is float64 torch on the CPU, computed from what the kernel is GIVEN; u = 2^-24, u64 =
2^-53; the one SAFETY = 4 multiplies every count of roundings; FLOOR = 1e-38 keeps a bound of exactly zero from dividing; a sum of
terms t_i is bounded by rule (B) of conv_bounds.py, (L + P) u sum |t_i|, L the longest chain of additions of one thread, P the
partials that meet afterwards.  The float64 reference's own sum of n terms errs by at most n u64 sum |t_i| (rule (S): any order);
that term is added wherever a sum is compared, so the same formulas serve a float64 kernel (step_bounds_sn.py).  No constant is fitted.
Conditions are evaluated from the float64 reference alone and raise ValueError.

Flat Adam (ffwm_adam_step, ffwm_adam_step_device).  The kernel receives b1 = float32(beta1), b2 = float32(beta2), e = float32(eps),
step = float32(lr / bc1), s = float32(sqrt(bc2)); 1 - b is exact in fp32 for b in [1/2, 1) (Sterbenz; asserted).  Per element
    m' = m + (g - m)(1 - b1)                     3 roundings:  |dm| <= rho 3 (|m| + (|g| + |m|)(1 - b1)),   rho = SAFETY u
    v' = b2 v + ((1 - b2) g) g                   4 roundings:  |dv| <= rho 4 (b2 |v| + (1 - b2) g^2) + ETA
       ETA = 2^-125: the two products of g underflow below 2^-126 (flushed or denormal: at most 2^-126 each, absolute)
    denom = sqrt(v') / s + e                     sqrt is monotone: |d sqrt| <= max(sqrt(v' + dv) - sqrt(v'), sqrt(v') - sqrt(max(v' - dv,
       0))) + rho sqrt(v' + dv); through the square root ETA becomes at most 2^-62.5 / s, ~1e-19 beside eps = 1e-8: stated, not silent.
       The division counts 3 (an implementation may cast the double sqrt(bc2) to float, take a float reciprocal and multiply: ATen's
       CPU kernels do), the addition 1:  d denom = d sqrt / s + rho (3 sqrt(v') / s + denom)
    p' = p - (step m') / denom                   |dp| <= (step dm + rho 2 step |m'|) / (denom - d denom)                (product, division)
                                                        + step |m'| d denom / (denom (denom - d denom))                 (the conditioning term)
                                                        + rho (|p| + step |m'| / denom)                                 (the subtraction)
  g = 0 with m = v = 0 leaves p bit-unchanged; a NaN g makes exactly its own p, m, v NaN.  The device-state entry computes lr / bc1 and
  sqrt(bc2) with the device's pow, whose accuracy no document states: float32(state[1]), float32(state[2]) must lie within one float32
  ulp of the host's, the reference takes them AS the kernel holds them, and every count above grows by one.

Fused L1 (ffwm_l1_multi).  Forward, per slot: out0 + sum over the problems of the slot of sc sum |x m - y m|, sc = float32(scale).
  A workgroup takes 4096 elements, 16 per thread on both paths (L = 16), 64 lanes + 4 waves meet, then one float atomic per workgroup
  in any order: P = 64 + 4 + (workgroups of all problems that share the slot).  d = fl(fl(x m) - fl(y m)) errs by u (|x m| + |y m|) +
  u |d|, the product with sc by one more:
    |out - ref| <= (rho (L + P + 2) + n u64) (|out0| + sum sc |d|) + rho 2 sum sc (|x m| + |y m|)
  Backward: bit-exact against the float32 restatement fl(fl(fl(g sc) sign(fl(x m) - fl(y m))) m) (the build keeps products and sums
  apart, -ffp-contract=off), and the sign equals the float64 sign wherever |d| > SAFETY 2 u (|x m| + |y m|); l1_inputs() nudges x until
  no element with d != 0 lies inside that margin, and L1Ref raises ValueError if one does (a condition, not a measurement).

Correlation column maximum (ffwm_correlation_colmax).  v_mfma_f32_32x32x2_f32 is a k-ordered chain of C fused multiply-adds:
    |prod_ij - ref_ij| <= (SAFETY C u + C u64) sum_k |s_ik t_kj|;   max is 1-Lipschitz: the bound of out[b, j] is the largest over i.
  Non-finite contract = torch.bmm(...).max(1): a NaN in source row i makes out[b, :] NaN, a NaN in target column j makes out[b, j] NaN
  alone, a column whose products are all -inf gives -inf, other samples keep their bounds.
  Exact family: small integers, at most 4 non-zeros per source row and target column: every product sum is an exact float32.

tests/test_step_bounds_cpu.py: fp32 restatements of each kernel (and torch.optim.Adam) meet every bound with SAFETY = 1 and the exact
families bit for bit; the mutants each miss an assertion.
"""
import math

import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 4.0
FLOOR = 1e-38
GUARD = 16
NAN = float("nan")


def ceil_div(a, b):
    return -(-a // b)


def f32(v):
    """The double nearest-float32 of a Python float: what `(float)v` hands the kernel."""
    return float(torch.tensor(v, dtype=torch.float32))


def require_exact(t, what="", dtype=torch.float32):
    """Prove that every value of the float64 tensor is representable in dtype, or raise."""
    t = t.double()
    if not torch.equal(t.to(dtype).double(), t):
        raise ValueError("%s: exact case not representable (%d values)" % (what, int((t.to(dtype).double() != t).sum())))
    return t


def guarded(t, device="cpu"):
    """A flat copy of t with GUARD NaN cells behind it."""
    out = torch.full((t.numel() + GUARD,), NAN, dtype=t.dtype, device=device)
    out[:t.numel()] = t.reshape(-1).to(device)
    return out


def guarded_nan(n, dtype=torch.float32, device="cpu"):
    return torch.full((n + GUARD,), NAN, dtype=dtype, device=device)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def check_guards(arr, n, what=""):
    tail = arr.detach().cpu()[n:]
    ref = torch.full_like(tail, NAN)
    assert tail.numel() == GUARD and torch.equal(bits(tail), bits(ref)), "%s: a guard cell behind element n - 1 was written: %s" % (what, tail.tolist())


class Checks:
    """Collects the worst error / bound per (stage, family); non-finite exactly where the reference is."""

    def __init__(self, what):
        self.what, self.rows, self.failures = what, {}, []

    def _row(self, stage, family, v):
        self.rows[(stage, family)] = max(self.rows.get((stage, family), 0.0), v)

    def bounded(self, stage, family, got, ref, bound):
        got = got.detach().to("cpu", torch.float64)
        ref = ref.double()
        assert got.shape == ref.shape, (stage, tuple(got.shape), tuple(ref.shape))
        bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
        fin = torch.isfinite(ref)
        same_kind = (torch.isfinite(got) == fin) & (fin | (torch.isnan(got) == torch.isnan(ref))) & (fin | torch.isnan(ref) | (got == ref))
        q = torch.where(fin & torch.isfinite(got), (got - ref).abs() / (bound + FLOOR), torch.zeros_like(ref))
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        worst = float(q.max()) if q.numel() else 0.0
        if not bool(same_kind.all()):
            self.failures.append("%s [%s]: %d values differ in kind (finite / NaN / inf) from the reference" % (stage, family, int((~same_kind).sum())))
            worst = math.inf
        elif worst > 1.0:
            self.failures.append("%s [%s]: error / bound = %.3g at flat index %d" % (stage, family, worst, int(q.reshape(-1).argmax())))
        self._row(stage, family, worst)

    def equal(self, stage, family, got, ref):
        """Bit for bit (NaN = NaN of any payload)."""
        got, ref = got.detach().cpu(), ref.detach().cpu().to(got.dtype)
        assert got.shape == ref.shape, (stage, tuple(got.shape), tuple(ref.shape))
        same = (bits(got) == bits(ref)) | (torch.isnan(got) & torch.isnan(ref))
        self._row(stage, family, 0.0 if bool(same.all()) else math.inf)
        if not bool(same.all()):
            self.failures.append("%s [%s]: not bit-exact: %d values differ, first at flat index %d" % (stage, family, int((~same).sum()), int((~same).reshape(-1).nonzero()[0])))

    def require(self, stage, family, ok, why):
        self._row(stage, family, 0.0 if ok else math.inf)
        if not ok:
            self.failures.append("%s [%s]: %s" % (stage, family, why))

    def finish(self, verbose=True):
        if verbose:
            print("STEPBOUND %s: %s" % (self.what, " ".join("%s/%s %.3g" % (s, f, v) for (s, f), v in sorted(self.rows.items()))))
        assert not self.failures, "%s: %s" % (self.what, "; ".join(self.failures))
        return dict(self.rows)


# ------------------------------------------------------------------------------------------------ the kernels' reductions in torch
def chain_sum(terms, threads):
    """[..., n] -> [..., threads]: thread t adds terms t, t + threads, ... in order, in the terms' dtype."""
    n = terms.shape[-1]
    L = max(ceil_div(n, threads), 1)
    pad = torch.zeros(terms.shape[:-1] + (L * threads - n,), dtype=terms.dtype)
    t = torch.cat([terms, pad], -1).view(terms.shape[:-1] + (L, threads))
    acc = t[..., 0, :].clone()
    for i in range(1, L):
        acc = acc + t[..., i, :]
    return acc


def tree_sum(x):
    """The xor butterfly of wave_sum over the last dimension (a power of two)."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def block_sum(per_thread):
    """[..., 256] -> [...]: wave butterflies, then the four waves in order."""
    w = tree_sum(per_thread.reshape(per_thread.shape[:-1] + (4, 64)))
    acc = w[..., 0]
    for k in range(1, 4):
        acc = acc + w[..., k]
    return acc


# ================================================================================================ flat Adam
ADAM_CONFIGS = {"gan": (2e-4, f32(0.5), f32(0.999), 1e-8), "plain": (1e-3, f32(0.9), f32(0.999), 1e-8)}     # betas representable
ADAM_FAMILIES = ("normal", "zero", "tiny", "huge")
ADAM_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025)
ADAM_BIG = 4096 * 256 * 4 + 1024 + 3          # the grid is capped at 4096 workgroups: a second sweep of 256 float4, and a tail of 3
ADAM_STEPS = (1, 2, 10 ** 6)
ADAM_ETA = 2.0 ** -125
ADAM_MUTANTS = ("bc2_without_sqrt", "eps_inside_sqrt", "beta1_swapped", "tail_skipped", "nan_poisons_float4")


def adam_family_index(n):
    i = torch.arange(n)
    return (i + i // 4) % 4                   # every family meets every float4 position


def adam_inputs(n, seed=0, nan_at=()):
    """-> p, g, m, v (float32) and the family index per element; nan_at: indices whose g is NaN."""
    gen = torch.Generator().manual_seed(9000 + seed + n % 100003)
    fam = adam_family_index(n)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.1
    m = torch.randn(n, generator=gen) * 0.05
    v = torch.rand(n, generator=gen) * 0.01
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    z, t, h = fam == 1, fam == 2, fam == 3
    g = torch.where(z, torch.zeros(n), g)
    m = torch.where(z, torch.zeros(n), m)
    v = torch.where(z, torch.zeros(n), v)
    g = torch.where(t, sign * 2.0 ** -70, g)
    v = torch.where(t & (torch.arange(n) % 8 < 4), torch.zeros(n), v)        # half of the tiny elements start from v = 0
    g = torch.where(h, sign * 2.0 ** 60, g)
    for i in nan_at:
        g[i] = NAN
    return p, g, m, v, fam


def adam_scalars(cfg, step):
    """(b1, b2, e, step_size, bc2_sqrt) as doubles holding the float32 values the kernel receives (host entry point)."""
    lr, beta1, beta2, eps = ADAM_CONFIGS[cfg]
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return f32(beta1), f32(beta2), f32(eps), f32(lr / bc1), f32(math.sqrt(bc2))


class AdamRef:
    def __init__(self, p, g, m, v, scalars, safety=SAFETY, extra=0):
        """extra: roundings added to every count (1 for the device-state entry point)."""
        b1, b2, e, step, s = scalars
        for b in (b1, b2):
            if not 0.5 <= b < 1.0:
                raise ValueError("beta = %r: 1 - beta is not exact in float32" % b)
        p, g, m, v = p.double(), g.double(), m.double(), v.double()
        rho = safety * U32
        self.m = m + (g - m) * (1 - b1)
        self.m_bound = rho * (3 + extra) * (m.abs() + (g.abs() + m.abs()) * (1 - b1))
        self.v = b2 * v + (1 - b2) * g * g
        self.v_bound = rho * (4 + extra) * (b2 * v.abs() + (1 - b2) * g * g) + ADAM_ETA
        root = torch.sqrt(self.v)
        hi = torch.sqrt(self.v + self.v_bound)
        lo = torch.sqrt((self.v - self.v_bound).clamp_min(0))
        d_root = torch.maximum(hi - root, root - lo) + rho * hi
        self.denom = root / s + e
        d_denom = d_root / s + rho * ((3 + extra) * root / s + self.denom)
        low = self.denom - d_denom
        if bool((low[torch.isfinite(low)] <= 0).any()):
            raise ValueError("Adam: the denominator's bound reaches zero")
        upd = step * self.m / self.denom
        self.p = p - upd
        self.p_bound = ((step * self.m_bound + rho * (2 + extra) * step * self.m.abs()) / low
                        + step * self.m.abs() * d_denom / (self.denom * low) + rho * (p.abs() + upd.abs()))
        self.frozen = (g == 0) & (m == 0) & (v == 0)
        self.p_in = p

    def check(self, ck, p, m, v, fam, frozen_p=False):
        """p, m, v: the kernel's arrays (with or without guard cells).  frozen_p: a step size of zero, p bit-unchanged everywhere."""
        n = self.m.numel()
        for name, arr in (("p", p), ("m", m), ("v", v)):
            if arr.numel() > n:
                check_guards(arr, n, ck.what + " " + name)
        p, m, v = p.detach().cpu()[:n], m.detach().cpu()[:n], v.detach().cpu()[:n]
        for k, name in enumerate(ADAM_FAMILIES):
            sel = fam == k
            if not bool(sel.any()):
                continue
            ck.bounded("m", name, m[sel], self.m[sel], self.m_bound[sel])
            ck.bounded("v", name, v[sel], self.v[sel], self.v_bound[sel])
            ck.bounded("p", name, p[sel], self.p[sel], self.p_bound[sel])
        still = torch.isfinite(self.p) if frozen_p else self.frozen
        if bool(still.any()):
            ck.equal("p unchanged", "frozen" if frozen_p else "zero", p[still], self.p_in[still].float())


def adam_emulate(p, g, m, v, scalars, mutant=None):
    """fp32 torch restatement of adam_one over the float4 body and the tail -> p, m, v."""
    b1, b2, e, step, s = (torch.tensor(x, dtype=torch.float32) for x in scalars)
    one = torch.tensor(1.0)
    c1, c2 = (b1, one - b1) if mutant == "beta1_swapped" else (one - b1, b1)
    m2 = m + (g - m) * c1 if mutant != "beta1_swapped" else m * c2 + g * c1            # (1 - b1) m + b1 g
    v2 = b2 * v + (one - b2) * g * g
    if mutant == "eps_inside_sqrt":
        denom = torch.sqrt(v2 + e) / s
    elif mutant == "bc2_without_sqrt":
        denom = torch.sqrt(v2) / (s * s) + e
    else:
        denom = torch.sqrt(v2) / s + e
    p2 = p - step * m2 / denom
    n = p.numel()
    if mutant == "tail_skipped" and n % 4:
        keep = torch.arange(n) >= n - n % 4
        p2, m2, v2 = torch.where(keep, p, p2), torch.where(keep, m, m2), torch.where(keep, v, v2)
    if mutant == "nan_poisons_float4":
        bad = torch.isnan(g)
        idx = torch.arange(n)
        body = idx < n - n % 4
        group = torch.zeros(ceil_div(n, 4) * 4, dtype=torch.bool)
        group[:n] = bad
        group = group.view(-1, 4).any(1, keepdim=True).expand(-1, 4).reshape(-1)[:n] & body
        p2 = torch.where(group, torch.full_like(p2, NAN), p2)
    return p2, m2, v2


def ulp32(x):
    x = torch.tensor(abs(x), dtype=torch.float32)
    return float(torch.nextafter(x, torch.tensor(math.inf)) - x)


# ================================================================================================ fused L1
L1_PER_BLOCK, L1_MAX = 4096, 32
L1_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 2)
L1_COUNTS = (1, 32, 33, 65)
L1_MUTANTS = ("mask_without_broadcast", "problem_33_dropped", "float4_tail_dropped", "scale_twice_backward")


class L1Problem:
    """One term: x, y flat float32 [n]; mask flat or None with (chw, hw); scale; slot; x_off / m_off: floats by which the arrays are
    shifted off 16-byte alignment when they are laid out for the kernel."""

    def __init__(self, x, y, mask=None, chw=1, hw=1, scale=1.0, slot=0, x_off=0, m_off=0, tag="plain"):
        self.x, self.y, self.mask, self.chw, self.hw, self.scale, self.slot = x, y, mask, chw, hw, scale, slot
        self.x_off, self.m_off, self.tag, self.n = x_off, m_off, tag, x.numel()
        if mask is not None and (chw % hw or self.n % chw):
            raise ValueError("mask layout")

    @property
    def vec(self):
        return self.x_off % 4 == 0 and (self.mask is None or (self.hw % 4 == 0 and self.m_off % 4 == 0))

    @property
    def blocks(self):
        return ceil_div(self.n, L1_PER_BLOCK)

    def mask_index(self):
        i = torch.arange(self.n)
        return (i // self.chw) * self.hw + (i % self.chw) % self.hw

    def m_full(self, dtype=torch.float32):
        if self.mask is None:
            return torch.ones(self.n, dtype=dtype)
        return self.mask.to(dtype)[self.mask_index()]


def l1_margin(pr):
    m = pr.m_full(torch.float64)
    xm, ym = pr.x.double() * m, pr.y.double() * m
    return xm - ym, SAFETY * 2 * U32 * (xm.abs() + ym.abs())


def l1_problem(n, seed, mask=None, scale=None, slot=0, x_off=0, m_off=0, tag="plain"):
    """mask: None, or (B, C, HW, full): x is [B, C, HW], the mask [B, 1, HW] or, full, [B, C, HW].  x is nudged off the kink."""
    gen = torch.Generator().manual_seed(5000 + seed)
    x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    if n >= 8:
        y[n // 3] = x[n // 3]                                     # d = 0 exactly, in every arithmetic
    mk, chw, hw = None, 1, 1
    if mask is not None:
        B, C, HW, full = mask
        assert n == B * C * HW
        chw, hw = C * HW, (C * HW if full else HW)
        mk = torch.rand(B * hw, generator=gen) * 1.5 - 0.25      # mostly positive, some negative, some exactly zero
        mk[torch.rand(B * hw, generator=gen) < 0.1] = 0.0
    pr = L1Problem(x, y, mk, chw, hw, f32(0.37 / max(n, 1)) if scale is None else scale, slot, x_off, m_off, tag)
    for _ in range(8):
        d, margin = l1_margin(pr)
        amb = (d != 0) & (d.abs() <= 2 * margin)
        if not bool(amb.any()):
            break
        m = pr.m_full(torch.float64)
        pr.x = torch.where(amb, (pr.x.double() + torch.where(d >= 0, 1.0, -1.0) * 8 * margin / m.abs().clamp_min(1e-30) * torch.sign(m)).float(), pr.x)
    return pr


class L1Ref:
    def __init__(self, problems, n_slots, out0, gout=None, safety=SAFETY):
        """out0 [n_slots] float32: what the result vector holds before the call; gout [n_slots]: the backward's incoming gradient."""
        self.problems, self.n_slots = problems, n_slots
        total = out0.double().clone()
        mag = out0.double().abs()
        cancel = torch.zeros(n_slots, dtype=torch.float64)
        blocks = [0] * n_slots
        terms = [0] * n_slots
        self.sign, self.gx = [], []
        self.gout_sign = None if gout is None else [float(torch.sign(g)) for g in gout]
        for pr in problems:
            d, margin = l1_margin(pr)
            if int(((d != 0) & (d.abs() <= margin)).sum()):
                raise ValueError("L1: %d elements within the two-rounding margin of the kink" % int(((d != 0) & (d.abs() <= margin)).sum()))
            sc = f32(pr.scale)
            total[pr.slot] += sc * d.abs().sum()
            mag[pr.slot] += sc * d.abs().sum()
            cancel[pr.slot] += sc * (margin / (SAFETY * 2 * U32)).sum()
            blocks[pr.slot] += pr.blocks
            terms[pr.slot] += pr.n
            self.sign.append(torch.sign(d))
            if gout is not None:                                   # the float32 restatement of the backward
                m = pr.m_full()
                gs = gout[pr.slot] * torch.tensor(sc, dtype=torch.float32)
                self.gx.append(gs * torch.sign(pr.x * m - pr.y * m) * m)
        self.out = total
        rho = safety * U32
        P = torch.tensor([64 + 4 + b for b in blocks], dtype=torch.float64)
        self.out_bound = (rho * (16 + P + 2) + torch.tensor(terms, dtype=torch.float64) * U64) * mag + rho * 2 * cancel

    def check_forward(self, ck, out, family="forward"):
        if out.numel() > self.n_slots:
            check_guards(out, self.n_slots, ck.what + " out")
        ck.bounded("out", family, out.detach().cpu()[:self.n_slots], self.out, self.out_bound)

    def check_backward(self, ck, gxs):
        """gxs: per problem the kernel's grad_x WITH its guard cells (None for a zero-length problem)."""
        for k, (pr, gx) in enumerate(zip(self.problems, gxs)):
            if pr.n == 0:
                continue
            check_guards(gx, pr.n, "%s gx of problem %d" % (ck.what, k))
            got = gx.detach().cpu()[:pr.n]
            ck.equal("grad_x", pr.tag, got, self.gx[k])
            m = pr.m_full(torch.float64)
            want = math.copysign(1.0, self.gout_sign[pr.slot] * pr.scale) * self.sign[k] * torch.sign(m) if self.gout_sign[pr.slot] else torch.zeros(pr.n, dtype=torch.float64)
            # the float64 sign: every element with d != 0 lies outside the margin (the constructor raised otherwise)
            ck.require("sign", pr.tag, bool((torch.sign(got.double()) == want).all()), "the sign differs from the float64 sign outside the margin")


def _first_of_second_launch(problems):
    """The index of the 33rd non-empty problem (a launch takes 32 non-empty ones), or -1."""
    full = [k for k, pr in enumerate(problems) if pr.n]
    return full[L1_MAX] if len(full) > L1_MAX else -1


def l1_emulate_forward(problems, n_slots, out0, mutant=None):
    """fp32 torch restatement: 4096 elements per workgroup, 16 per thread, wave butterflies, four waves, one atomic per workgroup."""
    out = out0.clone().float()
    for k, pr in enumerate(problems):
        if pr.n == 0 or (mutant == "problem_33_dropped" and k == _first_of_second_launch(problems)):
            continue
        if mutant == "mask_without_broadcast" and pr.mask is not None:
            m = pr.mask[torch.arange(pr.n) % pr.mask.numel()]
        else:
            m = pr.m_full()
        a = (pr.x * m - pr.y * m).abs()
        if mutant == "float4_tail_dropped" and pr.vec:
            a = a[:pr.n - pr.n % 4]
        sc = torch.tensor(pr.scale, dtype=torch.float32)
        pad = torch.cat([a, torch.zeros(pr.blocks * L1_PER_BLOCK - a.numel())]).view(pr.blocks, L1_PER_BLOCK)
        if pr.vec:
            q = pad.view(pr.blocks, 4, 256, 4)
            per = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])              # [blocks, 4, 256]
            acc = per[:, 0]
            for u in range(1, 4):
                acc = acc + per[:, u]
        else:
            acc = chain_sum(pad, 256)
        for s in block_sum(acc):
            out[pr.slot] = out[pr.slot] + s * sc
    return out


def l1_emulate_backward(problems, gout, mutant=None):
    gxs = []
    for k, pr in enumerate(problems):
        gx = guarded_nan(pr.n)
        if pr.n and not (mutant == "problem_33_dropped" and k == _first_of_second_launch(problems)):
            m = pr.mask[torch.arange(pr.n) % pr.mask.numel()] if (mutant == "mask_without_broadcast" and pr.mask is not None) else pr.m_full()
            sc = torch.tensor(pr.scale, dtype=torch.float32)
            gs = gout[pr.slot] * sc
            if mutant == "scale_twice_backward":
                gs = gs * sc
            val = gs * torch.sign(pr.x * m - pr.y * m) * m
            keep = pr.n - pr.n % 4 if (mutant == "float4_tail_dropped" and pr.vec) else pr.n
            gx[:keep] = val[:keep]
        gxs.append(gx)
    return gxs


def l1_cases():
    """name -> (problems, n_slots): the sizes, paths, mask layouts and problem counts of the issue."""
    cases = {}
    for n in L1_SIZES:
        cases["n%d" % n] = ([l1_problem(n, n, tag="float4"), l1_problem(n, n + 1, slot=1, x_off=1, tag="scalar")], 2)
    B, C = 2, 3
    cases["masks"] = ([l1_problem(B * C * 35, 11, mask=(B, C, 35, False), tag="mask_hw35"),
                       l1_problem(B * C * 32, 12, mask=(B, C, 32, False), slot=1, tag="mask_float4"),
                       l1_problem(B * C * 32, 13, mask=(B, C, 32, False), slot=2, m_off=1, tag="mask_misaligned"),
                       l1_problem(B * C * 32, 14, mask=(B, C, 32, True), slot=3, tag="mask_full"),
                       l1_problem(B * C * 2052, 15, mask=(B, C, 2052, False), slot=4, tag="mask_blocks")], 5)
    for count in L1_COUNTS:
        probs = []
        for k in range(count):
            n = (5, 64, 4097, 131)[k % 4]
            mask = (1, 1, 131, False) if n == 131 else None
            probs.append(l1_problem(n, 100 + k, mask=mask, slot=k % 3, x_off=k % 2, tag="count%d" % count))
        if count == 65:                                            # (33 stays 33 non-empty problems: a second launch of one)
            probs[7] = L1Problem(torch.randn(4)[:0], torch.randn(4)[:0], tag="empty")             # zero length in the middle ...
            probs[32] = L1Problem(torch.randn(4)[:0], torch.randn(4)[:0], slot=1, tag="empty")     # ... and at position 32
        cases["count%d" % count] = (probs, 3)
    cases["one_slot40"] = ([l1_problem((4097, 3 * 4096 + 2, 700)[k % 3], 300 + k, tag="one_slot") for k in range(40)], 1)
    return cases


# ================================================================================================ correlation column maximum
CORR_SHAPES = [(1, 1, 64), (2, 31, 64), (1, 32, 128), (2, 33, 64), (1, 127, 256), (1, 128, 64), (3, 129, 128), (2, 160, 256), (1, 160, 64)]
CORR_MUTANTS = ("ragged_tile_dropped", "transposed_readout", "nan_dropped", "floor_3e38")


def corr_inputs(B, N, C, seed=0):
    """Un-normalised source [B, N, C] and target [B, C, N] with a scale per row / column and an asymmetric target."""
    gen = torch.Generator().manual_seed(7700 + seed + 13 * N + C)
    scale = torch.randint(-6, 7, (B, N, 1), generator=gen).float()
    scale[:, 0], scale[:, N - 1] = 6.0, 6.0                      # the first and the last row carry maxima of many columns
    s = torch.randn(B, N, C, generator=gen) * torch.exp2(scale)
    t = (torch.randn(B, C, N, generator=gen) + 0.3) * torch.exp2(torch.randint(-4, 5, (B, 1, N), generator=gen).float())
    return s.contiguous(), t.contiguous()


def corr_exact_inputs(N, C, seed=0):
    """Small integers, <= 4 non-zeros per source row and target column; the arg-max row of one column each is planted at row 0, row N - 1,
    a row with row % 8 in 4..7 and one with row % 8 in 0..3 (the two halves of the MFMA C/D layout), and in the ragged last tile.
    -> s [1, N, C], t [1, C, N], the planted (row, column) pairs."""
    gen = torch.Generator().manual_seed(8800 + seed + N + C)
    s, t = torch.zeros(N, C), torch.zeros(C, N)
    for i in range(N):
        ks = torch.randperm(C, generator=gen)[:4]
        s[i, ks] = torch.randint(-2, 3, (4,), generator=gen).float()
        ks = torch.randperm(C, generator=gen)[:4]
        t[ks, i] = torch.randint(-2, 3, (4,), generator=gen).float()
    rows = sorted({0, N - 1, min(5, N - 1), min(34, N - 1), (N - 1) // 32 * 32, N // 2})
    cols = [(7 * k + N // 3) % N for k in range(len(rows))]
    planted = []
    for i, j in zip(rows, cols):
        if j in [c for _, c in planted]:
            continue
        ks = torch.randperm(C, generator=gen)[:4]
        t[:, j] = 0
        t[ks, j] = torch.tensor([3.0, -3.0, 3.0, 3.0])
        s[i] = 0
        s[i, ks] = torch.tensor([3.0, -3.0, 3.0, 3.0])
        planted.append((i, j))
    s, t = s.unsqueeze(0).contiguous(), t.unsqueeze(0).contiguous()
    prod = torch.bmm(s.double(), t.double())
    require_exact(prod, "correlation exact family")
    for i, j in planted:
        col = prod[0, :, j]
        if int(col.argmax()) != i or int((col == col.max()).sum()) != 1:
            raise ValueError("correlation exact family: the planted row %d is not the only maximum of column %d" % (i, j))
    return s, t, planted


class CorrRef:
    def __init__(self, s, t, safety=SAFETY):
        C = s.shape[2]
        sd, td = s.double(), t.double()
        prod = torch.bmm(sd, td)
        self.out = prod.max(1)[0]
        self.bound = ((safety * C * U32 + C * U64) * torch.bmm(sd.abs(), td.abs())).max(1)[0]
        self.bound = torch.where(torch.isfinite(self.bound), self.bound, torch.zeros_like(self.bound))

    def check(self, ck, out, family="normal", per_sample=None):
        B, N = self.out.shape
        if out.numel() > B * N:
            check_guards(out.reshape(-1), B * N, ck.what + " out")
        got = out.detach().cpu().reshape(-1)[:B * N].view(B, N)
        for b in range(B):
            ck.bounded("colmax", per_sample[b] if per_sample else family, got[b], self.out[b], self.bound[b])


def corr_nonfinite_inputs(N=33, C=64):
    """Sample 0: a NaN in source row 3; sample 1: a NaN in target column 5 and an all -inf column 7; sample 2: untouched."""
    s, t = corr_inputs(3, N, C, seed=5)
    s[0, 3 % N, 10] = NAN
    t[1, 20, 5 % N] = NAN
    s[1, :, 30] = -s[1, :, 30].abs() - 0.125
    t[1, 30, 7 % N] = math.inf
    return s, t


def corr_nonfinite_check(ck, s, t, out):
    N = s.shape[1]
    ref = CorrRef(s, t)
    want_nan = torch.zeros(3, N, dtype=torch.bool)
    want_nan[0] = True
    want_nan[1, 5 % N] = True
    assert torch.equal(torch.isnan(ref.out), want_nan) and float(ref.out[1, 7 % N]) == -math.inf        # the reference itself
    ref.check(ck, out, per_sample=["nan_source_row", "nan_target_column", "untouched"])


def corr_emulate(s, t, mutant=None):
    """The kernel's arithmetic in torch: per product a k-ordered chain of fp32 fused multiply-adds (the float product is exact in
    double; the sum is rounded to float once per step), row tiles of 32, running maxima that keep a NaN."""
    B, N, C = s.shape
    acc = torch.zeros(B, N, N)
    sd, td = s.double(), t.double()
    for k in range(C):
        acc = (acc.double() + sd[:, :, k:k + 1] * td[:, k:k + 1, :]).float()
    rows = N
    if mutant == "ragged_tile_dropped" and N % 32:
        rows = N - N % 32
    if mutant == "transposed_readout":
        acc = acc.transpose(1, 2)
    start = -3.0e38 if mutant in ("floor_3e38", "nan_dropped") else -math.inf
    best = torch.full((B, N), start)
    for i in range(rows):
        a = acc[:, i]
        take = (a > best) if mutant == "nan_dropped" else ((a > best) | torch.isnan(a))
        best = torch.where(take, a, best)
    return best
