"""Per-channel float64 error bounds and exact cases for the fused BatchNorm kernels of csrc/bn_lrelu.hip (a plain helper module,
not a conftest): ffwm_bn_lrelu_forward / _backward and ffwm_bn_res_act_forward / _backward.

Every reference is float64 torch on the CPU, computed from the kernel's ACTUAL inputs; u = 2^-24, u64 = 2^-53; one SAFETY = 4
multiplies every count of roundings, FLOOR = 1e-38 keeps a bound of exactly zero from dividing; no constant here is fitted.

The route (bn_route, restated from bn_slices / bn_launch of the .hip file)
  n = B HW values per channel.  n < 2048: a WAVE per channel (64 threads, 16 channels per 1024-thread workgroup; the sub-groups past
  C are dead: they shadow channel C - 1 and store nothing).  Otherwise a 1024-thread BLOCK per channel.  With a scratch buffer, HW % 4
  == 0 and n >= 2048 a channel is SPLIT into S = min(ceil(1024 / C), n / 16384, 32) slices (S >= 2) of the flat (plane, float4)
  index: ceil(B HW/4 / S) float4 each, the last one shorter.  HW % 4 == 0 takes the float4 path (4 loads in flight forward, 2
  backward, the last round ragged), anything else the scalar path.
  L = the longest chain of additions one thread makes: per element one addition (the float4 path adds a tree of 4 to the running sum:
      4 roundings per 4 elements), so L = the elements of a thread, rounds x unroll x 4 (float4) or B ceil(HW / threads) (scalar);
  P = the partial sums that meet afterwards: 64 lanes, + 16 waves in a block, + S slices (double atomics, any order).
  (B) of conv_bounds.py then bounds a double sum of terms t_i by (L + P) u64 sum |t_i|.

Forward statistics, per channel, in float64: mean, the biased var (two passes), invstd = 1 / sqrt(var + float32(eps)), A = E[x^2],
E|x|.  The kernel sums x and x^2 in double (x^2 is exact in double), so with rho64 = SAFETY (L + P + c) u64, c = 8 (s / n, ss / n,
mean^2, the subtraction, + eps, sqrt, the reciprocal, the reference's own rounding):
    |save_mean - mean|     <= u |mean| + rho64 E|x|                         (the cast to float; the sum)
    |save_invstd - invstd| <= invstd (2 u + 1/2 rho64 A / (var + eps))      (d invstd / invstd = -1/2 d var / (var + eps))
  The 2 u: the cast, and one for an implementation that rounds var to float first (1/2 u) and takes a float rsqrt.  d var: E[x^2]
  errs by (L + P) u64 A; mean^2 by 2 |mean| d mean <= 2 (L + P) u64 |mean| E|x| <= 2 (L + P) u64 A (Cauchy-Schwarz).  The first-order
  worst case is therefore 3 (L + P) u64 A + a few u64 A, which rho64 A covers for every L + P >= 1: for this one assertion most of
  SAFETY is spent on the cancellation of E[x^2] - mean^2, a factor 4/3 is left.  A / (var + eps) = 1 + mean^2 / var is the
  conditioning on |mean| / std: at mean = 256 std it is 65537, and an fp32 accumulation (u instead of u64) misses by ~ 2^29.
  Running statistics: R = (1 - m) old + m new in float64 with the caller's double m, new = mean or the UNBIASED var n / (n - 1)
  (n = 2 gives 2 var).  The kernel evaluates the float expression with mf = float(m): fl(1 - mf), two products, one addition -- 4
  roundings, + 1 for the cast of the unbiased variance -- and |mf - m| is known exactly:
    |run - R| <= SAFETY N u ((1 - m) |old| + m |new|) + |mf - m| (|old| + |new|) + m (bound of new),  N = 4 (mean), 5 (var).
  m = 1 has mf = m and 1 - m = 0 exactly: the old value may not leak at all.

Forward output: pre = gamma (x - mean) invstd + beta (+ res + rbias), mag = |gamma| invstd (|x| + |mean|) + |beta| (+ |res| + |rbias|),
    |y - act(pre)| <= rho mag + post u |ref| + FLOOR,  rho = SAFETY N u.
  N counts, for the kernel's form x sc + sh with sc = fl(gamma invstd_f), sh = fl(beta - fl(fl(mean_f gamma) invstd_f)) (+ rbias):
  invstd_f 2 (above), mean_f 1, gamma invstd 1, the shift 2 (its second product, the subtraction), the final multiply and add 2 (one
  if fused), and 1 for the u64-scale errors of the statistics: N = 9; the residual variant adds rbias and res: N = 11.  The other
  form, fl(fl(x - mean_f) sc) + beta, has mean_f 1, the subtraction 1, sc 3, the product 1, + beta 1 = 7 <= 9.  The "1 for the
  statistics" is a CONDITION, asserted on the CPU from the float64 reference alone (ValueError otherwise): on every element
    |gamma| invstd (rho64 E|x| + 1/2 rho64 A / (var + eps) (|x| + |mean|)) <= u mag.
  LeakyReLU is 1-Lipschitz for slopes in (0, 1] and rounds one product: post = 1.  (The slope enters as float32(slope), as the
  kernel receives it.)
  Sigmoid, 1 / (1 + __expf(-v)), is 1/4-Lipschitz, so the pre-activation's bound enters as rho mag / 4, and its own term is
    SAFETY 2 u |pre| ref (1 - ref)  +  K_SIG u ref.
  The first: __expf(v) = exp2(fl(v fl(log2 e))): the constant and the product err by u each, 2 u |v| log2 e in the exponent, 2 u |v|
  relative in e^-v, and d y = y (1 - y) x that.  The second covers the exponential instruction, 1 + e and the reciprocal.  No
  document available to this project states the accuracy of the hardware exponential, so nothing is claimed for it; as the issue
  prescribes, float32 torch.sigmoid (no __expf) was measured against float64 on the CPU: 2^24 uniform samples x 4 and a 2^24-point
  grid in each of [-87, -20], [-20, -1], [-1, 1], [1, 20], [20, 90], and 2^24 log-spaced |v| in [2^-40, 1] of both signs; the
  worst |sigmoid_f32 - sigmoid_f64| / (u sigmoid_f64) seen was 2.49 (at v = -16.636), SIGMOID_WORST = 2.5, K_SIG = SAFETY x 2.5 = 10.
  Results below 2^-126 are under FLOOR's care.

Backward.  The reference is a function of what the kernel is GIVEN: x, dy, gamma, beta, the float save_mean / save_invstd, and for
the residual variant the forward output y.  xhat = (x - mean_f) invstd_f (the kernel: 2 roundings), xabs = invstd_f (|x| + |mean_f|).
  mask: residual variant y > 0 (no ambiguity).  Plain variant gamma xhat + beta > 0 recomputed in fp32 (xhat 2, the product, the
  addition: rho_pre = SAFETY 4 u), ambiguous within margin = rho_pre (|gamma| xabs + |beta|) of zero.  backward_inputs() nudges x off
  the kink AFTER the statistics are fixed (the entry takes them as inputs) until every |pre| > 2 margin, and BackwardBound asserts
  that the count of elements with |pre| <= margin is exactly zero -- a condition on the CPU, not a measurement.  Deliberate
  exception: channels with gamma = 0, beta = 0 have pre = 0 in every arithmetic; their mask is the slope branch (`> 0`, as ATen).
  In the exact family pre is a small integer in every arithmetic, zeros included, and the condition is not needed.
  g = dy (mask) or fl(dy slope): the float product is what every fp32 implementation holds (dy slope has 48 bits, float64 rounds it
  once), so the reference takes g AS that float: d(res) = g is exact for LeakyReLU (torch.equal).  Sigmoid: g = dy y (1 - y), 3
  roundings (NG = 3, else 0): |d(res) - g| <= SAFETY 3 u |g|.
  rho64b = SAFETY (L_bwd + P + 2) u64 (the sum, s / n, the reference):
    d(beta)  = sum g:      u |ref| + (rho64b + SAFETY NG u) sum |g|
    d(gamma) = sum g xhat: u |ref| + (SAFETY (2 + NG) u + rho64b) sum |g| xabs         (xhat: 2; the product is exact in double)
    dx = gamma invstd_f (g - mean(g) - xhat mean(g xhat)), mag the same expression on absolute values (xabs for |xhat|):
         rho_dx = SAFETY (9 + NG) u + rho64b.  The longest path is the last term: xhat 2, mean(g xhat) 3 (its float cast, the 2 of
         xhat inside the sum), their product 1, the subtraction 1, gamma invstd 1, the final product 1 = 9; mean(g): 5; g: 4.

Non-finite inputs: a channel holding a NaN or an inf is non-finite where the reference is; every other channel keeps its bounds.

Input families, mixed ACROSS the channels of one tensor (channel c has FAMILIES[(c + rot) % 5]): `normal` 0.7 +- 2; `offset` mean
= +-256 std; `tiny_std` std 1e-3 (var < eps); `constant` -3.25 or float32(0.7) (var = 0); `huge` scale 2^60 (squares overflow fp32,
not double).  gamma positive, negative and zero by (c + 2 rot) % 3, half of the zero-gamma channels with beta = 0; grad_output
scaled by 2^-8 .. 2^8 per channel.

Exact family: x = +-1 balanced per channel (n even), eps = 0 (mean 0, var 1, invstd 1), gamma, beta, res, rbias, dy small integers,
slope 0.25 or 0.5, momentum 0.5 or 1 on integer running statistics.  require_exact proves that a float64 value is representable in
float32 or raises; then the assertion is torch.equal.  (The unbiased variance n / (n - 1) is rounded once, from the same double
expression, on both sides.)  dx is exact when mean(g) and mean(g xhat) are dyadic: n a power of two.

The fp32 stand-ins of tests/test_bn_bounds_cpu.py (ATen's CPU kernels and emulate_forward / emulate_backward below, the kernel's
arithmetic restated in torch) meet every bound with SAFETY = 1 and the exact family exactly; the mutants of the same restatement
each miss one.
"""
import math

import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 4.0
FLOOR = 1e-38
C64 = 8                      # roundings around the double sums of the forward statistics (docstring)
C64B = 2                     # ... of the backward sums
SIGMOID_WORST = 2.5          # measured, see the docstring
GUARD = 16                   # NaN cells behind the C entries of every per-channel array
FAMILIES = ("normal", "offset", "tiny_std", "constant", "huge")
WAVE, BLOCK_THREADS = 64, 1024


def _ceil_div(a, b):
    return -(-a // b)


def f32(v):
    """The double nearest-float32 of a Python float: what `(float)v` hands the kernel."""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ the route
def bn_slices(B, C, HW, scratch):
    if not scratch or HW % 4 != 0 or B * HW < 2048:
        return 1
    S = min(_ceil_div(1024, C), B * HW // 16384, 32)
    return 1 if S < 2 else S


class Route:
    """kind wave / block / split, threads per channel, S, float4 path or not, the slices' [first4, total4) ranges, dead sub-groups,
    and the (L, P) of the forward and backward sums."""

    def __init__(self, B, C, HW, scratch):
        n = B * HW
        self.B, self.C, self.HW, self.n = B, C, HW, n
        self.S = bn_slices(B, C, HW, scratch)
        self.threads = BLOCK_THREADS if n >= 2048 else WAVE
        per_block = BLOCK_THREADS // self.threads
        self.blocks = _ceil_div(C, per_block)
        self.dead = self.blocks * per_block - C
        self.kind = "split" if self.S > 1 else ("block" if self.threads == BLOCK_THREADS else "wave")
        self.vec = HW % 4 == 0
        self.hw4 = HW // 4 if self.vec else 0
        self.all4 = B * self.hw4
        chunk = _ceil_div(self.all4, self.S) if self.vec else 0
        self.slices = [(i * chunk, min(self.all4, (i + 1) * chunk)) for i in range(self.S)]
        if self.vec:
            longest = max(t - f for f, t in self.slices)
            self.L_fwd = 16 * _ceil_div(longest, 4 * self.threads)
            self.L_bwd = 8 * _ceil_div(longest, 2 * self.threads)
        else:
            self.L_fwd = self.L_bwd = B * _ceil_div(HW, self.threads)
        self.P = WAVE + (BLOCK_THREADS // WAVE if self.threads == BLOCK_THREADS else 0) + (self.S if self.S > 1 else 0)

    @property
    def path(self):
        return "float4" if self.vec else "scalar"

    def __repr__(self):
        return "%s/%s S=%d L=%d/%d P=%d dead=%d" % (self.kind, self.path, self.S, self.L_fwd, self.L_bwd, self.P, self.dead)


def bn_route(B, C, HW, scratch):
    return Route(B, C, HW, bool(scratch))


def scratch_doubles(C):
    """2 C sums + C 32-bit arrival counters, in doubles."""
    return 2 * C + (C + 1) // 2


# ------------------------------------------------------------------------------------------------ inputs
class Case:
    """One call's inputs (float32 CPU tensors; None = a NULL pointer) and scalars."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def shape(self):
        return tuple(self.x.shape)

    def family(self, c):
        return self.families[c]


# (slope, momentum, running statistics given, affine)
CONFIGS = {"a": (0.2, 0.1, True, True), "b": (0.25, 1.0, True, True), "c": (0.2, 0.1, False, False)}


def rotations(C):
    """Family rotations that show every family to a tensor of C channels."""
    return list(range(0, 5, C)) if C < 5 else [0]


def make_case(shape, res=False, act=0, cfg="a", rot=0, nonfinite=False, seed=0, huge_exp=60):
    B, C, H, W = shape
    slope, momentum, running, affine = CONFIGS[cfg]
    gen = torch.Generator().manual_seed(1000 * seed + 31 * rot + C + H * W)
    x = torch.randn(shape, generator=gen)
    families = []
    for c in range(C):
        fam = FAMILIES[(c + rot) % 5]
        families.append(fam)
        v = x[:, c]
        if fam == "normal":
            v = v * 2 + 0.7
        elif fam == "offset":
            v = v * 0.5 + (128.0 if (c // 5) % 2 == 0 else -128.0)
        elif fam == "tiny_std":
            v = v * 1e-3 + 0.3
        elif fam == "constant":
            v = torch.full_like(v, -3.25 if (c // 5) % 2 == 0 else 0.7)
        elif fam == "huge":
            v = (v + 0.5) * 2.0 ** huge_exp
        x[:, c] = v
    sel = (torch.arange(C) + 2 * rot) % 3
    gamma = (0.5 + torch.randn(C, generator=gen).abs()) * torch.tensor([1.0, -1.0, 0.0])[sel]
    beta = torch.randn(C, generator=gen) * 0.5
    beta[(sel == 2) & ((torch.arange(C) // 3) % 2 == 0)] = 0.0
    case = Case(x=x.contiguous(), gamma=gamma if affine else None, beta=beta if affine else None,
                run_mean=torch.randn(C, generator=gen) if running else None,
                run_var=(torch.rand(C, generator=gen) + 0.5) if running else None,
                res=torch.randn(shape, generator=gen) if res else None, rbias=torch.randn(C, generator=gen) if res else None,
                eps=1e-5, momentum=momentum, slope=slope, act=act, variant="res" if res else "plain", families=families,
                exact=False, nonfinite=[], cfg=cfg, rot=rot)
    if nonfinite:
        assert C >= 2
        case.x[B - 1, 0, H // 2, W - 1] = float("nan")
        case.nonfinite.append(0)
        if C >= 3:
            case.x[0, C - 1, 0, W // 2] = float("inf")
            case.nonfinite.append(C - 1)
    return case


def make_exact_case(shape, res=False, slope=0.25, momentum=0.5, seed=0):
    B, C, H, W = shape
    n = B * H * W
    if n % 2:
        raise ValueError("exact family: %d values per channel cannot be balanced" % n)
    gen = torch.Generator().manual_seed(7000 + seed + C + n)
    half = torch.cat([torch.ones(n // 2), -torch.ones(n // 2)])
    x = torch.empty(C, B, H * W)
    for c in range(C):
        x[c] = half[torch.randperm(n, generator=gen)].view(B, H * W)
    x = x.permute(1, 0, 2).reshape(shape).contiguous()

    def ints(lo, hi, *size):
        return torch.randint(lo, hi + 1, size, generator=gen).float()
    gamma = ints(-2, 3, C)
    if C >= 3:
        gamma[C // 2] = 0.0
    return Case(x=x, gamma=gamma, beta=ints(-2, 2, C), run_mean=ints(-3, 3, C) * 2, run_var=ints(1, 4, C) * 2,
                res=ints(-2, 2, *shape) if res else None, rbias=ints(-2, 2, C) if res else None, eps=0.0, momentum=momentum,
                slope=slope, act=0, variant="res" if res else "plain", families=["exact"] * C, exact=True, nonfinite=[], cfg="exact", rot=0)


def require_exact(t, what=""):
    """Prove that every value of the float64 tensor is a float32, or raise."""
    t = t.double()
    if not torch.equal(t.float().double(), t):
        bad = int((t.float().double() != t).sum())
        raise ValueError("%s: exact case not representable in float32 (%d values)" % (what, bad))
    return t


def guarded(C, fill=float("nan"), device="cpu"):
    """A per-channel output array with its GUARD cells, NaN-filled."""
    return torch.full((C + GUARD,), fill, dtype=torch.float32, device=device)


def check_guards(arr, C, what=""):
    tail = arr.detach().cpu()[C:]
    assert tail.numel() == GUARD and bool(torch.isnan(tail).all()), "%s: a guard cell behind channel C - 1 was written: %s" % (what, tail.tolist())


def _ch(t):
    return t.view(1, -1, 1, 1)


def _per_channel_max(q):
    return q if q.dim() == 1 else q.amax((0, 2, 3))


# ------------------------------------------------------------------------------------------------ the yardstick
class _Checks:
    """Collects error / bound per quantity and channel; non-finite exactly where the reference is."""

    def __init__(self, case, what):
        self.case, self.what, self.rows, self.failures = case, what, {}, []

    def bounded(self, name, got, ref, bound):
        got = got.detach().to("cpu", torch.float64)
        assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
        fin = torch.isfinite(ref)
        wrong = int((torch.isfinite(got) != fin).sum())
        q = torch.where(fin, (got - ref).abs() / (bound + FLOOR), torch.zeros_like(ref))
        q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
        pc = _per_channel_max(q)
        self.rows[name] = pc
        if wrong:
            self.failures.append("%s: %d values non-finite where the reference is finite, or the other way round" % (name, wrong))
        if pc.numel() and float(pc.max()) > 1.0:
            c = int(pc.argmax())
            self.failures.append("%s: error / bound = %.3g in channel %d (%s)" % (name, float(pc.max()), c, self.case.family(c)))

    def equal(self, name, got, ref64):
        got = got.detach().cpu()
        ref = ref64.float()
        same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
        self.rows[name] = _per_channel_max(torch.where(same, 0.0, math.inf).double())
        if not bool(same.all()):
            bad = (~same).nonzero()
            self.failures.append("%s: not bit-exact: %d values differ, first at %s" % (name, bad.shape[0], tuple(int(i) for i in bad[0])))

    def by_family(self):
        out = {}
        for name, pc in self.rows.items():
            for c in range(pc.numel()):
                f = self.case.family(c)
                out[f] = max(out.get(f, 0.0), float(pc[c]))
        return out

    def finish(self, verbose=True):
        fam = self.by_family()
        if verbose:
            print("BNBOUND %s: %s" % (self.what, " ".join("%s %.3g" % (k, v) for k, v in sorted(fam.items()))))
        assert not self.failures, "%s: %s" % (self.what, "; ".join(self.failures))
        return fam


def _sigmoid_term(pre, ref, safety):
    return safety * 2 * U32 * pre.abs() * ref * (1 - ref) + safety * SIGMOID_WORST * U32 * ref


class ForwardBound:
    def __init__(self, case, route, safety=SAFETY, what=""):
        self.case, self.route, self.safety = case, route, safety
        self.what = what or "%s fwd %s %s" % (case.variant, case.shape, route)
        x = case.x.double()
        B, C, H, W = x.shape
        n = B * H * W
        self.n = n
        mean = x.mean((0, 2, 3))
        var = ((x - _ch(mean)) ** 2).mean((0, 2, 3))
        eps = f32(case.eps)
        invstd = 1.0 / torch.sqrt(var + eps)
        A, E1 = (x * x).mean((0, 2, 3)), x.abs().mean((0, 2, 3))
        self.mean, self.var, self.invstd, self.A, self.E1 = mean, var, invstd, A, E1
        rho64 = safety * (route.L_fwd + route.P + C64) * U64
        self.mean_bound = U32 * mean.abs() + rho64 * E1
        self.invstd_bound = invstd * (2 * U32 + 0.5 * rho64 * A / (var + eps))
        if case.exact:
            for t, w in ((mean, "mean"), (invstd, "invstd")):
                require_exact(t, self.what + " " + w)
        # running statistics
        self.unbiased = var * n / (n - 1) if n > 1 else var
        if case.run_mean is not None:
            m, mf = case.momentum, f32(case.momentum)
            dm = abs(mf - m)
            om, ov = case.run_mean.double(), case.run_var.double()
            self.run_mean = (1 - m) * om + m * mean
            self.run_var = (1 - m) * ov + m * self.unbiased
            self.run_mean_bound = safety * 4 * U32 * (abs(1 - m) * om.abs() + m * mean.abs()) + dm * (om.abs() + mean.abs()) + m * self.mean_bound
            self.run_var_bound = (safety * 5 * U32 * (abs(1 - m) * ov.abs() + m * self.unbiased) + dm * (ov.abs() + self.unbiased)
                                  + m * rho64 * A * (n / (n - 1.0) if n > 1 else 1.0))
            if case.exact:
                require_exact(self.run_mean, self.what + " running_mean")
        # output
        g = case.gamma.double() if case.gamma is not None else torch.ones(C, dtype=torch.float64)
        b = case.beta.double() if case.beta is not None else torch.zeros(C, dtype=torch.float64)
        pre = _ch(g) * (x - _ch(mean)) * _ch(invstd) + _ch(b)
        mag = _ch(g.abs() * invstd) * (x.abs() + _ch(mean.abs())) + _ch(b.abs())
        nround = 9
        if case.res is not None:
            pre = pre + case.res.double()
            mag = mag + case.res.double().abs()
            if case.rbias is not None:
                pre = pre + _ch(case.rbias.double())
                mag = mag + _ch(case.rbias.double().abs())
            nround = 11
        rho64_full = SAFETY * (route.L_fwd + route.P + C64) * U64
        cond = _ch(g.abs() * invstd) * (_ch(rho64_full * E1) + _ch(0.5 * rho64_full * A / (var + eps)) * (x.abs() + _ch(mean.abs())))
        fin = torch.isfinite(pre)
        if bool((cond[fin] > U32 * mag[fin]).any()):
            raise ValueError("%s: the double statistics' own error exceeds one float rounding of the output: inputs too ill-conditioned" % self.what)
        self.pre, self.mag = pre, mag
        slope = f32(case.slope)
        if case.act == 1:
            self.ref = torch.sigmoid(pre)
            self.y_bound = 0.25 * safety * nround * U32 * mag + _sigmoid_term(pre, self.ref, safety)
        else:
            self.ref = torch.where(pre > 0, pre, pre * slope)
            self.y_bound = safety * nround * U32 * mag + U32 * self.ref.abs()
        if case.exact:
            require_exact(self.ref, self.what + " y")

    def check(self, y, save_mean, save_invstd, run_mean=None, run_var=None, verbose=True):
        """save_* / run_*: the arrays WITH their guard cells when longer than C."""
        C = self.case.x.shape[1]
        ck = _Checks(self.case, self.what)
        arrays = [("save_mean", save_mean, self.mean, self.mean_bound), ("save_invstd", save_invstd, self.invstd, self.invstd_bound)]
        if self.case.run_mean is not None:
            arrays += [("running_mean", run_mean, self.run_mean, self.run_mean_bound), ("running_var", run_var, self.run_var, self.run_var_bound)]
        for name, got, ref, bound in arrays:
            if got.numel() > C:
                check_guards(got, C, self.what + " " + name)
            if self.case.exact:
                ck.equal(name, got[:C], ref)
            else:
                ck.bounded(name, got[:C], ref, bound)
        if self.case.exact:
            ck.equal("y", y, self.ref)
        else:
            ck.bounded("y", y, self.ref, self.y_bound)
        return ck.finish(verbose)


# ------------------------------------------------------------------------------------------------ backward
def _pre_margin(x, gamma, beta, mean_f, invstd_f):
    C = x.shape[1]
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    xd = x.double()
    xhat = (xd - _ch(mean_f.double())) * _ch(invstd_f.double())
    xabs = _ch(invstd_f.double()) * (xd.abs() + _ch(mean_f.double().abs()))
    pre = _ch(g) * xhat + _ch(b)
    margin = SAFETY * 4 * U32 * (_ch(g.abs()) * xabs + _ch(b.abs()))
    free = _ch((g == 0) & (b == 0)).expand_as(pre)
    return g, b, xhat, xabs, pre, margin, free


def ambiguous(x, gamma, beta, mean_f, invstd_f, factor=1.0):
    """The elements whose fp32 mask could go either way: |pre| <= factor margin, outside the gamma = beta = 0 channels."""
    g, b, xhat, xabs, pre, margin, free = _pre_margin(x, gamma, beta, mean_f, invstd_f)
    return torch.isfinite(pre) & ~free & (pre.abs() <= factor * margin)


def backward_inputs(case, save_mean, save_invstd, y=None, seed=0):
    """-> a Case for the backward entry: x nudged off the kink of the plain variant (the statistics stay), grad_output, y."""
    B, C, H, W = case.shape
    gen = torch.Generator().manual_seed(4242 + seed + C + H * W)
    mean_f, invstd_f = save_mean.detach().cpu().float()[:C].clone(), save_invstd.detach().cpu().float()[:C].clone()
    x = case.x.clone()
    if case.exact:
        dy = torch.randint(-1, 2, case.shape, generator=gen).float()
    else:
        dy = torch.randn(case.shape, generator=gen) * _ch(torch.exp2(((torch.arange(C) * 5) % 17 - 8).float()))
        if case.variant == "plain":
            for _ in range(8):
                g, b, xhat, xabs, pre, margin, free = _pre_margin(x, case.gamma, case.beta, mean_f, invstd_f)
                amb = torch.isfinite(pre) & ~free & (pre.abs() <= 2 * margin)
                if not bool(amb.any()):
                    break
                step = 8 * margin / _ch(g.abs() * invstd_f.double()).expand_as(pre)       # (gamma = 0: never ambiguous, margin < |beta|)
                away = torch.where(pre >= 0, 1.0, -1.0) * torch.sign(_ch(g)).expand_as(pre)
                x = torch.where(amb, (x.double() + away * step).float(), x)
    bc = Case(**case.__dict__)
    bc.x, bc.dy, bc.save_mean, bc.save_invstd = x.contiguous(), dy.contiguous(), mean_f, invstd_f
    bc.y = None if y is None else y.detach().cpu().float().clone()
    return bc


class BackwardBound:
    def __init__(self, bc, route, safety=SAFETY, what="", float_sums=False):
        """float_sums: for a stand-in that adds d(beta) / d(gamma) in fp32 (ATen on the CPU does), (S) of conv_bounds.py: n terms in
        any order, n u sum |t|, added to those two bounds.  Never for the kernels: they sum in double."""
        self.case, self.route, self.safety = bc, route, safety
        self.what = what or "%s bwd %s %s" % (bc.variant, bc.shape, route)
        B, C, H, W = bc.shape
        n = B * H * W
        g, b, xhat, xabs, pre, margin, free = _pre_margin(bc.x, bc.gamma, bc.beta if bc.variant == "plain" else None, bc.save_mean, bc.save_invstd)
        slope = f32(bc.slope)
        dy = bc.dy.double()
        ng = 0
        if bc.variant == "plain":
            if not bc.exact:
                self.ambiguous = int(ambiguous(bc.x, bc.gamma, bc.beta, bc.save_mean, bc.save_invstd).sum())
                assert self.ambiguous == 0, "%s: %d elements within the fp32 margin of the activation's kink" % (self.what, self.ambiguous)
            gv = torch.where(pre > 0, dy, (dy * slope).float().double())
        elif bc.act == 1:
            yd = bc.y.double()
            gv = dy * yd * (1 - yd)
            ng = 3
        else:
            gv = torch.where(bc.y.double() > 0, dy, (dy * slope).float().double())
        self.g = gv
        rho64b = safety * (route.L_bwd + route.P + C64B) * U64
        sg = gv.abs().sum((0, 2, 3))
        self.dbeta = gv.sum((0, 2, 3))
        rho_s = safety * n * U32 if float_sums else 0.0
        self.dbeta_bound = U32 * self.dbeta.abs() + (rho64b + safety * ng * U32 + rho_s) * sg
        self.dgamma = (gv * xhat).sum((0, 2, 3))
        self.dgamma_bound = U32 * self.dgamma.abs() + (safety * (2 + ng) * U32 + rho64b + rho_s) * (gv.abs() * xabs).sum((0, 2, 3))
        k = _ch(g * bc.save_invstd.double())
        mg, mgx = _ch(self.dbeta / n), _ch(self.dgamma / n)
        self.dx = k * (gv - mg - xhat * mgx)
        self.dx_mag = k.abs() * (gv.abs() + _ch(sg / n) + xabs * _ch((gv.abs() * xabs).sum((0, 2, 3)) / n))
        self.dx_bound = (safety * (9 + ng) * U32 + rho64b) * self.dx_mag
        self.dres_bound = safety * 3 * U32 * gv.abs()
        self.ng = ng
        if bc.exact:
            for t, w in ((gv, "g"), (self.dbeta, "d(beta)"), (self.dgamma, "d(gamma)")):
                require_exact(t, self.what + " " + w)

    def require_exact_dx(self):
        """mean(g), mean(g xhat), and every step of dx representable: n a power of two and small integers."""
        n = self.case.x.numel() // self.case.x.shape[1]
        bc = self.case
        g = bc.gamma.double() if bc.gamma is not None else torch.ones(bc.x.shape[1], dtype=torch.float64)
        xhat = (bc.x.double() - _ch(bc.save_mean.double())) * _ch(bc.save_invstd.double())
        mg, mgx = _ch(self.dbeta / n), _ch(self.dgamma / n)
        k = _ch(g * bc.save_invstd.double())
        for t, w in ((mg, "mean(g)"), (mgx, "mean(g xhat)"), (self.g - mg, "g - mean(g)"), (xhat * mgx, "xhat mean(g xhat)"),
                     (self.g - mg - xhat * mgx, "the bracket"), (k, "gamma invstd"), (self.dx, "dx")):
            require_exact(t, self.what + " " + w)

    def check(self, dx, dgamma, dbeta, dres=None, exact_dx=False, verbose=True):
        C = self.case.x.shape[1]
        ck = _Checks(self.case, self.what)
        for name, got, ref, bound in (("d(gamma)", dgamma, self.dgamma, self.dgamma_bound), ("d(beta)", dbeta, self.dbeta, self.dbeta_bound)):
            if got is None:
                continue
            if got.numel() > C:
                check_guards(got, C, self.what + " " + name)
            if self.case.exact:
                ck.equal(name, got[:C], ref)
            else:
                ck.bounded(name, got[:C], ref, bound)
        if dx is not None:
            if self.case.exact and exact_dx:
                self.require_exact_dx()
                ck.equal("dx", dx, self.dx)
            else:
                ck.bounded("dx", dx, self.dx, self.dx_bound)
        if dres is not None:
            if self.ng == 0:
                ck.equal("d(res)", dres, self.g)
            else:
                ck.bounded("d(res)", dres, self.g, self.dres_bound)
        return ck.finish(verbose)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in torch
MUTANTS = ("fp32_variance", "first_slice_only", "ragged_group_skipped", "biased_running_var", "rbias_dropped", "mask_from_x",
           "uncentred_dgamma", "dead_subgroup_store")


def _channel_major(t, route):
    """[B, C, H, W] -> [C, n] in the order of the flat (plane, float4) index."""
    B, C = t.shape[:2]
    return t.permute(1, 0, 2, 3).reshape(C, B * route.HW)


def _kept(route):
    """ragged_group_skipped: the element mask [n] that loses the last, partial row of `threads` float4 of every slice."""
    keep = torch.ones(route.n, dtype=torch.bool)
    if route.vec:
        for f, t in route.slices:
            r = (t - f) % route.threads
            if r:
                keep[4 * (t - r):4 * t] = False
    return keep


def emulate_forward(case, route, mutant=None):
    """fp32 torch restatement of bn_lrelu_fwd_kernel: double sums, E[x^2] - mean^2, float sc / sh, y = act(x sc + sh (+ res)).
    -> y, save_mean, save_invstd, run_mean, run_var (per-channel arrays with NaN guard cells)."""
    x = case.x
    B, C, H, W = x.shape
    n = float(B * H * W)
    xc = _channel_major(x, route)
    keep = _kept(route) if mutant == "ragged_group_skipped" else torch.ones(route.n, dtype=torch.bool)
    if mutant == "first_slice_only" and route.S > 1:
        keep = torch.zeros(route.n, dtype=torch.bool)
        keep[4 * route.slices[0][0]:4 * route.slices[0][1]] = True
    xs = xc[:, keep]
    if mutant == "fp32_variance":
        mean32 = xs.sum(1) / torch.tensor(n, dtype=torch.float32)
        var = ((xs * xs).sum(1) / torch.tensor(n, dtype=torch.float32) - mean32 * mean32).double()
        mean = mean32.double()
    else:
        xd = xs.double()
        mean = xd.sum(1) / n
        var = (xd * xd).sum(1) / n - mean * mean
    var = torch.where((var > 0) | torch.isnan(var), var, torch.zeros_like(var))
    invstd = (1.0 / torch.sqrt(var + f32(case.eps))).float()
    meanf = mean.float()
    save_mean, save_invstd = guarded(C), guarded(C)
    save_mean[:C], save_invstd[:C] = meanf, invstd
    run_mean = run_var = None
    if case.run_mean is not None:
        m = torch.tensor(case.momentum, dtype=torch.float32)
        unb = var if (mutant == "biased_running_var" or n <= 1) else var * n / (n - 1)
        run_mean, run_var = guarded(C), guarded(C)
        run_mean[:C] = (1 - m) * case.run_mean + m * meanf
        run_var[:C] = (1 - m) * case.run_var + m * unb.float()
    if mutant == "dead_subgroup_store" and route.dead:
        save_mean[C], save_invstd[C] = meanf[C - 1], invstd[C - 1]
    ga = case.gamma if case.gamma is not None else torch.ones(C)
    be = case.beta if case.beta is not None else torch.zeros(C)
    sc = ga * invstd
    sh = be - meanf * ga * invstd
    if case.res is not None and case.rbias is not None and mutant != "rbias_dropped":
        sh = sh + case.rbias
    v = x * _ch(sc) + _ch(sh)
    if case.res is not None:
        v = v + case.res
    slope = torch.tensor(case.slope, dtype=torch.float32)
    y = 1.0 / (1.0 + torch.exp(-v)) if case.act == 1 else torch.where(v > 0, v, v * slope)
    if mutant == "ragged_group_skipped":
        yc = _channel_major(y, route).clone()
        yc[:, ~keep] = math.nan                                   # never written
        y = yc.view(C, B, H, W).permute(1, 0, 2, 3).contiguous()
    return y, save_mean, save_invstd, run_mean, run_var


def emulate_backward(bc, route, mutant=None):
    """fp32 torch restatement of bn_lrelu_bwd_kernel -> dx, dgamma, dbeta (guarded), dres (residual variant)."""
    x, dy = bc.x, bc.dy
    B, C, H, W = x.shape
    n = float(B * H * W)
    mean, invstd = bc.save_mean, bc.save_invstd
    ga = bc.gamma if bc.gamma is not None else torch.ones(C)
    be = bc.beta if (bc.beta is not None and bc.variant == "plain") else torch.zeros(C)
    slope = torch.tensor(bc.slope, dtype=torch.float32)
    xh = (x - _ch(mean)) * _ch(invstd)
    if bc.variant == "plain":
        mask = (x > 0) if mutant == "mask_from_x" else ((_ch(ga) * xh + _ch(be)) > 0)
        gv = torch.where(mask, dy, dy * slope)
    elif bc.act == 1:
        gv = dy * (bc.y * (1.0 - bc.y))
    else:
        gv = torch.where(bc.y > 0, dy, dy * slope)
    s = gv.double().sum((0, 2, 3))
    xs = (x * _ch(invstd)) if mutant == "uncentred_dgamma" else xh
    sx = (gv.double() * xs.double()).sum((0, 2, 3))
    dgamma, dbeta = guarded(C), guarded(C)
    dgamma[:C], dbeta[:C] = sx.float(), s.float()
    mg, mgx = (s / n).float(), (sx / n).float()
    k = ga * invstd
    dx = _ch(k) * (gv - _ch(mg) - xh * _ch(mgx))
    return dx, dgamma, dbeta, (gv if bc.variant == "res" else None)


# ------------------------------------------------------------------------------------------------ the matrix
# name: ((B, C, H, W), scratch given, the route it must take)
SHAPES = {
    "wave_scalar_dead11": ((3, 37, 5, 7), False, "wave"),
    "wave_few_float4": ((2, 16, 4, 4), False, "wave"),
    "wave_n2": ((1, 1, 1, 2), False, "wave"),
    "wave_rounds_ragged": ((1, 5, 1, 2044), False, "wave"),
    "wave_1030": ((8, 1030, 2, 2), False, "wave"),
    "block_2048": ((1, 3, 32, 64), False, "block"),
    "block_scalar": ((3, 2, 33, 31), False, "block"),
    "block_ragged1": ((2, 5, 40, 52), False, "block"),
    "block_ragged2": ((5, 2, 64, 68), False, "block"),
    "split_s2": ((2, 3, 128, 128), True, "split"),
    "split_s3": ((3, 2, 128, 128), True, "split"),
    "split_mid_plane": ((3, 4, 108, 104), True, "split"),
    "split_odd_float4": ((1, 2, 12, 2731), True, "split"),
    "split_s32": ((2, 1, 512, 512), True, "split"),
    "scratch_block_scalar": ((3, 2, 33, 31), True, "block"),
    "scratch_wave": ((2, 16, 4, 4), True, "wave"),
}
VARIANTS = {"plain": (False, 0), "res_lrelu": (True, 0), "res_sigmoid": (True, 1)}


def route_of(name):
    (B, C, H, W), scratch, kind = SHAPES[name]
    r = bn_route(B, C, H * W, scratch)
    assert r.kind == kind, (name, r)
    return r


def mixed_cases():
    """(shape name, variant, cfg, rot, nonfinite): every shape x variant x configuration; every family rotation with configuration a,
    one rotation (cycling) with b and c; a NaN / inf channel with configuration a wherever there is a second channel."""
    out = []
    for i, (name, (shape, _, _)) in enumerate(SHAPES.items()):
        rots = rotations(shape[1])
        for variant in VARIANTS:
            out += [(name, variant, "a", r, False) for r in rots]
            out += [(name, variant, "b", rots[i % len(rots)], False), (name, variant, "c", rots[(i + 1) % len(rots)], False)]
            if shape[1] >= 2:
                out.append((name, variant, "a", 0, True))
    return out


def exact_cases():
    """(shape name, variant, slope, momentum, dx exact): the shapes with an even n; dx bit for bit where n is a power of two."""
    out = []
    for i, (name, (shape, _, _)) in enumerate(SHAPES.items()):
        n = shape[0] * shape[2] * shape[3]
        if n % 2 == 0:
            for j, variant in enumerate(("plain", "res_lrelu")):
                out.append((name, variant, (0.25, 0.5)[(i + j) % 2], (0.5, 1.0)[i % 2], n & (n - 1) == 0))
    return out


def case_id(spec):
    return "-".join(("nonfinite" if s is True else "finite" if s is False else str(s)) for s in spec)


def build_mixed(spec, huge_exp=60):
    """huge_exp: the scale of the `huge` family, 2^60 for everything that sums in double; an implementation that sums squares in fp32
    (ATen on the CPU) overflows there -- the point of the family -- and can only stand in at 2^30."""
    name, variant, cfg, rot, nonfinite = spec
    res, act = VARIANTS[variant]
    return make_case(SHAPES[name][0], res, act, cfg, rot, nonfinite, huge_exp=huge_exp), route_of(name)


def build_exact(spec):
    name, variant, slope, momentum, _ = spec
    return make_exact_case(SHAPES[name][0], VARIANTS[variant][0], slope, momentum), route_of(name)
