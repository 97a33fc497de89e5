"""Per-element float64 error bounds, cases and a float32 emulation for the flat SGD step (csrc/sgd.hip, ffwm_sgd_step) -- a plain
helper module, not a conftest.  The convention is that of tests/landmark_bounds.py.

The reference is float64 torch on the CPU, started from the call's ACTUAL p, g and buf (float32 values, widened) and fed the actual
gradients of every step.  u = 2^-24, one SAFETY = 4 multiplies every count of roundings (U = SAFETY u), FLOOR = 1e-38 keeps a bound of
exactly zero from dividing.  The kernel's arithmetic per element and step (float32, no FMA contraction; lr, wd of the element's
segment's group and the momentum are doubles rounded to float32: one u each on the product they enter):
    t1 = wd * p          1 rounding (+ wd's)
    g' = g + t1          1 rounding
    t2 = momentum * buf  1 rounding (+ the momentum's)
    buf' = t2 + g'       1 rounding
    p' = fma(-lr, buf', p)   1 rounding; q = lr buf' is not rounded on its own (+ lr's)
FIVE roundings per element and step.  With e_p, e_buf the bounds carried in from the step before (0 at the start):
    e_buf' = momentum e_buf + wd e_p + U (2 |t1| + |g'| + 2 |t2| + |buf'|)
    e_p'   = e_p + lr e_buf' + U (|q| + |p'|)
A group with rate 0.0 leaves p unchanged BIT FOR BIT (asserted exactly), while buf still updates.  NaN guard cells before and behind
all three arrays must stay NaN.
"""
import math

import torch

U32 = 2.0 ** -24
SAFETY = 4.0
FLOOR = 1e-38
GUARD = 64                   # NaN cells before and behind params, grads and the momentum buffer (64 floats keep the 16-byte alignment)
MOMENTUM = 0.9
BASE_LR, DECAY = 1e-4, 1e-4
# the reference's four settings (lightcnn/finetune.py:74-86: weights, biases, fc2.weight, fc2.bias) and a frozen group
GROUPS = ((1 * BASE_LR, DECAY), (2 * BASE_LR, 0.0), (10 * BASE_LR, DECAY), (20 * BASE_LR, 0.0), (0.0, DECAY))


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "n%d segs%d %s" % (self.n, len(self.seg_end), self.name)


def _case(name, n, seg_end, seg_group, seed, steps=3, groups=GROUPS, scale=1.0):
    assert seg_end[-1] == n and list(seg_end) == sorted(set(seg_end)) and len(seg_end) == len(seg_group)
    gen = torch.Generator().manual_seed(7919 * seed + n)
    p = (torch.randn(n, generator=gen, dtype=torch.float64) * scale).float()
    buf = (torch.randn(n, generator=gen, dtype=torch.float64) * 0.1).float()
    grads = [(torch.randn(n, generator=gen, dtype=torch.float64) * 0.25).float() for _ in range(steps)]
    return Case(name=name, n=n, seg_end=list(seg_end), seg_group=list(seg_group), groups=[tuple(map(float, g)) for g in groups],
                p=p, buf=buf, grads=grads, momentum=MOMENTUM)


def cases():
    """n in {1, 3, 4, 5, 1027}: boundaries that are no multiples of 4, a segment of one element, every group kind, the frozen group;
    one case of 2^20 + 3 elements (several blocks, the grid-stride loop, a tail of three)."""
    out = [
        _case("one", 1, [1], [0], 1),
        _case("three", 3, [1, 3], [1, 4], 2),
        _case("four", 4, [3, 4], [2, 3], 3),
        _case("five", 5, [2, 3, 5], [0, 4, 1], 4),
        _case("odd-boundaries", 1027, [1, 6, 7, 130, 515, 1026, 1027], [0, 1, 4, 2, 3, 0, 1], 5),
        _case("one-segment", 1027, [1027], [2], 6),
    ]
    n = 2 ** 20 + 3
    ends = sorted(set([1, 2, 5, 79077 + 5, n - 2, n] + [k * 26215 + (k % 7) for k in range(1, 40)]))
    out.append(_case("large", n, ends, [k % 5 for k in range(len(ends))], 7))
    return out


def per_element(case):
    """(lr, wd) of every element, float64."""
    lr, wd = torch.empty(case.n, dtype=torch.float64), torch.empty(case.n, dtype=torch.float64)
    a = 0
    for e, k in zip(case.seg_end, case.seg_group):
        lr[a:e], wd[a:e] = case.groups[k][0], case.groups[k][1]
        a = e
    return lr, wd


class Bound:
    """The float64 reference and the bounds after every step: self.p[k], self.buf[k], self.p_bound[k], self.buf_bound[k] for k steps
    taken (index 0 = the start)."""

    def __init__(self, case, safety=SAFETY):
        self.case = case
        U = safety * U32
        lr, wd = per_element(case)
        self.lr = lr
        m = case.momentum
        p, b = case.p.double(), case.buf.double()
        ep, eb = torch.zeros_like(p), torch.zeros_like(p)
        self.p, self.buf, self.p_bound, self.buf_bound = [p], [b], [ep], [eb]
        for g in case.grads:
            t1 = wd * p
            gd = g.double() + t1
            t2 = m * b
            b = t2 + gd
            q = lr * b
            p = p - q
            eb = m * eb + wd * ep + U * (2 * t1.abs() + gd.abs() + 2 * t2.abs() + b.abs())
            ep = ep + lr * eb + U * (q.abs() + p.abs())
            self.p.append(p)
            self.buf.append(b)
            self.p_bound.append(ep)
            self.buf_bound.append(eb)

    def check(self, p, buf, steps, what="", factor=1.0, verbose=True):
        rows, fails = {}, []
        for name, got, ref, bound in (("p", p, self.p[steps], self.p_bound[steps]), ("buf", buf, self.buf[steps], self.buf_bound[steps])):
            r = (got.detach().cpu().double() - ref).abs() / (factor * bound + FLOOR)
            r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
            rows[name] = float(r.max())
        frozen = self.lr == 0
        if bool(frozen.any()) and not torch.equal(p.detach().cpu()[frozen], self.case.p[frozen]):
            fails.append("a parameter of a group with rate 0.0 changed")
        if verbose:
            print("SGDBOUND %s %r steps %d: %s" % (what, self.case, steps, " ".join("%s %.3g" % kv for kv in sorted(rows.items()))))
        fails += ["%s: error / bound = %.3g" % kv for kv in sorted(rows.items()) if not kv[1] <= 1.0]
        assert not fails, "%s %r: %s" % (what, self.case, "; ".join(fails))
        return rows


def emulate(case, steps, decay_everywhere=False):
    """The kernel's arithmetic in float32 torch on the CPU (the fma through a double product, which is exact, and one double sum).
    decay_everywhere=True is a deliberately wrong variant: the weight decay of group 0 applied to the groups without one.
    -> (p, buf) after `steps` steps."""
    lr, wd = per_element(case)
    if decay_everywhere:
        wd = torch.where(wd == 0, torch.full_like(wd, case.groups[0][1]), wd)
    lr, wd = lr.float(), wd.float()
    m = torch.tensor(case.momentum, dtype=torch.float32)
    p, b = case.p.clone(), case.buf.clone()
    for g in case.grads[:steps]:
        gd = g + wd * p
        b = m * b + gd
        p = (p.double() - lr.double() * b.double()).float()
    return p, b


def guarded(t, guard=GUARD):
    """[NaN x guard | t | NaN x guard] -> (whole, view of the middle)."""
    whole = torch.full((t.numel() + 2 * guard,), math.nan, dtype=t.dtype, device=t.device)
    whole[guard:guard + t.numel()] = t
    return whole, whole[guard:guard + t.numel()]


def guards_intact(whole, guard=GUARD):
    return bool(torch.isnan(whole[:guard]).all()) and bool(torch.isnan(whole[whole.numel() - guard:]).all())
