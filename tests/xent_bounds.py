"""Per-element float64 error bounds, input families and a float32 emulation for the fused classifier loss
(csrc/softmax_xent.hip, ffwm_softmax_xent) -- a plain helper module, not a conftest.  The convention is that of
tests/landmark_bounds.py.

The reference is float64 torch on the CPU, computed from the call's ACTUAL inputs (the float values it is handed, widened).
u = 2^-24 (2^-53 for a float64 call), one SAFETY = 4 multiplies every count of roundings (U = SAFETY u below), FLOOR = 1e-38 keeps a
bound of exactly zero from dividing.  No constant is fitted to the kernel's output: each is a count of roundings read off the
kernel's arithmetic, which is (row x of N logits, target t, C = ffwm_softmax_xent_chunk(); built without FMA contraction)
    pass 1, per chunk c    m_c = max x_j                                               exact
                           s_c = sum_j double(exp_T(x_j - m_c))                        1 rounding of the difference, exp_T, then double
    pass 2, per row        M = max_c m_c,  S = sum_c s_c exp(m_c - M),  lse = M + log S          all in double
                           row_loss = T(lse - x_t)                                     double, then 1 rounding to T
                           grad_j = (exp_T(x_j - T(lse)) - [j == t]) / T(B)            T(lse), the difference, exp_T, the -1, the division
    pass 3                 out[0] = T(sum_b loss_b / B) in double;  out[k] = T(hits_k) * T(100 / B)

exp_T is HIP's expf / exp: the HIP math API documents a maximum error of 1 ulp for both (EXP_ULP = 1; 1 ulp is a relative error of at
most 2 u).  A rounding error d of exp's ARGUMENT multiplies the result by exp(d): relative error expm1(d).

    A     = M - min finite x_j >= |x_j - m_c| of every finite element
    dS    = expm1(U A) + 2 EXP_ULP U + SAFETY 2^-53 (N + chunks + 8)                   relative error of S (and of every s_c)
    dlse  = dS + SAFETY 2^-53 (|M| + |log S| + |lse|)                                  absolute error of lse (d log S = dS / S)
    row_loss bound = dlse + U |loss|
    out[0] bound   = mean_b (dlse_b + SAFETY 2^-53 B |loss_b|) + U |out[0]|
    darg_j = dlse + U (|lse| + |x_j - lse|)                                            T(lse) and the difference
    grad bound_j = (p_j (expm1(darg_j) + 2 EXP_ULP U) + [j == t] U |p_j - 1| + TINY) / B + U |grad_j|
with p_j = exp(x_j - lse) and TINY the smallest normal number of T (a result below it may be flushed or lose bits).  A -inf logit has
p_j = 0 and is asserted == 0 exactly.  out[1], out[2]: 2 U |value| (two roundings).  Ranks and `skipped` are compared exactly; the
expected rank follows the entry point's rule (NaN above everything and equal to another NaN, ties to the lower index).
A module-level result multiplies the stored gradient by grad_output: 2 U |ref| more per element.
For a float64 call the reference rounds as often as the kernel does: the assertions take twice the bound.

Input families (FAMILIES):
    random         N(0,1) logits, spread so that two logits of a row differ by at least GAP after rounding (asserted here): the reference's
                   topk-based accuracy() is then well defined
    wide           uniform in [-80, 80): without the maximum subtracted exp overflows float32
    target_is_max  random, the target's logit raised above the row maximum
    ties           all logits equal: the rank is the target index, the loss log N
    masked         random, a quarter of the entries -inf, never the target: gradient exactly 0 there
    nan_row        random, one row holds a NaN (not on its target unless N = 1): that row and out[0] are NaN, the other rows meet their bounds
    outside        random, the targets of every other row (row 0 first) replaced in turn by -1, N and 2^40: counted, zero rows
"""
import math

import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 4.0
FLOOR = 1e-38
EXP_ULP = 1.0                # HIP math API: expf and exp, maximum error 1 ulp
GUARD = 64                   # NaN cells before and behind grad_logits and row_loss
GAP = 2e-6
FAMILIES = ("random", "wide", "target_is_max", "ties", "masked", "nan_row", "outside")


def shapes(C):
    """(B, N) for a chunk of C elements: single elements, odd sizes below a vector, below / at / above one chunk, a ragged fifth chunk,
    many rows, the workload's own."""
    return ((1, 1), (1, 2), (2, 5), (3, 6), (3, 257), (2, C - 1), (2, C), (2, C + 1), (1, 4 * C + 1), (64, 1000), (10, 79077))


def unit(dtype):
    return U32 if dtype == torch.float32 else U64


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def dtype(self):
        return self.logits.dtype

    def __repr__(self):
        return "%s B%d N%d %s" % (self.family, self.logits.shape[0], self.logits.shape[1], str(self.dtype).replace("torch.", ""))


def _spread_normal(B, N, gen, dtype):
    """N(0,1) rows whose sorted values are at least GAP apart (asserted after the rounding to `dtype`), in random order."""
    v = torch.sort(torch.randn(B, N, generator=gen, dtype=torch.float64), 1)[0]
    v = torch.cummax(v - GAP * torch.arange(N, dtype=torch.float64), 1)[0] + GAP * torch.arange(N, dtype=torch.float64)
    order = torch.argsort(torch.rand(B, N, generator=gen), 1)
    x = torch.empty_like(v).scatter_(1, order, v).to(dtype)
    if N > 1:
        assert float(torch.sort(x.double(), 1)[0].diff(dim=1).min()) > 0.25 * GAP, "two logits of a row closer than the gap"
    return x


def make_case(B, N, family, dtype=torch.float32, seed=0):
    assert family in FAMILIES
    gen = torch.Generator().manual_seed(104729 * seed + 131 * FAMILIES.index(family) + 17 * B + N)
    x = _spread_normal(B, N, gen, dtype)
    target = torch.randint(0, N, (B,), generator=gen)
    target[0] = N - 1
    target[-1] = 0 if B > 1 else target[-1]
    if family == "wide":
        x = ((torch.rand(B, N, generator=gen, dtype=torch.float64) * 160) - 80).to(dtype)
    elif family == "target_is_max":
        x[torch.arange(B), target] = (x.double().max(1)[0] + 1).to(dtype)
    elif family == "ties":
        x = torch.full((B, N), 0.5, dtype=dtype)
    elif family == "masked":
        off = torch.rand(B, N, generator=gen) < 0.25
        off[torch.arange(B), target] = False
        x = x.masked_fill(off, -math.inf)
    elif family == "nan_row":
        b = B // 2
        x[b, (int(target[b]) + 1) % N] = math.nan
    elif family == "outside":
        bad = torch.tensor([-1, N, 2 ** 40])
        for k, b in enumerate(range(0, B, 2)):
            target[b] = bad[k % 3]
    return Case(logits=x.contiguous(), target=target.contiguous(), family=family)


def expected_rank(x, target):
    """The entry point's rule on the exact values: NaN above everything and equal to another NaN, ties to the lower index; a target outside
    [0, N) gives N."""
    B, N = x.shape
    rank = torch.full((B,), N, dtype=torch.int64)
    for b in range(B):
        t = int(target[b])
        if not 0 <= t < N:
            continue
        row, xt = x[b], x[b, t]
        nan, tnan = torch.isnan(row), bool(torch.isnan(xt))
        above = (nan & (not tnan)) | (row > xt)
        same = (row == xt) | (nan & tnan)
        rank[b] = int(above.sum()) + int(same[:t].sum())
    return rank


class Bound:
    def __init__(self, case, chunk, safety=SAFETY):
        self.case = case
        T = case.dtype
        self.U = U = safety * unit(T)
        self.twice = 2.0 if T == torch.float64 else 1.0
        tiny = 2.0 ** -126 if T == torch.float32 else 2.0 ** -1022
        x = case.logits.double()
        B, N = x.shape
        chunks = (N + chunk - 1) // chunk
        t = case.target
        self.valid = valid = (t >= 0) & (t < N)
        self.skipped = int((~valid).sum())
        tc = t.clamp(0, N - 1)
        hot = torch.zeros(B, N, dtype=torch.float64).scatter_(1, tc.unsqueeze(1), 1.0) * valid.unsqueeze(1)
        M = x.masked_fill(torch.isnan(x), -math.inf).max(1, keepdim=True)[0]
        S = torch.exp(x - M).sum(1, keepdim=True)
        lse = M + torch.log(S)
        xt = x.gather(1, tc.unsqueeze(1))
        self.nan_rows = torch.isnan(x).any(1)
        self.row_loss = torch.where(valid, (lse - xt).squeeze(1), torch.zeros(B, dtype=torch.float64))
        p = torch.exp(x - lse)
        self.grad = torch.where(valid.unsqueeze(1), (p - hot) / B, torch.zeros_like(p))
        self.exact_zero = (x == -math.inf) | ~valid.unsqueeze(1)
        finite = torch.isfinite(x)
        A = M - x.masked_fill(~finite, math.inf).min(1, keepdim=True)[0]
        dS = torch.expm1(U * A) + 2 * EXP_ULP * U + safety * U64 * (N + chunks + 8)
        dlse = dS + safety * U64 * (M.abs() + torch.log(S).abs() + lse.abs())
        self.row_loss_bound = torch.where(valid, dlse.squeeze(1) + U * self.row_loss.abs(), torch.zeros(B, dtype=torch.float64))
        self.out0 = float(self.row_loss.sum()) / B
        self.out0_bound = float((torch.where(valid, dlse.squeeze(1), torch.zeros(B, dtype=torch.float64))
                                 + safety * U64 * B * self.row_loss.abs()).sum()) / B + U * abs(self.out0)
        darg = dlse + U * (lse.abs() + (x - lse).abs().masked_fill(~finite, 0.0))
        gb = (p * (torch.expm1(darg) + 2 * EXP_ULP * U) + hot * U * (p - 1).abs() + tiny) / B + U * self.grad.abs()
        self.grad_bound = torch.where(self.exact_zero, torch.zeros_like(gb), gb)
        self.rank = expected_rank(case.logits, t)
        self.prec = [100.0 * float((self.rank < k).sum()) / B for k in (1, 5)]

    def _ratio(self, got, ref, bound, rows):
        """max error / bound over the rows of `rows` (a bool mask over the first dimension)."""
        got = got.detach().to("cpu", torch.float64).reshape(ref.shape)[rows]
        r = (got - ref[rows]).abs() / (bound[rows] + FLOOR)
        r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
        return float(r.max()) if r.numel() else 0.0

    def check(self, out=None, row_loss=None, rank=None, grad=None, skipped=None, what="", factor=1.0, grad_output=1.0, verbose=True):
        """The entry point's outputs (any may be None) against the bounds.  grad_output: the gradient is a module-level result that was
        multiplied by it."""
        rows, fails = {}, []
        f = factor * self.twice
        ok = ~self.nan_rows
        any_nan = bool((self.nan_rows & self.valid).any())
        if out is not None:
            o = out.detach().cpu().double()
            if any_nan:
                if not math.isnan(float(o[0])):
                    fails.append("out[0] is not NaN although a row holds one")
            else:
                rows["out0"] = abs(float(o[0]) - self.out0) / (f * self.out0_bound + FLOOR)
            for i, k in enumerate((1, 5)):
                rows["prec%d" % k] = abs(float(o[1 + i]) - self.prec[i]) / (f * 2 * self.U * abs(self.prec[i]) + FLOOR)
        if row_loss is not None:
            rows["row_loss"] = self._ratio(row_loss, self.row_loss, f * self.row_loss_bound, ok)
            got = row_loss.detach().cpu()
            if not bool(torch.isnan(got[self.nan_rows & self.valid]).all()):
                fails.append("the loss of a row with a NaN is not NaN")
            if not bool((got[~self.valid] == 0).all()):
                fails.append("the loss of a skipped row is not 0")
        if grad is not None:
            ref = grad_output * self.grad
            bound = abs(grad_output) * self.grad_bound + (2 * self.U * ref.abs() if grad_output != 1.0 else 0.0)
            rows["grad"] = self._ratio(grad, ref, f * bound, ok)
            got = grad.detach().cpu().reshape(ref.shape)
            if not bool(torch.isnan(got[self.nan_rows & self.valid]).all()):
                fails.append("the gradient of a row with a NaN is not NaN everywhere")
            zero = self.exact_zero & ok.unsqueeze(1)
            if not bool((got[zero] == 0).all()):
                fails.append("grad != 0 on %d elements of -inf logits / skipped rows" % int((got[zero] != 0).sum()))
        if rank is not None and not torch.equal(rank.detach().cpu().long(), self.rank):
            fails.append("rank %s, expected %s" % (rank.detach().cpu().tolist()[:8], self.rank.tolist()[:8]))
        if skipped is not None and int(skipped) != self.skipped:
            fails.append("skipped = %d, expected %d" % (int(skipped), self.skipped))
        if verbose:
            print("XEBOUND %s %r: %s" % (what, self.case, " ".join("%s %.3g" % kv for kv in sorted(rows.items()))))
        fails += ["%s: error / bound = %.3g" % kv for kv in sorted(rows.items()) if not kv[1] <= 1.0]
        assert not fails, "%s %r: %s" % (what, self.case, "; ".join(fails))
        return rows


def emulate(case, chunk, subtract_max=True):
    """The kernel's arithmetic in torch on the CPU, in the case's dtype and the kernel's order: per chunk the maximum and the sum of
    exp_T(x - m) in double, the chunks combined in double, the gradient from T(lse).  subtract_max=False is a deliberately wrong variant
    (exp of the raw logits).  -> (out[3], row_loss, rank, grad, skipped)."""
    T = case.dtype
    x, t = case.logits, case.target
    B, N = x.shape
    valid = (t >= 0) & (t < N)
    tc = t.clamp(0, N - 1)
    ms, ss = [], []
    for c0 in range(0, N, chunk):
        part = x[:, c0:c0 + chunk]
        m = part.masked_fill(torch.isnan(part), -math.inf).max(1, keepdim=True)[0]
        if not subtract_max:
            m = torch.zeros_like(m)
        e = torch.exp(part - m)
        e = torch.where(part == -math.inf, torch.zeros_like(e), e)
        ms.append(m.double())
        ss.append(e.double().sum(1, keepdim=True))
    ms, ss = torch.cat(ms, 1), torch.cat(ss, 1)
    M = ms.max(1, keepdim=True)[0]
    scale = torch.exp(ms - M)
    S = torch.where(ss != 0, ss * scale, torch.zeros_like(ss)).sum(1, keepdim=True)
    lse = M + torch.log(S)
    loss = torch.where(valid, (lse - x.gather(1, tc.unsqueeze(1)).double()).squeeze(1), torch.zeros(B, dtype=torch.float64))
    p = torch.exp(x - lse.to(T))
    hot = torch.zeros(B, N, dtype=T).scatter_(1, tc.unsqueeze(1), 1.0)
    grad = torch.where(valid.unsqueeze(1), (p - hot) / torch.tensor(float(B), dtype=T), torch.zeros_like(p))
    rank = expected_rank(x, t)
    per = torch.tensor(100.0 / B, dtype=T)
    out = torch.stack(((loss.sum() / B).to(T), (rank < 1).sum().to(T) * per, (rank < 5).sum().to(T) * per))
    return out, loss.to(T), rank.to(torch.int32), grad, int((~valid).sum())


def reference_accuracy(output, target, topk=(1, 5)):
    """lightcnn/finetune.py:294-307 restated (reshape for the view that current PyTorch refuses)."""
    maxk = max(topk)
    pred = output.topk(maxk, 1, True, True)[1].t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    return [float(correct[:k].reshape(-1).float().sum(0).mul_(100.0 / target.size(0))) for k in topk]
