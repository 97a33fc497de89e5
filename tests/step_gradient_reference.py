"""What the FFWM train step hands to Adam, restated without any of the step's machinery, and the bound its gradients are held to.

The reference (`reference_passes`) is the hand-driven sequence that `FFWMTrainer.step()` computes on a CPU trainer bit for bit
(tests/test_step_gradients_cpu.py): forward, backward_D, netD's Adam step, backward_G, on a trainer that was BUILT on the CPU -- so
no kernel route, fused module, reducer view or HIP op is installed -- whose networks were then moved to the device and dtype asked
for.  In float64 it is the truth the device step is compared with; in float32 it is the yardstick: the G-side gradient of this
untrained step runs through many near-ties (max-pool, max-feature-map, ReLU and L1 sign kinks on nearly constant generated images),
some of which flip under ANY rounding, so plain float32 sits about 1e-2 (whole-net relative L2) from float64 on the generator side
and 2.5e-4 on the discriminator's.  The bound is a multiple of that distance: it is meant for dropped, duplicated, misplaced, stale
or mis-scaled contributions, not for last-bit errors (the kernels have their own per-element bounds).

    e32[p] = ||g32[p] - g64[p]||          r_N = ||g32_N - g64_N|| / ||g64_N||          T_N = number of tensors of net N
    tol[p] = M * max(e32[p], r_N * ||g64[p]||) + 16 u * ||g64_N|| / sqrt(T_N)          u = 2^-24, M = 4

The last term is the floor for the biases in front of a BatchNorm, whose gradient is mathematically zero (float64 norm ~1e-16):
16 roundings of the net's rms tensor norm.  M = 4: the yardstick is a single draw of a discrete quantity (kink flips), and the
device step rounds in another order and extent (Winograd transforms, atomics) than the plain float32 path.  A route that needs
more than 4 is a finding to chase, not a margin to widen.
"""
import contextlib
import math
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch_refs  # noqa: E402

NETS = ("flowNetF", "flowNetB", "netG", "netD")
LRS = (0.00005, 0.0004, 0.0004)          # opt_F, opt_G, opt_D (trainer.FFWMTrainer)
U = 2.0 ** -24
M = 4.0
ZERO_REL = 1e-9                          # a tensor whose float64 norm is below this fraction of its net's has a zero gradient


# ------------------------------------------------------------------------------------------------ the reference
def _warp(images, flow):
    # part_grids builds its grids in float32 whatever the images are: sample at those coordinates in the images' dtype
    return torch_refs.warp(images, flow.to(images.dtype))


def _warp_flipcat(feat, flow):
    return torch_refs.warp_flipcat(feat, flow.to(feat.dtype))


def graded_parameters(trainer):
    """{net: [(name, parameter)]} of everything an optimizer of the step owns (FlowNet's never-used occlusion branch is in none)."""
    out = {}
    for net in NETS:
        skip = "inter_conv_occ" if net.startswith("flowNet") else None
        out[net] = [(n, p) for n, p in getattr(trainer, net).named_parameters() if not (skip and n.startswith(skip))]
    return out


def plain_trainer(seed, ngf, batched_losses=False, crop=False):
    """The trainer the reference drives: built on the CPU, torch stand-ins for the warps, nets.GuidedFilter, separate loss passes."""
    from ffwm_amd import trainer
    return trainer.FFWMTrainer("cpu", seed=seed, ngf=ngf, warp=_warp, warp_flipcat=_warp_flipcat, batched_losses=batched_losses,
                               fused_l1=False, crop=crop)


def initial_weights(seed, ngf):
    """{net: {name: tensor}}: the weights every trainer of this seed starts from (the constructors seed the CPU generator)."""
    t = plain_trainer(seed, ngf)
    return {net: {n: p.detach().clone() for n, p in ps} for net, ps in graded_parameters(t).items()}


@contextlib.contextmanager
def _no_hip_kernels():
    """Inside: the frozen loss networks take their module path on a GPU too (nets.FUSED_ACTIVATIONS picks HIP kernels by the
    tensor's device), a call into the HIP library, by either binding, raises instead of computing the reference, and the vendor
    convolutions run on their deterministic algorithm.  Everything is put back on the way out."""
    from ffwm_amd import _ext, _lib, nets

    def refuse(*a, **k):
        raise AssertionError("the step-gradient reference reached a HIP kernel of ffwm_amd")
    saved = (nets.FUSED_ACTIVATIONS, _lib.load, _ext.get, torch.backends.cudnn.deterministic)
    nets.FUSED_ACTIVATIONS, _lib.load, _ext.get = False, refuse, refuse
    # the vendor convolutions on their deterministic algorithm: the float32 yardstick is ONE draw of where the kinks fall, and it
    # should be the same draw in every run
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        nets.FUSED_ACTIVATIONS, _lib.load, _ext.get, torch.backends.cudnn.deterministic = saved


def reference_passes(dtype, device, batch, seed, ngf, lrs, passes, crop=False):
    """`passes` passes of forward -> backward_D -> Adam(netD) -> backward_G on `batch` (a CPU batch of trainer.synthetic_batch),
    in `dtype` on `device`, from the weights of trainer seed `seed`.  `lrs` = (opt_F, opt_G, opt_D) learning rates; only the D step
    is applied -- the G-side gradients of a pass see the updated netD, nothing sees an updated generator.
    -> [{"grads": {net: {name: float64 CPU tensor}}, "losses": {name: float}}] per pass.  netD's gradients are those its Adam step
    received, i.e. from before its update."""
    t = plain_trainer(seed, ngf, crop=crop)
    t.red_G.remove()
    t.red_D.remove()
    device = torch.device(device)
    for name in NETS + ("lightCNN", "vgg"):
        getattr(t, name).to(device=device, dtype=dtype)
    t.device = device
    if crop:
        # losses.identity_network_input picks a HIP kernel for float32 GPU images: the PyTorch composition, at the float32 grid
        from ffwm_amd.identity_eval import crop_grid, torch_identity_input
        t._light_input = lambda x: torch_identity_input(x, True, grid=crop_grid(x.shape[0], 98, device=x.device).type_as(x))
    b = {k: v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device) for k, v in batch.items()}
    params = graded_parameters(t)
    opt_D = torch.optim.Adam(t.netD.parameters(), lr=lrs[2], betas=(0.5, 0.999))
    out = []
    with _no_hip_kernels():
        for _ in range(passes):
            for ps in params.values():
                for _, p in ps:
                    p.grad = None
            grads = {}

            def grab(net):
                grads[net] = {n: (torch.zeros_like(p) if p.grad is None else p.grad).detach().double().cpu() for n, p in params[net]}
            t.forward(b)
            for p in t.netD.parameters():
                p.requires_grad = True
            t.backward_D(b)
            grab("netD")
            opt_D.step()
            for p in t.netD.parameters():
                p.requires_grad = False
            t.backward_G(b)
            for net in ("flowNetF", "flowNetB", "netG"):
                grab(net)
            losses = {k: float(v.detach()) for k, v in t.losses.items()}
            losses["D"] = float(t.loss_D)
            t._drop_autograd_graph()
            out.append({"grads": grads, "losses": losses})
    return out


def conv_biases_feeding_batchnorm(trainer):
    """{net: [parameter name]}: biases of the (transposed) convolutions whose output goes straight into a BatchNorm2d, read from the
    modules.  The batch mean removes a per-channel constant, so their gradient is mathematically zero.  (A PixelShuffle between the
    two spreads four biases over one BatchNorm channel: those gradients are not zero.)"""
    out = {}
    for net, ps in graded_parameters(trainer).items():
        graded = {n for n, _ in ps}
        names = []
        for prefix, seq in getattr(trainer, net).named_modules():
            if not isinstance(seq, nn.Sequential):
                continue
            kids = list(seq.named_children())
            for (cn, c), (_, nxt) in zip(kids, kids[1:]):
                if isinstance(c, (nn.Conv2d, nn.ConvTranspose2d)) and c.bias is not None and isinstance(nxt, nn.BatchNorm2d):
                    name = ".".join(x for x in (prefix, cn, "bias") if x)
                    if name in graded:
                        names.append(name)
        out[net] = names
    return out


# ------------------------------------------------------------------------------------------------ the bound
def _sq(t):
    return float(t.double().pow(2).sum())


def net_norm(g):
    return math.sqrt(sum(_sq(v) for v in g.values()))


def net_distance(a, b):
    return math.sqrt(sum(_sq(a[k].double() - b[k].double()) for k in b))


class Tolerances(dict):
    """{net: {name: tol}} plus, per net: `net` (the whole-net bound M * ||g32_N - g64_N||), `r` (r_N) and `floor`."""

    def __init__(self):
        super().__init__()
        self.net, self.r, self.floor = {}, {}, {}


def bounds(g64, g32):
    """The tolerance of every tensor (module docstring) from the float64 gradients and the same harness run in float32."""
    tol = Tolerances()
    for net, ref in g64.items():
        assert set(ref) == set(g32[net]), net
        n64, d32 = net_norm(ref), net_distance(g32[net], ref)
        r = d32 / n64
        floor = 16 * U * n64 / math.sqrt(len(ref))
        tol[net] = {p: M * max(math.sqrt(_sq(g32[net][p].double() - ref[p])), r * math.sqrt(_sq(ref[p]))) + floor for p in ref}
        tol.net[net], tol.r[net], tol.floor[net] = M * d32, r, floor
    return tol


def floor_users(tol):
    """{net: [names]} of the tensors whose tolerance is mostly the floor (the floor exceeds the yardstick term)."""
    return {net: [p for p, v in t.items() if tol.floor[net] > v - tol.floor[net]] for net, t in tol.items()}


def zero_gradient_tensors(g64):
    """{net: [names]} of the tensors whose float64 norm is below ZERO_REL of their net's."""
    return {net: [p for p, v in g.items() if math.sqrt(_sq(v)) < ZERO_REL * net_norm(g)] for net, g in g64.items()}


def check(got, g64, tol, label="", relief=None):
    """Assert, for every tensor of every net, ||got[p] - g64[p]|| <= tol[p], and per net ||got_N - g64_N|| <= M ||g32_N - g64_N||.
    No tensor is left out: the nets and the names of `got` must be exactly the reference's.
    -> {net: {"tensor": max over p of error / (tol[p] / M), "net": whole-net error / (whole-net bound / M)}}, always against the
    tolerance proper: at most M for every net that `relief` does not name.
    A failure names the worst tensors with ||got[p]|| / ||g64[p]|| and the cosine: a scale error reads (2.0, 1.0) or (0.5, 1.0),
    a misplaced or stale gradient has a small cosine.
    `relief` {net: spec}, for a net the caller has MEASURED to miss M by conditioning (it states the figures), one of
      {"ratio": {"tensor": x, "net": y}}   the two ratios are held to x and y instead of M (a measured ratio x 1.5);
      {"one_group": [names, ...], "net": c}   every tensor over M must lie in ONE of the given groups of names, every other tensor
                                             stays at M, and the whole net within M or within c ||g64_N||."""
    assert set(got) == set(g64) == set(tol), (sorted(got), sorted(g64))
    ratios, bad = {}, []
    for net, ref in g64.items():
        spec = (relief or {}).get(net, {})
        m_t, m_n = spec.get("ratio", {}).get("tensor", M), spec.get("ratio", {}).get("net", M)
        assert set(got[net]) == set(ref), (net, sorted(set(got[net]) ^ set(ref))[:8])
        rows = []
        for p, r in ref.items():
            g = got[net][p].detach().double().cpu()
            assert g.shape == r.shape, (net, p, tuple(g.shape), tuple(r.shape))
            err = math.sqrt(_sq(g - r))
            err = float("inf") if err != err else err          # (a NaN fails)
            rows.append((err / (tol[net][p] / M), p, err, g, r))
        d = net_distance({p: got[net][p].detach().cpu() for p in ref}, ref)
        d = float("inf") if d != d else d
        ratios[net] = {"tensor": max(x[0] for x in rows), "net": d / (tol.net[net] / M)}
        failed = sorted((x for x in rows if x[0] > m_t), key=lambda x: -x[0])
        net_ok = ratios[net]["net"] <= m_n
        if "one_group" in spec:
            if any({x[1] for x in failed} <= set(group) for group in spec["one_group"]):
                failed = []
            net_ok = net_ok or d <= spec["net"] * net_norm(ref)
        if failed or not net_ok:
            lines = ["%s%s: whole-net error %.3e, bound %.3e (ratio %.2f of %g); %d of %d tensors over their tolerance"
                     % (label and label + " ", net, d, tol.net[net], ratios[net]["net"], m_n, len(failed), len(rows))]
            for ratio, p, err, g, r in (failed or sorted(rows, key=lambda x: -x[0]))[:6]:
                ng, nr = math.sqrt(_sq(g)), math.sqrt(_sq(r))
                cos = float((g * r).sum()) / (ng * nr) if ng > 0 and nr > 0 else float("nan")
                lines.append("    %-48s error %.3e tol %.3e (ratio %.2f)  |got|/|ref| %.4g  cosine %.4f"
                             % (p, err, tol[net][p], ratio, ng / nr if nr > 0 else float("inf"), cos))
            bad.append("\n".join(lines))
    assert not bad, "\n" + "\n".join(bad)
    return ratios


def format_ratios(rows):
    """rows: [(label, ratios as check returns them)] -> the table of the GPU test's docstring."""
    head = "%-34s" % "route" + "".join("%22s" % n for n in NETS)
    out = [head]
    for label, r in rows:
        out.append("%-34s" % label + "".join("%22s" % ("%.2f / %.2f" % (r[n]["tensor"], r[n]["net"])) for n in NETS))
    return "\n".join(out)
