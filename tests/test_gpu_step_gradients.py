"""The gradients the FFWM train step hands to Adam, on every route of the step, against a float64 step on the same device.

The reference is tests/step_gradient_reference.py: a trainer built on the CPU (no route, fused module, reducer view or HIP op) whose
networks are moved to the GPU, driven by hand -- forward, backward_D, Adam(netD), backward_G -- in float64 (the truth) and in
float32 (the yardstick of the bound).  tests/test_step_gradients_cpu.py shows that this sequence IS FFWMTrainer.step().
Scenario A: the real learning rates, one pass.  Scenario B: all learning rates 0, passes 1-4 on one batch: the weights stay put,
spectral norm's u / v advance, so every pass has its own gradients and a miscounted, stale or uncleared one shows.
Every route's gradients are read where Adam reads them (`p.grad`, which must alias the reducer's flat array) and go through
`check`; no tensor is left out.  flowNetF, flowNetB and netG are held to M = 4 on every route, netD on route 7; netD's two
reliefs on the other routes are stated, with their measurements, at the end of this text.

Measured on an MI355X (ngf=16, batch 2, trainer seed 0, batch seed 3).  A float64 pass takes 0.3-0.6 s, a float32 pass 0.2 s; the
whole fixture (5 + 5 passes, three CPU-side trainer constructions) 6-9 s inside the suite and 25 s in a fresh process, 18 s of which is
the vendor library's first use of its float32 kernels.  Under the 30 s that would have called for a committed fixture.

The reference runs the vendor convolutions on their deterministic algorithm (step_gradient_reference._no_hip_kernels).  Without that
the plain float32 pass is not reproducible to the last bit on the GPU, its kinks fall differently from run to run and r_N with them:
flowNetB read 2.3e-3 ... 7.8e-3 in ten draws and 1.6e-4 in an eleventh (routes 1-3 then read 21 for flowNetB with nothing wrong),
netD 2.7e-6 ... 2.5e-3 in fourteen.  With it two fresh processes gave the same figures to every digit printed, and scenario A equals
B pass 1 for flowNetB and netD, as it must.  Behind the rest of the suite in one process the draw is another one (the vendor library
chooses by what it has seen), again consistent in itself: A 2.5e-2 / 7.4e-3 / 6.6e-3 / 5.2e-4, pass 3 netD 3.5e-6; the ratios there were
at most 2.47 on the generator side, netD 0.56 / 0.31 on routes 1-3, 157.4 / 59.2 on routes 4-6 and 1.00 / 1.00 on route 7.  Fresh process:

Plain float32 against float64 on the GPU, r_N (whole-net relative L2):
    scenario        flowNetF    flowNetB    netG        netD
    A               1.94e-2     5.64e-3     7.64e-3     6.71e-4
    B pass 1        1.91e-2     5.64e-3     7.50e-3     6.71e-4
    B pass 2        1.84e-2     4.48e-3     8.22e-3     5.06e-4
    B pass 3        1.52e-2     6.15e-3     7.15e-3     3.37e-6
    B pass 4        1.52e-2     4.75e-3     7.19e-3     2.77e-4

Ratios error / (tol / M) as `check` returns them, worst tensor / whole net; M = 4 is the bound (both processes alike but for
flowNetB's worst tensor on routes 4-7, 0.68 ... 0.90):
    route                              flowNetF       flowNetB       netG           netD
    1 A eager default                  2.58 / 1.31    1.20 / 0.61    0.95 / 0.77    0.43 / 0.24
    2 A segmented backward             2.58 / 1.31    1.20 / 0.61    0.95 / 0.77    0.43 / 0.24
    3 A loss_precision=bf16x3          2.58 / 1.31    1.20 / 0.61    0.95 / 0.77    0.43 / 0.24
    4 B eager, step 3                  2.69 / 0.88    0.75 / 0.38    1.63 / 1.11    148.8 / 60.6
    5 B one graph, replay 1            2.69 / 0.88    0.76 / 0.38    1.63 / 1.11    148.8 / 60.6
    6 B three graphs, replay 1         2.69 / 0.88    0.69 / 0.38    1.63 / 1.11    148.8 / 60.6
    7 B one graph, replay 2            2.81 / 0.95    0.79 / 0.40    1.06 / 0.87    1.00 / 1.00
    control: pass 2 offered as pass 3  fails in all four networks (whole-net ratios of the order of 30 ... 50 on the generator side,
                                       thousands for netD)

netD misses M = 4 on routes 4-6, and on a first-step route in some runs, by CONDITIONING, not by a defect; the three generator-side
networks hold M = 4 everywhere.  netD's float32 gradient is a draw of a discrete quantity with few events: about one LeakyReLU of the
discriminator sits within rounding of its kink.  A flip changes the gradient that enters the BatchNorm in front of it, so it moves the
parameters of that BatchNorm and of everything before it IN THAT SCALE's net and nothing else (seen: nets.k.0.weight_orig, nets.k.1.*,
nets.k.3.weight_orig, nets.k.4.* for k = 0 or 1, five tensors over tolerance each time), by 2e-4 ... 5.5e-3 of the whole net's norm.
Which way it falls changes from run to run on EVERY float32 path, the plain one included: the forward pass of a step is not reproducible
to the last bit (the sum of img_GF128 differs in the tenth digit between identical trainers; scenario A and B pass 1 are the same
computation for netD and read 2.8e-4 and 6.7e-4 in one run, before the reference was made deterministic).  The draws, netD's
whole-net distance from float64 (the plain float32 ones from before that; the device step draws anew every run):
    plain float32, 14 draws     2.7e-6 and 2.9e-6 (no flip: reference pass 3, both runs), 4.3e-5, 2.7e-4 (x3), 2.8e-4 (x2), 5.1e-4 (x3),
                                6.7e-4, 8.1e-4, 8.3e-4, 2.5e-3 (nets.1.1.bias 1.2e-2 of its own norm)
    device, first step, 14      1.6e-4 eleven times (default x5, segmented x3, bf16x3 x3), 5.5e-3 three times (default once, bf16x3
                                twice: nets.1.1.bias 2.7e-2 of its own norm, nets.1.4.bias, nets.1.0.weight_orig, nets.1.1.weight and
                                nets.1.3.weight_orig over tolerance, nothing else; netD's ratios 93.1 / 19.5)
    device, pass 3, 12 draws    2.0e-4 every time (eager, one graph, three graphs; four runs): one flip in nets.0 against a yardstick without
So the relief is scoped to that mechanism and to where it was seen:
    routes 4-6   the issue's fallback: netD's ratios asserted at the measured values x 1.5 (ROUTES_4_6: 148.8 and 60.6 -> 223.2 and 90.9; four earlier runs read 171 ... 183 and 70 ... 77 against non-deterministic yardsticks, inside it too);
    routes 1-3   ONE_FLIP: the tensors over M = 4 must all belong to the first eight modules of ONE scale's net, every other tensor of
                 netD stays at M = 4, and the whole net within M = 4 or within 1.5 x 5.5e-3 of its norm, the largest single flip seen.
                 This departs from the issue's fallback (a fixed ratio per route): the ratio of two such draws spans 0.3 ... 2000.
    route 7      no relief: 1.00 / 1.00.
A larger flip than any seen would fail routes 1-6 with nothing wrong; the failure message names the tensors, which shows it.
"""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_gradient_reference as sgr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, NGF, BATCH_SEED = 0, 16, 3
# netD's two reliefs (module docstring).  Routes 4-6: the measured ratios x 1.5.  Routes 1-3: one LeakyReLU flip -- what is over M = 4
# lies in ONE scale's net, in the modules up to its last BatchNorm (0 conv, 1 BatchNorm, 3 conv, 4 BatchNorm, 6 conv, 7 BatchNorm);
# the whole net within 1.5 x the largest single flip measured, 5.5e-3 of its norm.
ROUTES_4_6 = {"netD": {"ratio": {"tensor": 1.5 * 148.8, "net": 1.5 * 60.6}}}
_SCALE = ["nets.%d.%d.%s" % (0, i, w) for i, ws in ((0, ("weight_orig", "bias")), (1, ("weight", "bias")), (3, ("weight_orig", "bias")),
                                                    (4, ("weight", "bias")), (6, ("weight_orig", "bias")), (7, ("weight", "bias")))
          for w in ws]
ONE_FLIP = {"netD": {"one_group": [[n.replace("nets.0.", "nets.%d." % k) for n in _SCALE] for k in range(3)], "net": 1.5 * 5.5e-3}}


def _batch(device):
    from ffwm_amd import trainer
    return trainer.synthetic_batch(2, device, seed=BATCH_SEED)


@pytest.fixture(scope="module", autouse=True)
def _vendor_autotune_off():
    """As the other whole-step tests: no autotuning of the vendor convolutions; the setting is put back when the module is through."""
    before = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    yield
    torch.backends.cudnn.benchmark = before


@pytest.fixture(scope="module")
def ref():
    """The float64 and plain float32 passes of both scenarios (5 + 5 passes), their tolerances and the common starting weights."""
    b = _batch("cpu")
    took = {}

    def run(dtype, lrs, passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sgr.reference_passes(dtype, DEV, b, SEED, NGF, lrs, passes)
        torch.cuda.synchronize()
        took[(dtype, passes)] = time.perf_counter() - t0
        return out
    a64, a32 = run(torch.float64, sgr.LRS, 1), run(torch.float32, sgr.LRS, 1)
    b64, b32 = run(torch.float64, (0.0, 0.0, 0.0), 4), run(torch.float32, (0.0, 0.0, 0.0), 4)
    print("\nreference passes (trainer construction on the CPU included): " +
          ", ".join("%s x %d: %.1f s" % (str(k[0])[6:], k[1], v) for k, v in took.items()))
    out = {"A": {"g64": a64[0]["grads"], "tol": sgr.bounds(a64[0]["grads"], a32[0]["grads"]), "losses": a64[0]["losses"]},
           "B": [{"g64": p64["grads"], "tol": sgr.bounds(p64["grads"], p32["grads"]), "losses": p64["losses"]}
                 for p64, p32 in zip(b64, b32)],
           "weights": sgr.initial_weights(SEED, NGF)}
    for label, tol in [("A", out["A"]["tol"])] + [("B pass %d" % (i + 1), p["tol"]) for i, p in enumerate(out["B"])]:
        print("plain float32 against float64, r_N, %-9s " % label + "  ".join("%s %.2e" % (n, tol.r[n]) for n in sgr.NETS))
    assert all(set(g) <= set(out["A"]["g64"]["netD"]) for g in ONE_FLIP["netD"]["one_group"])
    return out


def _trainer(ref, lr0=False, **kw):
    """A device trainer of the reference's seed, held to the reference's starting weights; lr0: the three learning rates 0, set the
    way a scheduler sets them."""
    from ffwm_amd import trainer
    t = trainer.FFWMTrainer(DEV, seed=SEED, ngf=NGF, **kw)
    for net, ps in sgr.graded_parameters(t).items():
        assert [n for n, _ in ps] == list(ref["weights"][net]), net
        for n, p in ps:
            assert torch.equal(p.detach().cpu(), ref["weights"][net][n]), (net, n)
    if lr0:
        for opt in (t.opt_F, t.opt_G, t.opt_D):
            opt.param_groups[0]["lr"] = 0.0
    return t


def _grads(t):
    """What Adam read in the step that just ran: p.grad (through the reducer's view where a capture path left it unset), which must
    be the parameter's slice of the reducer's flat gradient array."""
    torch.cuda.synchronize()
    out = {}
    for net, ps in sgr.graded_parameters(t).items():
        red = t.red_D if net == "netD" else t.red_G
        out[net] = {}
        for n, p in ps:
            view = red._view[p]
            g = p.grad if p.grad is not None else view
            assert g.data_ptr() == view.data_ptr() and g.shape == view.shape, (net, n)
            a, e = red.offset[p]
            assert view.data_ptr() == red.flat[a:e].data_ptr() and e - a == p.numel(), (net, n)
            out[net][n] = g.detach().double().cpu()
    return out


def _check(label, got, want, relief=None):
    ratios = sgr.check(got, want["g64"], want["tol"], label, relief=relief)
    print("\n" + sgr.format_ratios([(label, ratios)]))
    return ratios


def _weights_unmoved(t, ref):
    for net, ps in sgr.graded_parameters(t).items():
        for n, p in ps:
            assert torch.equal(p.detach().cpu(), ref["weights"][net][n]), (net, n)


# ------------------------------------------------------------------------------------------------ scenario A: the first step
def test_route_1_default_eager_first_step(ref):
    """netD's gradients are those from before its update; the G-side gradients see the updated netD."""
    t = _trainer(ref)
    assert t.flat_adam and t.red_G.gather and t.fused_l1 and t.batched_losses and not t.segmented
    t.step(_batch(DEV))
    _check("1 A eager default", _grads(t), ref["A"], ONE_FLIP)


def test_route_2_segmented_backward(ref):
    t = _trainer(ref, segmented_backward=True)
    t.step(_batch(DEV))
    _check("2 A segmented backward", _grads(t), ref["A"], ONE_FLIP)


def test_route_3_loss_networks_on_bf16x3(ref):
    """Same bound: the route claims float32-grade results."""
    t = _trainer(ref, loss_precision="bf16x3")
    t.step(_batch(DEV))
    _check("3 A loss_precision=bf16x3", _grads(t), ref["A"], ONE_FLIP)


# ------------------------------------------------------------------------------------------------ scenario B: learning rates 0
def test_reference_pass_2_would_not_pass_as_pass_3(ref):
    """The control of routes 4-7: a step that handed Adam the PREVIOUS step's gradients fails `check` in every one of the four
    networks, under the relief of routes 4-6 too (whole-net ratios of the order of 30 ... 50 on the generator side, thousands for netD)."""
    with pytest.raises(AssertionError) as e:
        sgr.check(ref["B"][1]["g64"], ref["B"][2]["g64"], ref["B"][2]["tol"], "control: pass 2 as pass 3", relief=ROUTES_4_6)
    print(str(e.value)[:1500])
    assert all("control: pass 2 as pass 3 %s:" % net in str(e.value) for net in sgr.NETS)


def test_route_4_third_eager_step_with_the_arena_served(ref):
    """The weight-gradient arena is served from the second step on and the buckets must be cleared between steps: the third step's
    gradients are reference pass 3 (and, by the control above, not pass 2)."""
    t = _trainer(ref, lr0=True)
    b = _batch(DEV)
    for _ in range(3):
        t.step(b)
    got = _grads(t)
    _weights_unmoved(t, ref)
    _check("4 B eager, step 3", got, ref["B"][2], ROUTES_4_6)


@pytest.fixture(scope="module")
def replays(ref):
    """Routes 5 and 7: capturable trainer, learning rates 0, capture(batch, warmup=2) -- two eager passes; the capture itself executes
    nothing -- then two replays: passes 3 and 4."""
    t = _trainer(ref, lr0=True, capturable=True)
    b = _batch(DEV)
    t.capture(b, warmup=2)
    assert len(t._graphs) == 1
    out = []
    for _ in range(2):
        t.step(b)
        out.append(_grads(t))
    _weights_unmoved(t, ref)
    t.release_graphs()
    return out


def test_route_5_first_replay_of_the_captured_step(ref, replays):
    _check("5 B one graph, replay 1", replays[0], ref["B"][2], ROUTES_4_6)


def test_route_7_second_replay_of_the_captured_step(ref, replays):
    _check("7 B one graph, replay 2", replays[1], ref["B"][3])


def test_route_6_first_replay_of_the_three_graph_split(ref):
    t = _trainer(ref, lr0=True, capturable=True)
    t.dp_active = True              # the data-parallel capture path (the reducers are world-size-1 no-ops here)
    b = _batch(DEV)
    t.capture(b, warmup=2, mode="serial")
    assert len(t._graphs) == 3
    t.step(b)
    got = _grads(t)
    _weights_unmoved(t, ref)
    t.release_graphs()
    _check("6 B three graphs, replay 1", got, ref["B"][2], ROUTES_4_6)


# ------------------------------------------------------------------------------------------------ the floor
def test_the_floor_serves_only_the_biases_in_front_of_a_batchnorm(ref):
    """The tensors with a zero float64 gradient (norm below 1e-9 of their net's: the ones that need the floor) are exactly the conv
    biases that feed a BatchNorm, counted from the modules, in every pass, and no other tensor's tolerance is mostly the floor --
    netD's included in every pass whose float32 draw holds a kink flip (r_N >= 1e-5).  In a pass without one (reference pass 3:
    r_N = 3.4e-6, rounding alone) the formula itself puts the floor, 16 u / sqrt(T) = 1.5e-7 of the net's norm, above 4 r_N |g64[p]|
    for every tensor below 1.4e-2 of the net's norm: there only the count is asserted for netD."""
    expected = sgr.conv_biases_feeding_batchnorm(sgr.plain_trainer(SEED, NGF))
    for case in [ref["A"]] + ref["B"]:
        zero, floored = sgr.zero_gradient_tensors(case["g64"]), sgr.floor_users(case["tol"])
        for net in sgr.NETS:
            assert len(zero[net]) == len(expected[net]) and sorted(zero[net]) == sorted(expected[net]), (net, len(zero[net]))
            if net != "netD" or case["tol"].r[net] >= 1e-5:
                assert set(floored[net]) <= set(zero[net]), (net, case["tol"].r[net], sorted(set(floored[net]) - set(zero[net])))
