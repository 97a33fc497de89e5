"""Four kernels of every train step -- the batched spectral norm (csrc/spectral_norm.hip), the flat Adam step (csrc/adam.hip), the fused
L1 terms (csrc/l1_loss.hip) and the correlation column maximum (csrc/correlation.hip) -- against the float64 yardsticks of
tests/step_bounds.py and tests/step_bounds_sn.py, straight through the C ABI.  Every output is pre-filled with NaN, every array carries
16 NaN guard cells that must be bit-identical afterwards.  Run with ``-m gpu`` on the MI355X.

``python tests/test_gpu_step_bounds.py --report profiles/step_bounds.txt [--parent-lib OTHER/libffwm_hip.so]`` writes the worst error /
bound per kernel, stage, shape class and family, and three timings of the profiler row correlation_colmax at (1, 4096, 128) -- with
--parent-lib also three of that library's, interleaved."""
import ctypes
import functools
import math
import os
import sys

import pytest
import torch

import step_bounds as sb
import step_bounds_sn as sn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = {}                                   # (kernel, stage, shape class, family) -> worst error / bound, for the report


def _lib():
    from ffwm_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _finish(ck, kernel, shape_class):
    try:
        rows = ck.finish()
    finally:
        for (stage, fam), v in ck.rows.items():
            key = (kernel, stage, shape_class, fam)
            ROWS[key] = max(ROWS.get(key, 0.0), v)
    return rows


def _g(t):
    return sb.guarded(t, DEV)


# ================================================================================================ spectral norm
def sn_forward(layers, power_iterations, saved=True):
    """One ffwm_spectral_norm_forward call over all layers: shared wv and sigma buffers, every array guarded -> output dicts (CPU)."""
    from ffwm_amd.spectral_norm import _SnLayer
    L, lib = _lib()
    dt = layers[0].W.dtype
    esz = layers[0].W.element_size()
    n = len(layers)
    total_rows = sum(l.rows for l in layers)
    wv = sb.guarded_nan(total_rows, dt, DEV)
    sigma = sb.guarded_nan(n, dt, DEV)
    arr = (_SnLayer * n)()
    keep, off = [], 0
    for k, l in enumerate(layers):
        bufs = {"W": l.W.to(DEV), "u": _g(l.u), "v": _g(l.v), "weight_sn": sb.guarded_nan(l.rows * l.cols, dt, DEV),
                "u_saved": sb.guarded_nan(l.rows, dt, DEV), "v_saved": sb.guarded_nan(l.cols, dt, DEV)}
        a = arr[k]
        a.weight, a.u, a.v, a.weight_sn = bufs["W"].data_ptr(), bufs["u"].data_ptr(), bufs["v"].data_ptr(), bufs["weight_sn"].data_ptr()
        a.wv, a.sigma = wv.data_ptr() + off * esz, sigma.data_ptr() + k * esz
        a.u_saved = bufs["u_saved"].data_ptr() if saved else None
        a.v_saved = bufs["v_saved"].data_ptr() if saved else None
        a.rows, a.cols = l.rows, l.cols
        keep.append((bufs, off))
        off += l.rows
    L.check(lib.ffwm_spectral_norm_forward(ctypes.cast(arr, ctypes.c_void_p), n, power_iterations, sn.SN_EPS, L.F32 if dt == torch.float32 else L.F64,
                                           _stream()), "ffwm_spectral_norm_forward")
    torch.cuda.synchronize()
    sb.check_guards(wv, total_rows, "wv")
    sb.check_guards(sigma, n, "sigma")
    wv_c, sig_c = wv.cpu(), sigma.cpu()
    outs = []
    for k, (l, (bufs, o)) in enumerate(zip(layers, keep)):
        sizes = {"u": l.rows, "v": l.cols, "weight_sn": l.rows * l.cols, "u_saved": l.rows, "v_saved": l.cols}
        out = {"wv": wv_c[o:o + l.rows], "sigma": sig_c[k:k + 1]}
        for name, size in sizes.items():
            sb.check_guards(bufs[name], size, "layer %d %s" % (k, name))
            out[name] = bufs[name].cpu()[:size]
        out["weight_sn"] = out["weight_sn"].view(l.rows, l.cols)
        if not saved:                                                      # never written: still NaN
            assert bool(torch.isnan(out.pop("u_saved")).all()) and bool(torch.isnan(out.pop("v_saved")).all())
        outs.append(out)
    return outs


def sn_backward(layers, grads, outs):
    """One ffwm_spectral_norm_backward call from the forward's u, v, sigma -> [(dW, partials)] (CPU)."""
    from ffwm_amd.spectral_norm import _SnGradLayer
    L, lib = _lib()
    dt = layers[0].W.dtype
    esz = layers[0].W.element_size()
    n = len(layers)
    total = sum(l.chunks for l in layers)
    partials = sb.guarded_nan(total, dt, DEV)
    arr = (_SnGradLayer * n)()
    keep, off = [], 0
    for k, (l, G, o) in enumerate(zip(layers, grads, outs)):
        bufs = [l.W.to(DEV), o["u"].to(DEV), o["v"].to(DEV), o["sigma"].to(DEV), G.to(DEV).contiguous(), sb.guarded_nan(l.rows * l.cols, dt, DEV)]
        a = arr[k]
        a.weight, a.u, a.v, a.sigma, a.grad_weight_sn, a.grad_weight = (b.data_ptr() for b in bufs)
        a.partials = partials.data_ptr() + off * esz
        a.rows, a.cols = l.rows, l.cols
        keep.append((bufs, off))
        off += l.chunks
    L.check(lib.ffwm_spectral_norm_backward(ctypes.cast(arr, ctypes.c_void_p), n, L.F32 if dt == torch.float32 else L.F64, _stream()),
            "ffwm_spectral_norm_backward")
    torch.cuda.synchronize()
    sb.check_guards(partials, total, "partials")
    pc = partials.cpu()
    res = []
    for k, (l, (bufs, o)) in enumerate(zip(layers, keep)):
        sb.check_guards(bufs[5], l.rows * l.cols, "layer %d grad_weight" % k)
        res.append((bufs[5].cpu()[:l.rows * l.cols].view(l.rows, l.cols), pc[o:o + l.chunks]))
    return res


def _sn_run(layers, grads, kernel, shape_class, pi=1):
    ck = sb.Checks("%s %s pi=%d" % (kernel, shape_class, pi))
    outs = sn_forward(layers, pi)
    for l, o in zip(layers, outs):
        sn.check_forward(ck, l, o, pi)
    if pi:
        for l, G, o, (dW, partials) in zip(layers, grads, outs, sn_backward(layers, grads, outs)):
            sn.check_backward(ck, l, G, o["u"], o["v"], o["sigma"], dW, partials)
        bare = sn_forward(layers, pi, saved=False)                          # u_saved = v_saved = NULL: the same bits
        for o, b in zip(outs, bare):
            for name in b:
                ck.equal(name + " (saved NULL)", "all", b[name], o[name])
    return _finish(ck, kernel, shape_class)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sn.SN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_spectral_norm_meets_the_per_stage_bounds(shape, dtype):
    """The five families of one shape as five neighbouring layers of one call (the zero and the NaN layer between finite ones), forward
    with and without the power iteration, and the backward from the kernel's own u, v, sigma."""
    layers = sn.family_layers(shape, dtype)
    grads = [sn.make_grad(l, k) for k, l in enumerate(layers)]
    kernel = "spectral_norm_f32" if dtype == torch.float32 else "spectral_norm_f64"
    _sn_run(layers, grads, kernel, "%dx%d" % shape, 1)
    _sn_run(layers, grads, kernel, "%dx%d" % shape, 0)


@pytest.mark.parametrize("count,first", [(c, f) for c in sn.SN_COUNTS for f in (True, False)], ids=lambda v: str(v))
def test_spectral_norm_layer_counts_cross_the_batch_of_32(count, first):
    layers = sn.count_layers(count, first)
    _sn_run(layers, [sn.make_grad(l, k) for k, l in enumerate(layers)], "spectral_norm_f32", "%d layers, multi-chunk %s" % (count, "first" if first else "last"))


@pytest.mark.parametrize("n", sn.SN_EXACT_ORDERS + (1024,))
def test_spectral_norm_is_exact_on_the_hadamard_family(n):
    for dtype in (torch.float32, torch.float64):
        layer, G = sn.make_exact_layer(n, dtype)
        _sn_run([layer], [G], "spectral_norm_f32" if dtype == torch.float32 else "spectral_norm_f64", "exact %d" % n)


# ================================================================================================ flat Adam
def adam_call(p, g, m, v, cfg, step=None, state=None):
    """ffwm_adam_step (step given) or ffwm_adam_step_device (state given) on guarded device copies -> p, m, v with their guard cells."""
    L, lib = _lib()
    lr, beta1, beta2, eps = sb.ADAM_CONFIGS[cfg]
    n = p.numel()
    dp, dg, dm, dv = _g(p), _g(g), _g(m), _g(v)
    if state is None:
        L.check(lib.ffwm_adam_step(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, lr, beta1, beta2, eps, step, L.F32, _stream()), "ffwm_adam_step")
    else:
        L.check(lib.ffwm_adam_step_device(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, lr, beta1, beta2, eps, state.data_ptr(), L.F32,
                                          _stream()), "ffwm_adam_step_device")
    torch.cuda.synchronize()
    sb.check_guards(dg, n, "g")
    return dp.cpu(), dm.cpu(), dv.cpu()


def _adam_host(n, cfg, step, nan_at=(), shape_class=None):
    p, g, m, v, fam = sb.adam_inputs(n, nan_at=nan_at)
    ref = sb.AdamRef(p, g, m, v, sb.adam_scalars(cfg, step))
    ck = sb.Checks("adam n=%d %s step %d" % (n, cfg, step))
    ref.check(ck, *adam_call(p, g, m, v, cfg, step=step), fam)
    return _finish(ck, "adam_flat", shape_class or ("n<=5" if n <= 5 else "n~1024" if n < 5000 else "two sweeps"))


@pytest.mark.parametrize("cfg", list(sb.ADAM_CONFIGS))
@pytest.mark.parametrize("step", sb.ADAM_STEPS)
def test_adam_step_meets_the_per_element_bounds(cfg, step):
    for n in sb.ADAM_SIZES:
        _adam_host(n, cfg, step)


@pytest.mark.parametrize("pos", [0, 1, 2, 3, "tail"])
def test_adam_nan_gradient_stays_in_its_own_element(pos):
    for n in (7, 1027):
        _adam_host(n, "gan", 2, nan_at=(n - 1 if pos == "tail" else 4 * ((n // 4) // 2) + pos,), shape_class="NaN g")


def _device_scalars(cfg, state):
    b1, b2, e, _, _ = sb.adam_scalars(cfg, 1)
    return b1, b2, e, sb.f32(float(state[1])), sb.f32(float(state[2]))


def _adam_device_call(ck, n, cfg, state, k, lr, seed, frozen=False):
    """One device-state call from fresh inputs; its scalars are read back and held to the host's within one float32 ulp."""
    _, beta1, beta2, _ = sb.ADAM_CONFIGS[cfg]
    p, g, m, v, fam = sb.adam_inputs(n, seed=seed)
    out = adam_call(p, g, m, v, cfg, state=state)
    st = state.cpu()
    want = (sb.f32(lr / (1.0 - beta1 ** k)), sb.f32(math.sqrt(1.0 - beta2 ** k)))
    ck.require("state[0]", "device", float(st[0]) == k, "step counter %r after %d calls" % (float(st[0]), k))
    for i, w in zip((1, 2), want):
        ck.require("state[%d]" % i, "device", abs(sb.f32(float(st[i])) - w) <= sb.ulp32(w), "float32(state[%d]) = %r, host %r" % (i, sb.f32(float(st[i])), w))
    sb.AdamRef(p, g, m, v, _device_scalars(cfg, st), extra=1).check(ck, *out, fam, frozen_p=frozen)


@pytest.mark.parametrize("cfg", list(sb.ADAM_CONFIGS))
def test_adam_device_state_counts_steps_and_takes_the_lr_override(cfg):
    lr = sb.ADAM_CONFIGS[cfg][0]
    state = torch.tensor([0.0, sb.NAN, sb.NAN, -1.0], dtype=torch.float64, device=DEV)
    ck = sb.Checks("adam device state " + cfg)
    for k, n in ((1, 1025), (2, 5), (3, 1023)):
        _adam_device_call(ck, n, cfg, state, k, lr, seed=k)
    state[3] = 0.0                                                             # frozen weights: p bit-unchanged, m and v advance
    _adam_device_call(ck, 1027, cfg, state, 4, 0.0, seed=4, frozen=True)
    state[3] = 3.0 * lr                                                        # the next call picks the new rate up
    _adam_device_call(ck, 1027, cfg, state, 5, 3.0 * lr, seed=5)
    _finish(ck, "adam_flat_device", "n~1024")


@pytest.mark.parametrize("entry", ["host", "device"])
def test_adam_second_grid_stride_sweep_and_tail(entry):
    if entry == "host":
        _adam_host(sb.ADAM_BIG, "gan", 2)
    else:
        state = torch.tensor([1.0, sb.NAN, sb.NAN, -1.0], dtype=torch.float64, device=DEV)
        ck = sb.Checks("adam device two sweeps")
        _adam_device_call(ck, sb.ADAM_BIG, "gan", state, 2, sb.ADAM_CONFIGS["gan"][0], seed=0)
        _finish(ck, "adam_flat_device", "two sweeps")


# ================================================================================================ fused L1
@functools.lru_cache(maxsize=None)
def _l1_cases():
    return sb.l1_cases()


def _shifted(t, off, copy=True):
    """A NaN-filled device buffer and its view from element `off` on (0: 16-byte aligned): t's values (copy) and the guard cells."""
    buf = torch.full((off + t.numel() + sb.GUARD,), sb.NAN, device=DEV)
    if copy:
        buf[off:off + t.numel()] = t.to(DEV)
    return buf, buf[off:]


def l1_call(problems, n_slots, out0=None, gout=None):
    """Forward (out0 given) or backward (gout given) -> the guarded result vector, or the guarded grad_x per problem."""
    from ffwm_amd.ops import _L1Problem
    L, lib = _lib()
    arr = (_L1Problem * len(problems))()
    keep, gxs = [], []
    for a, pr in zip(arr, problems):
        xb, x = _shifted(pr.x, pr.x_off)
        yb, y = _shifted(pr.y, pr.x_off)
        keep += [xb, yb]
        a.x, a.y, a.n, a.scale, a.slot = x.data_ptr(), y.data_ptr(), pr.n, pr.scale, pr.slot
        a.chw, a.hw = (pr.chw, pr.hw) if pr.mask is not None else (1, 1)
        if pr.mask is not None:
            mb, mk = _shifted(pr.mask, pr.m_off)
            keep.append(mb)
            a.mask = mk.data_ptr()
        if gout is not None:
            gb, gx = _shifted(pr.x, pr.x_off, copy=False)
            keep.append(gb)
            a.grad_x = gx.data_ptr()
            gxs.append(gx)
    out = None if out0 is None else _g(out0)
    go = None if gout is None else gout.to(DEV)
    L.check(lib.ffwm_l1_multi(ctypes.cast(arr, ctypes.c_void_p), len(problems), None if out is None else out.data_ptr(),
                              None if go is None else go.data_ptr(), n_slots, L.F32, _stream()), "ffwm_l1_multi")
    torch.cuda.synchronize()
    return out.cpu() if gout is None else [gx.cpu() if pr.n else None for gx, pr in zip(gxs, problems)]


L1_NAMES = ["n%d" % n for n in sb.L1_SIZES] + ["masks"] + ["count%d" % c for c in sb.L1_COUNTS] + ["one_slot40"]


@pytest.mark.parametrize("name", L1_NAMES)
def test_l1_multi_forward_bound_and_bit_exact_backward(name):
    problems, n_slots = _l1_cases()[name]
    out0 = torch.arange(n_slots, dtype=torch.float32) * 0.25 - 0.25            # the call must ADD to what the vector holds
    gout = torch.tensor([1.5, -0.75, 2.0, 0.0, 0.3][:n_slots])
    ref = sb.L1Ref(problems, n_slots, out0, gout)
    ck = sb.Checks("l1 " + name)
    ref.check_forward(ck, l1_call(problems, n_slots, out0=out0), family=name)
    ref.check_backward(ck, l1_call(problems, n_slots, gout=gout))
    _finish(ck, "l1_multi", name)


# ================================================================================================ correlation column maximum
def corr_call(s, t):
    L, lib = _lib()
    B, N, C = s.shape
    ds, dt = s.to(DEV).contiguous(), t.to(DEV).contiguous()
    out = sb.guarded_nan(B * N, torch.float32, DEV)
    L.check(lib.ffwm_correlation_colmax(ds.data_ptr(), dt.data_ptr(), out.data_ptr(), B, N, C, L.F32, _stream()), "ffwm_correlation_colmax")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("shape", sb.CORR_SHAPES, ids=lambda s: "B%d-N%d-C%d" % s)
def test_correlation_colmax_meets_the_mfma_chain_bound(shape):
    s, t = sb.corr_inputs(*shape)
    ck = sb.Checks("corr %s" % (shape,))
    sb.CorrRef(s, t).check(ck, corr_call(s, t))
    _finish(ck, "correlation_colmax", "N=%d C=%d" % shape[1:])


@pytest.mark.parametrize("N,C", [(1, 64), (31, 64), (33, 128), (129, 64), (160, 256)])
def test_correlation_colmax_is_exact_on_sparse_integers(N, C):
    s, t, planted = sb.corr_exact_inputs(N, C)
    ref = sb.require_exact(sb.CorrRef(s, t).out).float()
    out = corr_call(s, t)
    sb.check_guards(out, N, "out")
    ck = sb.Checks("corr exact N=%d C=%d" % (N, C))
    ck.equal("colmax", "exact", out[:N].view(1, N), ref)
    _finish(ck, "correlation_colmax", "N=%d C=%d" % (N, C))


@pytest.mark.parametrize("N,C", [(33, 64), (160, 128)])
def test_correlation_colmax_keeps_nan_and_minus_inf_as_torch_max_does(N, C):
    s, t = sb.corr_nonfinite_inputs(N, C)
    ck = sb.Checks("corr non-finite N=%d C=%d" % (N, C))
    sb.corr_nonfinite_check(ck, s, t, corr_call(s, t))
    _finish(ck, "correlation_colmax", "N=%d C=%d" % (N, C))


# ------------------------------------------------------------------------------------------------ the record
def _time_colmax(lib, check, runs=3, launches=20):
    """avg ms of the profiler row correlation_colmax at (1, 4096, 128), `runs` times."""
    g = torch.Generator().manual_seed(1)
    s, t = torch.randn(1, 4096, 128, generator=g).to(DEV), torch.randn(1, 128, 4096, generator=g).to(DEV)
    out = torch.empty(1, 4096, device=DEV)
    name, launched, ms, nbytes = ctypes.create_string_buffer(128), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    res = []
    for _ in range(runs):
        for phase in ("warm", "timed"):
            lib.ffwm_prof_enable(1 if phase == "timed" else 0)
            lib.ffwm_prof_reset()
            for _ in range(5 if phase == "warm" else launches):
                check(lib.ffwm_correlation_colmax(s.data_ptr(), t.data_ptr(), out.data_ptr(), 1, 4096, 128, 0, _stream()))
            torch.cuda.synchronize()
        for i in range(lib.ffwm_prof_collect()):
            lib.ffwm_prof_get(i, name, 128, ctypes.byref(launched), ctypes.byref(ms), ctypes.byref(nbytes))
            if name.value == b"correlation_colmax":
                res.append(ms.value / max(launched.value, 1))
        lib.ffwm_prof_enable(0)
    return res


def _report(path, parent_lib=None):
    L, lib = _lib()
    this = sys.modules[__name__]
    failed = []
    for name in sorted(dir(this)):
        fn = getattr(this, name)
        if not name.startswith("test_") or not callable(fn):
            continue
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        cases = [()]
        for m in marks:
            keys = [k.strip() for k in m.args[0].split(",")]
            cases = [c + ((v if len(keys) > 1 else (v,)),) for c in cases for v in m.args[1]]
        for c in cases:
            try:
                fn(*_ordered(fn, marks, c))
            except AssertionError as e:
                failed.append("%s%s: %s" % (name, c, str(e)[:300]))
    times = {"change": _time_colmax(lib, lambda rc: L.check(rc, "ffwm_correlation_colmax"))}
    if parent_lib:
        other = ctypes.CDLL(os.path.abspath(parent_lib))
        for fname in ("ffwm_correlation_colmax", "ffwm_prof_get"):
            getattr(other, fname).argtypes = getattr(lib, fname).argtypes

        def ok(rc):
            assert rc == 0, rc
        a, b = [], []
        for _ in range(3):                                                     # interleaved: parent, change, parent, change, ...
            a += _time_colmax(other, ok, runs=1)
            b += _time_colmax(lib, lambda rc: L.check(rc, "ffwm_correlation_colmax"), runs=1)
        times = {"parent": a, "change": b}
    lines = ["# worst |got - ref| / bound per kernel, stage, shape class and family (tests/step_bounds.py, tests/step_bounds_sn.py, SAFETY = %g);" % sb.SAFETY,
             "# 0 on an `equal` / exact row = bit for bit.  Written by `python tests/test_gpu_step_bounds.py --report` on %s." % torch.cuda.get_device_name(0),
             "%-20s %-22s %-34s %-18s %s" % ("kernel", "stage", "shape class", "family", "error/bound")]
    for (kernel, stage, shape_class, fam), v in sorted(ROWS.items()):
        lines.append("%-20s %-22s %-34s %-18s %.4f" % (kernel, stage, shape_class, fam, v))
    worst = max(ROWS.values())
    lines.append("# worst of all: %.4f over %d rows; failures: %d" % (worst, len(ROWS), len(failed)))
    lines += ["# FAILED " + f for f in failed]
    lines.append("# correlation_colmax at (B, N, C) = (1, 4096, 128), profiler row, avg ms of 20 launches, three runs each:")
    for who, vals in times.items():
        lines.append("#   %-7s %s   median %.4f  spread %.4f .. %.4f" % (who, "  ".join("%.4f" % v for v in vals), sorted(vals)[len(vals) // 2], min(vals), max(vals)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if worst <= 1.0 and not failed else 1


def _ordered(fn, marks, case):
    """Arguments by name: stacked parametrize marks list the innermost decorator first."""
    import inspect
    values = {}
    for m, grp in zip(marks, case):
        for k, v in zip([k.strip() for k in m.args[0].split(",")], grp):
            values[k] = v
    return [values[p] for p in inspect.signature(fn).parameters]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = sys.argv[1:]
    if len(args) in (2, 4) and args[0] == "--report" and (len(args) == 2 or args[2] == "--parent-lib"):
        sys.exit(_report(args[1], args[3] if len(args) == 4 else None))
    sys.exit("usage: test_gpu_step_bounds.py --report FILE [--parent-lib LIB]")
