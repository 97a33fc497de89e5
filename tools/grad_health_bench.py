"""What gradient health (csrc/grad_health.hip + the guarded Adam step of csrc/adam.hip) costs, measured two ways on an MI355X:

    python tools/grad_health_bench.py [--pairs 5] [--out profiles/grad_health.txt]

(a) One optimizer range, at the sizes of the three ranges of the batch-8 train step (opt_F, opt_G, opt_D of FFWMTrainer), as device
    time inside a captured graph:
        A  the composition a user would otherwise write: torch.linalg.vector_norm(g), torch.isfinite(g).all(), the clip multiply
           into a scratch array, ffwm_adam_step_device.  (Inside a graph A can only COMPUTE the finite flag: acting on it needs a
           host read, which is what the guard is there to avoid.)
        B  ffwm_grad_health + ffwm_adam_step_guarded (skip_nonfinite on, max_norm 1.0).
        H  ffwm_grad_health alone, also as GB/s over its 4 n bytes.
    Each leg is `calls` evaluations captured into one graph, the replay timed with device events; A and B alternate for --pairs
    pairs, reported as median and min-max.
(b) The captured FFWMTrainer step at batch 8 of two trainers of one seed, grad_health / skip_nonfinite off and on, replayed in
    alternating windows of --steps steps, reported the same way.
Every GPU step is a child process under its own time limit; the parent never opens the GPU, stops at the first step that fails
and writes what it has.  The feature switches no default: the numbers report a cost and gate nothing.  GPU only.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abtime import captured, line  # noqa: E402

DEV = "cuda:0"
LIMITS = {"a": 420, "b": 540}          # seconds per child
LR, B1, B2, EPS, MAX_NORM = 4e-4, 0.5, 0.999, 1e-8, 1.0


def part_a(args):
    import torch
    from ffwm_amd import _lib, trainer
    L = _lib.load()
    t = trainer.FFWMTrainer(DEV, seed=0)
    sizes = [(k, getattr(t, k).n) for k in ("opt_F", "opt_G", "opt_D")]
    del t
    torch.cuda.empty_cache()
    print("# (a) one optimizer range of the batch-8 train step, float32, device %s; A = vector_norm + isfinite().all() + clip multiply + "
          "ffwm_adam_step_device, B = ffwm_grad_health + ffwm_adam_step_guarded, H = ffwm_grad_health alone" % torch.cuda.get_device_name(0))
    print("#     %d evaluations per captured graph, median of 5 replays per run, %d alternating pairs" % (args.calls, args.pairs))
    for name, n in sizes:
        gen = torch.Generator(device=DEV).manual_seed(3)
        p = torch.randn(n, device=DEV, generator=gen)
        g = torch.randn(n, device=DEV, generator=gen) * 1e-3
        m, v, scaled = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
        state = {w: torch.tensor([0.0, 0.0, 0.0, -1.0], dtype=torch.float64, device=DEV) for w in "AB"}
        seg_end = torch.tensor([n], dtype=torch.int64, device=DEV)
        record, guard = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
        ws_bytes = L.ffwm_grad_health_workspace_bytes(n, 1)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
        keep = {}

        def stream():
            return torch.cuda.current_stream().cuda_stream

        def leg_a():
            norm = torch.linalg.vector_norm(g)
            keep["finite"] = torch.isfinite(g).all()
            torch.mul(g, torch.clamp(MAX_NORM / (norm + 1e-6), max=1.0), out=scaled)
            _lib.check(L.ffwm_adam_step_device(p.data_ptr(), scaled.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS,
                                               state["A"].data_ptr(), _lib.F32, stream()), "ffwm_adam_step_device")

        def leg_h():
            _lib.check(L.ffwm_grad_health(g.data_ptr(), n, seg_end.data_ptr(), 1, ws.data_ptr(), ws_bytes, record.data_ptr(), _lib.F32,
                                          stream()), "ffwm_grad_health")

        def leg_b():
            leg_h()
            _lib.check(L.ffwm_adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS,
                                                state["B"].data_ptr(), record.data_ptr(), 1, MAX_NORM, 1, guard.data_ptr(), _lib.F32,
                                                stream()), "ffwm_adam_step_guarded")

        ra, rb, rh = captured(leg_a, args.calls), captured(leg_b, args.calls), captured(leg_h, args.calls)
        ms = {"A": [], "B": [], "H": []}
        for _ in range(args.pairs):
            ms["A"].append(ra())
            ms["B"].append(rb())
            ms["H"].append(rh())
        tag = "%s n=%d" % (name, n)
        print(line("%s  A (composition)   " % tag, ms["A"], "us", 1e3))
        print(line("%s  B (health + guard)" % tag, ms["B"], "us", 1e3))
        print(line("%s  H (health alone)  " % tag, ms["H"], "us", 1e3))
        gbs = [4.0 * n / (x * 1e-3) / 1e9 for x in ms["H"]]
        print("%s  H reads 4 n = %.1f MB: median %.0f GB/s  min %.0f  max %.0f" % (tag, 4e-6 * n, statistics.median(gbs), min(gbs), max(gbs)))
        margin = statistics.median(ms["A"]) - statistics.median(ms["B"])
        worst = max(max(ms["A"]) - min(ms["A"]), max(ms["B"]) - min(ms["B"]))
        print("%s  A - B = %.3f us against the larger min-max spread %.3f us: B is %s; A / B = %.2f" % (
            tag, 1e3 * margin, 1e3 * worst, "below the composition by more than the spread" if margin > worst else
            ("NOT below the composition by more than the spread" if margin >= -worst else "SLOWER than the composition beyond the spread"),
            statistics.median(ms["A"]) / statistics.median(ms["B"])), flush=True)
        del ra, rb, rh


def part_b(args):
    import torch
    from ffwm_amd import trainer
    B = 8
    batch = trainer.synthetic_batch(B, DEV, seed=1)
    trainers = {}
    for on in (False, True):
        t = trainer.FFWMTrainer(DEV, seed=0, capturable=True, grad_health=on, skip_nonfinite=on)
        t.capture(batch, warmup=3)
        trainers[on] = t
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(t):
        t.step(batch, batch_increment=0)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.steps):
            t.step(batch, batch_increment=0)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.steps
    step = {False: [], True: []}
    for _ in range(args.pairs):
        for on in (False, True):
            step[on].append(window(trainers[on]))
    print("# (b) the captured FFWMTrainer step at batch %d, two trainers of one seed, %d steps per window, %d alternating pairs" % (
        B, args.steps, args.pairs))
    print(line("step  grad_health off", step[False], "ms"))
    print(line("step  grad_health on ", step[True], "ms"))
    margin = statistics.median(step[True]) - statistics.median(step[False])
    worst = max(max(v) - min(v) for v in step.values())
    print("step  on - off = %.3f ms against the larger min-max spread %.3f ms: %s" % (
        margin, worst, "the overhead is inside the spread" if abs(margin) <= worst else
        ("the guarded step is slower beyond the spread" if margin > 0 else "the guarded step is FASTER beyond the spread")))
    h = trainers[True].health()
    print("step  health() of the last replay: " + "; ".join(
        "%s norm %.4g max %.3g nonfinite %d" % (k, h[k]["norm"], h[k]["max_abs"], h[k]["nonfinite"]) for k in ("flowNetF", "flowNetB", "netG", "netD")))
    print("step  " + "; ".join("%s applied %d skipped %d" % (k, h[k]["steps_applied"], h[k]["steps_skipped"]) for k in ("opt_F", "opt_G", "opt_D")),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="evaluations per captured graph")
    ap.add_argument("--steps", type=int, default=10, help="train steps per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_health.txt"))
    ap.add_argument("--part", choices=("a", "b"), help="run one GPU step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.pairs < 5:
        sys.exit("grad_health_bench: at least five pairs")
    if args.part:
        import torch
        if not torch.cuda.is_available():
            sys.exit("grad_health_bench: needs an MI355X; a CPU run measures nothing")
        return part_a(args) if args.part == "a" else part_b(args)

    lines = []
    common = [sys.executable, os.path.abspath(__file__), "--pairs", str(args.pairs), "--calls", str(args.calls), "--steps", str(args.steps)]
    status = 0
    for part in ("a", "b"):
        try:
            r = subprocess.run(common + ["--part", part], capture_output=True, text=True, timeout=LIMITS[part], cwd=ROOT)
            text, status = r.stdout, r.returncode
            if status != 0:
                text += "grad_health_bench: part %s ended with status %d\n%s\n" % (part, status, r.stderr[-2000:])
        except subprocess.TimeoutExpired as e:
            text = (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout or "") \
                + "grad_health_bench: part %s passed its limit of %d s\n" % (part, LIMITS[part])
            status = 124
        print(text, end="", flush=True)
        lines.append(text)
        if status != 0:
            break              # nothing more is started on the GPU after a step that failed
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(lines))
    sys.exit(status)


if __name__ == "__main__":
    main()
