"""guided filter fwd + bwd of the train step's call ([8,3,128,128], r = 32): HIP-event time per direction (GF_NOPROF=1: no
events, for tools/gf_trace.sh).

``--general``: the shapes beyond that call -- [8,3,256,256] r = 32, [8,3,512,512] r = 32 and r = 64, and the second one with a
one-channel guide -- forward and forward + backward with both gradients, against ``nets.GuidedFilter`` (the PyTorch restatement a
user had to fall back to) on the same GPU, in the same process, alternating.  Prints one row per shape: microseconds (median of
the rounds, torch events around `iters` calls), the ratio, and the fraction of the HBM peak by algorithmic bytes (x, y in,
out out forward; x, y, g in, out, grad_x, grad_y out for forward + backward)."""
import os, torch, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffwm_amd import ops, _lib

HBM_PEAK = 8.0e12      # bytes / s, MI355X


def train_step_call():
    x = torch.rand(8, 3, 128, 128, device="cuda"); y = torch.rand_like(x); go = torch.rand_like(x)
    for _ in range(3):
        out, saved = ops.guided_filter_forward(x, y, 32); gx = ops.guided_filter_backward(x, y, saved, go, 32)
    torch.cuda.synchronize(); _lib.prof_reset(); _lib.prof_enable(os.environ.get("GF_NOPROF") != "1")
    for _ in range(20):
        out, saved = ops.guided_filter_forward(x, y, 32); gx = ops.guided_filter_backward(x, y, saved, go, 32)
    torch.cuda.synchronize(); _lib.prof_enable(False)
    print({k: round(v["avg_ms"] * 1e3, 1) for k, v in _lib.prof_collect().items()})


GENERAL = [
    # (B, Cx, Cy, H, W, r)
    (8, 3, 3, 256, 256, 32),
    (8, 3, 3, 512, 512, 32),
    (8, 3, 3, 512, 512, 64),
    (8, 1, 3, 512, 512, 32),
]


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def general(rounds=5, iters=10):
    from ffwm_amd import nets
    from ffwm_amd.external_function import GuidedFilter
    print("# shape (B,Cx,Cy,H,W,r)      pass      hip us   torch us   torch/hip   hip fraction of HBM peak (algorithmic bytes)")
    for case in GENERAL:
        B, Cx, Cy, H, W, r = case
        x = torch.rand(B, Cx, H, W, device="cuda"); y = torch.rand(B, Cy, H, W, device="cuda"); go = torch.rand_like(y)
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        hip, ref = GuidedFilter(r), nets.GuidedFilter(r)

        def fwd(m):
            with torch.no_grad():
                m(x, y)

        def fwd_bwd(m):
            xg.grad = yg.grad = None
            m(xg, yg).backward(go)

        px, py = x.numel() * 4, y.numel() * 4
        for name, fn, nbytes in (("fwd", fwd, px + 2 * py), ("fwd+bwd", fwd_bwd, 2 * px + 4 * py)):
            for m in (hip, ref):
                fn(m)                                       # warm-up: allocator, library
            t = {hip: [], ref: []}
            for _ in range(rounds):                         # alternating, same process
                for m in (hip, ref):
                    t[m].append(_time(lambda: fn(m), iters))
            th, tr = sorted(t[hip])[rounds // 2], sorted(t[ref])[rounds // 2]
            print("%-28s %-8s %8.1f %10.1f %10.1fx   %.3f" % (case, name, th, tr, tr / th, nbytes / (th * 1e-6) / HBM_PEAK))


if __name__ == "__main__":
    if "--general" in sys.argv:
        general()
    else:
        train_step_call()
