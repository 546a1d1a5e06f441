"""Grid travel time: ops.grid_travel_time at n = 129 for q = 8 sources on the speed grid
(ops.speed_grid, the Gibson margin) of the bench's 20 000-triangle synthetic obstacle mesh
(bench.py mesh_extras; the same mesh as path_clearance_probe.py).  Prints the pass count, the
wall time of a whole solve (host loop and its synchronisations included, HIP events around the
call), the time per pass and the HBM traffic that pass count implies at 2·4·n^3 bytes per
source per pass (one read and one write of T; the speed grid and the halo re-reads come on top),
for several (inner, check_every).  One GPU process, own warm-up, median of the timed runs.

    python tests/diag/eikonal_grid_probe.py [--runs 5] > profiles/eikonal_grid_probe.txt
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-ntfields_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pntf import evaluate, ops  # noqa: E402


def median_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=129)
    ap.add_argument("--sources", type=int, default=8)
    ap.add_argument("--tris", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(9)
    tris = ((torch.rand(a.tris, 1, 3, generator=g) - 0.5) * 0.8
            + torch.randn(a.tris, 3, 3, generator=g) * 0.02).to(dev)
    src = ((torch.rand(a.sources, 3, generator=g) - 0.5) * 0.9).to(dev)
    margin = evaluate.GIBSON_MARGIN
    n, q = a.n, a.sources
    med, lo, hi = median_ms(lambda: ops.speed_grid(tris, n, margin / 10, margin), a.warmup, a.runs)
    S = ops.speed_grid(tris, n, margin / 10, margin)
    print("eikonal_grid_probe: n = %d (%d nodes), q = %d sources, %d triangles; %s"
          % (n, n ** 3, q, a.tris, torch.cuda.get_device_name(dev)))
    print("speed grid: median %.3f ms (min %.3f, max %.3f); speed %.3g .. %.3g, %.1f %% of the "
          "nodes below 1" % (med, lo, hi, float(S.min()), float(S.max()),
                             100.0 * float((S < 1).double().mean())))
    base = None
    for inner, every in ((8, 4), (8, 1), (4, 4), (16, 4), (1, 16)):
        T, passes, conv = ops.grid_travel_time(S, src, inner=inner, check_every=every)
        if base is None:
            base = T
        same = bool(torch.equal(T.view(torch.int32), base.view(torch.int32)))
        p = int(passes.max())
        med, lo, hi = median_ms(lambda: ops.grid_travel_time(S, src, inner=inner,
                                                             check_every=every), a.warmup, a.runs)
        gb = 2 * 4 * n ** 3 * q * p / 1e9
        print("inner %2d check_every %2d: converged %s, passes %d (per source %s), T up to %.3g, "
              "bits equal to the first row's %s; median %.3f ms (min %.3f, max %.3f, %d runs), "
              "%.4f ms per pass; %.2f GB of T traffic = %.0f GB/s"
              % (inner, every, bool(conv.all()), p, passes.tolist(),
                 float(T[torch.isfinite(T)].max()), same, med, lo, hi, a.runs, med / p, gb,
                 gb / (med / 1e3)))


if __name__ == "__main__":
    main()
