"""Planned-path clearance: the polyline -> mesh kernel (ops.polyline_mesh_distance) on a batch
the planner's size — 1024 polylines of 1004 points (max_iter 500: 2·(500 + 2)) — over the
bench's 20 000-triangle synthetic obstacle mesh (bench.py mesh_extras).  For scale, the point
kernel (ops.point_mesh_distance) on the same polylines' vertices alone: the cost of the cheapest
sampled check, one sample per segment, which misses a wall between two vertices.  Paths are
straight start -> goal lines with a smooth sideways wave, in three sets of length up to 0.05,
0.3 and 1.0 (the longer the path, the likelier it passes through a triangle).
One GPU process, own warm-up, median of the timed runs (HIP events).

    python tests/diag/path_clearance_probe.py [--runs 11] > profiles/path_clearance_probe.txt
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-ntfields_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pntf import ops  # noqa: E402


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


def make_paths(q, L, reach, g):
    start = (torch.rand(q, 1, 3, generator=g) - 0.5) * 0.9
    d = torch.randn(q, 1, 3, generator=g)
    goal = (start + d / d.norm(dim=2, keepdim=True) * reach * torch.rand(q, 1, 1, generator=g))
    goal = goal.clamp(-0.45, 0.45)
    u = torch.linspace(0, 1, L)[None, :, None]
    side = torch.randn(q, 1, 3, generator=g) * 0.02
    return start + u * (goal - start) + side * torch.sin(3.0 * np.pi * u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--points", type=int, default=1004)
    ap.add_argument("--tris", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=11)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(9)
    tris = ((torch.rand(a.tris, 1, 3, generator=g) - 0.5) * 0.8
            + torch.randn(a.tris, 3, 3, generator=g) * 0.02).to(dev)
    cnt = torch.full((a.paths,), a.points, dtype=torch.int32, device=dev)
    pairs = a.paths * (a.points - 1) * a.tris
    print("path_clearance_probe: %d polylines x %d points x %d triangles = %.3g segment-triangle "
          "pairs; %s" % (a.paths, a.points, a.tris, pairs, torch.cuda.get_device_name(dev)))
    for reach in (0.05, 0.3, 1.0):
        pts = make_paths(a.paths, a.points, reach, g).to(dev)
        flat = pts.reshape(-1, 3)
        d, w = ops.polyline_mesh_distance(pts, cnt, tris)
        v = ops.point_mesh_distance(flat, tris).reshape(a.paths, a.points).amin(1)
        assert bool((d <= v).all())
        hit = d == 0
        print("reach %.2f: %d of %d paths pass through a triangle, of which the vertices alone "
              "miss %d (smallest vertex distance of those: median %.3g); clear paths: median "
              "clearance %.3g" % (reach, int(hit.sum()), a.paths, int((hit & (v > 0)).sum()),
                                  float(v[hit].median()) if hit.any() else float("nan"),
                                  float(d[~hit].median()) if (~hit).any() else float("nan")))
        for name, fn in (("polyline kernel (exact)", lambda: ops.polyline_mesh_distance(pts, cnt, tris)),
                         ("polyline kernel cap=0.05", lambda: ops.polyline_mesh_distance(pts, cnt, tris, cap=0.05)),
                         ("point kernel on the vertices + amin", lambda: ops.point_mesh_distance(
                             flat, tris).reshape(a.paths, a.points).amin(1))):
            med, lo, hi = median_ms(fn, a.warmup, a.runs)
            print("  %-38s median %9.3f ms  (min %.3f, max %.3f, %d runs)"
                  % (name, med, lo, hi, a.runs))


if __name__ == "__main__":
    main()
