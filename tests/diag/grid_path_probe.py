"""Grid paths: evaluate.path_optimality for 1024 queries at n = 65 on the speed grid of the
bench's 20 000-triangle synthetic obstacle mesh (the mesh of eikonal_grid_probe.py).  The
"planned" paths are straight polylines of 2 x 101 points between Gibson-style start / goal pairs
(synth.make_pairs): the probe times the evaluation, not a planner.  Per chunk of 64 queries it
prints the time of the grid solve (ops.grid_travel_time, host loop included), of the descent
kernel and of the polyline-time kernel on the descent's output (HIP events, median over the
chunks), then the polyline-time kernel on all planned paths and the wall time of the whole
path_optimality call with the solver's share of it.  One GPU process, own warm-up.

    python tests/diag/grid_path_probe.py > profiles/grid_path_probe.txt
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-ntfields_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pntf import evaluate, ops, synth  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--tris", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=101)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(9)
    tris = ((torch.rand(a.tris, 1, 3, generator=g) - 0.5) * 0.8
            + torch.randn(a.tris, 3, 3, generator=g) * 0.02).to(dev)
    xp = torch.from_numpy(synth.make_pairs(a.queries, 3, seed=11)).to(dev)
    t = torch.linspace(0.0, 0.5, a.rows, device=dev)[None, :, None]
    mid = 0.5 * (xp[:, None, :3] + xp[:, None, 3:])
    path = torch.cat([xp[:, None, :3] + 2 * t * (mid - xp[:, None, :3]),
                      xp[:, None, 3:] + 2 * t * (mid - xp[:, None, 3:])], dim=2).contiguous()
    steps = torch.full((a.queries,), a.rows - 1, dtype=torch.int32, device=dev)
    margin = evaluate.GIBSON_MARGIN
    n, q = a.n, a.queries
    S = ops.speed_grid(tris, n, margin / 10, margin)
    print("grid_path_probe: n = %d, q = %d queries in chunks of %d, %d triangles; %s"
          % (n, q, a.chunk, a.tris, torch.cuda.get_device_name(dev)))
    src, goal = path[:, 0, :3].contiguous(), path[:, 0, 3:].contiguous()
    sl = slice(0, a.chunk)                                          # warm-up: one chunk
    T, _, _ = ops.grid_travel_time(S, src[sl])
    d = ops.grid_descent(T, src[sl], goal[sl])
    ops.grid_polyline_time(S, d[0], d[1])
    torch.cuda.synchronize()
    rows, status, counts = [], [], []
    for lo in range(0, q, a.chunk):
        sl = slice(lo, min(lo + a.chunk, q))
        (T, passes, conv), ms_solve = timed(lambda: ops.grid_travel_time(S, src[sl]))
        d, ms_desc = timed(lambda: ops.grid_descent(T, src[sl], goal[sl]))
        _, ms_time = timed(lambda: ops.grid_polyline_time(S, d[0], d[1]))
        rows.append((ms_solve, ms_desc, ms_time, int(passes.max()), bool(conv.all())))
        status.append(d[2].cpu())
        counts.append(d[1].cpu())
    r = np.array([x[:3] for x in rows])
    status, counts = torch.cat(status).numpy(), torch.cat(counts).numpy()
    print("per chunk of %d (median, min, max over %d chunks), ms: solve %.3f (%.3f, %.3f), "
          "descent kernel %.4f (%.4f, %.4f), polyline-time kernel on the descent %.4f (%.4f, %.4f)"
          % (a.chunk, len(rows), np.median(r[:, 0]), r[:, 0].min(), r[:, 0].max(),
             np.median(r[:, 1]), r[:, 1].min(), r[:, 1].max(), np.median(r[:, 2]),
             r[:, 2].min(), r[:, 2].max()))
    print("passes per chunk %s, all converged %s" % (sorted(set(x[3] for x in rows)),
                                                     all(x[4] for x in rows)))
    print("descent status counts (ARRIVED, TRUNCATED, STALLED, BLOCKED, UNREACHABLE): %s; "
          "points per path: median %d, max %d of L = %d"
          % (np.bincount(status, minlength=5).tolist(), int(np.median(counts)), int(counts.max()),
             d[0].shape[1]))
    pp, pc = ops.plan_polylines(path, steps)
    _, ms_plan = timed(lambda: ops.grid_polyline_time(S, pp, pc))
    print("polyline-time kernel on all %d planned paths of %d points: %.4f ms"
          % (q, int(pc[0]), ms_plan))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = evaluate.path_optimality(path, steps, tris, n=n, chunk=a.chunk)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    solve = r[:, 0].sum()
    print("path_optimality, whole call: %.1f ms wall; the solver's chunks sum to %.1f ms = %.1f %% "
          "of it, the descent kernels to %.2f ms, the polyline-time kernels to %.2f ms"
          % (wall, solve, 100.0 * solve / wall, r[:, 1].sum(), r[:, 2].sum() + ms_plan))
    ok = torch.isfinite(rep.time_ratio)
    if bool(ok.any()):
        print("rows defined %d of %d; time_ratio median %.4f, floor_rel median %.4f, max %.4f"
              % (int(ok.sum()), q, float(rep.time_ratio[ok].median()),
                 float(rep.floor_rel[ok].median()), float(rep.floor_rel[ok].max())))
    else:
        print("no row defined")


if __name__ == "__main__":
    main()
