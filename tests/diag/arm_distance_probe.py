"""Arm -> mesh distance: the fused kernel (ops.arm_mesh_distance: FK + distance + minimum in
one launch) against the un-fused route (torch posing of the n x V cloud, ops.point_mesh_distance
with its Morton sort, amin per configuration) on the reference's own batch
(dataprocessing/speed_sampling_gpu.py:156: 50 000 configurations): a 6-revolute chain with
3 000 link vertices (500 per link) beside a 2 000-triangle obstacle, and the same with the
sampler's cap.  One GPU process, own warm-up, median of the timed runs (HIP events).

    python tests/diag/arm_distance_probe.py [--configs 50000] [--runs 11] \
        > profiles/arm_distance_probe.txt
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "p-ntfields_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import arm_oracle as A  # noqa: E402
from pntf import kin, ops  # noqa: E402


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
    ap.add_argument("--configs", type=int, default=50000)
    ap.add_argument("--verts", type=int, default=500, help="vertices per link (6 links)")
    ap.add_argument("--tris", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--cap", type=float, default=0.2, help="the sampler's 2·margin")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    spec = A.random_chain(rng, 6)
    chain = kin.SerialChain.from_arrays(A.origin_matrices(spec), [s[2] for s in spec],
                                        [s[3] for s in spec])
    dev = torch.device("cuda:0")
    th = torch.from_numpy(A.random_theta(rng, spec, a.configs).astype(np.float32)).to(dev)
    V = [torch.zeros((0, 3), device=dev)] + [
        torch.from_numpy(A.link_blob(rng, a.verts).astype(np.float32)).to(dev) for _ in range(6)]
    # small clustered triangles, as an obstacle mesh has them
    tris = torch.from_numpy(A.boxed_mesh(rng, a.tris, scale=0.03).astype(np.float32)).to(dev)
    nv = sum(v.shape[0] for v in V)

    def fused(cap=None):
        return ops.arm_mesh_distance(th, chain, V, tris, cap=cap)

    def unfused():
        fk = chain.forward_kinematics(th)
        cloud = torch.cat([torch.einsum("nij,vj->nvi", fk[:, f, :, :3], v) + fk[:, f, None, :, 3]
                           for f, v in enumerate(V) if v.shape[0]], dim=1)
        return ops.point_mesh_distance(cloud.reshape(-1, 3), tris).reshape(a.configs, nv).amin(1)

    diff = (fused() - unfused()).abs().max().item()
    capped = torch.equal(fused(a.cap), fused().clamp(max=a.cap))
    pairs = a.configs * nv * a.tris
    print("arm_distance_probe: %d configurations x %d vertices (6 links) x %d triangles = %.3g "
          "point-triangle pairs; %s" % (a.configs, nv, a.tris, pairs,
                                        torch.cuda.get_device_name(dev)))
    print("max |fused - unfused| = %.3g; capped == min(exact, cap) bitwise: %s" % (diff, capped))
    for name, fn in (("fused", fused), ("fused cap=%g" % a.cap, lambda: fused(a.cap)),
                     ("unfused (torch FK + point kernel + amin)", unfused)):
        med, lo, hi = median_ms(fn, a.warmup, a.runs)
        print("%-42s median %9.2f ms  (min %.2f, max %.2f, %d runs)  %.3g pairs/s"
              % (name, med, lo, hi, a.runs, pairs / (med * 1e-3)))


if __name__ == "__main__":
    main()
