"""Recorded bits of the three mesh-distance kernels (needs an MI355X and a built libpntf.so).

    python tests/golden/make_mesh_family_goldens.py [--out tests/golden]

Writes mesh_family_bits.npz: the inputs of tests/test_mesh_family_bits.py and, under "bits/",
what the library in the tree gives for them as raw uint32 / int32 bit patterns.  Run it at the
commit whose bits are to be kept — it was run once, at the last commit at which each kernel had
its own fill and finalize passes — and never to make a failing test pass.

Scenes, from the builders of the three kernels' own tests: one mesh of 257 triangles
(arm_oracle.boxed_mesh, small triangles all over the box), of which one is made flat and the
last — the whole second LDS tile — is moved into a far corner; 1025 points in a small cube;
a three-frame chain (fixed, revolute, prismatic) with 0, 1030 and 5 vertices and three
configurations; polylines of 0, 1, 2 and 1026 points (test_path_clearance.walk).  The caps lie
half way between the two smallest exact results, so they bind for some rows and not for all.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "p-ntfields_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import arm_oracle as A  # noqa: E402
import test_mesh_family_bits as T  # noqa: E402
from test_path_clearance import walk  # noqa: E402


def inputs():
    rng = np.random.default_rng(2026)
    tris = A.boxed_mesh(rng, 257, 0.02).astype(np.float32)
    tris[7, 2] = 0.5 * (tris[7, 0] + tris[7, 1])                      # zero area: c on ab
    tris[256] = np.float32(0.47) + rng.uniform(-0.02, 0.02, (3, 3)).astype(np.float32)
    f = {"tris": tris,
         "pts": (np.array([0.05, -0.1, 0.1]) + rng.uniform(-0.05, 0.05, (1025, 3))
                 ).astype(np.float32)}
    spec = [A.ROOT,
            ((0.06, 0.0, 0.03), (0.3, -0.2, 0.5), A.REVOLUTE, (1.0, 2.0, -2.0)),
            ((0.05, 0.04, 0.0), (0.0, 0.4, -0.3), A.PRISMATIC, (1.0, 0.0, 1.0))]
    f["arm_xyz"] = np.array([s[0] for s in spec])
    f["arm_rpy"] = np.array([s[1] for s in spec])
    f["arm_kind"] = np.array([T.KINDS.index(s[2]) for s in spec], np.int32)
    f["arm_axis"] = np.array([s[3] for s in spec])
    f["arm_theta"] = A.random_theta(rng, spec, 3).astype(np.float32)
    verts = [A.link_blob(rng, v).astype(np.float32) for v in (0, 1030, 5)]
    f["arm_verts"] = np.concatenate(verts)
    f["arm_voff"] = np.cumsum([0] + [len(v) for v in verts]).astype(np.int32)
    lines = [walk(rng, n, 0.0015, start=np.array([-0.2, -0.3, -0.25])) for n in (0, 1, 2, 1026)]
    f["poly_pts"] = np.zeros((4, 1026, 3), np.float32) + tris[0, 0]   # filler: a mesh vertex
    for c, p in enumerate(lines):
        f["poly_pts"][c, :len(p)] = p
    f["poly_cnt"] = np.array([len(p) for p in lines], np.int32)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    f = inputs()
    # caps from an exact run: half way between the two smallest results
    f["arm_cap"] = f["poly_cap"] = np.float32(np.inf)
    exact = T.run(f)
    for name in ("arm", "poly"):
        d = np.sort(exact[name + "_exact"].view(np.float32))
        assert np.isfinite(d[:2]).all() and d[1] - d[0] > 1e-4, (name, d)
        f[name + "_cap"] = np.float32(0.5 * (d[0] + d[1]))
    out = T.run(f)
    # no exact distance ties the cap to the bit (`where` could then be either value)
    assert not (out["poly_exact"].view(np.float32) == f["poly_cap"]).any()
    assert np.array_equal(out["point_c1"], out["point_c2"])
    path = os.path.join(args.out, T.FIXTURE)
    np.savez_compressed(path, **f, **{"bits/" + k: v for k, v in out.items()})
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    for k, v in out.items():
        print(k, v[:4] if v.dtype == np.int32 else v[:4].view(np.float32))


if __name__ == "__main__":
    main()
