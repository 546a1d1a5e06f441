"""The three mesh-distance kernels (point, arm, polyline) against recorded bits.

tests/golden/mesh_family_bits.npz holds the inputs and, as raw uint32 / int32 bit patterns, what
the library gave for them when the three kernels still had their own fill and finalize passes;
tests/golden/make_mesh_family_goldens.py wrote it on an MI355X.  The same calls (`run`, used
by the generator too) must give the same bits whatever is shared or moved between the
kernels later: a difference means the arithmetic of a (point, triangle) pair or the culling
changed.  No tolerance.

The shapes are the smallest at which the culled tile loop can go wrong: two workgroups with one live
lane in the second, two triangle tiles with one triangle in the second, the split route, vertex
and segment chunks with a nearly empty second chunk, empty and one-point polylines, a cap that
binds.  The last triangle (the whole second tile) lies in a far corner, so every workgroup
culls it, asserted on the CPU below from the oracle distances; the triangle nearest to a
workgroup's points is never culled, so the cull takes both branches.
"""
import numpy as np
import pytest
import torch

import arm_oracle as A
import golden_util as G
import segment_oracle as S
from oracle import mesh_oracle as M
from pntf import kin

FIXTURE = "mesh_family_bits.npz"
KINDS = (A.FIXED, A.REVOLUTE, A.PRISMATIC)
POINT_RUNS = (("point_1", 1, 1, 0), ("point_c1", 1025, 257, 1), ("point_c2", 1025, 257, 2))


def bits(x):
    return x.detach().cpu().numpy().view(np.uint32)


def arm_spec(f):
    return [(tuple(x), tuple(r), KINDS[k], tuple(a)) for x, r, k, a in
            zip(f["arm_xyz"], f["arm_rpy"], f["arm_kind"], f["arm_axis"])]


def arm_verts(f):
    return np.split(f["arm_verts"], f["arm_voff"][1:-1])


def run(f):
    """Every call of the fixture on the GPU: {name: uint32 bits (int32 for `where`)}; the
    fixture holds them under "bits/" + name."""
    from pntf import ops
    dev = torch.device("cuda:0")
    gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tris, pts = gpu(f["tris"]), gpu(f["pts"])
    out = {}
    for name, n, t, chunks in POINT_RUNS:
        out[name] = bits(ops.point_mesh_distance(pts[:n], tris[:t], chunks=chunks, order=False))
    spec = arm_spec(f)
    chain = kin.SerialChain.from_arrays(A.origin_matrices(spec), [s[2] for s in spec],
                                        [s[3] for s in spec])
    theta, verts = gpu(f["arm_theta"]), [gpu(v) for v in arm_verts(f)]
    poly, cnt = gpu(f["poly_pts"]), gpu(f["poly_cnt"])
    for tag, acap, pcap in (("exact", None, None),
                            ("cap", float(f["arm_cap"]), float(f["poly_cap"]))):
        out["arm_" + tag] = bits(ops.arm_mesh_distance(theta, chain, verts, tris, cap=acap))
        d, w = ops.polyline_mesh_distance(poly, cnt, tris, cap=pcap)
        out["poly_" + tag] = bits(d)
        out["poly_where_" + tag] = w.cpu().numpy().astype(np.int32)
    return out


def gap2(box_lo, box_hi, tri):
    """Squared distance between a point box and a triangle's AABB."""
    g = np.maximum(np.maximum(tri.min(0) - box_hi, box_lo - tri.max(0)), 0.0)
    return float(g @ g)


def surely_culled(points, tris, rule):
    """The last triangle against the box and the bound of a workgroup that owns `points` and
    has been through the triangles before it.  The bound is at most rule (np.max: the point
    kernel, np.min: arm and polyline) of the points' squared distances to those triangles; the
    last triangle's AABB is farther from the box than twice that (the kernel's slack is 1e-4
    relative and 1e-6 * 0.25 absolute)."""
    points = np.asarray(points, np.float64)
    bound = rule(M.point_mesh_distance(points, tris[:-1])) ** 2
    return gap2(points.min(0), points.max(0), tris[-1]) > 2 * bound + 1e-6


def test_fixture_takes_both_branches_of_the_cull():
    f = G.load(FIXTURE)
    tris = f["tris"].astype(np.float64)
    assert tris.shape == (257, 3, 3)
    ab, ac = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    nn, ab2, ac2 = (np.cross(ab, ac) ** 2).sum(1), (ab ** 2).sum(1), (ac ** 2).sum(1)
    assert (nn <= 1e-12 * ab2 * ac2).sum() == 1                  # one flat triangle (the record's test)
    # point kernel, chunks = 1: both workgroups (1024 points, and the last point alone)
    assert surely_culled(f["pts"][:1024], tris, np.max)
    assert surely_culled(f["pts"][1024:], tris, np.max)
    # arm: every vertex chunk of every configuration (1024 + 6 vertices of frame 1, 5 of frame 2)
    spec, verts = arm_spec(f), arm_verts(f)
    assert [len(v) for v in verts] == [0, 1030, 5] and [s[2] for s in spec] == list(KINDS)
    for th in f["arm_theta"].astype(np.float64):
        for fr, v in ((1, verts[1][:1024]), (1, verts[1][1024:]), (2, verts[2])):
            assert surely_culled(A.pose_points(spec, th[None], fr, v)[0], tris, np.min)
    # polylines, per chunk of 1024 segments: a wave's box lies inside its chunk's, and a segment
    # is never farther than its vertices
    assert f["poly_cnt"].tolist() == [0, 1, 2, 1026] and f["poly_pts"].shape == (4, 1026, 3)
    for p, n in zip(f["poly_pts"], f["poly_cnt"]):
        for chunk in (p[:min(n, 1025)], p[1024:n]):
            assert len(chunk) == 0 or surely_culled(chunk, tris, np.min)
    # the caps bind for some rows and not for others, on the CPU as in the recorded bits
    arm = A.arm_mesh_distance(spec, f["arm_theta"].astype(np.float64), verts, tris)
    assert (arm < f["arm_cap"] - 1e-5).any() and (arm > f["arm_cap"] + 1e-5).any()
    poly = np.array([S.polyline_distance(p[:n], tris)[0]
                     for p, n in zip(f["poly_pts"][1:], f["poly_cnt"][1:])])
    assert (poly < f["poly_cap"] - 1e-5).any() and (poly > f["poly_cap"] + 1e-5).any()
    # a distance equal to the cap may report either `where`: the fixture holds no such tie
    exact = f["bits/poly_exact"].view(np.float32)
    assert not (exact == np.float32(f["poly_cap"])).any()


@pytest.mark.gpu
def test_mesh_family_bits_equal_the_recorded_ones():
    f = G.load(FIXTURE)
    got = run(f)
    assert sorted("bits/" + k for k in got) == sorted(k for k in f.files if k.startswith("bits/"))
    for k, v in got.items():
        want = f["bits/" + k]
        assert v.dtype == want.dtype and np.array_equal(v, want), (k, v, want)
