"""The point, arm and polyline mesh-distance kernels on slivers, tiny and degenerate triangles.

All three kernels share one per-triangle record and one tri_d2 (csrc/pntf_mesh_geom.h).  Their
other parity tests draw well-shaped triangles and uniformly random points, which never put a
query above the FACE of a thin triangle — the one place where the record's unit normal
decides the result.  tests/mesh_cond_oracle.py builds those inputs; this file pins them on the
CPU and holds the kernels to their existing tolerances on them (2e-6 point and polyline,
3e-6 arm, against the fp64 oracles).

What the inputs found on an MI355X with the record as it was (fp32 cross product, inside test
at 0), worst kernel - oracle over the single-sliver cases, by aspect 1e-2 / 1e-3 / 1e-4 /
1e-5 / 3e-6:
    above the face               -2.5e-7  -3.4e-6  -2.6e-5  -1.0e-4  -1.8e-4   (over: 3e-7, 1.4e-6)
    in the plane beyond a tip      3e-8     3e-8   -2.9e-5  -6.8e-4  -9.6e-4
    lattice mesh -2.2e-5 / +5.9e-7; polyline through face queries -6.5e-6
and with the header as it is: 4e-8 on the single slivers, -2.3e-8 / +2.4e-7 on the lattice,
1.4e-10 on the polylines ("Conditioning of the triangle record").
Two defects, both fixed in build_record / tri_d2: the fp32 normal of a sliver (plane distance
too small by up to |q| 6e-8 / s) and the inside test at 0 (a point of the plane beyond a sharp
tip took the plane distance, ~0).  A copy of the header with either change undone fails this
file on the GPU; on the CPU the numpy restatement shows the same
(test_restated_header_shows_that_the_inputs_have_teeth).

The fp64 oracle is pinned here too.  Ericson's barycentric products cancel like 1e-16 / sin^2:
at aspect 3e-6 the oracle missed the long double plane distance by up to 2e-8 above faces and
by 2e-6 on points of the edges, and with a == b it measured every point against the vertex a.
It now takes the plane distance in the interior region and the three edges of a flat triangle
in every region (oracle/mesh_oracle.py), and holds 1e-9 against long double at EVERY aspect and
family used here, so no aspect is left out.
"""
import functools

import numpy as np
import pytest
import torch

import arm_oracle as A
import mesh_cond_oracle as C
import segment_oracle as S
from oracle import mesh_oracle as M
from pntf import kin

TOL = 2e-6               # tests/test_mesh.py: point kernel, coordinates in [-0.5, 0.5]
ARM_TOL = 3e-6           # tests/test_arm_sampler.py
ORACLE_PIN = 1e-9        # fp64 oracle against long double


@functools.lru_cache(maxsize=None)
def families():
    """The single-sliver cases with their oracle distances (computed once, never modified)."""
    out = []
    for fam, v, s, tri, pts, kind in C.family_cases():
        ref = M.point_mesh_distance(pts, tri[None])
        ref.setflags(write=False)
        out.append((fam, v, s, tri, pts, kind, ref))
    return out


@functools.lru_cache(maxsize=None)
def lattice():
    L = C.lattice_scene()
    L["ref"], L["near"] = C.nearest(L["pts"], L["tris"])
    for v in L.values():
        v.setflags(write=False)
    return L


def signed_worst(err):
    """(worst underestimate, worst overestimate) of kernel - oracle, both >= 0."""
    err = np.asarray(err, np.float64)
    return (max(0.0, -err.min()), max(0.0, err.max())) if err.size else (0.0, 0.0)


def report(title, rows):
    print(title)
    for key, (under, over) in rows.items():
        print("  %-28s worst underestimate %.3g, worst overestimate %.3g" % (key, under, over))


# ------------------------------------------------------------------ CPU: the inputs and the oracle


def test_families_are_the_triangles_they_claim():
    cases = families()
    assert len(cases) == 2 * 3 * len(C.ASPECTS) * 6
    heights = []
    for fam, v, s, tri, pts, kind, _ in cases:
        assert tri.dtype == np.float32 and pts.dtype == np.float32
        assert np.abs(tri).max() <= 0.5 and np.abs(pts).max() <= 0.5
        t = tri.astype(np.float64)
        e = [t[(v + 1) % 3] - t[v], t[(v + 2) % 3] - t[v]]
        sin = np.linalg.norm(np.cross(*e)) / np.linalg.norm(e[0]) / np.linalg.norm(e[1])
        cos = e[0] @ e[1]
        assert 0.6 * s < sin < 1.6 * s and (cos > 0) == (fam == "needle"), (fam, v, s, sin)
        assert C.sin2_at_a(tri) > C.FLAT_SIN2          # none is flat by the rule
        face = kind == C.FACE
        assert face.sum() == 16 and C.barycentrics(pts[face], tri).min() >= C.MARGIN
        h = C.plane_distance(pts[face], tri)
        assert h.min() > 0.9e-4 and h.max() < 0.31
        heights.append(h)
        assert sorted(set(kind)) == [C.FACE, C.ON, C.VERTEX, C.EDGE, C.EDGE_OUT, C.VORONOI]
    heights = np.concatenate(heights)           # 1e-4 .. 0.3, log-uniform
    assert heights.min() < 1.1e-4 and heights.max() > 0.25
    assert 0.2 < (heights < 1e-2).mean() < 0.8


def test_oracle_is_the_plane_distance_above_faces():
    worst = dict.fromkeys(C.ASPECTS, 0.0)
    for fam, v, s, tri, pts, kind, ref in families():
        face = kind == C.FACE
        worst[s] = max(worst[s], np.abs(ref[face] - C.plane_distance(pts[face], tri)).max())
    print("oracle - long double plane distance, worst per aspect:", worst)
    assert max(worst.values()) <= ORACLE_PIN


def test_oracle_against_long_double_on_every_query_kind():
    """Edges, vertices, tips and Voronoi boundaries too: the oracle's region tests are built
    from the same cancelling products as its interior point."""
    worst = {}
    for fam, v, s, tri, pts, kind, ref in families():
        err = np.abs(ref - C.reference_distance(pts, tri))
        for k in set(kind):
            key = (s, C.KIND_NAMES[k])
            worst[key] = max(worst.get(key, 0.0), err[kind == k].max())
    print("oracle - long double reference:", {k: "%.2g" % e for k, e in sorted(worst.items())})
    assert max(worst.values()) <= ORACLE_PIN


def test_restated_header_shows_that_the_inputs_have_teeth():
    """The numpy restatement of build_record / tri_d2 against the oracle.  With the record as it
    was (fp32 normal, inside test at 0) the face-region queries of every aspect <= 1e-3 exceed
    TOL; so do in-plane points beyond a tip at every aspect <= 1e-5 even with the fp64 normal
    as long as the inside test sits at 0; the header as it is holds TOL on every query."""
    face32 = dict.fromkeys(C.ASPECTS, 0.0)
    tip0 = dict.fromkeys(C.ASPECTS, 0.0)
    now = dict.fromkeys(C.ASPECTS, 0.0)
    under = over = 0.0
    for fam, v, s, tri, pts, kind, ref in families():
        e32 = C.emu_distance(pts, tri, "fp32", 0.0).astype(np.float64) - ref
        e0 = C.emu_distance(pts, tri, "fp64", 0.0).astype(np.float64) - ref
        e = C.emu_distance(pts, tri).astype(np.float64) - ref
        face32[s] = max(face32[s], np.abs(e32[kind == C.FACE]).max())
        tip0[s] = max(tip0[s], np.abs(e0[kind == C.EDGE_OUT]).max())
        now[s] = max(now[s], np.abs(e).max())
        u, o = signed_worst(e32[kind == C.FACE])
        under, over = max(under, u), max(over, o)
    print("fp32 normal, face region:", face32, "under %.3g over %.3g" % (under, over))
    print("fp64 normal, inside test at 0, beyond a tip:", tip0)
    print("header as it is, every query:", now)
    assert all(face32[s] > TOL for s in C.ASPECTS if s <= 1e-3)
    assert all(tip0[s] > TOL for s in C.ASPECTS if s <= 1e-5)
    assert max(now.values()) <= TOL
    assert under > 10 * over                   # the fp32 normal errs low: a small h wins the min


def test_oracle_is_continuous_across_the_flat_threshold():
    """Either side of sin^2 = 1e-12 the two evaluations — plane distance inside, nearest edge —
    agree within TOL (the triangle is narrower than that), so the rule's switch is invisible."""
    L = lattice()
    flat = np.flatnonzero(L["label"] == "threshold_flat")
    opened = np.flatnonzero(L["label"] == "threshold_open")
    assert len(flat) == 2 and len(opened) == 2
    s2 = C.sin2_at_a(L["tris"])
    assert (s2[flat] < 0.9e-12).all() and (s2[flat] > 0.2e-12).all()
    assert (s2[opened] > 1.1e-12).all() and (s2[opened] < 4e-12).all()
    for i in np.concatenate([flat, opened]):
        tri = L["tris"][i].astype(np.float64)
        pts = L["pts"][L["owner"] == i].astype(np.float64)
        a, b, c = tri
        edge = np.sqrt(np.minimum(np.minimum(M._seg_d2(pts, a, b - a), M._seg_d2(pts, a, c - a)),
                                  M._seg_d2(pts, b, c - b)))
        by_rule = np.sqrt(M.tri_d2(pts, tri[None]))
        face = np.where(C.barycentrics(pts, tri).min(-1) >= 0, C.plane_distance(pts, tri), edge)
        assert np.abs(by_rule - edge).max() <= TOL and np.abs(by_rule - face).max() <= TOL
        if i in flat:
            assert np.abs(by_rule - edge).max() <= 1e-12


def test_oracle_against_long_double_on_degenerate_tiny_and_threshold_triangles():
    """One triangle at a time, its own queries: a == b, a == c, b == c, a point, collinear with
    each vertex in the middle, edges down to 1e-7, and both sides of the flat threshold."""
    L = lattice()
    worst = {}
    for i in np.flatnonzero(~np.isin(L["label"], ("needle", "cap"))):
        pts = L["pts"][L["owner"] == i]
        err = np.abs(M.point_mesh_distance(pts, L["tris"][i][None])
                     - C.reference_distance(pts, L["tris"][i]))
        worst[L["label"][i]] = max(worst.get(L["label"][i], 0.0), err.max())
    print("oracle - long double reference:", worst)
    assert sorted(worst) == ["degenerate", "threshold_flat", "threshold_open", "tiny"]
    assert max(worst.values()) <= ORACLE_PIN


def test_lattice_queries_land_on_sliver_faces():
    L = lattice()
    tris, pts = L["tris"], L["pts"]
    assert len(tris) >= 257 and len(pts) >= 1025 + 1024
    assert np.abs(tris).max() <= 0.5 and np.abs(pts).max() <= 0.5
    sliver = np.isin(L["label"], ("needle", "cap"))
    for s in C.ASPECTS:
        assert (sliver & (L["aspect"] == s)).sum() >= 50
    assert sorted(set(L["label"])) == ["cap", "degenerate", "needle", "threshold_flat",
                                       "threshold_open", "tiny"]
    assert (L["label"] == "degenerate").sum() == len(C.DEGENERATE)
    assert sorted(L["aspect"][L["label"] == "tiny"]) == sorted(C.TINY_EDGES * 2)
    assert np.abs(tris[L["label"] == "tiny"]).max() > 0.44
    hit = sliver[L["near"]] & C.in_face_region(pts, tris, L["near"])
    print("nearest triangle is a sliver met in its face region: %.3f of %d queries; own "
          "triangle nearest: %.3f" % (hit.mean(), len(pts), (L["near"] == L["owner"]).mean()))
    assert hit.mean() >= 0.5
    # the same holds for the first workgroup + 1 point against the first tile + 1 triangle
    d, near = C.nearest(pts[:1025], tris[:257])
    assert (sliver[:257][near] & C.in_face_region(pts[:1025], tris[:257], near)).mean() >= 0.25
    # both LDS tiles hold slivers of every aspect
    for part in (slice(0, 256), slice(256, None)):
        assert set(C.ASPECTS) <= set(L["aspect"][part][sliver[part]])


# ------------------------------------------------------------------ GPU


def gpu(a):
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the cached scenes are read-only


def point_routes(pts, tris):
    """ops.point_mesh_distance by every route; asserts they agree bit for bit."""
    from pntf import ops
    P, T = gpu(pts), gpu(tris)
    outs = [ops.point_mesh_distance(P, T, chunks=c, order=o) for c in (1, 2, 0)
            for o in (False, True)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    return outs[0].cpu().numpy()


@pytest.mark.gpu
def test_point_kernel_on_single_slivers():
    """One triangle per call, every query of it (heights up to 0.3): the error per aspect and
    kind without a mesh minimum in between."""
    from pntf import ops
    face, rest, missed = {}, {}, []
    for fam, v, s, tri, pts, kind, ref in families():
        d = ops.point_mesh_distance(gpu(pts), gpu(tri[None]), chunks=1, order=False).cpu().numpy()
        assert np.isfinite(d).all()
        err = d.astype(np.float64) - ref
        for table, sel in ((face, kind == C.FACE), (rest, kind == C.EDGE_OUT)):
            u, o = signed_worst(err[sel])
            pu, po = table.get(s, (0.0, 0.0))
            table[s] = (max(pu, u), max(po, o))
        if not np.abs(err).max() < TOL:
            missed.append(("%s at %s, s = %g" % (fam, "abc"[v], s),
                           C.KIND_NAMES[kind[np.abs(err).argmax()]], np.abs(err).max()))
    report("point kernel - oracle, face region, per aspect:", face)
    report("point kernel - oracle, in the plane beyond a tip, per aspect:", rest)
    assert not missed, missed                   # every query of every case within TOL


@pytest.mark.gpu
def test_point_kernel_on_the_lattice():
    L = lattice()
    for n, t in ((len(L["pts"]), len(L["tris"])), (1025, 257)):
        pts, tris = L["pts"][:n], L["tris"][:t]
        ref = L["ref"] if t == len(L["tris"]) else M.point_mesh_distance(pts, tris)
        d = point_routes(pts, tris)
        assert d.shape == (n,) and np.isfinite(d).all()
        err = d.astype(np.float64) - ref
        rows = {}
        for name in sorted(set(L["label"])):
            sel = L["label"][L["owner"][:n]] == name
            rows["%s (%d x %d)" % (name, n, t)] = signed_worst(err[sel])
        report("point kernel - oracle on the lattice, by the family of the query's triangle:",
               rows)
        assert np.abs(err).max() < TOL          # every point, every family


def arm_chain(spec):
    return kin.SerialChain.from_arrays(A.origin_matrices(spec), [s[2] for s in spec],
                                       [s[3] for s in spec])


def far_face_query(L, i):
    """The face query of sliver i whose foot is farthest from its vertex a, (1, 3): the error of
    a tilted normal grows with the in-plane distance from a.  One vertex, because a minimum
    over many would hide every query but the lowest."""
    v = L["pts"][(L["owner"] == i) & (L["kind"] == C.FACE)]
    return v[[np.argmax(np.linalg.norm(v.astype(np.float64) - L["tris"][i][0], axis=1)
                        - C.plane_distance(v, L["tris"][i]))]]


def test_arm_link_vertices_would_show_an_fp32_normal():
    L = lattice()
    sliver = np.flatnonzero(np.isin(L["label"], ("needle", "cap")))
    err = []
    for i in sliver:
        v = far_face_query(L, i)
        err.append(abs(float(C.emu_distance(v, L["tris"][i], "fp32", 0.0)[0])
                       - C.plane_distance(v, L["tris"][i])[0]))
    assert (np.array(err) > ARM_TOL).sum() >= 2


@pytest.mark.gpu
def test_arm_kernel_fixed_link_above_sliver_faces():
    """A FIXED identity link whose one vertex is a face-region query of ONE sliver (the one
    farthest from the sliver's vertex a): one call per sliver of the mesh, and one with the face
    queries of all of them (4096+ vertices: several vertex chunks)."""
    from pntf import ops
    L = lattice()
    spec = [A.ROOT, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), A.FIXED, (1.0, 0.0, 0.0))]
    chain, T = arm_chain(spec), gpu(L["tris"])
    theta = np.zeros((2, 0), np.float32)
    rows = {}
    sliver = np.isin(L["label"], ("needle", "cap"))
    everything = L["pts"][sliver[L["owner"]] & (L["kind"] == C.FACE)]
    assert len(everything) > 4 * 1024
    missed = []
    for i in list(np.flatnonzero(sliver)) + [None]:
        v = everything if i is None else far_face_query(L, i)
        verts = [np.zeros((0, 3), np.float32), v]
        ref = A.arm_mesh_distance(spec, theta.astype(np.float64), verts, L["tris"])
        d = ops.arm_mesh_distance(gpu(theta), chain, [gpu(x) for x in verts], T).cpu().numpy()
        err = d.astype(np.float64) - ref
        s = "all" if i is None else "s = %g" % L["aspect"][i]
        u, o = signed_worst(err)
        pu, po = rows.get(s, (0.0, 0.0))
        rows[s] = (max(pu, u), max(po, o))
        assert d[0] == d[1]
        if not np.abs(err).max() < ARM_TOL:
            missed.append((s, d[0], ref[0]))
    report("arm kernel (fixed link) - oracle:", rows)
    assert not missed, missed


@pytest.mark.gpu
def test_arm_kernel_revolute_link_swings_across_slivers():
    """A revolute joint whose axis runs along a sliver, 0.05 above it, swings one vertex across
    the sliver's width at a height of 0.002: edge region, face region, edge region."""
    from pntf import ops
    L = lattice()
    T = gpu(L["tris"])
    rows = {}
    for s in (1e-3, 1e-4, 1e-5):
        i = int(np.flatnonzero((L["label"] == "needle") & (L["aspect"] == s))[0])
        tri = L["tris"][i].astype(np.float64)
        lens = [np.linalg.norm(tri[(k + 1) % 3] - tri[k]) for k in range(3)]
        k = int(np.argmax(lens))
        u = (tri[(k + 1) % 3] - tri[k]) / lens[k]
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        n /= np.linalg.norm(n)
        mid = tri.mean(0)
        width = 2 * np.linalg.norm(np.cross(tri - mid, u), axis=1).max()
        R, h0 = 0.05, 0.002
        spec = [A.ROOT, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), A.FIXED, (1.0, 0.0, 0.0)),
                (tuple(mid + R * n), (0.0, 0.0, 0.0), A.REVOLUTE, tuple(u))]
        swing = 3 * width / (R - h0)
        theta = np.linspace(-swing, swing, 65)[:, None].astype(np.float32)
        verts = [np.zeros((0, 3), np.float32)] * 2 + [(-(R - h0) * n)[None].astype(np.float32)]
        posed = A.pose_points(spec, theta.astype(np.float64), 2, verts[2])[:, 0]
        inside = C.barycentrics(posed.astype(np.float32), L["tris"][i]).min(-1) > 0
        assert 5 <= inside.sum() <= 60 and not inside[0] and not inside[-1]
        ref = A.arm_mesh_distance(spec, theta.astype(np.float64), verts, L["tris"])
        d = ops.arm_mesh_distance(gpu(theta), arm_chain(spec), [gpu(x) for x in verts],
                                  T).cpu().numpy()
        err = d.astype(np.float64) - ref
        rows["s = %g" % s] = signed_worst(err)
        assert np.abs(err).max() < ARM_TOL, (s, np.abs(err).max())
    report("arm kernel (revolute swing) - oracle:", rows)


@functools.lru_cache(maxsize=None)
def polylines():
    """Three polylines per picked sliver of the lattice (the first 4 of every aspect):
    above    through the sliver's face queries of one side (the segments stay over the face);
    pierce   from a face query straight through the face to its mirror image (distance 0);
    outside  across the plane 1e-5 .. 1e-4 outside the middle of the longest edge.
    -> (pts (q, Lmax, 3) float32, cnt (q,) int32, kind list, aspect (q,), oracle distances)."""
    L = lattice()
    rng = np.random.default_rng(3)
    lines, kinds, aspects = [], [], []
    for s in C.ASPECTS:
        for i in np.flatnonzero(np.isin(L["label"], ("needle", "cap")) & (L["aspect"] == s))[:4]:
            tri = L["tris"][i].astype(np.float64)
            n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            n /= np.linalg.norm(n)
            face = L["pts"][(L["owner"] == i) & (L["kind"] == C.FACE)].astype(np.float64)
            up = face[(face - tri[0]) @ n > 0]
            h = (face[0] - tri[0]) @ n
            k = int(np.argmax([np.linalg.norm(tri[(j + 1) % 3] - tri[j]) for j in range(3)]))
            e = tri[(k + 1) % 3] - tri[k]
            out = np.cross(e, n)
            out *= -np.sign(out @ (tri[(k + 2) % 3] - tri[k])) / np.linalg.norm(out)
            x = tri[k] + 0.5 * e + np.exp(rng.uniform(np.log(1e-5), np.log(1e-4))) * out
            for name, line in (("above", up), ("pierce", np.stack([face[0], face[0] - 2 * h * n])),
                               ("outside", np.stack([x + 0.01 * n, x - 0.01 * n]))):
                lines.append(line.astype(np.float32))
                kinds.append(name)
                aspects.append(s)
    Lmax = max(len(p) for p in lines)
    pts = np.zeros((len(lines), Lmax, 3), np.float32)
    for c, p in enumerate(lines):
        pts[c, :len(p)] = p
    cnt = np.array([len(p) for p in lines], np.int32)
    ref = np.array([S.polyline_distance(p, L["tris"])[0] for p in lines])
    return pts, cnt, kinds, np.array(aspects), ref


def test_polylines_are_the_three_kinds():
    pts, cnt, kinds, aspects, ref = polylines()
    kinds = np.array(kinds)
    assert (cnt[kinds == "above"] >= 2).all() and (cnt[kinds != "above"] == 2).all()
    assert (ref[kinds == "pierce"] == 0.0).all()
    assert (ref[kinds == "above"] > 0.9e-4).all()
    assert (ref[kinds == "outside"] > 0.9e-5).all() and (ref[kinds == "outside"] < 1.1e-4).all()
    assert np.abs(pts).max() <= 0.5


@pytest.mark.gpu
def test_polyline_kernel_above_through_and_beside_slivers():
    from pntf import ops
    L = lattice()
    pts, cnt, kinds, aspects, ref = polylines()
    d, where = ops.polyline_mesh_distance(gpu(pts), gpu(cnt), gpu(L["tris"]))
    d = d.cpu().numpy()
    assert np.isfinite(d).all()
    err = d.astype(np.float64) - ref
    rows = {}
    for name in ("above", "pierce", "outside"):
        for s in C.ASPECTS:
            rows["%s, s = %g" % (name, s)] = signed_worst(err[(np.array(kinds) == name)
                                                              & (aspects == s)])
    report("polyline kernel - oracle:", rows)
    assert np.abs(err).max() < TOL, (kinds[np.abs(err).argmax()], aspects[np.abs(err).argmax()])
