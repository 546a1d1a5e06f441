"""Planned-path clearance: the polyline -> mesh distance kernel (pntf_polyline_mesh_distance),
ops.plan_polylines, pntf.evaluate.path_report and Model.PlanReport.

Pinning: the reference never measures a path against the mesh (its scripts end in a viewer),
so parity is pinned by geometry: the fp64 oracle (tests/segment_oracle.py) is checked here
against closed forms and against a sampled sandwich that does not share its decomposition.

GPU tolerance: BOUND = 2e-7 absolute on the distance, coordinates in the unit box: four times
the worst error measured against the fp64 oracle over the parity cases below (WORST = 2.7e-8,
the "ragged" paths against a single triangle, distances up to 0.5), rounded up to one digit.
The point and arm kernels hold 2e-6 and 3e-6; this bound is about three fp32 ulps of 0.5.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import arm_oracle as A
import segment_oracle as S
from oracle import mesh_oracle as M
from pntf import _lib, evaluate, kin, synth

# Worst |kernel - oracle| over the parity cases (one 1.3e-8, ragged x 5 meshes 2.7e-8, repeat
# 2.3e-9, flat 2.5e-9, cluster 6.9e-9), measured on an MI355X: WORST.  BOUND = 4 x WORST
# (1.07e-7) rounded up to one digit.
WORST = 2.7e-8
BOUND = 2e-7
ARM_TOL = 3e-6          # tests/test_arm_sampler.py

TRI = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])


def dist1(p0, p1, tri=TRI):
    return float(np.sqrt(S.seg_tri_d2(np.asarray(p0, float), np.asarray(p1, float), tri)))


# ------------------------------------------------------------------ CPU: oracle pinning


def test_oracle_closed_forms():
    h = 0.37
    assert abs(dist1([0.2, 0.2, h], [0.3, 0.3, h]) - h) < 1e-14          # above the interior
    assert abs(dist1([-0.5, 0.3, h], [1.5, 0.3, h]) - h) < 1e-14         # ends outside, above
    assert dist1([0.2, 0.2, -1], [0.2, 0.2, 1]) == 0.0                    # pierces
    assert dist1([0.2, 0.2, 1], [0.2, 0.2, -1]) == 0.0
    assert dist1([0.2, 0.2, 0.0], [0.2, 0.2, 1]) == 0.0                   # starts on it
    assert abs(dist1([0.2, 0.2, 0.1], [0.2, 0.2, 1]) - 0.1) < 1e-14      # stops short of it
    assert abs(dist1([0.9, 0.9, -1], [0.9, 0.9, 1])                       # crosses the plane outside
               - np.sqrt(0.32)) < 1e-14
    # beyond vertex b: the segment x = 2, z = 0.3 is nearest to (1, 0, 0) at its own y = 0
    assert abs(dist1([2, -1, 0.3], [2, 1, 0.3]) - np.sqrt(1 + 0.09)) < 1e-14
    # skew to edge ab (the x axis), outside the triangle (y < 0): distance of two skew lines
    p, q = np.array([0.3, -0.4, -0.5]), np.array([0.7, -0.2, 0.6])
    n = np.cross(q - p, [1.0, 0, 0])
    assert abs(dist1(p, q) - abs(p @ n) / np.linalg.norm(n)) < 1e-14
    assert abs(dist1(p, q) - 0.30411) < 1e-5
    # coplanar segment across the triangle
    assert dist1([-0.5, 0.2, 0], [1.5, 0.2, 0]) < 1e-15
    assert dist1([0.1, 0.1, 0], [0.2, 0.3, 0]) == 0.0                     # coplanar, inside


def test_oracle_degenerate_inputs():
    rng = np.random.default_rng(0)
    p = rng.uniform(-1, 1, (200, 3))
    tri = rng.uniform(-1, 1, (200, 3, 3))
    np.testing.assert_allclose(S.seg_tri_d2(p, p, tri), M.tri_d2(p, tri), rtol=0, atol=1e-14)
    # a flat triangle (c on ab) is the segment ab
    a, b = rng.uniform(-1, 1, (2, 200, 3))
    flat = np.stack([a, b, a + 0.4 * (b - a)], axis=1)
    q = rng.uniform(-1, 1, (200, 3))
    np.testing.assert_allclose(S.seg_tri_d2(p, q, flat), S.seg_seg_d2(p, q, a, b), atol=1e-14)
    # a point triangle, and segment - segment with a zero-length member = point - segment
    dot = np.stack([a, a, a], axis=1)
    want = M._seg_d2(a, p, q - p)
    np.testing.assert_allclose(S.seg_tri_d2(p, q, dot), want, atol=1e-14)
    np.testing.assert_allclose(S.seg_seg_d2(p, q, a, a), want, atol=1e-14)
    np.testing.assert_allclose(S.seg_seg_d2(a, a, p, q), want, atol=1e-14)
    # parallel overlapping segments
    assert abs(S.seg_seg_d2([0, 0, 0.0], [2, 0, 0.0], [1, 1, 0.0], [5, 1, 0.0]) - 1) < 1e-15
    assert abs(S.seg_seg_d2([0, 0, 0.0], [2, 0, 0.0], [3, 1, 0.0], [5, 1, 0.0]) - 2) < 1e-15


def test_oracle_sandwich_against_sampling():
    """oracle <= sampled + 1e-12 and sampled <= oracle + delta / 2 for 300 random pairs: the
    sampled minimum of the POINT oracle shares no segment code with the oracle."""
    rng = np.random.default_rng(1)
    K, worst_lo, worst_hi, pierced = 1500, 0.0, 0.0, 0
    for i in range(300):
        tri = rng.uniform(-0.5, 0.5, (3, 3)) * rng.choice([1.0, 0.3])
        p0 = rng.uniform(-0.5, 0.5, 3)
        p1 = p0 + rng.normal(0, 0.3, 3) * rng.choice([1.0, 0.1])
        if i % 4 == 0:                       # aimed through (or just past) the triangle
            w = rng.dirichlet([1, 1, 1]) * rng.choice([1.0, 1.3])
            p1 = p0 + rng.uniform(0.8, 2.0) * (w @ tri / w.sum() - p0)
        d = dist1(p0, p1, tri)
        s = S.sampled_distance(p0, p1, tri, K)
        delta = np.linalg.norm(p1 - p0) / K
        pierced += d == 0.0
        worst_lo, worst_hi = max(worst_lo, d - s), max(worst_hi, s - d - delta / 2)
        assert d <= s + 1e-12 and s <= d + delta / 2, (i, d, s, delta)
    assert pierced >= 10
    print("sandwich: oracle - sampled <= %.3g, sampled - oracle - delta/2 <= %.3g, %d pierced"
          % (worst_lo, worst_hi, pierced))


# ------------------------------------------------------------------ CPU: library and torch layers


def test_polyline_symbols_and_validation_without_gpu():
    L = _lib.load()
    fake = ctypes.c_void_p(64)               # never dereferenced: validation comes first
    inf = float("inf")
    assert L.pntf_polyline_workspace_bytes(5) == 40 and L.pntf_polyline_workspace_bytes(0) == 0

    def call(pts=fake, q=5, Lp=9, cnt=fake, tris=fake, t=3, cap=inf, dist=fake, where=fake,
             ws=fake, wsb=40):
        return L.pntf_polyline_mesh_distance(pts, q, Lp, cnt, tris, t, cap, dist, where, ws, wsb,
                                             None)

    bad = [(dict(q=-1), b"negative"), (dict(t=-1), b"negative"), (dict(Lp=-1), b"negative"),
           (dict(pts=None), b"null"), (dict(cnt=None), b"null"), (dict(tris=None), b"null"),
           (dict(dist=None), b"null"), (dict(ws=None), b"null"), (dict(t=0), b"empty mesh"),
           (dict(cap=-1.0), b"cap must be >= 0"), (dict(cap=float("nan")), b"cap must be >= 0"),
           (dict(wsb=39), b"workspace too small"), (dict(ws=ctypes.c_void_p(68)), b"aligned"),
           (dict(Lp=65535 * 1024 + 2), b"65535")]
    for kw, text in bad:
        assert L.pntf_point_mesh_distance(None, 5, None, 3, None, 0, None) == 1   # other text
        assert call(**kw) == 1, kw
        err = L.pntf_mesh_last_error()
        assert b"pntf_polyline_mesh_distance" in err and text in err, (kw, err)
    assert L.pntf_polyline_mesh_distance(None, 0, 0, None, None, 0, inf, None, None, None, 0,
                                         None) == 0         # an empty batch is a no-op
    with pytest.raises(_lib.PntfError, match="empty mesh"):
        _lib.check(call(t=0), "pntf_polyline_mesh_distance")


def test_polyline_mesh_distance_has_no_cpu_path():
    from pntf import ops
    with pytest.raises(_lib.PntfError):
        ops.polyline_mesh_distance(torch.zeros(2, 4, 3), torch.tensor([4, 4]),
                                   torch.zeros(1, 3, 3))


def loop_polyline(path, s):
    dim = path.shape[1] // 2
    if s < 0:
        return np.zeros((0, dim), path.dtype)
    point0 = [path[i, :dim] for i in range(s + 1)]
    point1 = [path[i, dim:] for i in range(s + 1)]
    point1.reverse()
    return np.stack(point0 + point1)


@pytest.mark.parametrize("dim", [3, 6])
def test_plan_polylines_equals_loop(dim):
    from pntf import ops
    max_iter = 5
    steps = np.array([-1, 0, 1, max_iter + 1, 3], np.int32)
    path = np.random.default_rng(dim).normal(size=(5, max_iter + 2, 2 * dim)).astype(np.float32)
    pts, cnt = ops.plan_polylines(torch.from_numpy(path), torch.from_numpy(steps))
    assert pts.shape == (5, 2 * (max_iter + 2), dim) and pts.dtype == torch.float32
    assert cnt.dtype == torch.int32 and cnt.tolist() == [0, 2, 4, 2 * max_iter + 4, 8]
    for c in range(5):
        want = loop_polyline(path[c], int(steps[c]))
        np.testing.assert_array_equal(pts[c, :len(want)].numpy(), want)
        assert not pts[c, len(want):].any()
    with pytest.raises(_lib.PntfError):
        ops.plan_polylines(torch.from_numpy(path), torch.tensor([0, 0, 0, 0, max_iter + 2]))


def test_path_report_logic_with_injected_clearance():
    """Hand-made dim-3 paths: rows 0..steps are valid, later rows are the frozen copy."""
    tol = 0.1
    path = np.zeros((4, 4, 6), np.float32)
    # query 0: start walks +x by 0.3 twice, goal stays at x = 0.65: final gap 0.05 <= tol
    path[0, :, 3] = 0.65
    path[0, 1:, 0], path[0, 2:, 0] = 0.3, 0.6
    # query 1: used every iteration (steps = 3) and is still 0.5 apart
    path[1, :, 3] = 2.0
    path[1, :, 0] = [0.0, 0.5, 1.0, 1.5]
    # query 2: arrived, but touches the mesh; query 3: invalid env
    path[2, :, 4] = 0.08
    steps = torch.tensor([2, 3, 0, -1], dtype=torch.int32)
    clear = torch.tensor([0.2, 0.3, 0.0, float("inf")])
    rep = evaluate.path_report(torch.from_numpy(path), steps, tol, clearance=clear, safety=0.1)
    assert rep.converged.tolist() == [True, False, True, False]
    assert rep.success.tolist() == [True, False, False, False] and rep.success_rate == 0.25
    assert rep.length.dtype == torch.float64
    np.testing.assert_allclose(rep.length.numpy(), [0.3 + 0.3 + 0.05, 1.5 + 0.5, 0.08, 0.0],
                               atol=1e-7)
    assert rep.where.tolist() == [-1] * 4 and torch.equal(rep.clearance, clear)
    # clearance must exceed safety strictly
    rep = evaluate.path_report(torch.from_numpy(path), steps, tol, clearance=clear, safety=0.2)
    assert rep.success.tolist() == [False] * 4 and rep.success_rate == 0.0
    # converged reads the last valid row, not later rows
    path[0, 3, 3] = 9.0
    assert evaluate.path_report(torch.from_numpy(path), steps, tol,
                                clearance=clear).converged.tolist() == [True, False, True, False]
    with pytest.raises(_lib.PntfError):
        evaluate.path_report(torch.from_numpy(path), steps, tol)          # no mesh, no clearance
    with pytest.raises(_lib.PntfError):                                   # no CPU kernel
        evaluate.path_report(torch.from_numpy(path), steps, tol, tris=torch.zeros(1, 3, 3))


def test_arm_path_samples_respect_the_resolution():
    rng = np.random.default_rng(5)
    pts = torch.from_numpy(rng.uniform(-0.5, 0.5, (3, 6, 4)).astype(np.float32))
    pts[1, 2] = pts[1, 1]                                    # a zero-length segment
    cnt = torch.tensor([6, 3, 0], dtype=torch.int32)
    res = 0.2
    theta, qi, si = evaluate.arm_path_samples(pts, cnt, res)
    assert qi.tolist() == sorted(qi.tolist()) and set(qi.tolist()) == {0, 1}
    for c in (0, 1):
        th, sg = theta[qi == c].numpy(), si[qi == c].numpy()
        n = int(cnt[c])
        assert (np.diff(sg) >= 0).all() and sg[0] == 0 and sg[-1] == n - 2
        assert np.abs(np.diff(th, axis=0)).max() <= res * (1 + 1e-5)
        np.testing.assert_allclose(th[0], pts[c, 0].numpy() * evaluate.ARM_SCALE, rtol=1e-6)
        np.testing.assert_allclose(th[-1], pts[c, n - 1].numpy() * evaluate.ARM_SCALE, rtol=1e-6)
        for i in range(n - 1):                               # every vertex is a sample
            first = th[np.argmax(sg == i)]
            np.testing.assert_allclose(first, pts[c, i].numpy() * evaluate.ARM_SCALE, rtol=1e-6)


# ------------------------------------------------------------------ GPU


def walk(rng, n, step=0.02, start=None):
    """n points of a smoothly turning walk with steps of length `step`, kept in [-0.45, 0.45]^3."""
    p = np.empty((max(n, 1), 3))
    p[0] = rng.uniform(-0.4, 0.4, 3) if start is None else start
    d = rng.normal(size=3)
    for i in range(1, n):
        d = d / np.linalg.norm(d) + 0.5 * rng.normal(size=3)
        q = p[i - 1] + step * d / np.linalg.norm(d)
        d = np.where(np.abs(q) > 0.45, -d, d)
        p[i] = np.clip(q, -0.45, 0.45)
    return p[:n].astype(np.float32)


def small_mesh(rng, t, scale):
    return A.boxed_mesh(rng, t, scale).astype(np.float32)


RAGGED = [0, 1, 2, 7, 1025, 1026]
TILES = [1, 255, 256, 257, 513]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(list of polylines (cnt, 3) float32, triangles (t, 3, 3) float32)."""
    rng = np.random.default_rng({"one": 1, "ragged": 2, "repeat": 3, "flat": 4, "cluster": 5}[name])
    if name == "one":
        return [walk(rng, 2, 0.3)], small_mesh(rng, 1, 0.2)
    if name == "ragged":
        return [walk(rng, n) for n in RAGGED], small_mesh(rng, 513, 0.03)
    if name == "repeat":
        base = walk(rng, 40)
        lines = [np.repeat(base, 2, axis=0), np.repeat(base[:5], [1, 3, 1, 4, 2], axis=0),
                 np.repeat(base[7:8], 5, axis=0)]
        return lines, small_mesh(rng, 60, 0.05)
    if name == "flat":
        tris = small_mesh(rng, 12, 0.1)
        tris[0, 2] = 0.3 * tris[0, 0] + 0.7 * tris[0, 1]           # c on ab
        tris[1, 2] = tris[1, 0] + 1.8 * (tris[1, 1] - tris[1, 0])   # c beyond b on the line
        tris[2, 1] = tris[2, 0]                                      # a = b
        tris[3, 2] = tris[3, 1]                                      # b = c
        tris[4, 1] = tris[4, 2] = tris[4, 0]                         # a point
        return [walk(rng, n, 0.05) for n in (30, 30, 9)], tris[:8].copy()    # + three proper ones
    if name == "cluster":
        near = small_mesh(rng, 300, 0.01) * 0.2 + np.float32(0.38)
        far = small_mesh(rng, 300, 0.01) * 0.2 - np.float32(0.38)
        tris = np.concatenate([far[:150], near, far[150:]]).astype(np.float32)
        lines = [walk(rng, 300, 0.004, start=np.array([0.2, 0.25, 0.3])),
                 walk(rng, 1300, 0.0015, start=np.array([-0.2, -0.3, -0.25])),
                 walk(rng, 50, 0.02, start=np.zeros(3))]
        return lines, tris
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, t=None):
    """Per polyline (distance, where, runner_up) by the fp64 oracle, over the first t triangles."""
    lines, tris = scene(name)
    return [S.polyline_distance(p, tris[:t]) for p in lines]


def pack(lines, L=None, filler=None):
    """(q, L, 3) with the rows past each polyline's end filled with `filler` (default: a mesh
    vertex is passed by the caller, so that reading them would show as a zero distance)."""
    L = max([len(p) for p in lines] + [1]) if L is None else L
    pts = np.zeros((len(lines), L, 3), np.float32)
    pts[:] = 0.0 if filler is None else filler
    for c, p in enumerate(lines):
        pts[c, :len(p)] = p
    return pts, np.array([len(p) for p in lines], np.int32)


def gpu_distance(lines, tris, cap=None, L=None):
    from pntf import ops
    pts, cnt = pack(lines, L, filler=tris[0, 0])
    d, w = ops.polyline_mesh_distance(torch.from_numpy(pts).cuda(), torch.from_numpy(cnt).cuda(),
                                      torch.from_numpy(np.ascontiguousarray(tris)).cuda(), cap=cap)
    assert d.shape == (len(lines),) and d.dtype == torch.float32 and w.dtype == torch.int32
    return d.cpu().numpy(), w.cpu().numpy()


def check_against(ref, d, w, label):
    """Distances to BOUND, pierced polylines exactly 0, `where` wherever the oracle's runner-up
    is farther than BOUND.  Returns the worst error."""
    want = np.array([r[0] for r in ref])
    fin = np.isfinite(want)
    assert np.array_equal(np.isinf(d), ~fin) and (w[~fin] == -1).all()
    err = np.abs(d[fin] - want[fin]).max() if fin.any() else 0.0
    print("polyline distance vs oracle, %s: max abs error %.3g (distances %.3g .. %.3g, %d zero)"
          % (label, err, want[fin].min() if fin.any() else 0, want[fin].max() if fin.any() else 0,
             (want == 0).sum()))
    assert (d[want == 0.0] == 0.0).all(), "a pierced path must give exactly 0.0"
    assert err < BOUND
    for c, (dist, where, runner) in enumerate(ref):
        if np.isfinite(dist) and runner > dist + BOUND:
            assert w[c] == where, (label, c, w[c], where, dist, runner)
    return err


PARITY = [("one", None)] + [("ragged", t) for t in TILES] + [("repeat", None), ("flat", None),
                                                             ("cluster", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,t", PARITY)
def test_hip_polyline_distance_matches_oracle(name, t):
    lines, tris = scene(name)
    d, w = gpu_distance(lines, tris[:t])
    check_against(reference(name, t), d, w, "%s t=%d" % (name, len(tris[:t])))
    if name == "ragged":
        assert np.isinf(d[0]) and w[0] == -1 and w[1] == 0


def test_scenes_hold_the_cases_they_are_meant_to():
    """The clustered scene's paths stay within 0.2 of their own cluster, 0.6 from the other (so
    its tiles can be culled), and the ragged scene holds pierced and clear paths.  That tiles
    ARE culled there rests on this geometry: no test observes a skipped tile, the tests check
    that results with culling are right (parity, and bits independent of row and chunking)."""
    far = reference("cluster")
    assert far[0][0] < 0.2 and far[1][0] < 0.2
    rag = [r[0] for r in reference("ragged", 513)]
    assert any(x == 0.0 for x in rag) and any(np.isfinite(x) and x > 1e-3 for x in rag)


@pytest.mark.gpu
def test_hip_polyline_bits_independent_of_row_padding_and_chunking():
    lines, tris = scene("ragged")
    full, wf = gpu_distance(lines, tris)
    for c in (1, 3, 5):
        d, w = gpu_distance(lines[c:c + 1], tris)
        assert d[0].tobytes() == full[c].tobytes() and w[0] == wf[c]
    d, w = gpu_distance(lines[::-1], tris, L=3000)                 # other rows, other padding
    assert d[::-1].tobytes() == full.tobytes() and np.array_equal(w[::-1], wf)
    # 1026 points = 1025 segments = chunks [0, 1024) and [1024, 1025): the halves share point 1024
    p = lines[5]
    halves, wh = gpu_distance([p[:1025], p[1024:]], tris)
    assert np.minimum(halves[0], halves[1]).tobytes() == full[5].tobytes()
    want = wh[0] if halves[0] <= halves[1] else 1024 + wh[1]
    assert wf[5] == want


@pytest.mark.gpu
def test_hip_polyline_cap_is_bitwise_minimum():
    lines, tris = scene("cluster")
    lines = lines + scene("ragged")[0]
    exact, we = gpu_distance(lines, tris)
    fin = exact[np.isfinite(exact)]
    cap = float(np.float32(np.median(fin[fin > 0])))
    assert (fin < cap).any() and (fin > cap).any()
    capped, wc = gpu_distance(lines, tris, cap=cap)
    assert capped.tobytes() == np.minimum(exact, np.float32(cap)).tobytes()
    assert np.array_equal(wc, np.where(exact > cap, -1, we))
    zero, wz = gpu_distance(lines, tris, cap=0.0)
    assert not zero.any() and np.array_equal(wz, np.where(exact > 0, -1, we))


@pytest.mark.gpu
def test_hip_polyline_never_farther_than_its_vertices():
    """dist <= min over the vertices of the point kernel's distance, exactly (same tri_d2 bits),
    with equality for single points."""
    from pntf import ops
    for name in ("ragged", "cluster", "flat"):
        lines, tris = scene(name)
        d, _ = gpu_distance(lines, tris)
        R = torch.from_numpy(tris).cuda()
        for c, p in enumerate(lines):
            if len(p):
                v = ops.point_mesh_distance(torch.from_numpy(p).cuda(), R, order=False)
                assert d[c] <= v.min().item()
    lines, tris = scene("ragged")
    singles = [p[None] for p in lines[4][:300]]
    d, w = gpu_distance(singles, tris)
    v = ops.point_mesh_distance(torch.from_numpy(lines[4][:300]).cuda(),
                                torch.from_numpy(tris).cuda(), order=False)
    assert d.tobytes() == v.cpu().numpy().tobytes() and not w.any()


@pytest.mark.gpu
def test_hip_polyline_analytic_beside_and_through_a_box():
    lo, hi = np.array([-0.2, -0.1, -0.15]), np.array([0.25, 0.2, 0.1])
    tris = M.box_mesh(lo, hi).astype(np.float32)
    x = np.linspace(-0.45, 0.45, 31)
    gaps = [0.003, 0.05, 0.2]
    beside = [np.stack([x, np.full(31, hi[1] + g), np.full(31, 0.0)], 1).astype(np.float32)
              for g in gaps]
    # steps of 0.03 along y through the 0.02-thin slab below: every vertex is clear of it
    through = np.stack([x, np.zeros(31), np.zeros(31)], 1).astype(np.float32)
    d, w = gpu_distance(beside + [through], tris)
    want = np.array([np.float32(hi[1] + g) - np.float32(hi[1]) for g in gaps], np.float64)
    assert np.abs(d[:3] - want).max() < BOUND
    assert d[3] == 0.0 and w[3] == int(np.argmax(x[1:] >= lo[0]))       # first pierced segment
    slab = M.box_mesh([-0.4, -0.01, -0.4], [0.4, 0.01, 0.4]).astype(np.float32)
    y = -0.255 + 0.03 * np.arange(18)
    hop = np.stack([np.full(18, 0.1), y, np.full(18, -0.05)], 1).astype(np.float32)
    d, w = gpu_distance([hop], slab)
    from pntf import ops
    v = ops.point_mesh_distance(torch.from_numpy(hop).cuda(), torch.from_numpy(slab).cuda())
    assert v.min().item() > 0.004 and d[0] == 0.0 and w[0] == 8


def load_weights(net, dev):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()},
                        strict=True)
    net.to(dev).float().eval()


@pytest.mark.gpu
def test_plan_then_plan_report_end_to_end():
    from models import model_res_sigmoid_multi as md
    dev = torch.device("cuda:0")
    m = md.Model(".", ".", 3, 2, device="cuda:0")
    m.network = md.NN("cuda:0", 3)
    load_weights(m.network, dev)
    B = torch.from_numpy(synth.make_B(3)).to(dev)
    xp = torch.from_numpy(synth.make_pairs(5, 3, seed=11)).to(dev)
    tol, safety, max_iter = 0.06, 0.01, 20
    path, steps = m.Plan(xp, B, step=0.03, tol=tol, max_iter=max_iter)
    tris = M.box_mesh([-0.1, -0.1, -0.1], [0.1, 0.15, 0.1]).astype(np.float32)
    rep = m.PlanReport(path, steps, torch.from_numpy(tris), tol=tol, safety=safety)
    P, s = path.cpu().numpy(), steps.cpu().numpy()
    for c in range(5):
        line = loop_polyline(P[c], int(s[c]))
        gap = np.linalg.norm(P[c, s[c], 3:].astype(np.float64) - P[c, s[c], :3])
        assert abs(gap - tol) > 1e-6                      # the fp32 norm decides the same way
        dist, where, runner = S.polyline_distance(line, tris)
        length = np.linalg.norm(np.diff(line.astype(np.float64), axis=0), axis=1).sum()
        assert bool(rep.converged[c]) == (gap <= tol)
        assert abs(float(rep.length[c]) - length) < 1e-12
        assert abs(float(rep.clearance[c]) - dist) < BOUND and abs(dist - safety) > BOUND
        if runner > dist + BOUND:
            assert int(rep.where[c]) == where
        assert bool(rep.success[c]) == ((gap <= tol) and dist > safety)
    assert rep.success_rate == float(rep.success.double().mean())
    assert rep.clearance.dtype == torch.float32 and rep.where.dtype == torch.int32


@pytest.mark.gpu
def test_arm_plan_report_equals_oracle_on_the_same_samples():
    from models import model_res_sigmoid as ma
    from pntf import ops
    dev = torch.device("cuda:0")
    m = ma.Model(".", ".", 6, device="cuda:0")
    m.B = torch.from_numpy(synth.make_B(6, seed=12, arm=True))
    m.network = ma.NN("cuda:0", 6, m.B)
    load_weights(m.network, dev)
    xp = torch.from_numpy(synth.make_box_pairs(3, 6, seed=3) * 0.3).to(dev)
    tol, max_iter, res = 0.03, 20, 0.05
    path, steps = m.Plan(xp, step=0.015, tol=tol, max_iter=max_iter)
    rng = np.random.default_rng(6)
    text, spec, names = A.revolute_arm_urdf(6)
    chain = kin.SerialChain.from_urdf(text, names[-1])
    verts = [np.zeros((0, 3), np.float32)] * 2 + [A.link_blob(rng, 20).astype(np.float32)
                                                  for _ in range(6)]
    tris = M.box_mesh([0.15, -0.2, -0.2], [0.45, 0.2, 0.2]).astype(np.float32)
    rep = m.PlanReport(path, steps, chain, [torch.from_numpy(v).to(dev) for v in verts],
                       torch.from_numpy(tris), tol=tol, safety=0.005, resolution=res)
    # the same subdivided configurations, built on the CPU from the returned path
    pts, cnt = ops.plan_polylines(path.cpu(), steps.cpu())
    theta, qi, si = evaluate.arm_path_samples(pts, cnt, res)
    assert np.abs(np.diff(theta.numpy(), axis=0))[np.diff(qi.numpy()) == 0].max() <= res * 1.001
    d = A.arm_mesh_distance(spec, theta.numpy().astype(np.float64), verts, tris)
    for c in range(3):
        mine = d[qi.numpy() == c]
        assert abs(float(rep.clearance[c]) - mine.min()) < ARM_TOL
        near = si.numpy()[qi.numpy() == c][mine <= mine.min() + 2 * ARM_TOL]
        assert int(rep.where[c]) in near
        assert bool(rep.success[c]) == (bool(rep.converged[c]) and mine.min() > 0.005)
        assert abs(mine.min() - 0.005) > ARM_TOL
