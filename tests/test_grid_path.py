"""Grid paths: the descent and polyline-time kernels (pntf_grid_descent,
pntf_grid_polyline_time), ops.grid_descent, ops.grid_polyline_time,
pntf.evaluate.path_optimality and Model.PlanOptimality.

Pinning: the reference has no grid baseline, so the numpy oracle (tests/gridpath_oracle.py, a
restatement of include/pntf.h) is pinned here by closed forms: affine fields, a status per
construction, uniform speed, the exact distance field.

GPU bound, in the form of tests/test_eikonal_grid.py: the kernels and the oracle read the same
fp32 arrays (the fp64 oracle solve of scene(n) rounded to fp32, and that scene's speed), so the
HIP solver's rounding does not enter.  Per case e32 = oracle(fp32) against oracle(fp64), maximum
over the case's queries, and the kernel must stay within 4 x e32 of the fp64 oracle: for the
descent in tgoal and in the maximum distance from its points to the oracle's polyline, with the
status equal and cnt within 1 (the arrival test may flip at one step); for the polyline time in
time, with the +inf pattern equal.  Every descent query keeps e32 <= 0.05 h (asserted on the CPU):
that keeps the cases away from the field's cut loci, where any two roundings part ways.

Worst measured kernel errors against the fp64 oracle on an MI355X: WORST_DESCENT and WORST_TIME
below.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eikonal_oracle as E
import gridpath_oracle as G
from oracle import mesh_oracle as M
from pntf import _lib, evaluate, synth
from test_eikonal_grid import CORNER, FACE, OFF, SEALED, reference, scene, uniform

# measured on an MI355X, from the parity tests' prints; documentation only, nothing reads it.
# (n, radius, step) -> (kernel path error, e32 of the path, kernel tgoal error, e32 of tgoal)
# The kernel's errors equal the fp32 oracle's to every printed digit: with no FMA contraction and
# the same order of operations the two compute the same roundings.
WORST_DESCENT = {(9, 0, 0.5): (4.01e-7, 4.01e-7, 1.26e-7, 1.26e-7),
                 (9, 0, 1.0): (6.99e-7, 6.99e-7, 1.26e-7, 1.26e-7),
                 (9, 4, 0.5): (2.23e-6, 2.23e-6, 9.59e-8, 9.59e-8),
                 (9, 4, 1.0): (1.55e-6, 1.55e-6, 9.59e-8, 9.59e-8),
                 (17, 0, 0.5): (1.77e-6, 1.77e-6, 4.70e-7, 4.70e-7),
                 (17, 0, 1.0): (1.65e-6, 1.65e-6, 4.70e-7, 4.70e-7),
                 (17, 4, 0.5): (2.98e-7, 2.98e-7, 3.64e-8, 3.64e-8),
                 (17, 4, 1.0): (5.83e-7, 5.83e-7, 3.64e-8, 3.64e-8),
                 (33, 0, 0.5): (1.35e-6, 1.35e-6, 1.03e-7, 1.03e-7),
                 (33, 0, 1.0): (2.36e-5, 2.36e-5, 1.03e-7, 1.03e-7),
                 (33, 4, 0.5): (3.32e-7, 3.32e-7, 3.74e-7, 3.74e-7),
                 (33, 4, 1.0): (1.19e-5, 1.19e-5, 3.74e-7, 3.74e-7)}
# n -> (kernel time error, e32), times up to 101, 59 and 41
WORST_TIME = {9: (1.09e-5, 1.09e-5), 17: (3.31e-6, 3.31e-6), 33: (1.59e-4, 1.59e-4)}

SIZES = [9, 17, 33]
RADII = [0.0, 4.0]
STEPS = [0.5, 1.0]


# ------------------------------------------------------------------ CPU: oracle pinning


def affine(n, a, b=0.0):
    return E.nodes(n) @ np.asarray(a, np.float64) + b


def test_oracle_interpolation_reproduces_affine_functions():
    n, a, b = 9, np.array([0.7, -1.3, 2.1]), 0.4
    A = affine(n, a, b)
    h = 1.0 / (n - 1)
    x = np.array([[0.1234, -0.3121, 0.0417],        # interior
                  [0.5, 0.2 * h, -0.31],            # on the face x = +0.5
                  [-0.5, -0.5, 0.13],               # on an edge
                  [0.5, 0.5, 0.5], [-0.5, -0.5, -0.5],       # box corners
                  [-0.5 + 3 * h, -0.5 + 2 * h, -0.5 + 5 * h],  # exactly a node
                  [0.9, -0.2, 7.0]])                # outside: clamped to (0.5, -0.2, 0.5)
    V, g, blocked = G.interp(A, x)
    assert not blocked.any()
    assert np.abs(V - (G.clamp(x) @ a + b)).max() <= 1e-14
    assert np.abs(g - a).max() <= 1e-14
    i, w = G.cell(x, n)
    assert i.min() >= 0 and i.max() <= n - 2 and w.min() >= 0 and w.max() <= 1
    assert i[3].tolist() == [n - 2] * 3 and w[3].tolist() == [1.0] * 3
    # a NaN or infinite coordinate lands in range too
    i, w = G.cell(np.array([[np.nan, np.inf, -np.inf]]), n)
    assert i.min() >= 0 and i.max() <= n - 2 and np.isfinite(w).all()
    i, w = G.cell(np.array([[np.nan, np.inf, -np.inf]], np.float32), n)
    assert i.min() >= 0 and i.max() <= n - 2 and np.isfinite(w).all()
    # blocked: a non-finite corner; for the speed array also a corner <= 0
    B = A.copy()
    B[3, 2, 5] = np.inf
    hit = np.array([-0.5 + 2.5 * h, -0.5 + 1.5 * h, -0.5 + 4.5 * h])
    assert G.interp(B, hit[None])[2][0] and not G.interp(B, hit[None] + 2 * h)[2][0]
    Z = np.abs(A) + 1.0
    assert not G.interp(Z, hit[None], positive=True)[2][0]
    Z[3, 2, 5] = 0.0
    assert G.interp(Z, hit[None], positive=True)[2][0] and not G.interp(Z, hit[None])[2][0]


def test_oracle_affine_field_gives_the_straight_descent():
    """T = a . x with |a| = 3 on the 17^3 grid (dyadic nodes: T is exact in fp32).  The path is
    goal - k step h a/|a| until the ball test |x_k - x_s| <= max(radius, 2) h first holds, then
    x_s."""
    n, a = 17, np.array([2.0, 1.0, 2.0])
    h, unit = 1.0 / (n - 1), a / 3.0
    T = affine(n, a)[None].astype(np.float32)
    assert np.array_equal(T.astype(np.float64), affine(n, a)[None])
    goal = np.array([0.31, 0.12, 0.27], np.float32)
    for radius, step in ((0.0, 0.5), (4.0, 0.5), (3.0, 1.0), (0.0, 0.3)):
        D = 0.61
        src = (goal.astype(np.float64) - D * unit).astype(np.float32)
        Dx = np.linalg.norm(goal.astype(np.float64) - src)
        s, r = float(np.float32(step)) * h, max(radius, 2.0) * h
        k = int(np.ceil((Dx - r) / s))
        assert abs((Dx - r) / s - round((Dx - r) / s)) > 1e-3        # not a borderline count
        pts, cnt, status, tgoal = G.descent(T, src, goal, radius, step)
        assert status[0] == G.ARRIVED and cnt[0] == k + 2
        want = goal.astype(np.float64) - np.arange(k + 1)[:, None] * s * unit
        assert np.abs(pts[0, :k + 1] - want).max() <= 1e-13
        assert np.array_equal(pts[0, k + 1], src.astype(np.float64))
        assert not pts[0, k + 2:].any()
        assert abs(tgoal[0] - goal.astype(np.float64) @ a) <= 1e-14
        # the same in fp32, to fp32 accuracy
        p32, c32, s32, _ = G.descent(T, src, goal, radius, step, dtype=np.float32)
        assert p32.dtype == np.float32 and s32[0] == G.ARRIVED and abs(int(c32[0]) - k - 2) <= 1
        assert G.path_distance(p32, c32, pts, cnt)[0] <= 1e-5


def test_oracle_reaches_each_status_once_by_construction():
    n, a = 17, np.array([2.0, 1.0, 2.0])
    h = 1.0 / (n - 1)
    T = affine(n, a)[None].astype(np.float32)
    goal = np.array([0.31, 0.12, 0.27], np.float32)
    src = (goal - 0.61 * a / 3.0).astype(np.float32)
    run = lambda T, s, g, **kw: [v[0] for v in G.descent(T, s, g, **kw)]
    pts, cnt, status, _ = run(T, src, goal, radius=0.0)
    assert status == G.ARRIVED
    # L exactly sufficient, and one less
    assert run(T, src, goal, radius=0.0, L=int(cnt))[1:3] == [cnt, G.ARRIVED]
    p, c, s, _ = run(T, src, goal, radius=0.0, L=int(cnt) - 1)
    assert (c, s) == (cnt - 1, G.TRUNCATED) and np.array_equal(p, pts[:cnt - 1])
    p, c, s, _ = run(T, src, goal, radius=0.0, L=2)
    assert (c, s) == (2, G.TRUNCATED) and np.array_equal(p, pts[:2])
    # goal = source: one point; goal inside the ball: two
    assert run(T, src, src, radius=0.0)[1:3] == [1, G.ARRIVED]
    near = (src + np.float32(h) * np.array([0.9, -0.7, 0.5], np.float32)).astype(np.float32)
    p, c, s, _ = run(T, src, near, radius=0.0)
    assert (c, s) == (2, G.ARRIVED) and np.array_equal(p[1], src.astype(np.float64))
    p, c, s, _ = run(T, src, near, radius=0.0, L=2)
    assert (c, s) == (2, G.ARRIVED)
    # STALLED: a flat field; and a descent that runs into the box corner far from the source
    flat = np.ones_like(T)
    assert run(flat, src, goal)[1:3] == [1, G.STALLED]
    far = np.array([0.4, 0.4, 0.4], np.float32)
    p, c, s, _ = run(T, far, goal, radius=0.0)
    assert s == G.STALLED and np.array_equal(p[c - 1], [-0.5, -0.5, -0.5])
    # BLOCKED: a +inf node on the way; UNREACHABLE: the goal's own cell has it
    wall = T.copy()
    mid = goal.astype(np.float64) - 0.3 * a / 3.0
    wall[(0,) + tuple(G.cell(mid[None], n)[0][0])] = np.inf
    p, c, s, t = run(wall, src, goal, radius=0.0)
    assert s == G.BLOCKED and 1 < c < cnt and np.isfinite(t)
    assert not G.interp(wall[0], p[:c])[2].any()
    p, c, s, t = run(wall, src, mid.astype(np.float32), radius=0.0)
    assert (c, s) == (1, G.UNREACHABLE) and np.isinf(t)
    # the sealed shell of the solver's scene: no path leads out of it
    S, srcs = scene(9)
    T64, _, _ = reference(9, 0.0)
    p, c, s, t = run(T64[CORNER:CORNER + 1].astype(np.float32), srcs[CORNER], srcs[SEALED],
                     radius=0.0)
    assert (c, s) == (1, G.UNREACHABLE) and np.isinf(t) and not p[1:].any()


def test_oracle_descends_through_the_window_of_the_wall():
    """The source in front of the first slab's 2x2 window, the goal 4.3 h behind the slab.  Every
    cell that touches a wall node is blocked, so the window is a tunnel one cell wide: the path
    has to thread it.  (Scene-wide goals rarely arrive here: the speed jumps up to tenfold from
    node to node, and a fixed step then fails to lower T or meets a wall's cell.)"""
    n = 17
    S, _ = scene(n)
    h, a = 1.0 / (n - 1), n // 3
    src = (-0.5 + h * np.array([2.5, 1.5, 1.5])).astype(np.float32)
    goal = (-0.5 + h * np.array([9.3, 1.5, 1.5])).astype(np.float32)
    assert (S[a] == 0).sum() == n * n - 4 and (S[a, 1:3, 1:3] > 0).all()
    T64, _ = E.solve(S, src[None], 4.0)
    T = T64.astype(np.float32)
    pts, cnt, status, tgoal = G.descent(T, src, goal, 4.0, 0.25)
    k = int(cnt[0])
    assert status[0] == G.ARRIVED and k > 10 and np.isfinite(tgoal[0])
    V, _, blocked = G.interp(T[0], pts[0, :k - 1])               # the last point is the source
    assert not blocked.any() and (np.diff(V) < 0).all() and V[0] == tgoal[0]
    assert np.array_equal(pts[0, k - 1], src.astype(np.float64))
    u = (pts[0, :k, 0] + 0.5) / h                                # from behind the slab to its front
    assert u[0] > a + 4 and u[k - 2] > a and u[k - 1] < a


def test_oracle_polyline_time_under_uniform_speed():
    n = 17
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.5, 0.5, (4, 40, 3)).astype(np.float32)
    pts[1, 7] = pts[1, 6]                                        # a repeated point
    pts[2, 3] = [0.9, -0.7, 0.2]                                 # a point outside the box
    cnt = np.array([40, 23, 300, 2])                             # 300: clamped to L
    length = np.array([np.linalg.norm(np.diff(pts[c, :min(k, 40)].astype(np.float64), axis=0),
                                      axis=1).sum() for c, k in enumerate(cnt)])
    for s in (1.0, 0.37):
        t = G.polyline_time(uniform(n, s), pts, cnt)
        assert np.abs(t - length / np.float64(np.float32(s))).max() <= 1e-12
    for dtype in (np.float64, np.float32):
        S = scene(n)[0] + np.float32(0.25)                       # no walls
        t1 = G.polyline_time(S, pts, cnt, dtype=dtype)
        t2 = G.polyline_time(2 * S, pts, cnt, dtype=dtype)
        assert t1.dtype == dtype and np.array_equal(t2, t1 / 2) and (t1 > 0).all()
    assert np.array_equal(G.polyline_time(uniform(n), pts, [0, 1, -3, 1]), np.zeros(4))
    # a midpoint in a wall cell
    S = uniform(n)
    S[8, 8, 8] = 0.0
    line = np.zeros((2, 2, 3), np.float32)
    line[0] = [[-0.4, 0.01, 0.01], [0.4, 0.01, 0.01]]            # through the wall node's cells
    line[1] = [[-0.4, 0.3, 0.3], [0.4, 0.3, 0.3]]
    t = G.polyline_time(S, line, [2, 2])
    assert np.isinf(t[0]) and abs(t[1] - 0.8) <= 1e-6


# the grid's own numbers under uniform speed, from this test's print:
# n -> (worst path-length excess over |g - s|, relative; worst floor_rel)
MEASURED_FLOOR = {17: (8.55e-4, 8.55e-4), 33: (3.75e-4, 3.75e-4)}


@pytest.mark.parametrize("n", [17, 33])
def test_oracle_exact_distance_field_path_is_nearly_straight(n):
    """With T the nodes' exact distance to the source over a uniform speed, the descent's length
    can only exceed |g - s|; the excess and floor_rel are the grid's own numbers at this n.  The
    bound on the excess is the recorded value (MEASURED_FLOOR, as measured by this test, not
    chosen) times 2."""
    s = np.float32(0.6)
    src = np.array([[0.3237, -0.2213, 0.1771]], np.float32)
    goals = np.array([[-0.41, 0.33, -0.07], [-0.45, -0.48, -0.44], [0.5, 0.5, -0.5],
                      [-0.2, 0.4, 0.45]], np.float32)
    dist = np.linalg.norm(E.nodes(n) - src[0].astype(np.float64), axis=-1)
    T = np.repeat((dist / np.float64(s))[None], len(goals), axis=0).astype(np.float32)
    pts, cnt, status, tgoal = G.descent(T, np.repeat(src, len(goals), 0), goals, 4.0, 0.5)
    assert (status == G.ARRIVED).all()
    straight = np.linalg.norm(goals.astype(np.float64) - src[0], axis=1)
    length = np.array([np.linalg.norm(np.diff(pts[c, :cnt[c]], axis=0), axis=1).sum()
                       for c in range(len(goals))])
    time = G.polyline_time(uniform(n, s), pts, cnt)
    excess = (length / straight - 1).max()
    floor = (np.abs(time - tgoal) / tgoal).max()
    print("exact distance field, n=%d: length excess %.3g, floor_rel %.3g" % (n, excess, floor))
    assert (length >= straight * (1 - 1e-12)).all()
    assert excess <= 2 * MEASURED_FLOOR[n][0] and floor <= 2 * MEASURED_FLOOR[n][1]


# ------------------------------------------------------------------ the parity cases


@functools.lru_cache(maxsize=None)
def arrays(n, radius):
    """(T (3, n, n, n) fp32: the fp64 oracle solve of scene(n) from its CORNER, FACE and OFF
    sources, rounded; speed (n, n, n); sources (3, 3))."""
    S, src = scene(n)
    T64, _, _ = reference(n, radius)
    T = T64[[CORNER, FACE, OFF]].astype(np.float32)
    T.setflags(write=False)
    return T, S, src[[CORNER, FACE, OFF]]


def goals_of(n, src, k):
    """The goals of source k: on a box face, at a box corner, inside the init ball, the source
    itself, inside the sealed shell, and free ones."""
    h = np.float32(1.0 / (n - 1))
    inward = -np.sign(src + np.float32(1e-3)).astype(np.float32)
    _, srcs = scene(n)
    free = [src + h * inward * np.array(FREE_OFFSETS[n], np.float32)] if k == 0 else []
    return [np.array(FACE_GOALS[k], np.float32), np.array(CORNER_GOALS[k], np.float32),
            src + h * inward * np.array([0.3, 0.2, 0.25], np.float32), src.copy(),
            srcs[SEALED].copy()] + free


FACE_GOALS = [(0.5, 0.1234, -0.21), (-0.5, -0.3121, 0.2417), (-0.1234, 0.5, -0.3121)]
CORNER_GOALS = [(0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (-0.5, 0.5, -0.5)]
# The free goal of the CORNER source, in units of h from it: 6 to 8 cells away, in the same
# chamber, picked on the CPU so that the oracle's descent ARRIVES after several steps for every
# radius and step (scene(n)'s speed jumps up to tenfold from node to node, so a fixed step often
# fails to lower T or meets a wall's cell: most goals across the box end STALLED or BLOCKED).
FREE_OFFSETS = {9: (4.4, 4.6, 0.3), 17: (2.5, 2.5, 5.5), 33: (5.5, 3.5, 4.5)}
KINDS = ["face", "corner", "ball", "source", "sealed", "free"]
FREE = 5                                    # the free goal's query: a long path that ARRIVES


@functools.lru_cache(maxsize=None)
def case(n, radius, step):
    """The queries of one parity case and the oracle's answers: computed once, never modified."""
    T3, S, src3 = arrays(n, radius)
    row, goal, kind = [], [], []
    for k in range(3):
        for i, g in enumerate(goals_of(n, src3[k], k)):
            row.append(k), goal.append(g), kind.append(KINDS[min(i, 5)])
    row, goal = np.array(row), np.stack(goal)
    assert len(row) <= 16
    src = src3[row]
    T = T3[row]
    ref = G.descent(T, src, goal, radius, step)
    r32 = G.descent(T, src, goal, radius, step, dtype=np.float32)
    fin = np.isfinite(ref[3])
    e_path = G.path_distance(r32[0], r32[1], ref[0], ref[1])
    e_t = np.where(fin, np.abs(r32[3].astype(np.float64) - np.where(fin, ref[3], 0)), 0.0)
    return dict(T=T, S=S, src=src, goal=goal, kind=kind, row=row, ref=ref, r32=r32, e_path=e_path,
                e_t=e_t)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n", SIZES)
def test_cases_stay_off_the_cut_loci(n, radius, step):
    """Every descent query of the GPU cases: the fp32 and fp64 oracles agree in status, in cnt
    within 1 and in the path within 0.05 h, and the cases hold the kinds they are meant to."""
    c = case(n, radius, step)
    pts, cnt, status, tgoal = c["ref"]
    p32, c32, s32, t32 = c["r32"]
    h = 1.0 / (n - 1)
    print("n=%d radius=%g step=%g: status %s cnt %s e32 path %.3g h, tgoal %.3g"
          % (n, radius, step, status.tolist(), cnt.tolist(), c["e_path"].max() / h,
             c["e_t"].max()))
    assert np.array_equal(status, s32) and np.abs(cnt - c32).max() <= 1
    assert np.array_equal(np.isinf(tgoal), np.isinf(t32))
    assert c["e_path"].max() <= 0.05 * h
    for i, kind in enumerate(c["kind"]):
        if kind == "sealed":
            assert (status[i], cnt[i]) == (G.UNREACHABLE, 1)
        if kind == "source":
            assert (status[i], cnt[i]) == (G.ARRIVED, 1)
        if kind == "ball":
            assert (status[i], cnt[i]) == (G.ARRIVED, 2)
    # scene(n)'s speed jumps up to tenfold from node to node, so a fixed step often fails to
    # lower T (STALLED) or meets a wall's cell (BLOCKED): those ends are compared like any other
    far = np.isin(np.array(c["kind"]), ("face", "corner", "free"))
    assert (cnt[far] > 3).sum() >= 3
    assert c["kind"][FREE] == "free" and status[FREE] == G.ARRIVED and cnt[FREE] >= 5
    assert (np.abs(c["goal"]).max(axis=1) == 0.5).sum() >= 6


def lines_of(n):
    """Polylines for the time kernel: ragged cnt {0, 1, 2, 257, 513} with L = 520, repeated
    points, points outside the box, one polyline through a wall cell, and a descent path."""
    rng = np.random.default_rng(40 + n)
    S, _ = scene(n)
    L = 520
    pts = np.zeros((7, L, 3), np.float32)
    walk = np.cumsum(rng.normal(0, 0.4 / (n - 1), (5, L, 3)), axis=1)
    pts[:5] = (walk - walk.mean(axis=1, keepdims=True)).astype(np.float32)
    # keep rows 0..4 out of the shell and the slabs: a thin slice next to the i = 0 face
    pts[:5, :, 0] = (-0.5 + (0.9 / (n - 1)) * rng.uniform(0, 1, (5, L))).astype(np.float32)
    pts[3, 100] = pts[3, 99]
    pts[3, 300:303] = pts[3, 299]
    pts[4, 10] = [-0.8, 0.9, 0.1]
    pts[4, 400] = [-0.51, -3.0, 0.7]
    cnt = np.array([0, 1, 2, 257, 513, 2, 0], np.int32)
    c = n // 2
    x = -0.5 + (c + 0.5) / (n - 1)
    pts[5, :2] = [[x, x, -0.5], [x, x, 0.5]]                     # through the shell
    ref = case(n, 4.0, 0.5)["ref"]
    k = int(np.argmax(ref[1]))
    m = min(int(ref[1][k]), L)
    pts[6, :m], cnt[6] = ref[0][k, :m].astype(np.float32), m
    return S, pts, cnt


@functools.lru_cache(maxsize=None)
def time_case(n):
    S, pts, cnt = lines_of(n)
    t64 = G.polyline_time(S, pts, cnt)
    t32 = G.polyline_time(S, pts, cnt, dtype=np.float32)
    return S, pts, cnt, t64, t32


@pytest.mark.parametrize("n", SIZES)
def test_time_cases_hold_what_they_are_meant_to(n):
    S, pts, cnt, t64, t32 = time_case(n)
    assert np.array_equal(np.isinf(t64), np.isinf(t32))
    assert np.isinf(t64).tolist() == [False] * 5 + [True, False]
    assert t64[0] == 0 and t64[1] == 0 and (t64[[2, 3, 4, 6]] > 0).all()
    assert np.abs(pts[4, :513]).max() > 0.5 and (S > 0).all() == False   # noqa: E712


# ------------------------------------------------------------------ CPU: library and torch layers


def test_grid_path_rejections_without_gpu():
    """Every rejection of include/pntf.h returns nonzero on the host; the fake pointers are
    never dereferenced."""
    L = _lib.load()
    fake = ctypes.c_void_p(64)

    def descent(T=fake, n=9, q=3, src=fake, goal=fake, radius=4.0, step=0.5, rows=40, pts=fake,
                cnt=fake, status=fake, tgoal=fake):
        return L.pntf_grid_descent(T, n, q, src, goal, radius, step, rows, pts, cnt, status,
                                   tgoal, None)

    def time(speed=fake, n=9, pts=fake, q=3, rows=40, cnt=fake, sub=0.5, out=fake):
        return L.pntf_grid_polyline_time(speed, n, pts, q, rows, cnt, sub, out, None)

    nan = float("nan")
    bad = [(dict(n=1), b"n must be >= 2"), (dict(q=0), b"q must be >= 1"),
           (dict(radius=-1.0), b"radius"), (dict(radius=nan), b"radius"),
           (dict(step=0.0), b"step"), (dict(step=1.5), b"step"), (dict(step=nan), b"step"),
           (dict(rows=1), b"L must be >= 2"), (dict(T=None), b"null"), (dict(src=None), b"null"),
           (dict(goal=None), b"null"), (dict(pts=None), b"null"), (dict(cnt=None), b"null"),
           (dict(status=None), b"null"), (dict(tgoal=None), b"null"),
           (dict(n=1625), b"launch limits"), (dict(q=2 ** 35), b"launch limits")]
    for kw, text in bad:
        assert L.pntf_point_mesh_distance(None, 5, None, 3, None, 0, None) == 1   # other text
        assert descent(**kw) == 1, kw
        err = L.pntf_mesh_last_error()
        assert b"pntf_grid_descent" in err and text in err, (kw, err)
    bad = [(dict(n=1), b"n must be >= 2"), (dict(q=0), b"q must be >= 1"),
           (dict(rows=0), b"L must be >= 1"), (dict(sub=0.0), b"sub"), (dict(sub=-1.0), b"sub"),
           (dict(sub=nan), b"sub"), (dict(speed=None), b"null"), (dict(pts=None), b"null"),
           (dict(cnt=None), b"null"), (dict(out=None), b"null"),
           (dict(n=1625), b"launch limits"), (dict(q=2 ** 31), b"launch limits")]
    for kw, text in bad:
        assert L.pntf_point_mesh_distance(None, 5, None, 3, None, 0, None) == 1
        assert time(**kw) == 1, kw
        err = L.pntf_mesh_last_error()
        assert b"pntf_grid_polyline_time" in err and text in err, (kw, err)
    with pytest.raises(_lib.PntfError, match="step"):
        _lib.check(descent(step=2.0), "pntf_grid_descent")


def test_grid_path_ops_have_no_cpu_path():
    from pntf import ops
    with pytest.raises(_lib.PntfError, match="HIP device"):
        ops.grid_descent(torch.ones(1, 9, 9, 9), torch.zeros(1, 3), torch.zeros(1, 3))
    with pytest.raises(_lib.PntfError, match="HIP device"):
        ops.grid_polyline_time(torch.ones(9, 9, 9), torch.zeros(1, 4, 3),
                               torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.PntfError, match="HIP device"):
        evaluate.path_optimality(torch.zeros(1, 5, 6), torch.zeros(1, dtype=torch.int32),
                                 torch.zeros(1, 3, 3))


# ------------------------------------------------------------------ GPU


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the cached cases stay read-only


def gpu_descent(T, src, goal, radius, step, L=None):
    from pntf import ops
    out = ops.grid_descent(dev(T), dev(src), dev(goal), radius=radius, step=step, max_points=L)
    pts, cnt, status, tgoal = (t.cpu().numpy() for t in out)
    q, n = T.shape[0], T.shape[1]
    assert pts.shape == (q, G.default_points(n, step) if L is None else L, 3)
    assert pts.dtype == np.float32 and cnt.dtype == np.int32 and status.dtype == np.int32
    for c in range(q):
        assert cnt[c] >= 1 and not pts[c, cnt[c]:].any()
    return pts, cnt, status, tgoal


@pytest.mark.gpu
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n", SIZES)
def test_hip_grid_descent_matches_oracle(n, radius, step):
    c = case(n, radius, step)
    rp, rc, rs, rt = c["ref"]
    pts, cnt, status, tgoal = gpu_descent(c["T"], c["src"], c["goal"], radius, step)
    e_path, e_t = float(c["e_path"].max()), float(c["e_t"].max())
    fin = np.isfinite(rt)
    k_path = float(G.path_distance(pts, cnt, rp, rc).max())
    k_t = float(np.abs(tgoal[fin] - rt[fin]).max())
    h = 1.0 / (n - 1)
    print("grid descent vs fp64 oracle, n=%d radius=%g step=%g: path error %.3g (e32 %.3g = "
          "%.3g h), tgoal error %.3g (e32 %.3g), cnt %s"
          % (n, radius, step, k_path, e_path, e_path / h, k_t, e_t, cnt.tolist()))
    assert np.array_equal(status, rs)
    assert np.abs(cnt.astype(np.int64) - rc).max() <= 1
    assert np.array_equal(np.isinf(tgoal), ~fin) and (tgoal[~fin] > 0).all()
    assert k_t <= 4 * e_t
    assert k_path <= 4 * e_path
    assert np.array_equal(pts[:, 0], G.clamp(c["goal"]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 33])
def test_hip_grid_descent_bits_do_not_depend_on_batch_or_L(n):
    """A query alone equals the same query at positions 0, 7 and 8 of a batch of 9 (across the
    8-per-wave boundary), and for two values of L, both sufficient."""
    c = case(n, 4.0, 0.5)
    base = gpu_descent(c["T"], c["src"], c["goal"], 4.0, 0.5)
    Lmax = int(base[1].max())
    assert c["kind"][11] == "face" and c["row"][11] == 2
    assert base[2][FREE] == G.ARRIVED and base[1][FREE] >= 5
    for i in (FREE, 11):                    # the long arriving path; the face goal of OFF
        alone = gpu_descent(c["T"][i:i + 1], c["src"][i:i + 1], c["goal"][i:i + 1], 4.0, 0.5)
        k = int(alone[1][0])
        for a, b in zip(alone, base):
            assert a[0].tobytes() == b[i].tobytes()
        others = [j for j in range(len(c["row"])) if j != i]
        for pos in (0, 7, 8):
            idx = others[:pos] + [i] + others[pos:8]
            assert len(idx) == 9 and idx[pos] == i
            got = gpu_descent(c["T"][idx], c["src"][idx], c["goal"][idx], 4.0, 0.5)
            for a, b in zip(alone, got):
                assert a[0].tobytes() == b[pos].tobytes()
        for L in (Lmax, Lmax + 37):
            got = gpu_descent(c["T"][i:i + 1], c["src"][i:i + 1], c["goal"][i:i + 1], 4.0, 0.5,
                              L=L)
            assert got[1][0] == k and got[2][0] == alone[2][0] and got[3][0] == alone[3][0]
            assert got[0][0, :k].tobytes() == alone[0][0, :k].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 17])
def test_hip_grid_descent_truncates_at_L(n):
    """L exactly sufficient, one less, and L = 2: the same leading points, TRUNCATED.  The FREE
    query ARRIVES after several steps, so L = cnt - 1 stops the append of x_s itself: that guard
    is all that keeps x_s out of row L, which is the next query's row 0.  In a batch its
    neighbours come out as they do alone."""
    c = case(n, 4.0, 0.5)
    full = gpu_descent(c["T"], c["src"], c["goal"], 4.0, 0.5)
    k = int(full[1][FREE])
    assert full[2][FREE] == G.ARRIVED and k >= 5
    assert np.array_equal(full[0][FREE, k - 1], G.clamp(c["src"][FREE]))
    idx = [FREE - 1, FREE, FREE + 1]
    batch = gpu_descent(c["T"][idx], c["src"][idx], c["goal"][idx], 4.0, 0.5, L=k - 1)
    assert (batch[1][1], batch[2][1]) == (k - 1, G.TRUNCATED)
    assert batch[0][1].tobytes() == full[0][FREE, :k - 1].tobytes()
    for pos, i in ((0, FREE - 1), (2, FREE + 1)):
        alone = gpu_descent(c["T"][i:i + 1], c["src"][i:i + 1], c["goal"][i:i + 1], 4.0, 0.5,
                            L=k - 1)
        for a, b in zip(alone, batch):
            assert a[0].tobytes() == b[pos].tobytes()
        assert np.array_equal(batch[0][pos, 0], G.clamp(c["goal"][i]))
    for i, kind in enumerate(c["kind"][:6]):
        one = lambda L: gpu_descent(c["T"][i:i + 1], c["src"][i:i + 1], c["goal"][i:i + 1], 4.0,
                                    0.5, L=L)
        k = int(full[1][i])
        if k >= 2:
            p, cn, st, _ = one(k)
            assert (cn[0], st[0]) == (k, full[2][i]) and p[0].tobytes() == full[0][i, :k].tobytes()
        if k >= 3:
            p, cn, st, _ = one(k - 1)
            assert (cn[0], st[0]) == (k - 1, G.TRUNCATED)
            assert p[0].tobytes() == full[0][i, :k - 1].tobytes()
        p, cn, st, t = one(2)
        want = G.TRUNCATED if k > 2 else full[2][i]
        assert (cn[0], st[0]) == (min(k, 2), want) and t[0].tobytes() == full[3][i].tobytes()
        assert p[0, :cn[0]].tobytes() == full[0][i, :cn[0]].tobytes()


def gpu_time(S, pts, cnt, sub=0.5):
    from pntf import ops
    t = ops.grid_polyline_time(dev(S), dev(pts), dev(cnt), sub=sub)
    assert t.shape == (len(cnt),) and t.dtype == torch.float32
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_hip_grid_polyline_time_matches_oracle(n):
    S, pts, cnt, t64, t32 = time_case(n)
    fin = np.isfinite(t64)
    e32 = float(np.abs(t32[fin].astype(np.float64) - t64[fin]).max())
    got = gpu_time(S, pts, cnt)
    err = float(np.abs(got[fin] - t64[fin]).max())
    print("polyline time vs fp64 oracle, n=%d: max abs error %.3g, e32 %.3g, times %s"
          % (n, err, e32, got.tolist()))
    assert np.array_equal(np.isinf(got), ~fin) and (got[~fin] > 0).all()
    assert got[0] == 0.0 and got[1] == 0.0
    assert err <= 4 * e32
    # the same bits with other padding, in another batch order, and alone
    wide = np.concatenate([pts, np.full((len(cnt), 9, 3), 7.0, np.float32)], axis=1)
    assert gpu_time(S, wide, cnt).tobytes() == got.tobytes()
    assert gpu_time(S, pts[::-1], cnt[::-1])[::-1].tobytes() == got.tobytes()
    for c in (3, 4, 5):
        assert gpu_time(S, pts[c:c + 1], cnt[c:c + 1]).tobytes() == got[c:c + 1].tobytes()
    # doubling the speed halves every time exactly
    assert gpu_time(2 * S, pts, cnt).tobytes() == (got / 2).tobytes()


@pytest.mark.gpu
def test_grid_path_ops_reject_on_the_host():
    from pntf import ops
    T, S, src = arrays(9, 4.0)
    Td, Sd, sd = dev(T), dev(S), dev(src)
    cnt = torch.full((3,), 2, dtype=torch.int32).cuda()
    pts = torch.zeros(3, 4, 3).cuda()
    nan = sd.clone()
    nan[1, 2] = float("nan")
    bad = [lambda: ops.grid_descent(Td[0], sd, sd), lambda: ops.grid_descent(Td[:, :, :, :8], sd, sd),
           lambda: ops.grid_descent(Td, sd[:2], sd), lambda: ops.grid_descent(Td, sd, sd[:, :2]),
           lambda: ops.grid_descent(Td, sd, sd, step=0.0),
           lambda: ops.grid_descent(Td, sd, sd, step=1.01),
           lambda: ops.grid_descent(Td, sd, sd, radius=-1.0),
           lambda: ops.grid_descent(Td, sd, sd, max_points=1),
           lambda: ops.grid_descent(Td, nan, sd), lambda: ops.grid_descent(Td, sd, nan),
           lambda: ops.grid_descent(Td, sd.cpu(), sd),
           lambda: ops.grid_polyline_time(Sd[:8], pts, cnt),
           lambda: ops.grid_polyline_time(Sd, pts[:, :, :2], cnt),
           lambda: ops.grid_polyline_time(Sd, pts, cnt[:2]),
           lambda: ops.grid_polyline_time(Sd, pts, cnt.float()),
           lambda: ops.grid_polyline_time(Sd, pts, cnt, sub=0.0),
           lambda: ops.grid_polyline_time(Sd, pts, cnt, sub=-0.5),
           lambda: ops.grid_polyline_time(Sd, pts * float("inf"), cnt),
           lambda: ops.grid_polyline_time(Sd, pts, cnt.cpu())]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.PntfError):
            call()
            pytest.fail("call %d was accepted" % i)
    # q = 0: empty tensors, no launch
    out = ops.grid_descent(Td[:0], sd[:0], sd[:0])
    assert [tuple(t.shape) for t in out] == [(0, 66, 3), (0,), (0,), (0,)]
    assert ops.grid_polyline_time(Sd, pts[:0], cnt[:0]).shape == (0,)


BOX = (np.array([-0.2, -0.1, -0.15]), np.array([0.25, 0.2, 0.1]))


@pytest.mark.gpu
def test_plan_optimality_recomputed_from_the_returned_tensors():
    from models import model_res_sigmoid as ma
    from models import model_res_sigmoid_multi as md
    from pntf import ops
    d0 = torch.device("cuda:0")
    m = md.Model(".", ".", 3, 2, device="cuda:0")
    m.network = md.NN("cuda:0", 3)
    m.network.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()},
                              strict=True)
    m.network.to(d0).float().eval()
    n, margin, offset, radius, step, q = 17, 0.1, 0.01, 4.0, 0.5, 8
    Bt = torch.from_numpy(synth.make_B_table(2, 3)).to(d0)
    xp = torch.from_numpy(synth.make_pairs(q, 3, seed=11)).to(d0)
    env = torch.tensor([0, 1, 0, 5, 1, 0, 1, 0], dtype=torch.int32, device=d0)   # 5: no such env
    path, steps = m.Plan(xp, Bt, step=0.03, tol=0.06, max_iter=20, env=env)
    assert steps.tolist()[3] == -1 and (steps.cpu().numpy()[[0, 1, 2, 4, 5, 6, 7]] >= 0).all()
    tris = torch.from_numpy(M.box_mesh(*BOX).astype(np.float32))
    kw = dict(n=n, offset=offset, margin=margin, radius=radius, step=step)
    rep = m.PlanOptimality(path, steps, tris, **kw)
    # every number again from the tensors the layers below return, and the oracle
    S = ops.speed_grid(tris.to(d0), n, offset, margin)
    src, goal = path[:, 0, :3].contiguous(), path[:, 0, 3:].contiguous()
    T, _, conv = ops.grid_travel_time(S, src, radius=radius)
    Tn, Sn = T.cpu().numpy(), S.cpu().numpy()
    _, _, ds, dt = G.descent(Tn, src.cpu().numpy(), goal.cpu().numpy(), radius, step)
    d32 = G.descent(Tn, src.cpu().numpy(), goal.cpu().numpy(), radius, step, dtype=np.float32)
    # the descent's own points are the kernel's (its parity with the oracle is the test above):
    # they are priced and measured here by the oracle
    dp, dc, _, _ = (t.cpu().numpy() for t in ops.grid_descent(T, src, goal, radius=radius,
                                                               step=step))
    pp, pc = ops.plan_polylines(path, steps)
    pp, pc = pp.cpu().numpy(), pc.cpu().numpy()
    ptime = G.polyline_time(Sn, pp, pc)
    otime = G.polyline_time(Sn, dp, dc)
    plen = np.array([np.linalg.norm(np.diff(pp[c, :pc[c]].astype(np.float64), axis=0),
                                    axis=1).sum() for c in range(q)])
    olen = np.array([np.linalg.norm(np.diff(dp[c, :dc[c]].astype(np.float64), axis=0),
                                    axis=1).sum() for c in range(q)])
    got = {k: getattr(rep, k).cpu().numpy() for k in
           ("time", "length", "optimal_time", "optimal_path_time", "optimal_length", "time_ratio",
            "length_ratio", "floor_rel", "status", "solve_converged")}
    print("plan optimality: %s" % {k: v.tolist() for k, v in got.items()})
    assert np.array_equal(got["status"], ds) and np.array_equal(got["status"], d32[2])
    assert np.array_equal(got["solve_converged"], conv.cpu().numpy()) and conv.all().item()
    ok = (ds == G.ARRIVED) & np.isfinite(dt)
    planned = steps.cpu().numpy() >= 0
    assert ok.sum() >= 4 and planned.sum() == q - 1
    # tolerance: the kernels' rounding on these very inputs, 4 x the oracle's own fp32 error
    # (the parity bound)
    e_t = 4 * np.abs(d32[3].astype(np.float64) - dt)[ok].max()
    t32 = G.polyline_time(Sn, pp, pc, dtype=np.float32)
    e_p = 4 * np.abs(t32.astype(np.float64) - ptime)[planned].max()
    o32 = G.polyline_time(Sn, dp, dc, dtype=np.float32)
    e_o = 4 * np.abs(o32.astype(np.float64) - otime)[ok].max()
    for k in ("optimal_time", "optimal_path_time", "optimal_length", "floor_rel"):
        assert np.isfinite(got[k][ok]).all() and np.isnan(got[k][~ok]).all(), k
    for k in ("time", "length"):
        assert np.isfinite(got[k][planned]).all() and np.isnan(got[k][~planned]).all(), k
    for k in ("time_ratio", "length_ratio"):
        assert np.isfinite(got[k][ok & planned]).all() and np.isnan(got[k][~(ok & planned)]).all()
    assert np.abs(got["optimal_time"] - dt)[ok].max() <= e_t
    assert np.abs(got["time"] - ptime)[planned].max() <= e_p
    assert np.abs(got["optimal_path_time"] - otime)[ok].max() <= e_o
    assert np.abs(got["length"] - plen)[planned].max() <= 1e-12
    assert np.abs(got["optimal_length"] - olen)[ok].max() <= 1e-12
    both = ok & planned
    np.testing.assert_allclose(got["time_ratio"][both], (got["time"] / got["optimal_time"])[both],
                               rtol=1e-15)
    np.testing.assert_allclose(got["length_ratio"][both],
                               (got["length"] / got["optimal_length"])[both], rtol=1e-15)
    np.testing.assert_allclose(
        got["floor_rel"][ok],
        (np.abs(got["optimal_path_time"] - got["optimal_time"]) / got["optimal_time"])[ok],
        rtol=1e-15)
    assert (got["floor_rel"][ok] < 0.2).all()
    # chunk = 3 gives the same bits as chunk = 64
    rep3 = m.PlanOptimality(path, steps, tris, chunk=3, **kw)
    for f in ("time", "length", "optimal_time", "optimal_path_time", "optimal_length",
              "time_ratio", "length_ratio", "floor_rel", "status", "solve_converged"):
        a, b = getattr(rep, f).cpu().numpy(), getattr(rep3, f).cpu().numpy()
        assert a.tobytes() == b.tobytes(), f
    arm = ma.Model(".", ".", 6, device="cuda:0")
    with pytest.raises(_lib.PntfError, match="arm"):
        arm.PlanOptimality(path, steps, tris)
    m6 = md.Model(".", ".", 6, 2, device="cuda:0")
    with pytest.raises(_lib.PntfError, match="dim must be 3"):
        m6.PlanOptimality(path, steps, tris)
