"""Grid travel time: the Eikonal pass / init kernels (pntf_grid_travel_time_*),
ops.grid_travel_time, ops.speed_grid, pntf.evaluate.field_report and Model.FieldReport.

Pinning: the reference has no grid solver, so the fp64 oracle (tests/eikonal_oracle.py) is
pinned here by closed forms and by a heap-ordered fast-marching solve that shares only the
single-node update with it.

GPU bound: not fixed in advance.  For each parity case e32 = max |oracle(fp32) - oracle(fp64)|
over the case's sources and finite nodes is computed on the CPU — the scheme's own rounding in
the kernel's number format — and the kernel must stay within 4 x e32 of the fp64 oracle (four,
as in the other geometry kernels' bounds: FMA contraction and another operation order).  The
+inf pattern must equal the oracle's exactly.

Worst measured |kernel - oracle(fp64)| per case on an MI355X: WORST below, (n, radius) ->
(kernel error for inner 1, for inner 8, e32 of the case).  The largest ratio to e32 is 1.33
(n = 33, radius 0, inner 8: 1.15e-3 against e32 = 8.63e-4, T up to 6.5); the bound is 4.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eikonal_oracle as E
from oracle import mesh_oracle as M
from pntf import _lib, evaluate, synth

# measured on an MI355X, from the parity test's print; documentation only, nothing reads it
WORST = {(8, 0): (1.29e-5, 1.29e-5, 1.17e-5), (8, 4): (6.11e-6, 6.11e-6, 6.21e-6),
         (9, 0): (8.17e-6, 1.11e-5, 1.16e-5), (9, 4): (1.16e-5, 8.49e-6, 1.03e-5),
         (13, 0): (9.71e-5, 9.60e-5, 9.06e-5), (13, 4): (6.27e-5, 7.41e-5, 6.92e-5),
         (17, 0): (1.49e-4, 1.83e-4, 1.68e-4), (17, 4): (9.48e-5, 1.08e-4, 1.09e-4),
         (33, 0): (7.87e-4, 1.15e-3, 8.63e-4), (33, 4): (8.91e-4, 1.01e-3, 9.97e-4)}

SIZES = [8, 9, 13, 17, 33]
RADII = [0.0, 4.0]


# ------------------------------------------------------------------ scenes


@functools.lru_cache(maxsize=None)
def scene(n):
    """Random speed in [0.1, 1] (fp32) with a sealed 3^3 shell of walls around the centre node
    and, from n = 13, two wall slabs across the i axis, each with a 2x2 window in opposite
    corners.  Returns (speed (n, n, n), sources (4, 3) fp32: corner node, a node on a tile face,
    off-node, off-node inside the shell)."""
    rng = np.random.default_rng(100 + n)
    S = rng.uniform(0.1, 1.0, (n, n, n)).astype(np.float32)
    if n >= 13:
        a, b = n // 3, 2 * n // 3
        win_a, win_b = S[a, 1:3, 1:3].copy(), S[b, n - 3:n - 1, n - 3:n - 1].copy()
        S[a] = S[b] = 0.0
        S[a, 1:3, 1:3], S[b, n - 3:n - 1, n - 3:n - 1] = win_a, win_b
    c = n // 2
    mid = S[c, c, c]
    S[c - 1:c + 2, c - 1:c + 2, c - 1:c + 2] = 0.0
    S[c, c, c] = mid
    h = 1.0 / (n - 1)
    node = lambda i, j, k: -0.5 + h * np.array([i, j, k], np.float64)
    src = np.stack([node(0, 0, 0), node(2, 8 if n >= 9 else 7, 5), [0.3237, -0.2213, 0.1771],
                    node(c, c, c) + h * np.array([0.2, -0.3, 0.1])]).astype(np.float32)
    return S, src


CORNER, FACE, OFF, SEALED = range(4)
BATCHES = [(CORNER, FACE, OFF), (OFF, SEALED, CORNER)]


@functools.lru_cache(maxsize=None)
def reference(n, radius):
    """(T64 (4, n, n, n), e32, Jacobi sweeps) of scene(n): computed once, never modified."""
    S, src = scene(n)
    T64, sweeps = E.solve(S, src, radius, np.float64)
    T32, _ = E.solve(S, src, radius, np.float32)
    assert T32.dtype == np.float32 and np.array_equal(np.isinf(T32), np.isinf(T64))
    fin = np.isfinite(T64)
    e32 = float(np.abs(T32[fin].astype(np.float64) - T64[fin]).max())
    T64.setflags(write=False)
    return T64, e32, sweeps


def uniform(n, s=1.0):
    return np.full((n, n, n), s, np.float32)


# ------------------------------------------------------------------ CPU: oracle pinning


def test_oracle_uniform_speed_axis_lines_and_face_diagonal():
    n, s = 17, np.float32(0.7)
    h = 1.0 / (n - 1)
    src = (-0.5 + h * np.array([8, 8, 8])).astype(np.float32)          # exactly a node
    T, _ = E.solve(uniform(n, s), src, radius=0.0)
    T = T[0]
    assert T[8, 8, 8] == 0.0
    k = np.abs(np.arange(n) - 8)
    want = k * h / np.float64(s)
    for line in (T[:, 8, 8], T[8, :, 8], T[8, 8, :]):
        assert np.abs(line - want).max() <= 1e-15
    f = h / np.float64(s)
    for d in ((1, 1, 0), (1, 0, -1), (0, -1, 1)):
        assert abs(T[8 + d[0], 8 + d[1], 8 + d[2]] - f * (1 + 1 / np.sqrt(2))) <= 1e-15
    # the body diagonal neighbour: a = b = c = f(1 + 1/sqrt 2) -> t = a + f / sqrt 3
    assert abs(T[9, 9, 9] - f * (1 + 1 / np.sqrt(2) + 1 / np.sqrt(3))) <= 1e-15


def test_oracle_doubling_the_speed_halves_T_exactly():
    S, src = scene(9)
    for dtype in (np.float64, np.float32):
        T1, _ = E.solve(S, src[:3], 4.0, dtype)
        T2, _ = E.solve(2 * S, src[:3], 4.0, dtype)
        assert np.array_equal(T2, T1 / 2) and np.isfinite(T1).any()


def test_oracle_corridor_is_the_running_sum():
    n = 17                                                   # h = 1/16: the nodes are exact in fp32
    rng = np.random.default_rng(3)
    S = np.zeros((n, n, n), np.float32)
    S[:, 4, 7] = rng.uniform(0.1, 1.0, n).astype(np.float32)
    h = 1.0 / (n - 1)
    src = np.array([-0.5, -0.5 + 4 * h, -0.5 + 7 * h], np.float32)
    T, _ = E.solve(S, src, radius=0.0)
    f = h / S[:, 4, 7].astype(np.float64)
    want = np.concatenate([[0.0], np.cumsum(f[1:])])        # T_k = sum_{i=1..k} h / S_i
    assert np.array_equal(T[0, :, 4, 7], want)
    assert np.isinf(np.delete(T[0].reshape(n, -1), 4 * n + 7, axis=1)).all()


def test_oracle_equals_fast_marching_on_the_wall_and_window_case():
    S, src = scene(13)
    T64, _, _ = reference(13, 4.0)
    for c in (CORNER, OFF):
        F = E.fast_march(S, src[c], 4.0)
        assert np.array_equal(np.isinf(F), np.isinf(T64[c]))
        fin = np.isfinite(F)
        err = np.abs(F[fin] - T64[c][fin]).max()
        print("Jacobi vs fast marching, 13^3 source %d: %.3g (T up to %.3g)"
              % (c, err, F[fin].max()))
        assert err <= 1e-12 and F[fin].max() > 2.0


@pytest.mark.parametrize("n", [8, 13])
def test_oracle_sealed_region_stays_sealed(n):
    S, src = scene(n)
    T64, _, _ = reference(n, 0.0)
    c = n // 2
    assert S[c, c, c] > 0 and E.nearest_node(n, src[SEALED]) == (c, c, c)
    only = np.zeros(S.shape, bool)
    only[c, c, c] = True
    assert np.array_equal(np.isfinite(T64[SEALED]), only)
    for other in (CORNER, FACE, OFF):
        assert np.isinf(T64[other][c, c, c])
        assert np.array_equal(np.isfinite(T64[other]), (S > 0) & ~only)     # all the rest reached


def test_scenes_hold_the_cases_they_are_meant_to():
    for n in SIZES:
        S, src = scene(n)
        near = [E.nearest_node(n, s) for s in src]
        assert all(S[ijk] > 0 for ijk in near), (n, near)
        assert near[CORNER] == (0, 0, 0) and (near[FACE][1] % 8 in (0, 7))
        h = 1.0 / (n - 1)
        assert np.abs((src[OFF] + 0.5) / h - np.array(near[OFF])).min() > 0.01   # really off-node
        assert (S == 0).any() and S[S > 0].min() >= 0.1
    # the radius-4 ball of the sealed source reaches through the shell, as the scheme says
    T64, _, _ = reference(13, 4.0)
    assert np.isfinite(T64[SEALED]).sum() > 1


def floor_of(n, src, radius):
    """(mean, max) relative error of the uniform-speed solve against |x - x_s| outside the ball."""
    T, _ = E.solve(uniform(n), src, radius)
    dist = np.linalg.norm(E.nodes(n) - np.asarray(src, np.float32).astype(np.float64), axis=-1)
    assert (T[0] >= dist - 1e-14).all()                      # first order upwind overestimates
    out = ~E.ball(n, np.asarray(src, np.float32), radius)[0]
    rel = np.abs(T[0] - dist)[out] / dist[out]
    return rel.mean(), rel.max()


def test_oracle_uniform_speed_bounds_and_floor_decreases():
    src = [0.3237, -0.2213, 0.1771]
    f17, f33 = floor_of(17, src, 4.0), floor_of(33, src, 4.0)
    z17 = floor_of(17, src, 0.0)
    print("floor (mean, max): n=17 %s, n=33 %s; radius 0 at n=17 %s" % (f17, f33, z17))
    assert f33[0] < f17[0] < z17[0] and 0.0 < f33[0] < 0.06


# ------------------------------------------------------------------ CPU: library and torch layers


def test_grid_travel_time_rejections_without_gpu():
    """Every rejection of include/pntf.h returns nonzero on the host; the fake pointers are
    never dereferenced."""
    L = _lib.load()
    fake, other = ctypes.c_void_p(64), ctypes.c_void_p(128)

    def init(speed=fake, n=9, src=fake, q=3, radius=4.0, T=fake):
        return L.pntf_grid_travel_time_init(speed, n, src, q, radius, T, None)

    def step(speed=fake, n=9, q=3, Tin=fake, Tout=other, inner=8, changed=fake):
        return L.pntf_grid_travel_time_pass(speed, n, q, Tin, Tout, inner, changed, None)

    bad_init = [(dict(n=1), b"n must be >= 2"), (dict(n=-5), b"n must be >= 2"),
                (dict(q=0), b"q must be >= 1"), (dict(radius=-1.0), b"radius"),
                (dict(radius=float("nan")), b"radius"), (dict(speed=None), b"null"),
                (dict(src=None), b"null"), (dict(T=None), b"null"),
                (dict(q=65536), b"launch limits"), (dict(n=1625), b"launch limits"),
                (dict(n=2 ** 31 - 1), b"launch limits")]
    for kw, text in bad_init:
        assert L.pntf_point_mesh_distance(None, 5, None, 3, None, 0, None) == 1   # other text
        assert init(**kw) == 1, kw
        err = L.pntf_mesh_last_error()
        assert b"pntf_grid_travel_time_init" in err and text in err, (kw, err)
    bad_pass = [(dict(n=1), b"n must be >= 2"), (dict(q=0), b"q must be >= 1"),
                (dict(inner=0), b"inner must be >= 1"), (dict(speed=None), b"null"),
                (dict(Tin=None), b"null"), (dict(Tout=None), b"null"),
                (dict(changed=None), b"null"), (dict(Tout=fake), b"distinct"),
                (dict(q=65536), b"launch limits"), (dict(n=1625), b"launch limits")]
    for kw, text in bad_pass:
        assert L.pntf_point_mesh_distance(None, 5, None, 3, None, 0, None) == 1
        assert step(**kw) == 1, kw
        err = L.pntf_mesh_last_error()
        assert b"pntf_grid_travel_time_pass" in err and text in err, (kw, err)
    with pytest.raises(_lib.PntfError, match="distinct"):
        _lib.check(step(Tout=fake), "pntf_grid_travel_time_pass")


def test_grid_ops_have_no_cpu_path():
    from pntf import ops
    with pytest.raises(_lib.PntfError):
        ops.grid_travel_time(torch.ones(9, 9, 9), torch.zeros(1, 3))
    with pytest.raises(_lib.PntfError):
        ops.speed_grid(torch.zeros(1, 3, 3), 9, 0.01, 0.1)
    with pytest.raises(_lib.PntfError):
        evaluate.field_report(None, None, torch.zeros(1, 3, 3), torch.zeros(1, 3))


# ------------------------------------------------------------------ GPU


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_solve(n, idx, radius, **kw):
    from pntf import ops
    S, src = scene(n)
    T, passes, conv = ops.grid_travel_time(dev(S), dev(src[list(idx)]), radius=radius, **kw)
    assert T.shape == (len(idx), n, n, n) and T.dtype == torch.float32
    assert passes.dtype == torch.int32 and conv.dtype == torch.bool
    return T, passes.cpu().numpy(), conv.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("inner", [1, 8])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n", SIZES)
def test_hip_grid_travel_time_matches_oracle(n, radius, inner):
    from pntf import ops
    T64, e32, sweeps = reference(n, radius)
    S, _ = scene(n)
    # inner = 1 is the plain Jacobi iteration: it needs as many passes as the oracle sweeps
    kw = dict(max_passes=2 * sweeps + 16) if inner == 1 else {}
    worst, seen = 0.0, {}
    for idx in BATCHES:
        T, passes, conv = gpu_solve(n, idx, radius, inner=inner, **kw)
        assert conv.all(), (passes, sweeps)
        again, changed = ops.grid_travel_time_pass(dev(S), T, inner)       # a fixed point
        assert not changed.any().item() and torch.equal(again.view(torch.int32),
                                                        T.view(torch.int32))
        Tn = T.cpu().numpy()
        for row, c in enumerate(idx):
            assert np.array_equal(np.isinf(Tn[row]), np.isinf(T64[c])), (n, radius, c)
            fin = np.isfinite(T64[c])
            worst = max(worst, float(np.abs(Tn[row][fin] - T64[c][fin]).max()))
            if c in seen:                      # the same source in another batch: the same bits
                assert seen[c] == Tn[row].tobytes()
            seen[c] = Tn[row].tobytes()
        if radius == 0.0 and SEALED in idx:    # nothing leaves the shell
            c, row = n // 2, idx.index(SEALED)
            assert np.isfinite(Tn[row]).sum() == 1 and np.isfinite(Tn[row][c, c, c])
    print("grid travel time vs fp64 oracle, n=%d radius=%g inner=%d: max abs error %.3g, "
          "e32 %.3g (ratio %.2f), T up to %.3g, %d oracle sweeps, passes %s"
          % (n, radius, inner, worst, e32, worst / e32, T64[np.isfinite(T64)].max(), sweeps,
             passes.tolist()))
    assert worst <= 4 * e32


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 33])
def test_hip_grid_travel_time_bits_are_reproducible(n):
    """The same bits from two runs, for check_every 1 and 4, and for a source alone or in a
    batch."""
    idx = BATCHES[1]
    base, _, conv = gpu_solve(n, idx, 4.0)
    assert conv.all()
    bits = lambda t: t.view(torch.int32)
    again, _, _ = gpu_solve(n, idx, 4.0)
    assert torch.equal(bits(again), bits(base))
    every, p1, conv = gpu_solve(n, idx, 4.0, check_every=1)
    assert conv.all() and torch.equal(bits(every), bits(base))
    for row, c in enumerate(idx):
        alone, _, conv = gpu_solve(n, (c,), 4.0)
        assert conv.all() and torch.equal(bits(alone[0]), bits(base[row]))


@pytest.mark.gpu
def test_hip_grid_travel_time_runs_out_of_passes_and_returns():
    T, passes, conv = gpu_solve(33, BATCHES[0], 4.0, max_passes=2)
    assert not conv.any() and (passes == 2).all()
    assert torch.isfinite(T).any() and torch.isinf(T).any()


@pytest.mark.gpu
def test_hip_grid_travel_time_rejects_a_non_finite_speed():
    from pntf import ops
    S, src = scene(9)
    bad = S.copy()
    bad[1, 2, 3] = np.nan
    with pytest.raises(_lib.PntfError, match="finite"):
        ops.grid_travel_time(dev(bad), dev(src[:1]))


BOX = (np.array([-0.2, -0.1, -0.15]), np.array([0.25, 0.2, 0.1]))
MESH_TOL = 2e-6          # the point kernel's bound (tests/test_mesh.py)


@pytest.mark.gpu
def test_speed_grid_matches_the_mesh_oracle():
    from pntf import ops
    n, offset, margin = 9, 0.01, 0.1
    tris = M.box_mesh(*BOX).astype(np.float32)
    S = ops.speed_grid(dev(tris), n, offset, margin)
    assert S.shape == (n, n, n) and S.dtype == torch.float32
    nodes = E.nodes(n).reshape(-1, 3).astype(np.float32)
    want = M.speed_from_distance(M.point_mesh_distance(nodes, tris), offset, margin)
    got = S.cpu().numpy().reshape(-1)
    assert np.abs(got - want).max() <= MESH_TOL / margin + 1e-6
    assert got.min() == np.float32(np.float32(offset) / np.float32(margin)) and got.max() == 1.0
    assert np.array_equal(ops.grid_nodes(n, torch.device("cuda:0")).cpu().numpy(), nodes)


@pytest.mark.gpu
def test_field_report_recomputed_from_the_models_outputs():
    from models import model_res_sigmoid as ma
    from models import model_res_sigmoid_multi as md
    d0 = torch.device("cuda:0")
    m = md.Model(".", ".", 3, 2, device="cuda:0")
    m.network = md.NN("cuda:0", 3)
    m.network.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0).items()},
                              strict=True)
    m.network.to(d0).float().eval()
    m.B = torch.from_numpy(synth.make_B(3)).to(d0)
    n, margin, offset, radius = 17, 0.1, 0.01, 4.0
    tris = M.box_mesh(*BOX).astype(np.float32)
    src = np.array([[0.3237, -0.2213, 0.1771], [-0.41, 0.33, -0.07]], np.float32)
    rep = m.FieldReport(torch.from_numpy(tris), torch.from_numpy(src), n=n, offset=offset,
                        margin=margin, radius=radius)
    assert rep.converged.all().item() and rep.T_grid.shape == (2, n, n, n)
    S = rep.speed.cpu().numpy()
    T64, _ = E.solve(S, src, radius)                         # the oracle's T on the same speed
    U64, _ = E.solve(uniform(n), src, radius)
    # The report's grid solves are the kernel's: within 4 e32 of the oracle's (the parity bound),
    # e32 taken on these two solves.  An error delta in T moves |x - T| / T by at most
    # delta / T (1 + |x - T| / T), which is the tolerance on the rows below.
    e32 = lambda A, B: 4 * float(np.abs(B.astype(np.float64) - A)[np.isfinite(A)].max())
    dT = e32(T64, E.solve(S, src, radius, np.float32)[0])
    dU = e32(U64, E.solve(uniform(n), src, radius, np.float32)[0])
    nodes = E.nodes(n).reshape(-1, 3)
    nodes32 = torch.from_numpy(nodes.astype(np.float32)).to(d0)
    for c in range(2):
        xp = torch.cat([torch.from_numpy(src[c]).to(d0).expand(n ** 3, 3), nodes32], 1)
        with torch.no_grad():
            tm = m.TravelTimes(xp).reshape(-1).cpu().numpy().astype(np.float64)
            sm = m.Speed(xp).reshape(-1).cpu().numpy().astype(np.float64)
        tg = T64[c].reshape(-1)
        mask = ~E.ball(n, src[c], radius)[0].reshape(-1) & np.isfinite(tg)
        assert mask.sum() > n ** 3 // 2
        et = np.abs(tm - tg)[mask] / tg[mask]
        es = np.abs(sm - S.reshape(-1))
        dist = np.linalg.norm(nodes - src[c].astype(np.float64), axis=1)
        ef = np.abs(U64[c].reshape(-1) - dist)[mask] / dist[mask]
        got = {k: float(getattr(rep, k)[c]) for k in
               ("tt_mean_rel", "tt_max_rel", "speed_mean_abs", "speed_max_abs", "floor_mean_rel",
                "floor_max_rel")}
        print("field report source %d: %s" % (c, got))
        tT, tU = dT / tg[mask].min(), dU / dist[mask].min()   # + 1e-6: fp32 node coordinates
        assert abs(got["tt_mean_rel"] - et.mean()) <= tT * (1 + et.mean()) + 1e-9
        assert abs(got["tt_max_rel"] - et.max()) <= tT * (1 + et.max()) + 1e-9
        np.testing.assert_allclose(got["speed_mean_abs"], es.mean(), rtol=1e-6)
        np.testing.assert_allclose(got["speed_max_abs"], es.max(), rtol=1e-6)
        assert abs(got["floor_mean_rel"] - ef.mean()) <= tU * (1 + ef.mean()) + 1e-6
        assert abs(got["floor_max_rel"] - ef.max()) <= tU * (1 + ef.max()) + 1e-6
        assert 0.0 < got["floor_mean_rel"] < 0.1
    arm = ma.Model(".", ".", 6, device="cuda:0")
    with pytest.raises(_lib.PntfError, match="arm"):
        arm.FieldReport(torch.from_numpy(tris), torch.from_numpy(src))
    m6 = md.Model(".", ".", 6, 2, device="cuda:0")
    with pytest.raises(_lib.PntfError, match="dim must be 3"):
        m6.FieldReport(torch.from_numpy(tris), torch.from_numpy(src))
