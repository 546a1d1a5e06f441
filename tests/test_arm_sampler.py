"""Arm speed-sample generator: the fused FK + mesh-distance kernel (pntf_arm_mesh_distance),
pntf.kin.SerialChain and the arm functions of dataprocessing/speed_sampling_gpu.py
(reference :153-323).

Pinning: pytorch_kinematics and bvh_distance_queries are absent and the reference holds no
URDF, link mesh or vector for this path, so parity is pinned by the URDF convention and by
geometry: the fp64 oracle (tests/arm_oracle.py: Rodrigues' formula on points, tip to root)
is checked against closed forms here, and distances come from oracle/mesh_oracle.py.

GPU tolerance: 3e-6 absolute on the distance = the point kernel's 2e-6 (tests/test_mesh.py)
+ 1e-6 for posing in fp32 (distance is 1-Lipschitz in the point; an fp32 restatement of a
6-joint chain moved a vertex by at most 1.4e-7 against fp64 over 20 chains x 20 000
configurations, and 1e-6 is 7x that).
"""
import functools

import numpy as np
import pytest
import torch

import arm_oracle as A
from oracle import mesh_oracle as M
from pntf import _lib, kin

TOL = 3e-6
SAMPLER_BOX = (np.array([0.15, -0.2, -0.2]), np.array([0.45, 0.2, 0.2]))   # sampler obstacle


def chain_of(spec, names=None):
    return kin.SerialChain.from_arrays(A.origin_matrices(spec), [s[2] for s in spec],
                                       [s[3] for s in spec], names)


# ------------------------------------------------------------------ CPU: oracle pinning


def test_oracle_planar_2r_closed_form():
    l1, l2 = 0.23, 0.17
    spec = [A.ROOT, ((0, 0, 0), (0, 0, 0), A.REVOLUTE, (0, 0, 1)),
            ((l1, 0, 0), (0, 0, 0), A.REVOLUTE, (0, 0, 3.0))]
    th = np.random.default_rng(0).uniform(-np.pi, np.pi, (500, 2))
    tip = A.pose_points(spec, th, 2, np.array([[l2, 0.0, 0.0]]))[:, 0]
    want = np.stack([l1 * np.cos(th[:, 0]) + l2 * np.cos(th[:, 0] + th[:, 1]),
                     l1 * np.sin(th[:, 0]) + l2 * np.sin(th[:, 0] + th[:, 1]),
                     np.zeros(500)], axis=1)
    np.testing.assert_allclose(tip, want, atol=1e-12)


def test_oracle_prismatic_along_tilted_axis():
    axis = np.array([1.0, 2.0, -2.0])                       # |axis| = 3
    spec = [A.ROOT, ((0.1, -0.05, 0.02), (0, 0, 0), A.PRISMATIC, tuple(axis))]
    q = np.linspace(-0.3, 0.3, 31)[:, None]
    p = A.pose_points(spec, q, 1, np.array([[0.01, 0.02, 0.03]]))[:, 0]
    want = np.array([0.11, -0.03, 0.05]) + q * axis / 3.0
    np.testing.assert_allclose(p, want, atol=1e-12)


def test_oracle_rpy_known_answers():
    none = np.zeros((1, 0))
    roll = [A.ROOT, ((0, 0, 0), (np.pi / 2, 0, 0), A.FIXED, (1, 0, 0))]
    np.testing.assert_allclose(A.pose_points(roll, none, 1, np.array([[0.0, 1, 0]]))[0, 0],
                               [0, 0, 1], atol=1e-12)          # roll pi/2: y^ -> z^
    r, p, y = 0.3, -0.7, 1.1
    spec = [A.ROOT, ((0.01, 0.02, 0.03), (r, p, y), A.FIXED, (1, 0, 0))]
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    v = np.random.default_rng(1).normal(size=(50, 3))
    np.testing.assert_allclose(A.pose_points(spec, none, 1, v)[0],
                               v @ (Rz @ Ry @ Rx).T + [0.01, 0.02, 0.03], atol=1e-12)
    np.testing.assert_allclose(kin.rpy_matrix((r, p, y)), Rz @ Ry @ Rx, atol=1e-15)
    np.testing.assert_allclose(A.frame_matrices(spec, none)[0, 1],
                               A.origin_matrices(spec)[1], atol=1e-12)


# ------------------------------------------------------------------ CPU: SerialChain


def assert_same_chain(a, b):
    assert a.link_names == b.link_names and a.dof == b.dof
    np.testing.assert_array_equal(a.types, b.types)
    np.testing.assert_array_equal(a.cols, b.cols)
    np.testing.assert_allclose(a.origins, b.origins, atol=1e-7)
    np.testing.assert_allclose(a.axes, b.axes, atol=1e-7)
    for t in (a.origins, a.axes):
        assert t.dtype == np.float32 and t.flags.c_contiguous
    for t in (a.types, a.cols):
        assert t.dtype == np.int32 and t.flags.c_contiguous


def test_from_urdf_equals_from_arrays():
    c = kin.SerialChain.from_urdf(A.URDF7, "tool")
    assert c.link_names == A.URDF7_LINKS and c.dof == 4          # the side branch is ignored
    assert list(c.types) == [kin.FIXED, kin.REVOLUTE, kin.REVOLUTE, kin.FIXED, kin.PRISMATIC,
                             kin.REVOLUTE, kin.FIXED]
    assert list(c.cols) == [0, 0, 1, 0, 2, 3, 0]
    assert_same_chain(c, chain_of(A.URDF7_SPEC, A.URDF7_LINKS))
    np.testing.assert_allclose(np.linalg.norm(c.axes, axis=1), 1.0, atol=1e-6)
    # truncation at an inner link; the side branch is a chain of its own
    assert_same_chain(kin.SerialChain.from_urdf(A.URDF7, "l3"),
                      chain_of(A.URDF7_SPEC[:4], A.URDF7_LINKS[:4]))
    cam = kin.SerialChain.from_urdf(A.URDF7, "camera")
    assert cam.link_names == ["base", "l1", "l2", "camera"] and cam.dof == 3
    assert kin.SerialChain.from_urdf(A.URDF7, "base").link_names == ["base"]


@pytest.mark.parametrize("text,end", [
    (A.URDF7, "gripper"),                                              # absent
    (A.URDF7.replace("</robot>", '<link name="island"/></robot>'), "island"),   # unreachable
    (A.URDF7.replace('type="continuous"', 'type="floating"'), "tool"),
    (A.URDF7.replace('type="prismatic"', 'type="planar"'), "tool"),
    ("<robot><link", "tool"),
])
def test_from_urdf_errors(text, end):
    with pytest.raises(_lib.PntfError):
        kin.SerialChain.from_urdf(text, end)


def test_from_urdf_ignores_unsupported_joints_off_the_chain():
    text = A.URDF7.replace('name="j_cam" type="revolute"', 'name="j_cam" type="floating"')
    assert kin.SerialChain.from_urdf(text, "tool").dof == 4


@pytest.mark.parametrize("which", ["urdf7", "random6"])
def test_forward_kinematics_cpu_matches_oracle(which):
    rng = np.random.default_rng(3)
    spec = A.URDF7_SPEC if which == "urdf7" else A.random_chain(rng, 6)
    chain = kin.SerialChain.from_urdf(A.URDF7, "tool") if which == "urdf7" else chain_of(spec)
    th = A.random_theta(rng, spec, 300)
    got = chain.forward_kinematics(torch.from_numpy(th).float())
    assert got.shape == (300, len(spec), 3, 4) and got.dtype == torch.float32
    assert np.abs(got.numpy() - A.frame_matrices(spec, th.astype(np.float32))).max() < 1e-6
    with pytest.raises(_lib.PntfError):
        chain.forward_kinematics(torch.zeros(4, chain.dof + 1))


def test_arm_symbol_and_validation_without_gpu():
    import ctypes
    L = _lib.load()
    chain = chain_of(A.URDF7_SPEC)
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(64)               # never dereferenced: validation comes first
    voff = np.arange(8, dtype=np.int32)
    tables = [host(chain.origins), host(chain.types), host(chain.axes), host(chain.cols)]
    inf = float("inf")

    def call(theta=fake, n=5, dof=4, frames=7, tabs=tables, verts=fake, vo=voff, tris=fake,
             t=3, cap=inf, dist=fake):
        return L.pntf_arm_mesh_distance(theta, n, dof, frames, *tabs, verts, host(vo), tris, t,
                                        cap, dist, None)

    bad = [dict(n=-1), dict(theta=None), dict(dist=None), dict(tris=None), dict(verts=None),
           dict(tabs=[None] + tables[1:]), dict(tabs=tables[:3] + [None]),
           dict(frames=17), dict(frames=0), dict(dof=17),
           dict(dof=3),                                   # frame 5 reads column 3
           dict(t=0), dict(t=-1), dict(cap=-1.0), dict(cap=float("nan")),
           dict(vo=voff[::-1].copy())]
    for kw in bad:
        assert L.pntf_point_mesh_distance(None, 5, None, 3, None, 0, None) == 1   # other text
        assert call(**kw) == 1, kw
        assert b"pntf_arm_mesh_distance" in L.pntf_mesh_last_error(), kw
    assert call(dof=3) == 1 and b"column" in L.pntf_mesh_last_error()
    assert call(t=0) == 1 and b"empty mesh" in L.pntf_mesh_last_error()
    # an empty batch is a no-op whatever the pointers are
    assert L.pntf_arm_mesh_distance(None, 0, 0, 0, None, None, None, None, None, None, None, 0,
                                    inf, None, None) == 0
    with pytest.raises(_lib.PntfError, match="column"):
        _lib.check(call(dof=3), "pntf_arm_mesh_distance")


def test_arm_mesh_distance_has_no_cpu_path():
    from pntf import ops
    chain = chain_of(A.URDF7_SPEC)
    with pytest.raises(_lib.PntfError):
        ops.arm_mesh_distance(torch.zeros(4, 4), chain, [torch.zeros(1, 3)] * 7,
                              torch.zeros(1, 3, 3))


# ------------------------------------------------------------------ GPU

# (n, vertices per frame or "urdf7", triangles, triangle scale): a single point and triangle;
# an empty frame, a chunk boundary inside a frame (1025 = 1024 + 1) and ragged chunks; two
# triangle tiles with a ragged second one and six frames of 37 vertices behind an empty root;
# mixed joint types from the URDF; "cap": rows on both sides of 0.05.  The larger meshes use
# small triangles (random_mesh's `scale` 0.02): with its default 0.2 every configuration
# touches a triangle and all distances are ~1e-4.
CASES = {"one": (1, [1], 1, 0.2), "chunks": (3, [0, 1, 255, 1025], 7, 0.2),
         "tiles": (130, [0] + [37] * 6, 257, 0.02), "urdf7": (64, "urdf7", 300, 0.02),
         "cap": (130, [0, 0, 37, 37], 30, 0.02)}
SEEDS = {"one": 42, "chunks": 40, "tiles": 5, "urdf7": 43, "cap": 21}
PARITY = ["one", "chunks", "tiles", "urdf7"]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(spec, chain, theta, link vertices, triangles, oracle distances), computed once."""
    n, layout, t, scale = CASES[name]
    rng = np.random.default_rng(SEEDS[name])
    if layout == "urdf7":
        spec, chain = A.URDF7_SPEC, kin.SerialChain.from_urdf(A.URDF7, "tool")
        layout = [0, 20, 20, 20, 20, 20, 20]
    else:
        spec = A.random_chain(rng, len(layout) - 1)
        chain = chain_of(spec)
    th = A.random_theta(rng, spec, n).astype(np.float32)
    verts = [A.link_blob(rng, v).astype(np.float32) for v in layout]
    tris = A.boxed_mesh(rng, t, scale).astype(np.float32)
    assert np.abs(A.posed_cloud(spec, th, verts)).max() <= 0.5 and np.abs(tris).max() <= 0.5
    return spec, chain, th, verts, tris, A.arm_mesh_distance(spec, th, verts, tris)


def on_gpu(th, verts, tris):
    return (torch.from_numpy(th).cuda(), [torch.from_numpy(v).cuda() for v in verts],
            torch.from_numpy(tris).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_hip_arm_distance_matches_oracle(name):
    from pntf import ops
    spec, chain, th, verts, tris, ref = scene(name)
    T, V, R = on_gpu(th, verts, tris)
    d = ops.arm_mesh_distance(T, chain, V, R)
    assert d.shape == (len(th),) and d.dtype == torch.float32
    err = np.abs(d.cpu().numpy() - ref).max()
    print("arm distance vs oracle, %s: max abs error %.3g" % (name, err))
    assert err < TOL


@pytest.mark.gpu
def test_hip_arm_distance_link_dict_and_empty_batch():
    from pntf import ops
    spec, chain, th, verts, tris, ref = scene("urdf7")
    T, V, R = on_gpu(th, verts, tris)
    by_name = {n: v for n, v in zip(chain.link_names, V) if v.shape[0]}
    assert torch.equal(ops.arm_mesh_distance(T, chain, by_name, R[None]),
                       ops.arm_mesh_distance(T, chain, V, R))
    assert ops.arm_mesh_distance(T[:0], chain, V, R).shape == (0,)
    with pytest.raises(_lib.PntfError):
        ops.arm_mesh_distance(T, chain, {"elbow": V[1]}, R)


@pytest.mark.gpu
def test_hip_arm_distance_bits_independent_of_batch_and_chunking():
    """Row c alone = row c inside the batch of 130, and the vertices of each frame in another
    order (other chunks, other lanes) give the same bits: the minimum is order-independent and
    the culling exact."""
    from pntf import ops
    rng = np.random.default_rng(11)
    spec = A.random_chain(rng, 3)
    chain = chain_of(spec)
    th = A.random_theta(rng, spec, 130).astype(np.float32)
    verts = [A.link_blob(rng, v).astype(np.float32) for v in (0, 1, 255, 1025)]
    T, V, R = on_gpu(th, verts, A.boxed_mesh(rng, 257).astype(np.float32))
    full = ops.arm_mesh_distance(T, chain, V, R)
    for c in (0, 57, 129):
        assert torch.equal(ops.arm_mesh_distance(T[c:c + 1], chain, V, R), full[c:c + 1])
    assert torch.equal(ops.arm_mesh_distance(T[40:90], chain, V, R), full[40:90])
    P = [v[torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(f)).cuda()]
         for f, v in enumerate(V)]
    assert torch.equal(ops.arm_mesh_distance(T, chain, P, R), full)


@pytest.mark.gpu
def test_hip_arm_distance_cap_is_bitwise_minimum():
    """cap = 0.05 gives minimum(exact, 0.05) bit for bit.  Of the 130 oracle distances of this
    scene 77 lie below 0.05 and 53 above, none within 1e-5 of it (measured on the CPU when the
    seed was chosen)."""
    from pntf import ops
    spec, chain, th, verts, tris, ref = scene("cap")
    assert (ref < 0.05 - TOL).sum() == 77 and (ref > 0.05 + TOL).sum() == 53
    T, V, R = on_gpu(th, verts, tris)
    exact = ops.arm_mesh_distance(T, chain, V, R)
    capped = ops.arm_mesh_distance(T, chain, V, R, cap=0.05)
    assert (exact < 0.05).any() and (exact > 0.05).any()
    assert torch.equal(capped, torch.minimum(exact, torch.tensor(0.05, device="cuda")))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chunks", "urdf7"])
def test_hip_arm_distance_agrees_with_unfused_route(name):
    """torch posing + the point kernel + amin: another rounding path, so 3e-6, not bits."""
    from pntf import ops
    spec, chain, th, verts, tris, ref = scene(name)
    T, V, R = on_gpu(th, verts, tris)
    fk = chain.forward_kinematics(T)
    cloud = torch.cat([torch.einsum("nij,vj->nvi", fk[:, f, :, :3], v) + fk[:, f, None, :, 3]
                       for f, v in enumerate(V) if v.shape[0]], dim=1)
    unfused = ops.point_mesh_distance(cloud.reshape(-1, 3), R).reshape(len(th), -1).amin(dim=1)
    fused = ops.arm_mesh_distance(T, chain, V, R)
    assert (fused - unfused).abs().max().item() < TOL
    assert np.abs(unfused.cpu().numpy() - ref).max() < TOL


@pytest.mark.gpu
def test_hip_arm_distance_analytic_circle_next_to_box():
    """One vertex on a circle of radius 0.3 about z, next to (and through) a box."""
    from pntf import ops
    spec = [A.ROOT, ((0, 0, 0), (0, 0, 0), A.REVOLUTE, (0, 0, 1)),
            ((0.3, 0, 0), (0, 0, 0), A.FIXED, (1, 0, 0))]
    lo, hi = np.array([0.2, -0.1, -0.1]), np.array([0.45, 0.15, 0.1])
    th = np.linspace(-np.pi, np.pi, 721).astype(np.float32)[:, None]
    verts = [np.zeros((0, 3), np.float32)] * 2 + [np.zeros((1, 3), np.float32)]
    T, V, R = on_gpu(th, verts, M.box_mesh(lo, hi).astype(np.float32))
    d = ops.arm_mesh_distance(T, chain_of(spec), V, R).cpu().numpy()
    q = th[:, 0].astype(np.float64)
    p = np.stack([0.3 * np.cos(q), 0.3 * np.sin(q), 0 * q], axis=1)
    want = M.box_distance(p, lo, hi)
    assert want.min() < 1e-3 and want.max() > 0.3         # touches the box, and far from it
    assert np.abs(d - want).max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("dim,numsamples", [(3, 500), (6, 200)])
def test_arm_sampler_properties(tmp_path, dim, numsamples):
    """arm_rand_sample_bound_points on a dim-R arm (reach 0.4, 20 vertices per link) beside a
    box: shapes, dtypes, box membership, offset <= d(x0) <= margin and both speed columns,
    every returned pair recomputed by the oracle.  With this box, offset 0.005 and margin 0.1
    the oracle accepts 27.5 % (dim 3) and 50.1 % (dim 6) of 5000 uniform configurations
    (measured on the CPU, test_sampler_scene_acceptance_share), so the loop ends in a few
    rounds."""
    from dataprocessing import speed_sampling_gpu as S
    torch.manual_seed(dim)
    spec, link_verts = A.write_arm(str(tmp_path), dim, np.random.default_rng(dim))
    tris = M.box_mesh(SAMPLER_BOX[0], SAMPLER_BOX[1])
    v = tris.reshape(-1, 3)
    f = np.arange(len(v)).reshape(-1, 3)
    offset, margin = 0.005, 0.1
    X, speed = S.arm_rand_sample_bound_points(numsamples, dim, v, f, offset, margin,
                                              str(tmp_path), "arm", "link%d" % dim)
    assert X.shape == (numsamples, 2 * dim) and X.dtype == np.float32
    assert speed.shape == (numsamples, 2) and speed.dtype == np.float64
    assert np.all(np.abs(X) <= 0.5)
    d0 = A.arm_mesh_distance(spec, 2 * np.pi * X[:, :dim], link_verts, tris)
    d1 = A.arm_mesh_distance(spec, 2 * np.pi * X[:, dim:], link_verts, tris)
    assert np.all((d0 >= offset - TOL) & (d0 <= margin + TOL))
    np.testing.assert_allclose(speed[:, 0], M.speed_from_distance(d0, offset, margin),
                               atol=TOL / margin)
    np.testing.assert_allclose(speed[:, 1], M.speed_from_distance(d1, offset, margin),
                               atol=TOL / margin)
    chain = kin.SerialChain.from_urdf(open(str(tmp_path / "arm.urdf")).read(), "link%d" % dim)
    d = S.arm_obstacle_distance(torch.from_numpy(2 * np.pi * X[:5, :dim]).float().cuda(), chain,
                                str(tmp_path), torch.from_numpy(tris).float().cuda()[None])
    np.testing.assert_allclose(d.cpu().numpy(), d0[:5], atol=TOL)


def test_sampler_scene_acceptance_share():
    """The share of uniform configurations the oracle accepts in the sampler test's scene
    (>= 5 %, so its rejection loop is short), and the arm stays inside the box."""
    for dim in (3, 6):
        rng = np.random.default_rng(dim)
        text, spec, names = A.revolute_arm_urdf(dim)
        link_verts = [np.zeros((0, 3))] * 2 + [A.link_blob(rng, 20) for _ in range(dim)]
        th = 2 * np.pi * np.random.default_rng(99).uniform(-0.5, 0.5, (5000, dim))
        assert np.abs(A.posed_cloud(spec, th, link_verts)).max() <= 0.5
        d = A.arm_mesh_distance(spec, th, link_verts, M.box_mesh(*SAMPLER_BOX))
        share = np.mean((d >= 0.005) & (d <= 0.1))
        print("dim %d: oracle accepts %.1f %%" % (dim, 100 * share))
        assert share >= 0.05
