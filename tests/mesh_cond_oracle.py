"""Ill-conditioned triangles for the mesh-distance kernels — TEST INFRASTRUCTURE ONLY.

Generators of thin, tiny and degenerate float32 triangles with query points aimed at the places
where the kernels' per-triangle record (csrc/pntf_mesh_geom.h, build_record) can go wrong, an
exact plane distance to pin the fp64 oracle on them, and a numpy restatement of build_record
and tri_d2 in the header's precision, which shows on the CPU that the inputs have teeth: with
the unit normal taken from an fp32 cross product the face-region queries of a sliver miss the
point kernel's tolerance, with the normal taken in fp64 from the same fp32 vertices they hold
it.  The pattern of tests/gemm_oracle.py: the targeted inputs are proven to matter.

Why the face region: above the interior of a triangle the kernel returns min(h^2, e), h = q.n^.
For a triangle of aspect s (the sine of its smallest angle at `a`) the fp32 cross product
n = ab x ac cancels to |ab||ac|s, so the direction of n^ is off by about eps32 / s and h by
about |q| eps32 / s; a too small h wins the min.  Uniformly drawn query points almost never
have their foot inside a sliver, so random meshes and random points do not see this.

Everything is float32 with coordinates inside [-0.5, 0.5], the range the project's distance
tolerances are stated for.  Only `tests/` may import this module.
"""
import numpy as np

from oracle import mesh_oracle as M

ASPECTS = (1e-2, 1e-3, 1e-4, 1e-5, 3e-6)
TINY_EDGES = (1e-3, 1e-5, 1e-7)
FLAT_SIN2 = 1e-12                      # the record's and the oracle's rule, at vertex a
MARGIN = 0.05                          # face region: foot barycentrics at least this

FACE, ON, VERTEX, EDGE, EDGE_OUT, VORONOI, OTHER = range(7)
KIND_NAMES = ("face", "on", "vertex", "edge", "edge_out", "voronoi", "other")

f32, f64, ld = np.float32, np.float64, np.longdouble


# ------------------------------------------------------------------ exact-enough geometry

def _dot(x, y):
    return (x * y).sum(-1)


def _edges(tri, dtype=ld):
    t = np.asarray(tri, f32).astype(dtype)           # exact: the float32 vertices
    return t[..., 0, :], t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 0, :]


def sin2_at_a(tri):
    """sin^2 of the angle at vertex a of the float32 triangle(s), in long double."""
    _, ab, ac = _edges(tri)
    n = np.cross(ab, ac)
    den = _dot(ab, ab) * _dot(ac, ac)
    return np.where(den > 0, _dot(n, n) / np.where(den > 0, den, 1), 0).astype(f64)


def plane_distance(p, tri):
    """|(p - a).n^| with n^ from long double on the float32 vertices: the distance of every
    point whose foot lies in the triangle.  The cross product cancels to a relative 1e-19 / s,
    so this is good to ~1e-14 at the thinnest aspect used here."""
    a, ab, ac = _edges(tri)
    n = np.cross(ab, ac)
    q = np.asarray(p, f32).astype(ld) - a
    return (np.abs(_dot(q, n)) / np.sqrt(_dot(n, n))).astype(f64)


def barycentrics(p, tri):
    """(u, v, w) of the foot of p in the plane of the triangle, long double; p need not lie in
    the plane (its offset along n drops out of both triple products)."""
    a, ab, ac = _edges(tri)
    n = np.cross(ab, ac)
    x = np.asarray(p, f32).astype(ld) - a
    nn = _dot(n, n)
    v = _dot(np.cross(x, ac), n) / nn
    w = _dot(np.cross(ab, x), n) / nn
    return np.stack([1 - v - w, v, w], -1).astype(f64)


# ------------------------------------------------------------------ triangles

def frame(rng, tilt=None):
    """Orthonormal (u, w, n): uniformly random, or with n within `tilt` radians of +z."""
    if tilt is None:
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        return q[:, 0], q[:, 1], q[:, 2]
    ang, az = rng.uniform(0, tilt), rng.uniform(0, 2 * np.pi)
    n = np.array([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)])
    u = np.cross(n, rng.normal(size=3))
    u /= np.linalg.norm(u)
    return u, np.cross(n, u), n


def sliver(family, s, vertex, centre, size, fr):
    """One thin triangle, float32 (3, 3).  `needle`: angle asin(s) at the special vertex between
    two edges of length `size` (the other two angles are near pi/2).  `cap`: angle pi - asin(s)
    at the special vertex (the other two are about s/2).  The special vertex is vertex number
    `vertex` (0 = a, 1 = b, 2 = c; the orientation is kept): the record's `flat` test and its
    normal look at the angle at a only."""
    u, w, _ = fr
    phi = np.arcsin(s)
    if family == "needle":
        V = centre - 0.5 * size * u
        P = V + size * u
        Q = V + size * (np.cos(phi) * u + np.sin(phi) * w)
    else:
        V = centre + 0.05 * size * u
        P = V + 0.5 * size * u
        Q = V + 0.45 * size * (-np.cos(phi) * u + np.sin(phi) * w)
    return np.roll(np.stack([V, P, Q]), vertex, axis=0).astype(f32)


def tiny(edge, centre, fr):
    """A well-shaped triangle of edge length `edge` (1e-7 is three float32 steps at 0.45: the
    rounded triangle is whatever the grid leaves of it)."""
    u, w, _ = fr
    return np.stack([centre, centre + edge * u, centre + edge * (0.5 * u + 0.8 * w)]).astype(f32)


DEGENERATE = ("a==b", "a==c", "b==c", "a==b==c", "collinear_a_mid", "collinear_b_mid",
              "collinear_c_mid")


def degenerate(which, centre):
    """Exactly degenerate float32 triangles: the vertices are dyadic, so the collinear ones have
    an exactly zero cross product in any precision."""
    a = np.round(np.asarray(centre) * 1024) / 1024
    d = np.array([2.0 ** -5, -2.0 ** -6, 2.0 ** -7])
    e = np.array([2.0 ** -6, 2.0 ** -5, -2.0 ** -6])
    tri = {"a==b": [a, a, a + e], "a==c": [a, a + d, a], "b==c": [a, a + d, a + d],
           "a==b==c": [a, a, a],
           "collinear_a_mid": [a, a - d, a + d], "collinear_b_mid": [a - d, a, a + d],
           "collinear_c_mid": [a - d, a + d, a]}[which]
    return np.stack(tri).astype(f32)


def threshold_pair(rng, centres, size, fr, family="needle"):
    """Two triangles of the same frame and size on the two sides of sin^2 = 1e-12 at a, the
    first flat by the rule and the second not, both by at least 10 % (measured on the float32
    vertices: at this aspect the float32 grid moves sin^2 by more than that, hence the
    search).  Small coordinates keep the grid fine.  centres: one per triangle."""
    out = []
    for centre, (lo, hi) in zip(centres, ((0.2e-12, 0.9e-12), (1.1e-12, 4e-12))):
        for _ in range(2000):
            s = np.sqrt(rng.uniform(lo, hi))
            tri = sliver(family, s, 0, centre + rng.uniform(-1e-3, 1e-3, 3), size, fr)
            if lo < sin2_at_a(tri) < hi:
                break
        else:
            raise AssertionError("no float32 triangle found with sin^2 in (%g, %g)" % (lo, hi))
        out.append(tri)
    return out


# ------------------------------------------------------------------ query points

def queries(tri, rng, n_face=8, hmax=0.3, box=0.5, n_out=1):
    """Query points for one float32 triangle -> (pts (m, 3) float32, kind (m,)):
    FACE      n_face points above / below the face, foot barycentrics >= MARGIN AFTER the point
              was rounded to float32, heights log-uniform in [1e-4, hmax] on both sides;
    ON        one point of the face (rounded to float32, so within ~1e-8 of it);
    VERTEX    the three vertices (distance exactly 0);
    EDGE      a point of each edge;
    EDGE_OUT  n_out points of each edge's line beyond each of its ends, by 1e-4 .. 0.3 of the
              edge (log-uniform): in the plane, past the tip where two edges meet — the three
              half-plane tests of tri_d2 all sit within rounding of 0 there;
    VORONOI   from each vertex, straight out across an edge that ends there (the boundary of
              the vertex's and the edge's regions), lifted off the plane;
    OTHER     for a triangle without a normal: the points of its edges and a cloud around it.
    A FACE draw whose rounded foot leaves the margin is redrawn; every point lies in the box."""
    t = np.asarray(tri, f32).astype(f64)
    a, b, c = t
    n = np.cross(b - a, c - a)
    pts, kind = [], []

    def add(p, k):
        p = np.asarray(p, f64).astype(f32)
        if np.abs(p).max() <= box:
            pts.append(p)
            kind.append(k)
            return True
        return False

    for v in t:
        add(v, VERTEX)
    if not _dot(n, n) > 0 or sin2_at_a(tri) <= 1e-13:
        for i, j in ((0, 1), (0, 2), (1, 2)):
            add(t[i] + rng.uniform(0.2, 0.8) * (t[j] - t[i]), OTHER)
        for _ in range(n_face):
            add(t[rng.integers(3)] + rng.uniform(-0.04, 0.04, 3), OTHER)
        return np.stack(pts), np.array(kind)
    n /= np.linalg.norm(n)
    height = lambda: rng.choice([-1.0, 1.0]) * np.exp(rng.uniform(np.log(1e-4), np.log(hmax)))
    got = tries = 0
    while got < n_face and tries < 400 * n_face:
        tries += 1
        w = MARGIN + (1 - 3 * MARGIN) * rng.dirichlet([1, 1, 1])
        # spread the margin: w_i in [MARGIN, 1 - 2 MARGIN], sum 1
        p = (w @ t + height() * n).astype(f32)
        if np.abs(p).max() <= box and barycentrics(p, tri).min() >= MARGIN:
            got += add(p, FACE)
    w = MARGIN + (1 - 3 * MARGIN) * rng.dirichlet([1, 1, 1])
    add(w @ t, ON)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        add(t[i] + rng.uniform(0.2, 0.8) * (t[j] - t[i]), EDGE)
    for i in range(3):                              # beyond both ends of every edge
        for j in range(3):
            for _ in range(n_out if i != j else 0):
                beyond = np.exp(rng.uniform(np.log(1e-4), np.log(0.3)))
                add(t[i] + (1 + beyond) * (t[j] - t[i]), EDGE_OUT)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        e = t[j] - t[i]
        out = np.cross(e, n)                        # in-plane, away from the third vertex
        out *= -np.sign(out @ (t[k] - t[i])) / np.linalg.norm(out)
        add(t[i] + rng.uniform(1e-3, 0.03) * out + height() * n, VORONOI)
    return np.stack(pts), np.array(kind)


# ------------------------------------------------------------------ scenes

def family_cases(seed=0, reps=6, n_face=16, n_out=4):
    """`reps` triangles per (family, special vertex, aspect), freely oriented, long edge
    0.1-0.3 about the origin, each with its queries (heights up to 0.3):
    [(family, vertex, aspect, tri, pts, kind)], 30·reps cases.  Several orientations per
    combination: how far an fp32 normal is off depends on how the products happen to round."""
    rng = np.random.default_rng(seed)
    out = []
    for family in ("needle", "cap"):
        for vertex in range(3):
            for s in ASPECTS:
                for _ in range(reps):
                    tri = sliver(family, s, vertex, rng.uniform(-0.05, 0.05, 3),
                                 rng.uniform(0.1, 0.3), frame(rng))
                    pts, kind = queries(tri, rng, n_face=n_face, hmax=0.3, n_out=n_out)
                    out.append((family, vertex, s, tri, pts, kind))
    return out


def lattice_scene(seed=1, n_face=20, hmax=0.14):
    """One mesh with a triangle per cell of a 0.1 lattice (10 x 10 in x, y; layers z = -0.3, 0,
    0.3): 294 triangles, the queries of each (about 10000 points).  Slivers lie within 0.2 rad of
    their layer, span at most 0.08 and their queries rise at most `hmax` < half the layer
    spacing, so a query's nearest triangle is, nearly always, its own.
    -> dict(tris, label (T,) str, aspect (T,), pts, kind, owner)."""
    rng = np.random.default_rng(seed)
    g = -0.45 + 0.1 * np.arange(10)
    cells = [np.array([x, y, z]) for z in (-0.3, 0.0, 0.3) for y in g for x in g]
    is_corner = lambda c: abs(abs(c[0]) - 0.45) < 1e-9 and abs(abs(c[1]) - 0.45) < 1e-9
    is_mid = lambda c: abs(c[0]) < 0.1 and abs(c[1]) < 0.1 and c[2] == 0.0
    corner = [c for c in cells if is_corner(c)]                          # 12
    mid = [c for c in cells if is_mid(c)]                                # 4
    rest = [c for c in cells if not is_corner(c) and not is_mid(c)]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    tris, label, aspect = [], [], []

    def put(tri, name, s):
        tris.append(tri)
        label.append(name)
        aspect.append(s)

    for k, edge in enumerate(TINY_EDGES + TINY_EDGES):                   # near +-0.45
        put(tiny(edge, corner[2 * k], frame(rng)), "tiny", edge)
    for k in range(2):                                                   # 2 pairs straddling
        fr = frame(rng, 0.2)
        for tri, name in zip(threshold_pair(rng, mid[2 * k:2 * k + 2], 0.07, fr,
                                            ("needle", "cap")[k]),
                             ("threshold_flat", "threshold_open")):
            put(tri, name, 1e-6)
    for which in DEGENERATE:
        put(degenerate(which, rest.pop()), "degenerate", 0.0)
    combos = [(f, v, s) for f in ("needle", "cap") for v in range(3) for s in ASPECTS]
    k = 0
    while rest:
        f, v, s = combos[k % len(combos)]
        k += 1
        put(sliver(f, s, v, rest.pop(), rng.uniform(0.05, 0.08), frame(rng, 0.2)), f, s)
    order = rng.permutation(len(tris))              # slivers in both LDS tiles
    tris = np.stack(tris)[order]
    label, aspect = np.array(label)[order], np.array(aspect)[order]
    pts, kind, owner = [], [], []
    for i, tri in enumerate(tris):
        p, kd = queries(tri, rng, n_face=n_face, hmax=hmax)
        pts.append(p)
        kind.append(kd)
        owner.append(np.full(len(kd), i))
    order = rng.permutation(sum(len(p) for p in pts))   # every workgroup sees every kind
    return dict(tris=tris, label=label, aspect=aspect, pts=np.concatenate(pts)[order],
                kind=np.concatenate(kind)[order], owner=np.concatenate(owner)[order])


def nearest(pts, tris):
    """(distance, arg-min triangle) of the fp64 oracle, (n,) each."""
    d2 = M.tri_d2(np.asarray(pts, f64)[:, None, :], np.asarray(tris, f64)[None])
    return np.sqrt(d2.min(1)), d2.argmin(1)


def in_face_region(pts, tris, idx):
    """Does the foot of pts[i] lie strictly inside triangle idx[i] (all barycentrics > 0)?"""
    ok = sin2_at_a(tris[idx]) > FLAT_SIN2
    out = np.zeros(len(pts), bool)
    out[ok] = barycentrics(pts[ok], tris[idx][ok]).min(-1) > 0
    return out


# ------------------------------------------------------------------ the header, restated

def _fma(a, b, c):
    """fmaf: one rounding of the fp64 product-sum (the product of two floats is exact in fp64;
    the sum is rounded twice, which differs from a true fma in rare half-way cases only)."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _dot3(a, b):
    return _fma(a[..., 0], b[..., 0], _fma(a[..., 1], b[..., 1], a[..., 2] * b[..., 2]))


def _cross32(a, b):
    """The header's a.y*b.z - a.z*b.y ...: float32 products, float32 difference."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


INSIDE_TAU = f32(2.5e-7)               # the header's margin of the inside test
THIN_SIN2 = f32(1e-3)                  # the header's switch to an fp64 normal


def emu_record(tris, normal="fp64", tau=INSIDE_TAU):
    """build_record for float32 triangles (..., 3, 3), field by field.  normal = "fp64" (the
    header): where the fp32 cross product says sin^2 at a <= THIN_SIN2, the normal and `flat`
    from the exact edges in fp64, rounded to float32 once; everything else (edges, inverse lengths, in-plane edge normals from the stored n^) in
    float32; the inside test's offset -tau |m| beside each edge normal.  normal = "fp32",
    tau = 0: the record as it was before this test file existed — edges, cross product,
    `flat` and 1/sqrtf in float32 and an inside test at 0."""
    t = np.asarray(tris, f32)
    a, b, c = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    ab, ac, bc = b - a, c - a, c - b
    ab2, ac2, bc2 = _dot3(ab, ab), _dot3(ac, ac), _dot3(bc, bc)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        n = _cross32(ab, ac)
        nn = _dot3(n, n)
        flat = ~(nn > f32(1e-12) * ab2 * ac2)
        inv = np.where(flat, f32(0), f32(1) / np.sqrt(np.where(flat, f32(1), nn)))
        n = n * inv[..., None]
        if normal == "fp64":
            thin = ~(nn > THIN_SIN2 * ab2 * ac2)
            dab, dac = b.astype(f64) - a.astype(f64), c.astype(f64) - a.astype(f64)
            dn = np.cross(dab, dac)
            dnn = _dot(dn, dn)
            dflat = ~(dnn > 1e-12 * _dot(dab, dab) * _dot(dac, dac))
            dinv = np.where(dflat, 0.0, 1.0 / np.sqrt(np.where(dflat, 1.0, dnn)))
            flat = np.where(thin, dflat, flat)
            n = np.where(thin[..., None], (dn * dinv[..., None]).astype(f32), n)
        inv_len = lambda x: np.where(x > 0, f32(1) / np.where(x > 0, x, f32(1)), f32(0))
        return dict(a=a, ab=ab, ac=ac, bc=bc, iab=inv_len(ab2), iac=inv_len(ac2),
                    ibc=inv_len(bc2), flat=flat, n=n, m_ab=_cross32(n, ab), m_ac=_cross32(ac, n),
                    m_bc=_cross32(n, bc), w_ab=-f32(tau) * np.sqrt(ab2),
                    w_ac=-f32(tau) * np.sqrt(ac2), w_bc=-f32(tau) * np.sqrt(bc2))


def _seg_d2(q, e, ie):
    tt = np.clip(_dot3(q, e) * ie, f32(0), f32(1))
    r = np.stack([_fma(-tt, e[..., k], q[..., k]) for k in range(3)], -1)
    return _dot3(r, r)


def emu_tri_d2(p, rec):
    """tri_d2 of the header for points p (..., 3) float32 against the records, float32."""
    p = np.asarray(p, f32)
    q = p - rec["a"]
    qb = q - rec["ab"]
    e = np.minimum(_seg_d2(q, rec["ab"], rec["iab"]), _seg_d2(q, rec["ac"], rec["iac"]))
    e = np.minimum(e, _seg_d2(qb, rec["bc"], rec["ibc"]))
    h = _dot3(q, rec["n"])
    side = lambda x, m, w: _fma(x[..., 0], m[..., 0], _fma(x[..., 1], m[..., 1],
                                                           _fma(x[..., 2], m[..., 2], w)))
    inside = ((side(q, rec["m_ab"], rec["w_ab"]) >= 0) & (side(q, rec["m_ac"], rec["w_ac"]) >= 0)
              & (side(qb, rec["m_bc"], rec["w_bc"]) >= 0) & ~rec["flat"])
    return np.where(inside, np.minimum(h * h, e), e)


def emu_distance(pts, tri, normal="fp64", tau=INSIDE_TAU):
    """sqrtf(tri_d2) of every point against ONE triangle, float32 (n,)."""
    return np.sqrt(emu_tri_d2(pts, emu_record(np.asarray(tri, f32)[None], normal, tau)))


def reference_distance(pts, tri):
    """Distance to ONE float32 triangle in long double, by the decomposition the kernel uses
    (nearest edge, or the plane distance where the foot has no negative barycentric; `flat`
    by the rule): a check of the fp64 oracle where its own products cancel."""
    t = np.asarray(tri, f32).astype(ld)
    p = np.asarray(pts, f32).astype(ld)

    def seg(q, e):
        ee = _dot(e, e)
        tt = np.clip(_dot(q, e) / (ee if ee > 0 else 1), 0, 1) if ee > 0 else np.zeros(len(q))
        r = q - tt[:, None] * e
        return _dot(r, r)

    a, b, c = t
    e = np.minimum(np.minimum(seg(p - a, b - a), seg(p - a, c - a)), seg(p - b, c - b))
    if sin2_at_a(tri) <= FLAT_SIN2:
        return np.sqrt(e).astype(f64)
    n = np.cross(b - a, c - a)
    h2 = ((p - a) @ n) ** 2 / _dot(n, n)
    return np.sqrt(np.where(barycentrics(pts, tri).min(-1) >= 0, np.minimum(h2, e), e)).astype(f64)
