"""fp64 oracle for segment / polyline -> triangle-mesh distance — TEST INFRASTRUCTURE ONLY.

Same decomposition as the kernel (csrc/pntf_path_geom.h), written independently of it: the
squared distance of a (segment, triangle) pair is the minimum of the two endpoint distances
(oracle.mesh_oracle.tri_d2, Ericson §5.1.5 with its branches), the three segment-to-edge
distances by the textbook clamped routine (Ericson §5.1.9, with its case split and its
|d1|²|d2|² - (d1·d2)² denominator) and 0 when the segment pierces the triangle (the crossing
point of the plane, located by a division, and classified by barycentric coordinates).
Pinned in tests/test_path_clearance.py by closed forms and by a sampled sandwich that does not
share the decomposition.
"""
import numpy as np

from oracle import mesh_oracle as M

_dot = lambda x, y: np.einsum("...k,...k->...", x, y)


def seg_seg_d2(p1, q1, p2, q2):
    """Squared distance between segments p1-q1 and p2-q2 (..., 3), broadcasting (Ericson
    §5.1.9, ClosestPtSegmentSegment)."""
    p1, q1, p2, q2 = np.broadcast_arrays(*[np.asarray(x, np.float64) for x in (p1, q1, p2, q2)])
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = _dot(d1, d1), _dot(d2, d2), _dot(d2, r)
    c, b = _dot(d1, r), _dot(d1, d2)
    one = lambda x: np.where(x > 0, x, 1.0)
    denom = a * e - b * b
    s = np.where(denom > 1e-14 * a * e, np.clip((b * f - c * e) / one(denom), 0.0, 1.0), 0.0)
    s = np.where(a > 0, s, 0.0)
    t = np.where(e > 0, (b * s + f) / one(e), 0.0)
    s_lo = np.where(a > 0, np.clip(-c / one(a), 0.0, 1.0), 0.0)         # t < 0 -> t = 0
    s_hi = np.where(a > 0, np.clip((b - c) / one(a), 0.0, 1.0), 0.0)    # t > 1 -> t = 1
    s = np.where((t < 0) | ~(e > 0), s_lo, np.where(t > 1, s_hi, s))   # a point: t = 0
    t = np.clip(t, 0.0, 1.0)
    v = (p1 + s[..., None] * d1) - (p2 + t[..., None] * d2)
    return _dot(v, v)


def pierces(p0, p1, tri):
    """Does segment p0-p1 cross the triangle's plane at a point of the triangle?  Coplanar
    segments (both offsets zero) and flat triangles (the kernel's test) never do."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)
    nn = _dot(n, n)
    flat = nn <= 1e-12 * _dot(ab, ab) * _dot(ac, ac)
    h0, h1 = _dot(n, p0 - a), _dot(n, p1 - a)
    cross = (h0 * h1 <= 0) & (h0 != h1) & ~flat
    u = h0 / np.where(h0 != h1, h0 - h1, 1.0)
    x = p0 + u[..., None] * (p1 - p0) - a
    safe = np.where(nn > 0, nn, 1.0)
    v = _dot(np.cross(x, ac), n) / safe           # x = v·ab + w·ac in the plane
    w = _dot(np.cross(ab, x), n) / safe
    return cross & (v >= 0) & (w >= 0) & (v + w <= 1)


def seg_tri_d2(p0, p1, tri):
    """Squared distance from segments p0-p1 (..., 3) to triangles tri (..., 3, 3)."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    tri = np.asarray(tri, np.float64)
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    d = np.minimum(M.tri_d2(p0, tri), M.tri_d2(p1, tri))
    for u, v in ((a, b), (a, c), (b, c)):
        d = np.minimum(d, seg_seg_d2(p0, p1, u, v))
    return np.where(pierces(p0, p1, tri), 0.0, d)


def segment_distances(pts, tris, chunk=128):
    """Distance (cnt - 1,) of every segment of the polyline pts (cnt, 3) to the mesh; a single
    point (cnt 1) counts as one zero-length segment."""
    pts = np.asarray(pts, np.float64)
    tris = np.asarray(tris, np.float64)
    p0, p1 = (pts, pts) if len(pts) == 1 else (pts[:-1], pts[1:])
    out = np.empty(len(p0))
    for s in range(0, len(p0), chunk):
        d2 = seg_tri_d2(p0[s:s + chunk, None, :], p1[s:s + chunk, None, :], tris[None])
        out[s:s + chunk] = np.sqrt(d2.min(axis=1))
    return out


TIE = 1e-12      # fp64 rounding between two routes to the same closest point


def polyline_distance(pts, tris):
    """(distance, where, runner_up) of one polyline: the minimum over its segments, the lowest
    segment index within TIE of it (two segments nearest at their shared point tie, up to
    rounding) and the smallest distance of a segment outside that tie (inf if none).  An empty
    polyline gives (inf, -1, inf)."""
    if len(pts) == 0:
        return np.inf, -1, np.inf
    d = segment_distances(pts, tris)
    tie = d <= d.min() + TIE
    rest = d[~tie]
    return d.min(), int(np.argmax(tie)), (rest.min() if len(rest) else np.inf)


def sampled_distance(p0, p1, tri, k):
    """min over k + 1 evenly spaced points of the segment of the POINT oracle: an upper bound
    of the distance, and within |p1 - p0| / (2k) of it (the distance to a set is 1-Lipschitz)."""
    u = np.linspace(0.0, 1.0, k + 1)[:, None]
    p = np.asarray(p0, np.float64)[None] * (1 - u) + np.asarray(p1, np.float64)[None] * u
    return np.sqrt(M.tri_d2(p, np.asarray(tri, np.float64)[None]).min())
