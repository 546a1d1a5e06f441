"""CPU oracle for the grid-path kernels (pntf_grid_descent, pntf_grid_polyline_time) — TEST
INFRASTRUCTURE.

Restates the "Grid paths" text of include/pntf.h in numpy, operation by operation: the cell of a
point, the trilinear value and gradient summed in the written-down order, the descent of a solved
T from a goal back to its source, and the midpoint-rule travel time of polylines.  Every routine
runs in fp64 or, with dtype=np.float32, with every operation rounded to fp32 (the reference's own
rounding error, which sizes the kernels' bound), like tests/eikonal_oracle.py.  The arrays (T,
speed, points) are always taken as the fp32 values the kernels see.  The reference has no such
code; tests/test_grid_path.py pins this one by closed forms.
"""
import numpy as np

ARRIVED, TRUNCATED, STALLED, BLOCKED, UNREACHABLE = range(5)
MAX_PIECES = 65536
LANES = 256

# corner l = 4 di + 2 dj + dk
CORNERS = np.array([[l >> 2, (l >> 1) & 1, l & 1] for l in range(8)])


def clamp(x):
    """min(max(x, -0.5), 0.5) with the min / max that return the operand that is a number."""
    return np.fmin(np.fmax(x, x.dtype.type(-0.5)), x.dtype.type(0.5))


def cell(x, n):
    """Per axis: i = min((int)u, n - 2), w = u - i for u = (clamp(x) + 0.5)(n - 1); x (..., 3)."""
    dt = x.dtype.type
    u = (clamp(x) + dt(0.5)) * dt(n - 1)
    i = np.minimum(u.astype(np.int64), n - 2)
    return i, u - i.astype(x.dtype)


def sum8(t):
    return ((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])) + \
        ((t[..., 4] + t[..., 5]) + (t[..., 6] + t[..., 7]))


def interp(A, x, rows=None, positive=False, grad=True):
    """Value, gradient and blocked flag of the array A at the points x (m, 3) (x's dtype is the
    arithmetic's).  A is (n, n, n), or (q, n, n, n) with rows (m,) naming each point's array.
    Returns (V (m,), g (m, 3) or None, blocked (m,))."""
    n, dt = A.shape[-1], x.dtype.type
    i, w = cell(x, n)
    idx = i[:, None, :] + CORNERS[None]
    if A.ndim == 4:
        a = A[np.asarray(rows)[:, None], idx[..., 0], idx[..., 1], idx[..., 2]]
    else:
        a = A[idx[..., 0], idx[..., 1], idx[..., 2]]
    a = a.astype(x.dtype)
    blocked = ~np.isfinite(a).all(axis=1)
    if positive:
        blocked |= ~(a > 0).all(axis=1)
    sel = np.where(CORNERS[None] == 1, w[:, None, :], dt(1) - w[:, None, :])
    wa, wb, wc = sel[..., 0], sel[..., 1], sel[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        V = sum8(a * ((wa * wb) * wc))
        if not grad:
            return V, None, blocked
        sign = np.where(CORNERS == 1, dt(1), dt(-1))
        g = np.stack([sum8(sign[:, 0] * (a * (wb * wc))), sum8(sign[:, 1] * (a * (wa * wc))),
                      sum8(sign[:, 2] * (a * (wa * wb)))], axis=1) * dt(n - 1)
    return V, g, blocked


def default_points(n, step):
    return int(np.ceil(4.0 * (n - 1) / step)) + 2


def descent(T, src, goal, radius=4.0, step=0.5, L=None, dtype=np.float64):
    """pntf_grid_descent for T (q, n, n, n), src and goal (q, 3): (pts (q, L, 3) in `dtype`, cnt,
    status (q,) int32, tgoal (q,) in `dtype`).  All queries advance together; each is computed
    on its own."""
    T = np.asarray(T, np.float32)
    q, n = T.shape[0], T.shape[1]
    dt = dtype
    xs = clamp(np.asarray(src, np.float32).reshape(q, 3).astype(dt))
    x = clamp(np.asarray(goal, np.float32).reshape(q, 3).astype(dt))
    L = default_points(n, step) if L is None else int(L)
    h = dt(1) / dt(n - 1)
    r = max(dt(np.float32(radius)), dt(2)) * h
    r2, s = r * r, dt(np.float32(step)) * h
    pts = np.zeros((q, L, 3), dt)
    cnt = np.ones(q, np.int32)
    status = np.full(q, ARRIVED, np.int32)
    pts[:, 0] = x
    every = np.arange(q)
    V, g, blocked = interp(T, x, every)
    tgoal = np.where(blocked, dt(np.inf), V).astype(dt)
    status[blocked] = UNREACHABLE
    done = blocked.copy()
    bits = np.int64 if dt == np.float64 else np.int32
    while not done.all():
        d = x - xs
        arrived = ~done & ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2)
        need = arrived & (x.view(bits) != xs.view(bits)).any(axis=1)
        status[need & (cnt == L)] = TRUNCATED
        app = need & (cnt < L)
        pts[app, cnt[app]] = xs[app]
        cnt[app] += 1
        done |= arrived
        with np.errstate(invalid="ignore", over="ignore"):
            gn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        flat = ~done & (~(gn > 0) | ~np.isfinite(gn))
        status[flat] = STALLED
        done |= flat
        j = np.nonzero(~done)[0]
        if not len(j):
            break
        xn = clamp(x[j] - s * (g[j] / gn[j, None]))
        Vn, gnew, bl = interp(T, xn, j)
        status[j[bl]] = BLOCKED
        with np.errstate(invalid="ignore"):
            stall = ~bl & ~(Vn < V[j])
        status[j[stall]] = STALLED
        full = ~bl & ~stall & (cnt[j] == L)
        status[j[full]] = TRUNCATED
        go = ~bl & ~stall & ~full
        done[j[~go]] = True
        k = j[go]
        pts[k, cnt[k]] = xn[go]
        cnt[k] += 1
        x[k], V[k], g[k] = xn[go], Vn[go], gnew[go]
    return pts, cnt, status, tgoal


def polyline_time(speed, pts, cnt, sub=0.5, dtype=np.float64):
    """pntf_grid_polyline_time for speed (n, n, n), pts (q, L, 3), cnt (q,): time (q,) in
    `dtype`, with the kernel's order of additions (lane j of 256 owns segments j, j + 256, ...;
    the pairwise tree over adjacent lanes)."""
    speed = np.asarray(speed, np.float32)
    pts = np.asarray(pts, np.float32)
    n, dt = speed.shape[0], dtype
    q, L = pts.shape[0], pts.shape[1]
    piece = dt(np.float32(sub)) * (dt(1) / dt(n - 1))
    out = np.zeros(q, dt)
    for c in range(q):
        k = min(max(int(cnt[c]), 0), L)
        acc = np.zeros(LANES, dt)
        if k >= 2:
            P = pts[c, :k].astype(dt)
            a, d = P[:-1], P[1:] - P[:-1]
            with np.errstate(over="ignore", invalid="ignore"):
                ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            for i in range(k - 1):
                lane = i % LANES
                if not np.isfinite(ln[i]):
                    acc[lane] = acc[lane] + ln[i]
                    continue
                if ln[i] == 0:
                    continue
                with np.errstate(divide="ignore", over="ignore"):
                    mf = dt(min(max(np.ceil(ln[i] / piece), 1.0), MAX_PIECES))
                dl = ln[i] / mf
                t = (np.arange(int(mf)).astype(dt) + dt(0.5)) / mf
                mid = a[i] + t[:, None] * d[i]
                V, _, bl = interp(speed, mid, positive=True, grad=False)
                with np.errstate(divide="ignore", invalid="ignore"):
                    add = np.where(bl, dt(np.inf), dl / V).astype(dt)
                acc[lane] = np.cumsum(np.concatenate([acc[lane:lane + 1], add]), dtype=dt)[-1]
        while len(acc) > 1:
            acc = acc[0::2] + acc[1::2]
        out[c] = acc[0]
    return out


def point_polyline_distance(p, line):
    """Distance (fp64) from the point p (3,) to the polyline line (k, 3), k >= 1."""
    p, line = np.asarray(p, np.float64), np.asarray(line, np.float64)
    if len(line) == 1:
        return float(np.linalg.norm(p - line[0]))
    a, d = line[:-1], line[1:] - line[:-1]
    dd = (d * d).sum(axis=1)
    t = np.clip(((p - a) * d).sum(axis=1) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
    return float(np.linalg.norm(a + t[:, None] * d - p, axis=1).min())


def path_distance(pts, cnt, ref_pts, ref_cnt):
    """Per query, the maximum distance from each of its points to the reference's polyline."""
    return np.array([max(point_polyline_distance(p, ref_pts[c, :ref_cnt[c]])
                         for p in pts[c, :cnt[c]]) for c in range(len(cnt))])
