"""CPU oracle for the grid travel-time solver (pntf_grid_travel_time_*) — TEST INFRASTRUCTURE.

Restates the scheme of include/pntf.h in numpy: the Jacobi iteration of the first-order upwind
Eikonal update to its exact fixed point (`solve`), in fp64 or, with dtype=np.float32, with every
operation of the iteration rounded to fp32 (the reference's own rounding error, which sizes the
kernel's bound).  The initial state's geometry is fp64 in both, as in the kernel.  A heap-ordered
fast-marching solve (`fast_march`) shares only the single-node update with it and is kept for
one test.  The reference has no such solver; tests/test_eikonal_grid.py pins this one by closed
forms.
"""
import heapq

import numpy as np


def nodes(n):
    """Node coordinates (n, n, n, 3) float64: -0.5 + h (i, j, k), h = 1 / (n - 1)."""
    ax = -0.5 + (1.0 / (n - 1)) * np.arange(n, dtype=np.float64)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)


def nearest_node(n, src):
    u = (np.asarray(src, np.float64) + 0.5) * float(n - 1)
    return tuple(np.clip(np.floor(u + 0.5), 0, n - 1).astype(int))


def ball(n, src, radius):
    """(inside (n, n, n) bool, d2 (n, n, n)): the nearest node and |x - x_s|^2 <= (radius h)^2."""
    d = nodes(n) - np.asarray(src, np.float64)
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    rh = float(np.float32(radius)) * (1.0 / (n - 1))
    inside = d2 <= rh * rh
    inside[nearest_node(n, src)] = True
    return inside, d2


def init_state(speed, src, radius, dtype=np.float64):
    """T0 (n, n, n) for one source; speed and src are taken as the fp32 values the kernel sees."""
    speed = np.asarray(speed, np.float32)
    n = speed.shape[0]
    src = np.asarray(src, np.float32)
    inside, d2 = ball(n, src, radius)
    s_near = speed[nearest_node(n, src)]
    T = np.full(speed.shape, np.inf, dtype)
    if s_near > 0:
        m = inside & (speed > 0)
        if dtype == np.float32:
            T[m] = np.sqrt(d2[m]).astype(np.float32) / s_near
        else:
            T[m] = np.sqrt(d2[m]) / np.float64(s_near)
    return T


def node_update(a, b, c, f):
    """One update from the sorted per-axis minima a <= b <= c (arrays or scalars of one dtype)."""
    a, b, c, f = np.broadcast_arrays(a, b, c, f)
    with np.errstate(invalid="ignore", over="ignore"):
        t = a + f
        two = np.isfinite(b) & (t > b)
        a2, b2 = np.where(two, a, 0), np.where(two, b, 0)
        d = a2 - b2
        t = np.where(two, (a2 + b2 + np.sqrt(np.maximum(2 * f * f - d * d, 0))) / 2, t)
        three = two & np.isfinite(c) & (t > c)
        a3, b3, c3 = np.where(three, a, 0), np.where(three, b, 0), np.where(three, c, 0)
        s = a3 + b3 + c3
        disc = s * s - 3 * (a3 * a3 + b3 * b3 + c3 * c3 - f * f)
        t = np.where(three, (s + np.sqrt(np.maximum(disc, 0))) / 3, t)
    return t


def cell_f(speed, dtype):
    """f = h / S at the open nodes (h and the quotient in `dtype`), +inf at walls; open mask."""
    speed = np.asarray(speed, np.float32)
    n = speed.shape[0]
    open_ = speed > 0
    h = dtype(1) / dtype(n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(open_, h / np.where(open_, speed, 1).astype(dtype), np.inf).astype(dtype)
    return f, open_


def sweep(T, f, open_):
    """One Jacobi update of every node of T (..., n, n, n) from the previous values."""
    pad = [(0, 0)] * (T.ndim - 3) + [(1, 1)] * 3
    P = np.pad(T, pad, constant_values=np.inf)
    c = slice(1, -1)
    m = np.stack([np.minimum(P[..., :-2, c, c], P[..., 2:, c, c]),
                  np.minimum(P[..., c, :-2, c], P[..., c, 2:, c]),
                  np.minimum(P[..., c, c, :-2], P[..., c, c, 2:])])
    m.sort(axis=0)
    t = node_update(m[0], m[1], m[2], f)
    return np.where(open_, np.minimum(T, t), T).astype(T.dtype)


def solve(speed, srcs, radius=4.0, dtype=np.float64, max_sweeps=100000):
    """Fixed point of the Jacobi iteration for the sources srcs (q, 3): (T (q, n, n, n) in
    `dtype`, sweeps run until one changed nothing)."""
    srcs = np.atleast_2d(np.asarray(srcs, np.float32))
    T = np.stack([init_state(speed, s, radius, dtype) for s in srcs])
    f, open_ = cell_f(speed, dtype)
    for it in range(max_sweeps):
        new = sweep(T, f, open_)
        if np.array_equal(new, T):
            return T, it
        T = new
    raise RuntimeError("the Jacobi iteration did not reach its fixed point")


def fast_march(speed, src, radius=4.0):
    """Heap-ordered fast marching in fp64 from the same initial state: nodes are accepted in
    order of their value; accepting one recomputes its open neighbours."""
    T = init_state(speed, src, radius, np.float64)
    f, open_ = cell_f(speed, np.float64)
    n = T.shape[0]
    P = np.full((n + 2,) * 3, np.inf)
    P[1:-1, 1:-1, 1:-1] = T
    done = np.zeros(T.shape, bool)
    heap = [(T[ijk], ijk) for ijk in zip(*np.nonzero(np.isfinite(T)))]
    heapq.heapify(heap)
    steps = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
    while heap:
        t, (i, j, k) = heapq.heappop(heap)
        if done[i, j, k] or t > P[i + 1, j + 1, k + 1]:
            continue
        done[i, j, k] = True
        for di, dj, dk in steps:
            x, y, z = i + di, j + dj, k + dk
            if not (0 <= x < n and 0 <= y < n and 0 <= z < n) or done[x, y, z] or \
                    not open_[x, y, z]:
                continue
            a, b, c = sorted((min(P[x, y + 1, z + 1], P[x + 2, y + 1, z + 1]),
                              min(P[x + 1, y, z + 1], P[x + 1, y + 2, z + 1]),
                              min(P[x + 1, y + 1, z], P[x + 1, y + 1, z + 2])))
            new = float(node_update(np.float64(a), np.float64(b), np.float64(c), f[x, y, z]))
            if new < P[x + 1, y + 1, z + 1]:
                P[x + 1, y + 1, z + 1] = new
                heapq.heappush(heap, (new, (x, y, z)))
    return P[1:-1, 1:-1, 1:-1].copy()
