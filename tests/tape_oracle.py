"""Per-operation references of the Taylor-tape kernels (csrc/pntf_train.hip) — TEST ONLY.

One plain function per operation, written from the mathematics of the reference's
input_mapping_laplace, act_laplace, the start/goal merge, actout_laplace and Model.Loss, on the
plane layout of include/pntf.h: a Taylor tensor of m points and width w is (R, m, w),
R = 1 + ndir + nl planes [value | ndir first-derivative rows | nl second-derivative rows].

The functions are generic over what they compute on:

  * torch tensors of any float dtype: float64 is the reference, float32 the yardstick the
    tolerance constants are measured with (tests/test_tape_kernels.py), and with
    requires_grad inputs `vjp` takes every adjoint from torch.autograd — no hand-derived
    formula enters a reference adjoint;
  * `Bd` values, which carry beside the fp64 value v an error scale A >= |v|: the BOUND FORM.
    Every operation propagates A to first order with every term and coefficient replaced by
    its absolute value (a + b -> A_a + A_b, a·b -> A_a|b| + |a|A_b, f(a) -> |f(a)| + |f'(a)|A_a,
    a sum over n terms -> sqrt(n)·ΣA as the GEMM tests do), so that L' = σ'ΣJ² + σL gets
    |σ'|ΣJ² + σ|L| plus what the rounding of 10·y does to σ.  An fp32 evaluation in any
    operation order, with fused multiply-adds and library functions a few ulp off, errs by a
    small multiple of eps32·A elementwise.  An input is Bd(x) with A = |x| (exact in fp32).

The adjoints' bound forms are written out by hand (`act_bwd`, `merge_bwd`, `fourier_bwd`,
`head_vjp`, `loss_bwd`) in the same generic style; their values are checked against autograd
and against oracle/pntf_oracle.py by the host tests, so a slip in a bound form shows.
"""
import math

import torch

H = 128
SCALE = 10.0
TWO_PI = 2.0 * math.pi
EPS32 = 2.0 ** -23
TINY32 = 2.0 ** -126          # smallest normal fp32


# ------------------------------------------------------------------ bound-form values


class Bd:
    """fp64 value v with its first-order error scale A (>= |v|), in units of eps32."""

    def __init__(self, v, A=None):
        self.v = v
        self.A = v.abs() if A is None else A

    @property
    def shape(self):
        return self.v.shape

    def __getitem__(self, i):
        return Bd(self.v[i], self.A[i])

    def __neg__(self):
        return Bd(-self.v, self.A)

    def __add__(self, o):
        if isinstance(o, Bd):
            return Bd(self.v + o.v, self.A + o.A)
        return Bd(self.v + o, self.A + abs(o))

    __radd__ = __add__

    def __sub__(self, o):
        if isinstance(o, Bd):
            return Bd(self.v - o.v, self.A + o.A)
        return Bd(self.v - o, self.A + abs(o))

    def __rsub__(self, o):
        return Bd(o - self.v, self.A + abs(o))

    def __mul__(self, o):
        if isinstance(o, Bd):
            return Bd(self.v * o.v, self.A * o.v.abs() + self.v.abs() * o.A)
        return Bd(self.v * o, self.A * abs(o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Bd):
            return self * Bd(1.0 / o.v, 1.0 / o.v.abs() + o.A / (o.v * o.v))
        return Bd(self.v / o, self.A / abs(o))

    def __rtruediv__(self, o):
        return Bd(o / self.v, abs(o) * (1.0 / self.v.abs() + self.A / (self.v * self.v)))


def _isb(x):
    return isinstance(x, Bd)


def _val(x):
    return x.v if _isb(x) else x


def _fn(x, f, df):
    """f(x); bound form |f| + |f'|·A."""
    if not _isb(x):
        return f(x)
    fv = f(x.v)
    return Bd(fv, fv.abs() + df(x.v, fv).abs() * x.A)


def _exp(x):
    return _fn(x, torch.exp, lambda v, f: f)


def _log1p(x):
    return _fn(x, torch.log1p, lambda v, f: 1.0 / (1.0 + v))


def _sigmoid(x):
    return _fn(x, torch.sigmoid, lambda v, f: f * (1.0 - f))


def _sin(x):
    return _fn(x, torch.sin, lambda v, f: torch.cos(v))


def _cos(x):
    return _fn(x, torch.cos, lambda v, f: torch.sin(v))


def _sqrt(x):
    return _fn(x, torch.sqrt, lambda v, f: 0.5 / f)


def _abs(x):
    return Bd(x.v.abs(), x.A) if _isb(x) else x.abs()


def _clamp_max(x, hi):
    return Bd(x.v.clamp(max=hi), x.A) if _isb(x) else x.clamp(max=hi)


def _where(c, a, b):
    if _isb(a):
        return Bd(torch.where(c, a.v, b.v), torch.where(c, a.A, b.A))
    return torch.where(c, a, b)


def _max(a, b):
    return _where(_val(a) >= _val(b), a, b) if _isb(a) else torch.maximum(a, b)


def _min(a, b):
    return _where(_val(a) <= _val(b), a, b) if _isb(a) else torch.minimum(a, b)


def _cat(xs, dim):
    if _isb(xs[0]):
        return Bd(torch.cat([x.v for x in xs], dim), torch.cat([x.A for x in xs], dim))
    return torch.cat(xs, dim)


def _stack(xs, dim=0):
    if _isb(xs[0]):
        return Bd(torch.stack([x.v for x in xs], dim), torch.stack([x.A for x in xs], dim))
    return torch.stack(xs, dim)


def _rsum(x, dim):
    """Sum over `dim`; bound form sqrt(terms)·ΣA."""
    if _isb(x):
        return Bd(x.v.sum(dim), math.sqrt(max(x.v.shape[dim], 1)) * x.A.sum(dim))
    return x.sum(dim)


def _un(x, dim):
    return Bd(x.v.unsqueeze(dim), x.A.unsqueeze(dim)) if _isb(x) else x.unsqueeze(dim)


def bd(*xs):
    """fp64 bound-form inputs (A = |x|) of fp32 tensors; None stays None."""
    out = [None if x is None else Bd(x.double()) for x in xs]
    return out[0] if len(out) == 1 else out


# ------------------------------------------------------------------ elementwise


def sig10(y):
    """σ(10y) = softplus10'."""
    return _sigmoid(y * SCALE)


def softplus10(y):
    """torch.nn.Softplus(beta=10), threshold 20: the identity where 10y > 20."""
    soft = _log1p(_exp(_clamp_max(y * SCALE, 20.0))) / SCALE
    return _where(_val(y) * SCALE > 20.0, y, soft)


# ------------------------------------------------------------------ Fourier planes


def _fourier_parts(xp, Btab, env, dim):
    n = xp.shape[0]
    e = torch.zeros(n, dtype=torch.long) if env is None else env.long()
    w = Btab[e] * TWO_PI                                  # (n, dim, 128)
    x = _cat([xp[:, :dim], xp[:, dim:]], 0)               # starts, then goals
    ww = _cat([w, w], 0)
    q = 0.0
    for k in range(dim):
        q = x[:, k:k + 1] * ww[:, k] + q
    return ww, _sin(q), _cos(q)


def fourier(xp, Btab, env, dim, ndir, nl):
    """input_mapping / _grad / _laplace: Φ = [sin q | cos q], q = 2π x·B; xp (n, 2 dim),
    Btab (n_env, dim, 128), env (n) or None -> phi (1 + ndir + nl, 2n, 256)."""
    ww, s, c = _fourier_parts(xp, Btab, env, dim)
    planes = [_cat([s, c], 1)]
    for k in range(ndir):
        planes.append(_cat([ww[:, k] * c, -(ww[:, k] * s)], 1))
    if nl == 1:
        w2 = 0.0
        for k in range(dim):
            w2 = ww[:, k] * ww[:, k] + w2
        planes.append(_cat([-(w2 * s), -(w2 * c)], 1))
    elif nl:
        for k in range(dim):
            wk2 = ww[:, k] * ww[:, k]
            planes.append(_cat([-(wk2 * s), -(wk2 * c)], 1))
    return _stack(planes)


def fourier_bwd(gphi, xp, Btab, env, dim, ndir, nl):
    """Hand adjoint of `fourier` w.r.t. xp (the bound form of gx): (n, 2 dim)."""
    ww, s, c = _fourier_parts(xp, Btab, env, dim)
    n = xp.shape[0]
    G = gphi[0][:, :H] * c - gphi[0][:, H:] * s
    for k in range(ndir):
        G = G - ww[:, k] * (gphi[1 + k][:, :H] * s + gphi[1 + k][:, H:] * c)
    if nl == 1:
        w2 = 0.0
        for k in range(dim):
            w2 = ww[:, k] * ww[:, k] + w2
        G = G + w2 * (gphi[1 + ndir][:, H:] * s - gphi[1 + ndir][:, :H] * c)
    elif nl:
        for k in range(dim):
            g = gphi[1 + ndir + k]
            G = G + ww[:, k] * ww[:, k] * (g[:, H:] * s - g[:, :H] * c)
    gx = _stack([_rsum(G * ww[:, k], 1) for k in range(dim)], 1)       # (2n, dim)
    return _cat([gx[:n], gx[n:]], 1)


# ------------------------------------------------------------------ act_laplace


def act_planes(y, ndir, nl, act):
    """act_laplace on pre-activation planes y (R, m, w): h = softplus10(y), J' = σJ,
    L'_l = σ' Σ_{k∈l} J_k² + σ L_l (row l covers the J rows l·ndir/nl .. (l+1)·ndir/nl - 1).
    act == 2 (nl == 0): the out_backgrad encoder[0] quirk, J' = σ(10·softplus10(y))·J."""
    s = sig10(y[0])
    ds = s * (1.0 - s) * SCALE
    h = softplus10(y[0])
    out = [h]
    sJ = sig10(h) if act == 2 else s
    for k in range(ndir):
        out.append(y[1 + k] * sJ)
    gk = ndir // nl if nl else 0
    for l in range(nl):
        jj = 0.0
        for k in range(l * gk, (l + 1) * gk):
            jj = y[1 + k] * y[1 + k] + jj
        out.append(jj * ds + y[1 + ndir + l] * s)
    return _stack(out)


def act_bwd(y, g, ndir, nl, act):
    """Hand adjoint of `act_planes` (the bound form of dL/dy): g = dL/dh planes."""
    if act == 0:
        return g
    s = sig10(y[0])
    ds = s * (1.0 - s) * SCALE
    dds = ds * (1.0 - s * 2.0) * SCALE
    R = 1 + ndir + nl
    out = [None] * R
    gy = g[0] * s
    if nl == 0:
        sJ, dJ = s, ds
        if act == 2:
            sJ = sig10(softplus10(y[0]))
            dJ = sJ * (1.0 - sJ) * SCALE * s
        for k in range(ndir):
            gy = gy + g[1 + k] * y[1 + k] * dJ
            out[1 + k] = g[1 + k] * sJ
    gk = ndir // nl if nl else 0
    for l in range(nl):
        L, gL = y[1 + ndir + l], g[1 + ndir + l]
        jj = 0.0
        for k in range(l * gk, (l + 1) * gk):
            J, gJ = y[1 + k], g[1 + k]
            gy = gy + gJ * J * ds
            jj = J * J + jj
            out[1 + k] = gJ * s + gL * J * ds * 2.0
        gy = gy + gL * (jj * dds + L * ds)
        out[1 + ndir + l] = gL * s
    out[0] = gy
    return _stack(out)


# ------------------------------------------------------------------ start/goal merge


def merge_fwd(z, dim, nle):
    """Smooth max/min of the two endpoints: z (1 + dim + nle, 2n, 128) (starts, then goals) ->
    u (1 + 2 dim + 2 nle, n, 256) = [value | ∂xs | ∂xg | L_s | L_g], features [max | min].
    With d = zs - zg, s0 = σ(10d), s1 = 1 - s0, c = 10 s0 s1: value max/min ± log1p(e^-10|d|)/10;
    a start row J·[s0 | s1], a goal row J·[s1 | s0]; L_s = [c ΣJs² + Ls s0 | -c ΣJs² + Ls s1],
    L_g = [c ΣJg² + Lg s1 | -c ΣJg² + Lg s0].  dim = nle = 0: the value plane alone."""
    n = z.shape[1] // 2
    zs, zg = z[0][:n], z[0][n:]
    d = zs - zg
    lse = _log1p(_exp(-(_abs(d) * SCALE))) / SCALE
    s0 = sig10(d)
    s1 = 1.0 - s0
    c = s0 * s1 * SCALE
    u = [_cat([_max(zs, zg) + lse, _min(zs, zg) - lse], 1)]
    for k in range(dim):
        u.append(_cat([z[1 + k][:n] * s0, z[1 + k][:n] * s1], 1))
    for k in range(dim):
        u.append(_cat([z[1 + k][n:] * s1, z[1 + k][n:] * s0], 1))
    gk = dim // nle if nle else 0
    for e, (sa, sb) in enumerate(((s0, s1), (s1, s0))):
        for l in range(nle):
            jj = 0.0
            for k in range(l * gk, (l + 1) * gk):
                J = z[1 + k][:n] if e == 0 else z[1 + k][n:]
                jj = J * J + jj
            L = z[1 + dim + l][:n] if e == 0 else z[1 + dim + l][n:]
            u.append(_cat([c * jj + L * sa, L * sb - c * jj], 1))
    return _stack(u)


def merge_bwd(z, gu, dim, nle):
    """Hand adjoint of `merge_fwd` (the bound form of gz): gu (1 + 2 dim + 2 nle, n, 256) ->
    gz (1 + dim + nle, 2n, 128)."""
    n = z.shape[1] // 2
    d = z[0][:n] - z[0][n:]
    s0 = sig10(d)
    s1 = 1.0 - s0
    c = s0 * s1 * SCALE
    M = lambda r: gu[r][:, :H]            # noqa: E731
    m_ = lambda r: gu[r][:, H:]           # noqa: E731
    gk = dim // nle if nle else 1
    g_s0, g_c = 0.0, 0.0
    rows = [None] * (1 + dim + nle)
    dLs, dLg = [], []
    for l in range(nle):
        rs, rg = 1 + 2 * dim + l, 1 + 2 * dim + nle + l
        Ls, Lg = z[1 + dim + l][:n], z[1 + dim + l][n:]
        dLs.append(M(rs) - m_(rs))
        dLg.append(M(rg) - m_(rg))
        g_s0 = dLs[l] * Ls - dLg[l] * Lg + g_s0
        rows[1 + dim + l] = _cat([M(rs) * s0 + m_(rs) * s1, M(rg) * s1 + m_(rg) * s0], 0)
    for k in range(dim):
        Js, Jg = z[1 + k][:n], z[1 + k][n:]
        g_s0 = (M(1 + k) - m_(1 + k)) * Js - (M(1 + dim + k) - m_(1 + dim + k)) * Jg + g_s0
        gs = M(1 + k) * s0 + m_(1 + k) * s1
        gg = M(1 + dim + k) * s1 + m_(1 + dim + k) * s0
        if nle:
            l = k // gk
            g_c = dLs[l] * Js * Js + dLg[l] * Jg * Jg + g_c
            gs = gs + c * Js * dLs[l] * 2.0
            gg = gg + c * Jg * dLg[l] * 2.0
        rows[1 + k] = _cat([gs, gg], 0)
    kk = (g_s0 + g_c * (1.0 - s0 * 2.0) * SCALE) * c
    rows[0] = _cat([M(0) * s0 + m_(0) * s1 + kk, M(0) * s1 + m_(0) * s0 - kk], 0)
    return _stack(rows)


# ------------------------------------------------------------------ head


def head(v, w4, b4, dim, nle):
    """generator[4] + actout_laplace: v (1 + 2 dim + 2 nle, n, 128), w4 (128), b4 (1) ->
    τ = σ(0.1 (v_0·w4 + b4)) (n), ∇τ = y_k τ' (n, 2 dim), lap_l = τ'' Σ_{k∈l} y_k² + y_L τ'
    (n, 2 nle); τ' = 0.1 τ (1 - τ), τ'' = 0.1 τ' (1 - 2τ).  dim = nle = 0: τ alone."""
    nd, nlt = 2 * dim, 2 * nle
    yr = [_rsum(v[r] * w4, 1) for r in range(1 + nd + nlt)]
    t = _sigmoid((yr[0] + b4) * 0.1)
    dt = t * (1.0 - t) * 0.1
    ddt = dt * (1.0 - t * 2.0) * 0.1
    dtau = _stack([yr[1 + k] * dt for k in range(nd)], 1) if nd else None
    gk = dim // nle if nle else 1
    lap = []
    for l in range(nlt):
        jj = 0.0
        for k in range(l * gk, (l + 1) * gk):
            jj = yr[1 + k] * yr[1 + k] + jj
        lap.append(jj * ddt + yr[1 + nd + l] * dt)
    return t, dtau, (_stack(lap, 1) if nlt else None), (yr, dt, ddt)


def head_vjp(v, w4, b4, dim, nle, gt, gd, gl, cnt=None):
    """Hand adjoint of `head` (the bound forms of gv, gw4, gb4) under the upstream gt (n),
    gd (n, 2 dim), gl (n, 2 nle); None = zero.  cnt (n): how often each row counts in the
    sums gw4 and gb4 (a batch that repeats its rows), None = once."""
    nd, nlt = 2 * dim, 2 * nle
    t, _, _, (yr, dt, ddt) = head(v, w4, b4, dim, nle)
    dddt = (ddt * (1.0 - t * 2.0) - dt * dt * 2.0) * 0.1
    gk = dim // nle if nle else 1
    zero = dt * 0.0
    g0 = gt * dt if gt is not None else zero
    g = [None] * (1 + nd + nlt)
    for k in range(nd):
        J = yr[1 + k]
        gr = zero
        if gd is not None:
            g0 = g0 + gd[:, k] * J * ddt
            gr = gd[:, k] * dt
        if gl is not None:
            g0 = g0 + gl[:, k // gk] * J * J * dddt
            gr = gr + gl[:, k // gk] * J * ddt * 2.0
        g[1 + k] = gr
    for l in range(nlt):
        if gl is not None:
            g0 = g0 + gl[:, l] * yr[1 + nd + l] * ddt
            g[1 + nd + l] = gl[:, l] * dt
        else:
            g[1 + nd + l] = zero
    g[0] = g0
    gv = _stack([_un(gr, 1) * w4 for gr in g])
    if cnt is not None:
        g = [gr * cnt for gr in g]
    gw4 = 0.0
    for r, gr in enumerate(g):
        gw4 = _rsum(_un(gr, 1) * v[r], 0) + gw4
    return gv, gw4, _rsum(g[0], 0)


# ------------------------------------------------------------------ Model.Loss


def loss(t, dtau, lap, xp, yobs, dim, gamma, arm):
    """Model.Loss per pair from τ (n), ∇τ (n, 2 dim), the per-endpoint Laplacians lap (n, 2):
    D = x_goal - x_start, T0 = |D|², S_e = T0 |∇_eτ|² ± 2τ ∇_eτ·D + τ² (+ start, - goal),
    Ypred_e = 1 / (sqrt(S_e)/τ² + γ lap_e), diff = Σ_e (r_e + 1/r_e) - 4 with
    r_e = Ypred_e / yobs_e, or its square root for the arm model.  Returns diff (n) and the
    [S_0, S_1], [Ypred_0, Ypred_1] the inputs are conditioned on."""
    D = xp[:, dim:] - xp[:, :dim]
    T0 = 0.0
    for k in range(dim):
        T0 = D[:, k] * D[:, k] + T0
    diff, Ss, yps = 0.0, [], []
    for e, sgn in ((0, 1.0), (1, -1.0)):
        dd, nn = 0.0, 0.0
        for k in range(dim):
            dd = dtau[:, e * dim + k] * D[:, k] + dd
            nn = dtau[:, e * dim + k] * dtau[:, e * dim + k] + nn
        S = T0 * nn + t * dd * (2.0 * sgn) + t * t
        yp = 1.0 / (_sqrt(S) / (t * t) + lap[:, e] * gamma)
        yo = yobs[:, e]
        if arm:
            a, b = _sqrt(yp), _sqrt(yo)
            diff = a / b + b / a + diff
        else:
            diff = yp / yo + yo / yp + diff
        Ss.append(S)
        yps.append(yp)
    return diff - 4.0, Ss, yps


def loss_bwd(t, dtau, lap, xp, yobs, dim, gamma, scale, arm):
    """Hand adjoint of scale·Σ diff w.r.t. τ (n), ∇τ (n, 2 dim), lap (n, 2) (bound form)."""
    D = xp[:, dim:] - xp[:, :dim]
    T0 = 0.0
    for k in range(dim):
        T0 = D[:, k] * D[:, k] + T0
    gt, gd, gl = 0.0, [], []
    for e, sgn in ((0, 1.0), (1, -1.0)):
        dd, nn = 0.0, 0.0
        for k in range(dim):
            dd = dtau[:, e * dim + k] * D[:, k] + dd
            nn = dtau[:, e * dim + k] * dtau[:, e * dim + k] + nn
        S = T0 * nn + t * dd * (2.0 * sgn) + t * t
        rS = _sqrt(S)
        yp = 1.0 / (rS / (t * t) + lap[:, e] * gamma)
        yo = yobs[:, e]
        if arm:
            a, b = _sqrt(yp), _sqrt(yo)
            dfy = (1.0 / b - b / (a * a)) / (a * 2.0)
        else:
            dfy = 1.0 / yo - yo / (yp * yp)
        gQ = -(dfy * yp * yp * scale)
        gS = gQ / (rS * t * t * 2.0)
        gt = gQ * (-(rS * 2.0 / (t * t * t))) + gS * (dd * (2.0 * sgn) + t * 2.0) + gt
        for k in range(dim):
            gd.append(gS * (T0 * dtau[:, e * dim + k] * 2.0 + t * D[:, k] * (2.0 * sgn)))
        gl.append(gQ * gamma)
    return gt, _stack(gd, 1), _stack(gl, 1)


def head_loss(v, w4, b4, xp, yobs, dim, gamma, arm):
    """pntf_tt_head_loss forward: v (3 + 2 dim, n, 128) -> diff (n) (+ S, Ypred lists)."""
    t, dtau, lap, _ = head(v, w4, b4, dim, 1)
    return loss(t, dtau, lap, xp, yobs, dim, gamma, arm)


def head_loss_bwd(v, w4, b4, xp, yobs, dim, gamma, scale, arm, cnt=None):
    """Hand adjoint of scale·Σ head_loss (bound forms of gv, gw4, gb4)."""
    t, dtau, lap, _ = head(v, w4, b4, dim, 1)
    gt, gd, gl = loss_bwd(t, dtau, lap, xp, yobs, dim, gamma, scale, arm)
    return head_vjp(v, w4, b4, dim, 1, gt, gd, gl, cnt)


# ------------------------------------------------------------------ autograd adjoints


def vjp(fn, inputs, ups):
    """Σ_k <ups_k, fn(*inputs)_k> differentiated by torch.autograd w.r.t. every input: the
    reference adjoints.  fn returns a tensor or a tuple; ups None entries are skipped."""
    xs = [x.detach().clone().requires_grad_(True) for x in inputs]
    out = fn(*xs)
    out = out if isinstance(out, (tuple, list)) else (out,)
    tot = sum((o * u).sum() for o, u in zip(out, ups) if u is not None and o is not None)
    gs = torch.autograd.grad(tot, xs, allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for x, g in zip(xs, gs)]
