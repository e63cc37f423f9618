"""Shared by tests/test_mg_reference_host.py (CPU) and tests/test_gpu_mg_stage.py (GPU): the ctypes form of helm_mg_stage (include/helm.h) with a thin wrapper
around the test hook helm_debug_mg_stage, the cases, and a plain-numpy reference of the 2-D multigrid preconditioner of zephyr_amd/csrc/mg.hip written from
the formulas, generic over the number type: numpy.clongdouble ('exact', x87: 64-bit significand) or complex128 ('double': every stored vector rounded to
double, sums one term after the other in the order the kernels add them, without fused multiply-adds).  Nothing here touches a GPU.

    damped Jacobi from zero     u = omega_j dinv (.) f;  a sweep: u <- u + omega_j dinv (.) (f - A u)
    full weighting              fc[I, J] = sum_{di, dj} w(di) w(dj) r[2 I + di, 2 J + dj], w = (1, 2, 1) / 4, fine points outside the grid skipped
    bilinear prolongation       even points copy, odd points average their two (four) coarse neighbours, points beyond the coarse grid contribute zero
    nine-point stencil          (A x)[i] = sum_k C[k][i] x[i + off_k], k = oracle.helm_oracle.slot(dz, dx), neighbours outside the grid dropped
    dense coarse solve          u = invT^T f with the inverse it is handed
    strip lines                 Thomas elimination of the tridiagonal systems along z on the columns ix < W, ix >= nx - W (all iz), and along x on the rows
                                iz < W, iz >= nz - W (W <= ix < nx - W); u += wstrip T^-1 r, every line from the same r
    cycle                       u = jac0(f); nu1 - 1 sweeps; e = cycle(l + 1, restrict(f - A u)); with fmode, on levels l < fdepth whose coarse level is not
                                the last: e += V-cycle(l + 1, fc - A_c e); u += prolong(e); nu2 sweeps.  Last level: the dense solve.
    M^-1                        out = cycle(0, in, fdepth > 0); `sweeps` times: r = in - A_strip out, out += wstrip T^-1 r on the lines

Tolerances.  A stage with a short, fixed operation count has a counted bound (gamma_n = n u / (1 - n u), u = 2^-53, on moduli or per component as said at each
function).  Everything else: the stage is evaluated twice on the CPU, d = max |double - exact| per column, and the device is asked to lie within
MARGIN max(d, 64 u scale) of the exact result, scale = max |exact| of the column, MARGIN = 16 (the rule of tests/krylov_cases.py): d never comes from the device."""
import ctypes
import functools

import numpy as np

from oracle import helm_oracle as ho

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
MARGIN = 16.0
SENT = complex(-1.2345e300, 6.789e-300)
HELM_ERR_ARG, HELM_ERR_DEVICE, HELM_ERR_STATE = -1, -2, -3
JAC0, AXPY1, RESTRICT, PROLONG_ADD, COARSE_DENSE, LINE_FACTOR, LINE_SOLVE, LEVELS, PLANES, STRIP_RESID, CYCLE, APPLY = range(12)
MAX_LEVELS = 16


def have_x87():
    return np.finfo(np.longdouble).nmant >= 63


def gamma(n):
    return n * U / (1 - n * U)


# ---- the hook ----------------------------------------------------------------------------------------------------------------------------------------
class MgStage(ctypes.Structure):
    'helm_mg_stage of include/helm.h'
    _fields_ = [('device', ctypes.c_int), ('stage', ctypes.c_int), ('nz', ctypes.c_int), ('nx', ctypes.c_int), ('nrhs', ctypes.c_int), ('W', ctypes.c_int),
                ('op', ctypes.c_void_p), ('omega_j', ctypes.c_double), ('wstrip', ctypes.c_double), ('active', ctypes.c_void_p),
                ('x', ctypes.c_void_p), ('x_len', ctypes.c_longlong), ('y', ctypes.c_void_p), ('y_len', ctypes.c_longlong),
                ('m', ctypes.c_void_p), ('m_len', ctypes.c_longlong), ('r', ctypes.c_void_p), ('r_len', ctypes.c_longlong),
                ('zl', ctypes.c_void_p * 3), ('xl', ctypes.c_void_p * 3), ('zl_len', ctypes.c_longlong), ('xl_len', ctypes.c_longlong),
                ('cinvT', ctypes.c_void_p), ('cinvT_len', ctypes.c_longlong),
                ('level', ctypes.c_int), ('fmode', ctypes.c_int), ('nu1', ctypes.c_int), ('nu2', ctypes.c_int), ('fdepth', ctypes.c_int), ('sweeps', ctypes.c_int),
                ('nlevels', ctypes.c_int), ('lev_nz', ctypes.c_int * MAX_LEVELS), ('lev_nx', ctypes.c_int * MAX_LEVELS), ('lev_npml', ctypes.c_int * MAX_LEVELS),
                ('lev_dx', ctypes.c_double * MAX_LEVELS), ('lev_dz', ctypes.c_double * MAX_LEVELS),
                ('o_W', ctypes.c_int), ('o_sweeps', ctypes.c_int), ('o_nu1', ctypes.c_int), ('o_nu2', ctypes.c_int), ('o_fdepth', ctypes.c_int),
                ('o_nc', ctypes.c_int), ('o_ntiles', ctypes.c_int), ('o_tile_rows', ctypes.c_int),
                ('o_omega_j', ctypes.c_double), ('o_wstrip', ctypes.c_double), ('o_beta', ctypes.c_double), ('o_tau', ctypes.c_double), ('o_cpml', ctypes.c_double),
                ('tiles', ctypes.c_void_p), ('tiles_cap', ctypes.c_longlong)]


_VECS = {'x': 'x_len', 'y': 'y_len', 'm': 'm_len', 'r': 'r_len', 'cinvT': 'cinvT_len'}


def mg_stage(lib, stage, **f):
    """helm_debug_mg_stage.  Complex buffers are flat complex128 arrays (updated in place where the stage writes); `active` uint8; zl / xl lists of three flat
    arrays; a length the caller does not give is the array's.  Returns (rc, the structure)."""
    p = MgStage()
    p.stage, p.device = stage, f.pop('device', 0)
    keep = []
    for name, ln in _VECS.items():
        a = f.pop(name, None)
        assert a is None or (a.dtype == np.complex128 and a.flags.c_contiguous and a.ndim == 1), name
        setattr(p, name, a.ctypes.data_as(ctypes.c_void_p) if a is not None else None)
        setattr(p, ln, f.pop(ln, a.size if a is not None else 0))
        keep.append(a)
    for name in ('zl', 'xl'):
        arrs = f.pop(name, None)
        setattr(p, name + '_len', f.pop(name + '_len', arrs[0].size if arrs is not None else 0))
        for i in range(3):
            a = arrs[i] if arrs is not None else None
            assert a is None or (a.dtype == np.complex128 and a.flags.c_contiguous and a.ndim == 1), name
            getattr(p, name)[i] = a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        keep.append(arrs)
    act = f.pop('active', None)
    if act is not None:
        act = np.ascontiguousarray(act, dtype=np.uint8)
        p.active = act.ctypes.data_as(ctypes.c_void_p)
    tiles = f.pop('tiles', None)
    if tiles is not None:
        assert tiles.dtype == np.int32 and tiles.flags.c_contiguous
        p.tiles, p.tiles_cap = tiles.ctypes.data_as(ctypes.c_void_p), f.pop('tiles_cap', tiles.size)
    p.op = f.pop('op', None)
    for name in ('nu1', 'nu2', 'fdepth', 'sweeps'):
        setattr(p, name, f.pop(name, -1))
    for name in ('nz', 'nx', 'nrhs', 'W', 'level', 'fmode'):
        setattr(p, name, f.pop(name, 0))
    p.omega_j, p.wstrip = f.pop('omega_j', 0.0), f.pop('wstrip', 0.0)
    assert not f, 'unknown fields %s' % sorted(f)
    rc = lib.helm_debug_mg_stage(ctypes.byref(p))
    del keep, act
    return rc, p


# ---- number types --------------------------------------------------------------------------------------------------------------------------------------
def cast(a, dtype):
    return np.asarray(a).astype(dtype)


def real_of(dtype):
    return LD if dtype == CLD else np.float64


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- transfers ---------------------------------------------------------------------------------------------------------------------------------------------
def coarse_dims(nzf, nxf):
    return (nzf + 1) // 2, (nxf + 1) // 2


def restrict(r, mutant=None):
    """full weighting of r (ncol, nzf, nxf), in r's type: the nine terms added di = -1, 0, 1 outside, dj inside.  The weights are powers of two, so every product
    is exact and the eight additions give  |fc - exact| <= gamma_8 R|r|  per real component (R|.|: the same weighting of the absolute values)."""
    n, nzf, nxf = r.shape
    nzc, nxc = coarse_dims(nzf, nxf)
    pad = np.zeros((n, 2 * nzc + 1, 2 * nxc + 1), dtype=r.dtype)
    pad[:, 1:nzf + 1, 1:nxf + 1] = r
    out = np.zeros((n, nzc, nxc), dtype=r.dtype)
    rt = real_of(r.dtype) if np.iscomplexobj(r) else r.dtype.type
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            w = rt((2.0 if di == 0 else 1.0) * (2.0 if dj == 0 else 1.0) / 16.0)
            term = w * pad[:, 1 + di:1 + di + 2 * nzc:2, 1 + dj:1 + dj + 2 * nxc:2]
            if mutant == 'restrict_edge' and di == -1:
                term[:, 0] = w * pad[:, 2:3, 1 + dj:1 + dj + 2 * nxc:2][:, 0]          # the row above the grid mirrored in, not skipped
            out = out + term
    return out


def prolong_1d(nf, nc, rt, mutant=None):
    "the (nf, nc) matrix of linear interpolation along one axis: even points copy, odd points average, a coarse point beyond the grid contributes zero"
    P = np.zeros((nf, nc), dtype=rt)
    for i in range(nf):
        I = i // 2
        if i % 2 == 0:
            P[i, I] = 1
        else:
            P[i, I] = 0.5
            if I + 1 < nc and not (mutant == 'prolong_drop' and i >= nf - 2):
                P[i, I + 1] = 0.5
    return P


def prolong(e, nzf, nxf, mutant=None):
    """bilinear prolongation of e (ncol, nzc, nxc) to (ncol, nzf, nxf) in e's type.  Weights are powers of two; a fine point adds at most four exact products
    (three additions), whatever the order:  |P e - exact| <= gamma_3 P|e|  per real component."""
    rt = real_of(e.dtype) if np.iscomplexobj(e) else e.dtype.type
    n, nzc, nxc = e.shape
    Pz, Px = prolong_1d(nzf, nzc, rt, mutant), prolong_1d(nxf, nxc, rt)
    out = np.zeros((n, nzf, nxf), dtype=e.dtype)
    # the four terms in the order (I, J), (I, J + 1), (I + 1, J), (I + 1, J + 1)
    zi, xi = np.arange(nzf) // 2, np.arange(nxf) // 2
    for dI in (0, 1):
        wz = Pz[np.arange(nzf), np.minimum(zi + dI, nzc - 1)] * ((zi + dI < nzc) if dI else 1)
        for dJ in (0, 1):
            wx = Px[np.arange(nxf), np.minimum(xi + dJ, nxc - 1)] * ((xi + dJ < nxc) if dJ else 1)
            if dI:
                wz = np.where(np.arange(nzf) % 2 == 1, wz, 0)
            if dJ:
                wx = np.where(np.arange(nxf) % 2 == 1, wx, 0)
            src = e[:, np.minimum(zi + dI, nzc - 1)][:, :, np.minimum(xi + dJ, nxc - 1)]
            out = out + (wz[:, None] * wx[None, :]).astype(rt)[None] * src
    return out


# ---- stencil -------------------------------------------------------------------------------------------------------------------------------------------------
def stencil(C, X):
    "A X for planes C (9, nz, nx) and X (ncol, nz, nx) of one type, the planes added in the order of oracle.helm_oracle.slot"
    _, nz, nx = C.shape
    Y = np.zeros_like(X)
    for dz in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = ho.slot(dz, dx)
            z0, z1, x0, x1 = max(0, -dz), nz - max(0, dz), max(0, -dx), nx - max(0, dx)
            Y[:, z0:z1, x0:x1] += C[k][None, z0:z1, x0:x1] * X[:, z0 + dz:z1 + dz, x0 + dx:x1 + dx]
    return Y


def dinv_floored(C, frac, dtype=CLD):
    """what k_scale_planes leaves as dinv: 1 / d, d the centre plane, scaled up to frac times the row's absolute sum where it is smaller (phase kept); zero where the
    centre is zero"""
    C = cast(C, dtype)
    d = C[4].copy()
    rows = np.abs(C).sum(axis=0)
    ad = np.abs(d)
    small = (ad < frac * rows) & (ad > 0)
    d[small] = d[small] * (frac * rows[small] / ad[small])
    out = np.zeros_like(d)
    nzr = ad > 0
    out[nzr] = 1 / d[nzr]
    return out


# ---- strip lines ---------------------------------------------------------------------------------------------------------------------------------------------
def line_systems(C, W):
    """the tridiagonal systems of the strip: ((az, bz, cz), (ax, bx, cx)), each (2 W, len) in C's type; z-lines of length nz on the columns [0, W) u [nx - W, nx),
    x-lines of length nx - 2 W on the rows [0, W) u [nz - W, nz).  The first sub- and the last super-diagonal entry are zero (no neighbour on the line)."""
    _, nz, nx = C.shape
    cols = np.r_[0:W, nx - W:nx]
    rows = np.r_[0:W, nz - W:nz]
    z = [C[ho.slot(d, 0)][:, cols].T.copy() for d in (-1, 0, 1)]
    x = [C[ho.slot(0, d)][rows][:, W:nx - W].copy() for d in (-1, 0, 1)]
    for a, b, c in (z, x):
        a[:, 0] = 0
        c[:, -1] = 0
    return tuple(z), tuple(x)


def thomas_factors(a, b, c):
    "(m, cp, af): m_i = 1 / (b_i - a_i cp_{i-1}), cp_i = c_i m_i, af_i = -a_i m_i, along the last axis"
    m, cp, af = np.empty_like(b), np.empty_like(b), np.empty_like(b)
    prev = np.zeros_like(b[..., 0])
    for i in range(b.shape[-1]):
        m[..., i] = 1 / (b[..., i] - a[..., i] * prev)
        prev = c[..., i] * m[..., i]
        cp[..., i] = prev
        af[..., i] = -(a[..., i] * m[..., i])
    return m, cp, af


def thomas(a, b, c, d, mutant=None):
    """x with T x = d by Thomas elimination; a, b, c (L, len), d (ncol, L, len), one type.  Forward: cp_i = c_i / den_i, y_i = (d_i - a_i y_{i-1}) / den_i,
    den_i = b_i - a_i cp_{i-1}; backward: x_i = y_i - cp_i x_{i+1}."""
    n = b.shape[-1]
    m, cp, _ = thomas_factors(a, b, c)
    y = np.empty_like(d)
    prev = np.zeros_like(d[..., 0])
    for i in range(n):
        if mutant == 'carry_1024' and i == 1024:
            prev = np.zeros_like(prev)
        prev = (d[..., i] - a[None, :, i] * prev) * m[None, :, i]
        y[..., i] = prev
    x = np.empty_like(d)
    nxt = np.zeros_like(prev)
    for i in range(n - 1, -1, -1):
        if mutant == 'carry_1024' and i == 1023:
            nxt = np.zeros_like(nxt)
        nxt = y[..., i] - cp[None, :, i] * nxt
        x[..., i] = nxt
    return x


def line_relax(C, W, r, u, wstrip, mutant=None):
    "u + wstrip T^-1 r on every strip line (a new array; r, u (ncol, nz, nx) of C's type)"
    _, nz, nx = C.shape
    (az, bz, cz), (ax, bx, cx) = line_systems(C, W)
    cols = np.r_[0:W, nx - W:nx]
    rows = np.r_[0:W, nz - W:nz]
    out = u.copy()
    rt = real_of(u.dtype)
    xz = thomas(az, bz, cz, np.swapaxes(r[:, :, cols], 1, 2), mutant)               # (ncol, 2 W, nz)
    out[:, :, cols] += rt(wstrip) * np.swapaxes(xz, 1, 2)
    xx = thomas(ax, bx, cx, r[:, rows, W:nx - W], mutant)
    out[:, rows, W:nx - W] += rt(wstrip) * xx
    return out


def on_lines(nz, nx, W):
    "boolean (nz, nx): the points the strip lines cover"
    m = np.zeros((nz, nx), dtype=bool)
    m[:, :W] = m[:, nx - W:] = True
    m[:W, W:nx - W] = m[nz - W:, W:nx - W] = True
    return m


# ---- the hierarchy -----------------------------------------------------------------------------------------------------------------------------------------
def level_rules(nz, nx, dx, dz, npml, min_n=16):
    "the grids of mg_setup: [(nz, nx, dx, dz, npml)], halving with (n + 1) / 2, spacing doubled, npml_c = max((npml - 1) / 2 + 1, 2), and its stopping rule"
    out = []
    while True:
        out.append((nz, nx, dx, dz, npml))
        nzc, nxc = coarse_dims(nz, nx)
        npc = max((npml - 1) // 2 + 1, 2)
        if min(nz, nx) <= min_n or nzc < 2 * npc + 3 or nxc < 2 * npc + 3 or nz * nx <= 64:
            return out
        nz, nx, dx, dz, npml = nzc, nxc, 2 * dx, 2 * dz, npc


def inject(a):
    return np.ascontiguousarray(a[::2, ::2])


def dense_of(C):
    "the matrix of nine planes (9, nz, nx), dense complex128"
    return ho.coefficients_to_csr(np.asarray(C, dtype=np.complex128)).toarray()


class Hier(object):
    """the preconditioner on planes it is handed, in one number type.  levels: [(C (9, nz, nx), dinv (nz, nx))]; cinvT (nc, nc): the dense inverse of the last
    level, transposed; strip: the strip operator's planes or None; par: W, sweeps, nu1, nu2, fdepth, omega_j, wstrip.  All inputs complex128, upcast exactly."""

    def __init__(self, levels, cinvT, strip, par, dtype, mutant=None):
        self.dtype, self.mutant, self.par = dtype, mutant, dict(par)
        self.C = [cast(C, dtype) for C, _ in levels]
        self.dinv = [cast(d, dtype) for _, d in levels]
        self.cinvT = cast(cinvT, dtype)
        self.strip = cast(strip, dtype) if strip is not None else None
        self.dims = [C.shape[1:] for C, _ in levels]

    def with_par(self, **kw):
        h = Hier.__new__(Hier)
        h.__dict__.update(self.__dict__)
        h.par = dict(self.par, **{k: v for k, v in kw.items() if v is not None and v >= 0})
        return h

    def coarse(self, F):
        n = F.shape[0]
        f = F.reshape(n, -1)
        if self.dtype == CLD:
            u = f @ self.cinvT
        else:               # one term after the other, as a lane of k_coarse_dense adds them
            u = np.stack([np.cumsum(self.cinvT * f[j][:, None], axis=0)[-1] for j in range(n)])
        return u.reshape(F.shape)

    def sweep(self, l, u, f):
        om = real_of(self.dtype)(self.par['omega_j'])
        w = om * self.dinv[l]
        if self.mutant == 'omega_twice':
            w = om * w
        return u + w[None] * (f - stencil(self.C[l], u))

    def cycle(self, l, F, fmode):
        "u = vcycle(l, F); F (ncol, nz_l, nx_l)"
        F = cast(F, self.dtype)
        last = len(self.C) - 1
        if l == last:
            return self.coarse(F)
        om = real_of(self.dtype)(self.par['omega_j'])
        u = (om * self.dinv[l])[None] * F
        for _ in range(self.par['nu1'] - 1):
            u = self.sweep(l, u, F)
        r = F - stencil(self.C[l], u)
        fc = restrict(r)
        e = self.cycle(l + 1, fc, fmode)
        if fmode and l < self.par['fdepth'] and l + 1 < last and self.mutant != 'no_second_visit':
            g = fc - stencil(self.C[l + 1], e)
            e = e + self.cycle(l + 1, g, False)
        u = u + prolong(e, *self.dims[l])
        for _ in range(self.par['nu2']):
            u = self.sweep(l, u, F)
        return u

    def strip_resid(self, IN, OUT):
        return cast(IN, self.dtype) - stencil(self.strip, cast(OUT, self.dtype))

    def apply(self, IN):
        IN = cast(IN, self.dtype)
        out = self.cycle(0, IN, self.par['fdepth'] > 0)
        for _ in range(self.par['sweeps']):
            r = self.strip_resid(IN, out)
            out = line_relax(self.strip, self.par['W'], r, out, self.par['wstrip'])
        return out


# ---- tolerances --------------------------------------------------------------------------------------------------------------------------------------------
def colmax(a):
    a = np.asarray(a)
    return np.abs(a.reshape(a.shape[0], -1)).max(axis=1).astype(LD)


def floor_tol(exact, double):
    "per column: MARGIN max(d, 64 u scale), d = max |double - exact|, scale = max |exact|"
    d = colmax(cast(double, CLD) - exact)
    return MARGIN * np.maximum(d, 64 * U * colmax(exact))


def ratio_cols(dev, exact, tol):
    "max over columns of max |dev - exact| / tol; NaN or inf anywhere gives inf; a column whose tolerance is zero must be exact"
    err = colmax(cast(dev, CLD) - exact)
    if not np.all(np.isfinite(err)):
        return np.inf
    tol = np.asarray(tol, dtype=LD)
    if np.any(err[tol == 0] != 0):
        return np.inf
    nzr = tol > 0
    return float((err[nzr] / tol[nzr]).max()) if nzr.any() else 0.0


def ratio_parts(dev, exact, bound_re, bound_im):
    "max |component error| / its bound over real and imaginary parts; an element whose bound is zero must be exact"
    out = 0.0
    for part, bound in (('real', bound_re), ('imag', bound_im)):
        err = np.abs(getattr(np.asarray(dev), part).astype(LD) - getattr(exact, part))
        bound = np.asarray(bound, dtype=LD)
        if not np.all(np.isfinite(err)) or np.any(err[bound == 0] != 0):
            return np.inf
        nzr = bound > 0
        if nzr.any():
            out = max(out, float((err[nzr] / bound[nzr]).max()))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def restrict_bounds(r):
    "(exact, bound_re, bound_im) of RESTRICT for r (ncol, nzf, nxf) complex128"
    ex = restrict(cast(r, CLD))
    return ex, gamma(8) * restrict(np.abs(r.real).astype(LD)), gamma(8) * restrict(np.abs(r.imag).astype(LD))


def prolong_add_bounds(e, u):
    """(exact, bound_re, bound_im) of PROLONG_ADD: three additions inside P e and the one that adds it to u:  gamma_4 (|u| + P|e|) per component"""
    nzf, nxf = u.shape[1:]
    ex = cast(u, CLD) + prolong(cast(e, CLD), nzf, nxf)
    bre = gamma(4) * (np.abs(u.real).astype(LD) + prolong(np.abs(e.real).astype(LD), nzf, nxf))
    bim = gamma(4) * (np.abs(u.imag).astype(LD) + prolong(np.abs(e.imag).astype(LD), nzf, nxf))
    return ex, bre, bim


def jac0_bounds(dinv, f, omega):
    """(exact, bound_re, bound_im) of JAC0, s = omega dinv rounded once per component, then a complex product of two real products and one sum per component:
    gamma_3 (|s_re f_re| + |s_im f_im|) on the real part, gamma_3 (|s_re f_im| + |s_im f_re|) on the imaginary one"""
    s = LD(omega) * cast(dinv, CLD)
    f = cast(f, CLD)
    ex = s[None] * f
    bre = gamma(3) * (np.abs(s.real[None] * f.real) + np.abs(s.imag[None] * f.imag))
    bim = gamma(3) * (np.abs(s.real[None] * f.imag) + np.abs(s.imag[None] * f.real))
    return ex, bre, bim


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------------------
TRANSFER_GRIDS = [(2, 2), (3, 3), (7, 8), (8, 7), (17, 18), (35, 34), (3, 600)]
COARSE_NCS = [1, 81, 255, 256, 257, 700]
LINE_LENGTHS = [8, 16, 17, 1023, 1024, 1025, 2049, 2100]
LINE_W = 3

# hierarchy cases: kind 'eu' Eurus / 'mz' MiniZephyr; h = (dz, dx)
HIER_CASES = {
    'eu70x67':  dict(kind='eu', dims=(70, 67), h=(10., 10.), nPML=4, freq=12., seed=31),
    'mz67x70':  dict(kind='mz', dims=(67, 70), h=(10., 10.), nPML=4, freq=12., seed=32, freeSurf=(True, False, False, False)),
    'mz70x67T': dict(kind='mz', dims=(70, 67), h=(10., 10.), nPML=4, freq=12., seed=33, transposed=True),
    'eu66x72':  dict(kind='eu', dims=(66, 72), h=(8., 12.), nPML=4, freq=12., seed=34),
    'eu20x40':  dict(kind='eu', dims=(20, 40), h=(10., 10.), nPML=10, freq=12., seed=35),
}
BETA, CPML_WEAK, OMEGA_J, DIAG_FLOOR = 0.6, 30.0, 0.8, 0.5


@functools.lru_cache(maxsize=None)
def hier_model(name):
    "random heterogeneous model of the case: c = (1800 + 2200 rand)(1 + 0.01j), rho = 1000 + 600 rand"
    cs = HIER_CASES[name]
    rng = np.random.default_rng(cs['seed'])
    return dict(c=(1800. + 2200. * rng.random(cs['dims'])) * (1 + 0.01j), rho=1000. + 600. * rng.random(cs['dims']))


def hier_config(name):
    cs, m = HIER_CASES[name], hier_model(name)
    cfg = dict(nz=cs['dims'][0], nx=cs['dims'][1], dz=cs['h'][0], dx=cs['h'][1], freq=cs['freq'], nPML=cs['nPML'], c=m['c'], rho=m['rho'])
    for key in ('freeSurf', 'transposed'):
        if key in cs:
            cfg[key] = cs[key]
    return cfg


def shifted_tau(freq, tau_a=np.inf, beta=BETA):
    "1 / (omega beta / 2 + 1 / tau_A), omega = 2 pi |freq|"
    inv = 2.0 * np.pi * abs(complex(freq)) * beta / 2.0
    if np.isfinite(tau_a) and tau_a != 0:
        inv += 1.0 / tau_a
    return 1.0 / inv


def oracle_level_planes(name, cpml, level=0, tau=None):
    "the oracle's planes (9, nz_l, nx_l) of the case's level: that level's grid, the model injected `level` times, the shifted tau"
    cs, m = HIER_CASES[name], hier_model(name)
    nz, nx, dx, dz, npml = level_rules(cs['dims'][0], cs['dims'][1], cs['h'][1], cs['h'][0], cs['nPML'])[level]
    c, rho = m['c'], m['rho']
    for _ in range(level):
        c, rho = inject(c), inject(rho)
    tau = shifted_tau(cs['freq']) if tau is None else tau
    if cs['kind'] == 'eu':
        return np.ascontiguousarray(ho.eurus_coefficients(nz, nx, c, rho, cs['freq'], dx=dx, dz=dz, tau=tau, nPML=npml, cPML=cpml)[0])
    return ho.minizephyr_coefficients(nz, nx, c, rho, cs['freq'], dx=dx, dz=dz, tau=tau, nPML=npml, freeSurf=cs.get('freeSurf', (False,) * 4))


def solver_par(name):
    cs = HIER_CASES[name]
    W = cs['nPML'] + 2
    off = 2 * W + 2 > min(cs['dims'])
    return dict(W=W, sweeps=0 if off else 4, nu1=1, nu2=1, fdepth=3, omega_j=OMEGA_J, wstrip=1.0)


@functools.lru_cache(maxsize=None)
def oracle_hier_inputs(name):
    "(levels, cinvT, strip planes or None, par) of a case from the CPU oracle alone: what tests/test_mg_reference_host.py evaluates the reference on"
    cs = HIER_CASES[name]
    grids = level_rules(cs['dims'][0], cs['dims'][1], cs['h'][1], cs['h'][0], cs['nPML'])
    levels = []
    for l in range(len(grids)):
        C = oracle_level_planes(name, CPML_WEAK, l)
        levels.append((C, dinv_floored(C, DIAG_FLOOR, np.complex128)))
    cinvT = np.ascontiguousarray(np.linalg.inv(dense_of(levels[-1][0])).T)
    par = solver_par(name)
    strip = oracle_level_planes(name, 1e3, 0) if par['sweeps'] else None
    return levels, cinvT, strip, par


def hier_rhs(name, level_dims, ncol=4, seed=0):
    "ncol complex normal columns on a level's grid and one zero column behind them: (ncol + 1, nz, nx)"
    rng = np.random.default_rng(7000 + HIER_CASES[name]['seed'] + 13 * seed + level_dims[0])
    F = np.zeros((ncol + 1,) + tuple(level_dims), dtype=np.complex128)
    F[:ncol] = crand(rng, ncol, *level_dims)
    return F


def line_planes(kind, nz, nx):
    """nine planes for the free-standing line stages.  'eurus': the oracle's Eurus block 0 on a random model with the default C-PML (cPML = 1e3), the shifted
    damping of a 12 Hz solve and an absorbing layer of LINE_W cells -- the ill-conditioned layer the strip exists for.  'dominant': b = 1, a = c =
    -(1 - 1e-6) / 2 along both axes, every row scaled by a random complex factor of modulus 1/2 .. 2 (couplings decay by 1 - 1.4e-3 per point: what happens at
    point 1024 is felt 1000 points on), the four corner planes random (the lines must not read them)."""
    rng = np.random.default_rng(nz * 7919 + nx)
    if kind == 'eurus':
        c = (1800. + 2200. * rng.random((nz, nx))) * (1 + 0.01j)
        rho = 1000. + 600. * rng.random((nz, nx))
        return np.ascontiguousarray(ho.eurus_coefficients(nz, nx, c, rho, 12.0, dx=10.0, dz=10.0, tau=shifted_tau(12.0), nPML=LINE_W)[0])
    assert kind == 'dominant'
    C = crand(rng, 9, nz, nx)
    s = np.exp(2j * np.pi * rng.random((nz, nx))) * (0.5 + 1.5 * rng.random((nz, nx)))
    C[4] = s
    for k in (1, 3, 5, 7):
        C[k] = -0.5 * (1 - 1e-6) * s
    return C


def line_grids():
    "(nz, nx) of the LINE_SOLVE cases: every length along z at the narrow nx = 2 W + 2, then along x at the narrow nz"
    narrow = 2 * LINE_W + 2
    return [(n, narrow) for n in LINE_LENGTHS] + [(narrow, n + 2 * LINE_W) for n in LINE_LENGTHS]


# ---- operands and references of the free-standing stages (computed once, shared by the tests) ------------------------------------------------------------------
LINE_WSTRIP = 0.75


@functools.lru_cache(maxsize=None)
def line_case(kind, nz, nx, ncol):
    "(C, r, u, exact, tol): operands of LINE_SOLVE with W = LINE_W and the exact result u + wstrip T^-1 r with its per-column tolerance"
    C = line_planes(kind, nz, nx)
    rng = np.random.default_rng(nz * 31 + nx + 1000 * ncol)
    r, u = crand(rng, ncol, nz, nx), crand(rng, ncol, nz, nx)
    ex = line_relax(cast(C, CLD), LINE_W, cast(r, CLD), cast(u, CLD), LINE_WSTRIP)
    db = line_relax(C, LINE_W, r, u, LINE_WSTRIP)
    for a in (C, r, u, ex):
        a.setflags(write=False)
    return C, r, u, ex, floor_tol(ex, db)


def coarse_solve(invT, f, dtype):
    "u = invT^T f for f (ncol, nc): exact, or in double one term after the other"
    h = Hier([(np.zeros((9, 1, 1)), np.zeros((1, 1)))], invT, None, {}, dtype)
    return h.coarse(cast(f, dtype))


@functools.lru_cache(maxsize=None)
def coarse_case(nc, ncol=3):
    "(invT, f, exact, tol) of COARSE_DENSE: a random matrix, random columns"
    rng = np.random.default_rng(500 + nc)
    invT, f = crand(rng, nc, nc), crand(rng, ncol, nc)
    ex = coarse_solve(invT, f, CLD)
    return invT, f, ex, floor_tol(ex, coarse_solve(invT, f, np.complex128))
