"""Shared by tests/test_resid_reference.py (CPU) and tests/test_gpu_resid_stage.py (GPU): the ctypes form of helm_nm_stage (include/helm.h) with a thin
wrapper around the test hook helm_debug_nm_stage, the extended-precision reference r = q' - A x of the direct solver's residual check with the quantities
its bounds are made of, and the bounds themselves (u = 2^-53; every component of r is a 19-term real sum whose products are rounded once under FMA and twice
without; the bounds do not depend on the order of the sum):

    stored residual   |r - r_ref| <= 24 u S,  S = |q'| + sum_k |c_k| |x_k| in moduli; 28 with the scaled q' (one more complex multiply); S = 0: exact
    Uout              |U - conj(oscale x)| <= 4 u |oscale| |x|; the same bits when oscale = 1
    rr, r stored      |rr - sum |r_stored|^2| <= (2 N + 8) u rr      (r_stored: what came back, summed in extended precision)
    rr, r not stored  |sqrt(rr) - ||r_ref||_2| <= ||24 u S||_2 + (N + 4) u ||r_ref||_2
    qq                relative (2 N + 8) u, + 8 u when q is scaled
    PREP              Qt within 4 u (|premul| |rhs| + |sub|); the same bits when premul = 1 and there is no sub

A comes from the oracle (oracle.helm_oracle.coefficients_to_csr): the order of the planes is the oracle's, not re-derived from the kernel."""
import ctypes
import functools

import numpy as np

from oracle import helm_oracle as ho
from tests.zgemm_shapes import U, crand, have_x87  # noqa: F401  (have_x87: the tests skip without the 80-bit format)

LD, CLD = np.longdouble, np.clongdouble
RESID, PREP, PACK, SCATTER_ADD, RECOVER_X, TRANSPOSE_OUT, TRANSPOSE = range(7)
HELM_ERR_ARG, HELM_ERR_DEVICE, HELM_ERR_STATE = -1, -2, -3
SENT = complex(-1.2345e300, 6.789e-300)
NAN = complex(np.nan, np.nan)

GRIDS = [(1, 1), (3, 3), (4, 32), (5, 33), (3, 31), (9, 70), (33, 65), (2, 200), (130, 3)]
NCOLS = [1, 63, 64, 65, 127, 128, 129, 200, 256, 257, 300, 513]
OSCALES = (1 + 0j, 0.3 - 1.7j)


class NmStage(ctypes.Structure):
    'helm_nm_stage of include/helm.h'
    _fields_ = [('device', ctypes.c_int), ('stage', ctypes.c_int), ('nz', ctypes.c_int), ('nx', ctypes.c_int), ('N', ctypes.c_longlong),
                ('ncol', ctypes.c_int), ('nblk_cap', ctypes.c_int),
                ('planes', ctypes.c_void_p), ('planes_len', ctypes.c_longlong),
                ('Xin', ctypes.c_void_p), ('xin_len', ctypes.c_longlong), ('ldin', ctypes.c_int),
                ('Q', ctypes.c_void_p), ('q_len', ctypes.c_longlong), ('ldq', ctypes.c_int),
                ('qmap', ctypes.c_void_p),
                ('store', ctypes.c_int), ('qnorm', ctypes.c_int), ('xin_is_u', ctypes.c_int), ('conj', ctypes.c_int),
                ('Rout', ctypes.c_void_p), ('rout_len', ctypes.c_longlong),
                ('Uout', ctypes.c_void_p), ('uout_len', ctypes.c_longlong), ('ldu', ctypes.c_int),
                ('oscale', ctypes.c_double * 2), ('qmask', ctypes.c_void_p),
                ('rhs_ld', ctypes.c_longlong), ('row_off', ctypes.c_longlong),
                ('rr', ctypes.c_void_p), ('qq', ctypes.c_void_p), ('report', ctypes.c_int * 5)]


_BUFS = {'planes': 'planes_len', 'Xin': 'xin_len', 'Q': 'q_len', 'Rout': 'rout_len', 'Uout': 'uout_len'}


def nm_stage(lib, stage, nz=8, nx=8, ncol=1, **f):
    """helm_debug_nm_stage.  Complex buffers are flat complex128 arrays (updated in place where the stage writes), qmap int32, qmask uint8; a length the
    caller does not give is the array's.  Returns (rc, report, rr, qq)."""
    p = NmStage()
    p.device, p.stage, p.nz, p.nx, p.ncol = f.pop('device', 0), stage, nz, nx, ncol
    keep = []
    for name, ln in _BUFS.items():
        a = f.pop(name, None)
        assert a is None or (a.dtype == np.complex128 and a.flags.c_contiguous and a.ndim == 1), name
        setattr(p, name, a.ctypes.data_as(ctypes.c_void_p) if a is not None else None)
        setattr(p, ln, f.pop(ln, a.size if a is not None else 0))
        keep.append(a)
    for name, dt in (('qmap', np.int32), ('qmask', np.uint8)):
        a = f.pop(name, None)
        assert a is None or (a.dtype == dt and a.flags.c_contiguous), name
        setattr(p, name, a.ctypes.data_as(ctypes.c_void_p) if a is not None else None)
        keep.append(a)
    osc = complex(f.pop('oscale', 1 + 0j))
    p.oscale[0], p.oscale[1] = osc.real, osc.imag
    rr, qq = np.full(max(ncol, 1), np.nan), np.full(max(ncol, 1), np.nan)
    p.rr = None if f.pop('no_rr', False) else rr.ctypes.data_as(ctypes.c_void_p)
    p.qq = None if f.pop('no_qq', False) else qq.ctypes.data_as(ctypes.c_void_p)
    for name in ('N', 'nblk_cap', 'ldin', 'ldq', 'ldu', 'store', 'qnorm', 'xin_is_u', 'conj', 'rhs_ld', 'row_off'):
        setattr(p, name, f.pop(name, 0))
    assert not f, 'unknown fields %s' % sorted(f)
    rc = lib.helm_debug_nm_stage(ctypes.byref(p))
    return rc, tuple(p.report), rr, qq


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------------
def planes_of(kind, nz, nx):
    """nine coefficient planes (9, nz, nx): 'mz' / 'eurus' from the oracle on a random model with an absorbing layer (coefficient magnitudes vary over the
    grid; boundary rows are identity rows), 'random': every entry random with a random binary exponent, the entries that point outside the grid included
    (the kernel must multiply them by zero, not by a wrapped neighbour)"""
    rng = np.random.default_rng(nz * 1000 + nx)
    if kind == 'random':
        return crand(rng, 9, nz, nx) * np.ldexp(1.0, rng.integers(-8, 9, size=(9, nz, nx)))
    c = 1500.0 + 2000.0 * rng.random((nz, nx))
    rho = 1000.0 + 1500.0 * rng.random((nz, nx))
    npml = 3 if min(nz, nx) >= 7 else 2
    if kind == 'mz':
        return ho.minizephyr_coefficients(nz, nx, c, rho, 9.0, dx=12.0, dz=10.0, nPML=npml)
    assert kind == 'eurus'
    return np.ascontiguousarray(ho.eurus_coefficients(nz, nx, c, rho, 9.0, dx=12.0, dz=10.0, nPML=npml, theta=0.3, eps=0.2, delta=0.1)[0])


def kind_for(nz, nx, i=0):
    """the oracle's discretisations where the grid has an interior for them to differ from the identity in, random planes otherwise and every third time"""
    if min(nz, nx) < 4 or i % 3 == 2:
        return 'random'
    return ('mz', 'eurus')[i % 3]


@functools.lru_cache(maxsize=None)
def operands(kind, nz, nx, ncol, regime):
    """(C, x, q): x random of mixed magnitude per column; regime 'random': q independent of x, the residual is O(1), a dropped tap or a wrong column is O(1)
    against a bound near 1e-15; 'cancel': q = fl(A x), the residual cancels to rounding and only the componentwise bound means anything"""
    C = planes_of(kind, nz, nx)
    rng = np.random.default_rng((nz * 131 + nx) * 1000 + ncol)
    N = nz * nx
    x = crand(rng, N, ncol) * np.ldexp(1.0, rng.integers(-6, 7, size=(1, ncol)))
    if regime == 'cancel':
        q = ho.stencil_apply(C, x)
    else:
        assert regime == 'random'
        q = crand(rng, N, ncol) * np.ldexp(1.0, rng.integers(-6, 7, size=(1, ncol)))
    for a in (C, x, q):
        a.setflags(write=False)
    return C, x, q


# ---- extended-precision reference ------------------------------------------------------------------------------------------------------------------------
def csr_apply(A, data, X):
    """A X for the sparsity of the CSR matrix A with `data` in the place of its entries, in the (extended) type of data and X: one slot of the rows per pass"""
    Y = np.zeros((A.shape[0],) + X.shape[1:], dtype=np.result_type(data, X))
    cnt = np.diff(A.indptr)
    for k in range(int(cnt.max()) if cnt.size else 0):
        rows = np.flatnonzero(cnt > k)
        e = A.indptr[rows] + k
        Y[rows] += data[e][:, None] * X[A.indices[e]]
    return Y


class Ref(object):
    """r_ref = q' - A x in numpy.clongdouble and what the bounds need.  xin: the array the launch reads (u = conj(oscale x) when xin_is_u: then x = conj(u) and
    q' = oscale q unless oscale = 1); qkeep: boolean (N, ncol), q taken as zero where it is False (sparse right-hand sides)"""

    def __init__(self, C, xin, q, oscale=1 + 0j, xin_is_u=False, qkeep=None):
        A = ho.coefficients_to_csr(C)
        self.N, self.ncol = xin.shape
        self.oscale = complex(oscale)
        self.scaled = bool(xin_is_u) and self.oscale != 1
        self.const = 28 if self.scaled else 24
        self.x = (np.conj(xin) if xin_is_u else xin).astype(CLD)
        qe = q if qkeep is None else np.where(qkeep, q, 0)
        self.qp = CLD(self.oscale) * qe.astype(CLD) if self.scaled else qe.astype(CLD)
        self.r = self.qp - csr_apply(A, A.data.astype(CLD), self.x)
        self.S = np.abs(self.qp) + csr_apply(A, np.abs(A.data.astype(CLD)), np.abs(self.x))


def ratio(err, bound):
    """max |err| / bound; an element whose bound is zero must be exact; NaN or inf anywhere gives inf"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if not np.all(np.isfinite(err)):
        return np.inf
    if np.any(err[bound == 0] != 0):
        return np.inf
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ratio_stored(r, ref):
    return ratio(np.abs(r.astype(CLD) - ref.r), ref.const * U * ref.S)


def ratio_uout(u, ref, oscale):
    want = np.conj(CLD(complex(oscale)) * ref.x)
    if complex(oscale) == 1:
        return 0.0 if same_bits(u, want.astype(np.complex128)) else np.inf
    return ratio(np.abs(u.astype(CLD) - want), 4 * U * abs(complex(oscale)) * np.abs(ref.x))


def ratio_rr_stored(rr, r):
    s = (np.abs(r.astype(CLD)) ** 2).sum(axis=0)
    return ratio(np.abs(rr.astype(LD) - s), (2 * r.shape[0] + 8) * U * rr.astype(LD))


def ratio_rr_norms(rr, ref):
    if not np.all(rr >= 0):
        return np.inf
    nr = np.sqrt((np.abs(ref.r) ** 2).sum(axis=0))
    nb = np.sqrt(((ref.const * U * ref.S) ** 2).sum(axis=0))
    return ratio(np.abs(np.sqrt(rr.astype(LD)) - nr), nb + (ref.N + 4) * U * nr)


def ratio_qq(qq, ref):
    s = (np.abs(ref.qp) ** 2).sum(axis=0)
    return ratio(np.abs(qq.astype(LD) - s), (2 * ref.N + 8 + (8 if ref.scaled else 0)) * U * s)


def ratio_prep(Qt, rhs_win, premul, sub):
    """Qt (N, nrhs) against premul * rhs_win[r][i] - sub[r][i]; rhs_win, sub: (nrhs, N)"""
    premul = complex(premul)
    if premul == 1 and sub is None:
        return 0.0 if same_bits(Qt, rhs_win.T) else np.inf
    want = CLD(premul) * rhs_win.astype(CLD)
    bound = abs(premul) * np.abs(rhs_win).astype(LD)
    if sub is not None:
        want, bound = want - sub.astype(CLD), bound + np.abs(sub)
    return ratio(np.abs(Qt.astype(CLD) - want.T), 4 * U * bound.T)


# ---- a plain complex128 evaluation (what a correct fp64 kernel computes, without FMA) ------------------------------------------------------------------------
def resid_fp64(C, xin, q, oscale=1 + 0j, xin_is_u=False, qkeep=None, order=range(9), sequential=False):
    """(r, rr, qq, U) in complex128 / float64: the taps added in `order`, the norms by numpy's pairwise sum or one after the other"""
    _, nz, nx = C.shape
    oscale = complex(oscale)
    x = np.conj(xin) if xin_is_u else xin
    qe = q if qkeep is None else np.where(qkeep, q, 0)
    qp = oscale * qe if (xin_is_u and oscale != 1) else qe.copy()
    r = qp.reshape(nz, nx, -1).copy()
    X = x.reshape(nz, nx, -1)
    for k in order:
        sz, sx = ho.SLOT_OFFSETS[k]
        z0, z1, x0, x1 = max(0, -sz), nz - max(0, sz), max(0, -sx), nx - max(0, sx)
        r[z0:z1, x0:x1] -= C[k][z0:z1, x0:x1, None] * X[z0 + sz:z1 + sz, x0 + sx:x1 + sx]
    r = r.reshape(xin.shape)
    total = (lambda a: np.cumsum(a, axis=0)[-1]) if sequential else (lambda a: a.sum(axis=0))
    a2 = lambda a: a.real * a.real + a.imag * a.imag
    return r, total(a2(r)), total(a2(qp)), np.conj(oscale * x)
