"""Shared by tests/test_gaussnewton_host.py (CPU) and tests/test_gpu_gaussnewton.py (GPU): the exact diagonal of the Gauss-Newton
Hessian (illumination(kind='gaussNewton')), the small survey it is checked on cell by cell, its brute force, the 80-bit evaluations of the two device kernels
and the componentwise bounds they are held to.

The bounds.  u = 2^-53.

  k_lag_gram             per column and lag one complex FMA, two roundings per component; the sum over nsrc columns is in LG_WAVES = 4 register chains that are
                         then added in wave order (4 more), and one addition into C: the count of density_cases.c_lag.           c_gram = 2 nsrc + 4 + 1
                         The bound is c_gram u m, m = |C0| + sum_s |u_s[i]| |u_s[i + off]| (the `magnitude` evaluation of frechet.lagGram; either component of
                         a complex product is at most the product of the moduli).  A complex64 store adds C64 2^-24 (m - |C0|): both factors of every
                         product are within 2^-24 relative of the packed ones, (2 + 2^-24) 2^-24 per product, the term of pseudohessian_cases.
  k_gauss_newton_diagonal  a coefficient is within C_COEF u of its magnitude evaluation (pseudohessian_cases: 71), three of them enter a term, and so do two
                         plane entries that are exact inputs.  T = E Phi: at most nine complex FMAs per entry (18); S = Gamma T: nine more (18); the sum of
                         conj(E) S over the 33 coefficients (2 each, 66) -- each relative to the running sum of moduli, which the magnitude evaluation
                         (every factor by its modulus) bounds.  The end: alpha W (1), the product (1), the addition to H0 (1).
                                                                                                       C_GN = 3 C_COEF + 18 + 18 + 66 + 3
                         The bound is C_GN u (|H0| + alpha W M), M the `magnitude` evaluation of frechet.gaussNewtonDiagonal on the moduli of the planes.
"""
import numpy as np

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import pseudohessian_cases as pc
from zephyr_amd import frechet as fr

LD, CLD, U64 = fc.LD, fc.CLD, fc.U64
C64 = pc.C64
C_GN = 3 * pc.C_COEF + 18 + 18 + 66 + 3
c_gram = dc.c_lag

# ---- the small survey: every cell is compared ---------------------------------------------------------------------------------------------------------
SNZ, SNX, SNPML, SDX = 13, 17, 3, 12.5
SNSRC, SNREC = 3, 4
# the variants of the definition test: name -> (linearisation, parameter, the config keeps `rho`)
VARIANTS = {'scaler': ('scaler', 'c', True), 'operator_c': ('operator', 'c', True), 'operator_rho': ('operator', 'rho', True),
            'full_rho_given': ('full', 'c', True), 'full_gardner': ('full', 'c', False)}


def small_config(hd, density=True, **extra):
    "a 13 x 17 grid with nPML = 3 in the geometry style of frechet_cases.config: a fixed array, three frequencies, the last one damped"
    rng = np.random.default_rng(7)
    c, rho = rng.uniform(2000., 2600., (SNZ, SNX)), rng.uniform(1800., 2300., (SNZ, SNX))
    X, Z = SDX * (SNX - 1), SDX * (SNZ - 1)
    lo = SNPML + 1
    src = np.stack([np.linspace(SDX * lo, X - SDX * lo, SNSRC), np.full(SNSRC, SDX * 4.3)], axis=1)
    rec = np.stack([np.linspace(SDX * (lo + 0.4), X - SDX * (lo + 0.6), SNREC), np.full(SNREC, Z - SDX * (lo + 0.7))], axis=1)
    geom = dict(src=src, rec=rec, mode='fixed', sterms=ac.randc(rng, SNSRC), rterms=ac.randc(rng, SNREC))
    sc = dict(nx=SNX, nz=SNZ, dx=SDX, dz=SDX, c=c, rho=rho, nPML=SNPML, freeSurf=(True, False, False, False), freqs=list(fc.FREQS),
              sterms=ac.randc(rng, len(fc.FREQS)), geom=geom, parallel=False,
              Disc=ac.OracleMiniZephyrHDT if hd else ac.OracleMiniZephyrT, hostGradient=True)
    if hd:
        sc.update(scaleTerm=0.7 - 0.2j)
    if not density:
        del sc['rho']
    sc.update(extra)
    return sc


def small_pair(hd, density=True, **extra):
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    sc = small_config(hd, density, **extra)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def hvec_diagonal(prob, uF, cells, **kw):
    "e_i . Hvec(e_i) for the cells given"
    out = np.zeros(len(cells))
    for k, i in enumerate(cells):
        e = np.zeros(prob.nrow)
        e[i] = 1.0
        out[k] = prob.Hvec(None, e, u=uF, **kw)[i]
    return out


def cells_37x53():
    """about 36 cells of the 37 x 53 case: the four corners, cells on each boundary line and next to them, cells in each absorbing layer and under the free
    surface, and the interior"""
    nz, nx, n = fc.NZ, fc.NX, fc.NPML
    zx = [(0, 0), (0, nx - 1), (nz - 1, 0), (nz - 1, nx - 1),                                   # corners
          (0, 20), (nz - 1, 31), (17, 0), (22, nx - 1), (0, 1), (nz - 1, nx - 2),                # boundary lines
          (1, 1), (1, 25), (nz - 2, 26), (18, 1), (19, nx - 2), (1, nx - 2), (nz - 2, 1),        # next to them
          (2, 14), (3, 30), (n - 1, 40),                                                       # under the free surface
          (nz - 3, 12), (nz - n, 27), (nz - 4, nx - 4),                                        # bottom layer
          (15, 2), (20, n - 1), (16, nx - 3), (21, nx - n),                                    # side layers
          (n, n), (n, nx - n - 1), (nz - n - 1, n), (nz - n - 1, nx - n - 1),                   # the layers' inner edge
          (12, 20), (18, 26), (20, 33), (14, 40), (25, 15)]                                    # interior
    return [z * nx + x for z, x in zx]


def interior_cells_25(seed=5):
    "25 cells of the 37 x 53 case outside the absorbing layers"
    rng = np.random.default_rng(seed)
    n = fc.NPML
    z = rng.integers(n + 1, fc.NZ - n - 1, 25)
    x = rng.integers(n + 1, fc.NX - n - 1, 25)
    return sorted(set((z * fc.NX + x).tolist()))


def unit_planes(prob, sub, i, linearisation, parameter, dtype=np.complex128):
    "the planes of d A_f / d p_i for a resolved linearisation: what JvecBorn runs along e_i ('scaler' has none)"
    if linearisation == 'operator' and parameter == 'c':
        e = np.zeros(prob.nrow)
        e[i] = 1.0
        return fr.massPlanes(sub, e, dtype)
    return pc.unit_planes(sub, i, 'rho' if parameter == 'rho' else 'c', prob._gardnerChain() if parameter == 'c' else None, dtype)


def transposed_greens(prob, sv, ifreq):
    "g_r = A_f^-T R_r^H (N, nrec) from a sparse LU of the oracle matrix transposed"
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from zephyr_amd.sparse import planes_to_csr
    sub = prob.system.subProblems[ifreq]
    A = planes_to_csr(ac.oracle_planes(sub), int(sub.nz), int(sub.nx))          # (the forward system's operator: not transposed)
    lu = spla.splu(sp.csc_matrix(A.T))
    Rh = np.conj(np.asarray(sp.csr_matrix(sv.rVec(0, ifreq)).todense())).T
    return lu.solve(np.ascontiguousarray(Rh))


def brute_force(prob, sv, uF, cells, linearisation, parameter):
    "|scaleTerm|^2 sum_f sum_s sum_r |g_r^T (E_i u^_s)|^2 for the cells given, E_i u^ by applyPlanes on the planes along e_i"
    st = complex(prob.system.scaleTerm)
    out = np.zeros(len(cells))
    for ifreq, sub in enumerate(prob.system.subProblems):
        g = transposed_greens(prob, sv, ifreq)
        uh = np.conj(np.asarray(uF[ifreq]) / st)
        for k, i in enumerate(cells):
            r = fr.applyPlanes(unit_planes(prob, sub, i, linearisation, parameter), uh, sub.nz, sub.nx)
            out[k] += abs(st) ** 2 * float((np.abs(g.T @ r) ** 2).sum())
    return out


def rel(got, want):
    "max over cells of |got - want| / |want|; a cell where want is exactly 0 must be exactly 0"
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(want != 0, np.abs(got - want) / np.where(want != 0, np.abs(want), 1), np.where(got != 0, np.inf, 0))
    return float(r.max())


# ---- the kernels in 80-bit arithmetic -----------------------------------------------------------------------------------------------------------------
# widths either side of the new tile edge: k_lag_gram keeps a halo of two, 60 cells per wave
GRAM_CASES = dc.KERNEL_CASES + [(5, 60, 5), (5, 59, 1), (6, 121, 9)]


def gram_inputs(nz, nx, nsrc, seed=0):
    "U (nsrc, N) with columns of very different size and a non-zero C0 (13, N)"
    rng = np.random.default_rng(seed)
    N = nz * nx
    return ac.randc(rng, (nsrc, N)) * 10.0 ** rng.uniform(-3, 3, (nsrc, 1)), ac.randc(rng, (13, N))


def gram_touched(nz, nx):
    "bool (13, N): the entries whose partner i + off_l lies inside the grid"
    ones = np.ones((nz, nx))
    return np.stack([fr._at(ones, dz, dx).ravel() > 0 for dz, dx in fr.GRAM_LAGS])


def gram_reference(C0, U, nz, nx, dtype=CLD):
    "(ref, mag, added): C0 + lagGram(U) (untouched entries: C0), |C0| + the magnitude evaluation, and the latter alone"
    c0 = np.asarray(C0).astype(dtype)
    ut = np.asarray(U).T
    added = fr.lagGram(ut, nz, nx, dtype=dtype, magnitude=True)
    return c0 + fr.lagGram(ut, nz, nx, dtype=dtype), np.maximum(np.abs(c0.real), np.abs(c0.imag)) + added, added


def gram_from_outer(U, nz, nx):
    "the 25 diagonals of U U^H: {lag: (N,)} with entry i = (U U^H)[i, i + off] where the partner is inside the grid, 0 elsewhere"
    ut = np.asarray(U).T
    N = nz * nx
    G = ut @ np.conj(ut).T
    iz, ix = np.divmod(np.arange(N), nx)
    out = {}
    for dz in range(-2, 3):
        for dx in range(-2, 3):
            ok = (iz + dz >= 0) & (iz + dz < nz) & (ix + dx >= 0) & (ix + dx < nx)
            d = np.zeros(N, dtype=np.complex128)
            d[ok] = G[np.arange(N)[ok], (np.arange(N) + dz * nx + dx)[ok]]
            out[(dz, dx)] = d
    return out


GN_MODES = {'velocity': ('full', 'c', True), 'buoyancy': ('full', 'b', True), 'gardner': ('full', 'c', False), 'mass': ('operator', 'c', True),
            'diagonal': ('scaler', 'c', True)}


def combine_inputs(nz, nx, seed=0, nu=3, ng=4):
    """(Cu, Cg, touched): two sets of planes (13, N) that are the lag products of a few random columns of very different size (so Gamma and Phi are positive
    semi-definite and H >= 0), zero where the partner is outside the grid, and the mask of the entries k_lag_gram writes"""
    rng = np.random.default_rng(seed)
    N = nz * nx
    u = ac.randc(rng, (N, nu)) * 10.0 ** rng.uniform(-2, 2, (1, nu))
    g = ac.randc(rng, (N, ng)) * 10.0 ** rng.uniform(-2, 2, (1, ng))
    return fr.lagGram(u, nz, nx), fr.lagGram(g, nz, nx), gram_touched(nz, nx)


def combine_reference(op, Cu, Cg, mode, chain, alpha, W, H0, dtype=CLD):
    """(ref, mag): H0 + alpha W H and |H0| + alpha W M with H = frechet.gaussNewtonDiagonal on the planes Cu, Cg of the UNCONJUGATED solves: the kernel is fed their
    conjugates and conjugates its coefficients, which leaves the real trace as it is.  'diagonal': the unit weight, |w|^2 is the caller's W."""
    lin, par, _ = GN_MODES[mode]
    kw = dict(parameter=par, chain=chain, linearisation=lin, dtype=dtype)
    if lin == 'scaler':
        kw['weight'] = np.ones(np.shape(Cu)[1])
    H = fr.gaussNewtonDiagonal(op, Cu, Cg, **kw)
    M = fr.gaussNewtonDiagonal(op, Cu, Cg, magnitude=True, **kw)
    real = LD if dtype is CLD else np.float64
    w = real(alpha) * (real(1) if W is None else np.asarray(W).astype(real))
    h0 = np.asarray(H0).astype(real)
    return h0 + w * H, np.abs(h0) + w * M


worst_ratio = pc.worst_ratio
