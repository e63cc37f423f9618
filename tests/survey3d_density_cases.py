"""Shared by tests/test_survey3d_density_host.py (CPU) and tests/test_gpu_survey3d_density.py (GPU): the problem / survey pairs with derivatives3D=True, the
floor of the finite-difference check of dA[db], and the extended-precision references of the kernels of csrc/survey3d_density.hip with their rounding
bounds -- all counted here, before anything ran."""
import numpy as np

import zephyr_amd as za
from zephyr_amd import frechet3d
from tests import survey3d_cases as s3

U53 = s3.U53

# ---- the floor of A(b + db) - A(b) against dA[db] ------------------------------------------------------------------------------------------------------
# An entry of the oracle matrix is bbar (lx + ly + lz) + K mu.  Rounded operations of the Laplacian part: 1 / rho (1), the sum b_p + b_{p+o} (1; the halving
# is exact), each of lx, ly, lz a table value times a rounded scalar m m / h^2 (3 + 1 = 4, the three in parallel), their two additions (2), the product with
# bbar (1): 9.  Of the mass part: c^2 (2), rho c^2 (1), om~^2 (2), the complex division (4), mu (3) and the product (1): 13.  Their addition: 1.  So an entry
# carries at most 14 u relative to |bbar lap_o| + |K mu_o|; the perturbed matrix is built from rho' = 1 / (b + db), three more roundings (the sum, the
# division, and 1 / rho' again counted above): 17.  The difference of the two matrices therefore misses dA[db] by at most (14 + 17) u = 31 u of that
# magnitude -- the host maps' own rounding is smaller by the factor ||db / b|| -- taken as 40 u:
#     |A(b + db) - A(b) - dA[db]|_max <= 40 u max_o,p (|bbar lap_o| + |K mu_o|),
# which relative to |dA| ~ ||db / b|| |A| is the floor 40 u / ||db / b||.
FD_FLOOR_ULPS = 40


def fd_floor(op, L, b):
    '40 u max(|bbar lap_o| + |K mu_o|), bounded from above by 40 u (max b max |L| + max |b kappa| mu_0) with b the larger of the two buoyancy fields'
    mu0 = frechet3d.massWeight3(0, 0, 0)
    return FD_FLOOR_ULPS * U53 * (b.max() * abs(L).max() + (b * np.abs(frechet3d.kappa3(op))).max() * mu0)


def host_pair(grid, mode='fixed', gardner=False, **extra):
    'survey3d_cases.host_pair with derivatives3D=True; gardner: no `rho` in the config, the density follows the velocity'
    dims, npml, freqs = s3.HOST_GRIDS[grid]
    sc = s3.survey_config(dims, npml, freqs, mode)
    sc.update(Disc=s3.OracleHelm3D, hostGradient=True, scaleTerm=0.7 - 0.2j, premul=1.1 + 0.3j, tau=1.5, derivatives3D=True)
    if gardner:
        del sc['rho']
    sc.update(extra)
    prob, sv = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def small_config(dims, seed=0):
    'a heterogeneous model with complex c, dx != dy != dz, a finite tau and nPML = 2 on a small grid: the stretch tables differ cell to cell and axis to axis'
    nz, ny, nx = dims
    rng = np.random.default_rng(seed)
    c = (1800. + 1500. * rng.random(dims)) * (1 + 0.01j)
    rho = 1000. + 500. * rng.random(dims)
    return dict(nx=nx, ny=ny, nz=nz, dx=9., dy=11., dz=10., c=c, rho=rho, freq=11., tau=0.5, nPML=2, cPML=250.)


# ---- extended-precision references of the Laplacian kernels ---------------------------------------------------------------------------------------------
# The stretch tables.  The reference takes them from frechet3d.stretchTables3 (numpy, fp64), the kernels from the handle (C++, fp64): the same formulas, but
# cos, the complex divisions and the complex product are each side's own.  Per table value, normwise: gamma (cos and two products, 4 u), xi = 1 - i gamma / om~
# (a complex division, 4 u), xi + xi' (1), the complex product (3), the reciprocal (a complex division, 5): 17 u on either side, 34 u between the two,
# relative to |L| <= |Re L| + |Im L|.  L(0) = -(L(-1) + L(+1)) adds one rounding and no cancellation in the majorant, which carries |L(-1)|_1 + |L(+1)|_1
# ... both real parts are positive (Re xi = 1), so |L(0)|_1 is within a factor of that; 2 u more: 36 u.
#
# The arithmetic of lap3_sum per output component, relative to the majorant sum_o (|Lx|_1 m m / dx^2 + m |Ly|_1 m / dy^2 + m m |Lz|_1 / dz^2) |t_{p+o}|_1:
# along the deepest path, a three-term complex dot product with the table (each component: products and additions of six terms, 6 roundings at most), two
# weighted sums m0 b + m1 (a + c) (4 each: the rounded constant, the product, the neighbour addition, the final addition), the product with the rounded
# 1 / h^2 (2 + 1) and the two additions of the three parts (2): 6 + 8 + 3 + 2 = 19.  Fused multiply-adds only remove roundings.
#
# k_lap3_sources adds: t = (B_p + B_{p+o}) X (2), the product with coef / 2 (2 for the complex product; the halving is exact): 36 + 19 + 4 = 59, taken as
# 64 u; in add mode one more addition, relative to |R0|_1 + the majorant.
# k_lap3_imaging adds per column the product with the centre value (2) and the addition into the running sum (1, relative to the sum so far: k in all), and at
# the end the halving (exact) and the addition into P0 (1): 36 + 19 + 2 + k + 1 = 58 + k, taken as (64 + 2 k) u.
LAP_SOURCES_ULPS = 64


def lap_imaging_ulps(k):
    return 64 + 2 * k


def _ldr(a):
    return np.asarray(a).astype(np.longdouble)


def _lap_weights(op):
    """{(oz, oy, ox): (lap_o as a (nz, ny, nx) clongdouble array, its majorant as longdouble)}: the tables of frechet3d.stretchTables3 widened exactly, the
    constants m and 1 / h^2 in 80 bits"""
    nz, ny, nx = op.modelDims
    (Lx, Ly, Lz) = (tuple(s3._ld(t) for t in axis) for axis in frechet3d.stretchTables3(op))
    third, sixth = np.longdouble(2) / np.longdouble(3), np.longdouble(1) / np.longdouble(6)
    m = lambda o: third if o == 0 else sixth
    ix2, iy2, iz2 = (np.longdouble(1) / (np.longdouble(float(h)) * np.longdouble(float(h))) for h in (op.dx, op.dy, op.dz))
    out = {}
    for (oz, oy, ox) in s3.h3.OFFSETS3:
        tx, ty, tz = Lx[ox + 1][None, None, :], Ly[oy + 1][None, :, None], Lz[oz + 1][:, None, None]
        wx, wy, wz = m(oy) * m(oz) * ix2, m(ox) * m(oz) * iy2, m(ox) * m(oy) * iz2
        lap = np.broadcast_to(tx * wx + ty * wy + tz * wz, (nz, ny, nx))
        maj = np.broadcast_to(s3._l1(tx) * wx + s3._l1(ty) * wy + s3._l1(tz) * wz, (nz, ny, nx))
        out[(oz, oy, ox)] = (lap, maj)
    return out


def _shift(T, o):
    'T[p + o] on the grid, zero where p + o lies outside it; T (nz, ny, nx, ...)'
    nz, ny, nx = T.shape[:3]
    Tp = np.zeros((nz + 2, ny + 2, nx + 2) + T.shape[3:], dtype=T.dtype)
    Tp[1:-1, 1:-1, 1:-1] = T
    oz, oy, ox = o
    return Tp[1 + oz:1 + oz + nz, 1 + oy:1 + oy + ny, 1 + ox:1 + ox + nx]


def lap_sources_reference(op, U, B, coef, conj, R0=None):
    """(R, bound) for columns U (k, N): R[s] = coef / 2 sum_o lap_o(p) (B_p + B_{p+o}) X_s[p + o] on the interior rows in 80-bit arithmetic -- which is
    coef (1/2 B (.) L X + 1/2 L(B (.) X)) --, exact zeros on the boundary rows (store mode) or R0 there and R0 + the value inside (add mode: R0 given); the
    componentwise bound is LAP_SOURCES_ULPS u times the majorant (|Re coef| + |Im coef|) / 2 sum_o maj_o (|B_p| + |B_{p+o}|) |X|_1 (+ |R0|_1)."""
    dims = tuple(op.modelDims)
    k, N = U.shape
    X = s3._ld(np.conj(U) if conj else U).T.reshape(dims + (k,))
    Bl = _ldr(B).reshape(dims + (1,))
    W = _lap_weights(op)
    S = np.zeros(dims + (k,), dtype=np.clongdouble)
    maj = np.zeros(dims + (k,), dtype=np.longdouble)
    X1 = s3._l1(X)
    for o, (lap, lm) in W.items():
        S += lap[..., None] * ((Bl + _shift(Bl, o)) * _shift(X, o))
        maj += lm[..., None] * ((np.abs(Bl) + np.abs(_shift(Bl, o))) * _shift(X1, o))
    inside = s3._interior(dims)[..., None]
    half = np.clongdouble(coef) / 2
    val = np.where(inside, half * S, 0)
    vmaj = np.where(inside, (abs(coef.real) + abs(coef.imag)) / 2 * maj, 0)
    if R0 is not None:
        r0 = s3._ld(R0).T.reshape(dims + (k,))
        val = r0 + val
        vmaj = np.where(inside, vmaj + s3._l1(r0), 0)
    return val.reshape((N, k)).T, (LAP_SOURCES_ULPS * U53 * vmaj).reshape((N, k)).T


def lap_imaging_reference(op, UF, UB, P0, conj):
    """(P, bound): P = P0 + 1/2 sum_s (Z0_s (.) L F_s + F_s (.) L^T Z0_s) in 80-bit arithmetic, F = UF or conj(UF), Z0 = UB (or its conjugate) with the boundary
    rows masked; (L^T z)_j = sum_o lap_o(j - o) z_{j-o}, the tables read at j - o.  Bound: lap_imaging_ulps(k) u times
    |P0|_1 + 1/2 sum_s (|Z0|_1 sum_o maj_o(j) |F_{j+o}|_1 + |F|_1 sum_o maj_o(j - o) |Z0_{j-o}|_1)."""
    dims = tuple(op.modelDims)
    k, N = UF.shape
    inside = s3._interior(dims)[..., None]
    F = s3._ld(np.conj(UF) if conj else UF).T.reshape(dims + (k,))
    Z = np.where(inside, s3._ld(np.conj(UB) if conj else UB).T.reshape(dims + (k,)), 0)
    F1, Z1 = s3._l1(F), s3._l1(Z)
    LF, LTZ = np.zeros_like(F), np.zeros_like(F)
    mLF, mLTZ = np.zeros_like(F1), np.zeros_like(F1)
    for o, (lap, lm) in _lap_weights(op).items():
        LF += lap[..., None] * _shift(F, o)
        mLF += lm[..., None] * _shift(F1, o)
        back = tuple(-x for x in o)
        LTZ += _shift(lap[..., None] * Z, back)               # (lap_o (.) z)[j - o]
        mLTZ += _shift(lm[..., None] * Z1, back)
    P0l = s3._ld(P0).reshape(dims)
    P = P0l + (Z * LF + F * LTZ).sum(axis=3) / 2
    maj = s3._l1(P0l) + (Z1 * mLF + F1 * mLTZ).sum(axis=3) / 2
    return P.ravel(), (lap_imaging_ulps(k) * U53 * maj).ravel()


# ---- extended-precision reference of k_buoy3_chain ------------------------------------------------------------------------------------------------------
# Per cell, in 80 bits, each output bounded by its OWN majorant.  Rounded operations of the kernel:
#   b = 1 / rho (1);  chain = -(b b): (1 + d)^2 from b and one product, 3 u -- or -b / (4 Re c): b (1), the division (1; 4 Re c is exact), 2 u;
#   db = chain din: one more product, 4 u at most relative to |db_j|                                                                    -> CHAIN_DB_ULPS = 4
#   kappa = om~^2 / c^2 by Smith's division: c^2 (3 u normwise: two products and an addition per component), om~^2 (3 u), the division (6 u normwise: a
#   quotient, a product, an addition, two numerators of a product and an addition each, two divisions), and om~ itself is formed in fp64 on both sides
#   (2 pi f: 1 u, twice in the square): 14 u relative to |kappa_j|;  w kappa: a complex product, 3 u normwise: 17 u relative to |w| |kappa_j|
#   W = (w kappa) db: the error of db (4) and one product per component (1): 22 u relative to |w| |kappa_j| |db_j|
#   G += chain Re(w Plap + (w kappa) Pmass): Re(w Plap) two products and a subtraction, 2 u relative to |w|_1 |Plap|_1; Re((w kappa) Pmass) the error of
#   w kappa (17) and 2 more relative to |w kappa| |Pmass|_1; their addition (1); the product with the chain (3 + 1); the addition into G0 (1): 25 u relative to
#   |G0_j| + |chain_j| (|w|_1 |Plap_j|_1 + |w kappa_j| |Pmass_j|_1).
# W and G are taken at 32 u, the figure of the velocity chain's test.  Fused multiply-adds only remove roundings.
CHAIN_DB_ULPS = 4
CHAIN_ULPS = 32
# The Gardner chain of a handle whose density is the default one, against b = Re(c)^-0.25 / 310 in 80 bits: the handle's rho = 310 Re(c)^0.25 was formed in
# fp64 (the power, 2 u for the library's function, and the product, 1), then the kernel's 1 / rho, division and product (3): 6 u, taken as 8 u of |db_j|.
GARDNER_DB_ULPS = 8


def buoy_chain_reference(op, gardner, din, Plap, Pmass, G0, w):
    """{'DB' | 'W' | 'G': (reference, bound)} of k_buoy3_chain per cell in 80-bit arithmetic at the model of `op` (its c, its rho and its damped frequency):
    chain = -1 / rho^2 or (gardner) -(1 / rho) / (4 Re c); DB = chain din, W = w kappa DB, G = G0 + chain Re(w (Plap + kappa Pmass)), each with the bound
    counted above."""
    N = int(op.nrow)
    c = s3._ld(np.broadcast_to(np.asarray(op.c, dtype=np.complex128).ravel(), (N,)))
    rho = _ldr(np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), (N,)))
    om = np.clongdouble(frechet3d.dampedOmega3(op))
    kap = om * om / (c * c)
    b = np.longdouble(1) / rho
    chain = -b / (np.longdouble(4) * c.real) if gardner else -(b * b)
    wl = np.clongdouble(w)
    din, Plap, Pmass, G0 = _ldr(din), s3._ld(Plap), s3._ld(Pmass), _ldr(G0)
    db = chain * din
    W = wl * kap * db
    G = G0 + chain * (wl * (Plap + kap * Pmass)).real
    w1 = np.longdouble(abs(w.real)) + np.longdouble(abs(w.imag))
    majG = np.abs(G0) + np.abs(chain) * (w1 * s3._l1(Plap) + np.abs(wl * kap) * s3._l1(Pmass))
    return dict(DB=(db, CHAIN_DB_ULPS * U53 * np.abs(db)), W=(W, CHAIN_ULPS * U53 * np.abs(wl) * np.abs(kap) * np.abs(db)), G=(G, CHAIN_ULPS * U53 * majG))


def gardner_db_reference(op, din):
    '(db, bound): d b / d c din with b = Re(c)^-0.25 / 310 in 80 bits, and GARDNER_DB_ULPS u of |db_j|'
    N = int(op.nrow)
    cr = _ldr(np.broadcast_to(np.asarray(op.c, dtype=np.complex128).ravel().real, (N,)))
    b = np.power(cr, np.longdouble(-0.25)) / np.longdouble(310)
    db = -b / (np.longdouble(4) * cr) * _ldr(din)
    return db, GARDNER_DB_ULPS * U53 * np.abs(db)
