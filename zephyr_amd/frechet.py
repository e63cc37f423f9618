"""What the exact Frechet derivative of MiniZephyr (linearisation='operator' of HelmBaseProblem.JvecBorn / Jtvec / Hvec) is made of, in numpy: the mass
term of the 9-point operator.  MiniZephyr carries the velocity as K = (omega_d^2 / c^2 - ky^2) / rho of the NEIGHBOURING cell, spread over the nine slots of a
row by the mass weights, and overwrites its boundary rows by +-identity, so

    (dA) u = mask_int (.) M0(dK (.) u),      dK = -2 omega_d^2 v / (c^3 rho)

The host routes of problem.py evaluate this here; the device routes (device_survey.py) take the scalars from here and run the stencil in
k_virtual_sources_op / k_imaging_op (csrc/survey_frechet.hip).  The second part of the module is the derivative with respect to the density (parameter='rho'), the
third the total derivative with respect to the velocity (linearisation='full'): the mass term above, the PML stretch and the density that follows c; then
the second derivative of the operator and the transposed planes, what Hvec(resid=) adds to the Gauss-Newton product (k_velocity_curvature / k_stencil_sources_t,
csrc/survey_newton.hip); and the mixed second derivative with respect to velocity and buoyancy, what parameter='joint' adds to that (k_velocity_adjoint_b /
k_mixed_adjoint, csrc/survey_joint.hip); and the chain from the real velocity and the quality factor of a visco problem to the complex velocity its operators are
assembled at (`viscoChain`; k_visco_perturbation / k_velocity_planes_z / k_visco_chain_adjoint, csrc/survey_visco.hip)."""
import numpy as np


MZ_MASS = (0.6248, 0.09381, 0.000001297)      # centre, edge and corner weights of the lumped/consistent mass average (minizephyr.py:207-209)


def maskInterior(u, nz, nx):
    "a copy of u ((N,) or (N, k), N = nz nx, z-major) with the four boundary lines zeroed: mask_int (.) u"
    a = np.array(u).reshape((int(nz), int(nx)) + np.shape(u)[1:])
    a[0], a[-1], a[:, 0], a[:, -1] = 0, 0, 0, 0
    return a.reshape(np.shape(u))


def massStencil(u, nz, nx, mask=False):
    """M0 u: the constant 9-point stencil of the mass weights on the nz x nx grid (neighbours outside the grid contribute nothing), column by column of
    u ((N,) or (N, k)).  The sum runs centre, then the four edges (up, down, left, right), then the four corners -- the order of the device kernels.
    mask: mask_int (.) M0 u."""
    nz, nx = int(nz), int(nx)
    a = np.asarray(u).reshape((nz, nx) + np.shape(u)[1:])
    p = np.zeros((nz + 2, nx + 2) + a.shape[2:], dtype=a.dtype)
    p[1:-1, 1:-1] = a
    mc, md, me = MZ_MASS
    sh = lambda dz, dx: p[1 + dz:1 + dz + nz, 1 + dx:1 + dx + nx]
    out = mc * a + md * (((sh(-1, 0) + sh(1, 0)) + sh(0, -1)) + sh(0, 1)) + me * (((sh(-1, -1) + sh(-1, 1)) + sh(1, -1)) + sh(1, 1))
    out = out.reshape(np.shape(u))
    return maskInterior(out, nz, nx) if mask else out


def dampedOmega(op):
    "omega_d = 2 pi f - i / tau of an operator (f may be complex)"
    return 2.0 * np.pi * complex(op.freq) - 1j / float(op.tau)


def operatorWeight(op):
    "d K / d c of a MiniZephyr operator per cell, (N,) complex: K = (omega_d^2 / c^2 - (2 pi ky)^2) / rho, so -2 omega_d^2 / (c^3 rho), omega_d = 2 pi f - i / tau"
    om = dampedOmega(op)
    c = np.asarray(op.c, dtype=np.complex128).ravel()
    return -2.0 * om * om / (c * c * c * np.asarray(op.rho, dtype=np.float64).ravel())


# ---- the density derivative: every interior row of MiniZephyr is linear in the buoyancy b = 1 / rho ---------------------------------------------
# Written out from the assembly (minizephyr.py:90-243; csrc/mz_row.hpp mz_star).  With kappa = omega_d^2 / c^2 - (2 pi ky)^2 of a cell, the row factors
# X, Z, px, pz of the row's own cell (c and the PML only) and the averages a_o = (b_i + b_(i+o)) / 2 over the eight lags o = (sz, sx), row i is
#     corner   o:  e kappa b (i+o) + tc_o a_o                                tc_o = B ((Z + X) / (4 dxz) + (sz pz + sx px) / (4 dd))
#     vertical o:  d kappa b (i+o) + tv_o a_o + tzx (a_(sz,1) + a_(sz,-1))   tv_o = A (Z / dz + sz pz / 2) / dz,   tzx = B (Z - X) / (4 dxz)
#     horizontal:  d kappa b (i+o) + th_o a_o - tzx (a_(1,sx) + a_(-1,sx))   th_o = A (X / dx + sx px / 2) / dx
#     centre:      c kappa b (i)   - sum_o t_o a_o                           (the stiffness rows sum to zero)
# and the four boundary lines are +-identity whatever b is.  L : db -> the nine planes of d A / d b along db (`buoyancyPlanes`), L^T its plain transpose
# (`buoyancyAdjoint`).  The device kernels k_buoyancy_planes / k_buoyancy_adjoint (csrc/survey_frechet.hip) are these two; an interior row reads only cells inside
# the grid, so the edge padding of the assembly never enters.
MZ_STIFF = (0.5461, 0.4539)                   # the stiffness weights A, B of the rotated and the plain star (minizephyr.py:205-206)
LAGS = [(sz, sx) for sz in (-1, 0, 1) for sx in (-1, 0, 1)]      # slot k = 3 (sz + 1) + (sx + 1): plane k multiplies u(iz + sz, ix + sx)


def _real(dtype):
    return np.longdouble if np.dtype(dtype) == np.dtype(np.clongdouble) else np.float64


def _profile(n, npml, h, fs_low, fs_high):
    'the 1-D PML distance and sign profiles along an axis (minizephyr.py:98-118,126-127; the assignment order kept)'
    dist, sgn = np.zeros(n), np.zeros(n)
    dist[:npml] = np.arange(npml, 0, -1) * h
    dist[-npml:] = np.arange(1, npml + 1, 1) * h
    if not fs_high:
        sgn[-npml:] = -1.0
    if not fs_low:
        sgn[:npml] = 1.0
    return dist, sgn


def _pmlAxes(op, dtype):
    """(c, om, iom, (fx, distx, sgnx), (fz, distz, sgnz)) of a 2-D MiniZephyr operator in the arithmetic of dtype: the velocity (nz, nx), the damped angular
    frequency and i times it, and per axis the PML factor with the distance and sign profiles broadcast over the grid"""
    R = _real(dtype)
    nz, nx, npml = int(op.nz), int(op.nx), int(op.nPML)
    dx, dz = R(float(op.dx)), R(float(op.dz))
    c = np.asarray(op.c).astype(dtype).reshape((nz, nx))
    f = complex(op.freq)
    om = 2 * R(np.pi) * (R(f.real) + dtype(1j) * R(f.imag))          # (the double pi in either arithmetic: the operator is defined with it)
    tau = float(op.tau)
    if np.isfinite(tau) and tau != 0.0:
        om = om - dtype(1j) / R(tau)
    fs = tuple(bool(x) for x in op.freeSurf)
    lx, lz = dx * (npml - 1), dz * (npml - 1)
    fx, fz = 3 * np.log(R(1000)) / (2 * lx ** 3), 3 * np.log(R(1000)) / (2 * lz ** 3)
    distx, sgnx = _profile(nx, npml, float(op.dx), fs[3], fs[1])
    distz, sgnz = _profile(nz, npml, float(op.dz), fs[0], fs[2])
    return c, om, dtype(1j) * om, (fx, distx.astype(R)[None, :], sgnx.astype(R)[None, :]), (fz, distz.astype(R)[:, None], sgnz.astype(R)[:, None])


def rowFactors(op, dtype=np.complex128):
    """(X, Z, px, pz, kappa) of a 2-D MiniZephyr operator, each (nz, nx): the PML stretch factors of a row from the velocity of its own cell, and
    kappa = omega_d^2 / c^2 - (2 pi ky)^2 per cell.  dtype np.clongdouble: evaluated in 80-bit arithmetic."""
    R = _real(dtype)
    c, om, iom, (fx, distx, sgnx), (fz, distz, sgnz) = _pmlAxes(op, dtype)
    denx = fx * c * distx ** 2 + iom
    X = (iom / denx) ** 2
    px = sgnx * X * (2 * fx * c * distx) / denx
    denz = fz * c * distz ** 2 + iom
    Z = (iom / denz) ** 2
    pz = sgnz * Z * (2 * fz * c * distz) / denz
    aky = 2 * R(np.pi) * R(float(op.ky))
    kappa = om * om / (c * c) - aky * aky
    return X + 0 * c, Z + 0 * c, px + 0 * c, pz + 0 * c, kappa


def rowFactorsDc(op, dtype=np.complex128, magnitude=False):
    """d (X, Z, px, pz) / d c of `rowFactors`, each (nz, nx).  Per axis, with den = f c d^2 + i omega_d (f the PML factor, d the profile distance, s its
    sign), X = (i omega_d / den)^2 and p = s X 2 f c d / den:

        dX / dc = -2 X f d^2 / den,      dp / dc = s 2 f d (dX/dc c / den + X / den - X c f d^2 / den^2)

    Outside the layers d = 0 and all four vanish.  The factors are holomorphic in c: this is the derivative along a real perturbation of a complex c too.
    magnitude: the moduli, dp / dc as the sum of the moduli of its three terms (they cancel in part) -- what bounds the rounding of the evaluation."""
    c, _, iom, ax, az = _pmlAxes(op, dtype)
    out = []
    for f, d, s in (ax, az):
        den = f * c * d ** 2 + iom
        S = (iom / den) ** 2
        dS = -2 * S * (f * d ** 2) / den
        terms = (dS * c / den, S / den, -S * c * (f * d ** 2) / den ** 2)
        if magnitude:
            dS, dp = np.abs(dS), np.abs(s) * (2 * f * d) * ((np.abs(terms[0]) + np.abs(terms[1])) + np.abs(terms[2]))
        else:
            dp = s * (2 * f * d) * ((terms[0] + terms[1]) + terms[2])
        out.append((dS + 0 * c.real, dp + 0 * c.real) if magnitude else (dS + 0 * c, dp + 0 * c))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def massWeightDc(op, dtype=np.complex128):
    "d kappa / d c = -2 omega_d^2 / c^3 per cell (nz, nx), kappa = omega_d^2 / c^2 - (2 pi ky)^2, in the arithmetic of dtype"
    c, om = _pmlAxes(op, dtype)[:2]
    return -2 * om * om / (c * c * c)


def rowFactorsD2c(op, dtype=np.complex128, magnitude=False):
    """d^2 (X, Z, px, pz) / d c^2 of `rowFactors`, each (nz, nx).  Per axis, in the notation of `rowFactorsDc` and with a = f d^2, X = (i omega_d)^2 / den^2 and
    p = s 2 f d (i omega_d)^2 c / den^3, so

        d^2 X / dc^2 = 6 X a^2 / den^2,      d^2 p / dc^2 = s 2 f d (2 (d^2 X / dc^2) c / den - 6 X a / den^2)

    Outside the layers d = 0 and all four vanish.  magnitude: the moduli, d^2 p / dc^2 as the sum of the moduli of its two terms (they cancel in part)."""
    c, _, iom, ax, az = _pmlAxes(op, dtype)
    out = []
    for f, d, s in (ax, az):
        a = f * d ** 2
        den = a * c + iom
        S = (iom / den) ** 2
        Sa = S * a / den
        d2S = 6 * Sa * a / den
        terms = (2 * d2S * c / den, -6 * Sa / den)
        if magnitude:
            d2S, d2p = np.abs(d2S), np.abs(s) * (2 * f * d) * (np.abs(terms[0]) + np.abs(terms[1]))
        else:
            d2p = s * (2 * f * d) * (terms[0] + terms[1])
        out.append((d2S + 0 * c.real, d2p + 0 * c.real) if magnitude else (d2S + 0 * c, d2p + 0 * c))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def massWeightD2c(op, dtype=np.complex128):
    "d^2 kappa / d c^2 = 6 omega_d^2 / c^4 per cell (nz, nx), in the arithmetic of dtype"
    c, om = _pmlAxes(op, dtype)[:2]
    return 6 * om * om / ((c * c) * (c * c))


def _stiffness(op, rf, magnitude=False):
    """{lag: t_o} (nz, nx) and tzx of the header comment from the row factors.  magnitude: every term by its modulus, every difference a sum -- what bounds
    the rounding of the evaluation per component."""
    X, Z, px, pz = rf[:4]
    if magnitude:
        X, Z, px, pz = np.abs(X), np.abs(Z), np.abs(px), np.abs(pz)
    R = X.real.dtype.type
    A, B = R(MZ_STIFF[0]), R(MZ_STIFF[1])
    dx, dz = R(float(op.dx)), R(float(op.dz))
    dxz = (dx * dx + dz * dz) / 2
    dd = np.sqrt(dxz)
    s = (lambda v: abs(v)) if magnitude else (lambda v: v)
    t = {}
    for sz, sx in LAGS:
        if sz and sx:
            t[(sz, sx)] = B * ((Z + X) / (4 * dxz) + (s(sz) * pz + s(sx) * px) / (4 * dd))
        elif sz:
            t[(sz, sx)] = A * (Z / dz + s(sz) * pz / 2) / dz
        elif sx:
            t[(sz, sx)] = A * (X / dx + s(sx) * px / 2) / dx
    tzx = B * ((Z + X) if magnitude else (Z - X)) / (4 * dxz)
    return t, tzx


def _at(a, sz, sx):
    "a(i + o) on the grid, zero where i + o is outside: s[z, x] = a[z + sz, x + sx]"
    nz, nx = a.shape[:2]
    out = np.zeros_like(a)
    out[max(0, -sz):nz - max(0, sz), max(0, -sx):nx - max(0, sx)] = a[max(0, sz):nz - max(0, -sz), max(0, sx):nx - max(0, -sx)]
    return out


def _interiorMask(nz, nx):
    m = np.zeros((nz, nx), dtype=bool)
    m[1:-1, 1:-1] = True
    return m


def _starPlanes(t, tzx, b, kb, R, dtype, magnitude):
    """the nine planes of the star of the header comment from its stiffness factors (t, tzx), the buoyancy field b (nz, nx) that is averaged and the mass
    terms kb of the cells; boundary rows zero.  Linear in (t, tzx, kb) for a fixed b and in (b, kb) for fixed factors."""
    nz, nx = b.shape
    a = {o: (b + _at(b, *o)) / 2 for o in LAGS if o != (0, 0)}
    mc, md, me = [R(w) for w in MZ_MASS]
    sgn = 1 if magnitude else -1
    C = np.zeros((9, nz, nx), dtype=R if magnitude else dtype)
    centre = mc * kb
    for k, (sz, sx) in enumerate(LAGS):
        if (sz, sx) == (0, 0):
            continue
        o = (sz, sx)
        if sz and sx:
            C[k] = me * _at(kb, sz, sx) + t[o] * a[o]
        elif sz:
            C[k] = md * _at(kb, sz, sx) + t[o] * a[o] + tzx * (a[(sz, 1)] + a[(sz, -1)])
        else:
            C[k] = md * _at(kb, sz, sx) + t[o] * a[o] + sgn * tzx * (a[(1, sx)] + a[(-1, sx)])
        centre = centre + sgn * t[o] * a[o]
    C[4] = centre
    C[:, ~_interiorMask(nz, nx)] = 0
    return C


def buoyancyPlanes(op, db, dtype=np.complex128, magnitude=False):
    """L[db]: the nine planes (9, nz, nx) of d A / d b along the real buoyancy perturbation db (N,), boundary rows zero, for the 2-D MiniZephyr operator `op`
    (its c, PML, frequency, damping and ky; rho does not enter: A is linear in b).  magnitude: the same sum with every term replaced by its modulus."""
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    rf = rowFactors(op, dtype)
    kappa = np.abs(rf[4]) if magnitude else rf[4]
    t, tzx = _stiffness(op, rf, magnitude)
    b = np.asarray(db).astype(R).reshape((nz, nx))
    if magnitude:
        b = np.abs(b)
    return _starPlanes(t, tzx, b, kappa * b, R, dtype, magnitude)


def buoyancyAdjoint(op, P, dtype=np.complex128, magnitude=False, conj=False):
    """L^T P: (N,) with <L[db], P> = <db, L^T P> under the bilinear pairing sum_k sum_i (no conjugate), P (9, N) or (9, nz, nx) complex; its boundary rows
    are not read.  conj: conj(L)^T P.  magnitude: the sum of the moduli of the terms."""
    rf = rowFactors(op, dtype)
    return _buoyancyGather(op, P, rf[:4], rf[4], dtype, magnitude, conj)


def _buoyancyGather(op, P, rf, kappa, dtype, magnitude, conj):
    """the transpose of b -> star(rf_i, bn[b], Kn_k = kappa_j b_j) applied to the planes P, (N,): `buoyancyAdjoint` with the row factors and kappa of the operator,
    `mixedAdjointB` with their derivatives along a velocity perturbation.  rf: (X, Z, px, pz) of the rows (moduli with magnitude), kappa per cell."""
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    if conj:
        rf, kappa = tuple(np.conj(x) for x in rf), np.conj(kappa)
    kappa = np.abs(kappa) if magnitude else kappa
    t, tzx = _stiffness(op, rf, magnitude)
    Pl = np.asarray(P).astype(dtype).reshape((9, nz, nx)).copy()
    Pl[:, ~_interiorMask(nz, nx)] = 0
    if magnitude:
        Pl = np.abs(Pl)
        t = {o: v * _interiorMask(nz, nx) for o, v in t.items()}
    slot = {o: k for k, o in enumerate(LAGS)}
    sgn = 1 if magnitude else -1
    mc, md, me = [R(w) for w in MZ_MASS]
    mass = mc * Pl[4]
    avg = np.zeros((nz, nx), dtype=Pl.dtype)
    for o in LAGS:
        if o == (0, 0):
            continue
        sz, sx = o
        q = t[o] * (Pl[slot[o]] + sgn * Pl[4])
        if sz and sx:
            q = q + tzx * (Pl[slot[(sz, 0)]] + sgn * Pl[slot[(0, sx)]])
        # row i holds (b_i + b_(i+o)) / 2: half of q stays at i, half goes to j = i + o
        avg = avg + q / 2 + _at(q, -sz, -sx) / 2
        mass = mass + (me if sz and sx else md) * _at(Pl[slot[o]], -sz, -sx)
    return (avg + kappa * mass).ravel()


def applyPlanes(C, u, nz, nx):
    "sum_k C_k (.) u(i + off_k) column by column of u ((N,) or (N, k)), cells outside the grid contributing nothing: (dA) u for the planes C (9, nz, nx)"
    nz, nx = int(nz), int(nx)
    a = np.asarray(u).reshape((nz, nx) + np.shape(u)[1:])
    Cb = np.asarray(C).reshape((9, nz, nx) + (1,) * (a.ndim - 2))
    out = np.zeros(a.shape, dtype=np.result_type(a.dtype, Cb.dtype))
    for k, (sz, sx) in enumerate(LAGS):
        out = out + Cb[k] * _at(a, sz, sx)
    return out.reshape(np.shape(u))


def lagProducts(z, u, nz, nx, edges=False):
    """P (9, N): P_k[i] = sum_s z[i, s] u[i + off_k, s] for the nine lags, zero where i is on a boundary line (an interior i has every i + off_k inside the
    grid).  z, u: (N, nsrc).  sum_s z_s^T (dA) u_s = sum_k sum_i C_k[i] P_k[i] for planes C with zero boundary rows.  edges: the centre plane P_4 on the
    boundary lines too -- what planes with a centre entry there (Eurus: `eurusPlanes`) need."""
    nz, nx = int(nz), int(nx)
    za = np.asarray(z).reshape((nz, nx, -1))
    ua = np.asarray(u).reshape((nz, nx, -1))
    inside = _interiorMask(nz, nx)
    P = np.zeros((9, nz, nx), dtype=np.result_type(za.dtype, ua.dtype))
    for k, (sz, sx) in enumerate(LAGS):
        P[k] = np.where(inside, (za * _at(ua, sz, sx)).sum(axis=2), 0)
    if edges:
        P[4] = (za * ua).sum(axis=2)
    return P.reshape((9, nz * nx))


# ---- the total velocity derivative (linearisation='full'): the mass term, the PML stretch and the Gardner density -------------------------------------
# A row is star(row_i, bn, Kn) (csrc/mz_row.hpp mz_star): linear in (row, Kn) for fixed averaged buoyancies bn, and linear in (bn, Kn) for a fixed row.  The row
# factors are functions of c_i, the mass terms Kn_k = kappa_j b_j of c_j (j = i + o_k), so along a real dc
#     dC_i = star(dc_i d row_i / dc, bn[b], Kn_k = (-2 omega_d^2 / c_j^3) b_j dc_j)           the mass term ('operator') and the stretch
#          + star(row_i, bn[db], Kn_k = kappa_j db_j)                                        only where the density follows c: `buoyancyPlanes` of db
# with db = gardnerChain(c) dc for the default density rho = 310 Re(c)^0.25.  Boundary rows zero.  `velocityPlanes` is the map, `velocityAdjoint` the plain
# transpose of its first star (the second one's is `buoyancyAdjoint`); k_velocity_planes / k_velocity_adjoint (csrc/survey_frechet.hip) are the device kernels.

def gardnerChain(c):
    "d b / d c per cell, float64 (N,), of the default density: b = 1 / (310 Re(c)^0.25), so -0.25 b / Re(c)"
    cr = np.asarray(c).real.astype(np.float64).ravel()
    return -0.25 / (310. * cr ** 0.25) / cr


def viscoChain(c, Q, lam=0.0, dtype=np.complex128, magnitude=False):
    """(gamma, chi), each (N,): the derivatives of the complex velocity of a visco problem (distributors.ViscoMultiFreq.spUpdates),

        c~ = c (1 + lam q) (1 + i q / 2),     q = 1 / Q,     lam = ln(f / freqBase) / pi  (0 without dispersion),

    with respect to the real velocity c and to the quality factor Q per cell:

        gamma = d c~ / d c = (1 + lam q) (1 + i q / 2),      chi = d c~ / d Q = -c~ q^2 [ lam / (1 + lam q) + (i / 2) / (1 + i q / 2) ]

    Every coefficient of MiniZephyr with an explicit density is holomorphic in c~, so the derivative of A along real (dc, dQ) is the derivative along the
    complex perturbation gamma dc + chi dQ.  Evaluated through q: Q = inf gives gamma = 1, chi = 0 with no infinity in any product.  dtype np.clongdouble: in
    80-bit arithmetic.  magnitude: moduli, every sum a sum of moduli -- what bounds the rounding of the evaluation per component."""
    R = _real(dtype)
    cr = np.asarray(c).real.astype(R).ravel()
    q = 1 / np.broadcast_to(np.asarray(Q, dtype=np.float64).ravel(), cr.shape).astype(R)
    lam = R(lam)
    half = dtype(0.5j)
    if magnitude:
        gamma = (1 + abs(lam) * q) * (1 + q / 2)
        return gamma, (np.abs(cr) * gamma) * (q * q) * (abs(lam) / np.abs(1 + lam * q) + R(0.5) / np.abs(1 + half * q))
    disp, att = 1 + lam * q, 1 + half * q
    gamma = disp * att
    return gamma, -(cr * gamma) * (q * q) * (lam / disp + half / att)


def _rhoGrid(op):
    'the density of the operator as float64 (nz, nx): a scalar broadcast, an (nz, nx) array as it is, a flat one of nz nx entries (a multiscale sub-problem) reshaped'
    nz, nx = int(op.nz), int(op.nx)
    rho = np.asarray(op.rho, dtype=np.float64)
    return rho.reshape((nz, nx)) if rho.size == nz * nx else np.broadcast_to(rho, (nz, nx))


def _buoyancy(op, R):
    "b = 1 / rho (nz, nx) at the density the operator is assembled with (its config's, or the Gardner default)"
    return 1 / _rhoGrid(op).astype(R)


def _perturbation(dc, R, dtype, shape):
    """a velocity perturbation in the arithmetic of dtype: a real one is cast to the real type R as it always was; a complex one (the perturbation of the
    complex velocity of a visco problem, `viscoChain`) keeps both parts -- the row factors and kappa are holomorphic in c, so the same formulas hold"""
    dc = np.asarray(dc)
    return dc.astype(dtype if np.iscomplexobj(dc) else R).reshape(shape)


def velocityPlanes(op, dc, db=None, dtype=np.complex128, magnitude=False):
    """The nine planes (9, nz, nx) of d A / d c along the real velocity perturbation dc (N,), boundary rows zero, for the 2-D MiniZephyr operator `op`:
    mass term and PML stretch at the density of the operator.  db (N,): the buoyancy perturbation that goes with dc (gardnerChain(c) dc where the density
    follows c), whose planes `buoyancyPlanes(op, db)` are added.  magnitude: the same sum with every term replaced by its modulus.
    dc complex (explicit density only, db None): the derivative along that perturbation of a complex velocity, what a visco problem applies."""
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    v = _perturbation(dc, R, dtype, (nz, nx))
    b = _buoyancy(op, R)
    drow = [x * v for x in rowFactorsDc(op, dtype, magnitude)]
    dkb = massWeightDc(op, dtype) * b * v
    t, tzx = _stiffness(op, drow, magnitude)
    C = _starPlanes(t, tzx, b, np.abs(dkb) if magnitude else dkb, R, dtype, magnitude)
    return C if db is None else C + buoyancyPlanes(op, db, dtype, magnitude)


def velocityAdjoint(op, P, dtype=np.complex128, magnitude=False, conj=False, stretch=True):
    """V^T P: (N,) with <velocityPlanes(op, dc), P> = <dc, V^T P> under the bilinear pairing sum_k sum_i (no conjugate), P (9, N) or (9, nz, nx) complex; its
    boundary rows are not read.  Cell j takes (d kappa_j / dc) b_j times the mass weights from the planes of the rows around it, and from its own row the
    differentiated stiffness factors times the averaged buoyancies.  conj: conj(V)^T P.  magnitude: the sum of the moduli of the terms.  stretch False: the
    transpose of `massPlanes`, the mass term alone."""
    return _rowAdjoint(op, P, rowFactorsDc(op, dtype, magnitude), massWeightDc(op, dtype), dtype, magnitude, conj, stretch)


def _rowAdjoint(op, P, drow, dkappa, dtype, magnitude, conj, stretch, b=None):
    """the transpose of dc -> star(dc_i drow_i, bn[b], Kn_k = dkappa_j b_j dc_j) applied to the planes P, (N,): `velocityAdjoint` with the first derivatives of the row
    factors and of kappa, the per-cell factor of `velocityCurvature` with the second ones.  b (nz, nx): the field in the place of the buoyancy of the operator
    (`mixedAdjointC`; its moduli with magnitude)."""
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    b = _buoyancy(op, R) if b is None else b
    w = dkappa * b
    if conj:
        drow, w = tuple(np.conj(x) for x in drow), np.conj(w)
    t, tzx = _stiffness(op, drow, magnitude)
    Pl = np.asarray(P).astype(dtype).reshape((9, nz, nx)).copy()
    Pl[:, ~_interiorMask(nz, nx)] = 0
    if magnitude:
        Pl, w = np.abs(Pl), np.abs(w)
    slot = {o: k for k, o in enumerate(LAGS)}
    sgn = 1 if magnitude else -1
    mc, md, me = [R(x) for x in MZ_MASS]
    mass = mc * Pl[4]
    stiff = np.zeros((nz, nx), dtype=Pl.dtype)
    for o in LAGS:
        if o == (0, 0):
            continue
        sz, sx = o
        q = t[o] * (Pl[slot[o]] + sgn * Pl[4])
        if sz and sx:
            q = q + tzx * (Pl[slot[(sz, 0)]] + sgn * Pl[slot[(0, sx)]])
        stiff = stiff + (b + _at(b, sz, sx)) / 2 * q             # (zero on the boundary lines: the planes are zero there)
        mass = mass + (me if sz and sx else md) * _at(Pl[slot[o]], -sz, -sx)
    return (stiff + w * mass).ravel() if stretch else (w * mass).ravel()


# ---- the second derivative of the operator: what the full Newton Hessian adds to J^T J ---------------------------------------------------------------------
# With an explicit density a row is star(row_i(c_i), bn, Kn_k = kappa(c_j) b_j) and the star has no product of a row factor with a mass term, so
# d^2 A / dc_i dc_j = 0 for i != j: the second derivative along (p, q) is star(p_i q_i d^2 row_i / dc^2, bn[b], Kn_k = (d^2 kappa_j / dc^2) b_j p_j q_j)
# (`velocityPlanes2`), and its contraction with nine lag products is local to a cell (`velocityCurvature`; k_velocity_curvature, csrc/survey_newton.hip).  Where the
# density follows c (Gardner) b_j(c_j) multiplies row_i(c_i) in the averages and the mixed derivative is not zero: not built.

def velocityPlanes2(op, dc, dc2=None, dtype=np.complex128, magnitude=False, stretch=True):
    """The nine planes (9, nz, nx) of the second derivative of A along the real velocity perturbations dc and dc2 (default dc again) at the density of the operator,
    boundary rows zero: d/dh of velocityPlanes(op at c + h dc2, dc) at h = 0.  stretch False: the mass term alone, the derivative of `massPlanes`."""
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    v = np.asarray(dc).astype(R).reshape((nz, nx)) * np.asarray(dc if dc2 is None else dc2).astype(R).reshape((nz, nx))
    if magnitude:
        v = np.abs(v)
    b = _buoyancy(op, R)
    d2row = [x * (v if stretch else 0 * v) for x in rowFactorsD2c(op, dtype, magnitude)]
    d2kb = massWeightD2c(op, dtype) * b * v
    t, tzx = _stiffness(op, d2row, magnitude)
    return _starPlanes(t, tzx, b, np.abs(d2kb) if magnitude else d2kb, R, dtype, magnitude)


def velocityCurvature(op, P, p, conj=False, stretch=True, dtype=np.complex128, magnitude=False):
    """(N,): w with <dc2, w> = <velocityPlanes2(op, p, dc2), P> under the bilinear pairing for every dc2 -- the third term of the Newton Hessian-vector product,
    p_j [(d^2 kappa_j / dc^2) b_j (the mass gather of P at j) + (the stretch part of `velocityAdjoint` with d^2 row_j / dc^2)].  P (9, N) or (9, nz, nx) complex, its
    boundary rows not read; p (N,) real.  conj: the conjugated coefficients.  stretch False: the mass term alone.  magnitude: the sum of the moduli of the terms."""
    R = _real(dtype)
    v = np.asarray(p).astype(R).ravel()
    return (np.abs(v) if magnitude else v) * _rowAdjoint(op, P, rowFactorsD2c(op, dtype, magnitude), massWeightD2c(op, dtype), dtype, magnitude, conj, stretch)


# ---- the mixed second derivative with respect to velocity and buoyancy: what couples the two halves of a joint (c, rho) Newton product ------------------------
# A row star(row_i(c_i), bn[b], Kn_k = kappa(c_j) b_j) is bilinear in (row, bn) and linear in Kn, so d^2 A / db^2 = 0 and along a velocity perturbation p and a
# buoyancy perturbation beta
#     d^2 A / dc db [p, beta] = star(p_i d row_i / dc, bn[beta], Kn_k = (d kappa_j / dc) beta_j p_j)
# -- `velocityPlanes` with beta in the place of the buoyancy (`mixedPlanes`).  Its transpose in p is `velocityAdjoint` with beta for b (`mixedAdjointC`, local to
# a cell but for the mass gather); its transpose in beta is `buoyancyAdjoint` with the stiffness factors of ROW i replaced by p_i d row_i / dc and kappa_j by
# (d kappa_j / dc) p_j (`mixedAdjointB`: cell j sees p at the eight rows around it).  k_velocity_adjoint_b / k_mixed_adjoint (csrc/survey_joint.hip).

def mixedPlanes(op, dc, db, stretch=True, dtype=np.complex128, magnitude=False):
    """The nine planes (9, nz, nx) of d^2 A / dc db along the real velocity perturbation dc and the real buoyancy perturbation db (N,) each, any sign, boundary rows
    zero: d/dh of buoyancyPlanes(op at c + h dc, db) at h = 0.  stretch False: the mass term alone.  magnitude: every term by its modulus."""
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    v = np.asarray(dc).astype(R).reshape((nz, nx))
    beta = np.asarray(db).astype(R).reshape((nz, nx))
    if magnitude:
        v, beta = np.abs(v), np.abs(beta)
    drow = [x * (v if stretch else 0 * v) for x in rowFactorsDc(op, dtype, magnitude)]
    dkb = massWeightDc(op, dtype) * beta * v
    t, tzx = _stiffness(op, drow, magnitude)
    return _starPlanes(t, tzx, beta, np.abs(dkb) if magnitude else dkb, R, dtype, magnitude)


def mixedAdjointC(op, P, db, conj=False, stretch=True, dtype=np.complex128, magnitude=False):
    """M_c^T[db] P: (N,) with <mixedPlanes(op, dc, db), P> = <dc, M_c^T[db] P> under the bilinear pairing for every dc -- `velocityAdjoint` with db (N,) real, any
    sign, in the place of the buoyancy.  P (9, N) or (9, nz, nx) complex, its boundary rows not read.  conj: the conjugated coefficients.  stretch False: the mass
    term alone.  magnitude: the sum of the moduli of the terms."""
    R = _real(dtype)
    beta = np.asarray(db).astype(R).reshape((int(op.nz), int(op.nx)))
    return _rowAdjoint(op, P, rowFactorsDc(op, dtype, magnitude), massWeightDc(op, dtype), dtype, magnitude, conj, stretch, b=np.abs(beta) if magnitude else beta)


def mixedAdjointB(op, P, dc, conj=False, stretch=True, dtype=np.complex128, magnitude=False):
    """M_b^T[dc] P: (N,) with <mixedPlanes(op, dc, db), P> = <db, M_b^T[dc] P> under the bilinear pairing for every db -- `buoyancyAdjoint` with the stiffness factors
    of row i replaced by dc_i d row_i / dc and kappa_j by (d kappa_j / dc) dc_j; not local: cell j sees dc at the eight rows around it.  Arguments as
    `mixedAdjointC`, dc (N,) real."""
    R = _real(dtype)
    v = np.asarray(dc).astype(R).reshape((int(op.nz), int(op.nx)))
    if magnitude:
        v = np.abs(v)
    drow = [x * (v if stretch else 0 * v) for x in rowFactorsDc(op, dtype, magnitude)]
    return _buoyancyGather(op, P, drow, massWeightDc(op, dtype) * v, dtype, magnitude, conj)


def applyPlanesTransposed(C, U, nz=None, nx=None, magnitude=False):
    """(dA)^T U column by column of U ((N,) or (N, k)) from the planes C (9, nz, nx) (or (9, N) with nz, nx given) of dA, cells outside the grid contributing
    nothing: sum_k CT_k (.) U(i + off_k) with CT_k[i] = C_(8-k)[i + off_k], the transposed plane set, which is never formed.  magnitude: every term by its modulus."""
    if nz is None:
        nz, nx = np.shape(C)[1:3]
    nz, nx = int(nz), int(nx)
    a = np.asarray(U).reshape((nz, nx) + np.shape(U)[1:])
    Cb = np.asarray(C).reshape((9, nz, nx) + (1,) * (a.ndim - 2))
    if magnitude:
        a, Cb = np.abs(a), np.abs(Cb)
    out = np.zeros(a.shape, dtype=np.result_type(a.dtype, Cb.dtype))
    for k, (sz, sx) in enumerate(LAGS):
        out = out + _at(Cb[8 - k] * a, sz, sx)
    return out.reshape(np.shape(U))


# ---- the pseudo-Hessian diagonal of the exact derivatives ------------------------------------------------------------------------------------------
# H_p[i] = sum_s || (d A / d p_i) u_s ||^2 (Shin, Jang & Min 2001, on the operator that is differentiated).  A unit perturbation of cell i touches only the
# rows of the 3 x 3 block around i, and in those only the lags that point back into the block, so cells with equal (iz mod 3, ix mod 3) have disjoint
# supports: the planes of the nine colour indicators, `applyPlanes`, |.|^2 and a 3 x 3 box sum give H exactly.  k_pseudo_hessian (csrc/survey_hessian.hip) is the
# device kernel; it builds the per-cell coefficients instead.

def _boxSum(e, nz, nx):
    "sum of e (nz, nx) over the 3 x 3 block around every cell, cells outside the grid contributing nothing; the nine lags in the order of LAGS"
    out = np.zeros_like(e)
    for sz, sx in LAGS:
        out = out + _at(e, sz, sx)
    return out


def colourSum(nz, nx, planes, u, magnitude=False, box=True):
    """H[i] = sum_s sum_j |((d A)_i u_s)[j]|^2 over the rows j of the 3 x 3 block around i (box False: row i alone) from planes(v) -> (9, nz, nx), the planes of
    d A along the field v, evaluated on the nine colour indicators.  u (N, nsrc) in the arithmetic the planes are in; magnitude: u >= 0 real and the planes
    those of moduli, the squares plain."""
    N = nz * nx
    iz, ix = np.divmod(np.arange(N), nx)
    H = None
    for a in range(3):
        for b in range(3):
            mine = (iz % 3 == a) & (ix % 3 == b)
            if not mine.any():
                continue
            r = applyPlanes(planes(mine.astype(np.float64)), u, nz, nx)
            e = (np.square(r) if magnitude else np.square(r.real) + np.square(r.imag)).sum(axis=1).reshape((nz, nx))
            if box:
                e = _boxSum(e, nz, nx)
            H = np.zeros(N, dtype=e.dtype) if H is None else H
            H[mine] = e.ravel()[mine]
    return H


def pseudoHessianDiagonal(op, u, parameter='c', chain=None, dtype=np.complex128, magnitude=False):
    """H (N,), real in the arithmetic of dtype: H[i] = sum_s || (d A / d p_i) u_s ||_2^2 for the 2-D MiniZephyr operator `op` and the columns u (N,) or
    (N, nsrc) -- the unscaled solves u^, not the stored conjugates.  parameter 'c': the planes of `velocityPlanes` (mass term and PML stretch at the density of
    the operator; chain (N,) = d b / d c where the density follows c, whose buoyancy planes are added).  parameter 'b': those of `buoyancyPlanes`; 'rho':
    along -e_i / rho_i^2, i.e. H_b[i] / rho_i^4, in density units.  magnitude: sum_s sum_j (sum_n |E_i[j][n]| |u_s[n]|)^2, what bounds the rounding of the sum."""
    if parameter not in ('c', 'rho', 'b'):
        raise ValueError('parameter is %r: \'c\', \'rho\' or \'b\'' % (parameter,))
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    ua = np.asarray(u).reshape((nz * nx, -1))
    ua = np.abs(ua.astype(dtype)).astype(R) if magnitude else ua.astype(dtype)
    if parameter == 'c':
        ch = None if chain is None else np.asarray(chain, dtype=np.float64).ravel()
        planes = lambda v: velocityPlanes(op, v, None if ch is None else ch * v, dtype, magnitude)
    else:
        planes = lambda v: buoyancyPlanes(op, v, dtype, magnitude)
    H = colourSum(nz, nx, planes, ua, magnitude)
    if parameter == 'rho':
        rho = _rhoGrid(op).astype(R).ravel()
        H = H / (rho * rho * rho * rho)
    return H


def massWeightSquares(nz, nx):
    "S (N,) float64: the sum of m_k^2 over the interior rows of the 3 x 3 block around every cell, m the mass weights (centre, edges, corners)"
    nz, nx = int(nz), int(nx)
    inside = _interiorMask(nz, nx).astype(np.float64)
    mc, md, me = MZ_MASS
    S = np.zeros((nz, nx))
    for sz, sx in LAGS:
        m = mc if (sz, sx) == (0, 0) else (md if sz == 0 or sx == 0 else me)
        S = S + (m * m) * _at(inside, sz, sx)
    return S.ravel()


def operatorPseudoHessianWeight(op):
    """|w_i|^2 S_i, float64 (N,): the pseudo-Hessian diagonal of the mass term alone (linearisation='operator', parameter='c') is this times sum_s |u_s[i]|^2.
    (dA) u = mask_int M0(w e_i u) puts m_k w_i u[i] into the interior rows of the block around i: w = `operatorWeight`, S = `massWeightSquares`."""
    w = operatorWeight(op)
    return (np.square(w.real) + np.square(w.imag)) * massWeightSquares(op.nz, op.nx)


# ---- the exact diagonal of the Gauss-Newton Hessian ------------------------------------------------------------------------------------------------
# H[i] = sum_s sum_r |g_r^T E_i u_s|^2 with E_i = d A / d p_i, u_s = A^-1 premul q_s and g_r = A^-T R_r^H the receiver Green's functions.  E_i lives on the rows
# and columns of the 3 x 3 block around i (the section above), so with Gamma_i[j, j'] = sum_r g_r[j] conj(g_r[j']) and Phi_i[n, n'] = sum_s u_s[n] conj(u_s[n'])
# over the cells of that block
#     H[i] = Re sum_(j, n, j', n') conj(E_i[j', n']) Gamma_i[j, j'] E_i[j, n] Phi_i[n, n'] = Re tr(E^H Gamma^T E Phi).
# Two cells of a block are at most two steps apart in either direction: Gamma and Phi are read off the autocorrelation planes at the 25 lags of (-2..2)^2, 13 of
# which are stored (`lagGram`; the others are conjugates read at the shifted cell).  k_lag_gram and k_gauss_newton_diagonal (csrc/survey_hessian.hip) are the device
# kernels; conjugating both sets of planes and the coefficients together leaves H as it is, which is how they read the stored conjugates.
GRAM_LAGS = [(0, 0), (0, 1), (0, 2)] + [(dz, dx) for dz in (1, 2) for dx in (-2, -1, 0, 1, 2)]      # the stored half plane: plane l pairs cell i with i + GRAM_LAGS[l]


def lagGram(u, nz, nx, dtype=np.complex128, magnitude=False):
    """C (13, N): C[l][i] = sum_s u[i, s] conj(u[i + off_l, s]) for the 13 lags of GRAM_LAGS, zero where i + off_l is outside the grid.  u (N,) or (N, ncols).
    magnitude: sum_s |u[i, s]| |u[i + off_l, s]|, real."""
    nz, nx = int(nz), int(nx)
    ua = np.asarray(u).reshape((nz, nx, -1)).astype(dtype)
    if magnitude:
        ua = np.abs(ua)
    C = np.zeros((len(GRAM_LAGS), nz, nx), dtype=ua.dtype)
    for l, (dz, dx) in enumerate(GRAM_LAGS):
        C[l] = (ua * np.conj(_at(ua, dz, dx))).sum(axis=2)
    return C.reshape((len(GRAM_LAGS), nz * nx))


def _gramBlocks(C, nz, nx):
    "B (N, 9, 9): B[i, p, q] = sum_s u[i + o_p] conj(u[i + o_q]) over the slots of LAGS from the planes of `lagGram`; zero where either cell is outside the grid"
    Cl = np.asarray(C).reshape((len(GRAM_LAGS), nz, nx))
    where = {o: l for l, o in enumerate(GRAM_LAGS)}
    B = np.zeros((nz, nx, 9, 9), dtype=Cl.dtype)
    for p, (pz, px) in enumerate(LAGS):
        for q, (qz, qx) in enumerate(LAGS):
            lag = (qz - pz, qx - px)
            if lag in where:
                B[:, :, p, q] = _at(Cl[where[lag]], pz, px)
            else:
                B[:, :, p, q] = np.conj(_at(Cl[where[(-lag[0], -lag[1])]], qz, qx))
    return B.reshape((nz * nx, 9, 9))


def massPlanes(op, dc, dtype=np.complex128, magnitude=False):
    "the nine planes of linearisation='operator': the mass terms m_k (d kappa / dc) b dc of the neighbouring cell alone (`velocityPlanes` without the stretch)"
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    dkb = massWeightDc(op, dtype) * _buoyancy(op, R) * _perturbation(dc, R, dtype, (nz, nx))          # (dc complex: as `velocityPlanes`)
    if magnitude:
        dkb = np.abs(dkb)
    mc, md, me = [R(w) for w in MZ_MASS]
    C = np.zeros((9, nz, nx), dtype=dkb.dtype)
    for k, (sz, sx) in enumerate(LAGS):
        C[k] = (mc if (sz, sx) == (0, 0) else (me if sz and sx else md)) * _at(dkb, sz, sx)
    C[:, ~_interiorMask(nz, nx)] = 0
    return C


def blockCoefficients(nz, nx, planes):
    """E (N, 9, 9): E[i, j, n] the coefficient of d A / d p_i in row i + o_j at column i + o_n (slots of LAGS), from planes(v) -> (9, nz, nx) evaluated on the
    nine colour indicators (cells with equal (iz mod 3, ix mod 3) have disjoint 3 x 3 blocks)"""
    N = nz * nx
    iz, ix = np.divmod(np.arange(N), nx)
    slot = {o: k for k, o in enumerate(LAGS)}
    E = None
    for a in range(3):
        for b in range(3):
            mine = (iz % 3 == a) & (ix % 3 == b)
            if not mine.any():
                continue
            C = np.asarray(planes(mine.astype(np.float64))).reshape((9, nz, nx))
            E = np.zeros((N, 9, 9), dtype=C.dtype) if E is None else E
            for j, (jz, jx) in enumerate(LAGS):
                for n, (mz, mx) in enumerate(LAGS):
                    k = slot.get((mz - jz, mx - jx))
                    if k is not None:
                        E[mine, j, n] = _at(C[k], jz, jx).ravel()[mine]
    return E


def gaussNewtonTrace(E, Gamma, Phi, magnitude=False):
    "Re sum conj(E[j', n']) Gamma[j, j'] E[j, n] Phi[n, n'] per cell from (N, 9, 9) blocks, as T = E Phi, S = Gamma^T T, sum conj(E) S; magnitude: every term by its modulus"
    if magnitude:
        E, Gamma, Phi = np.abs(E), np.abs(Gamma), np.abs(Phi)
    T = np.einsum('ijn,inm->ijm', E, Phi)
    S = np.einsum('ijk,ijm->ikm', Gamma, T)
    return (np.conj(E) * S).sum(axis=(1, 2)).real


def gaussNewtonDiagonal(op, uh, gh, parameter='c', chain=None, linearisation='full', dtype=np.complex128, magnitude=False, weight=None):
    """H (N,), real in the arithmetic of dtype: H[i] = sum_s sum_r |g_r^T (d A / d p_i) u_s|^2 for the 2-D MiniZephyr operator `op` from the planes
    uh = lagGram(u) of the forward solves and gh = lagGram(g) of the receiver Green's functions (13, N) each.  linearisation 'full': d A / d p_i from
    `velocityPlanes` (chain (N,) = d b / d c where the density follows c) for parameter 'c', from `buoyancyPlanes` for 'b' and 'rho' ('rho': along
    -e_i / rho_i^2, density units); 'operator' with 'c': the mass term alone (`massPlanes`); 'scaler': the diagonal weight `weight` (N,), default the
    reference's -(2 pi f)^2 / c^3, so H = |w|^2 gh[0] uh[0].  magnitude: uh and gh those of moduli, every term of the trace by its modulus."""
    if parameter not in ('c', 'rho', 'b'):
        raise ValueError('parameter is %r: \'c\', \'rho\' or \'b\'' % (parameter,))
    if linearisation not in ('scaler', 'operator', 'full'):
        raise ValueError('linearisation is %r: \'scaler\', \'operator\' or \'full\'' % (linearisation,))
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    Cu = (np.abs(np.asarray(uh)).astype(R) if magnitude else np.asarray(uh).astype(dtype)).reshape((len(GRAM_LAGS), nz * nx))
    Cg = (np.abs(np.asarray(gh)).astype(R) if magnitude else np.asarray(gh).astype(dtype)).reshape((len(GRAM_LAGS), nz * nx))
    if linearisation == 'scaler':
        if weight is None:
            om = 2 * R(np.pi) * dtype(complex(op.freq))
            c = np.asarray(op.c).astype(dtype).ravel()
            weight = -(om * om) / (c * c * c)
        w = np.asarray(weight).astype(dtype).ravel()
        return (np.square(w.real) + np.square(w.imag)) * (Cg[0].real * Cu[0].real)
    if parameter != 'c':
        planes = lambda v: buoyancyPlanes(op, v, dtype, magnitude)
    elif linearisation == 'operator':
        planes = lambda v: massPlanes(op, v, dtype, magnitude)
    else:
        ch = None if chain is None else np.asarray(chain, dtype=np.float64).ravel()
        planes = lambda v: velocityPlanes(op, v, None if ch is None else ch * v, dtype, magnitude)
    H = gaussNewtonTrace(blockCoefficients(nz, nx, planes), _gramBlocks(Cg, nz, nx), _gramBlocks(Cu, nz, nx), magnitude)
    if parameter == 'rho':
        rho = _rhoGrid(op).astype(R).ravel()
        H = H / (rho * rho * rho * rho)
    return H


# ---- the per-cell 2 x 2 blocks of the joint (c, rho) Hessian ------------------------------------------------------------------------------------------
# With E^c_i = d A / d c_i (velocityPlanes at the operator's density for 'full', massPlanes for 'operator') and E^b_i = d A / d b_i (buoyancyPlanes), the block of
# cell i is the 2 x 2 Gram matrix of the pair: rows cc, cb, bb, in density units cc, -cb / rho_i^2, bb / rho_i^4 (d b / d rho = -1 / rho^2).  Both kinds use
# what the diagonals above use; only the cross term is new.  k_gauss_newton_blocks and k_pseudo_hessian_blocks (csrc/survey_hessian.hip) are the device kernels.

def gaussNewtonCrossTrace(Ea, Gamma, Eb, Phi, magnitude=False):
    """Re sum conj(Ea[j', n']) Gamma[j, j'] Eb[j, n] Phi[n, n'] per cell from (N, 9, 9) blocks, as T = Eb Phi, S = Gamma^T T, sum conj(Ea) S: the two-sided form
    of `gaussNewtonTrace`, symmetric in (Ea, Eb) for Hermitian Gamma and Phi; magnitude: every term by its modulus"""
    if magnitude:
        Ea, Eb, Gamma, Phi = np.abs(Ea), np.abs(Eb), np.abs(Gamma), np.abs(Phi)
    T = np.einsum('ijn,inm->ijm', Eb, Phi)
    S = np.einsum('ijk,ijm->ikm', Gamma, T)
    return (np.conj(Ea) * S).sum(axis=(1, 2)).real


def _checkBlocksLinearisation(linearisation):
    if linearisation not in ('operator', 'full'):
        raise ValueError('linearisation is %r: the (c, rho) blocks serve \'operator\' or \'full\' (the reference has no scaler for the density)' % (linearisation,))


def _densityRows(op, cc, cb, bb, R, magnitude):
    "(3, N): the (c, b) entries of a block in density units, rows cc, -cb / rho^2, bb / rho^4 (magnitude: +cb / rho^2)"
    rho = _rhoGrid(op).astype(R).ravel()
    r2 = rho * rho
    return np.stack([cc, (cb if magnitude else -cb) / r2, bb / (r2 * r2)])


def gaussNewtonBlocks(op, uh, gh, linearisation='full', dtype=np.complex128, magnitude=False):
    """B (3, N), real in the arithmetic of dtype: the 2 x 2 block of the Gauss-Newton Hessian of the pair (c_i, rho_i) per cell, rows H_cc, H_crho, H_rhorho,
        B[a, b][i] = sum_s sum_r Re conj(g_r^T E^a_i u_s) (g_r^T E^b_i u_s) = Re tr(E^a_i^H Gamma_i E^b_i Phi_i)
    from the planes uh = lagGram(u), gh = lagGram(g) of `gaussNewtonDiagonal`.  E^c_i from `velocityPlanes` at the density of the operator ('full') or
    `massPlanes` ('operator'); E^rho_i = -E^b_i / rho_i^2 with E^b_i from `buoyancyPlanes`.  Rows 0 and 2 are gaussNewtonDiagonal(parameter='c' / 'rho').
    magnitude: uh and gh those of moduli, every term by its modulus (the cross term too: +1 / rho^2)."""
    _checkBlocksLinearisation(linearisation)
    nz, nx = int(op.nz), int(op.nx)
    R = _real(dtype)
    Cu = (np.abs(np.asarray(uh)).astype(R) if magnitude else np.asarray(uh).astype(dtype)).reshape((len(GRAM_LAGS), nz * nx))
    Cg = (np.abs(np.asarray(gh)).astype(R) if magnitude else np.asarray(gh).astype(dtype)).reshape((len(GRAM_LAGS), nz * nx))
    if linearisation == 'operator':
        Ec = blockCoefficients(nz, nx, lambda v: massPlanes(op, v, dtype, magnitude))
    else:
        Ec = blockCoefficients(nz, nx, lambda v: velocityPlanes(op, v, None, dtype, magnitude))
    Eb = blockCoefficients(nz, nx, lambda v: buoyancyPlanes(op, v, dtype, magnitude))
    Gamma, Phi = _gramBlocks(Cg, nz, nx), _gramBlocks(Cu, nz, nx)
    cc = gaussNewtonCrossTrace(Ec, Gamma, Ec, Phi, magnitude)
    cb = gaussNewtonCrossTrace(Ec, Gamma, Eb, Phi, magnitude)
    bb = gaussNewtonCrossTrace(Eb, Gamma, Eb, Phi, magnitude)
    return _densityRows(op, cc, cb, bb, R, magnitude)


def pseudoHessianBlocks(op, u, linearisation='full', dtype=np.complex128, magnitude=False):
    """B (3, N), real in the arithmetic of dtype: the 2 x 2 block of the pseudo-Hessian of the pair (c_i, rho_i) per cell, rows H_cc, H_crho, H_rhorho,
        B[a, b][i] = sum_s Re <E^a_i u_s, E^b_i u_s>,
    the inner product over the rows of the 3 x 3 block around i; u (N,) or (N, nsrc) the unscaled solves.  E^c, E^rho as for `gaussNewtonBlocks`: it is that
    block with Gamma the identity.  Rows 0 and 2 are pseudoHessianDiagonal(parameter='c' / 'rho') ('operator': the closed form of
    `operatorPseudoHessianWeight`).  Evaluated on the nine colour indicators.  magnitude: every term by its modulus (the cross term too: +1 / rho^2)."""
    _checkBlocksLinearisation(linearisation)
    nz, nx = int(op.nz), int(op.nx)
    N = nz * nx
    R = _real(dtype)
    ua = np.asarray(u).reshape((N, -1))
    ua = np.abs(ua.astype(dtype)).astype(R) if magnitude else ua.astype(dtype)
    if linearisation == 'operator':
        planesC = lambda v: massPlanes(op, v, dtype, magnitude)
    else:
        planesC = lambda v: velocityPlanes(op, v, None, dtype, magnitude)
    iz, ix = np.divmod(np.arange(N), nx)
    out = np.zeros((3, N), dtype=R)
    for a in range(3):
        for b in range(3):
            mine = (iz % 3 == a) & (ix % 3 == b)
            if not mine.any():
                continue
            ind = mine.astype(np.float64)
            rc = applyPlanes(planesC(ind), ua, nz, nx)
            rb = applyPlanes(buoyancyPlanes(op, ind, dtype, magnitude), ua, nz, nx)
            if magnitude:
                terms = (rc * rc, rc * rb, rb * rb)
            else:
                terms = (np.square(rc.real) + np.square(rc.imag), rc.real * rb.real + rc.imag * rb.imag, np.square(rb.real) + np.square(rb.imag))
            for k, e in enumerate(terms):
                out[k, mine] = _boxSum(e.sum(axis=1).reshape((nz, nx)), nz, nx).ravel()[mine]
    return _densityRows(op, out[0], out[1], out[2], R, magnitude)


def blockSolve(B, g, damping):
    """z (2N,) float64: the stacked gradient g = [g_c; g_rho] (2N,) divided by the per-cell 2 x 2 blocks B (3, N) of `hessianBlocks`, cell by cell
        [[B0 + l_c, B1], [B1, B2 + l_rho]] z_i = [g_c[i]; g_rho[i]],     l_c = damping max(B0), l_rho = damping max(B2).
    damping must be > 0: blocks that are exactly zero exist (boundary cells), and with it every block is positive definite (a Gram matrix plus a positive
    diagonal).  With B1 = 0 this is g / (H + damping H.max()) one parameter at a time."""
    B = np.asarray(B, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] != 3:
        raise ValueError('B has shape %r: (3, N), the rows H_cc, H_crho, H_rhorho of hessianBlocks' % (B.shape,))
    N = B.shape[1]
    if g.ndim != 1 or g.size != 2 * N:
        raise ValueError('g has shape %r: the stacked vector [g_c; g_rho] of %d entries' % (g.shape, 2 * N))
    if not (np.ndim(damping) == 0 and float(damping) > 0.0 and np.isfinite(float(damping))):
        raise ValueError('damping is %r: a positive number (exactly zero blocks exist, so the undamped blocks are singular)' % (damping,))
    if not (np.all(np.isfinite(B)) and np.all(np.isfinite(g))):
        raise ValueError('B and g must be finite')
    lc, lr = float(damping) * (B[0].max() if N else 0.0), float(damping) * (B[2].max() if N else 0.0)
    if N and not (lc > 0.0 and lr > 0.0):
        raise ValueError('max(B[0]) = %g, max(B[2]) = %g: both diagonals need a positive entry for the damping to act' % (B[0].max(), B[2].max()))
    a, b, d = B[0] + lc, B[1], B[2] + lr
    det = a * d - b * b
    gc, gr = g[:N], g[N:]
    return np.concatenate([(d * gc - b * gr) / det, (a * gr - b * gc) / det])


# ---- the derivative maps of the Eurus block M1 (eps == delta) ---------------------------------------------------------------------------------------------
# Written out from the assembly (eurus.py:28-485; csrc/eu_row.hpp eu_m1_row).  A row of M1 is linear and homogeneous in the buoyancies b = 1 / rho and the mass
# terms K = omega_d^2 b / c^2 of the 3 x 3 cells around it (edge-clamped: a neighbour outside the grid is the nearest cell inside); its C-PML averages are 1-D
# functions of cPML and omega_d and do not depend on the model, theta and delta of the row's own cell are coefficients.  The entry built from the property
# neighbour (sz, sx) lies in the matrix slot (-sz, sx), the reference's z-flipped ordering.  The four boundary lines keep their centre entry EE alone -- which
# depends on the model, unlike MiniZephyr's +-identity.  Along real (dc, db):
#     dC = V[dc] + L[db],    L[db] = row(b -> db, K -> omega_d^2 db / c^2),    V[dc] = the mass entries at K -> -2 omega_d^2 b dc / c^3
# `eurusPlanes` is the map, `eurusAdjoint` the plain transposes of both halves; k_eurus_planes / k_eurus_adjoint (csrc/survey_eurus.hip) are the device kernels.
EU_MASS = (0.6287326, 0.25 * 0.3712667, 0.25 * (1.0 - 0.6287326 - 0.3712667))      # centre, edge, corner (eurus.py:229-269)
EU_W1 = 0.4382634                                                                 # the blend of the rotated and the plain stiffness star


def _euGamma(n, npml, h, cpml):
    'the C-PML damping profile along an axis in float64, as the library makes it (eurus.py:77-91)'
    L = h * (npml - 1)
    vals = np.arange(npml) * h
    g = np.zeros(n)
    g[:npml] = cpml * np.cos((np.pi / 2) * (vals / L))
    g[n - npml:] = cpml * np.cos((np.pi / 2) * (vals[::-1] / L))
    return g


def _euSetup(op, dtype):
    """what a row of M1 takes from the operator alone, in the arithmetic of dtype: (c, b, om2, pml, tti) with c (nz, nx) complex, b = 1 / rho, om2 = omega_d^2, pml
    the dict of the averages xM, xP, zM, zP, xC, zC and the factors Lx4, Lx, Lz4, Lz broadcast over the grid, tti = (Ax, Bx, Bz) of the row's own theta, delta"""
    R = _real(dtype)
    nz, nx, npml = int(op.nz), int(op.nx), int(op.nPML)
    c = np.asarray(op.c).astype(dtype).reshape((nz, nx))
    b = 1 / np.asarray(op.rho).astype(R).reshape((nz, nx))
    f = complex(op.freq)
    om = 2 * R(np.pi) * (R(f.real) + dtype(1j) * R(f.imag))
    tau = float(op.tau)
    if np.isfinite(tau) and tau != 0.0:
        om = om - dtype(1j) / R(tau)
    dx, dz = R(float(op.dx)), R(float(op.dz))
    pad = lambda g: np.concatenate((g[:1], g, g[-1:])).astype(R)
    xi_x = 1 - (dtype(1j) * pad(_euGamma(nx, npml, float(op.dx), float(op.cPML)))) / om
    xi_z = 1 - (dtype(1j) * pad(_euGamma(nz, npml, float(op.dz), float(op.cPML)))) / om
    xC, zC = xi_x[1:-1][None, :], xi_z[1:-1][:, None]
    pml = dict(xM=((xi_x[:-2] + xi_x[1:-1]) / 2)[None, :], xP=((xi_x[1:-1] + xi_x[2:]) / 2)[None, :], xC=xC,
               zM=((xi_z[:-2] + xi_z[1:-1]) / 2)[:, None], zP=((xi_z[1:-1] + xi_z[2:]) / 2)[:, None], zC=zC,
               Lx4=1 / (4 * xC * dx * dx), Lx=1 / (xC * dx * dx), Lz4=1 / (4 * zC * dz * dz), Lz=1 / (zC * dz * dz))
    theta = np.asarray(op.theta).astype(R).reshape((nz, nx))
    delta = np.asarray(op.delta).astype(R).reshape((nz, nx))
    ct2, st2, s2t = np.cos(theta) ** 2, np.sin(theta) ** 2, np.sin(2 * theta)
    tti = (1 + (2 * delta) * ct2, (-delta) * s2t, 1 + (2 * delta) * st2)
    return c, b, om * om, pml, tti


def _euNeighbours(a):
    "{(sz, sx): a at the edge-clamped neighbour (iz + sz, ix + sx)} of a field (nz, nx)"
    nz, nx = a.shape
    p = np.pad(a, 1, mode='edge')
    return {(sz, sx): p[1 + sz:1 + sz + nz, 1 + sx:1 + sx + nx] for sz, sx in LAGS}


def _euRow(bf, Kf, pml, tti, R, dtype, magnitude, edges=True):
    """the nine planes (9, nz, nx), matrix slot order, of the rows of M1 from the buoyancy field bf and the mass-term field Kf (both (nz, nx), read at the clamped
    neighbours).  magnitude: every term by its modulus, every difference a sum.  Edge rows keep the centre entry alone (edges False: nothing).  bf None: the mass
    entries alone, what the row is at b = 0 (the stiffness is linear in b), without evaluating the stiffness."""
    nz, nx = Kf.shape
    if bf is None:
        K = _euNeighbours(np.abs(Kf) if magnitude else Kf)
        wm1, wm2, wm3 = (R(w) for w in EU_MASS)
        return _euEdgeRows({(sz, sx): (wm1 if sz == 0 and sx == 0 else wm2 if sz == 0 or sx == 0 else wm3) * K[sz, sx] for sz, sx in LAGS}, nz, nx, R, dtype, magnitude, edges)
    if magnitude:
        bf, Kf = np.abs(bf), np.abs(Kf)
        pml = {k: np.abs(v) for k, v in pml.items()}
        # (1 / |xM| is what the modulus of b / xM needs: the averages enter as divisors)
        tti = tuple(np.abs(t) for t in tti)
    s = 1 if magnitude else -1
    b, K = _euNeighbours(bf), _euNeighbours(Kf)
    xM, xP, zM, zP, xC, zC = (pml[k] for k in ('xM', 'xP', 'zM', 'zP', 'xC', 'zC'))
    Lx4, Lx, Lz4, Lz = (pml[k] for k in ('Lx4', 'Lx', 'Lz4', 'Lz'))
    sq1 = (b[1, -1] + b[1, 0] + b[0, -1] + b[0, 0]) / 4
    sq2 = (b[1, 0] + b[1, 1] + b[0, 0] + b[0, 1]) / 4
    sq3 = (b[0, -1] + b[0, 0] + b[-1, -1] + b[-1, 0]) / 4
    sq4 = (b[0, 0] + b[0, 1] + b[-1, 0] + b[-1, 1]) / 4
    s1x, s2x, s3x, s4x = sq1 / xM, sq2 / xP, sq3 / xM, sq4 / xP
    s1z, s2z, s3z, s4z = sq1 / zM, sq2 / zM, sq3 / zP, sq4 / zP
    l1, l2, l3, l4 = (b[1, 0] + b[0, 0]) / 2, (b[0, -1] + b[0, 0]) / 2, (b[0, 0] + b[0, 1]) / 2, (b[0, 0] + b[-1, 0]) / 2
    ln1, ln2, ln3, ln4 = l1 / zM, l2 / xM, l3 / xP, l4 / zP
    ln1c, ln2c, ln3c, ln4c = l1 / xC, l2 / zC, l3 / zC, l4 / xC
    wm1, wm2, wm3 = (R(w) for w in EU_MASS)
    w1, w1c = R(EU_W1), 1 - R(EU_W1)
    Ax, Bx, Bz = tti
    ax, bx, az, bz, axf, bzf = Lx4 * Ax, Lx4 * Bx, Lz4 * Bx, Lz4 * Bz, Lx * Ax, Lz * Bz
    ent = {}          # by property neighbour
    ent[-1, -1] = wm3 * K[-1, -1] + w1 * (ax * s3x + s * (bx * s3z) + s * (az * s3x) + bz * s3z) + w1c * (s * (bx * ln2c) + s * (az * ln4c))
    ent[-1, 0] = wm2 * K[-1, 0] + w1 * (s * (ax * (s3x + s4x)) + bx * (s4z + s * s3z) + az * (s3x + s * s4x) + bz * (s3z + s4z)) \
        + w1c * (bx * (ln3c + s * ln2c) + bzf * ln4)
    ent[-1, 1] = wm3 * K[-1, 1] + w1 * (ax * s4x + bx * s4z + az * s4x + bz * s4z) + w1c * (bx * ln3c + az * ln4c)
    ent[0, -1] = wm2 * K[0, -1] + w1 * (ax * (s3x + s1x) + bx * (s3z + s * s1z) + az * (s1x + s * s3x) + s * (bz * (s3z + s1z))) \
        + w1c * (axf * ln2 + az * (ln1c + s * ln4c))
    ent[0, 0] = wm1 * K[0, 0] + w1 * (s * (ax * (s1x + s2x + s3x + s4x)) + bx * ((s2z + s3z) + s * (s1z + s4z)) + az * ((s2x + s3x) + s * (s1x + s4x))
                                      + s * (bz * (s1z + s2z + s3z + s4z))) + w1c * (s * (axf * (ln2 + ln3)) + s * (bzf * (ln1 + ln4)))
    ent[0, 1] = wm2 * K[0, 1] + w1 * (ax * (s2x + s4x) + bx * (s2z + s * s4z) + az * (s4x + s * s2x) + s * (bz * (s2z + s4z))) \
        + w1c * (axf * ln3 + az * (ln4c + s * ln1c))
    ent[1, -1] = wm3 * K[1, -1] + w1 * (ax * s1x + bx * s1z + az * s1x + bz * s1z) + w1c * (bx * ln2c + az * ln1c)
    ent[1, 0] = wm2 * K[1, 0] + w1 * (s * (ax * (s2x + s1x)) + bx * (s1z + s * s2z) + az * (s2x + s * s1x) + bz * (s2z + s1z)) \
        + w1c * (bx * (ln2c + s * ln3c) + bzf * ln1)
    ent[1, 1] = wm3 * K[1, 1] + w1 * (ax * s2x + s * (bx * s2z) + s * (az * s2x) + bz * s2z) + w1c * (s * (bx * ln3c) + s * (az * ln1c))
    return _euEdgeRows(ent, nz, nx, R, dtype, magnitude, edges)


def _euEdgeRows(ent, nz, nx, R, dtype, magnitude, edges):
    'the entries by property neighbour into the nine planes by matrix slot (-sz, sx); edge rows keep the centre entry alone (edges False: nothing)'
    C = np.zeros((9, nz, nx), dtype=R if magnitude else dtype)
    for (sz, sx), e in ent.items():
        C[3 * (-sz + 1) + (sx + 1)] = e
    edge = ~_interiorMask(nz, nx)
    centre = C[4][edge]
    C[:, edge] = 0
    if edges:
        C[4][edge] = centre
    return C


def eurusPlanes(op, dc=None, db=None, dtype=np.complex128, magnitude=False, edges=True):
    """V[dc] + L[db]: the nine planes (9, nz, nx) of d M1 along the real perturbations dc of the velocity and db of the buoyancy ((N,) each, either may be None)
    for the Eurus operator `op` with eps == delta (its c, rho, theta, delta, C-PML, frequency and damping).  Edge rows carry the derivative of their centre
    entry, with the clamped neighbours counted as the assembly counts them.  dtype np.clongdouble: 80-bit arithmetic; magnitude: the same sum with every
    term replaced by its modulus.  edges False (for tests): the edge rows zero, as if they did not depend on the model."""
    return _euPlanes(_euSetup(op, dtype), dc, db, dtype, magnitude, edges)


def _euPlanes(setup, dc, db, dtype, magnitude, edges):
    'eurusPlanes from the _euSetup of the operator; dc alone takes the mass entries only'
    R = _real(dtype)
    c, b, om2, pml, tti = setup
    nz, nx = c.shape
    field = lambda v: np.asarray(v).astype(R).reshape((nz, nx))
    dbf = field(db) if db is not None else None if dc is not None else np.zeros((nz, nx), dtype=R)
    if magnitude:
        om2, c = np.abs(om2), np.abs(c)
        dK = 2 * om2 * b * np.abs(field(dc)) / (c * c * c) if dc is not None else None
        if dbf is not None:
            dKb = om2 * np.abs(dbf) / (c * c)
            dK = dKb if dK is None else dKb + dK
    else:
        dK = (-2 * om2) * b * field(dc) / (c * c * c) if dc is not None else None
        if dbf is not None:
            dKb = om2 * dbf / (c * c)
            dK = dKb if dK is None else dKb + dK
    return _euRow(dbf, dK, pml, tti, R, dtype, magnitude, edges)


def eurusAdjoint(op, P, conj=False, dtype=np.complex128, magnitude=False, edges=True):
    """(V^T P, L^T P): (N,) each with <V[dc] + L[db], P> = <dc, V^T P> + <db, L^T P> under the bilinear pairing sum_k sum_i (no conjugate), P (9, N) or (9, nz, nx)
    complex; on edge rows its centre plane alone is read.  conj: the transposes of the conjugated maps.  magnitude: the sum of the moduli of the terms.  A row
    reads the 3 x 3 (clamped) cells around it, so cells with equal (iz mod 3, ix mod 3) never meet in a row: the planes of the nine colour indicators are the
    coefficients of every row with respect to its one cell of that colour, and a 3 x 3 box sum of coefficient times P gathers them at the cell.
    Cost: one setup of the operator and, per colour, one full row evaluation (L) and one of the mass entries alone (V) -- nine assemblies of an nz x nx
    operator per call.  It is the reference of k_eurus_adjoint and the route without a GPU; on large grids it is slow next to the kernel."""
    nz, nx = int(op.nz), int(op.nx)
    N = nz * nx
    Pl = np.asarray(P).astype(dtype).reshape((9, nz, nx))
    if magnitude:
        Pl = np.abs(Pl)
    iz, ix = np.divmod(np.arange(N), nx)
    setup = _euSetup(op, dtype)
    gc, gb = np.zeros(N, dtype=Pl.dtype), np.zeros(N, dtype=Pl.dtype)
    for a in range(3):
        for bcol in range(3):
            mine = (iz % 3 == a) & (ix % 3 == bcol)
            if not mine.any():
                continue
            ind = mine.astype(np.float64)
            for g, coef in ((gc, _euPlanes(setup, ind, None, dtype, magnitude, edges)), (gb, _euPlanes(setup, None, ind, dtype, magnitude, edges))):
                if conj and not magnitude:
                    coef = np.conj(coef)
                g[mine] = _boxSum((coef * Pl).sum(axis=0), nz, nx).ravel()[mine]
    return gc, gb
