"""Device pipelines of the exact 3-D derivative: `Helm3DProblem.Jtvec(adjoint='transpose', linearisation='operator')` and `JvecBorn(linearisation='operator')`
over forward fields in HBM.  The loops, the workspaces and the item steps are those of device_survey.py (`runOnDevices`, `Workspace`, `_backSources`,
`_sampling`, the stored items of a `DeviceFields`); what differs is what an item runs between them -- the three kernels of csrc/survey3d.hip.

    pipeline               items    what fills R                                   columns solved   what consumes U                          what comes down
    bornFromFields3        stored   -(1 / premul) M~(chi dc (.) conj(slice))        k (A)            sampleDevice, receivers as they are      nrec x k samples per item
    gradientFromFields3    stored   qb of R^H r                                    k (A^T)          k_mass3_imaging into P, then the chain   one float64 partial G per worker

With a buoyancy part (parameter 'rho' / 'joint', or the Gardner density: csrc/survey3d_density.hip) the Born right-hand side also receives
-(1 / premul) (1/2 db (.) L u^ + 1/2 L(db (.) u^)), ADDED by k_lap3_sources to what k_mass3_sources stored (its weight then carries kappa db), and the gradient reads the same
U once more: k_lap3_imaging into a second N-plane, k_buoy3_chain into the partial ((2 N,) for 'joint').  Still one solve per item either way.

The sampling and back-source kernels work on op.N rows and CSR rows: nothing in them knows the grid's dimension.  Nothing of size N k crosses to the host.
A 3-D item builds its multigrid hierarchy in the prepare step of `runOnDevices` (Helm3D.heavyPrepare: strictly one item ahead), for the forward and for the
transposed wrapper alike.
"""
import ctypes

import numpy as np

from . import _lib
from . import parallel
from .device_survey import _backSources, _partial, _prepareBackSources, _sampling, _storedItems, runOnDevices


def _p(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def massSourcesDevice(op, d_u, nsrc, d_w, coef, d_r, conj=True, ldu=None, ldr=None):
    'R[s] = coef M~(W (.) conj-or-not(U[s])) on the device (helm_mass3_sources_device); all device pointers, leading dimensions default to N'
    N = int(op.nrow)
    coef = complex(coef)
    _lib.check(_lib.load().helm_mass3_sources_device(op.handle, _p(d_u), int(nsrc), int(N if ldu is None else ldu), _p(d_w), coef.real, coef.imag, 1 if conj else 0,
                                                     _p(d_r), int(N if ldr is None else ldr)), op.handle)


def massImagingAccumulateDevice(op, d_uf, d_ub, nsrc, d_p, ldf=None, ldb=None):
    'P += sum_s UF[s] (.) M~^T UB[s] on the device (helm_mass3_imaging_accumulate_device)'
    N = int(op.nrow)
    _lib.check(_lib.load().helm_mass3_imaging_accumulate_device(op.handle, _p(d_uf), int(N if ldf is None else ldf), _p(d_ub), int(N if ldb is None else ldb), int(nsrc),
                                                                _p(d_p)), op.handle)


def massChainDevice(op, d_p, w, d_dc, d_out):
    'd_dc given: out = w chi dc (N complex128); d_dc None: out += Re(w chi P) (N float64) -- chi at the model and frequency of the handle (helm_mass3_chain_device)'
    w = complex(w)
    _lib.check(_lib.load().helm_mass3_chain_device(op.handle, None if d_p is None else _p(d_p), w.real, w.imag, None if d_dc is None else _p(d_dc), _p(d_out)), op.handle)


def lapSourcesDevice(op, d_u, nsrc, d_b, coef, d_r, conj=True, add=False, ldu=None, ldr=None):
    'R[s] (+)= coef (1/2 B (.) (L X[s]) + 1/2 L(B (.) X[s])), X = conj-or-not(U), B (N,) float64 on the device (helm_lap3_sources_device)'
    N = int(op.nrow)
    coef = complex(coef)
    _lib.check(_lib.load().helm_lap3_sources_device(op.handle, _p(d_u), int(nsrc), int(N if ldu is None else ldu), _p(d_b), coef.real, coef.imag, 1 if conj else 0,
                                                    1 if add else 0, _p(d_r), int(N if ldr is None else ldr)), op.handle)


def lapImagingAccumulateDevice(op, d_uf, d_ub, nsrc, d_p, conj=False, ldf=None, ldb=None):
    'P += 1/2 sum_s (UB0[s] (.) L UF[s] + UF[s] (.) L^T UB0[s]), both fields conjugated as they are read when conj (helm_lap3_imaging_accumulate_device)'
    N = int(op.nrow)
    _lib.check(_lib.load().helm_lap3_imaging_accumulate_device(op.handle, _p(d_uf), int(N if ldf is None else ldf), _p(d_ub), int(N if ldb is None else ldb), int(nsrc),
                                                               1 if conj else 0, _p(d_p)), op.handle)


def buoyChainDevice(op, gardner, d_in, d_plap, d_pmass, w, d_db, d_out):
    """chain = -1 / rho^2, or d b / d c of the Gardner density when `gardner`.  d_in given: db = chain d_in (N float64) and out = w kappa db (N complex128);
    d_in None: out += chain Re(w (Plap + kappa Pmass)) (N float64) (helm_buoy3_chain_device)"""
    w = complex(w)
    opt = lambda t: None if t is None else _p(t)
    _lib.check(_lib.load().helm_buoy3_chain_device(op.handle, 1 if gardner else 0, opt(d_in), opt(d_plap), opt(d_pmass), w.real, w.imag, opt(d_db), _p(d_out)), op.handle)


def _realBuffer(ws, name, n):
    'n float64 over a complex128 buffer of the workspace'
    import torch
    return torch.view_as_real(ws.buffer(name, (n + 1) // 2)).reshape(-1)[:n]


def bornFromFields3(prob, F, dc, dbuoy=None, gardner=False):
    """Born data (nrec, nsrc, nfreq) from forward fields in HBM of the velocity perturbation dc (N,) float64 (None: none) and, with dbuoy (N,) float64, of the
    density perturbation dbuoy -- or, when `gardner`, of the density that follows the velocity perturbation dbuoy.  Per stored item: W = chi dc on the item's
    GPU (the vectors go up once per worker), with a buoyancy part db = chain dbuoy and W += kappa db; R = -(1 / premul) M~(W (.) conj(slice)) -- the slice is
    conj(u^), unscaled --, plus -(1 / premul) (1/2 db (.) L u^ + 1/2 L(db (.) u^)) ADDED by k_lap3_sources: ONE right-hand side, the forward operator solves
    the k columns once and the samples through the receiver CSR come down, times the scaleTerm."""
    import torch
    F.checkCurrent(prob)
    data, stage, sample = _sampling(prob, F.ownedFreqs, F.scale)
    if not F.items:
        return data
    dc = None if dc is None else np.ascontiguousarray(dc, dtype=np.float64)
    dbuoy = None if dbuoy is None else np.ascontiguousarray(dbuoy, dtype=np.float64)
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        d_uF, _ = F.pointers(ifreq, c0)
        staged = stage(ws, ifreq, c0, c1)
        W, U, R = ws.buffer('W3', Ni), ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
        if dc is not None:
            vd = ws.cached(('born3_dc', id(dc)), lambda: _lib.to_device(dc, dev, np.float64), keep=dc)
        if dbuoy is not None:
            bd = vd if dbuoy is dc else ws.cached(('born3_db', id(dbuoy)), lambda: _lib.to_device(dbuoy, dev, np.float64), keep=dbuoy)
            DB, Wb = _realBuffer(ws, 'DB3', Ni), (ws.buffer('W3b', Ni) if dc is not None else W)
        _lib.wait_torch_stream(dev)
        if dc is not None:
            massChainDevice(op, None, 1.0, vd, W)
        if dbuoy is not None:
            buoyChainDevice(op, gardner, bd, None, None, 1.0, DB, Wb)
            if dc is not None:
                W.add_(Wb)
                _lib.wait_torch_stream(dev)
        massSourcesDevice(op, d_uF, k, W, -1.0 / complex(op.premul), R, conj=True)
        if dbuoy is not None:
            lapSourcesDevice(op, d_uF, k, DB, -1.0 / complex(op.premul), R, conj=True, add=True)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        sample(op, ifreq, c0, c1, staged, U.data_ptr())
    runOnDevices(devs, items, one)
    return data


def gradientFromFields3(prob, F, qb, resid, system, parameter='c', gardner=False):
    """J^T r, float64 (N,) -- (2 N,), [g_c; g_rho], for parameter='joint' --, from forward fields in HBM: per stored item the k back-sources R_s^H r_s are made
    on the item's GPU (qb / resid those of the Hermitian residual) and solved ONCE through the TRANSPOSED operator of `system`; U = conj(z~),
    z~ = premul A^-T R^H r.  k_mass3_imaging forms P = sum_s slice_s (.) M~^T U_s = conj(sum_s u^_s (.) M~^T z~_s), torch conjugates the one N-plane, and the
    chain kernel adds Re(w chi conj(P)), w = -conj(scaleTerm) / premul, to the worker's float64 partial ('c', 'joint', and the Gardner total).  The buoyancy
    half ('rho', 'joint', gardner) reads the same U and the same mass plane: k_lap3_imaging forms Plap = 1/2 sum_s (z~0_s (.) L u^_s + u^_s (.) L^T z~0_s),
    conjugating both columns as it stages them (L is complex), and k_buoy3_chain adds chain Re(w (Plap + kappa conj(P))), chain = -1 / rho^2 or the Gardner
    d b / d c.  The partials are summed on the host, then ONE all-reduce over ranks when sharded."""
    import torch
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    scale = F.scale
    wantC = gardner or parameter in ('c', 'joint')
    wantB = gardner or parameter in ('rho', 'joint')
    nG = 2 * N if parameter == 'joint' else N
    parts = []
    if F.items:
        _prepareBackSources(sv, qb, F.ownedFreqs)
        devs, items = _storedItems(system, F)

        def one(ws, op, ifreq, c0, c1):
            k, Ni = c1 - c0, int(op.nrow)
            d_uF, _ = F.pointers(ifreq, c0)
            G = _partial(ws, 'H', nG, torch.float64)         # (the workspace's float64 partial: this call accumulates nothing else there)
            P, U, R = ws.buffer('P3', Ni), ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
            _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
            P.zero_()
            if wantB:
                Pl = ws.buffer('P3l', Ni)
                Pl.zero_()
            _lib.wait_torch_stream(ws.device)
            op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
            massImagingAccumulateDevice(op, d_uF, U, k, P)
            torch.conj_physical_(P)
            _lib.wait_torch_stream(ws.device)
            w = -np.conj(scale) / complex(op.premul)
            if wantC:
                massChainDevice(op, P, w, None, G)
            if wantB:
                lapImagingAccumulateDevice(op, d_uF, U, k, Pl, conj=True)
                buoyChainDevice(op, gardner, None, Pl, P, w, None, G[N:] if parameter == 'joint' else G)
        parts = [ws.H for ws in runOnDevices(devs, items, one) if ws.H is not None]
    g = np.zeros(nG, dtype=np.float64)
    for G in parts:
        torch.cuda.synchronize(G.device)
        g += _lib.from_device(G)
    return parallel.allreduce_sum(g) if prob._sharded else g


# ---- the pseudo-Hessian diagonal and the (c, rho) blocks (csrc/survey3d_hessian.hip) ------------------------------------------------------------------------
PH3_MODES = {'buoyancy': 0, 'gardner': 1, 'blocks': 2}


def ph3CoefficientsDevice(op, mode, d_a0, d_h, d_s, d_c=None, d_smu=None):
    """the coefficient planes of the handle's model (helm_ph3_coefficients_device): mode 'buoyancy', 'gardner' or 'blocks'; d_a0 (and d_c) N complex128, d_h, d_s (and
    d_smu) N float64, all on the device"""
    opt = lambda t: None if t is None else _p(t)
    _lib.check(_lib.load().helm_ph3_coefficients_device(op.handle, PH3_MODES[mode], _p(d_a0), _p(d_h), _p(d_s), opt(d_c), opt(d_smu)), op.handle)


def ph3MomentsAccumulateDevice(op, d_u, nsrc, planes, alpha, d_w, d_h, blocks=False, conj=True, ldu=None, ldh=None):
    """H += alpha W (S' E + D), or with `blocks` the three rows H_cc, H_crho, H_rhorho at stride ldh, over the columns of U (helm_ph3_moments_accumulate_device);
    planes = (A0, h, S') or (A0, h, S', C', Smu) as ph3CoefficientsDevice made them, d_w None: no weight"""
    N = int(op.nrow)
    opt = lambda t: None if t is None else _p(t)
    pl = list(planes) + [None] * (5 - len(planes))
    _lib.check(_lib.load().helm_ph3_moments_accumulate_device(op.handle, _p(d_u), int(nsrc), int(N if ldu is None else ldu), 1 if conj else 0, 1 if blocks else 0,
                                                              _p(pl[0]), _p(pl[1]), _p(pl[2]), opt(pl[3]), opt(pl[4]), float(alpha), opt(d_w), _p(d_h),
                                                              int(N if ldh is None else ldh)), op.handle)


def pseudoHessianFromFields3(prob, F, parameter='c', gardner=False, perFreq=False, blocks=False):
    """The exact pseudo-Hessian from forward fields in HBM: float64 (N,) -- (nfreq, N) with perFreq --, or with `blocks` the rows H_cc, H_crho, H_rhorho, (3, N) --
    (nfreq, 3, N).  No solve: every stored item reads its slice where it lies and adds to its worker's partial.  The slice is conj(u^), unscaled: the kernels
    conjugate it as they stage it and |scaleTerm|^2 is the factor alpha.
    parameter 'c' with an explicit density: the closed form, k_energy with the weight Smu / |c^3 rho|^2 (made by torch once per worker and model, as the 2-D
    'operator' route makes its weight) and 4 |om~^2|^2 |scaleTerm|^2 in alpha; neither kernel of survey3d_hessian.hip runs.  Otherwise k_ph3_coefficients fills the coefficient planes of the item's operator in the workspace -- once per worker
    and frequency -- and k_ph3_moments walks the columns: 'rho' with W = 1 / rho^4, the Gardner total derivative without a weight, the blocks with the density
    factors of the kernel.  The partials are summed on the host, then ONE all-reduce over ranks when sharded."""
    from . import frechet3d
    from .device_survey import _blocksRow, _cachedInverseC3Rho, _energyRow, _sumEnergyPartials
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    shape = ((sv.nfreq, 3, N) if perFreq else (3, N)) if blocks else ((sv.nfreq, N) if perFreq else (N,))
    if not F.items:
        return _sumEnergyPartials(prob, [], shape)
    scale = F.scale
    a2 = scale.real * scale.real + scale.imag * scale.imag
    closed = not blocks and parameter == 'c' and not gardner
    mode = 'blocks' if blocks else ('gardner' if gardner else 'buoyancy')
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        d_uF, _ = F.pointers(ifreq, c0)
        row = (_blocksRow if blocks else _energyRow)(ws, shape, ifreq)
        if closed:
            # |chi|^2 Smu = 4 |om~^2|^2 Smu / |c^3 rho|^2: the frequency goes into alpha, the rest is one array per worker and model
            cm, rho = op.c, op.rho

            def weight():
                inv = _cachedInverseC3Rho(ws, op)
                return (inv.real * inv.real + inv.imag * inv.imag) * _lib.to_device(frechet3d.massWeightSquares3(op.modelDims), dev, np.float64)
            W = ws.cached(('ph3_velocity_weight', id(cm), id(rho)), weight, keep=(cm, rho))
            om = frechet3d.dampedOmega3(op)
            _lib.wait_torch_stream(dev)
            op.energyAccumulateDevice(d_uF, k, 4.0 * abs(om * om) ** 2 * a2, W.data_ptr(), row, rows=Ni)
            return
        W = None
        if parameter == 'rho' and not blocks:
            rho = op.rho
            W = ws.cached(('ph_inv_rho4', id(rho)), lambda: _lib.to_device(np.broadcast_to(np.asarray(rho, dtype=np.float64).ravel(), (Ni,)) ** -4.0, dev, np.float64), keep=rho)
        planes = [ws.buffer('ph3_A0', Ni), _realBuffer(ws, 'ph3_h', Ni), _realBuffer(ws, 'ph3_S', Ni)]
        if blocks:
            planes += [ws.buffer('ph3_C', Ni), _realBuffer(ws, 'ph3_Smu', Ni)]
        state = ws.cached('ph3_planes_of', dict)
        _lib.wait_torch_stream(dev)                       # (covers the zeroed partial and the weight)
        if state.get('key') != (ifreq, id(op)):
            ph3CoefficientsDevice(op, mode, *planes)
            state['key'] = (ifreq, id(op))
        ph3MomentsAccumulateDevice(op, d_uF, k, planes, a2, W, row, blocks=blocks, conj=True, ldh=Ni)
    return _sumEnergyPartials(prob, [ws.H for ws in runOnDevices(devs, items, one, factor=False) if ws.H is not None], shape)
