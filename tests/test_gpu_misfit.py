"""GPU: the kernels of csrc/survey_misfit.hip through their entry points (helm_misfit_moments_device, helm_misfit_terms_device, helm_misfit_adjoint_device)
against the functions of zephyr_amd/misfit.py evaluated in 80-bit arithmetic, under the bounds tests/misfit_cases.py counts from the kernels' operation order
('logarithmic': MARGIN max(delta, 64 u majorant), delta the error of a numpy complex128 evaluation).  nrec 1, 7 and 130, 1, 5 and 67 columns (a partial wave, more
than one workgroup), ld > ncol with NaN in the padding, weights absent and with dead samples that hold NaN, every kind, a given and an estimated source, the
receiver phase and the weight panel on and off; a column has the same bits alone, first and last in a batch of 67, and on a second run."""
import ctypes

import numpy as np
import pytest

from tests import misfit_cases as mc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
NAN = complex(np.nan, np.nan)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64)


@pytest.fixture(scope='module')
def op(helm_lib):
    'a library handle, created and never assembled: the kernels use its device and its stream'
    from zephyr_amd import _lib

    class Raw(object):
        handle = helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 8, 8, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert Raw.handle, _lib.last_error(None)
    yield Raw
    helm_lib.helm_destroy(Raw.handle)


def padded(x, ld, fill, dtype):
    out = np.full((x.shape[0], ld), fill, dtype=dtype)
    out[:, :x.shape[1]] = x
    return out


class Panels(object):
    'the inputs of a case on the device, [nrec][ld] with NaN beyond the ncol columns'

    def __init__(self, p, d, w2, s, ld):
        import torch
        self.dev = torch.device('cuda', 0)
        self.nrec, self.ncol = p.shape
        self.ld = ld
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.P, self.D = up(padded(p, ld, NAN, np.complex128)), up(padded(d, ld, NAN, np.complex128))
        self.W = None if w2 is None else up(padded(w2, ld, np.nan, np.float64))
        self.S = up(s.astype(np.complex128))
        self.up = up

    def ptr(self, t):
        return None if t is None else P(t.data_ptr())

    def moments(self, lib, op):
        import torch
        from zephyr_amd import _lib
        mom = torch.full((self.ncol, 3), np.nan, dtype=torch.float64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        _lib.check(lib.helm_misfit_moments_device(op.handle, self.ptr(self.P), self.ptr(self.D), self.ptr(self.W), self.ld, self.nrec, self.ncol, self.ptr(mom)), op.handle)
        return mom.cpu().numpy()

    def terms(self, lib, op, kind):
        import torch
        from zephyr_amd import _lib
        psi = torch.full((self.nrec, self.ld), NAN, dtype=torch.complex128, device=self.dev)
        out = torch.full((self.ncol, 3), np.nan, dtype=torch.float64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        par = mc.kernel_par(kind)
        _lib.check(lib.helm_misfit_terms_device(op.handle, mc.CODES[kind], par[0], par[1], self.ptr(self.P), self.ptr(self.D), self.ptr(self.W), self.ptr(self.S),
                                                self.ld, self.nrec, self.ncol, self.ptr(psi), self.ptr(out)), op.handle)
        psi = psi.cpu().numpy()
        assert np.all(np.isnan(psi[:, self.ncol:]))                      # (the padding is not written)
        return psi[:, :self.ncol].copy(), out.cpu().numpy()

    def adjoint(self, lib, op, kind, psi, coef, phase, weights, inplace=True, par=None):
        import torch
        from zephyr_amd import _lib
        PSI = self.up(padded(psi, self.ld, NAN, np.complex128))
        C = None if coef is None else self.up(coef.astype(np.float64))
        PH = None if phase is None else self.up(phase.astype(np.complex128))
        V = self.P.clone() if inplace else torch.full((self.nrec, self.ld), NAN, dtype=torch.complex128, device=self.dev)
        src = V if inplace else self.P
        GN = torch.full((self.nrec, self.ld), np.nan, dtype=torch.float64, device=self.dev) if weights else None
        torch.cuda.synchronize(self.dev)
        par = mc.kernel_par(kind) if par is None else par
        _lib.check(lib.helm_misfit_adjoint_device(op.handle, mc.CODES[kind], par[0], par[1], self.ptr(PSI), self.ptr(self.S), self.ptr(C), self.ptr(src),
                                                  self.ptr(self.D), self.ptr(self.W), self.ptr(PH), self.ld, self.nrec, self.ncol, self.ptr(V), self.ptr(GN)), op.handle)
        v = V.cpu().numpy()
        assert np.all(np.isnan(v[:, self.ncol:]))
        gn = None
        if weights:
            gn = GN.cpu().numpy()
            assert np.all(np.isnan(gn[:, self.ncol:]))
            gn = gn[:, :self.ncol].copy()
        return v[:, :self.ncol].copy(), gn


def check_conditions(p, d, w2, s, weighted):
    "the conditions on the inputs, on the 80-bit values, with no sample discarded: they keep every branch decision the same in both precisions"
    c = mc.conditions(p, d, w2, s)
    assert c['margin'] > 1e-6 and c['theta'] <= 3. and 1e-3 <= c['ratio'][0] and c['ratio'][1] <= 1e3
    assert c['live'] + c['dead'] == p.size and (c['dead'] > 0) == (weighted and p.size > 3)
    if c['live'] > 1:
        assert c['below'] > 0 and c['above'] > 0
    return c


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('ncol', [1, 5, 67])
@pytest.mark.parametrize('nrec', [1, 7, 130])
def test_the_kernels_against_the_80_bit_evaluation(helm_lib, op, nrec, ncol, weighted):
    """the moments, psi, phi_j and c_j of every kind, and the adjoint source with and without the second term, the receiver phase and the weight panel, within
    their counted bounds ('logarithmic': 16 max(delta, 64 u majorant) per column); the worst ratio of every quantity is printed"""
    p, d, w2, s = mc.panel_inputs(nrec, ncol, seed=1000 * nrec + ncol, weighted=weighted)
    check_conditions(p, d, w2, s, weighted)
    live = np.ones(p.shape, dtype=bool) if w2 is None else w2 > 0
    rng = np.random.default_rng(nrec + ncol)
    dv = Panels(p, d, w2, s, ncol + 3)
    worst = {}
    mom_ref = None
    for kind in mc.KINDS:
        mom_ref, psi_ref, out_ref, maj = mc.reference(kind, p, d, w2, s)
        if kind == 'l2':
            mom = dv.moments(helm_lib, op)
            worst['moments'] = mc.worst(mom, mom_ref, mc.c_moments(nrec) * mc.U64 * maj['mom'])
        psi, out = dv.terms(helm_lib, op, kind)
        assert np.all(psi[~live] == 0) and np.all(np.isfinite(psi)) and np.all(np.isfinite(out))
        if kind == 'logarithmic':
            _, psi64, out64, _ = mc.reference(kind, p, d, w2, s, dtype=np.complex128)
            delta = mc.column_error(psi64, psi_ref)
            held = mc.MARGIN * np.maximum(delta, 64 * mc.U64 * maj['psi'].max(axis=0))
            worst['psi logarithmic'] = mc.held_ratio(mc.column_error(psi, psi_ref), held)
            delta = np.abs(out64.astype(mc.LD) - out_ref)
            held = mc.MARGIN * np.maximum(delta, 64 * mc.U64 * maj['out'])
            worst['phi, c logarithmic'] = mc.held_ratio(np.abs(out.astype(mc.LD) - out_ref), held)
        else:
            worst['psi ' + kind] = mc.worst(psi, psi_ref, mc.C_PSI * mc.U64 * maj['psi'])
            worst['phi ' + kind] = mc.worst(out[:, 0], out_ref[:, 0], mc.c_phi(nrec) * mc.U64 * maj['out'][:, 0])
            worst['c ' + kind] = mc.worst(out[:, 1:], out_ref[:, 1:], mc.c_c(nrec) * mc.U64 * maj['out'][:, 1:])
        # the adjoint source: psi as an input (the 80-bit one, rounded), a given source (no coefficients) and an estimated one (e = c / b, f = 2 Re(c s) / b of
        # the columns, rounded to doubles: the kernel's exact inputs), the phase and the weight panel on and off
        psi_in = np.asarray(psi_ref, dtype=np.complex128)
        c = out_ref[:, 1] + 1j * out_ref[:, 2]
        b = np.where(mom_ref[:, 2] > 0, mom_ref[:, 2], 1)
        e = c / b
        coef = np.stack([e.real, e.imag, 2 * (c * s.astype(mc.CLD)).real / b], axis=1).astype(np.float64)
        if kind == 'l2':
            coef = rng.uniform(-1., 1., coef.shape)                      # (zero to rounding for least squares: arbitrary ones exercise the term)
        phase = np.exp(1j * rng.uniform(-np.pi, np.pi, nrec))
        par = mc.kernel_par(kind)
        if kind == 'logarithmic':
            par = (par[0], par[0])                                       # (the weight panel exists for alpha = beta)
        for cf, ph, wanted, inplace in ((None, None, False, True), (coef, phase, True, True), (coef, None, True, False), (None, phase, False, False)):
            v, gn = dv.adjoint(helm_lib, op, kind, psi_in, cf, ph, wanted, inplace=inplace, par=par)
            v_ref, mag, gn_ref, factor = mc.adjoint_reference(kind, psi_in, s, cf, p, d, w2, ph)
            assert np.all(v[~live] == 0)
            name = 'v %s%s%s' % (kind, '' if cf is None else ' +term', '' if ph is None else ' +phase')
            worst[name] = mc.worst(v, v_ref, mc.C_V * mc.U64 * mag)
            if wanted:
                assert np.all(gn[~live] == 0) and np.all(gn >= 0)
                worst['weights ' + kind] = max(worst.get('weights ' + kind, 0.), mc.worst(gn, gn_ref, mc.U64 * gn_ref * factor))
    print('nrec %d ncol %d weighted %s: worst ratios %s' % (nrec, ncol, weighted, {k: '%.3g' % v for k, v in sorted(worst.items())}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('kind', mc.KINDS)
def test_a_column_has_the_same_bits_wherever_it_stands(helm_lib, op, kind):
    "alone, first and last of a batch of 67, and on a second run: a_j, b_j, phi_j, c_j, psi and v of the column are the same bits"
    nrec = 130
    p, d, w2, s = mc.panel_inputs(nrec, 67, seed=77)
    col = (p[:, 5:6], d[:, 5:6], w2[:, 5:6], s[5:6])
    for j in (0, 66):
        p[:, j], d[:, j], w2[:, j], s[j] = col[0][:, 0], col[1][:, 0], col[2][:, 0], col[3][0]
    rng = np.random.default_rng(3)
    coef1 = rng.uniform(-1., 1., (1, 3))
    coef = rng.uniform(-1., 1., (67, 3))
    coef[0] = coef[66] = coef1[0]
    phase = np.exp(1j * rng.uniform(-np.pi, np.pi, nrec))

    def run(pn, cf):
        mom = pn.moments(helm_lib, op)
        psi, out = pn.terms(helm_lib, op, kind)
        v, _ = pn.adjoint(helm_lib, op, kind, psi, cf, phase, False)
        return mom, out, psi, v
    lone = run(Panels(*col, 1), coef1)
    again = run(Panels(*col, 4), coef1)
    batch = run(Panels(p, d, w2, s, 70), coef)
    second = run(Panels(p, d, w2, s, 70), coef)
    for a, b in zip(batch, second):
        assert np.array_equal(bits(a), bits(b))
    for a, b in zip(lone, again):
        assert np.array_equal(bits(a), bits(b))
    for j in (0, 66):
        for name, a, b in zip(('moments', 'phi, c', 'psi', 'v'), lone, batch):
            mine = b[j:j + 1] if name in ('moments', 'phi, c') else b[:, j:j + 1]
            assert np.array_equal(bits(a), bits(mine)), (name, j)


def test_refusals(helm_lib, op):
    'bad arguments are refused before anything is launched'
    import torch
    from zephyr_amd import _lib
    dev = torch.device('cuda', 0)
    t = torch.zeros((4, 4), dtype=torch.complex128, device=dev)
    r = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    q = lambda x: P(x.data_ptr())
    assert helm_lib.helm_misfit_moments_device(op.handle, q(t), q(t), None, 3, 4, 4, q(r)) == -1                  # ld < ncol
    assert helm_lib.helm_misfit_moments_device(op.handle, P(t.data_ptr() + 8), q(t), None, 4, 4, 4, q(r)) == -1    # a misaligned panel
    assert helm_lib.helm_misfit_terms_device(op.handle, 7, 0., 0., q(t), q(t), None, q(t), 4, 4, 4, q(t.clone()), q(r)) == -1
    assert 'kind 7' in _lib.last_error(op.handle)
    assert helm_lib.helm_misfit_terms_device(op.handle, 1, 0., 0., q(t), q(t), None, q(t), 4, 4, 4, q(t.clone()), q(r)) == -1          # a threshold of 0
    assert helm_lib.helm_misfit_terms_device(op.handle, 0, 0., 0., q(t), q(t), None, q(t), 4, 4, 4, q(t), q(r)) == -1                  # psi over the samples
    g = torch.zeros((4, 4), dtype=torch.float64, device=dev)
    assert helm_lib.helm_misfit_adjoint_device(op.handle, 3, 1., 0.7, q(t.clone()), q(t), None, q(t), q(t.clone()), None, None, 4, 4, 4, q(t), q(g)) == -4
    assert 'not a real diagonal' in _lib.last_error(op.handle)
