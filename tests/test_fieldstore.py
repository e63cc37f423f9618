"""CPU: the complex64 store's format as fieldstore.pack_reference / unpack_reference state it, held to the bound of the format on columns from 1e-300 to
1e300 (a plain conversion to complex64 fails the same check), and the bookkeeping of DeviceFields on CPU tensors with a stub problem."""
import types

import numpy as np
import pytest

from tests.fieldstore_cases import NCOL, pack_columns, pack_bound_violations


@pytest.mark.parametrize('N', [1, 257, 4800])
def test_pack_reference_meets_the_format_bound_and_a_plain_conversion_does_not(N):
    from zephyr_amd.fieldstore import pack_reference, unpack_reference
    U = pack_columns(N)
    assert U.shape == (N, NCOL) and np.all(U[:, 1] == 0)
    comp = np.maximum(np.abs(U.real), np.abs(U.imag))
    assert comp[:, 2].argmax() == N - 1
    P, e = pack_reference(U)
    assert P.dtype == np.complex64 and P.shape == U.shape and e.dtype == np.int32 and e.shape == (NCOL,)
    # the exponents: 2^e <= m < 2^(e+1) where no clamp applies, 0 for the zero column, the clamp for the subnormal one
    m = comp.max(axis=0)
    for s in range(NCOL):
        if m[s] == 0:
            assert e[s] == 0
        elif m[s] >= 2.0 ** -1021:
            assert np.ldexp(1.0, int(e[s])) <= m[s] and m[s] / 2 < np.ldexp(1.0, int(e[s])), (s, m[s], e[s])
        else:
            assert e[s] == -1021
    assert e[5] == -1021 and e[0] == 2 and e.min() < -900 and e.max() > 900
    comp32 = np.maximum(np.abs(P.real), np.abs(P.imag)).max(axis=0)
    assert np.all(comp32 < 2.0) and np.all(comp32[(m >= 2.0 ** -1021)] >= 1.0)          # the scaled column maximum lies in [1, 2)
    V = unpack_reference(P, e)
    assert V.dtype == np.complex128
    assert pack_bound_violations(U, V, e) == 0
    if N > 1:
        tiny = U[N // 2, 0]
        assert tiny != 0 and abs(V[N // 2, 0] - tiny) <= 2.0 ** (2 - 126)                # the element 2^-140 of its column's maximum
    # the check can fail: fp32's own range overflows on the large columns and flushes the small ones
    with np.errstate(over='ignore'):
        plain = U.astype(np.complex64).astype(np.complex128)
    assert pack_bound_violations(U, plain, e) > 0
    for s in (3, 4):
        assert pack_bound_violations(U[:, s:s + 1], plain[:, s:s + 1], e[s:s + 1]) > 0


def make_store(dtype, scale=0.5 - 0.25j, N=37):
    import torch
    from zephyr_amd.fieldstore import DeviceFields, pack_reference
    rng = np.random.default_rng(4)
    nfreq, nsrc = 3, 13
    items = [(0, 0, 1, 0, 6), (1, 0, 1, 6, 13), (0, 0, 2, 0, 13)]                 # frequency 1 in two source batches, frequency 2 whole, frequency 0 not owned
    full = {f: rng.standard_normal((N, nsrc)) + 1j * rng.standard_normal((N, nsrc)) for f in (1, 2)}
    slices, exps = [], ([] if dtype == 'complex64' else None)
    for _, _, f, c0, c1 in items:
        part = full[f][:, c0:c1]
        if dtype == 'complex64':
            P, e = pack_reference(part)
            slices.append(torch.from_numpy(np.ascontiguousarray(P.T)))
            exps.append(torch.from_numpy(e))
        else:
            slices.append(torch.from_numpy(np.ascontiguousarray(part.T)))
    F = DeviceFields(nfreq, nsrc, items, slices, exps, stamp=3, scale=scale, dtype=dtype)
    return F, full, items


@pytest.mark.parametrize('dtype', ['complex128', 'complex64'])
def test_device_fields_bookkeeping_on_cpu_tensors(dtype):
    from zephyr_amd.fieldstore import pack_reference, unpack_reference
    scale, N = 0.5 - 0.25j, 37
    F, full, items = make_store(dtype, scale, N)
    assert len(F) == 3 and F.items == items and F.ownedFreqs == [1, 2] and F.dtype == dtype and F.stamp == 3 and F.scale == scale
    for f in (1, 2):
        u = F[f]
        assert u.shape == (N, 13) and u.dtype == np.complex128
        if dtype == 'complex128':
            assert np.array_equal(u, scale * full[f])
        else:
            want = np.hstack([unpack_reference(*pack_reference(full[f][:, c0:c1])) for _, _, ff, c0, c1 in items if ff == f])
            assert np.array_equal(u, scale * want)
            assert np.abs(u - scale * full[f]).max() <= 2.0 ** -22 * np.abs(full[f]).max()
    assert np.array_equal(F[-1], F[2])
    with pytest.raises(KeyError):
        F[0]
    it = iter(F)                                              # lazy: the first frequency is not owned, and only asking for it says so
    with pytest.raises(KeyError):
        next(it)
    esize = 16 if dtype == 'complex128' else 8
    assert F.nbytes == {0: 2 * 13 * N * esize + (0 if dtype == 'complex128' else 2 * 13 * 4)}
    F.checkCurrent(types.SimpleNamespace(_modelStamp=3))
    with pytest.raises(ValueError):
        F.checkCurrent(types.SimpleNamespace(_modelStamp=4))
    F.release()
    assert F.nbytes == {} and F.released
    with pytest.raises(KeyError):
        F[1]
    with pytest.raises(ValueError):
        F.checkCurrent(types.SimpleNamespace(_modelStamp=3))


def test_every_frequency_owned_iterates_like_fields():
    import torch
    from zephyr_amd.fieldstore import DeviceFields
    rng = np.random.default_rng(1)
    full = [rng.standard_normal((5, 2)) + 1j * rng.standard_normal((5, 2)) for _ in range(2)]
    F = DeviceFields(2, 2, [(0, 0, 0, 0, 2), (0, 0, 1, 0, 2)], [torch.from_numpy(np.ascontiguousarray(u.T)) for u in full])
    got = list(F)
    assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, full))
    with pytest.raises(ValueError):
        DeviceFields(2, 2, [], [], dtype='float32')


def test_memory_check_names_both_figures_and_the_half_size_store():
    from zephyr_amd.fieldstore import check_fits
    check_fits({0: 10, 1: 20}, {0: 10, 1: 21})
    with pytest.raises(MemoryError) as ei:
        check_fits({0: 10, 1: 4300000000}, {0: 10, 1: 123456789})
    assert '4300000000' in str(ei.value) and '123456789' in str(ei.value) and "fieldsDtype='complex64'" in str(ei.value)


def test_model_stamp_follows_clear_cache_and_the_host_route_refuses_device_fields():
    import os
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g6_survey.npz'))
    nz, nx = g['c'].shape
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=g['c'], rho=g['rho'], nPML=6, freqs=list(g['freqs']), Disc=za.MiniZephyrHD, sterms=g['sterms'],
              geom=dict(src=g['src'], rec=g['rec'], mode='fixed'), hostGradient=True, fieldsDtype='complex64')
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert prob.fieldsDtype == 'complex64' and Helm2DProblem(dict(sc, fieldsDtype='complex128')).fieldsDtype == 'complex128'
    s0 = prob._modelStamp
    prob.updateModel(g['c'])                                   # the same model: nothing is cleared
    assert prob._modelStamp == s0
    prob.updateModel(g['c'] + 1.0)
    assert prob._modelStamp == s0 + 1
    prob.clearCache()
    assert prob._modelStamp == s0 + 2
    with pytest.raises(RuntimeError):                          # hostGradient: fields() stays the route
        prob.fieldsDevice()
