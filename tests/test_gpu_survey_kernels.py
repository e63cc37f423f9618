"""GPU: what csrc/survey.hip makes structural.  The energy and sampling loops exist once, as templates over the reader of the forward field
(csrc/survey_internal.hpp; each pair of entry points is one launcher), so the
complex64 entry point on a packed field and the complex128 entry point on the unpacked field run the same arithmetic on the same numbers: the same bits
(imaging: test_imaging_c64_kernel_against_extended_precision of tests/test_gpu_fieldstore.py).  And the plain sampling entry point, which multiplies by
nothing, gives the values of the accumulating ones at alpha = 1, beta = 0."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_moving as tm
from tests.test_gpu_fieldstore import op, wide_fields          # noqa: F401  (op: the 60 x 80 operator, a fixture)
from tests.test_gpu_moving import surveys                      # noqa: F401  (the two moving arrays, a fixture)

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
randc = tm.randc
UNROLL = 8                              # HELM_ENERGY_UNROLL of csrc/helm_internal.hpp


def packed_and_unpacked(rng, nsrc, rows, dev):
    'device arrays (nsrc, rows) of a complex64 store and of exactly what a consumer reads from it, and the exponents'
    import torch
    from zephyr_amd.fieldstore import pack_reference, unpack_reference
    Pk, e = pack_reference(wide_fields(rng, nsrc, rows))
    Uh = unpack_reference(Pk, e)
    return (torch.from_numpy(np.ascontiguousarray(Pk.T)).to(dev), torch.from_numpy(e).to(dev), torch.from_numpy(np.ascontiguousarray(Uh.T)).to(dev))


# nsrc on both sides of the unroll, and a remainder after two full groups; each with and without a weight; columns further apart than N once
@pytest.mark.parametrize('nsrc,weighted,pad', [(n, w, 0) for n in (1, UNROLL - 1, UNROLL, UNROLL + 1, 2 * UNROLL + 1) for w in (True, False)] + [(UNROLL + 1, True, 3)])
def test_energy_c64_on_the_packed_field_is_energy_c128_on_the_unpacked_field_bit_for_bit(helm_lib, op, nsrc, weighted, pad):
    import torch
    from zephyr_amd import _lib
    dev = torch.device('cuda', op.device)
    N = op.nrow
    ld = N + pad
    rng = np.random.default_rng(700 + 10 * nsrc + weighted + pad)
    dP, dX, dU = packed_and_unpacked(rng, nsrc, ld, dev)
    alpha = 0.37 if weighted else 1.0
    dW = torch.from_numpy(10.0 ** rng.uniform(-3, 3, N)).to(dev) if weighted else None
    wptr = P(dW.data_ptr()) if weighted else None
    E0 = rng.uniform(0.0, 1.0, N) * float((dU[:, :N].abs() ** 2).sum(dim=0).mean())
    d64, d128 = torch.from_numpy(E0).to(dev), torch.from_numpy(E0).to(dev)
    torch.cuda.synchronize(dev)
    _lib.check(helm_lib.helm_energy_accumulate_c64_device(op.handle, P(dP.data_ptr()), P(dX.data_ptr()), nsrc, ld, alpha, wptr, P(d64.data_ptr())), op.handle)
    _lib.check(helm_lib.helm_energy_accumulate_device(op.handle, P(dU.data_ptr()), nsrc, ld, alpha, wptr, P(d128.data_ptr())), op.handle)
    e64, e128 = d64.cpu().numpy(), d128.cpu().numpy()
    assert np.isfinite(e64).all() and (e64 > E0).any()                              # (something was added)
    assert np.array_equal(e64.view(np.uint64), e128.view(np.uint64))


@pytest.mark.parametrize('nsrc', [1, 5, 13])
def test_sample_rows_c64_on_the_packed_field_is_sample_rows_on_the_unpacked_field_bit_for_bit(helm_lib, op, surveys, nsrc):
    'both moving arrays of tests/test_gpu_moving.py, row stride nrec and 0, every (alpha, beta) of its COEFFS; beta = 0: the accumulator holds NaN'
    import torch
    from zephyr_amd import _lib
    dev = torch.device('cuda', op.device)
    N = op.nrow
    for name, sv in surveys:
        M = sv.stackedReceivers(0)
        nrec = sv.nrec
        rng = np.random.default_rng(900 * nsrc + nrec)
        dP, dX, dU = packed_and_unpacked(rng, nsrc, N, dev)
        out0 = randc(rng, (nrec, nsrc))
        csr = tm.upload_csr(M, dev)
        for stride in (nrec, 0):
            for alpha, beta in tm.COEFFS:
                def start():
                    return torch.full((nrec, nsrc), float('nan'), dtype=torch.complex128, device=dev) if beta == 0 else torch.from_numpy(out0).to(dev)
                d64, d128 = start(), start()
                torch.cuda.synchronize(dev)
                _lib.check(helm_lib.helm_sample_rows_c64_device(op.handle, P(dP.data_ptr()), P(dX.data_ptr()), nsrc, N, P(csr[0].data_ptr()), P(csr[1].data_ptr()),
                                                                P(csr[2].data_ptr()), nrec, stride, alpha.real, alpha.imag, beta.real, beta.imag,
                                                                P(d64.data_ptr())), op.handle)
                tm.sample_rows(helm_lib, op, dU.data_ptr(), nsrc, N, csr, 0, nrec, stride, alpha, beta, d128.data_ptr())
                o64, o128 = d64.cpu().numpy(), d128.cpu().numpy()
                assert np.isfinite(o64.view(np.float64)).all() and np.abs(o64).max() > 0, (name, stride, alpha, beta)
                assert np.array_equal(o64.view(np.float64), o128.view(np.float64)), (name, stride, alpha, beta)


def test_plain_sampling_gives_the_values_of_the_accumulating_entry_points_at_alpha_one_beta_zero(helm_lib, op):
    """37 receivers x 9 sources = 333 outputs: a full workgroup and 77 lanes of a second.  Rows of 0 to 11 entries.  The values are compared, not the
    bits: the accumulating kernels multiply the sum by 1 + 0i, which may turn a -0.0 into +0.0 and changes nothing else of a finite sum."""
    import torch
    from zephyr_amd import _lib
    dev = torch.device('cuda', op.device)
    N, nrec, nsrc = op.nrow, 37, 9
    assert nrec * nsrc > 256 and (nrec * nsrc) % 256 != 0
    rng = np.random.default_rng(37 * 9)
    length = rng.integers(0, 12, nrec)
    length[[4, 36]] = 0, 11
    indptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    nnz = int(indptr[-1])
    csr = (torch.from_numpy(indptr).to(dev), torch.from_numpy(rng.integers(0, N, nnz).astype(np.int64)).to(dev), torch.from_numpy(randc(rng, nnz)).to(dev))
    dU = torch.from_numpy(randc(rng, (nsrc, N))).to(dev)
    outs = [torch.full((nrec, nsrc), float('nan'), dtype=torch.complex128, device=dev) for _ in range(3)]
    torch.cuda.synchronize(dev)
    ptrs = [P(c.data_ptr()) for c in csr]
    _lib.check(helm_lib.helm_sample_device(op.handle, P(dU.data_ptr()), nsrc, N, *ptrs, nrec, P(outs[0].data_ptr())), op.handle)
    _lib.check(helm_lib.helm_sample_accumulate_device(op.handle, P(dU.data_ptr()), nsrc, N, *ptrs, nrec, 1.0, 0.0, 0.0, 0.0, P(outs[1].data_ptr())), op.handle)
    tm.sample_rows(helm_lib, op, dU.data_ptr(), nsrc, N, csr, 0, nrec, 0, 1.0 + 0j, 0j, outs[2].data_ptr())
    plain, acc, rows = (o.cpu().numpy() for o in outs)
    assert np.isfinite(plain.view(np.float64)).all() and np.all(plain[4] == 0) and np.all(plain[36] != 0)
    assert np.array_equal(plain, acc) and np.array_equal(plain, rows)
