"""Shared by tests/test_zgemm_choice.py (CPU) and tests/test_gpu_zgemm_tiles.py (GPU): the instantiations of the tile kernel k_zgemm3, the shapes the
GPU tests run, thin wrappers around the two test hooks of include/helm.h, and the extended-precision reference with its componentwise bound."""
import ctypes

import numpy as np

# tile index -> (rows, columns) of C per workgroup (choose_tile, zephyr_amd/csrc/nd_gemm.hip)
TILES = {0: (64, 64), 1: (32, 128), 2: (16, 256), 3: (64, 32), 4: (32, 64), 5: (16, 128), 6: (32, 32), 7: (16, 64), 8: (128, 16)}

# every instantiation of the dense kernel: name -> (tile, K slab, XR)
INSTANTIATIONS = {'tile%d-slab8' % t: (t, 8, 0) for t in range(9)}
INSTANTIATIONS.update({'tile6-slab16': (6, 16, 0), 'tile7-slab16': (7, 16, 0), 'xr': (None, 8, 1)})

# (M, N, K, batch) whose UNFORCED choice is that instantiation; tile 2 has none (test_zgemm_choice.py shows that no shape has)
NATURAL = {
    'tile0-slab8': (64, 256, 64, 64), 'tile1-slab8': (32, 128, 40, 300), 'tile3-slab8': (64, 32, 32, 300), 'tile4-slab8': (32, 64, 32, 300),
    'tile5-slab8': (16, 128, 16, 300), 'tile6-slab8': (200, 256, 64, 20), 'tile7-slab8': (8, 64, 8, 300), 'tile8-slab8': (128, 16, 200, 400),
    'tile6-slab16': (65, 67, 9, 2), 'tile7-slab16': (9, 256, 9, 40), 'xr': (49, 256, 81, 5),
}
# the shapes test_batched_zgemm (tests/test_gpu_direct.py) had before the natural-choice shapes above were added to it
SMALL = [(64, 64, 8, 1), (36, 256, 64, 7), (1, 1, 1, 3), (65, 67, 9, 2), (130, 33, 71, 3), (9, 256, 9, 40),
         (100, 16, 500, 3), (8, 16, 384, 1), (893, 16, 2900, 2), (37, 5, 1000, 2), (64, 1, 2000, 1), (13, 9, 447, 4),
         (300, 16, 1027, 1), (1900, 16, 3001, 2), (129, 7, 1024, 5), (40, 16, 1032, 9),
         (49, 256, 81, 5), (49, 64, 49, 3), (49, 100, 7, 2), (49, 300, 83, 2), (49, 32, 49, 4)]
# split over the inner dimension: (M, N, K, batch) -> factor (768 / (batch * ceil(M / 128)) clamped to 2 .. 16).  A is shared by the batch (sa = 0) where a
# private copy per item would be hundreds of MB.  K = 1027 / 1040: chunks that do not divide K; 1025 with 16 chunks of 72: an empty last chunk (15 x 72 = 1080)
SPLITK = {(300, 16, 1027, 1): 16, (129, 7, 1025, 5): 16, (20, 3, 1027, 50): 15, (20, 3, 1030, 52): 14, (20, 5, 1027, 56): 13, (40, 3, 1040, 64): 12,
          (150, 2, 1027, 33): 11, (150, 2, 1027, 35): 10, (150, 2, 1027, 40): 9, (250, 4, 1030, 48): 8, (200, 2, 1027, 50): 7, (130, 2, 1027, 64): 6,
          (300, 2, 1027, 50): 5, (385, 3, 1027, 48): 4, (513, 2, 1025, 51): 3, (513, 2, 1027, 52): 2}

ALPHA_BETA = ((1 + 0j, 0j), (-1 + 0j, 1 + 0j), (0.3 - 0.2j, 0.5 + 0.1j))          # the pairs of test_batched_zgemm
K_LIST = (1, 3, 4, 5, 8, 9, 16, 17, 71, 256)                                       # k groups of four, slabs of 8 / 16: every remainder
U = 2.0 ** -53


def choice(lib, M, N, K, batch, nf_div=1, force_tile=-1, force_slab=0, have_handle=1, mode=0):
    """helm_debug_zgemm_choice: (tile, K slab, XR, split factor, split chunk), or the negative return code"""
    rep = (ctypes.c_int * 5)()
    rc = lib.helm_debug_zgemm_choice(M, N, K, batch, nf_div, force_tile, force_slab, have_handle, mode, rep)
    return tuple(rep) if rc == 0 else rc


def instantiation_of(rep):
    """name in INSTANTIATIONS of a report (a split launch runs tile 8 with the slab of 8)"""
    if rep[2]:
        return 'xr'
    return 'tile%d-slab%d' % (rep[0], rep[1])


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def zgemm_ex(lib, M, N, K, batch, A, lda, sa, B, ldb, sb, C, ldc, sc, alpha, beta, device=0, **opt):
    """helm_debug_zgemm_ex on flat complex128 buffers (C and the output arenas are updated in place).  Returns (rc, report)."""
    from zephyr_amd import _lib
    p = _lib.ZgemmEx()
    p.device, p.M, p.N, p.K, p.batch = device, M, N, K, batch
    p.lda, p.ldb, p.ldc, p.sa, p.sb, p.sc = lda, ldb, ldc, sa, sb, sc
    p.alpha[0], p.alpha[1], p.beta[0], p.beta[1] = alpha.real, alpha.imag, beta.real, beta.imag
    p.A, p.a_len = _p(A), (A.size if A is not None else 0)
    p.B, p.b_len = _p(B), (B.size if B is not None else 0)
    p.C, p.c_len = _p(C), (C.size if C is not None else 0)
    p.force_tile, p.force_slab, p.xcd_map, p.ntc = opt.pop('force_tile', -1), opt.pop('force_slab', 0), opt.pop('xcd_map', -1), opt.pop('ntc', 0)
    p.zr0, p.zr1 = opt.pop('zr', (0, 0))
    p.zc0, p.zc1 = opt.pop('zc', (0, 0))
    p.sk0, p.sk1 = opt.pop('sk', (0, 0))
    p.tm64, p.c_is_b = opt.pop('tm64', 0), opt.pop('c_is_b', 0)
    tabs = [opt.pop(k, None) for k in ('tabB', 'tabCi', 'tabCo')]
    for t in tabs:
        assert t is None or (t.dtype == np.int32 and t.flags.c_contiguous)
    p.tabB, p.tabCi, p.tabCo = [_p(t) for t in tabs]
    p.tab_len = opt.pop('tab_len', min([t.size for t in tabs if t is not None] or [0]))
    p.tab_stride, p.offB, p.offCi, p.offCo = opt.pop('tab_stride', 0), opt.pop('offB', 0), opt.pop('offCi', 0), opt.pop('offCo', 0)
    p.ldx, p.arena_rows = opt.pop('ldx', 0), opt.pop('arena_rows', 0)
    arenas = [opt.pop(k, None) for k in ('Bx', 'Bx2', 'Cix', 'Cox', 'Cox2')]
    for a in arenas:
        assert a is None or (a.dtype == np.complex128 and a.flags.c_contiguous and a.size >= p.arena_rows * p.ldx)
    p.Bx, p.Bx2, p.Cix, p.Cox, p.Cox2 = [_p(a) for a in arenas]
    p.k2, p.cj_out = opt.pop('k2', 0), opt.pop('cj_out', 0)
    osc = opt.pop('oscale', 1 + 0j)
    p.oscale[0], p.oscale[1] = osc.real, osc.imag
    act = opt.pop('act', None)
    assert act is None or (act.dtype == np.int32 and act.size >= batch * ((N + 63) // 64))
    p.act = _p(act)
    assert not opt, 'unknown options %s' % sorted(opt)
    for a in (A, B, C):
        assert a is None or (a.dtype == np.complex128 and a.flags.c_contiguous and a.ndim == 1)
    rc = lib.helm_debug_zgemm_ex(ctypes.byref(p))
    return rc, tuple(p.report)


def strided(buf, batch, rows, cols, ld, stride, offset=0):
    """(batch, rows, cols) view of a flat buffer: element (z, r, c) at offset + z stride + r ld + c"""
    it = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=(batch, rows, cols), strides=(stride * it, ld * it, it), writeable=False)


def have_x87():
    return np.finfo(np.longdouble).eps < 2e-19


def reference(A, B, Cin, alpha, beta):
    """alpha A B + beta Cin in numpy.clongdouble from complex128 operands (batched), and S = |alpha| |A| |B| + |beta| |Cin| in fp64"""
    ld = np.clongdouble
    ref = ld(alpha) * np.matmul(A.astype(ld), B.astype(ld))
    S = abs(alpha) * np.matmul(np.abs(A), np.abs(B))
    if beta != 0:
        ref = ref + ld(beta) * Cin.astype(ld)
        S = S + abs(beta) * np.abs(Cin)
    return ref, S


def worst_ratio(out, ref, S, K, extra=0):
    """max over the elements of |out - ref| / (4 (K + 4 + extra) u S); an element whose bound is zero must be exact.  NaN anywhere gives inf."""
    err = np.abs(out.astype(np.clongdouble) - ref).astype(np.float64)
    bound = 4.0 * (K + 4 + extra) * U * S
    if not np.all(np.isfinite(err)):
        return np.inf
    if np.any(err[bound == 0] != 0):
        return np.inf
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def mixed_rows(rng, A):
    """rows of A scaled by 2^randint(-20, 20): a dropped term is not hidden under a large neighbour"""
    return A * np.ldexp(1.0, rng.integers(-20, 21, size=A.shape[:-1] + (1,)))
