"""CPU: what gemm() (zephyr_amd/csrc/nd_gemm.hip) launches for a shape, asked through helm_debug_zgemm_choice -- the code the launch itself runs, no GPU.
The shapes tests/test_gpu_zgemm_tiles.py and test_batched_zgemm run reach, unforced, every instantiation of the tile kernel that production can reach;
tile 2 (16 x 256) is reachable by forcing only; the properties of the choice the comments in choose_tile() / gemm() state; and helm_debug_zgemm_ex refuses
malformed input before it touches a device."""
import numpy as np
import pytest

from tests import zgemm_shapes as zs

HELM_ERR_ARG = -1
TABLE, MASKS, TM64 = 1, 2, 4


def tiles64(M, N, batch):
    return batch * ((M + 63) // 64) * ((N + 63) // 64)


def lattice():
    """1 ... 2100 on a coarse lattice plus the borders of every tile size (k t - 1, k t, k t + 1 for the first multiples)"""
    v = set(range(1, 2101, 37)) | {2100}
    for t in (16, 32, 49, 64, 128, 256):
        for k in range(1, 6):
            v |= {k * t - 1, k * t, k * t + 1}
    return sorted(x for x in v if 1 <= x <= 2100)


def test_gpu_shape_list_reaches_every_reachable_instantiation(helm_lib):
    for name, shape in zs.NATURAL.items():
        assert zs.instantiation_of(zs.choice(helm_lib, *shape)) == name, (name, shape)
    reached, factors = set(), set()
    for shape in list(zs.NATURAL.values()) + zs.SMALL + list(zs.SPLITK):
        rep = zs.choice(helm_lib, *shape)
        reached.add(zs.instantiation_of(rep))
        if rep[3]:
            assert rep[:3] == (8, 8, 0)                      # a split launch runs the 128 x 16 tile
            factors.add(rep[3])
    assert reached == set(zs.INSTANTIATIONS) - {'tile2-slab8'}
    for shape, f in zs.SPLITK.items():
        rep = zs.choice(helm_lib, *shape)
        assert rep[3] == f and rep[4] % 8 == 0 and rep[4] * f >= shape[2], (shape, rep)
    assert factors == set(range(2, 17))
    # chunks that do not divide K, and an empty last chunk (chunk f - 1 begins past K)
    assert any(shape[2] % zs.choice(helm_lib, *shape)[4] for shape in zs.SPLITK)
    assert any((f - 1) * zs.choice(helm_lib, *shape)[4] >= shape[2] for shape, f in zs.SPLITK.items())
    # the unsplit 128 x 16 tile is in the list too
    assert zs.choice(helm_lib, *zs.NATURAL['tile8-slab8'])[3] == 0
    # without a handle nothing is split (no scratch to keep the partial products in)
    assert zs.choice(helm_lib, 300, 16, 1027, 1, have_handle=0)[3] == 0


def test_tile_2_is_reachable_by_forcing_only(helm_lib):
    vals = lattice()
    seen = {}
    for mode in (0, TABLE, MASKS):
        for batch in (1, 7, 64, 300, 5000):
            for K in (8, 64):
                for M in vals:
                    for N in vals:
                        rep = zs.choice(helm_lib, M, N, K, batch, mode=mode)
                        seen.setdefault(rep[0], (M, N, K, batch, mode))
                        # tile 8 never for more than 16 columns
                        assert not (rep[0] == 8 and N > 16), (M, N, K, batch, mode, rep)
    assert sorted(seen) == [0, 1, 3, 4, 5, 6, 7, 8], seen
    for M in (1, 16, 17, 32, 33, 64):                         # one row tile per matrix: 7, 3 or 0
        for N in (1, 32, 33, 256, 1000):
            for batch in (1, 300):
                rep = zs.choice(helm_lib, M, N, 16, batch, mode=MASKS | TM64)
                assert rep[:2] == ((7 if M <= 16 else (3 if N <= 32 else 0)), 8)
    assert zs.choice(helm_lib, 16, 256, 16, 300, force_tile=2) == (2, 8, 0, 0, 0)


def test_properties_of_the_choice(helm_lib):
    vals = [v for v in lattice() if v <= 700]
    for batch in (1, 3, 40, 300, 3000):
        for M in vals:
            for N in vals:
                for mode in (0, TABLE):
                    rep = zs.choice(helm_lib, M, N, 24, batch, mode=mode)
                    assert rep[2] == (1 if M == 49 and N >= 64 else 0)                       # XR: the 49-row leaves with at least 64 columns, nothing else
                    if not rep[2]:
                        assert (rep[1] == 16) == (tiles64(M, N, batch) < 256), (M, N, batch, rep)     # latency mode iff fewer than 256 tiles of 64 x 64
                        assert rep[1] == 8 or rep[0] in (6, 7)
                    else:
                        assert rep[1] == 8
                assert zs.choice(helm_lib, M, N, 24, batch, mode=MASKS)[2] == 0              # masked products never take the XR tile
    # the choice is made for one frequency's share of a multi-frequency launch
    for M, N, K, batch in list(zs.NATURAL.values()) + zs.SMALL + list(zs.SPLITK):
        for nf in (2, 3, 8):
            assert zs.choice(helm_lib, M, N, K, batch * nf, nf_div=nf) == zs.choice(helm_lib, M, N, K, batch), (M, N, K, batch, nf)
    # forcing: every tile with the slab of 8, tiles 6 and 7 with either slab; forcing switches the XR tile off
    for t in range(9):
        N = 16 if t == 8 else 100
        assert zs.choice(helm_lib, 49, N, 9, 3, force_tile=t)[:3] == (t, 8, 0)
        assert zs.choice(helm_lib, 49, N, 9, 3, force_tile=t, force_slab=8)[:3] == (t, 8, 0)
    for t in (6, 7):
        assert zs.choice(helm_lib, 49, 100, 9, 5000, force_tile=t, force_slab=16)[:3] == (t, 16, 0)
    for bad in (dict(force_tile=9), dict(force_tile=-2), dict(force_tile=0, force_slab=16), dict(force_slab=8), dict(force_tile=6, force_slab=4),
                dict(force_tile=8), dict(nf_div=0), dict(mode=8)):
        assert zs.choice(helm_lib, 49, 100, 9, 3, **bad) == HELM_ERR_ARG, bad
    assert zs.choice(helm_lib, 65, 10, 9, 3, mode=TM64) == HELM_ERR_ARG


def dense_args(M=20, N=30, K=10, batch=2, pad=0):
    lda, ldb, ldc = K + pad, N + pad, N + pad
    A, B, C = np.zeros(batch * M * lda, complex), np.zeros(batch * K * ldb, complex), np.zeros(batch * M * ldc, complex)
    return [M, N, K, batch, A, lda, M * lda, B, ldb, K * ldb, C, ldc, M * ldc, 1 + 0j, 0j]


def table_args(M=20, N=30, K=10, batch=2, rows=64):
    a = dense_args(M, N, K, batch)
    a[7], a[10] = None, None
    stride = K + 2 * M
    rng = np.random.default_rng(1)
    tab = rng.integers(-1, rows, size=batch * stride).astype(np.int32)
    arena = np.zeros(rows * N, complex)
    opt = dict(tabB=tab, tabCi=tab, tabCo=tab, tab_stride=stride, offB=0, offCi=K, offCo=K + M, ldx=N, arena_rows=rows, Bx=arena, Cix=arena, Cox=arena.copy())
    return a, opt


def test_zgemm_ex_refuses_malformed_input_before_it_touches_a_device(helm_lib):
    """Every case is refused with HELM_ERR_ARG by the host-side check that runs before hipSetDevice: the answer is the same with and without a GPU
    (a well-formed call answers HELM_ERR_DEVICE on a host without one)."""
    def rc(a, **opt):
        return zs.zgemm_ex(helm_lib, *a, **opt)[0]
    # leading dimensions smaller than the width
    for i in (5, 8, 11):
        a = dense_args(pad=1)
        a[i] -= 2
        assert rc(a) == HELM_ERR_ARG, i
    # buffers shorter than the strides say, negative strides, overlapping items of C
    for i, v in ((4, 'short'), (7, 'short'), (10, 'short'), (6, -1), (9, -1), (12, 0)):
        a = dense_args()
        a[i] = a[i][:-1] if v == 'short' else v
        assert rc(a) == HELM_ERR_ARG, i
    # non-positive dimensions, forcing outside the instantiations, masks outside the matrix
    for i in (0, 1, 2, 3):
        a = dense_args()
        a[i] = 0
        assert rc(a) == HELM_ERR_ARG
    a = dense_args()
    for opt in (dict(force_tile=9), dict(force_tile=3, force_slab=16), dict(force_tile=8), dict(xcd_map=3), dict(zr=(5, 21)), dict(zr=(7, 5)), dict(zc=(0, 31)),
                dict(sk=(3, 21)), dict(sk=(-1, 4)), dict(k2=1), dict(cj_out=1), dict(act=np.zeros(8, np.int32))):
        assert rc(a, **opt) == HELM_ERR_ARG, opt
    # one row tile per matrix with more than 64 rows; C over B without it, or with strides that differ
    assert rc(dense_args(M=65), tm64=1) == HELM_ERR_ARG
    a = dense_args(M=10, K=10)
    a[10] = None
    assert rc(a, c_is_b=1) == HELM_ERR_ARG
    a[11] += 1
    assert rc(a, c_is_b=1, tm64=1) == HELM_ERR_ARG
    # row tables: an index outside its arena, K above the kernel's table of B rows, a table shorter than the batch needs, a missing arena
    a, opt = table_args()
    for name in ('tabB', 'tabCi', 'tabCo'):
        o = dict(opt)
        t = o[name].copy()
        t[len(t) // 2 + {'tabB': 0, 'tabCi': 10, 'tabCo': 30}[name]] = 64
        o[name] = t
        assert rc(a, **o) == HELM_ERR_ARG, name
    assert rc(a, **dict(opt, tab_len=len(opt['tabB']) - 1)) == HELM_ERR_ARG
    assert rc(a, **dict(opt, ldx=29)) == HELM_ERR_ARG
    assert rc(a, **dict(opt, k2=11)) == HELM_ERR_ARG
    for name in ('Bx', 'Cix', 'Cox'):
        assert rc(a, **dict(opt, **{name: None})) == HELM_ERR_ARG, name
    assert rc(a, **dict(opt, Cox2=opt['Cox'])) == HELM_ERR_ARG
    a[14] = 1 + 0j                                        # beta != 0 without tabCi reads the dense C, which is not there
    assert rc(a, **dict(opt, tabCi=None, Cix=None)) == HELM_ERR_ARG
    a[14] = 0j
    big, bopt = table_args(K=513, rows=600)
    assert rc(big, **bopt) == HELM_ERR_ARG
    ok, oopt = table_args(K=512, rows=600)
    assert rc(ok, **oopt) != HELM_ERR_ARG
    # ... and the well-formed calls these were made from pass the check
    assert rc(dense_args()) != HELM_ERR_ARG and rc(dense_args(pad=1)) != HELM_ERR_ARG
    assert rc(a, **opt) != HELM_ERR_ARG
