"""Forward wavefields kept in HBM between `prob.fieldsDevice(m)`, `survey.dpred(m, u=F)` and `prob.Jtvec(m, v, u=F)`.

The reference solves the forward fields once per model and uses them twice (`u = prob.fields(m)`, then `dpred(m, u=u)` and `Jtvec(m, resid, u=u)`:
problem.py:124-164, survey.py:190-198).  `DeviceFields` is that `u` with the arrays left where they were solved: one torch tensor per work item
(frequency, source batch) of shape (k, Ni) in layout 'rhs' on the item's GPU, the items it was dealt, the problem's model stamp at the time, and
the system's scaleTerm (the store holds the unscaled solves, as the mux pipeline's buffers do).  The pipelines that fill and read it are
`device_survey.fields`, `dpredFromFields` and `gradientFromFields`.

A 2.5-D problem may keep the fields of every cross-line wavenumber apart (`fieldsDevice(perKy=True)`): a slice then has a leading ky axis, and `LiveKyFields` stands
for such a store where `u=None` asks for none to be allocated.

The store is complex128, or complex64 with one power-of-two scale per column (`fieldsDtype='complex64'`, half the memory): `pack_reference` /
`unpack_reference` state that format in numpy, csrc/survey.hip (the pack) and csrc/survey_internal.hpp (the readers) implement it.
"""
import numpy as np

from . import _lib

DTYPES = ('complex128', 'complex64')
EXP_CLAMP = 1021            # 2^+-1021 are normal doubles: scaling by them is exact


def pack_reference(U):
    """(P, e) of the complex64 store for the columns of U (N, nsrc) complex: e[s] the binary exponent of m_s = max_i max(|Re|, |Im|)
    (2^e <= m_s < 2^(e+1), clamped to +-1021, 0 for a zero column; NaN entries do not count), P[:, s] = complex64(U[:, s] * 2^-e[s]) rounded to nearest."""
    U = np.asarray(U, dtype=np.complex128)
    U = U.reshape((U.shape[0], -1))
    comp = np.maximum(np.abs(U.real), np.abs(U.imag))
    m = np.fmax.reduce(comp, axis=0, initial=0.0) if comp.shape[0] else np.zeros(U.shape[1])
    _, ex = np.frexp(m)                              # m = f * 2^ex with 0.5 <= f < 1 (subnormal m included): the binary exponent is ex - 1
    e = np.where(m == 0, 0, np.where(np.isfinite(m), np.clip(ex.astype(np.int64) - 1, -EXP_CLAMP, EXP_CLAMP), EXP_CLAMP)).astype(np.int32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        s = np.ldexp(1.0, -e)[None, :]
        P = np.empty(U.shape, dtype=np.complex64)
        P.real = (U.real * s).astype(np.float32)
        P.imag = (U.imag * s).astype(np.float32)
    return P, e


def unpack_reference(P, e):
    'what a consumer of the complex64 store reads: complex128 (double)P[:, s] * 2^e[s]'
    P = np.asarray(P)
    P = P.reshape((P.shape[0], -1))
    s = np.ldexp(1.0, np.asarray(e, dtype=np.int32))[None, :]
    with np.errstate(under='ignore'):
        return (P.real.astype(np.float64) * s) + 1j * (P.imag.astype(np.float64) * s)


def check_fits(need, free):
    """MemoryError unless every device of `need` {device: bytes the store and its working buffers take there} finds them in `free` {device: bytes free}"""
    for dev in sorted(need):
        if need[dev] > free[dev]:
            raise MemoryError('the forward wavefields do not fit on GPU %s: %d bytes needed, %d bytes free (a store of half the size: fieldsDtype=\'complex64\')'
                              % (dev, need[dev], free[dev]))


class DeviceFields(object):
    """The forward wavefields of one model in device memory, as `fieldsDevice` left them.

    items:  [(worker, device, ifreq, c0, c1)], the work items the fields were solved as; dpred(u=F) and Jtvec(u=F) run over these again, so that every item
            finds its slice on its own GPU
    slices: one torch tensor (c1 - c0, Ni) per item, column s of the frequency's wavefields in row s - c0 (layout 'rhs'), unscaled
    exps:   None (complex128), or one int32 tensor (c1 - c0,) per item: the column exponents of the complex64 store
    stamp:  the problem's model stamp when the fields were solved; scale: the system's scaleTerm
    nky:    None, or the number of cross-line wavenumbers of a per-ky store of a 2.5-D problem (fieldsDevice(perKy=True)): a slice is then (nky, c1 - c0, Ni),
            block ky the unscaled solves of ky operator ky, and the exponents (nky, c1 - c0), one per column and ky; kyCoef the nky (alpha, beta) pairs of
            MiniZephyr25D._kyCoefficients the ky sum is formed with (the composite's own scale term inside).  nky None: a 2.5-D slice holds the ky SUM.
    """

    live = False             # (True: `LiveKyFields`, which holds nothing)

    def __init__(self, nfreq, nsrc, items, slices, exps=None, stamp=0, scale=1.0, dtype='complex128', nky=None, kyCoef=None):
        if dtype not in DTYPES:
            raise ValueError('fieldsDtype is %r: one of %s' % (dtype, ', '.join(DTYPES)))
        if len(items) != len(slices) or (exps is not None and len(exps) != len(items)):
            raise ValueError('one slice (and one exponent vector) per item')
        self.nfreq, self.nsrc = int(nfreq), int(nsrc)
        self.items = [tuple(it) for it in items]
        self.stamp, self.scale, self.dtype = stamp, complex(scale), dtype
        self.nky = None if nky is None else int(nky)
        self.kyCoef = None if kyCoef is None else [(complex(a), complex(b)) for a, b in kyCoef]
        self._store = {(it[2], it[3]): (sl, None if exps is None else exps[j]) for j, (it, sl) in enumerate(zip(self.items, slices))}

    def __len__(self):
        return self.nfreq

    @property
    def ownedFreqs(self):
        'the frequencies held here, in the order they were dealt'
        seen = []
        for _, _, ifreq, _, _ in self.items:
            if ifreq not in seen:
                seen.append(ifreq)
        return seen

    @property
    def released(self):
        return bool(self.items) and not self._store

    def checkCurrent(self, prob, perKy=False):
        """ValueError unless these are the fields of the problem's current model (and still held) and of the kind the caller reads: perKy False, the fields (of
        a 2.5-D problem: the ky sum); True, the per-ky store of fieldsDevice(perKy=True); None, either"""
        if self.released:
            raise ValueError('these device fields were released')
        if perKy is not None and bool(perKy) != (self.nky is not None):
            if perKy:
                raise ValueError('these device fields hold the ky SUM: the exact derivatives of a 2.5-D problem need the fields per ky, fieldsDevice(perKy=True)')
            raise ValueError('these device fields hold the fields per ky (fieldsDevice(perKy=True)), which the exact derivatives and dpred read: this route reads the '
                             'ky sum, fieldsDevice()')
        if self.stamp != getattr(prob, '_modelStamp', None):
            raise ValueError('these device fields belong to an earlier model (stamp %s, the problem is at %s): call fieldsDevice() again after updateModel'
                             % (self.stamp, getattr(prob, '_modelStamp', None)))

    def slice(self, ifreq, c0):
        '(tensor, exponents or None) of the item that starts at source c0 of frequency ifreq'
        return self._store[(ifreq, c0)]

    def pointers(self, ifreq, c0, ky=None):
        """(d_u, d_exp) of that item as the kernels take them: the device address of its slice, and of its column exponents or None (complex128).  ky: of block
        ky of a per-ky store, (c1 - c0, Ni) like the slice of a plain one"""
        sl, ex = self._store[(ifreq, c0)]
        if ky is None:
            return sl.data_ptr(), None if ex is None else ex.data_ptr()
        if self.nky is None or not 0 <= int(ky) < self.nky:
            raise IndexError('block %r of a store with nky = %r' % (ky, self.nky))
        ky = int(ky)
        return sl.data_ptr() + ky * sl.stride(0) * sl.element_size(), None if ex is None else ex.data_ptr() + ky * ex.stride(0) * ex.element_size()

    def _download(self, sl, ex):
        'the (Ni, k) complex128 columns of a (k, Ni) slice or block, unpacked where the store is complex64'
        part = np.asarray(_lib.from_device_pinned(sl))
        return np.array(part.T) if ex is None else unpack_reference(part.T, np.asarray(_lib.from_device(ex)))

    def kyBlocks(self, ifreq):
        """(nky, N, nsrc) complex128: the fields of frequency ifreq per ky, downloaded, every block scaled by the scale terms of the wrapper and of the composite
        -- what prob.fields(perKy=True)[ifreq] would be, and what the host routes of the exact 2.5-D derivatives take"""
        if self.nky is None:
            raise ValueError('these device fields hold the ky SUM: fieldsDevice(perKy=True) keeps the fields per ky')
        mine = [it for it in self.items if it[2] == int(ifreq) and (int(ifreq), it[3]) in self._store]
        if not mine:
            raise KeyError('frequency %d is not held by this store (held: %s)' % (ifreq, self.ownedFreqs if self._store else 'nothing'))
        out = None
        for _, _, _, c0, c1 in mine:
            sl, ex = self._store[(int(ifreq), c0)]
            for ky in range(self.nky):
                part = self._download(sl[ky], None if ex is None else ex[ky])
                if out is None:
                    out = np.empty((self.nky, part.shape[0], self.nsrc), dtype=np.complex128)
                out[ky, :, c0:c1] = part
        return out * (self.scale * self.kyCoef[-1][0])          # (alpha of the last term is the composite's scale term)

    def __getitem__(self, ifreq):
        'the (N, nsrc) complex128 array prob.fields()[ifreq] would be: downloaded, scaled by scaleTerm'
        ifreq = int(ifreq)
        if ifreq < 0:
            ifreq += self.nfreq
        mine = [it for it in self.items if it[2] == ifreq and (ifreq, it[3]) in self._store]
        if not mine:
            raise KeyError('frequency %d is not held by this store (held: %s)' % (ifreq, self.ownedFreqs if self._store else 'nothing'))
        if self.nky is not None:
            # the ky sum in the order and with the coefficients the composite forms it with (MiniZephyr25D._kyCoefficients), then the wrapper's scale
            out = None
            for _, _, _, c0, c1 in mine:
                sl, ex = self._store[(ifreq, c0)]
                acc = None
                for ky, (a, b) in enumerate(self.kyCoef):
                    part = a * self._download(sl[ky], None if ex is None else ex[ky])
                    acc = part if acc is None else b * acc + part
                if out is None:
                    out = np.empty((acc.shape[0], self.nsrc), dtype=np.complex128)
                out[:, c0:c1] = acc
            if self.scale != 1.0:
                out *= self.scale
            return out
        out = None
        for _, _, _, c0, c1 in mine:
            sl, ex = self._store[(ifreq, c0)]
            part = np.asarray(_lib.from_device_pinned(sl))                   # (c1 - c0, Ni)
            if out is None:
                out = np.empty((part.shape[1], self.nsrc), dtype=np.complex128)
            out[:, c0:c1] = part.T if ex is None else unpack_reference(part.T, np.asarray(_lib.from_device(ex)))
        if self.scale != 1.0:
            out *= self.scale
        return out

    def __iter__(self):
        'the frequencies one at a time, each downloaded when it is asked for: list(F) is what prob.fields() returns'
        return (self[i] for i in range(self.nfreq))

    @property
    def nbytes(self):
        '{device: bytes of this store held there}'
        held = {}
        for _, dev, ifreq, c0, _ in self.items:
            if (ifreq, c0) in self._store:
                sl, ex = self._store[(ifreq, c0)]
                held[dev] = held.get(dev, 0) + sl.numel() * sl.element_size() + (0 if ex is None else ex.numel() * ex.element_size())
        return held

    def release(self):
        'free the store (the tensors go back to the allocator of their device); the object remembers only what it was'
        self._store = {}


class LiveKyFields(DeviceFields):
    """`u=None` of the exact derivatives of a 2.5-D problem on the device: the items a per-ky store would be dealt and its coefficients, and NO store -- the
    pipelines of device_survey solve the forward fields of a ky into their workspace just before they use them (`qf`: the survey's source columns) and drop
    them.  It stands where a per-ky DeviceFields stands; nothing can be downloaded from it."""

    live = True

    def __init__(self, nfreq, nsrc, items, stamp, scale, nky, kyCoef, qf):
        DeviceFields.__init__(self, nfreq, nsrc, items, [None] * len(items), None, stamp, scale, 'complex128', nky=nky, kyCoef=kyCoef)
        self.qf = qf

    @property
    def released(self):
        return False

    @property
    def nbytes(self):
        return {}

    def pointers(self, ifreq, c0, ky=None):
        raise ValueError('these fields are solved when they are used and are not held: fieldsDevice(perKy=True) keeps them')

    slice = kyBlocks = __getitem__ = pointers
