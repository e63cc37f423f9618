"""Survey geometry: source / receiver vectors, data projection, residual back-sources.

Interface of zephyr/middleware/survey.py:27-206 (HelmBaseSurvey / Helm2DSurvey) without the SimPEG
base classes: the arithmetic on the hot path (getSources, _lazyProjectFields,
getResidualSources, dpred) is kept, the inversion-framework glue is not.
"""
import numpy as np
import scipy.sparse as sp

from .config import BaseSCCache
from .source import SparseKaiserSource
from . import parallel
from . import device_survey
from .fieldstore import DeviceFields


class HelmBaseSurvey(BaseSCCache):

    initMap = {
        #   key            required  rename        cast
        'geom':           (True,     None,         dict),
        'freqs':          (True,     None,         tuple),
        'sterms':         (False,    '_sterms',    np.complex128),
    }

    def __init__(self, systemConfig, **kwargs):
        BaseSCCache.__init__(self, systemConfig, **kwargs)
        self.prob = None

    # ---- geometry ------------------------------------------------------------------------------
    # What the reference spells out as one property per key (survey.py:52-107) is a table here: attribute -> (key of `geom`, default when the
    # key is absent).  Defaults that depend on the survey are callables of it.
    _GEOM_FIELDS = {
        'mode':    ('mode',   'fixed'),
        'sLocs':   ('src',    None),
        'rLocs':   ('rec',    None),
        'ssTerms': ('sterms', lambda sv: np.ones((sv.nsrc,), dtype=np.complex128)),
        'srTerms': ('rterms', lambda sv: np.ones((sv.nrec,), dtype=np.complex128)),
    }

    def __getattr__(self, name):
        # (only reached for names that are not instance / class attributes)
        fields = type(self)._GEOM_FIELDS
        if name in fields:
            key, default = fields[name]
            geom = self.__dict__.get('_geom')
            if geom is None:
                raise AttributeError(name)
            if key in geom:
                return geom[key]
            return default(self) if callable(default) else default
        raise AttributeError('%s has no attribute %r' % (type(self).__name__, name))

    @property
    def geom(self):
        return self._geom

    @geom.setter
    def geom(self, value):
        if value.get('mode', 'fixed') not in {'fixed', 'relative'}:
            raise Exception('%s objects only work with \'fixed\' or \'relative\' receiver arrays' % (self.__class__.__name__,))
        self._geom = value

    @property
    def nfreq(self):
        return len(self.freqs)

    @property
    def tsTerms(self):
        return self.__dict__.get('_sterms', np.ones(self.nfreq, dtype=np.complex128))

    @staticmethod
    def _rows(locs):
        return 0 if locs is None else locs.shape[0]

    nsrc = property(lambda self: self._rows(self.sLocs))
    nrec = property(lambda self: self._rows(self.rLocs))
    nD = property(lambda self: self.nsrc * self.nrec * self.nfreq)

    @property
    def RHSGenerator(self):
        gen = self.__dict__.get('_RHSGenerator')
        if gen is None:
            gen = self._RHSGenerator = self.geom.get('GeneratorClass', SparseKaiserSource)
        return gen

    # ---- source / receiver vectors (survey.py:109-128) ------------------------------------------------
    def _vecKey(self, kind, ifreq, *source):
        'key (kind, grid key of frequency ifreq[, source]) of an entry of the vector cache: the one spelling of its keys'
        return (kind, self._gridKey(ifreq)) + source

    def _cachedOn(self, kind, ifreq, make, *source):
        'the entry of the vector cache under _vecKey(kind, ifreq[, source]), made by make() on first use'
        cache = self.__dict__.setdefault('_vecCache', {})
        key = self._vecKey(kind, ifreq, *source)
        if key not in cache:
            cache[key] = make()
        return cache[key]

    def sVecs(self, ifreq=0):
        'source matrix S diag(ssTerms) on the grid of frequency ifreq, (N_ifreq, nsrc); made once per grid'
        return self._cachedOn('S', ifreq, lambda: self._weightedColumnsOn(ifreq, self.sLocs, self.ssTerms))

    def rVec(self, isrc, ifreq=0):
        """receiver sampling matrix of source isrc on the grid of frequency ifreq, (nrec, N_ifreq): one for all sources with a fixed array, one per source
        when the array moves with it"""
        moving = self.mode != 'fixed'
        return self._cachedOn('R', ifreq, lambda: self._weightedColumnsOn(ifreq, self.rLocs + self.sLocs[isrc] if moving else self.rLocs, self.srTerms).T,
                              *((isrc,) if moving else ()))

    def rVecs(self, ifreq):
        return (self.rVec(i, ifreq) for i in range(self.nsrc))

    def _gridKey(self, ifreq):
        'which cached vectors frequency ifreq uses (None: the one grid of this survey)'
        return None

    def scaledConfig(self, ifreq):
        'the survey config on the grid of frequency ifreq (one grid for every frequency here)'
        return self.systemConfig

    def _weightedColumnsOn(self, ifreq, locs, terms):
        'one column per location from the survey\'s source generator on the grid of frequency ifreq, column j scaled by terms[j]'
        return self.RHSGenerator(self.scaledConfig(ifreq))(locs) * sp.diags((terms,), (0,))

    # ---- a moving array as ONE matrix: what the device paths of problem.py upload ---------------------------------
    def stackedReceivers(self, ifreq=0):
        """The receiver matrices of every source in one CSR, (nsrc * nrec, N): row s * nrec + r is row r of rVec(s).  Made by ONE call of the generator
        rVec uses, on the concatenated locations -- the same entries to the bit, so whatever the host path does with a location (clipping at the edges,
        a free surface) is what the device samples.  One per grid key; the rows of the sources c0 .. c1-1 are the contiguous range
        indptr[c0 * nrec : c1 * nrec + 1]."""
        def stack():
            moving = self.mode != 'fixed'
            where = np.concatenate([self.rLocs + self.sLocs[s] if moving else self.rLocs for s in range(self.nsrc)])
            M = sp.csr_matrix(self._weightedColumnsOn(ifreq, where, np.tile(self.srTerms, self.nsrc)).T)
            M.sum_duplicates()
            return M
        return self._cachedOn('Rstack', ifreq, stack)

    def adjointPlan(self, ifreq=0):
        """getResidualSources as a gather: the entries of stackedReceivers sorted by (source, cell, receiver) and grouped into the touched (source, cell)
        pairs.  A dict of
            tptr (ntouch + 1, int64)   entries tptr[t] .. tptr[t+1] of trec / tval belong to pair t
            tsrc (ntouch, int32), tcell (ntouch, int64)   the pair's source and grid cell
            trec (nnz, int32), tval (nnz, complex128)     receiver and weight of every entry, by receiver within a pair
            src_ptr (nsrc + 1, int64)  pairs src_ptr[c0] .. src_ptr[c1] are those of the sources c0 .. c1-1: a batch is a sub-range, nothing is copied
        so that  qb[cell, s] = sum_e tval[e] resid[trec[e], s]  over the entries of pair (s, cell), summed in stored order (receivers of one source share
        cells: the patches of neighbours overlap).  Validated here -- helm_rhs_from_samples_device trusts it."""
        def build():
            M = self.stackedReceivers(ifreq)
            nrec, nsrc, N = self.nrec, self.nsrc, M.shape[1]
            row = np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr))
            src, rec, cell = row // nrec, row % nrec, M.indices.astype(np.int64)
            order = np.lexsort((rec, cell, src))                 # by source, then cell, then receiver
            src, rec, cell, val = src[order], rec[order], cell[order], M.data[order]
            first = np.ones(src.size, dtype=bool)
            first[1:] = (src[1:] != src[:-1]) | (cell[1:] != cell[:-1])
            starts = np.flatnonzero(first)
            plan = dict(tptr=np.append(starts, src.size).astype(np.int64), tsrc=src[starts].astype(np.int32), tcell=cell[starts].astype(np.int64),
                        trec=rec.astype(np.int32), tval=np.ascontiguousarray(val, dtype=np.complex128), nrec=nrec, nsrc=nsrc, rows=N)
            plan['src_ptr'] = np.searchsorted(plan['tsrc'], np.arange(nsrc + 1)).astype(np.int64)
            if src.size and not (0 <= cell.min() and cell.max() < N and 0 <= rec.min() and rec.max() < nrec and 0 <= src.min() and src.max() < nsrc
                                 and np.all(np.diff(plan['tsrc']) >= 0) and np.all(np.diff(plan['tptr']) >= 1)):
                raise ValueError('adjoint plan of the receiver array addresses cells, receivers or sources outside the survey')
            return plan
        return self._cachedOn('Rplan', ifreq, build)

    # ---- hot-path pieces ------------------------------------------------------------------------------
    def getSources(self):
        'per-frequency source matrices qf[f] = S diag(ssTerms) conj(tsTerms[f]) (survey.py:162-169)'
        qs = self.sVecs()
        ts = self.tsTerms
        if isinstance(ts, (list, np.ndarray)):
            ts = np.asarray(ts)
            if ts.ndim < 2:
                return [qs * t.conjugate() for t in ts]
            return [qs * sp.diags((t.conjugate(),), (0,)) for t in ts]
        return qs

    def _projectOne(self, uFreq, out, ifreq=0):
        'out[:, isrc] = R_isrc uFreq[:, isrc] for one frequency'
        if self.mode == 'fixed':
            out[:, :] = self.rVec(0, ifreq) * uFreq
        else:
            for isrc in range(self.nsrc):
                out[:, isrc] = self.rVec(isrc, ifreq) * uFreq[:, isrc]

    def _lazyProjectFields(self, u, owned=None):
        'data[:, isrc, ifreq] = R uF_ifreq[:, isrc] (survey.py:152-160); `owned` lists the frequency indices `u` yields'
        data = np.zeros((self.nrec, self.nsrc, self.nfreq), dtype=np.complex128)
        idx = range(self.nfreq) if owned is None else owned
        for ifreq, uFreq in zip(idx, u):
            self._projectOne(np.asarray(uFreq), data[:, :, ifreq], ifreq)
        return data

    def getResidualSources(self, resid):
        """back-sources qb[f][:, s] = R_s^T resid[:, s, f] (survey.py:171-188).  With a fixed receiver array every source shares one R, and the nsrc
        sparse products per frequency of the reference collapse into one, R^T (resid[:, :, f]) -- the same columns, built in one call."""
        if self.mode == 'fixed':
            # R^T is N x nrec with a patch of cells per receiver: only the rows some receiver touches are nonzero.  One sparse x dense product on those
            # rows per frequency (R^T restricted to them stays CSR: ~81 entries per receiver whatever nrec is -- densified it would be O(nrec^2)),
            # handed back as a CSR matrix built from its arrays (sorted rows, every column present): no sparse-sparse product, no sort.
            cache = self.__dict__.setdefault('_vecCache', {})
            ns = resid.shape[1]
            out, layouts = [], {}
            for ifreq in range(self.nfreq):
                key = self._vecKey('RtRows', ifreq)       # (one R per grid: a multiscale survey has one per distinct scale; the key serves `layouts` too)
                if key not in cache:
                    Rt = sp.csr_matrix(self.rVec(0, ifreq).T)
                    Rt.sum_duplicates()
                    rows = np.flatnonzero(np.diff(Rt.indptr))
                    cache[key] = (rows, sp.csr_matrix(Rt[rows, :]), Rt.shape[0])
                rows, Rsub, N = cache[key]
                if key not in layouts:
                    indptr = np.zeros(N + 1, dtype=np.int64)
                    indptr[rows + 1] = ns
                    np.cumsum(indptr, out=indptr)
                    layouts[key] = (indptr, np.tile(np.arange(ns, dtype=np.int32), rows.size))
                indptr, indices = layouts[key]
                block = np.asarray(Rsub @ np.ascontiguousarray(resid[:, :, ifreq]))      # sparse (rows, nrec) x dense (nrec, nsrc) -> dense (rows, nsrc)
                m = sp.csr_matrix((block.ravel(), indices, indptr), shape=(N, ns))
                m.has_sorted_indices = True
                out.append(m)
            return out
        return [sp.hstack([self.rVec(isrc, ifreq).T * sp.csc_matrix(resid[:, isrc, ifreq].reshape((self.nrec, 1)))
                           for isrc in range(self.nsrc)])
                for ifreq in range(self.nfreq)]

    def dpred(self, m=None, u=None):
        'predicted data, ravel of (nrec, nsrc, nfreq) in C order (survey.py:190-198)'
        if self.prob is None:
            raise Exception('%s instance is not paired to a problem' % (self.__class__.__name__,))
        if u is None:
            owned = self.prob.ownedFreqs
            if sp.issparse(self.sVecs(0)) and self.prob._deviceGradientAvailable():
                self.prob.updateModel(m)
                data = self.prob._dpredDevice(owned)          # wavefields never leave HBM
            else:
                data = self._lazyProjectFields(self.prob.lazyFields(m), owned)
            if self.prob._sharded:
                data = parallel.allreduce_sum(data)
            return data.ravel()
        if isinstance(u, DeviceFields):
            # forward fields left in HBM by prob.fieldsDevice(): sampled there, only the receiver panels come back
            self.prob.updateModel(m)
            data = device_survey.dpredFromFields(self.prob, u)
            if self.prob._sharded:
                data = parallel.allreduce_sum(data)
            return data.ravel()
        return self._lazyProjectFields(u).ravel()

    @property
    def postProcessors(self):
        return [lambda x: x for _ in self.freqs]

    @property
    def preProcessors(self):
        return [lambda x: x for _ in self.freqs]


class HelmMultiGridSurvey(HelmBaseSurvey):
    """Survey of a multiscale problem (zephyr/middleware/survey.py:209-334): frequency i lives on the grid of MultiGridHelper's scale i.
    Source and receiver vectors are made by the survey's source generator on that grid (one cache per distinct scale), `getSources()` and
    `getResidualSources()` return per-frequency matrices on those grids, and the pre- / post-processors are the down- / up-scalers.
    The config carries what MultiGridHelper needs (cMin, targetGPW; maxScale, minScale optional).  Unlike the reference, a receiver array
    that moves with the source (mode 'relative') is cached per scale and source."""

    @property
    def mgHelper(self):
        if '_mgHelper' not in self.__dict__:
            from .distributors import MultiGridHelper
            sc = dict(self.systemConfig)
            sc['freqs'] = list(self.freqs)
            self._mgHelper = MultiGridHelper(sc)
        return self._mgHelper

    @property
    def postProcessors(self):
        return self.mgHelper.upScalers

    @property
    def preProcessors(self):
        return self.mgHelper.downScalers

    def _gridKey(self, ifreq):
        return self.mgHelper.scales[ifreq]

    def scaledConfig(self, ifreq):
        'the survey config on the grid of frequency ifreq (survey.py:246-253)'
        scs = self.__dict__.setdefault('_scScales', {})
        key = self._gridKey(ifreq)
        if key not in scs:
            sc = dict(self.systemConfig)
            sc.update(self.mgHelper.downScalers[ifreq].scaleUpdate)
            scs[key] = sc
        return scs[key]

    def getSources(self):
        'per-frequency source matrices on their grids (survey.py:289-297)'
        ts = self.tsTerms
        if isinstance(ts, (list, np.ndarray)):
            out = []
            for ifreq, t in enumerate(np.asarray(ts)):
                qs = self.sVecs(ifreq)
                out.append(qs * sp.diags((t.conjugate(),), (0,)) if np.ndim(t) > 0 else qs * t.conjugate())
            return out
        return [self.sVecs(ifreq) * np.conjugate(ts) for ifreq in range(self.nfreq)]

    def _projectOne(self, uFreq, out, ifreq=0):
        # (wavefields up-scaled to the native grid, as fields() returns them, are brought back to the frequency's grid first: survey.py:264-275)
        if uFreq.shape[0] != self.rVec(0, ifreq).shape[1]:
            uFreq = self.preProcessors[ifreq] * uFreq
        HelmBaseSurvey._projectOne(self, uFreq, out, ifreq)


class Helm2DSurvey(HelmBaseSurvey):
    pass


class Helm3DSurvey(HelmBaseSurvey):
    """Survey on a 3-D grid (no counterpart in the reference, whose sources refuse `ny`): the config carries nx, ny, nz (and dx, dy, dz, the origins), and
    `geom` (x, y, z) triples as source and receiver locations -- for mode 'relative' the receiver triples are offsets from each source.  Everything else is
    HelmBaseSurvey: the source generator (SparseKaiserSource by default, its separable 3-D form) makes the columns of S and the rows of R on the one grid, and
    `dpred`, the stacked receivers and the adjoint plan work on N = nz ny nx rows.  Pairs with Helm3DProblem only."""

    def __init__(self, systemConfig, **kwargs):
        if systemConfig.get('ny', None) is None:
            raise ValueError('Helm3DSurvey requires parameter \'ny\': without it the config describes a 2-D grid (Helm2DSurvey)')
        HelmBaseSurvey.__init__(self, systemConfig, **kwargs)
        for name, key in (('sLocs', 'src'), ('rLocs', 'rec')):
            locs = getattr(self, name)
            if locs is not None and (np.ndim(locs) != 2 or np.shape(locs)[1] != 3):
                raise ValueError('geom[%r] of a Helm3DSurvey is an (n, 3) array of (x, y, z) locations, not of shape %s' % (key, np.shape(locs)))


class Helm2DMultiGridSurvey(Helm2DSurvey, HelmMultiGridSurvey):
    'zephyr/middleware/survey.py:337-340'
    pass


class Helm25DSurvey(HelmBaseSurvey):
    'zephyr/middleware/survey.py:343-346'
    pass


class Helm25DMultiGridSurvey(Helm25DSurvey, HelmMultiGridSurvey):
    'zephyr/middleware/survey.py:349-350'
    pass

