"""Device pipeline of a survey: `Survey.dpred` and the mux branch of `Problem.Jtvec` with the wavefields kept in HBM.

Both are the same loop.  The owned frequencies are dealt as work items (frequency, source batch) over the GPUs (`deviceItems`), every item runs on
the worker thread of its GPU with the next item's factorisation started ahead of time (`runOnDevices`), and its device memory comes from the
`Workspace` of its worker and GPU, which lives for one call.  An item of `dpred` expands its sources, solves and samples; an item of `gradient` fills
[qf | qb], solves and adds its imaging sum to the worker's partial gradient by one of two adding steps, chosen once per call.

The same loop serves forward fields that outlive a call (`fieldstore.DeviceFields`, at the end of the module): `fields` solves them into a store,
`dpredFromFields` samples the store and `gradientFromFields` images against it, both over the items the store recorded.  `illumination` and
`illuminationFromFields` (last section) are the same two loops again with the energy kernel in the place of the imaging kernel and a float64 partial.

The pipelines, one row each.  Every row is a body of its own made of the shared item steps of the next section.

    pipeline                items                what fills R                        columns solved   what consumes U                       what comes down
    dpred                   dealt                source columns                      k                sampleDevice (2.5-D: sampleSumDevice) nrec x k samples per item
    fields                  dealt, then stored   source columns                      k                the store's slice (complex64: pack)   nothing
    dpredFromFields         stored               --                                  0                -- (sampleDevice reads the slice)     nrec x k samples per item
    bornFromFields          stored               virtual sources conj(W (.) slice)   k                sampleDevice, conjugated receivers    nrec x k samples per item
      linearisation='operator'                   coef mask M0(W (.) conj(slice))     k                sampleDevice, receivers as they are   nrec x k samples per item
      parameter='rho'                            coef sum_k L[db]_k shift_k(conj(slice)) k            sampleDevice, receivers as they are   nrec x k samples per item
      linearisation='full'                       the same with the planes V[dc] (+ L[db]) k           sampleDevice, receivers as they are   nrec x k samples per item
    gradient                dealt                [qf | qb]                           2k               imaging kernel, uF and uB from U      one partial G per worker
    gradientFromFields      stored               qb                                  k                imaging kernel, uF from the slice     one partial G per worker
      linearisation='operator'                   qb of R^H r                         k                imaging kernel with the mass stencil  one partial G per worker
      parameter='rho'                            qb of R^H r                         k                lag imaging into P, then L^T P        one partial G per worker
      linearisation='full'                       qb of R^H r                         k                lag imaging into P, then V^T P        one partial G per worker
                                                                                                      (no `rho`: and L^T P into Gb)         (and one Gb)
    newtonFromFields        stored               qb of R^H r; the planes of p on     3k               lag imaging into P0 and P1, then      one partial G per worker
                                                 the slice; the gathered samples of                   V^T P1 and the curvature kernel on P0 (parameter='rho': and one Gb)
                                                 du plus the transposed planes on lambda
      parameter='joint'                          the same with the planes of [c; rho]  3k               the same, and the two mixed transposes one stacked partial G (2N), and Gb
                                                                                                      on P0 (k_velocity_adjoint_b, k_mixed_adjoint)
    jointGradientFromFields stored               qb of R^H r                         k                lag imaging into P, then V^T P and    one stacked partial G (2N) per worker
                                                                                                      L^T P into the halves of G
    kyBornFromFields        stored (per ky)      per ky: the planes of the ky handle   nky k            per ky: samples accumulated on the    nrec x k samples per item
                                                 on the block of that ky                              device into the item's result
    kyGradientFromFields    stored (per ky)      qb of R^H r, once per item            nky k            per ky: lag imaging into P against    one stacked partial G (2N) per worker
                                                                                                      the block of that ky, V_ky^T P, L_ky^T P
    misfitFromFields        stored               -- (the samples of the slice become   0, then the k    the misfit kernels on the sample      3 k doubles per item, twice; then what
                                                 the adjoint source, in place)        of the gradient  panel, then the gradient pipeline     the gradient pipeline brings down
    misfitOnePass           dealt                source columns, then the gather      2k               sampling and the misfit kernels, then 3 k doubles per item, twice; one
                                                 from the item's adjoint source                        the imaging or plane kernels on U     partial G per worker
    illumination           dealt                source or receiver columns          k                energy kernel                         one partial H per worker
    illuminationFromFields  stored               --                                  0                -- (energy kernel reads the slice)    one partial H per worker
      kind='gaussNewton'                         receiver columns, once per worker   nrec, once per   lag Gram of the slice, then the       one partial H per worker
                                                 and frequency                       worker and freq. combine kernel

Three rules hold everywhere below.  The shared steps carry them, so that a new pipeline inherits them with the steps it calls, and
tests/test_gpu_pipeline_order.py holds the order of library calls and waits of every item against a recorded one.

* Stream hand-over.  The library runs on its own streams.  Every torch operation whose result a library call reads (an upload, an element-wise
  product, `zero_()`, `fill_()`, a fresh tensor the library writes) is followed by `_lib.wait_torch_stream(dev)` before that call.
* Main-thread preparation.  The survey's caches are not thread-safe: whatever the survey caches (`adjointPlan`, `stackedReceivers`, the fixed
  array's CSR, `getSources`, `getResidualSources`, the post-processors) is made on the calling thread before the workers start.
* Helper lookups.  `to_device`, `from_device` and `from_device_pinned` are reached as attributes of `_lib` at call time (`_lib.from_device(...)`),
  never imported by name: the transfer-counting tests replace them on the module.
"""
import math

import numpy as np
import scipy.sparse as sp

from . import _lib
from . import dispatch
from . import frechet
from . import parallel


class Workspace(object):
    """Device memory of one worker on one GPU for one call of dpred / Jtvec: named complex128 buffers whose storage only grows, the constants that
    are uploaded once (`cached`), the worker's partial gradient `G` (`Gb`: its buoyancy part where the density follows c) and its partial illumination `H`."""

    def __init__(self, device):
        self.device = device            # (a torch.device)
        self.G = None                   # (the partial gradient of this worker and GPU: made on first use by the gradient pipeline)
        self.Gb = None                  # (the partial buoyancy gradient of linearisation='full' without an explicit density: made on first use)
        self.H = None                   # (its partial illumination, float64 (N,) or (nfreq, N): made on first use by the illumination pipeline)
        self._storage = {}
        self._constants = {}

    def buffer(self, name, shape):
        'a contiguous complex128 view of exactly `shape` (a number of elements, or a tuple) over the storage of `name`: new storage only when the request exceeds it'
        import torch
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        n = math.prod(int(s) for s in shape)
        store = self._storage.get(name)
        if store is None or store.numel() < n:
            store = self._storage[name] = torch.empty(n, dtype=torch.complex128, device=self.device)
        return store[:n].view(shape)

    def cached(self, key, make, keep=None):
        'make() once per key.  `keep`: an object that has to live as long as the entry (one whose id is part of the key)'
        if key not in self._constants:
            self._constants[key] = (make(), keep)
        return self._constants[key][0]


# ---- dealing and running the items -------------------------------------------------------------------------------------------------------------
def _workerDevices(sysw):
    "the GPUs the workers of a system wrapper run on, in worker order (a wrapper without a parallel mode: the GPU of its first operator)"
    return list(sysw.devices) if hasattr(sysw, 'devices') else [sysw.subProblems[0].device]


def deviceItems(sysw, owned, ncols):
    """Work items (worker, operator, ifreq, c0, c1) for the owned frequencies: frequency-major over the system wrapper's devices (a GPU keeps the operators
    of its frequencies); with fewer frequencies than GPUs the `ncols` source columns of a frequency are split over the spare ones."""
    subs = sysw.subProblems
    devs = _workerDevices(sysw)
    nw = len(devs)
    split = max(1, nw // max(1, len(owned))) if hasattr(sysw, '_replica') else 1
    split = min(split, max(1, ncols))
    items = []
    for pos, ifreq in enumerate(owned):
        bounds = [ncols * j // split for j in range(split + 1)]
        for j in range(split):
            if j == 0:          # the frequency's own operator, on the worker of the GPU it lives on
                op = subs[ifreq]
                w = devs.index(op.device) if op.device in devs else (pos * split) % nw
                if split > 1 and devs[(pos * split) % nw] == op.device:
                    w = (pos * split) % nw
            else:               # a copy of it on a spare GPU for another batch of its sources
                w = (pos * split + j) % nw
                op = sysw._replica(ifreq, j, devs[w])
            items.append((w, op, ifreq, bounds[j], bounds[j + 1]))
    return devs, items


def runOnDevices(devs, items, fn, factor=True):
    """Run fn(ws, op, ifreq, c0, c1) for every item on the worker thread of its GPU, the factorisation of the worker's next item started ahead of
    time (factor=False: the items solve nothing, nothing is prepared).  `ws` is the worker's Workspace on the GPU of the operator it is running.
    Returns the workspaces, in worker order."""
    import torch
    workers = [{} for _ in devs]          # per worker: device index -> Workspace
    queues = [[] for _ in devs]
    # the factorisations of a worker's next two operators are enqueued together (discretization.prefactor_many: the fronts of both frequencies in the same
    # batched launches); an item's own prepare step then only builds and assembles its operator
    from .discretization import prefactor_many
    group = 2 if factor and all(getattr(type(op), 'VARIANT', None) in (_lib.HELM_MINIZEPHYR, _lib.HELM_EURUS) for _, op, _, _, _ in items) else 1      # (2-D operators: what helm_prefactor_many takes)
    for w, op, ifreq, c0, c1 in items:
        def solve(_p, w=w, op=op, ifreq=ifreq, c0=c0, c1=c1):
            ws = workers[w].get(op.device)
            if ws is None:
                ws = workers[w][op.device] = Workspace(torch.device('cuda', op.device))
            return fn(ws, op, ifreq, c0, c1)
        if not factor:
            prep = None
        elif group > 1:
            prep = (lambda op=op: (op.handle, op)[1])
        else:
            prep = op.prefactor if hasattr(op, 'prefactor') else None
        queues[w].append(dispatch.WorkItem(solve, prep))
    pipes = dispatch.dispatch(list(zip(devs, queues)), lookahead=1, group=group, group_prepare=prefactor_many if group > 1 else None)
    try:
        [it.future.result() for q in queues for it in q]
    finally:
        for p in pipes:
            p.join()
    return [ws for worker in workers for ws in worker.values()]


class DevicePanels(object):
    """(nrec, k) complex128 panels of work items, each on the GPU of its item: what stands for `resid` in the gradient pipelines when the adjoint source was made
    on the device (`misfitFromFields`).  panel(ifreq, c0, c1) is the tensor of the item with the sources c0 .. c1-1 of frequency ifreq."""

    def __init__(self):
        self._panels = {}

    def put(self, ifreq, c0, c1, tensor):
        self._panels[(int(ifreq), int(c0), int(c1))] = tensor

    def panel(self, ifreq, c0, c1):
        return self._panels[(int(ifreq), int(c0), int(c1))]


# ---- [qf | qb] of an item ----------------------------------------------------------------------------------------------------------------------
def _muxTriplets(mats, c0, c1, rows):
    """(row, col, val, shape) of [m_0[:, c0:c1] | m_1[:, c0:c1] | ...] from the matrices' own arrays (no format conversion, no sort of 10^5..10^6 entries):
    what rhsFromSparseDevice takes as triplets"""
    k = c1 - c0
    parts = []
    for j, m in enumerate(mats):
        mc = m if (c0 == 0 and c1 == m.shape[1]) else sp.csc_matrix(m)[:, c0:c1]
        if not (sp.isspmatrix_csr(mc) or sp.isspmatrix_csc(mc)) or not mc.has_canonical_format:
            mc = sp.csr_matrix(mc)
            mc.sum_duplicates()
        coo = mc.tocoo(copy=False)
        parts.append((coo.row, coo.col + j * k, coo.data))
    return (np.concatenate([p_[0] for p_ in parts]), np.concatenate([p_[1] for p_ in parts]), np.concatenate([p_[2] for p_ in parts]), (rows, len(parts) * k))


def _planOnDevice(ws, sv, ifreq):
    'the survey\'s adjoint plan of frequency ifreq\'s grid with its arrays on the workspace\'s GPU: uploaded once per worker and grid key'
    def upload():
        plan = sv.adjointPlan(ifreq)
        pd = dict(plan)
        for name in ('tptr', 'tsrc', 'tcell', 'trec', 'tval'):
            pd[name] = _lib.to_device(plan[name], ws.device)
        return pd
    return ws.cached(('plan', sv._gridKey(ifreq)), upload)


def _fillMuxDevice(ws, sv, op, qf_i, qb, resid, ifreq, c0, c1, d_R, rows):
    """d_R ([2k][rows], k = c1 - c0) = [qf | qb] of the sources c0 .. c1-1 of frequency ifreq.  qb given (fixed array): both halves as sparse triplets in
    one upload.  qb None (the array moves with the source): the qf half from triplets, the qb half by `_backSources`."""
    if qb is not None:
        op.rhsFromSparseDevice(_muxTriplets((qf_i, qb[ifreq]), c0, c1, rows), d_R)
        return
    op.rhsFromSparseDevice(_muxTriplets((qf_i,), c0, c1, rows), d_R)
    _backSources(ws, sv, op, None, resid, ifreq, c0, c1, d_R + (c1 - c0) * rows * 16, rows)


# ---- the item steps the pipelines share ----------------------------------------------------------------------------------------------------------
# A step may enqueue torch work (uploads, element-wise products, zero_(), fresh tensors) and does not wait for it: the item body issues the
# _lib.wait_torch_stream between its steps and the first library call that reads their results.  A step that itself calls the library on what it
# has just uploaded (`_backSources` for a moving array; rhsFromSparseDevice inside `_expandColumns`) waits before that call.  What a step needs from
# the survey's caches has a half that runs on the calling thread, before the workers start: `_prepareBackSources`, and the set-up of `_sampling`.

def _ofFrequency(q, ifreq):
    "the column matrix of frequency ifreq: `q` is one matrix per frequency (a multiscale survey), or one for all of them"
    return q[ifreq] if isinstance(q, (list, tuple)) else q


def _expandColumns(op, q, ifreq, c0, c1, R):
    "R ([c1 - c0][rows]) = columns c0 .. c1-1 of the frequency's sparse column matrix, expanded on the item's GPU: only the entries cross PCIe"
    op.rhsFromSparseDevice(sp.csc_matrix(_ofFrequency(q, ifreq))[:, c0:c1], R.data_ptr())


def _prepareBackSources(sv, qb, freqs):
    "calling-thread half of `_backSources`: the survey's adjoint plans of a moving array (the survey caches them; a fixed array brings its qb)"
    if qb is None:
        for ifreq in freqs:
            sv.adjointPlan(ifreq)


def _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, d_R, rows):
    """d_R ([k][rows], k = c1 - c0) = the back-sources R_s^T resid[:, s, ifreq] of the sources c0 .. c1-1.  qb given (fixed array): the host-built
    sparse matrix as triplets.  qb None (the array moves with the source): the gather of the survey's adjoint plan from the item's residual samples
    resid[:, c0:c1, ifreq] -- 16 nrec k bytes up instead of ~81 entries of 28 B per sample, and no sparse products on the host.  resid a `DevicePanels`
    (the adjoint source of a misfit, made on the device): the item's panel is used where it lies, nothing goes up; qb is None then, for a fixed array too --
    the adjoint plan is built from the stacked receivers, which serve both modes."""
    if isinstance(resid, DevicePanels):
        plan = _planOnDevice(ws, sv, ifreq)
        panel = resid.panel(ifreq, c0, c1)
        _lib.wait_torch_stream(ws.device)
        op.rhsFromSamplesDevice(panel.data_ptr(), c1 - c0, plan, c0, c1, d_R, rows=rows)
        return
    if qb is not None:
        op.rhsFromSparseDevice(_muxTriplets((qb[ifreq],), c0, c1, rows), d_R)
        return
    plan = _planOnDevice(ws, sv, ifreq)
    panel = _lib.to_device(resid[:, c0:c1, ifreq], ws.device, np.complex128)       # (nrec, k), one contiguous panel
    _lib.wait_torch_stream(ws.device)
    op.rhsFromSamplesDevice(panel.data_ptr(), c1 - c0, plan, c0, c1, d_R, rows=rows)


def _inverseCube(c, dev):
    '1 / c^3 on `dev` from one upload of the model array c'
    cd = _lib.to_device(np.asarray(c).ravel(), dev, np.complex128)
    return 1.0 / (cd * cd * cd)


def _cachedInverseCube(ws, cm):
    "1 / c^3 of the model array cm, made once per worker (the id stays this array's while the entry lives: it keeps the array)"
    return ws.cached(('inv_c3', id(cm)), lambda: _inverseCube(cm, ws.device), keep=cm)


def _cachedInverseC3Rho(ws, op):
    """1 / (c^3 rho) of the operator's model, made once per worker: the cached 1 / c^3 and one upload of rho -- the per-cell factor of
    d K / d c = -2 omega_d^2 / (c^3 rho), what linearisation='operator' weighs with"""
    cm, rho = op.c, op.rho
    inv = _cachedInverseCube(ws, cm)
    return ws.cached(('inv_c3_rho', id(cm), id(rho)), lambda: inv / _lib.to_device(np.asarray(rho, dtype=np.float64).ravel(), ws.device, np.float64), keep=(cm, rho))


def _partial(ws, name, shape, dtype):
    "the worker's partial result ws.<name> ('G': gradient -- 2 N entries, [c; b], for parameter='joint' --, 'Gb': its buoyancy part, 'H': illumination), zeroed on first use"
    import torch
    if getattr(ws, name) is None:
        setattr(ws, name, torch.zeros(shape, dtype=dtype, device=ws.device))
    return getattr(ws, name)


def _checkItemsFit(items, held, work):
    """MemoryError unless every GPU has room for what its items leave there, the sum of held(op, c0, c1) bytes, beside the largest working set
    work(op, c0, c1) of an item there"""
    import torch
    from .fieldstore import check_fits
    need, peak = {}, {}
    for _, op, _, c0, c1 in items:
        need[op.device] = need.get(op.device, 0) + held(op, c0, c1)
        peak[op.device] = max(peak.get(op.device, 0), work(op, c0, c1))
    check_fits({d: need[d] + peak[d] for d in need}, {d: torch.cuda.mem_get_info(d)[0] for d in need})


# ---- the two ways an item's imaging sum reaches G ----------------------------------------------------------------------------------------------
# An adding step is called once per item, before the solve, and returns (scaler, target, finish): the item's imaging kernel accumulates
# scaler (.) sum_s uF (.) uB into `target`, then finish() runs (None: nothing left to do).  A step may enqueue torch work for what it returns; it
# does not wait for it -- the item body issues the one wait_torch_stream between the step and the solve.

def _addOnNativeGrid(prob, scale):
    """The wavefields are on the gradient's grid: the imaging kernel goes straight into G with the scaler -(omega^2 / c^3) scale^2, one kernel per item."""
    sv = prob.survey
    plain_scaler = prob._plainGradientScaler()

    def step(ws, op, ifreq, Ni):
        dev = ws.device
        if plain_scaler:
            # -(omega^2 / c^3) scale^2 on the GPU from one upload of the model per worker: on the host the complex power and division of problem.py:74-81 cost
            # 6 ms per frequency at 512^2 (numpy), in the thread whose only other job is to keep the solve stream fed
            omega = 2 * np.pi * sv.freqs[ifreq]
            scaler = _cachedInverseCube(ws, op.c) * complex(-(omega ** 2) * scale * scale)
        else:
            scaler = _lib.to_device(prob.gradientScaler(ifreq) * scale * scale, dev, np.complex128)
        return scaler, ws.G, None
    return step


def _addOperator(prob, scale):
    """linearisation='operator' on the gradient's grid: the adding step hands out W = 2 scale conj(omega_d^2 / premul) / (conj(c)^3 rho), the weight of
    k_imaging_op (G += W (.) sum_s U_s (.) M0(mask_int (.) uB_s), U_s and uB_s the unscaled solves: the scaleTerm enters once)"""
    import torch
    from .frechet import dampedOmega

    def step(ws, op, ifreq, Ni):
        om = dampedOmega(op)
        return torch.conj(_cachedInverseC3Rho(ws, op)).resolve_conj() * complex(2.0 * scale * np.conj(om * om / complex(op.premul))), ws.G, None
    return step


def _addUpscaled(prob, scale):
    """Every frequency on its own grid (a multiscale survey): the imaging sum P = scale^2 sum_s uF (.) uB is accumulated there, then
    G += pp(scaler) (.) pp(P) in one grid transfer (problem.py:152: the product of two up-scaled fields), the up-scaled scaler -(omega^2 / c^3)
    made once per worker and frequency from the operator's coarse c."""
    import torch
    sv, N = prob.survey, prob.nrow
    pps = sv.postProcessors

    def step(ws, op, ifreq, Ni):
        dev = ws.device
        P, unit = ws.buffer('P', Ni), ws.buffer('unit', Ni)

        def upscaled_scaler():
            omega = 2 * np.pi * sv.freqs[ifreq]
            sc = _inverseCube(op.c, dev) * complex(-(omega ** 2))
            S = torch.empty(N, dtype=torch.complex128, device=dev)
            _lib.wait_torch_stream(dev)
            pps[ifreq].apply_device(sc, S, k=1)
            return S
        S = ws.cached(('scaler', ifreq), upscaled_scaler)
        P.zero_()
        unit.fill_(scale * scale)
        G = ws.G
        return unit, P, lambda: pps[ifreq].apply_device(P, G, k=1, op=op, beta=1., mul=S)
    return step


# ---- the pipelines -----------------------------------------------------------------------------------------------------------------------------
def gradient(prob, qb, owned, resid):
    """Mux branch of Jtvec with the wavefields kept in HBM: per work item (frequency, source batch) [qf | qb] of its sources is made on the item's GPU
    and solved there on the frequency's own grid, and scaler * sum_s uF (.) uB is added to that GPU's partial gradient.  The partial gradients are
    summed on the host, then ONE all-reduce over ranks when the frequencies are sharded.  qb None: the back-sources of a moving receiver array,
    made on the device from `resid` (nrec, nsrc, nfreq)."""
    import torch
    from .survey import HelmMultiGridSurvey
    sv = prob.survey
    nsrc, N = sv.nsrc, prob.nrow
    scale = complex(prob.system.scaleTerm)
    qf = sv.getSources()
    if not owned:
        return _sumPartials(prob, [])
    _prepareBackSources(sv, qb, owned)
    devs, items = deviceItems(prob.system, owned, nsrc)
    add = _addUpscaled(prob, scale) if isinstance(sv, HelmMultiGridSurvey) else _addOnNativeGrid(prob, scale)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        _partial(ws, 'G', N, torch.complex128)
        U, R = ws.buffer('U', 2 * k * Ni), ws.buffer('R', 2 * k * Ni)
        # [qf | qb] of the item's sources: sparse triplets (or residual samples) up, dense on the device
        _fillMuxDevice(ws, sv, op, _ofFrequency(qf, ifreq), qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        scaler, target, finish = add(ws, op, ifreq, Ni)
        _lib.wait_torch_stream(ws.device)                # (covers the torch work the adding step has just enqueued -- scaler product, zero_(), fill_(): keep it between the two)
        op.solveDevice(R.data_ptr(), U.data_ptr(), 2 * k, Ni)
        op.imagingAccumulateDevice(U.data_ptr(), U.data_ptr() + k * Ni * 16, k, scaler.data_ptr(), target.data_ptr())
        if finish is not None:
            finish()
    return _sumPartials(prob, [ws.G for ws in runOnDevices(devs, items, one) if ws.G is not None])


def _sumPartials(prob, parts, n=None):
    """the gradient from the workers' partial gradients: summed on the host, then ONE all-reduce over ranks when the frequencies are sharded (no partial:
    a rank that owns no frequency brings zeros to that all-reduce).  n: the length of a partial where it is not the grid's (2 N: the stacked [c; b] of
    parameter='joint')"""
    import torch
    N = prob.nrow if n is None else int(n)
    if len(parts) == 1:
        G = parts[0]
        if prob._sharded:
            parallel.allreduce_sum_device(G)
        torch.cuda.synchronize(G.device)
        return _lib.from_device(G)
    g = np.zeros(N, dtype=np.complex128)
    for G in parts:                                   # per-GPU partial gradients: 16 B per grid point each
        torch.cuda.synchronize(G.device)
        g += _lib.from_device(G)
    return parallel.allreduce_sum(g) if prob._sharded else g


def _receiverMatrices(sv, owned):
    """{grid key: receiver CSR} for the owned frequencies (None: the one grid of a single-grid survey): the survey's stacked matrices for an array that
    moves with the source, the one matrix of a fixed array.  Made on the calling thread (the survey caches them)."""
    Rms = {}
    for ifreq in owned:
        gk = sv._gridKey(ifreq)
        if gk not in Rms:
            if sv.mode != 'fixed':
                Rm = sv.stackedReceivers(ifreq)
            else:
                Rm = sp.csr_matrix(sv.rVec(0, ifreq))
                Rm.sum_duplicates()
            Rms[gk] = Rm
    return Rms


def _csrOnDevice(ws, Rm, gk, nrec, stride, c0):
    """the receiver CSR as sampleDevice / sampleSumDevice take it, (rowptr, col, val, nrec[, stride]): uploaded once per worker and grid key; with a row
    stride (a moving array) the rows of the batch's sources start at c0 * nrec"""
    dev = ws.device
    csr = ws.cached(('csr', gk), lambda: (_lib.to_device(Rm.indptr, dev, np.int64), _lib.to_device(Rm.indices, dev, np.int64),
                                     _lib.to_device(Rm.data, dev, np.complex128), nrec))
    if stride:
        csr = (csr[0][c0 * nrec:], csr[1], csr[2], nrec, stride)
    return csr


def _sampling(prob, freqs, scale, conj=False):
    """What the three routes that end in receiver samples share: (data, stage, sample).  `data` is the (nrec, nsrc, nfreq) result, zeros; the receiver
    matrices of the frequencies `freqs` are made here, on the calling thread (conj: their conjugates, for Born data).  One receiver CSR per grid key
    (None: the one grid of a single-grid survey).  A receiver array that moves with the source is sampled through the survey's stacked CSR, source s from
    its own rows s * nrec .. (row stride nrec); a fixed one through the one matrix (stride 0).

    stage(ws, ifreq, c0, c1) -> (csr, out): the item's torch work, the CSR on the worker's GPU (uploaded once per worker and grid key) and the (nrec, k)
    buffer the samples go to.  It comes BEFORE the item's wait_torch_stream, which is why sampling is handed out in two halves.
    sample(op, ifreq, c0, c1, staged, d_u, d_exp): sampleDevice of the k wavefields at d_u (d_exp: the column exponents of a complex64 store, or None)
    and data[:, c0:c1, ifreq] = scale * samples.  d_u None: the item has put its samples into `out` itself (the 2.5-D sum of dpred)."""
    sv = prob.survey
    nrec = sv.nrec
    data = np.zeros((nrec, sv.nsrc, sv.nfreq), dtype=np.complex128)
    stride = nrec if sv.mode != 'fixed' else 0
    Rms = _receiverMatrices(sv, freqs)
    if conj:
        Rms = {gk: Rm.conj() for gk, Rm in Rms.items()}

    def stage(ws, ifreq, c0, c1):
        gk = sv._gridKey(ifreq)
        return _csrOnDevice(ws, Rms[gk], ('conj', gk) if conj else gk, nrec, stride, c0), ws.buffer('out', (nrec, c1 - c0))

    def sample(op, ifreq, c0, c1, staged, d_u, d_exp=None):
        csr, out = staged
        if d_u is not None:
            op.sampleDevice(d_u, c1 - c0, csr, out.data_ptr(), d_exp=d_exp)      # (returns when the samples are there: helm_sample_device waits for its own stream)
        data[:, c0:c1, ifreq] = scale * _lib.from_device(out)          # (disjoint slices per item: no two workers write the same entries)
    return data, stage, sample


def dpred(prob, owned):
    """Predicted data (nrec, nsrc, nfreq) with the wavefields kept in HBM: per work item (frequency, source batch) the sparse sources are expanded on the
    item's GPU and solved there on the frequency's own grid, and only the receiver samples R u (nrec x sources) come back."""
    sv = prob.survey
    data, stage, sample = _sampling(prob, owned, complex(prob.system.scaleTerm))
    if not owned:
        return data
    qf = sv.getSources()
    devs, items = deviceItems(prob.system, owned, sv.nsrc)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        staged = stage(ws, ifreq, c0, c1)
        R = ws.buffer('R', k * Ni)
        _expandColumns(op, qf, ifreq, c0, c1, R)         # (its own wait covers what `stage` has enqueued)
        if hasattr(op, 'sampleSumDevice'):               # a composite (2.5-D ky sum): its samples are accumulated per ky, it keeps its own wavefield scratch
            op.sampleSumDevice(R.data_ptr(), k, staged[0], staged[1].data_ptr(), rows=Ni)      # (sampling is linear: the N x k sum over ky is never formed)
            d_u = None
        else:
            U = ws.buffer('U', k * Ni)
            op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
            d_u = U.data_ptr()
        sample(op, ifreq, c0, c1, staged, d_u)
    runOnDevices(devs, items, one)
    return data


# ---- forward fields kept between calls (fieldstore.DeviceFields) ------------------------------------------------------------------------------
# `fields` solves the forward wavefields once into a store that outlives the call; `dpredFromFields` and `gradientFromFields` are dpred and the
# u-given branch of Jtvec over the store's OWN items (not a fresh deal), so that every item finds its slice on the GPU it was solved on.

def _storedItems(sysw, F):
    "(devs, items) as runOnDevices takes them from the items a store recorded: the frequency's own operator for its first batch, the system's replica j for batch j"
    batch, items = {}, []
    for w, dev, ifreq, c0, c1 in F.items:
        j = batch.get(ifreq, 0)
        batch[ifreq] = j + 1
        op = sysw.subProblems[ifreq] if j == 0 else sysw._replica(ifreq, j, dev)
        items.append((w, op, ifreq, c0, c1))
    return _workerDevices(sysw), items


def fields(prob, owned, dtype='complex128', perKy=False):
    """The forward wavefields of the owned frequencies solved into a DeviceFields: per work item the sparse sources are expanded on the item's GPU and
    solved straight into the item's slice of the store (complex128), or into the workspace and packed into it (complex64).  Nothing comes down.
    perKy (the operators are 2.5-D composites): the slice of an item is (nky, k, Ni) and every ky operator solves into its own block, in the order and with the
    factor scheduling of the composite's ky loop (complex64: packed block by block, one exponent per column and ky); the ky sum is not formed."""
    import torch
    from .fieldstore import DeviceFields, DTYPES
    from .survey import HelmMultiGridSurvey
    sv = prob.survey
    if isinstance(sv, HelmMultiGridSurvey) and not prob._multiscaleServed():          # (with multiscaleDerivatives every frequency's slice lives on ITS grid: Ni = op.nrow)
        raise NotImplementedError('fieldsDevice serves single-grid surveys: on a multiscale survey the u-given branch of Jtvec multiplies the native-grid forward '
                                  'field by the up-scaled back-propagated one per source (two grid transfers per source), which has not been built on the device')
    if dtype not in DTYPES:
        raise ValueError('fieldsDtype is %r: one of %s' % (dtype, ', '.join(DTYPES)))
    nsrc = sv.nsrc
    scale = complex(prob.system.scaleTerm)
    stamp = prob._modelStamp
    nky, kyCoef = None, None
    if perKy:
        comp = prob.system.subProblems[0]
        nky = len(comp.subProblems)
        kyCoef = [comp._kyCoefficients(ky) for ky in range(nky)]
    if not owned:
        return DeviceFields(sv.nfreq, nsrc, [], [], None if dtype == 'complex128' else [], stamp, scale, dtype, nky=nky, kyCoef=kyCoef)
    qf = sv.getSources()
    devs, items = deviceItems(prob.system, owned, nsrc)
    packed = dtype == 'complex64'
    esize = 8 if packed else 16
    blocks = nky if perKy else 1
    # what every GPU has to hold: its slices (and exponents), nky blocks of them in a per-ky store, and the largest working set of an item there (R; U as well
    # when the store is packed)
    _checkItemsFit(items, held=lambda op, c0, c1: blocks * (c1 - c0) * (int(op.nrow) * esize + (4 if packed else 0)),
                   work=lambda op, c0, c1: (c1 - c0) * int(op.nrow) * 16 * (2 if packed else 1))
    tdtype = torch.complex64 if packed else torch.complex128
    lead = (nky,) if perKy else ()
    slices = [torch.empty(lead + (c1 - c0, int(op.nrow)), dtype=tdtype, device=torch.device('cuda', op.device)) for _, op, _, c0, c1 in items]
    exps = [torch.empty(lead + (c1 - c0,), dtype=torch.int32, device=sl.device) for sl, (_, _, _, c0, c1) in zip(slices, items)] if packed else None
    F = DeviceFields(sv.nfreq, nsrc, [(w, op.device, ifreq, c0, c1) for w, op, ifreq, c0, c1 in items], slices, exps, stamp, scale, dtype, nky=nky, kyCoef=kyCoef)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        sl, ex = F.slice(ifreq, c0)
        R = ws.buffer('R', k * Ni)
        _expandColumns(op, qf, ifreq, c0, c1, R)
        U = ws.buffer('U', k * Ni) if packed and perKy else None
        _lib.wait_torch_stream(ws.device)
        if perKy:
            def each(ky, sub):
                d_u, d_exp = F.pointers(ifreq, c0, ky)
                if not packed:
                    sub.solveDevice(R.data_ptr(), d_u, k, Ni)
                else:
                    sub.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
                    sub.packDevice(U.data_ptr(), k, d_u, d_exp, rows=Ni)
            op._kyLoop(each)
        elif not packed:
            op.solveDevice(R.data_ptr(), sl.data_ptr(), k, Ni)           # (no copy: the solve's output IS the slice)
        else:
            U = ws.buffer('U', k * Ni)
            op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
            op.packDevice(U.data_ptr(), k, sl.data_ptr(), ex.data_ptr(), rows=Ni)      # (returns when the slice and its exponents are complete)
    try:
        runOnDevices(devs, items, one)
    except BaseException:
        F.release()
        raise
    return F


def dpredFromFields(prob, F):
    """Predicted data (nrec, nsrc, nfreq) from forward fields already in HBM: no solve, every item samples its slice of the store (row stride 0 for a fixed
    array, nrec for one that moves with the source) and only the receiver samples come back."""
    F.checkCurrent(prob, perKy=None)
    data, stage, sample = _sampling(prob, F.ownedFreqs, F.scale)
    if not F.items:
        return data
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        staged = stage(ws, ifreq, c0, c1)
        _lib.wait_torch_stream(ws.device)
        if F.nky is not None:
            # a per-ky store: the samples of every block accumulated with the composite's coefficients -- sampling is linear, the summed field is never formed
            sub = op._liveSub()
            for ky, (a, b) in enumerate(F.kyCoef):
                _sampleAccumulate(sub, *F.pointers(ifreq, c0, ky), c1 - c0, int(op.nrow), staged[0], staged[1], a, b)
            if op.kyRelease:
                del sub.factors
            sample(op, ifreq, c0, c1, staged, None)
            return
        sample(op, ifreq, c0, c1, staged, *F.pointers(ifreq, c0))
    runOnDevices(devs, items, one, factor=False)
    return data


def _sampleAccumulate(sub, d_u, d_exp, k, rows, csr, out, alpha, beta):
    """out (nrec, k) = alpha R u + beta out for the k columns at d_u (d_exp: the exponents of a complex64 block, or None), csr as `_csrOnDevice` made it; beta 0:
    `out` need not be initialised.  Returns when the samples are there."""
    import ctypes
    lib = _lib.load()
    rowptr, col, val, nrec = csr[:4]
    stride = int(csr[4]) if len(csr) > 4 else 0
    a, b = complex(alpha), complex(beta)
    tail = (int(k), int(rows), ctypes.c_void_p(rowptr.data_ptr()), ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr()), int(nrec), stride,
            a.real, a.imag, b.real, b.imag, ctypes.c_void_p(out.data_ptr()))
    if d_exp is not None:
        _lib.check(lib.helm_sample_rows_c64_device(sub.handle, ctypes.c_void_p(d_u), ctypes.c_void_p(d_exp), *tail), sub.handle)
    else:
        _lib.check(lib.helm_sample_rows_device(sub.handle, ctypes.c_void_p(d_u), *tail), sub.handle)


def _factorBytes(op):
    """What the direct factors of one 2-D operator of op's grid take in device memory, from the elimination-tree plan (host only): per front the inverse of
    its s x s pivot block and the two s x m coupling blocks, 16 B per entry.  A 2.5-D composite keeps one set per ky; one that releases its ky operators as it
    goes (kyRelease) holds two groups of its ky loop at the most, the one being solved and the one prefactored ahead (minizephyr.ky_schedule)."""
    import ctypes
    lib = _lib.load()
    nz, nx, leaf = int(op.nz), int(op.nx), int(_lib.tuning().nd_leaf)
    n = lib.helm_direct_plan(nz, nx, leaf, None, 0)
    if n <= 0:
        return 0
    plan = np.zeros((n, 12), dtype=np.int32)
    if lib.helm_direct_plan(nz, nx, leaf, plan.ctypes.data_as(ctypes.c_void_p), n) != n:
        return 0
    sm = plan[:, 6].astype(np.int64), plan[:, 7].astype(np.int64)
    one = int(16 * np.sum(sm[0] * (sm[0] + 2 * sm[1])))
    subs = getattr(op, 'subProblems', None)
    if subs is None:
        return one
    from .minizephyr import KY_GROUP
    return one * (min(len(subs), 2 * KY_GROUP) if getattr(op, 'kyRelease', False) else len(subs))


def _checkSecondFactorsFit(items, planes=0, cols=None, blocks=2, beside=None):
    """MemoryError unless every GPU has room for what a pass through the TRANSPOSED operators adds to a resident forward pass: their factors -- the factors of
    A and of A^T are held side by side -- and the item's U and R (planes: and that many model-sized complex128 planes, the lag products of parameter='rho';
    cols: the columns solved per item where they are not the item's own, the receiver columns of kind='gaussNewton'; blocks: the column blocks of an item where
    they are more than U and R, the four of `newtonFromFields`; beside: {(ifreq, c0): the forward operator an item solves with as well} where the forward
    factors may not be resident either -- u=None of the 2.5-D routes, which walks A_ky and A_ky^T together: 2 nky factor sets per frequency, two groups of each
    with kyRelease)"""
    seen = set()

    def unmade(op):
        'the factors an operator has yet to make, counted with its first item'
        first = id(op) not in seen
        seen.add(id(op))
        return _factorBytes(op) if first and not op.factors and str(getattr(op, 'method', 'auto')).lower() in ('auto', 'direct') else 0
    partner = {} if beside is None else {id(op): beside[(ifreq, c0)] for _, op, ifreq, c0, _ in items}

    def factors(op, c0, c1):
        other = partner.get(id(op))
        return unmade(op) + (unmade(other) if other is not None else 0)
    _checkItemsFit(items, held=factors, work=lambda op, c0, c1: (blocks * (c1 - c0 if cols is None else cols) + planes) * int(op.nrow) * 16)


def gradientFromFields(prob, F, qb, resid, system=None, linearisation='scaler', parameter='c', chain=None):
    """The u-given branch of Jtvec (problem.py:154-162) with the forward fields read from the store: per item only the k back-sources are made and solved
    (nsrc columns per frequency, not 2 nsrc), scaler * sum_s uF (.) uB goes into the GPU's partial gradient, and the real part of the sum is returned.
    qb None: the back-sources of a moving receiver array, made on the device from `resid` (nrec, nsrc, nfreq).  system: the wrapper whose operators
    back-propagate (default prob.system; prob.adjointSystem for Jtvec(adjoint='transpose') -- the same devices and replicas, so every item still finds
    its slice on its own GPU).  linearisation='operator' (with the transposed system, qb / resid those of R_s^H r): the same items, calls and waits with the
    weight of `_addOperator` and k_imaging_op, the mass stencil on the back-propagated columns fused into the imaging sum.  parameter='rho': the gradient
    with respect to the BUOYANCY, `_gradientPlanesFromFields` (the caller applies d b / d rho).  linearisation='full': the same pipeline with the transpose
    of the velocity planes; chain (N,) float64, d b / d c where the density follows c, or None."""
    import torch
    if parameter == 'rho':
        return _gradientPlanesFromFields(prob, F, qb, resid, system)
    if linearisation == 'full':
        return _gradientPlanesFromFields(prob, F, qb, resid, system, velocity=True, chain=chain)
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    scale = F.scale
    if not F.items:
        return _sumPartials(prob, []).real
    _prepareBackSources(sv, qb, F.ownedFreqs)
    devs, items = _storedItems(prob.system if system is None else system, F)
    if system is not None:
        _checkSecondFactorsFit(items)
    exact = linearisation == 'operator'
    add = _addOperator(prob, scale) if exact else _addOnNativeGrid(prob, scale)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        d_uF, d_exp = F.pointers(ifreq, c0)
        _partial(ws, 'G', N, torch.complex128)
        U, R = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
        _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        scaler, target, finish = add(ws, op, ifreq, Ni)
        _lib.wait_torch_stream(ws.device)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        if exact:
            op.imagingOpAccumulateDevice(d_uF, U.data_ptr(), k, scaler.data_ptr(), target.data_ptr(), d_exp=d_exp, rows=Ni)
        else:
            op.imagingAccumulateDevice(d_uF, U.data_ptr(), k, scaler.data_ptr(), target.data_ptr(), d_exp=d_exp)
        if finish is not None:
            finish()
    return _sumPartials(prob, [ws.G for ws in runOnDevices(devs, items, one) if ws.G is not None]).real


def bornFromFields(prob, F, v, linearisation='scaler', parameter='c', db=None):
    """prob.JvecBorn(u=F): Born data (nrec, nsrc, nfreq) of the model perturbation v (N,) from forward fields already in HBM.  Per stored item
    W = v (.) gradientScaler(f) scaleTerm is made on the item's GPU (v and the model go up once per worker), the virtual-source kernel writes
    conj(W (.) slice) -- the store holds the unscaled solves, hence the scaleTerm in W -- the forward operator solves the k columns, and the samples
    through the CONJUGATED receiver CSR (row stride 0 for a fixed array, nrec for one that moves with the source) come down: nrec x k values per item.
    linearisation='operator': `_bornOperatorFromFields`; with parameter='rho' (v the BUOYANCY perturbation -v_rho / rho^2): `_bornPlanesFromFields`.
    linearisation='full': the same pipeline with the velocity planes of v; db (N,) float64 the buoyancy perturbation that goes with v where the density follows
    c, or None.  parameter='joint': v the velocity half and db = -v_rho / rho^2 the buoyancy half of a stacked [c; rho] perturbation -- one set of planes
    V[v] + L[db] and one solve ('operator': the mass term of V alone)."""
    if parameter == 'joint':
        return _bornPlanesFromFields(prob, F, db, dc=v, stretch=linearisation == 'full')
    if parameter == 'rho':
        return _bornPlanesFromFields(prob, F, v)
    if linearisation == 'full':
        return _bornPlanesFromFields(prob, F, db, dc=v)
    if linearisation == 'operator':
        return _bornOperatorFromFields(prob, F, v)
    F.checkCurrent(prob)
    sv = prob.survey
    scale = F.scale
    data, stage, sample = _sampling(prob, F.ownedFreqs, scale, conj=True)
    if not F.items:
        return data
    plain_scaler = prob._plainGradientScaler()
    v = np.ascontiguousarray(v, dtype=np.complex128)
    host_w = None if plain_scaler else {ifreq: v * np.asarray(prob.gradientScaler(ifreq)).ravel() * scale for ifreq in F.ownedFreqs}
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        d_uF, d_exp = F.pointers(ifreq, c0)
        staged = stage(ws, ifreq, c0, c1)
        if plain_scaler:
            inv = _cachedInverseCube(ws, op.c)
            vd = ws.cached(('born_v', id(v)), lambda: _lib.to_device(v, dev, np.complex128), keep=v)
            omega = 2 * np.pi * sv.freqs[ifreq]
            W = inv * vd * complex(-(omega ** 2) * scale)
        else:
            W = ws.cached(('born_w', ifreq, id(v)), lambda: _lib.to_device(host_w[ifreq], dev, np.complex128), keep=v)
        U, R = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
        _lib.wait_torch_stream(dev)
        op.virtualSourcesDevice(d_uF, k, W.data_ptr(), R.data_ptr(), d_exp=d_exp, rows=Ni)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        sample(op, ifreq, c0, c1, staged, U.data_ptr())
    runOnDevices(devs, items, one)
    return data


def _bornOperatorFromFields(prob, F, v):
    """prob.JvecBorn(u=F, linearisation='operator'): the derivative of dpred along v.  The items, calls and waits of `bornFromFields` with
    W = dK = -2 omega_d^2 v / (c^3 rho) (the cached 1 / c^3, one upload of rho and of v per worker), k_virtual_sources_op in the place of
    k_virtual_sources -- R = -(1 / premul) mask_int (.) M0(W (.) conj(slice)), the slice being conj(u^) unscaled -- and the receiver CSR as it is, not
    conjugated; the scaleTerm multiplies the samples."""
    from .frechet import dampedOmega
    F.checkCurrent(prob)
    data, stage, sample = _sampling(prob, F.ownedFreqs, F.scale)
    if not F.items:
        return data
    v = np.ascontiguousarray(v, dtype=np.complex128)
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        d_uF, d_exp = F.pointers(ifreq, c0)
        staged = stage(ws, ifreq, c0, c1)
        vd = ws.cached(('born_v', id(v)), lambda: _lib.to_device(v, dev, np.complex128), keep=v)
        om = dampedOmega(op)
        W = _cachedInverseC3Rho(ws, op) * vd * complex(-2.0 * om * om)
        U, R = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
        _lib.wait_torch_stream(dev)
        op.virtualSourcesOpDevice(d_uF, k, W.data_ptr(), -1.0 / complex(op.premul), R.data_ptr(), conj=True, d_exp=d_exp, rows=Ni)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        sample(op, ifreq, c0, c1, staged, U.data_ptr())
    runOnDevices(devs, items, one)
    return data


def _jointPlanes(ws, fop, dcd, dbd, C, stretch, spare):
    """C = V[dc] + L[db] of the forward operator `fop`, the planes of a stacked [c; rho] perturbation: one call of k_velocity_planes; stretch False
    ('operator'): k_mass_planes into C, k_buoyancy_planes into `spare` (nine planes the caller has no other use for yet) and their sum by torch, followed by the
    hand-over to the library's stream"""
    if stretch:
        fop.velocityPlanesDevice(dcd.data_ptr(), dbd.data_ptr(), C.data_ptr())
        return
    fop.massPlanesDevice(dcd.data_ptr(), C.data_ptr())
    if dbd is None:          # (the mass term alone: 'operator' along a velocity perturbation on a multiscale pairing)
        return
    fop.buoyancyPlanesDevice(dbd.data_ptr(), spare.data_ptr())
    C.add_(spare)
    _lib.wait_torch_stream(ws.device)


def _bornPlanesFromFields(prob, F, db, dc=None, stretch=True):
    """prob.JvecBorn(u=F, linearisation='operator', parameter='rho'): the derivative of dpred along the buoyancy perturbation db (N,) float64.  The items,
    calls and waits of `_bornOperatorFromFields` with the virtual-source step in two calls: k_buoyancy_planes makes the nine planes L_f[db] of the item's
    frequency in the workspace (db goes up once per worker), k_stencil_sources writes R = -(1 / premul) sum_k L_f[db]_k (.) shift_k(conj(slice)).
    dc given (N,) float64: prob.JvecBorn(u=F, linearisation='full'), the total derivative along the velocity perturbation dc -- the same body with
    k_velocity_planes in the place of k_buoyancy_planes: the planes V_f[dc] of the mass term and the PML stretch, plus L_f[db] where the density follows c
    (db = (d b / d c) dc then; None with an explicit density).  stretch False (parameter='joint' with linearisation='operator', dc and db both given): the
    mass term of V[dc] alone plus L[db], `_jointPlanes`.
    A multiscale pairing hands db / dc as {ifreq: array on the grid of that frequency} (one array object per grid, so a worker uploads it once per grid)."""
    F.checkCurrent(prob)
    data, stage, sample = _sampling(prob, F.ownedFreqs, F.scale)
    if not F.items:
        return data
    perGrid = isinstance(db, dict) or isinstance(dc, dict)
    if not perGrid:
        db = None if db is None else np.ascontiguousarray(db, dtype=np.float64)
        dc = None if dc is None else np.ascontiguousarray(dc, dtype=np.float64)
    allDb, allDc = db, dc
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        db, dc = (None if x is None else x[ifreq] for x in (allDb, allDc)) if perGrid else (allDb, allDc)
        d_uF, d_exp = F.pointers(ifreq, c0)
        staged = stage(ws, ifreq, c0, c1)
        dbd = None if db is None else ws.cached(('born_db', id(db)), lambda: _lib.to_device(db, dev, np.float64), keep=db)
        dcd = None if dc is None else ws.cached(('born_dc', id(dc)), lambda: _lib.to_device(dc, dev, np.float64), keep=dc)
        U, R, C = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('planes', 9 * Ni)
        spare = None if stretch else ws.buffer('lags', 9 * Ni)
        _lib.wait_torch_stream(dev)
        if not stretch:
            _jointPlanes(ws, op, dcd, dbd, C, False, spare)
        elif dcd is None:
            op.buoyancyPlanesDevice(dbd.data_ptr(), C.data_ptr())
        else:
            op.velocityPlanesDevice(dcd.data_ptr(), None if dbd is None else dbd.data_ptr(), C.data_ptr())
        op.stencilSourcesDevice(d_uF, k, C.data_ptr(), -1.0 / complex(op.premul), R.data_ptr(), conj=True, d_exp=d_exp, rows=Ni)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        sample(op, ifreq, c0, c1, staged, U.data_ptr())
    runOnDevices(devs, items, one)
    return data


def _gradientPlanesFromFields(prob, F, qb, resid, system, velocity=False, chain=None):
    """prob.Jtvec(u=F, adjoint='transpose', linearisation='operator', parameter='rho') up to d b / d rho: the gradient with respect to the buoyancy, float64
    (N,).  The items and shared steps of `gradientFromFields` (qb / resid those of R_s^H r, `system` the transposed operators) with the imaging step in two
    calls: k_lag_imaging adds P_k = sum_s uB_s (.) shift_k(slice_s) of the item's columns to nine planes of the workspace, zeroed per item, and
    k_buoyancy_adjoint adds -(scaleTerm / conj(premul)) conj(L_f)^T P to the worker's partial G -- the slice and the solves are the conjugates of u^ and z,
    so the coefficients of L are conjugated, not the fields, and the real part is taken at the end.
    velocity: prob.Jtvec(u=F, adjoint='transpose', linearisation='full'), the gradient with respect to the velocity -- the same body with k_velocity_adjoint
    (conj(V_f)^T P) in the place of k_buoyancy_adjoint.  chain (N,) float64 (the density follows c): k_buoyancy_adjoint as well, into a second partial Gb,
    which the real d b / d c multiplies once, after the sum over frequencies and workers."""
    import torch
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    scale = F.scale
    gardner = velocity and chain is not None
    if not F.items:
        g = _sumPartials(prob, []).real
        return g + chain * _sumPartials(prob, []).real if gardner else g
    _prepareBackSources(sv, qb, F.ownedFreqs)
    devs, items = _storedItems(prob.system if system is None else system, F)
    _checkSecondFactorsFit(items, planes=9)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        d_uF, d_exp = F.pointers(ifreq, c0)
        G = _partial(ws, 'G', N, torch.complex128)
        Gb = _partial(ws, 'Gb', N, torch.complex128) if gardner else None
        U, R, P = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('lags', 9 * Ni)
        _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        P.zero_()
        _lib.wait_torch_stream(ws.device)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        op.lagImagingAccumulateDevice(d_uF, U.data_ptr(), k, P.data_ptr(), d_exp=d_exp, rows=Ni)
        w = -scale / np.conj(complex(op.premul))
        if not velocity:
            op.buoyancyAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
        else:
            op.velocityAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
            if gardner:
                op.buoyancyAdjointDevice(P.data_ptr(), w, Gb.data_ptr(), conj=True)
    wss = runOnDevices(devs, items, one)
    g = _sumPartials(prob, [ws.G for ws in wss if ws.G is not None]).real
    return g + chain * _sumPartials(prob, [ws.Gb for ws in wss if ws.Gb is not None]).real if gardner else g


def jointGradientFromFields(prob, F, qb, resid, system, linearisation):
    """prob.Jtvec(u=F, adjoint='transpose', parameter='joint') up to d b / d rho on the second half: [g_c; g_b], float64 (2 N,), from ONE back-propagation per
    stored item.  The item body of `_gradientPlanesFromFields` with both transposes applied to the same lag products P0: k_velocity_adjoint (the mass-only one
    for linearisation='operator') into the first half of the worker's partial G (2 N complex128), k_buoyancy_adjoint into the second.  One all-reduce of the
    stacked vector where the frequencies are sharded."""
    import torch
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    scale = F.scale
    stretch = linearisation == 'full'
    if not F.items:
        return _sumPartials(prob, [], n=2 * N).real
    _prepareBackSources(sv, qb, F.ownedFreqs)
    devs, items = _storedItems(system, F)
    _checkSecondFactorsFit(items, planes=9)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        d_uF, d_exp = F.pointers(ifreq, c0)
        G = _partial(ws, 'G', 2 * N, torch.complex128)
        U, R, P = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('lags', 9 * Ni)
        _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        P.zero_()
        _lib.wait_torch_stream(ws.device)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        op.lagImagingAccumulateDevice(d_uF, U.data_ptr(), k, P.data_ptr(), d_exp=d_exp, rows=Ni)
        w = -scale / np.conj(complex(op.premul))
        if getattr(op, 'eurusDerivatives', False):
            op.jointAdjointDevice(P.data_ptr(), w, G.data_ptr(), G.data_ptr() + 16 * N, conj=True)          # (Eurus: both transposes from one read of P)
            return
        if stretch:
            op.velocityAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
        else:
            op.massAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
        op.buoyancyAdjointDevice(P.data_ptr(), w, G.data_ptr() + 16 * N, conj=True)
    wss = runOnDevices(devs, items, one)
    return _sumPartials(prob, [ws.G for ws in wss if ws.G is not None], n=2 * N).real


def multiscaleGradientFromFields(prob, F, qb, resid, system, linearisation, parameter):
    """prob.Jtvec(u=F, adjoint='transpose') of a multiscale pairing (multiscaleDerivatives=True) with 'operator' or 'full': g = sum_f S_f^T g_f, float64 (N,), or
    (2 N,) [g_c; g_rho] for parameter='joint'.  The item body of `jointGradientFromFields` on the grid of the item's frequency, with the adjoint kernels adding
    into a partial of THAT grid (zeroed per item) instead of the worker's native one; what depends on the model at a cell is applied there -- -1 / rho_f^2 on
    a density half, Gardner's d b / d c at c_f on the buoyancy gradient that joins the velocity one -- and ONE transposed grid transfer (`ds.adjoint`, k = 1 or
    2, beta = 1, queued on the operator's stream) adds the item's partial to the worker's native G.  The real part is taken at the end: S_f is real."""
    import torch
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    scale = F.scale
    stretch = linearisation == 'full'
    joint, density = parameter == 'joint', parameter == 'rho'
    halves = 2 if joint else 1
    if not F.items:
        return _sumPartials(prob, [], n=halves * N).real
    _prepareBackSources(sv, qb, F.ownedFreqs)
    devs, items = _storedItems(system, F)
    _checkSecondFactorsFit(items, planes=9)
    chains = {ifreq: prob._gridChains(ifreq) for ifreq in F.ownedFreqs}          # (host arrays, made on the calling thread)
    ups = [ds.adjoint for ds in sv.preProcessors]

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        d_uF, d_exp = F.pointers(ifreq, c0)
        G = _partial(ws, 'G', halves * N, torch.complex128)
        gk = sv._gridKey(ifreq)
        brho, bc = chains[ifreq]
        gardner = stretch and not density and bc is not None
        brho_d = ws.cached(('grid_brho', gk), lambda: _lib.to_device(brho, dev, np.float64)) if density or joint else None
        bc_d = ws.cached(('grid_bc', gk), lambda: _lib.to_device(bc, dev, np.float64)) if gardner else None
        U, R, P, T = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('lags', 9 * Ni), ws.buffer('gridG', 2 * Ni)
        first, second = T[:Ni], T[Ni:]
        _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        P.zero_()
        T.zero_()
        _lib.wait_torch_stream(dev)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        op.lagImagingAccumulateDevice(d_uF, U.data_ptr(), k, P.data_ptr(), d_exp=d_exp, rows=Ni)
        w = -scale / np.conj(complex(op.premul))
        # (every adjoint call returns when its output is complete, so the torch work below reads finished partials)
        if density:
            op.buoyancyAdjointDevice(P.data_ptr(), w, first.data_ptr(), conj=True)
            first.mul_(brho_d)
        else:
            if stretch:
                op.velocityAdjointDevice(P.data_ptr(), w, first.data_ptr(), conj=True)
            else:
                op.massAdjointDevice(P.data_ptr(), w, first.data_ptr(), conj=True)
            if gardner or joint:
                op.buoyancyAdjointDevice(P.data_ptr(), w, second.data_ptr(), conj=True)
                if joint:
                    second.mul_(brho_d)
                else:
                    first.addcmul_(second, bc_d.to(torch.complex128))
        _lib.wait_torch_stream(dev)
        ups[ifreq].apply_device(T[:halves * Ni], G, k=halves, op=op, beta=1.)
    wss = runOnDevices(devs, items, one)
    return _sumPartials(prob, [ws.G for ws in wss if ws.G is not None], n=halves * N).real


# ---- 2.5-D problems: the exact derivatives from the per-ky store -------------------------------------------------------------------------------------
# The operator of an item is a MiniZephyr25D composite and the store holds the unscaled solves of every ky operator in a block of its own (`fields(perKy=True)`).
# The derivative of the data is a sum over ky of the 2-D expressions of the SAME ky, so the two pipelines below are the item bodies of `_bornPlanesFromFields` and
# of `jointGradientFromFields` with a ky loop inside the item: the composite's own `_kyLoop` (ascending ky, the factorisations of the next group of ky operators
# enqueued one group ahead of their solves, a ky operator destroyed after its step with kyRelease).  Every kernel runs on the ky operator's handle, which carries
# its ky; its premul is the quadrature weight.  What crosses PCIe per item is what the 2-D item moves; nothing crosses per ky.

def _kyTotalScale(F):
    "the wrapper's scale term times the composite's own: what multiplies the unscaled per-ky solves of a per-ky store"
    return F.scale * F.kyCoef[-1][0]


def liveKyFields(prob):
    """What stands for the per-ky store with u=None: the items `fields(perKy=True)` would deal and the composite's coefficients, nothing allocated
    (fieldstore.LiveKyFields).  Made on the calling thread: the survey caches its sources."""
    from .fieldstore import LiveKyFields
    sv = prob.survey
    comp = prob.system.subProblems[0]
    nky = len(comp.subProblems)
    owned = prob.ownedFreqs
    items = deviceItems(prob.system, owned, sv.nsrc)[1] if owned else []
    return LiveKyFields(sv.nfreq, sv.nsrc, [(w, op.device, ifreq, c0, c1) for w, op, ifreq, c0, c1 in items], prob._modelStamp, complex(prob.system.scaleTerm), nky,
                        [comp._kyCoefficients(ky) for ky in range(nky)], sv.getSources())


def _kyLoopBoth(op, fop, each):
    """each(ky, sub, fsub) over the ky operators of the transposed composite `op` and of the forward composite `fop` together, in the order of ky_schedule: the
    factorisations of A_ky^T and of A_ky enqueued one group ahead of their solves; kyRelease destroys both after the step"""
    from .discretization import prefactor_many
    from .minizephyr import KY_GROUP, ky_schedule
    subs, fsubs = op.subProblems, fop.subProblems
    for step, arg in ky_schedule(len(subs), KY_GROUP):
        if step == 'prefactor':
            prefactor_many([subs[ky] for ky in arg])
            prefactor_many([fsubs[ky] for ky in arg])
        else:
            each(arg, subs[arg], fsubs[arg])
            if op.kyRelease:
                del subs[arg].factors
                del fsubs[arg].factors


def kyBornFromFields(prob, F, dc, db, stretch):
    """prob.JvecBorn(u=FK, linearisation='operator' | 'full') of a 2.5-D problem: the derivative of dpred along the velocity perturbation dc and the buoyancy
    perturbation db ((N,) float64, either may be None).  Per stored item and ky: the planes V_ky[dc] (stretch False: k_mass_planes) + L_ky[db] from the ky handle,
    k_stencil_sources on the block of that ky, the solve through A_ky, and the receiver samples accumulated into the item's nrec x k result on the device.  One
    download per item."""
    F.checkCurrent(prob, perKy=True)
    data, stage, sample = _sampling(prob, F.ownedFreqs, _kyTotalScale(F))
    if not F.items:
        return data
    db = None if db is None else np.ascontiguousarray(db, dtype=np.float64)
    dc = None if dc is None else np.ascontiguousarray(dc, dtype=np.float64)
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        staged = stage(ws, ifreq, c0, c1)
        dbd = None if db is None else ws.cached(('born_db', id(db)), lambda: _lib.to_device(db, dev, np.float64), keep=db)
        dcd = None if dc is None else ws.cached(('born_dc', id(dc)), lambda: _lib.to_device(dc, dev, np.float64), keep=dc)
        U, R, C = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('planes', 9 * Ni)
        spare = ws.buffer('lags', 9 * Ni) if (not stretch and dcd is not None and dbd is not None) else None
        if F.live:          # (u = None: the source columns once per item, the forward fields of a ky solved into the workspace just before they are used)
            Q, UF = ws.buffer('Q', k * Ni), ws.buffer('UF', k * Ni)
            _expandColumns(op, F.qf, ifreq, c0, c1, Q)
        _lib.wait_torch_stream(dev)

        def each(ky, sub):
            if F.live:
                sub.solveDevice(Q.data_ptr(), UF.data_ptr(), k, Ni)
                d_uF, d_exp = UF.data_ptr(), None
            else:
                d_uF, d_exp = F.pointers(ifreq, c0, ky)
            if dcd is None:
                sub.buoyancyPlanesDevice(dbd.data_ptr(), C.data_ptr())
            elif stretch:
                sub.velocityPlanesDevice(dcd.data_ptr(), None if dbd is None else dbd.data_ptr(), C.data_ptr())
            elif dbd is None:
                sub.massPlanesDevice(dcd.data_ptr(), C.data_ptr())
            else:
                _jointPlanes(ws, sub, dcd, dbd, C, False, spare)
            sub.stencilSourcesDevice(d_uF, k, C.data_ptr(), -1.0 / complex(sub.premul), R.data_ptr(), conj=True, d_exp=d_exp, rows=Ni)
            sub.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
            _sampleAccumulate(sub, U.data_ptr(), None, k, Ni, staged[0], staged[1], 1.0, 0.0 if ky == 0 else 1.0)
        op._kyLoop(each)
        sample(op, ifreq, c0, c1, staged, None)
    runOnDevices(devs, items, one)
    return data


def kyGradientFromFields(prob, F, qb, resid, system, stretch, wantC, wantB):
    """prob.Jtvec(u=FK, adjoint='transpose', linearisation='operator' | 'full') of a 2.5-D problem up to the real chains: [g_c; g_b], float64 (2 N,) (a half that
    is not wanted stays zero).  Per stored item the back-sources are made ONCE -- they are the same for all ky --; per ky: the solve through A_ky^T (`system`, the
    transposed composites), P zeroed, k_lag_imaging against the block of the SAME ky, and the transposes with the ky handle's parameters and
    w = -st / conj(premul_ky) into the halves of the worker's partial (k_velocity_adjoint, the mass-only one with stretch False; k_buoyancy_adjoint).  One
    all-reduce of the stacked vector where the frequencies are sharded."""
    import torch
    F.checkCurrent(prob, perKy=True)
    sv = prob.survey
    N = prob.nrow
    scale = _kyTotalScale(F)
    if not F.items:
        return _sumPartials(prob, [], n=2 * N).real
    _prepareBackSources(sv, qb, F.ownedFreqs)
    devs, items = _storedItems(system, F)
    forward = {(ifreq, c0): op for _, op, ifreq, c0, _ in _storedItems(prob.system, F)[1]} if F.live else None
    _checkSecondFactorsFit(items, planes=9, blocks=4 if F.live else 2, beside=forward)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        G = _partial(ws, 'G', 2 * N, torch.complex128)
        U, R, P = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('lags', 9 * Ni)
        _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        if F.live:          # (u = None: see kyBornFromFields; the forward fields come from the forward composite of the same frequency and batch, on the same GPU)
            Q, UF = ws.buffer('Q', k * Ni), ws.buffer('UF', k * Ni)
            _expandColumns(op, F.qf, ifreq, c0, c1, Q)
        _lib.wait_torch_stream(ws.device)

        def each(ky, sub, fsub=None):
            if F.live:
                fsub.solveDevice(Q.data_ptr(), UF.data_ptr(), k, Ni)
                d_uF, d_exp = UF.data_ptr(), None
            else:
                d_uF, d_exp = F.pointers(ifreq, c0, ky)
            P.zero_()
            _lib.wait_torch_stream(ws.device)
            sub.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
            sub.lagImagingAccumulateDevice(d_uF, U.data_ptr(), k, P.data_ptr(), d_exp=d_exp, rows=Ni)
            w = -scale / np.conj(complex(sub.premul))
            if wantC and stretch:
                sub.velocityAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
            elif wantC:
                sub.massAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
            if wantB:
                sub.buoyancyAdjointDevice(P.data_ptr(), w, G.data_ptr() + 16 * N, conj=True)
        if F.live:
            _kyLoopBoth(op, forward[(ifreq, c0)], each)
        else:
            op._kyLoop(each)
    wss = runOnDevices(devs, items, one)
    return _sumPartials(prob, [ws.G for ws in wss if ws.G is not None], n=2 * N).real


# ---- visco problems: the chain from (c, Q) to the complex velocity --------------------------------------------------------------------------------
# The operators of a visco wrapper hold the complex velocity c~_f of their frequency; the derivative along real (dc, dQ) is the derivative along the complex
# perturbation gamma_f dc + chi_f dQ (frechet.viscoChain).  The two pipelines below are the item bodies of `_bornPlanesFromFields` / `_bornOperatorFromFields` and of
# `_gradientPlanesFromFields` / `gradientFromFields` with the chain kernels of csrc/survey_visco.hip inserted.  Q goes up once per worker and call; the chain itself
# is made in the kernels from the handle's c~, Q and the scalar lam_f.  What a worker caches per frequency (1 / (c~^3 rho), keyed by the operator's own model array)
# lives in its Workspace, which goes with the call.

def _viscoQOnDevice(ws, Q):
    return ws.cached(('visco_Q', id(Q)), lambda: _lib.to_device(Q, ws.device, np.float64), keep=Q)


def viscoBornFromFields(prob, F, vc, vQ, linearisation, Q, lams):
    """prob.JvecBorn(u=F, parameter='c' | 'Q' | 'cQ') of a visco problem: the derivative of dpred along the real perturbations vc and vQ (N,) float64, either may be
    None.  Per stored item k_visco_perturbation makes dc~ = gamma_f vc + chi_f vQ; then 'full': k_velocity_planes_z and k_stencil_sources, the body of
    `_bornPlanesFromFields`; 'operator': k_virtual_sources_op with the complex weight W = -2 omega_d^2 dc~ / (c~^3 rho), the body of `_bornOperatorFromFields`.
    One Born solve per item.  Q (N,) float64, lams the dispersion scalar per frequency."""
    from .frechet import dampedOmega
    F.checkCurrent(prob)
    data, stage, sample = _sampling(prob, F.ownedFreqs, F.scale)
    if not F.items:
        return data
    stretch = linearisation == 'full'
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        d_uF, d_exp = F.pointers(ifreq, c0)
        staged = stage(ws, ifreq, c0, c1)
        Qd = _viscoQOnDevice(ws, Q)
        vcd = None if vc is None else ws.cached(('born_dc', id(vc)), lambda: _lib.to_device(vc, dev, np.float64), keep=vc)
        vQd = None if vQ is None else ws.cached(('born_dq', id(vQ)), lambda: _lib.to_device(vQ, dev, np.float64), keep=vQ)
        U, R, dcz = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('dcz', Ni)
        C = ws.buffer('planes', 9 * Ni) if stretch else None
        inv = None if stretch else _cachedInverseC3Rho(ws, op)
        _lib.wait_torch_stream(dev)
        op.viscoPerturbationDevice(Qd.data_ptr(), lams[ifreq], None if vcd is None else vcd.data_ptr(), None if vQd is None else vQd.data_ptr(), dcz.data_ptr())
        if stretch:
            op.velocityPlanesComplexDevice(dcz.data_ptr(), C.data_ptr())
            op.stencilSourcesDevice(d_uF, k, C.data_ptr(), -1.0 / complex(op.premul), R.data_ptr(), conj=True, d_exp=d_exp, rows=Ni)
        else:
            om = dampedOmega(op)
            W = inv * dcz * complex(-2.0 * om * om)          # (dcz is complete: the library call has returned)
            _lib.wait_torch_stream(dev)
            op.virtualSourcesOpDevice(d_uF, k, W.data_ptr(), -1.0 / complex(op.premul), R.data_ptr(), conj=True, d_exp=d_exp, rows=Ni)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        sample(op, ifreq, c0, c1, staged, U.data_ptr())
    runOnDevices(devs, items, one)
    return data


def viscoGradientFromFields(prob, F, qb, resid, system, linearisation, parameter, Q, lams):
    """prob.Jtvec(u=F, adjoint='transpose', parameter='c' | 'Q' | 'cQ') of a visco problem: float64 (N,), or [g_c; g_Q] (2 N,), from ONE back-propagation and one
    imaging pass per stored item, whatever the parameter.  The item's complex cell gradient T -- conj(V_f)^T P of `_gradientPlanesFromFields` for 'full', the imaging
    sum of k_imaging_op for 'operator' -- goes into a buffer zeroed per item (a worker's items belong to different frequencies), and k_visco_chain_adjoint adds
    conj(gamma_f) T and conj(chi_f) T into the worker's partial: the pipeline holds the conjugates of the fields, so T is the conjugate of the host route's t_f.
    One all-reduce of the (N,) or (2 N,) vector where the frequencies are sharded."""
    import torch
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    scale = F.scale
    stretch = linearisation == 'full'
    wantC, wantQ = parameter in ('c', 'cQ'), parameter in ('Q', 'cQ')
    n = 2 * N if parameter == 'cQ' else N
    if not F.items:
        return _sumPartials(prob, [], n=n).real
    _prepareBackSources(sv, qb, F.ownedFreqs)
    devs, items = _storedItems(system, F)
    _checkSecondFactorsFit(items, planes=10 if stretch else 1)
    add = None if stretch else _addOperator(prob, scale)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        d_uF, d_exp = F.pointers(ifreq, c0)
        G = _partial(ws, 'G', n, torch.complex128)
        Qd = _viscoQOnDevice(ws, Q)
        U, R, T = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni), ws.buffer('T', Ni)
        _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        T.zero_()
        if stretch:
            P = ws.buffer('lags', 9 * Ni)
            P.zero_()
        else:
            W = add(ws, op, ifreq, Ni)[0]
        _lib.wait_torch_stream(ws.device)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        if stretch:
            op.lagImagingAccumulateDevice(d_uF, U.data_ptr(), k, P.data_ptr(), d_exp=d_exp, rows=Ni)
            op.velocityAdjointDevice(P.data_ptr(), -scale / np.conj(complex(op.premul)), T.data_ptr(), conj=True)
        else:
            op.imagingOpAccumulateDevice(d_uF, U.data_ptr(), k, W.data_ptr(), T.data_ptr(), d_exp=d_exp, rows=Ni)
        op.viscoChainAdjointDevice(Qd.data_ptr(), lams[ifreq], T.data_ptr(), G.data_ptr() if wantC else None,
                                   (G.data_ptr() + (16 * N if wantC else 0)) if wantQ else None, conj=True)
    wss = runOnDevices(devs, items, one)
    return _sumPartials(prob, [ws.G for ws in wss if ws.G is not None], n=n).real


def newtonFromFields(prob, F, p, qb, resid, system, linearisation, parameter):
    """prob.Hvec(u=F, resid=): the full Newton Hessian of 1/2 ||dpred - dobs||^2 times p (N,) float64, float64 (N,), from forward fields already in HBM.  Three
    solves of the item's k columns per stored item, made of the steps of `_gradientPlanesFromFields` and `_bornPlanesFromFields`; `system` the transposed
    operators, whose items the loop runs over (the forward operator of an item is that of the same frequency and batch: the same GPU), qb / resid those of
    R_s^H r.  The store and every solve hold the conjugates of u^, lambda, du and dlambda, so the coefficients are conjugated, not the fields:

      1. lambda~ = the transposed solve of the back-sources of resid                                  (what the gradient solves)
      2. the planes C of p, once per item (k_velocity_planes, k_mass_planes for 'operator', or k_buoyancy_planes of -p / rho^2); R = -(1 / premul) C shift(conj(slice)) (k_stencil_sources),
         du~ = the forward solve
      3. the samples of du~ times scaleTerm (and the phase of `_hermitianResidual`) gathered into back-sources through the survey's adjoint plan
         (helm_rhs_from_samples_device, fixed and moving arrays alike), plus the conjugate of -(1 / conj(premul)) C^H lambda~, which k_stencil_sources_t adds
         to R where it lies; dlambda~ = the transposed solve
      4. P1 += lag(dlambda~, slice) + lag(lambda~, du~), P0 += lag(lambda~, slice) (k_lag_imaging), then G += w conj(V)^T P1 (k_velocity_adjoint) + w p (.) the
         conjugated second derivative contracted with P0 (k_velocity_curvature), w = -scaleTerm / conj(premul).

    parameter='rho': the buoyancy transpose of P1 into G and of P0 into Gb; the worker's partial is then (d b / d rho) G + p (d^2 b / d rho^2) Gb, so that the ranks
    still end in one all-reduce.  linearisation is the resolved one; 'operator' with parameter='c' runs k_mass_planes, the mass-only k_velocity_adjoint and the
    curvature kernel without its stretch part.  Four column blocks (R, lambda~, du~, dlambda~) and 27 planes per worker.

    parameter='joint': p = [p_c; p_rho] (2 N,), the result (2 N,).  The same item body with the planes of the stacked perturbation, V[p_c] + L[db],
    db = -p_rho / rho^2 (`_jointPlanes`), and three partials: the c half of G takes V^T P1, the curvature along p_c and M_c^T[db] P0 (k_velocity_adjoint_b: the
    velocity transpose at the buoyancy db); the b half of G takes L^T P1 and M_b^T[p_c] P0 (k_mixed_adjoint); Gb takes L^T P0.  The worker's partial is then
    [G_c; (d b / d rho) G_b + p_rho (d^2 b / d rho^2) Gb]: one stacked vector, one all-reduce.  The workspace stays at four column blocks and 27 planes ('operator'
    borrows P1, before it is needed, for the second set of planes)."""
    import torch
    F.checkCurrent(prob)
    sv = prob.survey
    N, nrec = prob.nrow, sv.nrec
    scale = F.scale
    density = parameter == 'rho'
    joint = parameter == 'joint'
    stretch = linearisation == 'full'                  # ('operator' with parameter='c': the mass term alone in planes, transpose and curvature)
    if not F.items:
        return _sumPartials(prob, [], n=2 * N if joint else None).real
    p = np.ascontiguousarray(p, dtype=np.float64)
    if joint:
        pert, prho = np.ascontiguousarray(p[:N]), np.ascontiguousarray(p[N:])          # (the velocity half; the density half and its buoyancy perturbation)
        pertb = np.ascontiguousarray(prob._buoyancyChain() * prho)
    else:
        pert = np.ascontiguousarray(prob._buoyancyChain() * p) if density else p
    owned = F.ownedFreqs
    _prepareBackSources(sv, None, owned)                 # (the adjoint plans: step 3 gathers the samples of du through them for a fixed array too, whose qb serves step 1 only)
    Rms = _receiverMatrices(sv, owned)
    stride = nrec if sv.mode != 'fixed' else 0
    phase = scale * np.asarray(prob._hermitianResidual(np.ones((nrec, 1, 1), dtype=np.complex128)), dtype=np.complex128).reshape((nrec, 1))
    devs, items = _storedItems(system, F)
    forward = {(ifreq, c0): op for _, op, ifreq, c0, _ in _storedItems(prob.system, F)[1]}
    _checkSecondFactorsFit(items, planes=27, blocks=4)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        dev = ws.device
        fop = forward[(ifreq, c0)]
        pm = complex(op.premul)
        d_uF, d_exp = F.pointers(ifreq, c0)
        G = _partial(ws, 'G', 2 * N if joint else N, torch.complex128)
        Gb = _partial(ws, 'Gb', N, torch.complex128) if density or joint else None
        vd = ws.cached(('newton_v', id(pert)), lambda: _lib.to_device(pert, dev, np.float64), keep=pert)          # (p, or the buoyancy perturbation that goes with it)
        bd = ws.cached(('newton_b', id(pertb)), lambda: _lib.to_device(pertb, dev, np.float64), keep=pertb) if joint else None
        ph = ws.cached(('newton_phase',), lambda: _lib.to_device(phase, dev, np.complex128))
        gk = sv._gridKey(ifreq)
        csr, out = _csrOnDevice(ws, Rms[gk], gk, nrec, stride, c0), ws.buffer('out', (nrec, k))
        plan = _planOnDevice(ws, sv, ifreq)
        R, L, D, Z = ws.buffer('R', k * Ni), ws.buffer('U', k * Ni), ws.buffer('dU', k * Ni), ws.buffer('dL', k * Ni)
        C, P0, P1 = ws.buffer('planes', 9 * Ni), ws.buffer('lags', 9 * Ni), ws.buffer('lags1', 9 * Ni)
        # 1. lambda~
        _backSources(ws, sv, op, qb, resid, ifreq, c0, c1, R.data_ptr(), Ni)
        P0.zero_()
        P1.zero_()
        _lib.wait_torch_stream(dev)
        op.solveDevice(R.data_ptr(), L.data_ptr(), k, Ni)
        # 2. du~
        if joint:
            _jointPlanes(ws, fop, vd, bd, C, stretch, P1)          # (P1 is not in use yet: zeroed again below where it served as the spare planes)
            if not stretch:
                P1.zero_()
                _lib.wait_torch_stream(dev)
        elif density:
            fop.buoyancyPlanesDevice(vd.data_ptr(), C.data_ptr())
        elif stretch:
            fop.velocityPlanesDevice(vd.data_ptr(), None, C.data_ptr())
        else:
            fop.massPlanesDevice(vd.data_ptr(), C.data_ptr())
        fop.stencilSourcesDevice(d_uF, k, C.data_ptr(), -1.0 / pm, R.data_ptr(), conj=True, d_exp=d_exp, rows=Ni)
        fop.solveDevice(R.data_ptr(), D.data_ptr(), k, Ni)
        # 3. dlambda~
        fop.sampleDevice(D.data_ptr(), k, csr, out.data_ptr())
        out.mul_(ph)                                     # (in place: nrec x k)
        _lib.wait_torch_stream(dev)
        op.rhsFromSamplesDevice(out.data_ptr(), k, plan, c0, c1, R.data_ptr(), rows=Ni)
        op.stencilSourcesTransposedDevice(L.data_ptr(), k, C.data_ptr(), np.conj(-1.0 / pm), R.data_ptr(), conj=True, rows=Ni, accumulate=True)      # (R += its conjugate: no block of its own)
        op.solveDevice(R.data_ptr(), Z.data_ptr(), k, Ni)
        # 4. the lag products and their transposes
        op.lagImagingAccumulateDevice(d_uF, L.data_ptr(), k, P0.data_ptr(), d_exp=d_exp, rows=Ni)
        op.lagImagingAccumulateDevice(d_uF, Z.data_ptr(), k, P1.data_ptr(), d_exp=d_exp, rows=Ni)
        op.lagImagingAccumulateDevice(D.data_ptr(), L.data_ptr(), k, P1.data_ptr(), rows=Ni)
        w = -scale / np.conj(pm)
        if joint:
            # G = [G_c; G_b]: the c half takes V^T P1, the curvature and M_c^T[db] P0; the b half L^T P1 and M_b^T[p_c] P0; Gb = L^T P0, which d^2 b / d rho^2 multiplies
            d_gb = G.data_ptr() + 16 * N
            if stretch:
                op.velocityAdjointDevice(P1.data_ptr(), w, G.data_ptr(), conj=True)
            else:
                op.massAdjointDevice(P1.data_ptr(), w, G.data_ptr(), conj=True)
            op.velocityCurvatureDevice(P0.data_ptr(), vd.data_ptr(), w, G.data_ptr(), conj=True, stretch=stretch)
            op.velocityAdjointBuoyancyDevice(P0.data_ptr(), bd.data_ptr(), w, G.data_ptr(), conj=True, stretch=stretch)
            op.buoyancyAdjointDevice(P1.data_ptr(), w, d_gb, conj=True)
            op.mixedAdjointDevice(P0.data_ptr(), vd.data_ptr(), w, d_gb, conj=True, stretch=stretch)
            op.buoyancyAdjointDevice(P0.data_ptr(), w, Gb.data_ptr(), conj=True)
        elif density:
            op.buoyancyAdjointDevice(P1.data_ptr(), w, G.data_ptr(), conj=True)
            op.buoyancyAdjointDevice(P0.data_ptr(), w, Gb.data_ptr(), conj=True)
        else:
            if stretch:
                op.velocityAdjointDevice(P1.data_ptr(), w, G.data_ptr(), conj=True)
            else:
                op.massAdjointDevice(P1.data_ptr(), w, G.data_ptr(), conj=True)
            op.velocityCurvatureDevice(P0.data_ptr(), vd.data_ptr(), w, G.data_ptr(), conj=True, stretch=stretch)
    wss = [ws for ws in runOnDevices(devs, items, one) if ws.G is not None]
    if density:
        chain, curve = prob._buoyancyChain(), p * prob._buoyancyCurvature()
        for ws in wss:
            ws.G.mul_(_lib.to_device(chain, ws.device, np.float64)).add_(ws.Gb * _lib.to_device(curve, ws.device, np.float64))
    elif joint:
        chain, curve = prob._buoyancyChain(), prho * prob._buoyancyCurvature()
        for ws in wss:          # (the buoyancy half alone: the three partials become one stacked vector per worker, and the ranks still end in one all-reduce)
            ws.G[N:].mul_(_lib.to_device(chain, ws.device, np.float64)).add_(ws.Gb * _lib.to_device(curve, ws.device, np.float64))
    return _sumPartials(prob, [ws.G for ws in wss], n=2 * N if joint else None).real


# ---- illumination / diagonal pseudo-Hessian ---------------------------------------------------------------------------------------------------
# H = sum_f w_f (.) sum_s |u_s|^2 of wavefields that are in HBM anyway: `illumination` solves them into the workspace and drops them,
# `illuminationFromFields` reads a store.  One kernel per item (helm_energy_accumulate_device, or its complex64 form) adds alpha * W (.) sum_s |U_s|^2 to
# the worker's float64 partial `ws.H`; the store and the workspace hold the unscaled solves, so |scaleTerm|^2 is part of alpha.
# With linearisation='full' or parameter='rho' the kernel is helm_pseudo_hessian_accumulate_device instead (`_accumulate`): the same item bodies.
# kind='gaussNewton' (the exact diagonal of J^T J) reads a store through the TRANSPOSED operators' items: per item k_lag_gram makes the 13 autocorrelation planes
# of the slice and k_gauss_newton_diagonal combines them with the planes of the receiver Green's functions, which the worker makes once per frequency and call
# (`_receiverGram`); `illumination` solves the store first and drops it.

def _energyWeight(prob, kind, scale, freqs, linearisation='scaler', parameter='c'):
    """step(ws, op, ifreq) -> (mode, d_chain, alpha, d_w): the accumulate call of an item (`_accumulate`) and what it multiplies its sum by.  mode None: the
    energy kernel, alpha (.) W (.) sum_s |U_s|^2; else the mode of BaseDiscretization.pseudoHessianAccumulateDevice with its chain.  alpha is a float, d_w and
    d_chain device addresses of float64 arrays the worker's cache keeps, or None.
    'energy': |scale|^2 and no array.  'pseudoHessian', linearisation 'scaler': |gradientScaler|^2 |scale|^2 = omega^4 / |c|^6 |scale|^2
    -- with the problem's own scaler W = |1 / c^3|^2 is made once per worker from the cached inv_c3 of _addOnNativeGrid and omega^4 |scale|^2 goes into
    alpha (no torch work per item); otherwise |prob.gradientScaler(ifreq)|^2 is made here, on the calling thread, and uploaded once per worker and
    frequency.  'operator' (the resolved one) with 'c': the closed form, the energy kernel with W = S / |c^3 rho|^2 (S the squared mass weights of the interior
    rows around a cell) and 4 |omega_d|^4 |scale|^2 in alpha.  'full': the velocity star, with d b / d c of the Gardner density where the config gives none.
    'rho': the buoyancy star and W = 1 / rho^4.  A step may enqueue torch work; the item body issues the wait_torch_stream."""
    a2 = scale.real * scale.real + scale.imag * scale.imag
    if kind == 'energy':
        return lambda ws, op, ifreq: (None, None, a2, None)
    if kind == 'gaussNewton':
        # (mode, d_chain, alpha, d_w) of BaseDiscretization.gaussNewtonDiagonalDevice from the pseudo-Hessian's: the same star, chain and density weight.  The
        # planes of the receiver columns are those of conj(premul g_r), so the exact derivatives divide |premul|^2 out; the diagonal weight of 'scaler' keeps
        # it (its data carry premul) and takes |scale|^2 once more, for the scaled virtual source; the mass term alone has a mode of its own and no weight
        base = _energyWeight(prob, 'pseudoHessian', scale, freqs, linearisation, parameter)

        def step(ws, op, ifreq):
            mode, d_chain, alpha, d_w = base(ws, op, ifreq) if not (linearisation == 'operator' and parameter == 'c') else ('mass', None, a2, None)
            if mode is None:
                return 'diagonal', None, abs(alpha) * a2, d_w          # (|omega^2|^2: a damped frequency is complex)
            pm = complex(op.premul)
            return mode, d_chain, alpha / (pm.real * pm.real + pm.imag * pm.imag), d_w
        return step
    if parameter == 'rho':
        def step(ws, op, ifreq):
            rho = op.rho
            W = ws.cached(('ph_inv_rho4', id(rho)), lambda: _lib.to_device(np.broadcast_to(np.asarray(rho, dtype=np.float64).ravel(), (int(op.nrow),)) ** -4.0, ws.device, np.float64),
                          keep=rho)
            return 'buoyancy', None, a2, W.data_ptr()
        return step
    if linearisation == 'full':
        gardner = not prob._hasDensity()

        def step(ws, op, ifreq):
            if not gardner:
                return 'velocity', None, a2, None
            cm = op.c
            ch = ws.cached(('ph_chain', id(cm)), lambda: _lib.to_device(frechet.gardnerChain(np.broadcast_to(np.asarray(cm).ravel(), (int(op.nrow),))), ws.device,
                                                                        np.float64), keep=cm)
            return 'gardner', ch.data_ptr(), a2, None
        return step
    if linearisation == 'operator':
        def step(ws, op, ifreq):
            cm, rho = op.c, op.rho
            inv = _cachedInverseC3Rho(ws, op)
            W = ws.cached(('ph_operator_weight', id(cm), id(rho)),
                          lambda: (inv.real * inv.real + inv.imag * inv.imag) * _lib.to_device(frechet.massWeightSquares(op.nz, op.nx), ws.device, np.float64),
                          keep=(cm, rho))
            om = frechet.dampedOmega(op)
            return None, None, 4.0 * abs(om * om) ** 2 * a2, W.data_ptr()
        return step
    sv = prob.survey
    if prob._plainGradientScaler():
        def step(ws, op, ifreq):
            cm = op.c
            inv = _cachedInverseCube(ws, cm)
            W = ws.cached(('abs2_inv_c3', id(cm)), lambda: inv.real * inv.real + inv.imag * inv.imag, keep=cm)
            omega = 2 * np.pi * sv.freqs[ifreq]
            return None, None, (omega ** 4) * a2, W.data_ptr()
        return step
    host = {}
    for ifreq in freqs:
        w = np.asarray(prob.gradientScaler(ifreq)).ravel()
        host[ifreq] = np.square(w.real) + np.square(w.imag)

    def step(ws, op, ifreq):
        return None, None, a2, ws.cached(('abs2_scaler', ifreq), lambda: _lib.to_device(host[ifreq], ws.device, np.float64)).data_ptr()
    return step


def _accumulate(op, d_u, k, spec, row, d_exp, rows):
    "the accumulate call a step of `_energyWeight` chose: the energy kernel, or the pseudo-Hessian kernel in its mode"
    mode, d_chain, alpha, d_w = spec
    if mode is None:
        op.energyAccumulateDevice(d_u, k, alpha, d_w, row, d_exp=d_exp, rows=rows)
    else:
        op.pseudoHessianAccumulateDevice(d_u, k, mode, d_chain, alpha, d_w, row, d_exp=d_exp, rows=rows)


def _energyRow(ws, shape, ifreq):
    "device pointer of the row of the worker's partial illumination that frequency ifreq adds to (the partial zeroed on first use)"
    import torch
    H = _partial(ws, 'H', shape, torch.float64)
    return H.data_ptr() + (ifreq * shape[1] * 8 if len(shape) == 2 else 0)


def _sumEnergyPartials(prob, parts, shape):
    "the illumination from the workers' partials: summed on the host (8 B per cell and row each), then ONE all-reduce over ranks when the frequencies are sharded"
    import torch
    h = np.zeros(shape, dtype=np.float64)
    for H in parts:
        torch.cuda.synchronize(H.device)
        h += _lib.from_device(H)
    return parallel.allreduce_sum(h) if prob._sharded else h


def _receiverGram(prob, freqs):
    """gram(ws, op, ifreq) -> the 13 planes Gamma_f (a complex128 tensor the worker's cache keeps for the call) of kind='gaussNewton': the nrec columns of the
    fixed array's rVec(0, f).T expanded as back-sources are, solved with the TRANSPOSED operator `op` into the workspace, and one k_lag_gram into zeroed planes.
    The matrices are made here, on the calling thread.  gram issues its own wait_torch_stream before its library calls and returns when the planes are complete."""
    import torch
    sv = prob.survey
    nrec = sv.nrec
    q = {}
    for ifreq in freqs:
        gk = sv._gridKey(ifreq)
        if gk not in q:
            q[gk] = sp.csc_matrix(sv.rVec(0, ifreq).T)

    def gram(ws, op, ifreq):
        def make():
            Ni = int(op.nrow)
            U, R = ws.buffer('U', nrec * Ni), ws.buffer('R', nrec * Ni)
            Cg = torch.zeros(13 * Ni, dtype=torch.complex128, device=ws.device)
            _expandColumns(op, q[sv._gridKey(ifreq)], ifreq, 0, nrec, R)
            _lib.wait_torch_stream(ws.device)
            op.solveDevice(R.data_ptr(), U.data_ptr(), nrec, Ni)
            op.lagGramAccumulateDevice(U.data_ptr(), nrec, Cg.data_ptr(), rows=Ni)
            return Cg
        return ws.cached(('gn_gamma', ifreq), make)
    return gram


def illumination(prob, owned, kind, side, perFreq, linearisation='scaler', parameter='c'):
    """prob.illumination(u=None) with the wavefields kept in HBM (single-grid surveys): per work item (frequency, column batch) the sparse columns -- the
    sources, or the receiver array used as sources -- are expanded on the item's GPU, solved into the workspace's U and accumulated into the worker's
    partial.  Nothing is stored and only the result comes down."""
    sv = prob.survey
    N = prob.nrow
    shape = (sv.nfreq, N) if perFreq else (N,)
    if kind == 'gaussNewton':
        # two sets of columns per frequency through two sets of factors: the forward fields go into a store, which `illuminationFromFields` reads and this call drops
        F = fields(prob, owned, prob.fieldsDtype)
        try:
            return illuminationFromFields(prob, F, kind, perFreq, linearisation, parameter)
        finally:
            F.release()
    if not owned:
        return _sumEnergyPartials(prob, [], shape)
    scale = complex(prob.system.scaleTerm)
    if side == 'source':
        q, ncols = sv.getSources(), sv.nsrc
    else:
        q, ncols = sp.csc_matrix(sv.rVec(0, owned[0]).T), sv.nrec            # (one grid: the one matrix of a fixed array; srTerms included, no tsTerms)
    weight = _energyWeight(prob, kind, scale, owned, linearisation, parameter)
    devs, items = deviceItems(prob.system, owned, ncols)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        row = _energyRow(ws, shape, ifreq)
        U, R = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
        _expandColumns(op, q, ifreq, c0, c1, R)
        spec = weight(ws, op, ifreq)
        _lib.wait_torch_stream(ws.device)                # (covers the zeroed partial and the weight: keep it between the torch work and the library calls)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        _accumulate(op, U.data_ptr(), k, spec, row, None, Ni)
    return _sumEnergyPartials(prob, [ws.H for ws in runOnDevices(devs, items, one) if ws.H is not None], shape)


def illuminationFromFields(prob, F, kind, perFreq, linearisation='scaler', parameter='c'):
    """prob.illumination(u=F) from forward fields already in HBM: no solve, every item of the store reads its slice where it lies, in either store
    format, and adds it to its worker's partial."""
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    shape = (sv.nfreq, N) if perFreq else (N,)
    if not F.items:
        return _sumEnergyPartials(prob, [], shape)
    weight = _energyWeight(prob, kind, F.scale, F.ownedFreqs, linearisation, parameter)
    if kind == 'gaussNewton':
        # the items of the TRANSPOSED operators (the same devices and replicas: every item finds its slice on its own GPU), which solve the receiver columns;
        # the two kernels need an assembled 2-D MiniZephyr handle of the frequency, which those are
        gram = _receiverGram(prob, F.ownedFreqs)
        devs, items = _storedItems(prob.adjointSystem, F)
        _checkSecondFactorsFit(items, planes=26, cols=sv.nrec)

        def one(ws, op, ifreq, c0, c1):
            k, Ni = c1 - c0, int(op.nrow)
            d_uF, d_exp = F.pointers(ifreq, c0)
            row = _energyRow(ws, shape, ifreq)
            mode, d_chain, alpha, d_w = weight(ws, op, ifreq)
            Cu = ws.buffer('gram', 13 * Ni)
            Cu.zero_()
            Cg = gram(ws, op, ifreq)
            _lib.wait_torch_stream(ws.device)
            op.lagGramAccumulateDevice(d_uF, k, Cu.data_ptr(), d_exp=d_exp, rows=Ni)
            op.gaussNewtonDiagonalDevice(mode, d_chain, d_w, Cu.data_ptr(), Cg.data_ptr(), alpha, row)
        return _sumEnergyPartials(prob, [ws.H for ws in runOnDevices(devs, items, one) if ws.H is not None], shape)
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        d_uF, d_exp = F.pointers(ifreq, c0)
        row = _energyRow(ws, shape, ifreq)
        spec = weight(ws, op, ifreq)
        _lib.wait_torch_stream(ws.device)
        _accumulate(op, d_uF, k, spec, row, d_exp, Ni)
    return _sumEnergyPartials(prob, [ws.H for ws in runOnDevices(devs, items, one, factor=False) if ws.H is not None], shape)


# ---- per-cell 2 x 2 blocks of the joint (c, rho) Hessian -----------------------------------------------------------------------------------------
# The item steps of `illumination` / `illuminationFromFields` with a partial of three rows per frequency (H_cc, H_crho, H_rhorho) and the accumulate calls of
# the block kernels: k_pseudo_hessian_blocks where the pseudo-Hessian kernel stood, k_gauss_newton_blocks on the same 26 planes where the diagonal's trace stood.
# The density weights are the kernels' own (the handle's rho), so there is no weight array: alpha is |scaleTerm|^2 (over |premul|^2 for 'gaussNewton', whose
# receiver planes carry premul).

def _blocksRow(ws, shape, ifreq):
    "device pointer of the three rows of the worker's partial blocks that frequency ifreq adds to (the partial zeroed on first use)"
    import torch
    H = _partial(ws, 'H', shape, torch.float64)
    return H.data_ptr() + (ifreq * 3 * shape[-1] * 8 if len(shape) == 3 else 0)


def hessianBlocks(prob, owned, kind, side, perFreq, linearisation='full'):
    """prob.hessianBlocks(u=None) with the wavefields kept in HBM (single-grid surveys): `illumination` with the block kernels.  'gaussNewton' solves the forward
    fields into a store, which `hessianBlocksFromFields` reads and this call drops."""
    sv = prob.survey
    N = prob.nrow
    shape = (sv.nfreq, 3, N) if perFreq else (3, N)
    if kind == 'gaussNewton':
        F = fields(prob, owned, prob.fieldsDtype)
        try:
            return hessianBlocksFromFields(prob, F, kind, perFreq, linearisation)
        finally:
            F.release()
    if not owned:
        return _sumEnergyPartials(prob, [], shape)
    scale = complex(prob.system.scaleTerm)
    a2 = scale.real * scale.real + scale.imag * scale.imag
    if side == 'source':
        q, ncols = sv.getSources(), sv.nsrc
    else:
        q, ncols = sp.csc_matrix(sv.rVec(0, owned[0]).T), sv.nrec            # (one grid: the one matrix of a fixed array; srTerms included, no tsTerms)
    stretch = linearisation == 'full'
    devs, items = deviceItems(prob.system, owned, ncols)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        row = _blocksRow(ws, shape, ifreq)
        U, R = ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
        _expandColumns(op, q, ifreq, c0, c1, R)
        _lib.wait_torch_stream(ws.device)                # (covers the zeroed partial: keep it between the torch work and the library calls)
        op.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
        op.pseudoHessianBlocksDevice(U.data_ptr(), k, stretch, a2, row, ldh=Ni, rows=Ni)
    return _sumEnergyPartials(prob, [ws.H for ws in runOnDevices(devs, items, one) if ws.H is not None], shape)


def hessianBlocksFromFields(prob, F, kind, perFreq, linearisation='full'):
    """prob.hessianBlocks(u=F) from forward fields already in HBM: no forward solve, every item of the store reads its slice where it lies, in either store
    format, and adds its three rows to its worker's partial."""
    F.checkCurrent(prob)
    sv = prob.survey
    N = prob.nrow
    shape = (sv.nfreq, 3, N) if perFreq else (3, N)
    if not F.items:
        return _sumEnergyPartials(prob, [], shape)
    scale = F.scale
    a2 = scale.real * scale.real + scale.imag * scale.imag
    stretch = linearisation == 'full'
    if kind == 'gaussNewton':
        gram = _receiverGram(prob, F.ownedFreqs)
        devs, items = _storedItems(prob.adjointSystem, F)
        _checkSecondFactorsFit(items, planes=26, cols=sv.nrec)

        def one(ws, op, ifreq, c0, c1):
            k, Ni = c1 - c0, int(op.nrow)
            d_uF, d_exp = F.pointers(ifreq, c0)
            row = _blocksRow(ws, shape, ifreq)
            pm = complex(op.premul)
            Cu = ws.buffer('gram', 13 * Ni)
            Cu.zero_()
            Cg = gram(ws, op, ifreq)
            _lib.wait_torch_stream(ws.device)
            op.lagGramAccumulateDevice(d_uF, k, Cu.data_ptr(), d_exp=d_exp, rows=Ni)
            op.gaussNewtonBlocksDevice(stretch, Cu.data_ptr(), Cg.data_ptr(), a2 / (pm.real * pm.real + pm.imag * pm.imag), row, ldh=Ni)
        return _sumEnergyPartials(prob, [ws.H for ws in runOnDevices(devs, items, one) if ws.H is not None], shape)
    devs, items = _storedItems(prob.system, F)

    def one(ws, op, ifreq, c0, c1):
        k, Ni = c1 - c0, int(op.nrow)
        d_uF, d_exp = F.pointers(ifreq, c0)
        row = _blocksRow(ws, shape, ifreq)
        _lib.wait_torch_stream(ws.device)
        op.pseudoHessianBlocksDevice(d_uF, k, stretch, a2, row, ldh=Ni, d_exp=d_exp, rows=Ni)
    return _sumEnergyPartials(prob, [ws.H for ws in runOnDevices(devs, items, one, factor=False) if ws.H is not None], shape)


# ---- the data misfit: value, source estimate and gradient with the data kept in HBM ----------------------------------------------------------------------
# misfit.DataMisfit on what these pipelines serve (Helm2DProblem over MiniZephyr / MiniZephyrHD on one grid; 'c', 'rho', 'joint'; 'operator', 'full').  The
# samples of an item stay where the sampling kernel wrote them: the kernels of csrc/survey_misfit.hip turn the panel into the adjoint source in place, the
# back-sources are gathered from it (`_backSources` with a DevicePanels) and what comes down per item is 3 k doubles twice.  `misfitFromFields` runs over a store
# and hands its panels to the existing gradient pipelines; `misfitOnePass` solves the forward columns of an item, images against them and forgets them.
#
# The sums of a group that spans columns (source='perFrequency') and the division a / b are formed on the host, from the per-column sums in column order by
# the same function in every route (`_misfitSources`, `_misfitCoefficients`): a route changes where the columns come from, not the bits of s.

MISFIT_KINDS = {'l2': 0, 'huber': 1, 'hybrid': 2, 'logarithmic': 3}


def _misfitSetup(prob, phi):
    "calling-thread half of the misfit item steps: the kernel's kind and parameters, the receiver phase of `_hermitianResidual` (None: real receiver terms)"
    pr = phi.params
    par = {'l2': (0., 0.), 'huber': (pr.get('threshold', 0.), 0.), 'hybrid': (pr.get('epsilon', 0.), 0.),
           'logarithmic': (pr.get('amplitude', 0.), pr.get('phase', 0.))}[phi.kind]
    return dict(kind=MISFIT_KINDS[phi.kind], par=(float(par[0]), float(par[1])), phase=prob._hermitianPhase())


def _misfitData(ws, phi, ifreq, c0, c1):
    "the item's dobs and w2 panels (w2: None without weights) on the worker's GPU: uploaded once per DataMisfit and GPU, kept with the DataMisfit"
    key = (ws.device.index, int(ifreq), int(c0), int(c1))
    held = phi._devicePanels
    if key not in held:
        D = _lib.to_device(np.ascontiguousarray(phi.dobs[:, c0:c1, ifreq]), ws.device, np.complex128)
        W = None if phi.weights is None else _lib.to_device(np.ascontiguousarray(phi.weights[:, c0:c1, ifreq]), ws.device, np.float64)
        held[key] = (D, W)
    return held[key]


def _ptr(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def misfitMomentsDevice(op, P, D, W):
    "(k, 3) float64 on the host: (Re a_j, Im a_j, b_j) of the columns of the (nrec, k) panels P, D (complex128) and W (float64 or None) on op's GPU"
    import torch
    nrec, k = P.shape
    mom = torch.empty((k, 3), dtype=torch.float64, device=P.device)
    _lib.wait_torch_stream(P.device)
    _lib.check(_lib.load().helm_misfit_moments_device(op.handle, _ptr(P), _ptr(D), _ptr(W), int(P.stride(0)), int(nrec), int(k), _ptr(mom)), op.handle)
    return _lib.from_device(mom)


def misfitTermsDevice(op, kind, par, P, D, W, s, PSI):
    "PSI (a panel like P) = psi at the source factors s (k complex128, host) and (k, 3) float64 on the host: (phi_j, Re c_j, Im c_j)"
    import torch
    nrec, k = P.shape
    S = _lib.to_device(np.ascontiguousarray(s, dtype=np.complex128), P.device, np.complex128)
    out = torch.empty((k, 3), dtype=torch.float64, device=P.device)
    _lib.wait_torch_stream(P.device)
    _lib.check(_lib.load().helm_misfit_terms_device(op.handle, int(kind), par[0], par[1], _ptr(P), _ptr(D), _ptr(W), _ptr(S), int(P.stride(0)), int(nrec), int(k),
                                                    _ptr(PSI), _ptr(out)), op.handle)
    return _lib.from_device(out)


def misfitAdjointDevice(op, kind, par, PSI, s, coef, P, D, W, phase, V, GN=None):
    """V (P itself, or a panel like it) = phase (conj(s) psi + w2 (e d - f p)); coef (k, 3) float64 on the host or None (a given source); phase a device tensor of
    nrec complex128 or None; GN: None or a float64 panel like P for the Gauss-Newton weights"""
    nrec, k = P.shape
    S = _lib.to_device(np.ascontiguousarray(s, dtype=np.complex128), P.device, np.complex128)
    C = None if coef is None else _lib.to_device(np.ascontiguousarray(coef, dtype=np.float64), P.device, np.float64)
    _lib.wait_torch_stream(P.device)
    _lib.check(_lib.load().helm_misfit_adjoint_device(op.handle, int(kind), par[0], par[1], _ptr(PSI), _ptr(S), _ptr(C), _ptr(P), _ptr(D), _ptr(W), _ptr(phase),
                                                      int(P.stride(0)), int(nrec), int(k), _ptr(V), _ptr(GN)), op.handle)


def _misfitSources(phi, ifreq, mom, c0=0):
    """s of the columns c0 .. c0 + len(mom) - 1 of frequency ifreq, complex128, from their moments (len, 3).  The columns are a whole group or several: one
    (source, frequency) each, or -- 'perFrequency' -- all the columns of the frequency"""
    if phi.source == 'given':
        return np.ones(len(mom), dtype=np.complex128) if phi._given is None else np.array(phi._given[c0:c0 + len(mom), ifreq])
    a, b = mom[:, 0] + 1j * mom[:, 1], mom[:, 2]
    if phi.source == 'perFrequency':
        a, b = np.full(a.shape, a.sum()), np.full(b.shape, b.sum())
    if np.any(b == 0):
        from .misfit import _groupName
        raise ValueError('no source estimate for %s: its weighted predicted energy sum w2 |p|^2 is zero' % _groupName(phi.source, c0 + int(np.flatnonzero(b == 0)[0]), ifreq))
    return a / b


def _misfitCoefficients(phi, mom, out, s):
    "(e, f) of the same columns as the adjoint kernel takes them, (len, 3) float64: e = c / b, f = 2 Re(c s) / b of the column's group (an estimated source)"
    c, b = out[:, 1] + 1j * out[:, 2], mom[:, 2]
    if phi.source == 'perFrequency':
        c, b = np.full(c.shape, c.sum()), np.full(b.shape, b.sum())
    e = c / b
    return np.stack([e.real, e.imag, 2 * (c * s).real / b], axis=1)


def _misfitSampler(prob, freqs, scale):
    """sampled(ws, op, ifreq, c0, c1, d_u, d_exp) -> a fresh (nrec, k) panel on the item's GPU with p = scale R u of the k wavefields at d_u; the receiver CSR is
    the one `_sampling` uploads (made here, on the calling thread)"""
    import torch
    sv = prob.survey
    nrec = sv.nrec
    stride = nrec if sv.mode != 'fixed' else 0
    Rms = _receiverMatrices(sv, freqs)

    def sampled(ws, op, ifreq, c0, c1, d_u, d_exp):
        gk = sv._gridKey(ifreq)
        csr = _csrOnDevice(ws, Rms[gk], gk, nrec, stride, c0)
        P = torch.empty((nrec, c1 - c0), dtype=torch.complex128, device=ws.device)
        _lib.wait_torch_stream(ws.device)
        op.sampleDevice(d_u, c1 - c0, csr, P.data_ptr(), d_exp=d_exp)
        if scale != 1.0:
            P.mul_(scale)
        return P
    return sampled


class _MisfitState(object):
    "what the passes of a misfit evaluation share: per-column sums of every owned frequency on the host, the panels of every item on its GPU"

    def __init__(self, prob, phi):
        _, nsrc, nfreq = phi.shape
        self.phi, self.setup = phi, _misfitSetup(prob, phi)
        self.mom = np.zeros((nfreq, nsrc, 3))
        self.out = np.zeros((nfreq, nsrc, 3))
        self.S = np.zeros((nsrc, nfreq), dtype=np.complex128)
        self.coef = np.zeros((nfreq, nsrc, 3))
        self.held = {}                     # (ifreq, c0) -> (P, D, W, PSI)
        self.panels = DevicePanels()

    def moments(self, ws, op, ifreq, c0, c1, P):
        import torch
        D, W = _misfitData(ws, self.phi, ifreq, c0, c1)
        self.held[(ifreq, c0)] = (P, D, W, torch.empty_like(P))
        if self.phi.source != 'given':
            self.mom[ifreq, c0:c1] = misfitMomentsDevice(op, P, D, W)

    def sources(self, ifreq, c0=0, c1=None):
        self.S[c0:c1, ifreq] = _misfitSources(self.phi, ifreq, self.mom[ifreq, c0:c1], c0)

    def terms(self, op, ifreq, c0, c1):
        P, D, W, PSI = self.held[(ifreq, c0)]
        self.out[ifreq, c0:c1] = misfitTermsDevice(op, self.setup['kind'], self.setup['par'], P, D, W, self.S[c0:c1, ifreq], PSI)

    def coefficients(self, ifreq, c0=0, c1=None):
        if self.phi.source != 'given':
            self.coef[ifreq, c0:c1] = _misfitCoefficients(self.phi, self.mom[ifreq, c0:c1], self.out[ifreq, c0:c1], self.S[c0:c1, ifreq])

    def adjoint(self, ws, op, ifreq, c0, c1):
        P, D, W, PSI = self.held.pop((ifreq, c0))
        ph = self.setup['phase']
        phase = None if ph is None else ws.cached(('misfit_phase', id(ph)), lambda: _lib.to_device(ph, ws.device, np.complex128), keep=ph)
        coef = None if self.phi.source == 'given' else self.coef[ifreq, c0:c1]
        misfitAdjointDevice(op, self.setup['kind'], self.setup['par'], PSI, self.S[c0:c1, ifreq], coef, P, D, W, phase, P)
        self.panels.put(ifreq, c0, c1, P)

    def item(self, ws, op, ifreq, c0, c1, P):
        "all passes of an item whose groups lie inside it"
        self.moments(ws, op, ifreq, c0, c1, P)
        self.sources(ifreq, c0, c1)
        self.terms(op, ifreq, c0, c1)
        self.coefficients(ifreq, c0, c1)
        self.adjoint(ws, op, ifreq, c0, c1)

    def result(self, prob, owned):
        "(value, source terms): summed over the owned frequencies, then over ranks where the frequencies are sharded"
        nsrc, nfreq = self.S.shape
        pack = np.zeros(1 + 2 * nsrc * nfreq)
        pack[0] = sum(float(np.add.reduce(self.out[ifreq, :, 0])) for ifreq in owned)
        own = np.zeros(nfreq, dtype=bool)
        own[list(owned)] = True
        pack[1:] = np.where(own[None, :], self.S, 0).ravel().view(np.float64)
        if prob._sharded:
            pack = parallel.allreduce_sum(pack)
        return float(pack[0]), np.array(pack[1:]).view(np.complex128).reshape(nsrc, nfreq)


def _itemsPerFrequency(items):
    n = {}
    for it in items:
        n[it[2]] = n.get(it[2], 0) + 1
    return n


def misfitInOnePass(phi, items):
    "True when no group of the misfit spans two items: a given or per-source factor, or every frequency's columns in one item"
    return phi.source in ('given', 'perSource') or all(n == 1 for n in _itemsPerFrequency(items).values())


def _panelGradient(prob, F, panels, linearisation, parameter):
    "the device branch of Jtvec(adjoint='transpose') with the adjoint source in `panels`, up to the real chain on a density half (the caller applies d b / d rho)"
    adj = prob.adjointSystem
    if parameter == 'joint':
        return jointGradientFromFields(prob, F, None, panels, adj, linearisation)
    if parameter == 'rho':
        return gradientFromFields(prob, F, None, panels, system=adj, linearisation=linearisation, parameter='rho')
    if linearisation == 'full':
        return gradientFromFields(prob, F, None, panels, system=adj, linearisation='full', chain=prob._gardnerChain())
    return gradientFromFields(prob, F, None, panels, system=adj, linearisation=linearisation)


def misfitFromFields(prob, F, phi, linearisation, parameter):
    """(value, source terms (nsrc, nfreq), gradient) of the misfit `phi` from forward fields in HBM; linearisation 'operator' or 'full' as `_resolveLinearisation`
    left it, parameter 'c', 'rho' or 'joint'; the gradient is what the pipeline of that pair returns (a density half still wants d b / d rho).
    Pass 1 over the store's own items: sample, scale, k_misfit_moments -- 3 k doubles per item come down.  Host: s per group.  Pass 2: k_misfit_terms, 3 k doubles
    down.  Host: c per group.  Pass 3: k_misfit_adjoint in place of the samples.  Then the gradient pipeline with the panels as `resid`.  Where no group spans
    two items (`misfitInOnePass`) the three passes are one."""
    F.checkCurrent(prob)
    owned = F.ownedFreqs
    st = _MisfitState(prob, phi)
    if F.items:
        sampled = _misfitSampler(prob, owned, F.scale)
        devs, items = _storedItems(prob.system, F)
        collapse = misfitInOnePass(phi, items)

        def first(ws, op, ifreq, c0, c1):
            P = sampled(ws, op, ifreq, c0, c1, *F.pointers(ifreq, c0))
            if collapse:
                st.item(ws, op, ifreq, c0, c1, P)
            else:
                st.moments(ws, op, ifreq, c0, c1, P)
        runOnDevices(devs, items, first, factor=False)
        if not collapse:
            for ifreq in owned:
                st.sources(ifreq)
            runOnDevices(devs, items, lambda ws, op, ifreq, c0, c1: st.terms(op, ifreq, c0, c1), factor=False)
            for ifreq in owned:
                st.coefficients(ifreq)
            runOnDevices(devs, items, st.adjoint, factor=False)
    g = _panelGradient(prob, F, st.panels, linearisation, parameter)
    val, S = st.result(prob, owned)
    return val, S, g


def misfitOnePass(prob, phi, linearisation, parameter):
    """`misfitFromFields` without a store, for a misfit whose groups lie inside the items (`misfitInOnePass`): per freshly dealt item the sources are expanded and
    solved forward into the workspace, sampled, the misfit kernels make the adjoint source in place of the samples, the back-sources are gathered from the panel,
    solved through the transposed operator of the same GPU and replica, and the imaging or plane kernels of the gradient pipeline of (linearisation, parameter)
    run against the workspace's forward fields.  Only the fields of one item are held; the factors of A and of A^T are resident side by side.  The kernels, their
    inputs and the order in which a worker adds to its partial are those of the store route over a complex128 store: the same bits where the items coincide."""
    import torch
    sv = prob.survey
    N = prob.nrow
    owned = prob.ownedFreqs
    scale = complex(prob.system.scaleTerm)
    joint, density = parameter == 'joint', parameter == 'rho'
    planes = joint or density or linearisation == 'full'
    stretch = linearisation == 'full'
    chain = prob._gardnerChain() if (linearisation == 'full' and not joint and not density) else None
    gardner = chain is not None
    n = 2 * N if joint else N
    st = _MisfitState(prob, phi)
    wss = []
    if owned:
        qf = sv.getSources()
        adj = prob.adjointSystem
        devs, items = deviceItems(prob.system, owned, sv.nsrc)
        back = deviceItems(adj, owned, sv.nsrc)[1]                # (the same deal: the transposed operator of the same frequency, batch and GPU)
        partner = {(ifreq, c0): aop for _, aop, ifreq, c0, _ in back}
        _prepareBackSources(sv, None, owned)
        _checkSecondFactorsFit(back, planes=9 if planes else 0, blocks=3, beside={(ifreq, c0): op for _, op, ifreq, c0, _ in items})
        sampled = _misfitSampler(prob, owned, scale)
        add = None if planes else _addOperator(prob, scale)

        def one(ws, op, ifreq, c0, c1):
            k, Ni = c1 - c0, int(op.nrow)
            aop = partner[(ifreq, c0)]
            G = _partial(ws, 'G', n, torch.complex128)
            Gb = _partial(ws, 'Gb', N, torch.complex128) if gardner else None
            UF, U, R = ws.buffer('UF', k * Ni), ws.buffer('U', k * Ni), ws.buffer('R', k * Ni)
            _expandColumns(op, qf, ifreq, c0, c1, R)
            _lib.wait_torch_stream(ws.device)
            op.solveDevice(R.data_ptr(), UF.data_ptr(), k, Ni)
            st.item(ws, op, ifreq, c0, c1, sampled(ws, op, ifreq, c0, c1, UF.data_ptr(), None))
            _backSources(ws, sv, aop, None, st.panels, ifreq, c0, c1, R.data_ptr(), Ni)
            if not planes:
                scaler, target, _ = add(ws, aop, ifreq, Ni)
                _lib.wait_torch_stream(ws.device)
                aop.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
                aop.imagingOpAccumulateDevice(UF.data_ptr(), U.data_ptr(), k, scaler.data_ptr(), target.data_ptr(), d_exp=None, rows=Ni)
                return
            P = ws.buffer('lags', 9 * Ni)
            P.zero_()
            _lib.wait_torch_stream(ws.device)
            aop.solveDevice(R.data_ptr(), U.data_ptr(), k, Ni)
            aop.lagImagingAccumulateDevice(UF.data_ptr(), U.data_ptr(), k, P.data_ptr(), d_exp=None, rows=Ni)
            w = -scale / np.conj(complex(aop.premul))
            if density:
                aop.buoyancyAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
                return
            if stretch:
                aop.velocityAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
            else:
                aop.massAdjointDevice(P.data_ptr(), w, G.data_ptr(), conj=True)
            if joint:
                aop.buoyancyAdjointDevice(P.data_ptr(), w, G.data_ptr() + 16 * N, conj=True)
            elif gardner:
                aop.buoyancyAdjointDevice(P.data_ptr(), w, Gb.data_ptr(), conj=True)
        wss = runOnDevices(devs, items, one)
    g = _sumPartials(prob, [ws.G for ws in wss if ws.G is not None], n=n).real
    if gardner:
        g = g + chain * _sumPartials(prob, [ws.Gb for ws in wss if ws.Gb is not None]).real
    val, S = st.result(prob, owned)
    return val, S, g
