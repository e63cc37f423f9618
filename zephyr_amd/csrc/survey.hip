// The plumbing of a survey, what it runs on the device besides the solves and the derivatives: right-hand sides from sparse sources and from residual samples
// (and the support bits of the former), axpby, the pack of the optional complex64 store of forward wavefields, the imaging condition, illumination (energy), the
// virtual sources of the Born data and receiver sampling.  Each kernel stands beside the C entry point that launches it.  The derivative kernels of the 2-D
// MiniZephyr operator are in survey_frechet.hip, the two Hessian diagonals in survey_hessian.hip; survey_internal.hpp holds what the three share, the complex64
// store's format and its readers among it.
#include "survey_internal.hpp"

// ------------------------------------------------------------------------------------------
// right-hand sides from sparse data
// ------------------------------------------------------------------------------------------
// dense right-hand sides from the triplets of a sparse matrix (no duplicate entries): R[col][row] = val
__global__ __launch_bounds__(256) void k_rhs_from_coo(const long long *__restrict__ row, const int *__restrict__ col, const cplx *__restrict__ val,
                                                      long long nnz, cplx *__restrict__ R, long long rows, int nrhs, int node_major) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long long)gridDim.x * blockDim.x) {
        if (node_major) R[row[k] * nrhs + col[k]] = val[k];          // the reference's (rows, nrhs) C-order array
        else R[(long long)col[k] * rows + row[k]] = val[k];
    }
}
int helm_launch_rhs_from_coo(helm_op *op, const long long *row, const int *col, const cplx *val, long long nnz, cplx *R, int nrhs, long long rows, int node_major) {
    HIP_TRY(op, hipMemsetAsync(R, 0, (size_t)nrhs * rows * sizeof(cplx), op->stream));
    if (nnz > 0) HELM_LAUNCH(k_rhs_from_coo, dim3((unsigned)std::min<long long>((nnz + 255) / 256, 65535)), dim3(256), 0, op->stream, row, col, val, nnz, R, rows, nrhs, node_major);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

extern "C" int helm_rhs_from_coo_device(helm_op *op, const void *d_row, const void *d_col, const void *d_val, long long nnz, void *dR, int nrhs, long long rows) {
    return helm_rhs_from_coo_device_layout(op, d_row, d_col, d_val, nnz, dR, nrhs, rows, 0);
}

extern "C" int helm_rhs_from_coo_device_layout(helm_op *op, const void *d_row, const void *d_col, const void *d_val, long long nnz, void *dR, int nrhs, long long rows, int flags) {
    helm_tuning_refresh();
    if (!op || !dR || nrhs < 1 || rows < 1 || nnz < 0 || (nnz > 0 && (!d_row || !d_col || !d_val))) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    int rc = helm_launch_rhs_from_coo(op, (const long long *)d_row, (const int *)d_col, (const cplx *)d_val, nnz, (cplx *)dR, nrhs, rows, (flags & HELM_RHS_NODE_MAJOR) ? 1 : 0);
    if (rc) return rc;
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}

__global__ __launch_bounds__(256) void k_support_from_coo(const long long *row, const int *col, long long nnz, long long rows, int nrhs, unsigned *words) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nnz; k += (long long)gridDim.x * blockDim.x) {
        const long long r = row[k]; const int c = col[k];
        if (r < 0 || r >= rows || c < 0 || c >= nrhs) continue;
        atomicOr(&words[r >> 2], (1u << (c >> 6)) << (8 * (int)(r & 3)));
    }
}
// bits (rows bytes, rounded up to a multiple of 4, on the device) from the triplets of a sparse right-hand-side matrix (device arrays as for
// helm_rhs_from_coo_device_layout): what helm_set_rhs_support takes
extern "C" int helm_rhs_support_from_coo(helm_op *op, const void *d_row, const void *d_col, long long nnz, void *d_bits, long long rows, int nrhs) {
    helm_tuning_refresh();
    if (!op || !d_bits || rows < 1 || nrhs < 1 || nrhs > 512 || nnz < 0 || (nnz > 0 && (!d_row || !d_col))) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HIP_TRY(op, hipMemsetAsync(d_bits, 0, (size_t)((rows + 3) / 4) * 4, op->stream));
    if (nnz > 0) HELM_LAUNCH(k_support_from_coo, dim3((unsigned)std::min<long long>((nnz + 255) / 256, 4096)), dim3(256), 0, op->stream,
                                    (const long long *)d_row, (const int *)d_col, nnz, rows, nrhs, (unsigned *)d_bits);
    return launched(op);
}

// Back-sources of a receiver array that moves with the source, R[s - src0][cell] = sum_r R_s[r][cell] resid[r][s - src0], as a GATHER over the touched
// (source, cell) pairs: pair t owns the entries tptr[t] .. tptr[t+1] of (trec, tval), ordered by receiver, and is written by exactly one thread in that
// order.  Receivers of one source share cells (their patches overlap), so a scatter over the entries would need atomics and the sum would depend on
// their order; this one is the same bits on every run.  resid: [nrec][ld], column s - src0 belongs to source s.  R: [nsrc][rows], zeroed by the entry point.
__global__ __launch_bounds__(256) void k_rhs_from_samples(const cplx *__restrict__ resid, long long ld, int src0, const long long *__restrict__ tptr,
                                                          const int *__restrict__ tsrc, const long long *__restrict__ tcell, const int *__restrict__ trec,
                                                          const cplx *__restrict__ tval, long long ntouch, cplx *__restrict__ R, long long rows) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < ntouch; t += (long long)gridDim.x * blockDim.x) {
        const int s = tsrc[t] - src0;
        cplx acc = cmake(0.0, 0.0);
        for (long long e = tptr[t]; e < tptr[t + 1]; ++e) cfma(acc, tval[e], resid[(long long)trec[e] * ld + s]);
        R[(long long)s * rows + tcell[t]] = acc;
    }
}
// Back-sources R_s^T resid[:, s] of the sources src0 .. src0 + nsrc - 1 from the residual samples of one frequency (survey.py:171-188, the moving-array
// branch): only the nrec x nsrc samples cross PCIe, the dense right-hand sides are made here.  The plan arrays are trusted (the caller validated them when it
// built them: cells < rows, receivers < nrec, sources ascending within [src0, src0 + nsrc)).
extern "C" int helm_rhs_from_samples_device(helm_op *op, const void *d_resid, long long ld_resid, int nrec, int nsrc, int src0, const void *d_tptr, const void *d_tsrc,
                                            const void *d_tcell, const void *d_trec, const void *d_tval, long long ntouch, void *dR, long long rows) {
    helm_tuning_refresh();
    if (!op || !d_resid || !dR || nrec < 1 || nsrc < 1 || src0 < 0 || ld_resid < nsrc || rows < 1 || ntouch < 0) return HELM_ERR_ARG;
    if (ntouch > 0 && (!d_tptr || !d_tsrc || !d_tcell || !d_trec || !d_tval)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HIP_TRY(op, hipMemsetAsync(dR, 0, (size_t)nsrc * rows * sizeof(cplx), op->stream));
    if (ntouch > 0) HELM_LAUNCH(k_rhs_from_samples, dim3((unsigned)std::min<long long>((ntouch + 255) / 256, 65535)), dim3(256), 0, op->stream,
                                (const cplx *)d_resid, ld_resid, src0, (const long long *)d_tptr, (const int *)d_tsrc, (const long long *)d_tcell,
                                (const int *)d_trec, (const cplx *)d_tval, ntouch, (cplx *)dR, rows);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// axpby
// ------------------------------------------------------------------------------------------
// Y = beta Y + alpha X over n complex128 values: the ky accumulation of the 2.5-D composite.  A pure streaming pass (48 B per element, 32 with BETA0):
// one 16-byte load / store per lane and element, 64-bit indices.  A workgroup takes 256 CONSECUTIVE elements, one per lane, and there is a workgroup per 256
// elements up to AXPBY_BLOCKS (n <= 2^30: a single trip through the loop), striding beyond: measured on 0.27 .. 8.6 GB operands, this order ran at 5.8-5.9 TB/s
// where 2048 workgroups striding with four elements 8 MB apart in flight per lane ran at 4.5-5.0, and two to eight elements per lane in a workgroup-contiguous
// tile at 5.3-5.6.  BETA0: Y is write-only.
constexpr int AXPBY_BLOCKS = 1 << 22;
// one element.  Contraction is pinned off: each complex product is rounded on its own (within sqrt(5) u of the exact one in modulus) and ONE addition follows
// (+ u), the error model (sqrt(5) + 1) u (|alpha||x| + |beta||y|) the tests hold this kernel to; a chain of four FMAs per component has no such bound.  The
// kernel moves 48 B per element: the three extra roundings are free.
__device__ __forceinline__ cplx axpby1(cplx alpha, cplx x, cplx beta, cplx y) {
#pragma clang fp contract(off)
    const cplx p = cmake(alpha.x * x.x - alpha.y * x.y, alpha.x * x.y + alpha.y * x.x);
    const cplx r = cmake(beta.x * y.x - beta.y * y.y, beta.x * y.y + beta.y * y.x);
    return cmake(p.x + r.x, p.y + r.y);
}
template <bool BETA0>
__global__ __launch_bounds__(256) void k_axpby(const cplx *__restrict__ X, cplx *__restrict__ Y, long long n, cplx alpha, cplx beta) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        Y[i] = BETA0 ? cmul(alpha, X[i]) : axpby1(alpha, X[i], beta, Y[i]);
}

// Y = beta Y + alpha X over n complex128 values on the device (the ky accumulation of the 2.5-D composite; beta == 0: Y is not read).  Returns when Y is
// complete: the next term of the sum is added on ANOTHER handle's stream.
extern "C" int helm_axpby_device(helm_op *op, double alpha_re, double alpha_im, const void *dX, double beta_re, double beta_im, void *dY, long long n) {
    helm_tuning_refresh();
    if (!op || !dX || !dY || n < 1 || dX == dY) return HELM_ERR_ARG;
    if ((((uintptr_t)dX) | ((uintptr_t)dY)) & 15) return HELM_ERR_ARG;       // (complex128 values are read and written as 16-byte vectors)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)std::min<long long>((n + 255) / 256, AXPBY_BLOCKS));
    const cplx alpha = cmake(alpha_re, alpha_im), beta = cmake(beta_re, beta_im);
    if (beta.x == 0.0 && beta.y == 0.0) HELM_LAUNCH(k_axpby<true>, grid, dim3(256), 0, op->stream, (const cplx *)dX, (cplx *)dY, n, alpha, beta);
    else HELM_LAUNCH(k_axpby<false>, grid, dim3(256), 0, op->stream, (const cplx *)dX, (cplx *)dY, n, alpha, beta);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the complex64 store: pack
// ------------------------------------------------------------------------------------------
constexpr int PACK_MAX_BLOCKS = 1024;      // workgroups per column (<= 4 partial maxima per lane in the second pass)

// the largest of v over the workgroup, in every lane: wave64 butterfly, then the four wave results through LDS.  max is exact and associative, and the
// order is fixed anyway.  Leaves the LDS reusable (ends on a barrier).
__device__ __forceinline__ double block_max(double v, double *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double m = lds[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, lds[w]);
    __syncthreads();
    return m;
}

// e of the store's format (survey_internal.hpp) from the bits of m >= 0 (NaN never arrives: fmax drops it)
__device__ __forceinline__ int column_exponent(double m) {
    if (m == 0.0) return 0;
    const int biased = (int)((__double_as_longlong(m) >> 52) & 0x7ff);       // 0: subnormal (below 2^-1022), 2047: infinity
    return max(-1021, min(1021, biased - 1023));
}

// pass 1: part[s][b] = max over the elements workgroup b takes of column s of max(|Re|, |Im|).  grid (nblk, nsrc): one workgroup row per column.
__global__ __launch_bounds__(256) void k_pack_colmax(const cplx *__restrict__ U, long long ld, double *__restrict__ part) {
    __shared__ double lds[4];
    const cplx *col = U + (long long)blockIdx.y * ld;
    double m = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += (long long)gridDim.x * blockDim.x) {
        const cplx x = col[i];                                           // (one 16-byte load)
        m = fmax(m, fmax(fabs(x.x), fabs(x.y)));
    }
    m = block_max(m, lds);
    if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = m;
}

// pass 2: every workgroup of row s reduces the row's partial maxima (the same values in the same order: the same exponent in all of them), workgroup 0
// records it, and each converts the elements it took in pass 1: 16-byte load, exact scaling, round to nearest, 8-byte store.
__global__ __launch_bounds__(256) void k_pack_c64(const cplx *__restrict__ U, long long ld, const double *__restrict__ part, cplxf32 *__restrict__ out,
                                                  int *__restrict__ exps) {
    __shared__ double lds[4];
    const int s = blockIdx.y;
    double m = 0.0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += blockDim.x) m = fmax(m, part[(long long)s * gridDim.x + b]);
    m = block_max(m, lds);
    const int e = column_exponent(m);
    if (blockIdx.x == 0 && threadIdx.x == 0) exps[s] = e;
    const double sc = pow2(-e);
    const cplx *col = U + (long long)s * ld;
    cplxf32 *o = out + (long long)s * ld;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += (long long)gridDim.x * blockDim.x) {
        const cplx x = col[i];
        o[i] = make_float2((float)(x.x * sc), (float)(x.y * sc));
    }
}

extern "C" int helm_pack_c64_device(helm_op *op, const void *dU, int nsrc, long long ld, void *dOut, void *dExp) {
    helm_tuning_refresh();
    if (!op || !dU || !dOut || !dExp || nsrc < 1 || nsrc > 65535 || ld < 1) return HELM_ERR_ARG;
    if ((((uintptr_t)dU) & 15) || (((uintptr_t)dOut) & 7) || (((uintptr_t)dExp) & 3)) return HELM_ERR_ARG;       // (16-byte loads, 8-byte stores)
    HIP_TRY(op, hipSetDevice(op->device));
    const int nblk = (int)std::min<long long>((ld + 1023) / 1024, PACK_MAX_BLOCKS);
    const size_t pbytes = (size_t)nsrc * nblk * sizeof(double);
    double *part = (double *)helm_pool_alloc(op->device, pbytes);
    if (!part) HELM_FAIL(op, HELM_ERR_DEVICE, "helm_pack_c64_device: no device memory for %zu bytes of partial maxima", pbytes);
    const dim3 grid((unsigned)nblk, (unsigned)nsrc);
    HELM_LAUNCH(k_pack_colmax, grid, dim3(256), 0, op->stream, (const cplx *)dU, ld, part);
    HELM_LAUNCH(k_pack_c64, grid, dim3(256), 0, op->stream, (const cplx *)dU, ld, (const double *)part, (cplxf32 *)dOut, (int *)dExp);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(op->stream);
    helm_pool_free(op->device, part, pbytes);
    HIP_TRY(op, e1);
    HIP_TRY(op, e2);
    return HELM_OK;
}

// ------------------------------------------------------------------------------------------
// the loops over a forward field, one body and one launcher for both formats of the store (FieldC128 / FieldC64, HostField)
// ------------------------------------------------------------------------------------------
// G[i] += scaler[i] * sum_s UF[s][i] * UB[s][i]      (problem.py:152)
template <class F>
__global__ __launch_bounds__(256) void k_imaging(F uf, const cplx *__restrict__ ub, int nsrc, const cplx *__restrict__ scaler, cplx *__restrict__ g, long long N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        cplx acc = cmake(0.0, 0.0);
        for (int s = 0; s < nsrc; ++s) cfma(acc, uf.value(uf.load((long long)s * N + i), s), ub[(long long)s * N + i]);
        cplx gv = g[i];
        cfma(gv, scaler[i], acc);
        g[i] = gv;
    }
}

// The two entry points size their grids differently: the complex128 one keeps the cap of the Krylov vector kernels it was written beside (1024 workgroups, a
// grid-stride loop beyond 2^18 cells), the complex64 one a workgroup per 256 cells up to 2^20.
static int imaging_launch(helm_op *op, HostField UF, const void *dUB, int nsrc, const void *dScaler, void *dG, long long max_blocks) {
    helm_tuning_refresh();
    if (!op || !UF.present() || !dUB || !dScaler || !dG || nsrc < 1) return HELM_ERR_ARG;       // (this pair checks no alignment)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)std::min<long long>((op->N + 255) / 256, max_blocks));
    return UF.with([&](auto F) {
        HELM_LAUNCH(k_imaging<decltype(F)>, grid, dim3(256), 0, op->stream, F, (const cplx *)dUB, nsrc, (const cplx *)dScaler, (cplx *)dG, op->N);
        return launched(op);
    });
}
extern "C" int helm_imaging_accumulate_device(helm_op *op, const void *dUF, const void *dUB, int nsrc, const void *dScaler, void *dG) {
    return imaging_launch(op, HostField::c128(dUF), dUB, nsrc, dScaler, dG, 1024);
}
extern "C" int helm_imaging_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, const void *dUB, int nsrc, const void *dScaler, void *dG) {
    return imaging_launch(op, HostField::packed(dUF32, dExp), dUB, nsrc, dScaler, dG, 1 << 20);
}

// E[i] += alpha (W ? W[i] : 1) sum_s |U[s ld + i]|^2: one lane per cell, the sum over s in the order s = 0, 1, ...  (no atomics: the same bits on every run).
// A pure read stream of nsrc N values against N doubles of read-modify-write: HELM_ENERGY_UNROLL independent loads are issued before the first square,
// which at one 256-lane workgroup per 256 cells and a grid capped at HELM_ENERGY_MAX_BLOCKS keeps 32 KB (complex128) per workgroup in flight.
template <class F>
__global__ __launch_bounds__(256) void k_energy(F U, int nsrc, long long ld, double alpha, const double *__restrict__ W, double *__restrict__ E, long long N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        double acc = 0.0;
        int s = 0;
        for (; s + HELM_ENERGY_UNROLL <= nsrc; s += HELM_ENERGY_UNROLL) {
            typename F::raw x[HELM_ENERGY_UNROLL];
#pragma unroll
            for (int j = 0; j < HELM_ENERGY_UNROLL; ++j) x[j] = U.load((long long)(s + j) * ld + i);
#pragma unroll
            for (int j = 0; j < HELM_ENERGY_UNROLL; ++j) {
                const cplx v = U.value(x[j], s + j);
                acc += v.x * v.x + v.y * v.y;
            }
        }
        for (; s < nsrc; ++s) {
            const cplx v = U.value(U.load((long long)s * ld + i), s);
            acc += v.x * v.x + v.y * v.y;
        }
        const double w = W ? alpha * W[i] : alpha;
        E[i] = E[i] + w * acc;
    }
}
static unsigned energy_blocks(const helm_op *op) { return (unsigned)std::min<long long>((op->N + 255) / 256, HELM_ENERGY_MAX_BLOCKS); }

// E += alpha W sum_s |U_s|^2 (the illumination of HelmBaseProblem.illumination).  Returns when E is complete.
static int energy_launch(helm_op *op, HostField U, int nsrc, long long ld, double alpha, const void *dW, void *dE) {
    helm_tuning_refresh();
    if (!op || !U.ok() || !dE || nsrc < 1 || ld < op->N || !(alpha >= 0.0)) return HELM_ERR_ARG;       // (!(alpha >= 0): negative or NaN)
    if ((((uintptr_t)dE) & 7) || (((uintptr_t)dW) & 7)) return HELM_ERR_ARG;       // (doubles)
    HIP_TRY(op, hipSetDevice(op->device));
    return U.with([&](auto F) {
        HELM_LAUNCH(k_energy<decltype(F)>, dim3(energy_blocks(op)), dim3(256), 0, op->stream, F, nsrc, ld, alpha, (const double *)dW, (double *)dE, op->N);
        return launched(op);
    });
}
extern "C" int helm_energy_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, double alpha, const void *dW, void *dE) {
    return energy_launch(op, HostField::c128(dU), nsrc, ld, alpha, dW, dE);
}
extern "C" int helm_energy_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, double alpha, const void *dW, void *dE) {
    return energy_launch(op, HostField::packed(dU32, dExp), nsrc, ld, alpha, dW, dE);
}

// R[s ldr + i] = conj(W[i] U[s ldu + i]): the right-hand sides of the Born data (HelmBaseProblem.JvecBorn), W = v (.) gradientScaler.  k_energy's pattern:
// one lane per cell in a grid-stride loop over at most HELM_ENERGY_MAX_BLOCKS workgroups, W[i] read once, HELM_ENERGY_UNROLL columns loaded before the first
// product.  A stream of nsrc N reads against nsrc N 16-byte writes.  Each component is two products and one sum (contracted or not: at most three roundings of
// terms bounded by |Re W||Re u| + |Im W||Im u|, cross terms for the imaginary part); the conjugation is exact.  No atomics: the same bits on every run.
template <class F>
__global__ __launch_bounds__(256) void k_virtual_sources(F U, int nsrc, long long ldu, const cplx *__restrict__ W, cplx *__restrict__ R, long long ldr, long long N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const cplx w = W[i];
        int s = 0;
        for (; s + HELM_ENERGY_UNROLL <= nsrc; s += HELM_ENERGY_UNROLL) {
            typename F::raw x[HELM_ENERGY_UNROLL];
#pragma unroll
            for (int j = 0; j < HELM_ENERGY_UNROLL; ++j) x[j] = U.load((long long)(s + j) * ldu + i);
#pragma unroll
            for (int j = 0; j < HELM_ENERGY_UNROLL; ++j) R[(long long)(s + j) * ldr + i] = cconj(cmul(w, U.value(x[j], s + j)));
        }
        for (; s < nsrc; ++s) R[(long long)s * ldr + i] = cconj(cmul(w, U.value(U.load((long long)s * ldu + i), s)));
    }
}

// R[s][i] = conj(W[i] U[s][i]) for s < nsrc, i < N (the handle's grid): U [nsrc][ldu] complex128, W N complex128, R [nsrc][ldr] complex128, ldu, ldr >= N.  R must
// not overlap U or W.  Returns when R is complete.
static int virtual_sources_launch(helm_op *op, HostField U, int nsrc, long long ldu, const void *dW, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (!op || !U.ok() || !dW || !dR || nsrc < 1 || ldu < op->N || ldr < op->N || U.u == dR || dW == dR) return HELM_ERR_ARG;
    if ((((uintptr_t)dW) | ((uintptr_t)dR)) & 15) return HELM_ERR_ARG;       // (16-byte loads and stores)
    HIP_TRY(op, hipSetDevice(op->device));
    return U.with([&](auto F) {
        HELM_LAUNCH(k_virtual_sources<decltype(F)>, dim3(energy_blocks(op)), dim3(256), 0, op->stream, F, nsrc, ldu, (const cplx *)dW, (cplx *)dR, ldr, op->N);
        return launched(op);
    });
}
extern "C" int helm_virtual_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, void *dR, long long ldr) {
    return virtual_sources_launch(op, HostField::c128(dU), nsrc, ldu, dW, dR, ldr);
}
extern "C" int helm_virtual_sources_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dW, void *dR, long long ldr) {
    return virtual_sources_launch(op, HostField::packed(dU32, dExp), nsrc, ldu, dW, dR, ldr);
}

// receiver sampling: sum_k val[k] U[s][col[k]] over the entries k of sparse row r + s * row_stride (one thread per (r, s), fixed order).
// row_stride = 0: one receiver array for every source; row_stride >= nrec: source s has rows [s * row_stride, s * row_stride + nrec) of its own (an array
// that moves with the source, the per-source matrices stacked into one CSR).  ACC = false: out[r][s] = the sum, alpha / beta / beta0 unused (no product
// with one: an infinite sample stays infinite).  ACC = true: out[r][s] = beta out[r][s] + alpha sum (the ky sum of a 2.5-D survey's data: sampling is
// linear, so the summed wavefields are never formed); beta0: out is write-only -- an uninitialised accumulator is legal for the first term.
template <class F, bool ACC>
__global__ __launch_bounds__(256) void k_sample(F U, int nsrc, long long ld, const long long *__restrict__ rowptr, const long long *__restrict__ col,
                                                const cplx *__restrict__ val, int nrec, long long row_stride, cplx alpha, cplx beta, int beta0,
                                                cplx *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nrec * nsrc) return;
    const int r = (int)(t / nsrc), sidx = (int)(t % nsrc);
    const long long row = r + sidx * row_stride;
    cplx acc = cmake(0.0, 0.0);
    for (long long k = rowptr[row]; k < rowptr[row + 1]; ++k) cfma(acc, val[k], U.value(U.load((long long)sidx * ld + col[k]), sidx));
    if (ACC) {
        cplx o = cmul(alpha, acc);
        if (!beta0) cfma(o, beta, out[t]);
        out[t] = o;
    } else out[t] = acc;
}
template <class F, bool ACC>
static int launch_sample(helm_op *op, F U, int nsrc, long long ld, const void *d_rowptr, const void *d_col, const void *d_val, int nrec, long long row_stride,
                         cplx alpha, cplx beta, void *d_out) {
    const long long tot = (long long)nrec * nsrc;
    const int beta0 = (beta.x == 0.0 && beta.y == 0.0) ? 1 : 0;
    HELM_LAUNCH((k_sample<F, ACC>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, op->stream, U, nsrc, ld, (const long long *)d_rowptr,
                (const long long *)d_col, (const cplx *)d_val, nrec, row_stride, alpha, beta, beta0, (cplx *)d_out);
    return launched(op);
}

extern "C" int helm_sample_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col, const void *d_val, int nrec, void *d_out) {
    helm_tuning_refresh();
    if (!op || !dU || !d_rowptr || !d_col || !d_val || !d_out || nsrc < 1 || nrec < 1) return HELM_ERR_ARG;       // (ld is not checked here; the accumulating ones do)
    HIP_TRY(op, hipSetDevice(op->device));
    return launch_sample<FieldC128, false>(op, FieldC128{(const cplx *)dU}, nsrc, ld, d_rowptr, d_col, d_val, nrec, 0, cmake(0.0, 0.0), cmake(0.0, 0.0), d_out);
}

// out = beta out + alpha R u: helm_sample_device into an accumulator (the ky sum of 2.5-D data; beta == 0: out is not read)
static int sample_rows_launch(helm_op *op, HostField U, int nsrc, long long ld, const void *d_rowptr, const void *d_col, const void *d_val, int nrec,
                              long long row_stride, cplx alpha, cplx beta, void *d_out) {
    helm_tuning_refresh();
    if (!op || !U.present() || !d_rowptr || !d_col || !d_val || !d_out || nsrc < 1 || nrec < 1 || ld < 1) return HELM_ERR_ARG;       // (no alignment is checked)
    if (row_stride != 0 && row_stride < nrec) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    return U.with([&](auto F) { return launch_sample<decltype(F), true>(op, F, nsrc, ld, d_rowptr, d_col, d_val, nrec, row_stride, alpha, beta, d_out); });
}
extern "C" int helm_sample_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col, const void *d_val, int nrec,
                                             double alpha_re, double alpha_im, double beta_re, double beta_im, void *d_out) {
    return sample_rows_launch(op, HostField::c128(dU), nsrc, ld, d_rowptr, d_col, d_val, nrec, 0, cmake(alpha_re, alpha_im), cmake(beta_re, beta_im), d_out);
}

// helm_sample_accumulate_device with a row stride per source: source s samples CSR row r + s * row_stride (0: one array for all sources; >= nrec: the
// per-source matrices of an array that moves with the source, stacked into one CSR of nsrc * row_stride rows)
extern "C" int helm_sample_rows_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col, const void *d_val, int nrec,
                                       long long row_stride, double alpha_re, double alpha_im, double beta_re, double beta_im, void *d_out) {
    return sample_rows_launch(op, HostField::c128(dU), nsrc, ld, d_rowptr, d_col, d_val, nrec, row_stride, cmake(alpha_re, alpha_im), cmake(beta_re, beta_im), d_out);
}
extern "C" int helm_sample_rows_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, const void *d_rowptr, const void *d_col,
                                           const void *d_val, int nrec, long long row_stride, double alpha_re, double alpha_im, double beta_re, double beta_im,
                                           void *d_out) {
    return sample_rows_launch(op, HostField::packed(dU32, dExp), nsrc, ld, d_rowptr, d_col, d_val, nrec, row_stride, cmake(alpha_re, alpha_im),
                              cmake(beta_re, beta_im), d_out);
}
