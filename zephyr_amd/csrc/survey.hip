// What a survey runs on the device besides the solves: right-hand sides from sparse sources and from residual samples, receiver sampling, the imaging
// condition, illumination (energy), axpby, the optional complex64 store of forward wavefields, the mass stencil of the exact Frechet derivative fused into
// the virtual sources and the imaging sum, the exact density derivative: the buoyancy map, its stencil on stored columns, the nine lag products and its
// transpose, the planes of the total velocity derivative and their transpose, the pseudo-Hessian diagonal of these derivatives, and (last section) the exact
// diagonal of the Gauss-Newton Hessian: the autocorrelation planes of a set of columns and the per-cell trace.  Each kernel stands beside the C entry point that
// launches it.
//
// The complex64 store (zephyr_amd/fieldstore.py, config key fieldsDtype='complex64'): a wavefield column s is kept as
// complex64 values x * 2^-e_s with ONE power-of-two scale per column, e_s the binary exponent of the column's largest component
// (2^e_s <= max_i max(|Re|, |Im|) < 2^(e_s+1), clamped to +-1021; 0 for a zero column).  The scaling is exact, so the only rounding is the conversion to
// fp32 (2^-24 relative where the scaled value is a normal fp32 number), and fields of any magnitude survive where a plain conversion would overflow or
// flush.  A consumer reads (double)x^ * 2^e_s, exact again.  The imaging, energy and sampling loops exist once, as templates over the reader of the
// forward field (FieldC128 / FieldC64 below): the complex64 entry points give the complex128 sum of the unpacked field term for term because it is the
// same loop.
#include "helm_internal.hpp"
#include "mz_row.hpp"
#include <algorithm>
#include <utility>

// what every entry point here ends on: the launch error, then the stream drained (the result is complete when the call returns)
static int launched(helm_op *op) {
    HIP_TRY(op, hipGetLastError());
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}

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
typedef float2 cplxf32;      // what the store holds: 8 bytes per value

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

// e of the header comment from the bits of m >= 0 (NaN never arrives: fmax drops it)
__device__ __forceinline__ int column_exponent(double m) {
    if (m == 0.0) return 0;
    const int biased = (int)((__double_as_longlong(m) >> 52) & 0x7ff);       // 0: subnormal (below 2^-1022), 2047: infinity
    return max(-1021, min(1021, biased - 1023));
}
__device__ __forceinline__ double pow2(int e) { return __longlong_as_double((long long)(e + 1023) << 52); }      // |e| <= 1021: a normal number

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
// the loops over a forward field, one body for both formats of the store
// ------------------------------------------------------------------------------------------
// How a kernel reads the field, passed by value: load(i) is the raw 16- or 8-byte load of element i, value(x, s) what a loaded element of column s stands
// for.  The two are separate so that a kernel can issue several loads before the first use.
struct FieldC128 {
    typedef cplx raw;
    const cplx *__restrict__ u;
    __device__ __forceinline__ raw load(long long i) const { return u[i]; }
    __device__ __forceinline__ cplx value(raw x, int) const { return x; }
    // value() in two steps, for a loop that reads one column many times: scale(s) once, scaled(x, scale) per element
    __device__ __forceinline__ double scale(int) const { return 1.0; }
    __device__ __forceinline__ cplx scaled(raw x, double) const { return x; }
};
struct FieldC64 {
    typedef cplxf32 raw;
    const cplxf32 *__restrict__ u;
    const int *__restrict__ exps;
    __device__ __forceinline__ raw load(long long i) const { return u[i]; }
    // each component is scaled in fp64 (exact: 2^(2 e_s) alone would overflow where the field does not)
    __device__ __forceinline__ cplx value(raw x, int s) const { const double sc = pow2(exps[s]); return cmake((double)x.x * sc, (double)x.y * sc); }
    __device__ __forceinline__ double scale(int s) const { return pow2(exps[s]); }
    __device__ __forceinline__ cplx scaled(raw x, double sc) const { return cmake((double)x.x * sc, (double)x.y * sc); }
};

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
extern "C" int helm_imaging_accumulate_device(helm_op *op, const void *dUF, const void *dUB, int nsrc, const void *dScaler, void *dG) {
    helm_tuning_refresh();
    if (!op || !dUF || !dUB || !dScaler || !dG || nsrc < 1) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const unsigned blocks = (unsigned)std::min<long long>((op->N + 255) / 256, 1024);
    HELM_LAUNCH(k_imaging<FieldC128>, dim3(blocks), dim3(256), 0, op->stream, FieldC128{(const cplx *)dUF}, (const cplx *)dUB, nsrc, (const cplx *)dScaler,
                (cplx *)dG, op->N);
    return launched(op);
}

extern "C" int helm_imaging_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, const void *dUB, int nsrc, const void *dScaler, void *dG) {
    helm_tuning_refresh();
    if (!op || !dUF32 || !dExp || !dUB || !dScaler || !dG || nsrc < 1) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const unsigned blocks = (unsigned)std::min<long long>((op->N + 255) / 256, 1 << 20);
    HELM_LAUNCH(k_imaging<FieldC64>, dim3(blocks), dim3(256), 0, op->stream, FieldC64{(const cplxf32 *)dUF32, (const int *)dExp}, (const cplx *)dUB, nsrc,
                (const cplx *)dScaler, (cplx *)dG, op->N);
    return launched(op);
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
extern "C" int helm_energy_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, double alpha, const void *dW, void *dE) {
    helm_tuning_refresh();
    if (!op || !dU || !dE || nsrc < 1 || ld < op->N || !(alpha >= 0.0)) return HELM_ERR_ARG;       // (!(alpha >= 0): negative or NaN)
    if ((((uintptr_t)dU) & 15) || (((uintptr_t)dE) & 7) || (((uintptr_t)dW) & 7)) return HELM_ERR_ARG;       // (16-byte loads of U; doubles)
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_energy<FieldC128>, dim3(energy_blocks(op)), dim3(256), 0, op->stream, FieldC128{(const cplx *)dU}, nsrc, ld, alpha, (const double *)dW,
                (double *)dE, op->N);
    return launched(op);
}

extern "C" int helm_energy_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, double alpha, const void *dW, void *dE) {
    helm_tuning_refresh();
    if (!op || !dU32 || !dExp || !dE || nsrc < 1 || ld < op->N || !(alpha >= 0.0)) return HELM_ERR_ARG;       // (!(alpha >= 0): negative or NaN)
    if ((((uintptr_t)dU32) & 7) || (((uintptr_t)dExp) & 3) || (((uintptr_t)dE) & 7) || (((uintptr_t)dW) & 7)) return HELM_ERR_ARG;       // (8-byte loads of U32; doubles)
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_energy<FieldC64>, dim3(energy_blocks(op)), dim3(256), 0, op->stream, FieldC64{(const cplxf32 *)dU32, (const int *)dExp}, nsrc, ld, alpha,
                (const double *)dW, (double *)dE, op->N);
    return launched(op);
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
extern "C" int helm_virtual_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (!op || !dU || !dW || !dR || nsrc < 1 || ldu < op->N || ldr < op->N || dU == dR || dW == dR) return HELM_ERR_ARG;
    if ((((uintptr_t)dU) | ((uintptr_t)dW) | ((uintptr_t)dR)) & 15) return HELM_ERR_ARG;       // (16-byte loads and stores)
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_virtual_sources<FieldC128>, dim3(energy_blocks(op)), dim3(256), 0, op->stream, FieldC128{(const cplx *)dU}, nsrc, ldu, (const cplx *)dW, (cplx *)dR, ldr, op->N);
    return launched(op);
}

extern "C" int helm_virtual_sources_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dW, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (!op || !dU32 || !dExp || !dW || !dR || nsrc < 1 || ldu < op->N || ldr < op->N || dU32 == dR || dW == dR) return HELM_ERR_ARG;
    if ((((uintptr_t)dU32) & 7) || (((uintptr_t)dExp) & 3) || ((((uintptr_t)dW) | ((uintptr_t)dR)) & 15)) return HELM_ERR_ARG;       // (8-byte loads of U32)
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_virtual_sources<FieldC64>, dim3(energy_blocks(op)), dim3(256), 0, op->stream, FieldC64{(const cplxf32 *)dU32, (const int *)dExp}, nsrc, ldu, (const cplx *)dW,
                (cplx *)dR, ldr, op->N);
    return launched(op);
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
    if (!op || !dU || !d_rowptr || !d_col || !d_val || !d_out || nsrc < 1 || nrec < 1) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    return launch_sample<FieldC128, false>(op, FieldC128{(const cplx *)dU}, nsrc, ld, d_rowptr, d_col, d_val, nrec, 0, cmake(0.0, 0.0), cmake(0.0, 0.0), d_out);
}

// out = beta out + alpha R u: helm_sample_device into an accumulator (the ky sum of 2.5-D data; beta == 0: out is not read)
extern "C" int helm_sample_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col, const void *d_val, int nrec,
                                             double alpha_re, double alpha_im, double beta_re, double beta_im, void *d_out) {
    helm_tuning_refresh();
    if (!op || !dU || !d_rowptr || !d_col || !d_val || !d_out || nsrc < 1 || nrec < 1 || ld < 1) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    return launch_sample<FieldC128, true>(op, FieldC128{(const cplx *)dU}, nsrc, ld, d_rowptr, d_col, d_val, nrec, 0, cmake(alpha_re, alpha_im),
                                          cmake(beta_re, beta_im), d_out);
}

// helm_sample_accumulate_device with a row stride per source: source s samples CSR row r + s * row_stride (0: one array for all sources; >= nrec: the
// per-source matrices of an array that moves with the source, stacked into one CSR of nsrc * row_stride rows)
extern "C" int helm_sample_rows_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col, const void *d_val, int nrec,
                                       long long row_stride, double alpha_re, double alpha_im, double beta_re, double beta_im, void *d_out) {
    helm_tuning_refresh();
    if (!op || !dU || !d_rowptr || !d_col || !d_val || !d_out || nsrc < 1 || nrec < 1 || ld < 1) return HELM_ERR_ARG;
    if (row_stride != 0 && row_stride < nrec) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    return launch_sample<FieldC128, true>(op, FieldC128{(const cplx *)dU}, nsrc, ld, d_rowptr, d_col, d_val, nrec, row_stride, cmake(alpha_re, alpha_im),
                                          cmake(beta_re, beta_im), d_out);
}

extern "C" int helm_sample_rows_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, const void *d_rowptr, const void *d_col,
                                           const void *d_val, int nrec, long long row_stride, double alpha_re, double alpha_im, double beta_re, double beta_im,
                                           void *d_out) {
    helm_tuning_refresh();
    if (!op || !dU32 || !dExp || !d_rowptr || !d_col || !d_val || !d_out || nsrc < 1 || nrec < 1 || ld < 1) return HELM_ERR_ARG;
    if (row_stride != 0 && row_stride < nrec) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    return launch_sample<FieldC64, true>(op, FieldC64{(const cplxf32 *)dU32, (const int *)dExp}, nsrc, ld, d_rowptr, d_col, d_val, nrec, row_stride,
                                         cmake(alpha_re, alpha_im), cmake(beta_re, beta_im), d_out);
}

// ------------------------------------------------------------------------------------------
// the exact Frechet derivative of MiniZephyr: the mass stencil fused into the virtual sources and into the imaging sum
// ------------------------------------------------------------------------------------------
// MiniZephyr carries the velocity as K = (omega_d^2 / c^2 - ky^2) / rho of the NEIGHBOURING cell, spread over the nine slots of a row by the mass weights
// (assemble.hip: centre cc, edges dc, corners ec), and its four boundary lines are +-identity rows.  So (dA) u = mask_int (.) M0(dK (.) u): M0 the constant
// 9-point stencil of those weights (cells outside the grid contribute nothing), mask_int zero on the boundary lines.  HelmBaseProblem.JvecBorn /
// Jtvec(linearisation='operator') need M0 applied to k columns on the way to the solver (k_virtual_sources_op) and, transposed -- M0^T mask_int = M0 mask_int,
// the weights are symmetric -- to the back-propagated columns inside the imaging sum (k_imaging_op).
//
// Both kernels walk the grid the same way.  A wave takes a tile of OP_TILE_X output cells along x, one lane per cell, plus one halo lane at either end (lanes 0 and
// 63 load and never store), and OP_ROWS output rows, which it walks down with a rolling window of three rows per column held in registers: per row and column
// the value t of the lane's own cell and h = t(x - 1) + t(x + 1), fetched from the neighbouring lanes (no LDS, no barrier: waves run independently).  Row z is
//     mc t(z) + md ((t(z-1) + t(z+1)) + h(z)) + me (h(z-1) + h(z+1))
// OP_UNROLL columns are walked together, and the loads of the next row are issued before the arithmetic of the current one.  A field element is loaded once per
// kernel except for the halo: one lane in 32 and two rows in OP_ROWS + 2 are loaded by two waves (neighbours in the grid, hence in flight together).
// The order of every sum is fixed by the code: the same bits on every run.
constexpr double MZ_MC = 0.6248, MZ_MD = 0.09381, MZ_ME = 0.000001297;      // (assemble.hip cc, dc, ec)
constexpr int OP_TILE_X = 62;       // output cells per wave along x
constexpr int OP_ROWS = 32;         // output rows per wave
constexpr int OP_UNROLL = 4;        // columns walked together

struct MassRow { cplx t, h; };

// t(x - 1) + t(x + 1) from the neighbouring lanes.  Lane 0 and lane 63 get their own value for the missing neighbour: they are halo lanes, whose h is never used.
__device__ __forceinline__ cplx lane_neighbours(cplx t) {
    const double lx = __shfl_up(t.x, 1, 64), ly = __shfl_up(t.y, 1, 64), rx = __shfl_down(t.x, 1, 64), ry = __shfl_down(t.y, 1, 64);
    return cmake(lx + rx, ly + ry);
}
__device__ __forceinline__ cplx mass_row(const MassRow &up, const MassRow &mid, const MassRow &dn) {
    const cplx e = cmake((up.t.x + dn.t.x) + mid.h.x, (up.t.y + dn.t.y) + mid.h.y);
    const cplx c = cmake(up.h.x + dn.h.x, up.h.y + dn.h.y);
    return cmake(MZ_MC * mid.t.x + MZ_MD * e.x + MZ_ME * c.x, MZ_MC * mid.t.y + MZ_MD * e.y + MZ_ME * c.y);
}

// where a wave works: its tile and rows from the flat job index (x tiles fastest), its lane's cell
struct OpJob {
    int x, z0, z1; bool live, xin, store;
    __device__ __forceinline__ OpJob(int nz, int nx) {
        const int lane = threadIdx.x & 63;
        const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X, nzc = (nz + OP_ROWS - 1) / OP_ROWS;
        const long long job = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        live = job < (long long)ntx * nzc;
        const int tile = live ? (int)(job % ntx) : 0, chunk = live ? (int)(job / ntx) : 0;
        x = tile * OP_TILE_X + lane - 1;
        z0 = chunk * OP_ROWS;
        z1 = min(z0 + OP_ROWS, nz);
        xin = x >= 0 && x < nx;
        store = lane >= 1 && lane <= OP_TILE_X && x < nx;
    }
};
static dim3 op_grid(const helm_op *op, int groups) {
    const long long jobs = (long long)((op->nx + OP_TILE_X - 1) / OP_TILE_X) * ((op->nz + OP_ROWS - 1) / OP_ROWS);
    return dim3((unsigned)((jobs + 3) / 4), (unsigned)groups);
}

// R[s ldr + i] = coef mask_int[i] M0(W (.) (CONJ ? conj(U[s]) : U[s]))[i] for the nsrc columns, i over the nz x nx grid.  grid.y: groups of OP_UNROLL columns.
// Per cell and column 16 (8: complex64 store) bytes read and 16 written; W is read once per group of columns (16 B per cell against 4 x 32).
template <class F, bool CONJ>
__global__ __launch_bounds__(256) void k_virtual_sources_op(F U, int nsrc, long long ldu, const cplx *__restrict__ W, cplx coef, cplx *__restrict__ R, long long ldr,
                                                            int nz, int nx) {
    const OpJob job(nz, nx);
    if (!job.live) return;                                  // (a whole wave: the lane exchanges below stay complete)
    const int s0 = blockIdx.y * OP_UNROLL, ncol = min(OP_UNROLL, nsrc - s0);
    const int x = job.x;
    typename F::raw raw[OP_UNROLL];
    cplx w;
    MassRow up[OP_UNROLL], mid[OP_UNROLL], dn[OP_UNROLL];
    double sc[OP_UNROLL];                                   // (the columns' scales, read once: not a dependent load per row)
#pragma unroll
    for (int j = 0; j < OP_UNROLL; ++j) sc[j] = U.scale(s0 + min(j, ncol - 1));

    // the loads of row z (nothing outside the grid); the products and the neighbour exchange of what was loaded
    auto fetch = [&](int z) {
        const bool in = job.xin && z >= 0 && z < nz;
        const long long i = (long long)z * nx + x;
        w = in ? W[i] : cmake(0.0, 0.0);
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) raw[j] = (in && j < ncol) ? U.load((long long)(s0 + j) * ldu + i) : typename F::raw{};
    };
    auto make = [&](MassRow *row) {
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) {
            cplx u = U.scaled(raw[j], sc[j]);
            if (CONJ) u = cconj(u);
            row[j].t = cmul(w, u);
            row[j].h = lane_neighbours(row[j].t);
        }
    };
    fetch(job.z0 - 1); make(up);
    fetch(job.z0); make(mid);
    fetch(job.z0 + 1);
    for (int z = job.z0; z < job.z1; ++z) {
        make(dn);
        if (z + 1 < job.z1) fetch(z + 2);                  // (wave-uniform)
        const bool inside = z >= 1 && z <= nz - 2 && x >= 1 && x <= nx - 2;
        if (job.store) {
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j)
                if (j < ncol) R[(long long)(s0 + j) * ldr + i] = inside ? cmul(coef, mass_row(up[j], mid[j], dn[j])) : cmake(0.0, 0.0);
        }
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) { up[j] = mid[j]; mid[j] = dn[j]; }
    }
}

static int virtual_sources_op_args(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, void *dR, long long ldr) {
    if (!op || !dU || !dW || !dR || nsrc < 1 || nsrc > 65535 * OP_UNROLL || ldu < op->N || ldr < op->N || dU == dR || dW == dR) return HELM_ERR_ARG;
    if (op->variant != HELM_MINIZEPHYR || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the mass stencil of the exact derivative is that of the 2-D MiniZephyr operator");
    return HELM_OK;
}

// R[s][i] = coef mask_int[i] M0(W (.) U[s])[i] (conj != 0: M0(W (.) conj(U[s]))) for s < nsrc, i < N (the handle's nz x nx grid): U [nsrc][ldu] complex128, W N
// complex128, R [nsrc][ldr] complex128, ldu, ldr >= N.  R must not overlap U or W.  Returns when R is complete.
extern "C" int helm_virtual_sources_op_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im, int conj,
                                              void *dR, long long ldr) {
    helm_tuning_refresh();
    if (int rc = virtual_sources_op_args(op, dU, nsrc, ldu, dW, dR, ldr)) return rc;
    if ((((uintptr_t)dU) | ((uintptr_t)dW) | ((uintptr_t)dR)) & 15) return HELM_ERR_ARG;       // (16-byte loads and stores)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid = op_grid(op, (nsrc + OP_UNROLL - 1) / OP_UNROLL);
    const FieldC128 U{(const cplx *)dU};
    if (conj) HELM_LAUNCH((k_virtual_sources_op<FieldC128, true>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dW, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    else HELM_LAUNCH((k_virtual_sources_op<FieldC128, false>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dW, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    return launched(op);
}

extern "C" int helm_virtual_sources_op_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im,
                                                  int conj, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (int rc = virtual_sources_op_args(op, dU32, nsrc, ldu, dW, dR, ldr)) return rc;
    if (!dExp || (((uintptr_t)dU32) & 7) || (((uintptr_t)dExp) & 3) || ((((uintptr_t)dW) | ((uintptr_t)dR)) & 15)) return HELM_ERR_ARG;       // (8-byte loads of U32)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid = op_grid(op, (nsrc + OP_UNROLL - 1) / OP_UNROLL);
    const FieldC64 U{(const cplxf32 *)dU32, (const int *)dExp};
    if (conj) HELM_LAUNCH((k_virtual_sources_op<FieldC64, true>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dW, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    else HELM_LAUNCH((k_virtual_sources_op<FieldC64, false>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dW, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    return launched(op);
}

// G[i] += W[i] sum_s UF[s ldf + i] M0(mask_int (.) UB[s])[i]: the stencil on the back-propagated field inside the imaging sum, no intermediate array.  A workgroup
// of IMG_WAVES waves owns a tile of OP_TILE_X x IMG_ROWS cells of G.  The columns go to its waves in groups of OP_UNROLL, group g to wave g mod IMG_WAVES; a wave walks
// the tile's rows once per group (the walk of the header comment) and keeps its sum per cell in an LDS slice of its own.  After one barrier wave r adds the slices
// of row r in wave order and then W (.) sum to G: one writer per cell and a fixed order, so no atomics and the same bits on every run.
// Per cell and column 16 (8: complex64 store) bytes of UF and 16 of UB, the latter times (1 + 2 / IMG_ROWS) (1 + 2 / OP_TILE_X) for the halo; W and G once per cell.
// Rows are short because the columns of a tile are spread over the waves of ONE workgroup: with a wave per 32 rows and every column, 512^2 cells gave 144 waves
// to 1024 SIMDs and the kernel ran at 0.7 TB/s.
constexpr int IMG_ROWS = 8;         // output rows per workgroup
constexpr int IMG_WAVES = 8;        // waves per workgroup: 64 KB of LDS
static_assert(IMG_ROWS <= IMG_WAVES, "wave r finishes row r");

template <class F>
__global__ __launch_bounds__(64 * IMG_WAVES) void k_imaging_op(F UF, long long ldf, const cplx *__restrict__ UB, long long ldb, int nsrc, const cplx *__restrict__ W,
                                                               cplx *__restrict__ G, int nz, int nx) {
    __shared__ cplx part[IMG_WAVES][IMG_ROWS][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * OP_TILE_X + lane - 1, z0 = (int)(blockIdx.x / ntx) * IMG_ROWS;
    const bool store = lane >= 1 && lane <= OP_TILE_X && x < nx;
    cplx rawb[OP_UNROLL];
    MassRow up[OP_UNROLL], mid[OP_UNROLL], dn[OP_UNROLL];
    const int ngroups = (nsrc + OP_UNROLL - 1) / OP_UNROLL;
    for (int g = wave; g < ngroups; g += IMG_WAVES) {          // (wave-uniform: the lane exchanges stay complete)
        const int s0 = g * OP_UNROLL, ncol = min(OP_UNROLL, nsrc - s0);
        double sc[OP_UNROLL];                               // (the columns' scales, read once per group: not a dependent load per row)
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) sc[j] = UF.scale(s0 + min(j, ncol - 1));
        // the loads of row z of UB with mask_int applied: nothing outside the grid, nothing from its boundary lines
        auto fetch = [&](int z) {
            const bool in = z >= 1 && z <= nz - 2 && x >= 1 && x <= nx - 2;
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j) rawb[j] = (in && j < ncol) ? UB[(long long)(s0 + j) * ldb + i] : cmake(0.0, 0.0);
        };
        auto make = [&](MassRow *row) {
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j) { row[j].t = rawb[j]; row[j].h = lane_neighbours(rawb[j]); }
        };
        fetch(z0 - 1); make(up);
        fetch(z0); make(mid);
        fetch(z0 + 1);
#pragma unroll 1
        for (int r = 0; r < IMG_ROWS; ++r) {
            const int z = z0 + r;
            make(dn);
            if (r + 1 < IMG_ROWS) fetch(z + 2);
            cplx acc = cmake(0.0, 0.0);
            if (store && z < nz) {
                const long long i = (long long)z * nx + x;
                typename F::raw rawf[OP_UNROLL];
#pragma unroll
                for (int j = 0; j < OP_UNROLL; ++j) rawf[j] = j < ncol ? UF.load((long long)(s0 + j) * ldf + i) : typename F::raw{};
#pragma unroll
                for (int j = 0; j < OP_UNROLL; ++j)
                    if (j < ncol) cfma(acc, UF.scaled(rawf[j], sc[j]), mass_row(up[j], mid[j], dn[j]));
            }
            part[wave][r][lane] = g == wave ? acc : cadd(part[wave][r][lane], acc);      // (the wave's own slice: no other wave touches it before the barrier)
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j) { up[j] = mid[j]; mid[j] = dn[j]; }
        }
    }
    __syncthreads();
    if (wave < IMG_ROWS && store && z0 + wave < nz) {
        cplx sum = part[0][wave][lane];                          // (nsrc >= 1: wave 0 has a group)
        for (int w = 1; w < min(IMG_WAVES, ngroups); ++w) sum = cadd(sum, part[w][wave][lane]);
        const long long i = (long long)(z0 + wave) * nx + x;
        cplx gv = G[i];
        cfma(gv, W[i], sum);
        G[i] = gv;
    }
}
static dim3 imaging_op_grid(const helm_op *op) {
    return dim3((unsigned)(((op->nx + OP_TILE_X - 1) / OP_TILE_X) * ((op->nz + IMG_ROWS - 1) / IMG_ROWS)));
}

static int imaging_op_args(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, const void *dW, void *dG) {
    if (!op || !dUF || !dUB || !dW || !dG || nsrc < 1 || ldf < op->N || ldb < op->N || dUF == dG || dUB == dG || dW == dG) return HELM_ERR_ARG;
    if (op->variant != HELM_MINIZEPHYR || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the mass stencil of the exact derivative is that of the 2-D MiniZephyr operator");
    return HELM_OK;
}

// G[i] += W[i] sum_s UF[s][i] M0(mask_int (.) UB[s])[i] for i < N: UF [nsrc][ldf], UB [nsrc][ldb], W and G N complex128.  G must not overlap the others.  Returns when G
// is complete.
extern "C" int helm_imaging_op_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, const void *dW, void *dG) {
    helm_tuning_refresh();
    if (int rc = imaging_op_args(op, dUF, ldf, dUB, ldb, nsrc, dW, dG)) return rc;
    if ((((uintptr_t)dUF) | ((uintptr_t)dUB) | ((uintptr_t)dW) | ((uintptr_t)dG)) & 15) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_imaging_op<FieldC128>, imaging_op_grid(op), dim3(64 * IMG_WAVES), 0, op->stream, FieldC128{(const cplx *)dUF}, ldf, (const cplx *)dUB, ldb, nsrc, (const cplx *)dW,
                (cplx *)dG, op->nz, op->nx);
    return launched(op);
}

extern "C" int helm_imaging_op_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc,
                                                     const void *dW, void *dG) {
    helm_tuning_refresh();
    if (int rc = imaging_op_args(op, dUF32, ldf, dUB, ldb, nsrc, dW, dG)) return rc;
    if (!dExp || (((uintptr_t)dUF32) & 7) || (((uintptr_t)dExp) & 3) || ((((uintptr_t)dUB) | ((uintptr_t)dW) | ((uintptr_t)dG)) & 15)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_imaging_op<FieldC64>, imaging_op_grid(op), dim3(64 * IMG_WAVES), 0, op->stream, FieldC64{(const cplxf32 *)dUF32, (const int *)dExp}, ldf, (const cplx *)dUB, ldb, nsrc,
                (const cplx *)dW, (cplx *)dG, op->nz, op->nx);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the exact density derivative of MiniZephyr: the buoyancy map L, its stencil on stored columns, the nine lag products and L^T
// ------------------------------------------------------------------------------------------
// Every interior row of MiniZephyr is a linear, homogeneous function of the buoyancy field b = 1 / rho (mz_row.hpp mz_star: the mass terms carry
// kappa b of the neighbouring cell, kappa = omega_d^2 / c^2 - ky^2; every stiffness term is a row factor -- X, Z, px, pz of the row's own cell, which depend
// on c and the PML only -- times an average (b_i + b_(i+o)) / 2), and the four boundary lines are +-identity.  So the derivative of A along a perturbation
// db of the buoyancy is the nine planes dC = L[db], the assembly's own formulas evaluated on db with the boundary rows zero, and
//     (dA) u = sum_k dC_k (.) shift_k(u)                                  (k_buoyancy_planes, then k_stencil_sources on the stored columns)
//     sum_s z_s^T (dA) u_s = sum_k sum_i dC_k[i] P_k[i],   P_k[i] = sum_s z_s[i] u_s[i + off_k]     (k_lag_imaging: nine model-sized planes)
//     g_b = L^T P                                                         (k_buoyancy_adjoint: a gather over the 3 x 3 rows around a cell)
// HelmBaseProblem.JvecBorn / Jtvec(linearisation='operator', parameter='rho') put these together (device_survey.py); db = -v / rho^2 and g_rho = -g_b / rho^2
// are the caller's.  Planes are [9][N] with the slot order of the operator, k = 3 (dz + 1) + (dx + 1).

static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}
static int mz_handle_args(helm_op *op, const char *what) {
    if (op->variant != HELM_MINIZEPHYR || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "%s: the density and velocity derivatives are those of the 2-D MiniZephyr operator", what);
    return HELM_OK;
}

__device__ __forceinline__ MzRow mz_row_at(const MzParams &P, const cplx *__restrict__ c, int iz, int ix) {
    double dX, sX, dZ, sZ;
    mz_profile_at(P.nx, P.npml, P.dx, P.fs3, P.fs1, ix, dX, sX);
    mz_profile_at(P.nz, P.npml, P.dz, P.fs0, P.fs2, iz, dZ, sZ);
    return mz_row_factors(P, c[(long long)iz * P.nx + ix], dX, sX, dZ, sZ);
}

// dC = L[db]: one lane per cell, the assembly's star (mz_star) on the perturbation.  An interior row reads only cells inside the grid, so there is no padding.
__global__ __launch_bounds__(256) void k_buoyancy_planes(MzParams P, const cplx *__restrict__ c, const double *__restrict__ db, cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);
    cplx out[9];
    if (iz == 0 || iz == P.nz - 1 || ix == 0 || ix == P.nx - 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = cmake(0.0, 0.0);
    } else {
        const MzRow row = mz_row_at(P, c, iz, ix);
        double bn[9];
        cplx Kn[9];
        const double b0 = db[i];
#pragma unroll
        for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
            for (int sx = -1; sx <= 1; ++sx) {
                const long long j = i + (long long)sz * P.nx + sx;
                const double bj = db[j];
                const cplx k = mz_kappa(P, c[j]);
                bn[mz_slot(sz, sx)] = (b0 + bj) / 2.0;
                Kn[mz_slot(sz, sx)] = cmake(k.x * bj, k.y * bj);
            }
        mz_star(P, row, bn, Kn, out);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) C[(long long)k * N + i] = out[k];
}

// dC[9][N] = L[db] for the operator the handle holds (its c, PML and the frequency of its last assembly): db N float64, dC 9 N complex128, boundary rows zero.
// Returns when dC is complete.
extern "C" int helm_buoyancy_planes_device(helm_op *op, const void *dDb, void *dC) {
    helm_tuning_refresh();
    if (!op || !dDb || !dC) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_buoyancy_planes_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || (((uintptr_t)dDb) & 7) || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dDb, (size_t)op->N * 8, dC, (size_t)op->N * 9 * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_buoyancy_planes_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_buoyancy_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)dDb, (cplx *)dC);
    return launched(op);
}

// R[s ldr + i] = coef sum_k C_k[i] (CONJ ? conj(U[s]) : U[s])[i + off_k] for the nsrc columns, cells outside the grid contributing nothing: the walk of
// k_virtual_sources_op (a tile of OP_TILE_X cells and OP_ROWS rows per wave, OP_UNROLL columns together, a rolling window of three rows in registers), with
// the left and right neighbours kept apart because their coefficients differ.  The nine planes are read once per group of columns: per cell and column 16 (8)
// bytes read and 16 written, plus 144 / OP_UNROLL.  The sum runs k = 0 .. 8: the same bits on every run.
struct LagRow { cplx t, l, r; };
__device__ __forceinline__ void lane_left_right(cplx t, cplx &l, cplx &r) {
    l = cmake(__shfl_up(t.x, 1, 64), __shfl_up(t.y, 1, 64));          // (lane 0 and lane 63 are halo lanes: their l / r are never used)
    r = cmake(__shfl_down(t.x, 1, 64), __shfl_down(t.y, 1, 64));
}

template <class F, bool CONJ>
__global__ __launch_bounds__(256) void k_stencil_sources(F U, int nsrc, long long ldu, const cplx *__restrict__ C, cplx coef, cplx *__restrict__ R, long long ldr,
                                                         int nz, int nx) {
    const OpJob job(nz, nx);
    if (!job.live) return;                                  // (a whole wave: the lane exchanges below stay complete)
    const long long N = (long long)nz * nx;
    const int s0 = blockIdx.y * OP_UNROLL, ncol = min(OP_UNROLL, nsrc - s0);
    const int x = job.x;
    typename F::raw raw[OP_UNROLL];
    LagRow up[OP_UNROLL], mid[OP_UNROLL], dn[OP_UNROLL];
    double sc[OP_UNROLL];
#pragma unroll
    for (int j = 0; j < OP_UNROLL; ++j) sc[j] = U.scale(s0 + min(j, ncol - 1));
    auto fetch = [&](int z) {
        const bool in = job.xin && z >= 0 && z < nz;
        const long long i = (long long)z * nx + x;
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) raw[j] = (in && j < ncol) ? U.load((long long)(s0 + j) * ldu + i) : typename F::raw{};
    };
    auto make = [&](LagRow *row) {
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) {
            cplx u = U.scaled(raw[j], sc[j]);
            if (CONJ) u = cconj(u);
            row[j].t = u;
            lane_left_right(u, row[j].l, row[j].r);
        }
    };
    fetch(job.z0 - 1); make(up);
    fetch(job.z0); make(mid);
    fetch(job.z0 + 1);
    for (int z = job.z0; z < job.z1; ++z) {
        make(dn);
        if (z + 1 < job.z1) fetch(z + 2);                  // (wave-uniform)
        if (job.store) {
            const long long i = (long long)z * nx + x;
            cplx ck[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) ck[k] = C[(long long)k * N + i];
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j)
                if (j < ncol) {
                    cplx acc = cmake(0.0, 0.0);
                    cfma(acc, ck[0], up[j].l); cfma(acc, ck[1], up[j].t); cfma(acc, ck[2], up[j].r);
                    cfma(acc, ck[3], mid[j].l); cfma(acc, ck[4], mid[j].t); cfma(acc, ck[5], mid[j].r);
                    cfma(acc, ck[6], dn[j].l); cfma(acc, ck[7], dn[j].t); cfma(acc, ck[8], dn[j].r);
                    R[(long long)(s0 + j) * ldr + i] = cmul(coef, acc);
                }
        }
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) { up[j] = mid[j]; mid[j] = dn[j]; }
    }
}

static int stencil_sources_args(helm_op *op, const void *dU, size_t esize, int nsrc, long long ldu, const void *dC, void *dR, long long ldr) {
    if (!op || !dU || !dC || !dR || nsrc < 1 || nsrc > 65535 * OP_UNROLL || ldu < op->N || ldr < op->N) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_stencil_sources_device")) return rc;
    const size_t rbytes = (size_t)nsrc * ldr * sizeof(cplx);
    if (ranges_overlap(dU, (size_t)nsrc * ldu * esize, dR, rbytes) || ranges_overlap(dC, (size_t)op->N * 9 * sizeof(cplx), dR, rbytes)) return HELM_ERR_ARG;
    return HELM_OK;
}

// R[s][i] = coef sum_k C_k[i] U[s][i + off_k] (conj != 0: conj(U[s])) for s < nsrc, i < N (the handle's nz x nx grid): U [nsrc][ldu] complex128, C [9][N]
// complex128 (helm_buoyancy_planes_device), R [nsrc][ldr] complex128, ldu, ldr >= N.  R must not overlap U or C.  Returns when R is complete.
extern "C" int helm_stencil_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im, int conj,
                                           void *dR, long long ldr) {
    helm_tuning_refresh();
    if (int rc = stencil_sources_args(op, dU, sizeof(cplx), nsrc, ldu, dC, dR, ldr)) return rc;
    if ((((uintptr_t)dU) | ((uintptr_t)dC) | ((uintptr_t)dR)) & 15) return HELM_ERR_ARG;       // (16-byte loads and stores)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid = op_grid(op, (nsrc + OP_UNROLL - 1) / OP_UNROLL);
    const FieldC128 U{(const cplx *)dU};
    if (conj) HELM_LAUNCH((k_stencil_sources<FieldC128, true>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dC, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    else HELM_LAUNCH((k_stencil_sources<FieldC128, false>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dC, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    return launched(op);
}

extern "C" int helm_stencil_sources_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im,
                                               int conj, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (int rc = stencil_sources_args(op, dU32, sizeof(cplxf32), nsrc, ldu, dC, dR, ldr)) return rc;
    if (!dExp || (((uintptr_t)dU32) & 7) || (((uintptr_t)dExp) & 3) || ((((uintptr_t)dC) | ((uintptr_t)dR)) & 15)) return HELM_ERR_ARG;       // (8-byte loads of U32)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid = op_grid(op, (nsrc + OP_UNROLL - 1) / OP_UNROLL);
    const FieldC64 U{(const cplxf32 *)dU32, (const int *)dExp};
    if (conj) HELM_LAUNCH((k_stencil_sources<FieldC64, true>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dC, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    else HELM_LAUNCH((k_stencil_sources<FieldC64, false>), grid, dim3(256), 0, op->stream, U, nsrc, ldu, (const cplx *)dC, cmake(coef_re, coef_im), (cplx *)dR, ldr, op->nz, op->nx);
    return launched(op);
}

// P_k[i] += sum_s UB[s ldb + i] UF[s ldf + i + off_k] for the nine lags k and the interior cells i (the boundary lines of P are left as they are: the rows of
// dC are zero there; an interior cell has every neighbour inside the grid).  A workgroup of LAG_WAVES waves owns a tile of OP_TILE_X x LAG_ROWS cells.  Column s
// goes to wave s mod LAG_WAVES, which keeps the 9 LAG_ROWS sums of its lane's cells in REGISTERS over all its columns: per column it loads the LAG_ROWS + 2 rows
// of UF and the LAG_ROWS rows of UB at once (ten 16-byte loads in flight per lane), gets the left and right neighbours of UF from the adjacent lanes and
// does 9 LAG_ROWS complex FMAs.  Then the waves add their sums into ONE LDS tile in wave order (36 KiB; nine accumulators per cell and wave side by side, the
// scheme of k_imaging_op, would be 9 x 64 KiB), and wave r adds row r to P: one writer per entry, a fixed order, no atomics -- the same bits on every run.
// Per cell and column 16 B of UB and 16 (8) B of UF, the latter times (1 + 2 / LAG_ROWS)(1 + 2 / OP_TILE_X) for the halo, which neighbouring workgroups read at the
// same time; the nine planes of P once per call.
constexpr int LAG_ROWS = 4;         // output rows per workgroup: 72 accumulator doubles per lane
constexpr int LAG_WAVES = 4;        // waves per workgroup
static_assert(LAG_ROWS <= LAG_WAVES, "wave r finishes row r");

template <class F>
__global__ __launch_bounds__(64 * LAG_WAVES) void k_lag_imaging(F UF, long long ldf, const cplx *__restrict__ UB, long long ldb, int nsrc, cplx *__restrict__ P,
                                                                int nz, int nx) {
    __shared__ cplx part[LAG_ROWS][9][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * OP_TILE_X + lane - 1, z0 = (int)(blockIdx.x / ntx) * LAG_ROWS;
    const bool xin = x >= 0 && x < nx;
    const bool store = lane >= 1 && lane <= OP_TILE_X && x >= 1 && x <= nx - 2;
    const long long N = (long long)nz * nx;
    cplx acc[LAG_ROWS][9];
#pragma unroll
    for (int r = 0; r < LAG_ROWS; ++r)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[r][k] = cmake(0.0, 0.0);
    for (int s = wave; s < nsrc; s += LAG_WAVES) {             // (wave-uniform: the lane exchanges stay complete)
        const double sc = UF.scale(s);
        typename F::raw rf[LAG_ROWS + 2];
        cplx rb[LAG_ROWS];
#pragma unroll
        for (int r = 0; r < LAG_ROWS + 2; ++r) {
            const int z = z0 - 1 + r;
            rf[r] = (xin && z >= 0 && z < nz) ? UF.load((long long)s * ldf + (long long)z * nx + x) : typename F::raw{};
        }
#pragma unroll
        for (int r = 0; r < LAG_ROWS; ++r) {
            const int z = z0 + r;
            rb[r] = (store && z >= 1 && z <= nz - 2) ? UB[(long long)s * ldb + (long long)z * nx + x] : cmake(0.0, 0.0);      // (zero off the interior: nothing is added there)
        }
#pragma unroll
        for (int wr = 0; wr < LAG_ROWS + 2; ++wr) {            // row z0 - 1 + wr of UF serves the output rows wr - 2 (dz = +1), wr - 1 (dz = 0) and wr (dz = -1)
            LagRow w;
            w.t = UF.scaled(rf[wr], sc);
            lane_left_right(w.t, w.l, w.r);
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                const int r = wr - 1 - dz;
                if (r >= 0 && r < LAG_ROWS) {
                    cfma(acc[r][3 * (dz + 1) + 0], rb[r], w.l);
                    cfma(acc[r][3 * (dz + 1) + 1], rb[r], w.t);
                    cfma(acc[r][3 * (dz + 1) + 2], rb[r], w.r);
                }
            }
        }
    }
    for (int w = 0; w < LAG_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < LAG_ROWS; ++r)
#pragma unroll
                for (int k = 0; k < 9; ++k) part[r][k][lane] = w == 0 ? acc[r][k] : cadd(part[r][k][lane], acc[r][k]);
        }
        __syncthreads();
    }
    if (wave < LAG_ROWS) {
        const int z = z0 + wave;
        if (store && z >= 1 && z <= nz - 2) {
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                cplx *p = P + (long long)k * N + i;
                *p = cadd(*p, part[wave][k][lane]);
            }
        }
    }
}
static dim3 lag_grid(const helm_op *op) {
    return dim3((unsigned)(((op->nx + OP_TILE_X - 1) / OP_TILE_X) * ((op->nz + LAG_ROWS - 1) / LAG_ROWS)));
}

static int lag_imaging_args(helm_op *op, const void *dUF, size_t esize, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    if (!op || !dUF || !dUB || !dP || nsrc < 1 || ldf < op->N || ldb < op->N) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_lag_imaging_accumulate_device")) return rc;
    const size_t pbytes = (size_t)op->N * 9 * sizeof(cplx);
    if (ranges_overlap(dUF, (size_t)nsrc * ldf * esize, dP, pbytes) || ranges_overlap(dUB, (size_t)nsrc * ldb * sizeof(cplx), dP, pbytes)) return HELM_ERR_ARG;
    return HELM_OK;
}

// P[k][i] += sum_s UB[s][i] UF[s][i + off_k] for k < 9 and the interior cells i of the handle's grid: UF [nsrc][ldf], UB [nsrc][ldb], P [9][N] complex128.  P must
// not overlap the fields.  Returns when P is complete.
extern "C" int helm_lag_imaging_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    helm_tuning_refresh();
    if (int rc = lag_imaging_args(op, dUF, sizeof(cplx), ldf, dUB, ldb, nsrc, dP)) return rc;
    if ((((uintptr_t)dUF) | ((uintptr_t)dUB) | ((uintptr_t)dP)) & 15) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_lag_imaging<FieldC128>, lag_grid(op), dim3(64 * LAG_WAVES), 0, op->stream, FieldC128{(const cplx *)dUF}, ldf, (const cplx *)dUB, ldb, nsrc, (cplx *)dP,
                op->nz, op->nx);
    return launched(op);
}

extern "C" int helm_lag_imaging_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    helm_tuning_refresh();
    if (int rc = lag_imaging_args(op, dUF32, sizeof(cplxf32), ldf, dUB, ldb, nsrc, dP)) return rc;
    if (!dExp || (((uintptr_t)dUF32) & 7) || (((uintptr_t)dExp) & 3) || ((((uintptr_t)dUB) | ((uintptr_t)dP)) & 15)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_lag_imaging<FieldC64>, lag_grid(op), dim3(64 * LAG_WAVES), 0, op->stream, FieldC64{(const cplxf32 *)dUF32, (const int *)dExp}, ldf, (const cplx *)dUB, ldb, nsrc,
                (cplx *)dP, op->nz, op->nx);
    return launched(op);
}

// G[j] += w sum_(k, i) L_((k, i), j) P_k[i] (CONJ: conj(L)): the transpose of k_buoyancy_planes as a gather, one lane per cell j over the interior rows i = j - o of
// the 3 x 3 block around it.  Row i holds b_j three ways: kappa_j b_j times the mass weight in the plane of the lag o; (b_i + b_j) / 2 in the average of that
// lag; and, for i = j, b_i / 2 in all eight averages.  With T the row's own stiffness factors (mz_star: corners tc, verticals tv, horizontals th, the cross
// term tzx) the coefficient of the average of lag o is
//     Q_o = T_o (P_o - P_4)  [+ tzx (P_(sz, 0) - P_(0, sx)) for a corner o = (sz, sx)]
// (the centre plane takes every average with the opposite sign: the stiffness rows sum to zero).  One writer per cell, a fixed order.
struct MzStiff { cplx tv[2], th[2], tc[2][2], tzx; };
template <bool CONJ>
__device__ __forceinline__ MzStiff mz_stiffness(const MzParams &P, MzRow row) {
    if (CONJ) { row.X = cconj(row.X); row.Z = cconj(row.Z); row.px = cconj(row.px); row.pz = cconj(row.pz); }
    const double dxx = P.dx * P.dx, dzz = P.dz * P.dz, dxz = (dxx + dzz) / 2.0, dd = sqrt(dxz);
    MzStiff t;
    const cplx ZpX = cscale(cadd(row.Z, row.X), 1.0 / (4 * dxz));
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double sg = a ? 1.0 : -1.0;
        t.tv[a] = cscale(cadd(cscale(row.Z, 1.0 / P.dz), cscale(row.pz, sg / 2.0)), MZ_WA / P.dz);
        t.th[a] = cscale(cadd(cscale(row.X, 1.0 / P.dx), cscale(row.px, sg / 2.0)), MZ_WA / P.dx);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const double sx = b ? 1.0 : -1.0;
            t.tc[a][b] = cscale(cadd(ZpX, cscale(cadd(cscale(row.pz, sg), cscale(row.px, sx)), 1.0 / (4 * dd))), MZ_WB);
        }
    }
    t.tzx = cscale(csub(row.Z, row.X), MZ_WB / (4 * dxz));
    return t;
}
// Q_o of row i for the lag o = (sz, sx) != (0, 0)
__device__ __forceinline__ cplx lag_coefficient(const MzStiff &t, const cplx *__restrict__ Pl, long long N, long long i, int sz, int sx) {
    const cplx d = csub(Pl[(long long)mz_slot(sz, sx) * N + i], Pl[4 * N + i]);
    if (sz == 0) return cmul(t.th[(sx + 1) / 2], d);
    if (sx == 0) return cmul(t.tv[(sz + 1) / 2], d);
    cplx q = cmul(t.tc[(sz + 1) / 2][(sx + 1) / 2], d);
    cfma(q, t.tzx, csub(Pl[(long long)mz_slot(sz, 0) * N + i], Pl[(long long)mz_slot(0, sx) * N + i]));
    return q;
}

template <bool CONJ>
__global__ __launch_bounds__(256) void k_buoyancy_adjoint(MzParams P, const cplx *__restrict__ c, const cplx *__restrict__ Pl, cplx w, cplx *__restrict__ G) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int jz = (int)(j / P.nx), jx = (int)(j % P.nx);
    cplx mass = cmake(0.0, 0.0), avg = cmake(0.0, 0.0);
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int iz = jz - sz, ix = jx - sx;                 // row i sees cell j at the lag (sz, sx)
            if (iz < 1 || iz > P.nz - 2 || ix < 1 || ix > P.nx - 2) continue;
            const long long i = (long long)iz * P.nx + ix;
            const MzStiff t = mz_stiffness<CONJ>(P, mz_row_at(P, c, iz, ix));
            const double m = (sz == 0 && sx == 0) ? MZ_WC : ((sz == 0 || sx == 0) ? MZ_WD : MZ_WE);
            const cplx p = Pl[(long long)mz_slot(sz, sx) * N + i];
            mass.x += m * p.x; mass.y += m * p.y;
            if (sz == 0 && sx == 0) {
#pragma unroll
                for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
                    for (int ox = -1; ox <= 1; ++ox)
                        if (oz != 0 || ox != 0) avg = cadd(avg, lag_coefficient(t, Pl, N, i, oz, ox));
            } else avg = cadd(avg, lag_coefficient(t, Pl, N, i, sz, sx));
        }
    cplx kap = mz_kappa(P, c[j]);
    if (CONJ) kap = cconj(kap);
    cplx sum = cscale(avg, 0.5);
    cfma(sum, kap, mass);
    cplx g = G[j];
    cfma(g, w, sum);
    G[j] = g;
}

// G[j] += w sum_(k, i) L_((k, i), j) P_k[i] for j < N (conj != 0: the conjugated coefficients), L the map of helm_buoyancy_planes_device for the operator the
// handle holds: P [9][N] complex128 (its boundary rows are not read), G N complex128.  G must not overlap P.  Returns when G is complete.
extern "C" int helm_buoyancy_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG) {
    helm_tuning_refresh();
    if (!op || !dP || !dG) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_buoyancy_adjoint_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dP) | ((uintptr_t)dG)) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dP, (size_t)op->N * 9 * sizeof(cplx), dG, (size_t)op->N * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_buoyancy_adjoint_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
    if (conj) HELM_LAUNCH(k_buoyancy_adjoint<true>, grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const cplx *)dP, cmake(w_re, w_im), (cplx *)dG);
    else HELM_LAUNCH(k_buoyancy_adjoint<false>, grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const cplx *)dP, cmake(w_re, w_im), (cplx *)dG);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the total velocity derivative of MiniZephyr (linearisation='full'): mass term, PML stretch and the density that follows c
// ------------------------------------------------------------------------------------------
// A row is mz_star(row_i, bn, Kn): linear in (row, Kn) for fixed averaged buoyancies bn and linear in (bn, Kn) for a fixed row.  The row factors are functions of
// c_i, the mass terms Kn_k = kappa_j b_j of c_j (j = i + o_k), so along a real dc the nine planes of dA are
//     dC_i = mz_star(dc_i d row_i / dc, bn[b], Kn_k = (d kappa_j / dc) b_j dc_j)        (the mass term of k_virtual_sources_op and the stretch it leaves out)
//          + mz_star(row_i, bn[db], Kn_k = kappa_j db_j)                               (only where the density follows c: db = (d b / d c) dc, the caller's)
// with b = 1 / rho of the model the handle assembled with, boundary rows zero.  The forward and imaging loops are those of the density derivative
// (k_stencil_sources, k_lag_imaging); the transpose of the second star is k_buoyancy_adjoint.

__device__ __forceinline__ MzRow mz_row_dc_at(const MzParams &P, const cplx *__restrict__ c, int iz, int ix) {
    double dX, sX, dZ, sZ;
    mz_profile_at(P.nx, P.npml, P.dx, P.fs3, P.fs1, ix, dX, sX);
    mz_profile_at(P.nz, P.npml, P.dz, P.fs0, P.fs2, iz, dZ, sZ);
    return mz_row_factors_dc(P, c[(long long)iz * P.nx + ix], dX, sX, dZ, sZ);
}

// dC = V[dc] (+ L[db] when db is given): one lane per cell, the assembly's star once or twice.  An interior row reads only cells inside the grid.
__global__ __launch_bounds__(256) void k_velocity_planes(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ dc,
                                                         const double *__restrict__ db, cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);
    cplx out[9];
    if (iz == 0 || iz == P.nz - 1 || ix == 0 || ix == P.nx - 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = cmake(0.0, 0.0);
    } else {
        MzRow drow = mz_row_dc_at(P, c, iz, ix);
        const double v0 = dc[i];
        drow.X = cscale(drow.X, v0); drow.Z = cscale(drow.Z, v0); drow.px = cscale(drow.px, v0); drow.pz = cscale(drow.pz, v0);
        double bn[9];
        cplx Kn[9];
        const double b0 = 1.0 / rho[i];
#pragma unroll
        for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
            for (int sx = -1; sx <= 1; ++sx) {
                const long long j = i + (long long)sz * P.nx + sx;
                const double bj = 1.0 / rho[j];
                bn[mz_slot(sz, sx)] = (b0 + bj) / 2.0;
                Kn[mz_slot(sz, sx)] = cscale(mz_kappa_dc(P, c[j]), bj * dc[j]);
            }
        mz_star(P, drow, bn, Kn, out);
        if (db) {
            const MzRow row = mz_row_at(P, c, iz, ix);
            cplx more[9];
            const double d0 = db[i];
#pragma unroll
            for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
                for (int sx = -1; sx <= 1; ++sx) {
                    const long long j = i + (long long)sz * P.nx + sx;
                    const double dj = db[j];
                    bn[mz_slot(sz, sx)] = (d0 + dj) / 2.0;
                    Kn[mz_slot(sz, sx)] = cscale(mz_kappa(P, c[j]), dj);
                }
            mz_star(P, row, bn, Kn, more);
#pragma unroll
            for (int k = 0; k < 9; ++k) out[k] = cadd(out[k], more[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) C[(long long)k * N + i] = out[k];
}

// dC[9][N] = V[dc] + (dDb ? L[db] : 0) for the operator the handle holds (its c and rho, PML and the frequency of its last assembly): dc, db N float64 (db may be
// NULL), dC 9 N complex128, boundary rows zero.  Returns when dC is complete.
extern "C" int helm_velocity_planes_device(helm_op *op, const void *dDc, const void *dDb, void *dC) {
    helm_tuning_refresh();
    if (!op || !dDc || !dC) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_velocity_planes_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dDc) | ((uintptr_t)dDb)) & 7) || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;
    const size_t cbytes = (size_t)op->N * 9 * sizeof(cplx);
    if (ranges_overlap(dDc, (size_t)op->N * 8, dC, cbytes) || (dDb && ranges_overlap(dDb, (size_t)op->N * 8, dC, cbytes))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_velocity_planes_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_velocity_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const double *)dDc,
                (const double *)dDb, (cplx *)dC);
    return launched(op);
}

// G[j] += w sum_(k, i) V_((k, i), j) P_k[i] (CONJ: conj(V)): the transpose of the first star of k_velocity_planes, one lane per cell j.  The mass part is the
// gather of k_buoyancy_adjoint over the interior rows i = j - o, times (d kappa_j / dc) b_j.  The stretch part is local to row j: its differentiated stiffness
// factors dT (mz_stiffness is linear in the row) times the averaged buoyancies a_o = (b_j + b_(j+o)) / 2 and the Q-differences of P at j (lag_coefficient); a
// boundary row has none.  One writer per cell, a fixed order; the boundary rows of P are not read.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_velocity_adjoint(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const cplx *__restrict__ Pl, cplx w,
                                                          cplx *__restrict__ G) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int jz = (int)(j / P.nx), jx = (int)(j % P.nx);
    const double bj = 1.0 / rho[j];
    cplx mass = cmake(0.0, 0.0), stretch = cmake(0.0, 0.0);
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int iz = jz - sz, ix = jx - sx;                 // row i sees cell j at the lag (sz, sx)
            if (iz < 1 || iz > P.nz - 2 || ix < 1 || ix > P.nx - 2) continue;
            const double m = (sz == 0 && sx == 0) ? MZ_WC : ((sz == 0 || sx == 0) ? MZ_WD : MZ_WE);
            const cplx p = Pl[(long long)mz_slot(sz, sx) * N + (long long)iz * P.nx + ix];
            mass.x += m * p.x; mass.y += m * p.y;
        }
    if (jz >= 1 && jz <= P.nz - 2 && jx >= 1 && jx <= P.nx - 2) {
        const MzStiff dt = mz_stiffness<CONJ>(P, mz_row_dc_at(P, c, jz, jx));
#pragma unroll
        for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
            for (int ox = -1; ox <= 1; ++ox)
                if (oz != 0 || ox != 0) {
                    const double a = (bj + 1.0 / rho[j + (long long)oz * P.nx + ox]) / 2.0;
                    stretch = cadd(stretch, cscale(lag_coefficient(dt, Pl, N, j, oz, ox), a));
                }
    }
    cplx dk = cscale(mz_kappa_dc(P, c[j]), bj);
    if (CONJ) dk = cconj(dk);
    cplx sum = stretch;
    cfma(sum, dk, mass);
    cplx g = G[j];
    cfma(g, w, sum);
    G[j] = g;
}

// G[j] += w sum_(k, i) V_((k, i), j) P_k[i] for j < N (conj != 0: the conjugated coefficients), V the map of helm_velocity_planes_device with dDb NULL for the
// operator the handle holds: P [9][N] complex128 (its boundary rows are not read), G N complex128.  G must not overlap P.  Returns when G is complete.
extern "C" int helm_velocity_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG) {
    helm_tuning_refresh();
    if (!op || !dP || !dG) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_velocity_adjoint_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dP) | ((uintptr_t)dG)) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dP, (size_t)op->N * 9 * sizeof(cplx), dG, (size_t)op->N * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_velocity_adjoint_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
    if (conj) HELM_LAUNCH(k_velocity_adjoint<true>, grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const cplx *)dP, cmake(w_re, w_im), (cplx *)dG);
    else HELM_LAUNCH(k_velocity_adjoint<false>, grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const cplx *)dP, cmake(w_re, w_im), (cplx *)dG);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the pseudo-Hessian diagonal of the exact derivatives: H[i] += alpha W[i] sum_s || (d A / d p_i) u^_s ||^2
// ------------------------------------------------------------------------------------------
// A unit perturbation of cell i (of its velocity, or of its buoyancy) touches only the rows j of the 3 x 3 block around i, and in those only the lags that point
// back into the block (frechet.pseudoHessianDiagonal states the same).  Per cell that is a small matrix E_i, independent of the source:
//     row i             nine coefficients: mz_star on the differentiated row factors and d kappa_i / dc b_i (velocity), on the row itself with the averages
//                       1 / 2 and kappa_i (buoyancy)
//     row j = i - o     velocity: the one mass weight m_o d kappa_i / dc b_i at the lag o, which multiplies u[i] -- the eight rows together are
//                       |d kappa_i / dc b_i|^2 sum_j m_o^2 |u[i]|^2, one real weight S_i.
//                       buoyancy: m_o kappa_i + T_o(j) / 2 at the lag o and -T_o(j) / 2 at the centre, T the row's own stiffness factor (mz_stiffness); a corner
//                       row has +-tzx(j) / 2 at the two lags beside o as well.  2 coefficients per edge row, 4 per corner row: 9 + 8 + 16 = 33.
//     Gardner           velocity + chain_i x buoyancy, coefficient by coefficient (the mass weight of the velocity part joins the lag o of row j).
// The stored fields are conj(u^): the coefficients are conjugated once instead (|conj(E) conj(u)| = |E u|).
//
// The walk: a workgroup of PH_WAVES waves owns OP_TILE_X cells of one grid row, one lane per cell plus a halo lane at either end.  The lane's E_i stays in
// registers for the whole kernel; the columns go to the waves in groups of PH_UNROLL (group g to wave g mod PH_WAVES).  Per column a lane loads the three rows
// z - 1, z, z + 1 of its own x (3 PH_UNROLL loads in flight), takes the left and right neighbours from the adjacent lanes, forms the up to nine row sums and adds
// their squared moduli to one double.  The waves add their sums into one LDS row in wave order and wave 0 adds alpha W (.) sum to H: one writer per cell, a
// fixed order, no atomics -- the same bits on every run.  Rows z - 1 and z + 1 are the halo: the workgroups of the neighbouring rows load them at the same time.
// PACKED: E_i is read from an array [ph_ncoef(MODE)][N] that k_pseudo_hessian_coefficients wrote (the same function, one lane per cell) instead of being built
// by every wave of the workgroup.
enum { PH_VELOCITY = 0, PH_BUOYANCY = 1, PH_GARDNER = 2 };
constexpr int PH_WAVES = 4;         // waves per workgroup
constexpr int PH_UNROLL = 4;        // columns a wave loads together

// e[a]: the edge rows j = i - o, o = (-1, 0), (1, 0), (0, -1), (0, 1): {lag o, centre}.  k[a]: the corner rows, a = 2 [sz > 0] + [sx > 0]: {lag o, lag (0, sx) -> cell
// i - (sz, 0), lag (sz, 0) -> cell i - (0, sx), centre}.  S: the real weight of |u[i]|^2 (velocity alone).
struct PhCoef { cplx c[9]; cplx e[4][2]; cplx k[4][4]; double S; };
__host__ __device__ constexpr int ph_ncoef(int mode) { return mode == PH_VELOCITY ? 10 : 33; }

template <int MODE>
__device__ __forceinline__ void ph_coefficients(const MzParams &P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ chain,
                                                int iz, int ix, PhCoef &E) {
    const cplx zero = cmake(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < 9; ++k) E.c[k] = zero;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        E.e[a][0] = E.e[a][1] = zero;
        E.k[a][0] = E.k[a][1] = E.k[a][2] = E.k[a][3] = zero;
    }
    E.S = 0.0;
    const long long i = (long long)iz * P.nx + ix;
    const cplx ci = c[i];
    const cplx kap = mz_kappa(P, ci);
    const double ch = MODE == PH_GARDNER ? chain[i] : 1.0;
    const cplx w = MODE != PH_BUOYANCY ? cscale(mz_kappa_dc(P, ci), 1.0 / rho[i]) : zero;       // d K_i / d c_i at the density of the handle
    if (iz >= 1 && iz <= P.nz - 2 && ix >= 1 && ix <= P.nx - 2) {           // row i: the assembly's star on the unit perturbation
        double bn[9];
        cplx Kn[9];
        if (MODE != PH_BUOYANCY) {
            const double b0 = 1.0 / rho[i];
#pragma unroll
            for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
                for (int sx = -1; sx <= 1; ++sx) {
                    bn[mz_slot(sz, sx)] = (b0 + 1.0 / rho[i + (long long)sz * P.nx + sx]) / 2.0;
                    Kn[mz_slot(sz, sx)] = zero;
                }
            Kn[4] = w;
            mz_star(P, mz_row_dc_at(P, c, iz, ix), bn, Kn, E.c);
        }
        if (MODE != PH_VELOCITY) {
            cplx more[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) { bn[k] = 0.5; Kn[k] = zero; }
            bn[4] = 1.0;
            Kn[4] = kap;
            mz_star(P, mz_row_at(P, c, iz, ix), bn, Kn, more);
#pragma unroll
            for (int k = 0; k < 9; ++k) E.c[k] = MODE == PH_GARDNER ? cadd(E.c[k], cscale(more[k], ch)) : more[k];
        }
    }
    double m2 = 0.0;
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            if (sz == 0 && sx == 0) continue;
            const int jz = iz - sz, jx = ix - sx;                 // row j sees cell i at the lag (sz, sx)
            if (jz < 1 || jz > P.nz - 2 || jx < 1 || jx > P.nx - 2) continue;
            const double m = (sz == 0 || sx == 0) ? MZ_WD : MZ_WE;
            if (MODE == PH_VELOCITY) { m2 += m * m; continue; }
            const MzStiff T = mz_stiffness<false>(P, mz_row_at(P, c, jz, jx));
            const cplx t = sx == 0 ? T.tv[(sz + 1) / 2] : (sz == 0 ? T.th[(sx + 1) / 2] : T.tc[(sz + 1) / 2][(sx + 1) / 2]);
            cplx lag = cscale(cadd(cscale(kap, m), cscale(t, 0.5)), ch);
            if (MODE == PH_GARDNER) lag = cadd(lag, cscale(w, m));
            const cplx ctr = cscale(t, -0.5 * ch);
            if (sz != 0 && sx != 0) {
                const int a = 2 * ((sz + 1) / 2) + (sx + 1) / 2;
                E.k[a][0] = lag;
                E.k[a][1] = cscale(T.tzx, -0.5 * ch);            // row j's lag (0, sx): the horizontal neighbours take -tzx
                E.k[a][2] = cscale(T.tzx, 0.5 * ch);             // row j's lag (sz, 0)
                E.k[a][3] = ctr;
            } else {
                const int a = sx == 0 ? (sz + 1) / 2 : 2 + (sx + 1) / 2;
                E.e[a][0] = lag;
                E.e[a][1] = ctr;
            }
        }
    if (MODE == PH_VELOCITY) E.S = m2 * (w.x * w.x + w.y * w.y);
#pragma unroll
    for (int k = 0; k < 9; ++k) E.c[k] = cconj(E.c[k]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        E.e[a][0] = cconj(E.e[a][0]); E.e[a][1] = cconj(E.e[a][1]);
#pragma unroll
        for (int q = 0; q < 4; ++q) E.k[a][q] = cconj(E.k[a][q]);
    }
}

// the packed order of a cell's coefficients: c[0..8], then (velocity) S, or e[0..3][0..1], k[0..3][0..3]
template <int MODE, class FN>
__device__ __forceinline__ void ph_each(PhCoef &E, FN &&fn) {
#pragma unroll
    for (int k = 0; k < 9; ++k) fn(k, E.c[k]);
    if (MODE == PH_VELOCITY) {
        cplx s = cmake(E.S, 0.0);
        fn(9, s);
        E.S = s.x;
    } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) { fn(9 + 2 * a, E.e[a][0]); fn(10 + 2 * a, E.e[a][1]); }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) fn(17 + 4 * a + q, E.k[a][q]);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_pseudo_hessian_coefficients(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho,
                                                                     const double *__restrict__ chain, cplx *__restrict__ Epk) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    PhCoef E;
    ph_coefficients<MODE>(P, c, rho, chain, (int)(i / P.nx), (int)(i % P.nx), E);
    ph_each<MODE>(E, [&](int q, cplx &v) { Epk[(long long)q * N + i] = v; });
}

template <class F, int MODE, bool PACKED>
__global__ __launch_bounds__(64 * PH_WAVES) void k_pseudo_hessian(F U, int nsrc, long long ld, MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho,
                                                                  const double *__restrict__ chain, const cplx *__restrict__ Epk, double alpha,
                                                                  const double *__restrict__ W, double *__restrict__ H) {
    __shared__ double part[64];
    const int nz = P.nz, nx = P.nx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * OP_TILE_X + lane - 1, z = (int)(blockIdx.x / ntx);
    const bool xin = x >= 0 && x < nx;
    const bool store = lane >= 1 && lane <= OP_TILE_X && x < nx;
    const long long N = (long long)nz * nx, i = (long long)z * nx + x;
    PhCoef E;
    if (store) {
        if (PACKED) ph_each<MODE>(E, [&](int q, cplx &v) { v = Epk[(long long)q * N + i]; });
        else ph_coefficients<MODE>(P, c, rho, chain, z, x, E);
    } else {
        ph_each<MODE>(E, [&](int, cplx &v) { v = cmake(0.0, 0.0); });       // (a halo lane adds nothing)
    }
    double acc = 0.0;
    const int ngroups = (nsrc + PH_UNROLL - 1) / PH_UNROLL;
    for (int g = wave; g < ngroups; g += PH_WAVES) {          // (wave-uniform: the lane exchanges stay complete)
        const int s0 = g * PH_UNROLL, ncol = min(PH_UNROLL, nsrc - s0);
        typename F::raw raw[PH_UNROLL][3];
        double sc[PH_UNROLL];
#pragma unroll
        for (int j = 0; j < PH_UNROLL; ++j) {
            sc[j] = U.scale(s0 + min(j, ncol - 1));
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int zz = z - 1 + r;
                raw[j][r] = (xin && j < ncol && zz >= 0 && zz < nz) ? U.load((long long)(s0 + j) * ld + (long long)zz * nx + x) : typename F::raw{};
            }
        }
#pragma unroll
        for (int j = 0; j < PH_UNROLL; ++j) {
            cplx v[9];                                          // the 3 x 3 block around the lane's cell in the slot order of the operator
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                v[3 * r + 1] = U.scaled(raw[j][r], sc[j]);
                lane_left_right(v[3 * r + 1], v[3 * r], v[3 * r + 2]);
            }
            cplx r0 = cmake(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 9; ++k) cfma(r0, E.c[k], v[k]);
            double sum = cabs2(r0);
            if (MODE == PH_VELOCITY) sum += E.S * cabs2(v[4]);
            else {
#pragma unroll
                for (int a = 0; a < 4; ++a) {                   // the edge row j = i - o sits at the slot of -o
                    const int sz = a < 2 ? 2 * a - 1 : 0, sx = a < 2 ? 0 : 2 * (a - 2) - 1;
                    cplx r1 = cmul(E.e[a][0], v[4]);
                    cfma(r1, E.e[a][1], v[mz_slot(-sz, -sx)]);
                    sum += cabs2(r1);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int sz = 2 * (a / 2) - 1, sx = 2 * (a % 2) - 1;
                    cplx r2 = cmul(E.k[a][0], v[4]);
                    cfma(r2, E.k[a][1], v[mz_slot(-sz, 0)]);     // j + (0, sx) = i - (sz, 0)
                    cfma(r2, E.k[a][2], v[mz_slot(0, -sx)]);     // j + (sz, 0) = i - (0, sx)
                    cfma(r2, E.k[a][3], v[mz_slot(-sz, -sx)]);
                    sum += cabs2(r2);
                }
            }
            if (j < ncol) acc += sum;
        }
    }
    for (int w = 0; w < PH_WAVES; ++w) {
        if (wave == w) part[lane] = w == 0 ? acc : part[lane] + acc;
        __syncthreads();
    }
    if (wave == 0 && store) H[i] = H[i] + (W ? alpha * W[i] : alpha) * part[lane];
}

template <class F>
static int pseudo_hessian_launch(helm_op *op, F U, size_t esize, const void *dU, int nsrc, long long ld, int mode, const void *dChain, const void *dE, double alpha,
                                 const void *dW, void *dH, const char *what) {
    if (!op || !dU || !dH || nsrc < 1 || ld < op->N || !(alpha >= 0.0) || mode < PH_VELOCITY || mode > PH_GARDNER) return HELM_ERR_ARG;
    if ((mode == PH_GARDNER) != (dChain != nullptr) && !dE) return HELM_ERR_ARG;       // (the chain goes with the Gardner mode alone; packed coefficients carry it)
    if (int rc = mz_handle_args(op, what)) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dChain) | ((uintptr_t)dW) | ((uintptr_t)dH)) & 7) || (((uintptr_t)dE) & 15)) return HELM_ERR_ARG;
    const size_t hbytes = (size_t)op->N * 8;
    if (ranges_overlap(dU, (size_t)nsrc * ld * esize, dH, hbytes) || (dW && ranges_overlap(dW, hbytes, dH, hbytes)) || (dChain && ranges_overlap(dChain, hbytes, dH, hbytes)) ||
        (dE && ranges_overlap(dE, (size_t)op->N * ph_ncoef(mode) * sizeof(cplx), dH, hbytes)))
        return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "%s: the handle holds no assembled operator", what);
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)(((op->nx + OP_TILE_X - 1) / OP_TILE_X) * op->nz)), block(64 * PH_WAVES);
    const cplx *c = (const cplx *)op->d_c, *E = (const cplx *)dE;
    const double *rho = (const double *)op->d_rho, *chain = (const double *)dChain, *W = (const double *)dW;
    double *H = (double *)dH;
#define PH_GO(MODE) do { \
        if (E) HELM_LAUNCH((k_pseudo_hessian<F, MODE, true>), grid, block, 0, op->stream, U, nsrc, ld, P, c, rho, chain, E, alpha, W, H); \
        else HELM_LAUNCH((k_pseudo_hessian<F, MODE, false>), grid, block, 0, op->stream, U, nsrc, ld, P, c, rho, chain, E, alpha, W, H); } while (0)
    if (mode == PH_VELOCITY) PH_GO(PH_VELOCITY);
    else if (mode == PH_BUOYANCY) PH_GO(PH_BUOYANCY);
    else PH_GO(PH_GARDNER);
#undef PH_GO
    return launched(op);
}

// H[i] += alpha (W ? W[i] : 1) sum_{s<nsrc} sum_j |sum_n E_i[j][n] U[s ld + n]|^2 for i < N: U the stored (conjugated) fields, E_i the derivative of the operator the
// handle holds with respect to the velocity of cell i (mode 0, at the handle's density), to its buoyancy (mode 1), or to its velocity with the buoyancy following
// it by dChain (mode 2: dChain N float64, NULL otherwise).  dE NULL: the coefficients are built in the kernel; else the array of
// helm_pseudo_hessian_coefficients_device for the same mode and chain.  Returns when H is complete.
extern "C" int helm_pseudo_hessian_accumulate_packed_device(helm_op *op, const void *dU, int nsrc, long long ld, int mode, const void *dChain, const void *dE,
                                                            double alpha, const void *dW, void *dH) {
    helm_tuning_refresh();
    if (((uintptr_t)dU) & 15) return HELM_ERR_ARG;
    return pseudo_hessian_launch(op, FieldC128{(const cplx *)dU}, sizeof(cplx), dU, nsrc, ld, mode, dChain, dE, alpha, dW, dH, "helm_pseudo_hessian_accumulate_device");
}
extern "C" int helm_pseudo_hessian_accumulate_packed_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int mode, const void *dChain,
                                                                const void *dE, double alpha, const void *dW, void *dH) {
    helm_tuning_refresh();
    if (!dExp || (((uintptr_t)dU32) & 7) || (((uintptr_t)dExp) & 3)) return HELM_ERR_ARG;
    return pseudo_hessian_launch(op, FieldC64{(const cplxf32 *)dU32, (const int *)dExp}, sizeof(cplxf32), dU32, nsrc, ld, mode, dChain, dE, alpha, dW, dH,
                                 "helm_pseudo_hessian_accumulate_c64_device");
}
extern "C" int helm_pseudo_hessian_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, int mode, const void *dChain, double alpha, const void *dW,
                                                     void *dH) {
    return helm_pseudo_hessian_accumulate_packed_device(op, dU, nsrc, ld, mode, dChain, nullptr, alpha, dW, dH);
}
extern "C" int helm_pseudo_hessian_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int mode, const void *dChain,
                                                         double alpha, const void *dW, void *dH) {
    return helm_pseudo_hessian_accumulate_packed_c64_device(op, dU32, dExp, nsrc, ld, mode, dChain, nullptr, alpha, dW, dH);
}

// dE[ph_ncoef(mode)][N] complex128: the coefficients E_i of every cell, what the _packed entry points read (10 planes for mode 0, 33 otherwise)
extern "C" int helm_pseudo_hessian_coefficients_device(helm_op *op, int mode, const void *dChain, void *dE) {
    helm_tuning_refresh();
    if (!op || !dE || mode < PH_VELOCITY || mode > PH_GARDNER || (mode == PH_GARDNER) != (dChain != nullptr)) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_pseudo_hessian_coefficients_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || (((uintptr_t)dChain) & 7) || (((uintptr_t)dE) & 15)) return HELM_ERR_ARG;
    if (dChain && ranges_overlap(dChain, (size_t)op->N * 8, dE, (size_t)op->N * ph_ncoef(mode) * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_pseudo_hessian_coefficients_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
    const cplx *c = (const cplx *)op->d_c;
    const double *rho = (const double *)op->d_rho, *chain = (const double *)dChain;
    if (mode == PH_VELOCITY) HELM_LAUNCH(k_pseudo_hessian_coefficients<PH_VELOCITY>, grid, dim3(256), 0, op->stream, P, c, rho, chain, (cplx *)dE);
    else if (mode == PH_BUOYANCY) HELM_LAUNCH(k_pseudo_hessian_coefficients<PH_BUOYANCY>, grid, dim3(256), 0, op->stream, P, c, rho, chain, (cplx *)dE);
    else HELM_LAUNCH(k_pseudo_hessian_coefficients<PH_GARDNER>, grid, dim3(256), 0, op->stream, P, c, rho, chain, (cplx *)dE);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the exact diagonal of the Gauss-Newton Hessian: H[i] += alpha W[i] sum_s sum_r |g_r^T (d A / d p_i) u^_s|^2
// ------------------------------------------------------------------------------------------
// With E_i the coefficients of the section above, Gamma_i[j, j'] = sum_r g_r[j] conj(g_r[j']) and Phi_i[n, n'] = sum_s u_s[n] conj(u_s[n']) over the cells of the
// 3 x 3 block around i, the double sum is Re sum conj(E[j', n']) Gamma[j, j'] E[j, n] Phi[n, n'] (frechet.gaussNewtonDiagonal states the same).  Two cells of a
// block are at most two steps apart in either direction, so Gamma and Phi are read off the autocorrelation planes at the 25 lags of (-2..2)^2, of which the
// half plane (0, 0), (0, 1), (0, 2), (1, -2..2), (2, -2..2) is stored; the other twelve are conjugates, read at the shifted cell.  k_lag_gram makes the 13 planes of
// a set of columns, k_gauss_newton_diagonal evaluates the trace per cell.
//
// k_lag_gram: C[l][i] += sum_s U[s ld + i] conj(U[s ld + i + off_l]) for the 13 lags l and every cell i whose partner i + off_l is inside the grid; the other
// entries are not touched.  The walk of k_lag_imaging with one field and a halo of two: a workgroup of LG_WAVES waves owns a tile of LG_TILE_X x LG_ROWS cells, one
// lane per cell of a row plus two halo lanes at either end.  Column s goes to wave s mod LG_WAVES, which keeps the 13 LG_ROWS sums of its lane's cells in REGISTERS
// over all its columns: per column it loads the rows z0 .. z0 + LG_ROWS + 1 of its own x (the half plane looks down only), gets the partners one and two cells
// to the left and right from the adjacent lanes and does 13 LG_ROWS complex FMAs.  Then the waves add their sums into ONE LDS tile in wave order and wave r adds
// row r to C: one writer per entry, a fixed order, no atomics -- the same bits on every run.  Per cell and column 16 (8) B times (1 + 2 / LG_ROWS)(1 + 4 / LG_TILE_X).
constexpr int LG_TILE_X = 60;       // output cells per wave along x: 64 lanes less two halo lanes at either end
constexpr int LG_ROWS = 4;          // output rows per workgroup: 104 accumulator doubles per lane
constexpr int LG_WAVES = 4;         // waves per workgroup
constexpr int LG_NLAG = 13;
static_assert(LG_ROWS <= LG_WAVES, "wave r finishes row r");
__host__ __device__ constexpr int lg_plane(int dz, int dx) { return dz == 0 ? dx : 3 + 5 * (dz - 1) + (dx + 2); }      // (dz, dx) of the stored half plane -> l

template <class F>
__global__ __launch_bounds__(64 * LG_WAVES) void k_lag_gram(F U, long long ld, int nsrc, cplx *__restrict__ C, int nz, int nx) {
    __shared__ cplx part[LG_ROWS][LG_NLAG][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + LG_TILE_X - 1) / LG_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * LG_TILE_X + lane - 2, z0 = (int)(blockIdx.x / ntx) * LG_ROWS;
    const bool xin = x >= 0 && x < nx;
    const bool store = lane >= 2 && lane < 2 + LG_TILE_X && x < nx;
    const long long N = (long long)nz * nx;
    cplx acc[LG_ROWS][LG_NLAG];
#pragma unroll
    for (int r = 0; r < LG_ROWS; ++r)
#pragma unroll
        for (int l = 0; l < LG_NLAG; ++l) acc[r][l] = cmake(0.0, 0.0);
    for (int s = wave; s < nsrc; s += LG_WAVES) {               // (wave-uniform: the lane exchanges stay complete)
        const double sc = U.scale(s);
        typename F::raw raw[LG_ROWS + 2];
#pragma unroll
        for (int r = 0; r < LG_ROWS + 2; ++r) {
            const int z = z0 + r;
            raw[r] = (xin && z < nz) ? U.load((long long)s * ld + (long long)z * nx + x) : typename F::raw{};      // (zero outside the grid: such pairs are never stored)
        }
        cplx t[LG_ROWS + 2];
#pragma unroll
        for (int r = 0; r < LG_ROWS + 2; ++r) t[r] = U.scaled(raw[r], sc);
#pragma unroll
        for (int wr = 0; wr < LG_ROWS + 2; ++wr) {              // row z0 + wr is the partner row of the output rows wr (dz = 0), wr - 1 and wr - 2
            cplx sh[5];                                         // the row at x - 2 .. x + 2 (a halo lane's missing neighbours are its own value: never stored)
            sh[2] = t[wr];
            sh[0] = cmake(__shfl_up(t[wr].x, 2, 64), __shfl_up(t[wr].y, 2, 64));
            sh[1] = cmake(__shfl_up(t[wr].x, 1, 64), __shfl_up(t[wr].y, 1, 64));
            sh[3] = cmake(__shfl_down(t[wr].x, 1, 64), __shfl_down(t[wr].y, 1, 64));
            sh[4] = cmake(__shfl_down(t[wr].x, 2, 64), __shfl_down(t[wr].y, 2, 64));
#pragma unroll
            for (int dz = 0; dz <= 2; ++dz) {
                const int r = wr - dz;
                if (r < 0 || r >= LG_ROWS) continue;
#pragma unroll
                for (int dx = (dz == 0 ? 0 : -2); dx <= 2; ++dx) cfma_conj(acc[r][lg_plane(dz, dx)], sh[dx + 2], t[r]);      // += t[r] conj(partner)
            }
        }
    }
    for (int w = 0; w < LG_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < LG_ROWS; ++r)
#pragma unroll
                for (int l = 0; l < LG_NLAG; ++l) part[r][l][lane] = w == 0 ? acc[r][l] : cadd(part[r][l][lane], acc[r][l]);
        }
        __syncthreads();
    }
    if (wave < LG_ROWS) {
        const int z = z0 + wave;
        if (store && z < nz) {
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int dz = 0; dz <= 2; ++dz)
#pragma unroll
                for (int dx = (dz == 0 ? 0 : -2); dx <= 2; ++dx) {
                    if (z + dz >= nz || x + dx < 0 || x + dx >= nx) continue;       // (the partner is outside the grid: the entry stays as it is)
                    cplx *p = C + (long long)lg_plane(dz, dx) * N + i;
                    *p = cadd(*p, part[wave][lg_plane(dz, dx)][lane]);
                }
        }
    }
}

static int lag_gram_args(helm_op *op, const void *dU, size_t esize, int nsrc, long long ld, void *dC, const char *what) {
    if (!op || !dU || !dC || nsrc < 1 || ld < op->N) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, what)) return rc;
    if (ranges_overlap(dU, (size_t)nsrc * ld * esize, dC, (size_t)op->N * LG_NLAG * sizeof(cplx))) return HELM_ERR_ARG;
    return HELM_OK;
}
static dim3 lag_gram_grid(const helm_op *op) {
    return dim3((unsigned)(((op->nx + LG_TILE_X - 1) / LG_TILE_X) * ((op->nz + LG_ROWS - 1) / LG_ROWS)));
}

// C[l][i] += sum_{s<nsrc} U[s ld + i] conj(U[s ld + i + off_l]) for the 13 lags l of the stored half plane and the cells i of the handle's grid whose partner is
// inside it: U [nsrc][ld], C [13][N] complex128.  C must not overlap U.  Returns when C is complete.
extern "C" int helm_lag_gram_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, void *dC) {
    helm_tuning_refresh();
    if (int rc = lag_gram_args(op, dU, sizeof(cplx), nsrc, ld, dC, "helm_lag_gram_accumulate_device")) return rc;
    if ((((uintptr_t)dU) | ((uintptr_t)dC)) & 15) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_lag_gram<FieldC128>, lag_gram_grid(op), dim3(64 * LG_WAVES), 0, op->stream, FieldC128{(const cplx *)dU}, ld, nsrc, (cplx *)dC, op->nz, op->nx);
    return launched(op);
}

extern "C" int helm_lag_gram_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, void *dC) {
    helm_tuning_refresh();
    if (int rc = lag_gram_args(op, dU32, sizeof(cplxf32), nsrc, ld, dC, "helm_lag_gram_accumulate_c64_device")) return rc;
    if (!dExp || (((uintptr_t)dU32) & 7) || (((uintptr_t)dExp) & 3) || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_lag_gram<FieldC64>, lag_gram_grid(op), dim3(64 * LG_WAVES), 0, op->stream, FieldC64{(const cplxf32 *)dU32, (const int *)dExp}, ld, nsrc, (cplx *)dC,
                op->nz, op->nx);
    return launched(op);
}

// k_gauss_newton_diagonal: one lane per cell.  The lane's E_i is the coefficient set of ph_coefficients (conjugated once there: the planes it is fed are those
// of the stored conjugates, and conjugating E, Gamma and Phi together leaves the real trace as it is) as a flat list of GN_NCOEF (row, column) entries over the
// slots of the block.  Gamma now couples the rows of the block, so the velocity modes carry the eight mass rows with their complex factor m_o d kappa_i / dc b_i
// (gn_mass_rows) where k_pseudo_hessian has the one real weight S_i.  Per column n' of Phi the lane loads its nine entries and forms t = E Phi[:, n']; per row j'
// that has a coefficient in that column it adds Re conj(E[j', n']) sum_j Gamma[j, j'] t[j], the nine entries of Gamma loaded where they are used.  Both loops are
// real loops over wave-uniform indices: with the 45 entries of the Hermitian Gamma held in registers beside the 33 coefficients, or with the loops unrolled (the
// compiler then hoists every load of the planes to the top), the full modes spilt 164 to 842 registers to scratch.  About 600 complex multiply-adds and 380
// cached 16-byte loads per cell, every sum in the order of the code.  One writer per cell, no atomics, no LDS, no scratch.
enum { GN_VELOCITY = 0, GN_BUOYANCY = 1, GN_GARDNER = 2, GN_MASS = 3, GN_DIAGONAL = 4 };
constexpr int GN_NCOEF = 33;        // the packed order of ph_each: c[0..8], e[0..3][0..1], k[0..3][0..3]

// the slot of the block a coefficient's row and column are: row i has the nine lags; the edge row j = i - o sits at the slot of -o and holds {lag o -> i, centre};
// the corner row holds {lag o -> i, lag (0, sx) -> i - (sz, 0), lag (sz, 0) -> i - (0, sx), centre}
__host__ __device__ constexpr int gn_row(int q) {
    if (q < 9) return 4;
    if (q < 17) {
        const int a = (q - 9) / 2, sz = a < 2 ? 2 * a - 1 : 0, sx = a < 2 ? 0 : 2 * (a - 2) - 1;
        return 3 * (-sz + 1) + (-sx + 1);
    }
    const int a = (q - 17) / 4, sz = 2 * (a / 2) - 1, sx = 2 * (a % 2) - 1;
    return 3 * (-sz + 1) + (-sx + 1);
}
__host__ __device__ constexpr int gn_col(int q) {
    if (q < 9) return q;
    if (q < 17) return (q - 9) % 2 == 0 ? 4 : gn_row(q);
    const int a = (q - 17) / 4, t = (q - 17) % 4, sz = 2 * (a / 2) - 1, sx = 2 * (a % 2) - 1;
    return t == 0 ? 4 : (t == 1 ? 3 * (-sz + 1) + 1 : (t == 2 ? 3 + (-sx + 1) : gn_row(q)));
}
// the coefficients a mode can have: the velocity star at a fixed density has its own row and one mass weight per neighbouring row; the mass term alone one per row
__host__ __device__ constexpr bool gn_live(int mode, int q) {
    if (mode == GN_VELOCITY) return q < 9 || gn_col(q) == 4;
    if (mode == GN_MASS) return gn_col(q) == 4;
    return true;
}

// entry (p, q) of a cell's block from the planes of k_lag_gram, sum over the columns of u[i + o_p] conj(u[i + o_q]); zero where either cell is outside the grid
// (no coefficient is non-zero there: an interior row has every neighbour inside)
__device__ __forceinline__ cplx gn_gram(const cplx *__restrict__ C, long long N, int nz, int nx, int iz, int ix, int p, int q) {
    const int az = iz + p / 3 - 1, ax = ix + p % 3 - 1, bz = iz + q / 3 - 1, bx = ix + q % 3 - 1;
    if (az < 0 || az >= nz || ax < 0 || ax >= nx || bz < 0 || bz >= nz || bx < 0 || bx >= nx) return cmake(0.0, 0.0);
    const int dz = bz - az, dx = bx - ax;
    if (dz > 0 || (dz == 0 && dx >= 0)) return C[(long long)lg_plane(dz, dx) * N + (long long)az * nx + ax];
    return cconj(C[(long long)lg_plane(-dz, -dx) * N + (long long)bz * nx + bx]);
}

// the mass weight m_o w of cell i in the interior rows j = i - o around it (conjugated, as ph_coefficients leaves its own): entries 9 + 2 a and 17 + 4 a
__device__ __forceinline__ void gn_mass_rows(const MzParams &P, int iz, int ix, cplx w, cplx (&e)[GN_NCOEF]) {
    auto put = [&](int sz, int sx, double m, cplx &out) {
        const int jz = iz - sz, jx = ix - sx;
        if (jz >= 1 && jz <= P.nz - 2 && jx >= 1 && jx <= P.nx - 2) out = cconj(cscale(w, m));
    };
    put(-1, 0, MZ_WD, e[9]); put(1, 0, MZ_WD, e[11]); put(0, -1, MZ_WD, e[13]); put(0, 1, MZ_WD, e[15]);
    put(-1, -1, MZ_WE, e[17]); put(-1, 1, MZ_WE, e[21]); put(1, -1, MZ_WE, e[25]); put(1, 1, MZ_WE, e[29]);
}

// fn(std::integral_constant<int, 0>) .. fn(std::integral_constant<int, N - 1>) in order: a loop whose index is a constant expression in its body
template <class FN, int... I>
__device__ __forceinline__ void gn_for_each(FN &&fn, std::integer_sequence<int, I...>) { (fn(std::integral_constant<int, I>{}), ...); }
template <int N, class FN>
__device__ __forceinline__ void gn_for(FN &&fn) { gn_for_each(fn, std::make_integer_sequence<int, N>{}); }

template <int MODE>
__device__ __forceinline__ void gn_coefficients(const MzParams &P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ chain,
                                                int iz, int ix, cplx (&e)[GN_NCOEF]) {
#pragma unroll
    for (int q = 0; q < GN_NCOEF; ++q) e[q] = cmake(0.0, 0.0);
    const long long i = (long long)iz * P.nx + ix;
    if (MODE == GN_BUOYANCY || MODE == GN_GARDNER) {
        PhCoef E;
        ph_coefficients<MODE == GN_BUOYANCY ? PH_BUOYANCY : PH_GARDNER>(P, c, rho, chain, iz, ix, E);
        ph_each<PH_BUOYANCY>(E, [&](int q, cplx &v) { e[q] = v; });
        return;
    }
    const cplx w = cscale(mz_kappa_dc(P, c[i]), 1.0 / rho[i]);          // d K_i / d c_i at the density of the handle
    if (MODE == GN_VELOCITY) {
        PhCoef E;
        ph_coefficients<PH_VELOCITY>(P, c, rho, chain, iz, ix, E);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = E.c[k];
    } else if (iz >= 1 && iz <= P.nz - 2 && ix >= 1 && ix <= P.nx - 2) {
        e[4] = cconj(cscale(w, MZ_WC));
    }
    gn_mass_rows(P, iz, ix, w, e);
}

template <int MODE>
__global__ __launch_bounds__(64) void k_gauss_newton_diagonal(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ chain,
                                                              const cplx *__restrict__ Cu, const cplx *__restrict__ Cg, double alpha, const double *__restrict__ W,
                                                              double *__restrict__ H) {
    const int nz = P.nz, nx = P.nx;
    const long long N = (long long)nz * nx, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double wgt = W ? alpha * W[i] : alpha;
    if (MODE == GN_DIAGONAL) {                                  // the diagonal weight of 'scaler': the zero-lag planes alone, |w_i|^2 in W
        H[i] = H[i] + wgt * (Cg[i].x * Cu[i].x);
        return;
    }
    const int iz = (int)(i / nx), ix = (int)(i % nx);
    cplx e[GN_NCOEF];
    gn_coefficients<MODE>(P, c, rho, chain, iz, ix, e);
    double h = 0.0;
#pragma unroll 1
    for (int n2 = 0; n2 < 9; ++n2) {                            // (a real loop: unrolled, the compiler hoists every load of the planes to the top and spills)
        cplx phi[9], t[9];                                      // (compile-time indices inside: e, phi and t stay in registers)
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            phi[n] = gn_gram(Cu, N, nz, nx, iz, ix, n, n2);
            t[n] = cmake(0.0, 0.0);
        }
        gn_for<GN_NCOEF>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            if constexpr (gn_live(MODE, q)) cfma(t[gn_row(q)], e[q], phi[gn_col(q)]);
        });
#pragma unroll 1
        for (int j2 = 0; j2 < 9; ++j2) {                        // (a real loop too: the entries of Gamma are loaded where they are used)
            cplx ec = cmake(0.0, 0.0);
            bool any = false;
            gn_for<GN_NCOEF>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                if (gn_live(MODE, q) && gn_row(q) == j2 && gn_col(q) == n2) { ec = e[q]; any = true; }      // (uniform over the wave; at most one q)
            });
            if (!any) continue;
            cplx s = cmake(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 9; ++j) cfma(s, gn_gram(Cg, N, nz, nx, iz, ix, j, j2), t[j]);
            h = fma(ec.x, s.x, h);
            h = fma(ec.y, s.y, h);                              // Re conj(e) s
        }
    }
    H[i] = H[i] + wgt * h;
}

// H[i] += alpha (W ? W[i] : 1) Re tr(E_i^H Gamma_i E_i Phi_i) for i < N: Phi from dCu and Gamma from dCg, two sets of 13 planes of helm_lag_gram_accumulate_device
// (of the stored forward fields and of the receiver columns solved with the transposed operator, as they are).  E_i the derivative of the operator the handle holds
// with respect to the velocity of cell i (mode 0, at the handle's density), to its buoyancy (mode 1), to its velocity with the buoyancy following it by dChain
// (mode 2: dChain N float64, NULL otherwise), its mass term alone (mode 3: linearisation='operator'), or the unit diagonal (mode 4: 'scaler', the weight |w_i|^2
// in dW; H[i] += alpha W[i] Gamma_i[i, i] Phi_i[i, i]).  dW, dH: N float64; alpha >= 0.  Returns when H is complete.
extern "C" int helm_gauss_newton_diagonal_device(helm_op *op, int mode, const void *dChain, const void *dW, const void *dCu, const void *dCg, double alpha, void *dH) {
    helm_tuning_refresh();
    if (!op || !dCu || !dCg || !dH || !(alpha >= 0.0) || mode < GN_VELOCITY || mode > GN_DIAGONAL || (mode == GN_GARDNER) != (dChain != nullptr)) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_gauss_newton_diagonal_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dChain) | ((uintptr_t)dW) | ((uintptr_t)dH)) & 7) || ((((uintptr_t)dCu) | ((uintptr_t)dCg)) & 15)) return HELM_ERR_ARG;
    const size_t hbytes = (size_t)op->N * 8, cbytes = (size_t)op->N * LG_NLAG * sizeof(cplx);
    if (ranges_overlap(dCu, cbytes, dH, hbytes) || ranges_overlap(dCg, cbytes, dH, hbytes) || (dW && ranges_overlap(dW, hbytes, dH, hbytes)) ||
        (dChain && ranges_overlap(dChain, hbytes, dH, hbytes)))
        return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_gauss_newton_diagonal_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 63) / 64)), block(64);
    const cplx *c = (const cplx *)op->d_c, *Cu = (const cplx *)dCu, *Cg = (const cplx *)dCg;
    const double *rho = (const double *)op->d_rho, *chain = (const double *)dChain, *W = (const double *)dW;
    double *H = (double *)dH;
#define GN_GO(MODE) HELM_LAUNCH(k_gauss_newton_diagonal<MODE>, grid, block, 0, op->stream, P, c, rho, chain, Cu, Cg, alpha, W, H)
    if (mode == GN_VELOCITY) GN_GO(GN_VELOCITY);
    else if (mode == GN_BUOYANCY) GN_GO(GN_BUOYANCY);
    else if (mode == GN_GARDNER) GN_GO(GN_GARDNER);
    else if (mode == GN_MASS) GN_GO(GN_MASS);
    else GN_GO(GN_DIAGONAL);
#undef GN_GO
    return launched(op);
}
