// The optional complex64 store of forward wavefields (zephyr_amd/fieldstore.py, config key fieldsDtype='complex64'): a wavefield column s is kept as
// complex64 values x * 2^-e_s with ONE power-of-two scale per column, e_s the binary exponent of the column's largest component
// (2^e_s <= max_i max(|Re|, |Im|) < 2^(e_s+1), clamped to +-1021; 0 for a zero column).  The scaling is exact, so the only rounding is the conversion to
// fp32 (2^-24 relative where the scaled value is a normal fp32 number), and fields of any magnitude survive where a plain conversion would overflow or
// flush.  A consumer reads (double)x^ * 2^e_s, exact again.  Four kernels: the pack, and the imaging, energy and sampling loops of kernels.hip with the forward
// field read in this format.  The complex128 paths never come here.
#include "helm_internal.hpp"
#include <algorithm>

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

// G[i] += scaler[i] * sum_s (UF32[s][i] * 2^e_s) * UB[s][i]: k_imaging (kernels.hip) with the forward field read from the complex64 store.  The
// rescaling is exact, so the sum is k_imaging's sum of the unpacked field, term for term.
__global__ __launch_bounds__(256) void k_imaging_c64(const cplxf32 *__restrict__ uf, const int *__restrict__ exps, const cplx *__restrict__ ub, int nsrc,
                                                     const cplx *__restrict__ scaler, cplx *__restrict__ g, long long N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        cplx acc = cmake(0.0, 0.0);
        for (int s = 0; s < nsrc; ++s) {
            const double sc = pow2(exps[s]);
            const cplxf32 f = uf[(long long)s * N + i];
            cfma(acc, cmake((double)f.x * sc, (double)f.y * sc), ub[(long long)s * N + i]);
        }
        cplx gv = g[i];
        cfma(gv, scaler[i], acc);
        g[i] = gv;
    }
}

// E[i] += alpha (W ? W[i] : 1) sum_s |U32[s ld + i] * 2^e_s|^2: k_energy (kernels.hip) with the field read from the complex64 store, 8-byte loads.  Each
// component is scaled in fp64 before it is squared (exact, and 2^(2 e_s) alone would overflow where the field does not), so the sum is k_energy's sum of
// the unpacked field, term for term.
__global__ __launch_bounds__(256) void k_energy_c64(const cplxf32 *__restrict__ U, const int *__restrict__ exps, int nsrc, long long ld, double alpha,
                                                    const double *__restrict__ W, double *__restrict__ E, long long N) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const cplxf32 *col = U + i;
        double acc = 0.0;
        int s = 0;
        for (; s + HELM_ENERGY_UNROLL <= nsrc; s += HELM_ENERGY_UNROLL) {
            cplxf32 f[HELM_ENERGY_UNROLL];
#pragma unroll
            for (int j = 0; j < HELM_ENERGY_UNROLL; ++j) f[j] = col[(long long)(s + j) * ld];
#pragma unroll
            for (int j = 0; j < HELM_ENERGY_UNROLL; ++j) {
                const double sc = pow2(exps[s + j]);
                const double re = (double)f[j].x * sc, im = (double)f[j].y * sc;
                acc += re * re + im * im;
            }
        }
        for (; s < nsrc; ++s) {
            const cplxf32 f = col[(long long)s * ld];
            const double sc = pow2(exps[s]);
            const double re = (double)f.x * sc, im = (double)f.y * sc;
            acc += re * re + im * im;
        }
        const double w = W ? alpha * W[i] : alpha;
        E[i] = E[i] + w * acc;
    }
}

// k_sample_acc (kernels.hip) with U read from the complex64 store: out[r][s] = beta out[r][s] + alpha sum_k val[k] (U32[s][col[k]] * 2^e_s) over the
// entries of sparse row r + s * row_stride
__global__ __launch_bounds__(256) void k_sample_acc_c64(const cplxf32 *__restrict__ U, const int *__restrict__ exps, int nsrc, long long ld,
                                                        const long long *__restrict__ rowptr, const long long *__restrict__ col, const cplx *__restrict__ val,
                                                        int nrec, long long row_stride, cplx alpha, cplx beta, int beta0, cplx *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nrec * nsrc) return;
    const int r = (int)(t / nsrc), sidx = (int)(t % nsrc);
    const long long row = r + sidx * row_stride;
    const double sc = pow2(exps[sidx]);
    cplx acc = cmake(0.0, 0.0);
    for (long long k = rowptr[row]; k < rowptr[row + 1]; ++k) {
        const cplxf32 f = U[(long long)sidx * ld + col[k]];
        cfma(acc, val[k], cmake((double)f.x * sc, (double)f.y * sc));
    }
    cplx o = cmul(alpha, acc);
    if (!beta0) cfma(o, beta, out[t]);
    out[t] = o;
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

extern "C" int helm_imaging_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, const void *dUB, int nsrc, const void *dScaler, void *dG) {
    helm_tuning_refresh();
    if (!op || !dUF32 || !dExp || !dUB || !dScaler || !dG || nsrc < 1) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const unsigned blocks = (unsigned)std::min<long long>((op->N + 255) / 256, 1 << 20);
    HELM_LAUNCH(k_imaging_c64, dim3(blocks), dim3(256), 0, op->stream, (const cplxf32 *)dUF32, (const int *)dExp, (const cplx *)dUB, nsrc,
                (const cplx *)dScaler, (cplx *)dG, op->N);
    HIP_TRY(op, hipGetLastError());
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}

extern "C" int helm_energy_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, double alpha, const void *dW, void *dE) {
    helm_tuning_refresh();
    if (!op || !dU32 || !dExp || !dE || nsrc < 1 || ld < op->N || !(alpha >= 0.0)) return HELM_ERR_ARG;       // (!(alpha >= 0): negative or NaN)
    if ((((uintptr_t)dU32) & 7) || (((uintptr_t)dExp) & 3) || (((uintptr_t)dE) & 7) || (((uintptr_t)dW) & 7)) return HELM_ERR_ARG;       // (8-byte loads of U32; doubles)
    HIP_TRY(op, hipSetDevice(op->device));
    const unsigned blocks = (unsigned)std::min<long long>((op->N + 255) / 256, HELM_ENERGY_MAX_BLOCKS);
    HELM_LAUNCH(k_energy_c64, dim3(blocks), dim3(256), 0, op->stream, (const cplxf32 *)dU32, (const int *)dExp, nsrc, ld, alpha, (const double *)dW,
                (double *)dE, op->N);
    HIP_TRY(op, hipGetLastError());
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}

extern "C" int helm_sample_rows_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, const void *d_rowptr, const void *d_col,
                                           const void *d_val, int nrec, long long row_stride, double alpha_re, double alpha_im, double beta_re, double beta_im,
                                           void *d_out) {
    helm_tuning_refresh();
    if (!op || !dU32 || !dExp || !d_rowptr || !d_col || !d_val || !d_out || nsrc < 1 || nrec < 1 || ld < 1) return HELM_ERR_ARG;
    if (row_stride != 0 && row_stride < nrec) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const long long tot = (long long)nrec * nsrc;
    const int beta0 = (beta_re == 0.0 && beta_im == 0.0) ? 1 : 0;
    HELM_LAUNCH(k_sample_acc_c64, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, op->stream, (const cplxf32 *)dU32, (const int *)dExp, nsrc, ld,
                (const long long *)d_rowptr, (const long long *)d_col, (const cplx *)d_val, nrec, row_stride, cmake(alpha_re, alpha_im), cmake(beta_re, beta_im),
                beta0, (cplx *)d_out);
    HIP_TRY(op, hipGetLastError());
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}
