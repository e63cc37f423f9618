// Vector kernels that the three solve drivers share (capi.hip, solve_direct.hip, krylov.hip): right-hand side in, wavefield out, norms.
// grid.x over the points with a grid-stride loop, grid.y = right-hand side.
#include "helm_internal.hpp"
#include <algorithm>
#include <type_traits>

namespace {

// out[b*out_ld + out_off + i] = scale[i] * (premul * rhs[b*rhs_ld + row_off + i] - sub[b*N + i])
// sub may be null.  T is the scale: void (none; the pointer is not read), cplx (1 / diagonal) or double (inverse row norms, applied as a real factor).
template <class T>
__global__ __launch_bounds__(256) void k_prep_rhs(const cplx *__restrict__ rhs, long long rhs_ld, long long row_off, cplx premul,
                                                  const cplx *__restrict__ sub, const T *__restrict__ scale,
                                                  cplx *__restrict__ out, long long out_ld, long long out_off, long long N) {
    const int b = blockIdx.y;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        cplx v = cmul(premul, rhs[(long long)b * rhs_ld + row_off + i]);
        if (sub) v = csub(v, sub[(long long)b * N + i]);
        if constexpr (std::is_same<T, cplx>::value) v = cmul(scale[i], v);
        if constexpr (std::is_same<T, double>::value) v = cscale(v, scale[i]);
        out[(long long)b * out_ld + out_off + i] = v;
    }
}

// partial (a, a)
__global__ __launch_bounds__(256) void k_norm2(const cplx *__restrict__ a, long long N, double *__restrict__ part, int nblk) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    double s[1] = {0.0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x)
        s[0] += cabs2(a[(long long)b * N + i]);
    block_sum<1>(s, red);
    if (threadIdx.x == 0) part[((long long)b * 4) * nblk + blockIdx.x] = s[0];
}

// out = sign * |in| as a complex number with zero imaginary part (attainable-accuracy estimate of the coupled system)
__global__ __launch_bounds__(256) void k_abs_cplx(const cplx *__restrict__ in, cplx *__restrict__ out, long long n, double sign) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const cplx v = in[i];
        out[i] = cmake(sign * hypot(v.x, v.y), 0.0);
    }
}

// U = conj(x), input and output both strided / offset
__global__ __launch_bounds__(256) void k_finish_ex(const cplx *__restrict__ x, long long x_ld, long long x_off, cplx *__restrict__ U, long long u_ld,
                                                   long long row_off, long long N) {
    const int b = blockIdx.y;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x)
        U[(long long)b * u_ld + row_off + i] = cconj(x[(long long)b * x_ld + x_off + i]);
}

// v[b][i] *= rs[i] in place (row equilibration of a residual before a refinement pass of the coupled system)
__global__ __launch_bounds__(256) void k_rowscale_inplace(cplx *v, const double *__restrict__ rs, long long NV) {
    const int b = blockIdx.y;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < NV; i += (long long)gridDim.x * blockDim.x) {
        cplx *p = v + (long long)b * NV + i;
        *p = cscale(*p, rs[i]);
    }
}

}  // namespace

int helm_vec_num_blocks(const helm_op *op) { return vec_blocks(op->Nv > 0 ? op->Nv : op->N); }

// N rows of every right-hand side (one field of the operator); at most one of scale / rs
int helm_launch_prep_rhs(helm_op *op, const cplx *dRHS, long long rhs_ld, long long row_off, cplx premul, const cplx *sub, const cplx *scale, const double *rs,
                         cplx *out, long long out_ld, long long out_off, int nrhs) {
    const dim3 grid(vec_blocks(op->N), nrhs);
    if (rs) HELM_LAUNCH(k_prep_rhs<double>, grid, dim3(256), 0, op->stream, dRHS, rhs_ld, row_off, premul, sub, rs, out, out_ld, out_off, op->N);
    else if (scale) HELM_LAUNCH(k_prep_rhs<cplx>, grid, dim3(256), 0, op->stream, dRHS, rhs_ld, row_off, premul, sub, scale, out, out_ld, out_off, op->N);
    else HELM_LAUNCH(k_prep_rhs<void>, grid, dim3(256), 0, op->stream, dRHS, rhs_ld, row_off, premul, sub, (const void *)nullptr, out, out_ld, out_off, op->N);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

int helm_launch_finish(helm_op *op, const cplx *x, long long x_ld, long long x_off, cplx *dU, long long u_ld, long long row_off, int nrhs) {
    dim3 grid(vec_blocks(op->N), nrhs);
    HELM_LAUNCH(k_finish_ex, grid, dim3(256), 0, op->stream, x, x_ld, x_off, dU, u_ld, row_off, op->N);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

int helm_launch_norm2(helm_op *op, const cplx *a, int nrhs) {
    dim3 grid(vec_blocks(op->Nv), nrhs);
    HELM_LAUNCH(k_norm2, grid, dim3(256), 0, op->stream, a, op->Nv, (double *)op->d_part, (int)grid.x);
    return HELM_OK;
}

int helm_launch_abs(helm_op *op, const cplx *in, cplx *out, long long n, double sign) {
    HELM_LAUNCH(k_abs_cplx, dim3((unsigned)std::min<long long>((n + 255) / 256, 1 << 20)), dim3(256), 0, op->stream, in, out, n, sign);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

int helm_launch_rowscale_inplace(helm_op *op, cplx *v, const double *rs, long long NV, int nrhs) {
    HELM_LAUNCH(k_rowscale_inplace, dim3(vec_blocks(NV), nrhs), dim3(256), 0, op->stream, v, rs, NV);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}
