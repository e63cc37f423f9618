// Grid transfer of the multiscale family (zephyr/backend/interpolation.py:180-205, SplineGridInterpolator): a field on a regular
// (nz_a, nx_a) grid is carried to another regular grid with the same origin by not-a-knot cubic spline interpolation along each axis
// (what scipy's RectBivariateSpline(kx=3, ky=3, s=0) computes), evaluation points beyond the input's extent clamped to its edge.
//
// The transfer is separable, T = Wz (x) Wx, and each 1-D operator is a dense matrix whose rows decay geometrically away from the diagonal
// (a factor 2 - sqrt(3) per input node).  helm_regrid_axis builds it on the host -- a banded collocation solve per output point -- and keeps
// a window of at most 64 taps per output point (taps below 2^-60 of the row's largest dropped).  A plan uploads both axes' windows once;
// applying it is two windowed passes on the GPU:
//   k_regrid_z contracts the row axis: one output per lane, lanes along the contiguous axis, so every tap is one coalesced row of a wave;
//   k_regrid_x contracts the contiguous axis: a workgroup owns a tile of output columns, keeps its taps in registers, and streams the rows
//              of the fields through LDS (each input element read from HBM once per pass).
// The pass that shrinks the data most runs first (fewer FMAs on the intermediate), the second writes the caller's output through the
// epilogue out = beta out + mul (.) (gain T in).
#include "helm_internal.hpp"
#include <algorithm>
#include <vector>

namespace {

const int kRegridMaxTaps = 64;

// values of the k + 1 B-splines that are nonzero on [t[m], t[m+1]) at x (de Boor's recurrence)
void bspline_values(const std::vector<double> &t, int m, double x, double *N) {
    const int k = 3;
    double left[k + 1], right[k + 1];
    N[0] = 1.0;
    for (int j = 1; j <= k; ++j) {
        left[j] = x - t[m + 1 - j];
        right[j] = t[m + j] - x;
        double saved = 0.0;
        for (int r = 0; r < j; ++r) {
            const double tmp = N[r] / (right[r + 1] + left[j - r]);
            N[r] = saved + right[r + 1] * tmp;
            saved = left[j - r] * tmp;
        }
        N[j] = saved;
    }
}

// interval m (3 <= m <= n-1) of the not-a-knot knot vector that holds x
int knot_interval(const std::vector<double> &t, int n, double x) {
    int lo = 3, hi = n - 1;
    if (x >= t[n - 1]) return n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (t[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Row j of the 1-D transfer for nodes i h_in (i < n_in) -> points j h_out (j < n_out), as windows: start[j] and W taps each.
// Returns W (>= 1) or < 0.
int axis_windows(int n, double h_in, int n_out, double h_out, std::vector<int> &start, std::vector<double> &taps) {
    if (n < 4 || n_out < 1 || !(h_in > 0) || !(h_out > 0)) return HELM_ERR_ARG;
    std::vector<double> x(n), t(n + 4);
    for (int i = 0; i < n; ++i) x[i] = i * h_in;
    // not-a-knot knots (scipy make_interp_spline, k = 3): x0 four times, x[2 .. n-3], x[n-1] four times
    for (int i = 0; i < 4; ++i) { t[i] = x[0]; t[n + i] = x[n - 1]; }
    for (int i = 2; i <= n - 3; ++i) t[i + 2] = x[i];
    // collocation matrix A[i][j] = B_j(x_i): band of half-width 3, LU without pivoting (B-spline collocation matrices are totally positive)
    const int bw = 3, ld = 2 * bw + 1;
    std::vector<double> A((size_t)n * ld, 0.0);
    auto a = [&](int i, int j) -> double & { return A[(size_t)i * ld + (j - i + bw)]; };
    for (int i = 0; i < n; ++i) {
        const int m = knot_interval(t, n, x[i]);
        double N[4];
        bspline_values(t, m, x[i], N);
        for (int r = 0; r < 4; ++r) {
            const int j = m - 3 + r;
            if (std::abs(j - i) > bw) { if (N[r] != 0.0) return HELM_ERR_STATE; continue; }
            a(i, j) = N[r];
        }
    }
    for (int kk = 0; kk < n; ++kk) {
        const double piv = a(kk, kk);
        if (piv == 0.0) return HELM_ERR_STATE;
        for (int i = kk + 1; i <= std::min(kk + bw, n - 1); ++i) {
            const double l = a(i, kk) / piv;
            a(i, kk) = l;
            for (int j = kk + 1; j <= std::min(kk + bw, n - 1); ++j) a(i, j) -= l * a(kk, j);
        }
    }
    // weights of point p: w^T = b(p)^T A^-1, i.e. U^T y = b, L^T w = y
    const double xmax = x[n - 1];
    std::vector<double> w(n);
    std::vector<int> first(n_out), last(n_out);
    std::vector<std::vector<double>> rows(n_out);
    int W = 1;
    for (int jo = 0; jo < n_out; ++jo) {
        const double p = std::min(std::max(jo * h_out, 0.0), xmax);
        const int m = knot_interval(t, n, p);
        double N[4];
        bspline_values(t, m, p, N);
        std::fill(w.begin(), w.end(), 0.0);
        for (int r = 0; r < 4; ++r) w[m - 3 + r] = N[r];
        for (int j = m - 3; j < n; ++j) {             // U^T y = b (lower triangular; b is zero before m - 3)
            double s = w[j];
            for (int i = std::max(m - 3, j - bw); i < j; ++i) s -= a(i, j) * w[i];
            w[j] = s / a(j, j);
        }
        for (int i = n - 1; i >= 0; --i) {            // L^T w = y (unit upper triangular)
            double s = w[i];
            for (int j = i + 1; j <= std::min(i + bw, n - 1); ++j) s -= a(j, i) * w[j];
            w[i] = s;
        }
        double amax = 0.0;
        for (int i = 0; i < n; ++i) amax = std::max(amax, std::abs(w[i]));
        const double cut = std::ldexp(amax, -60);
        int f = 0, l = n - 1;
        while (std::abs(w[f]) < cut) ++f;
        while (std::abs(w[l]) < cut) --l;
        while (l - f + 1 > kRegridMaxTaps) {          // (the window is at most 64 wide: the smaller end goes)
            if (std::abs(w[f]) <= std::abs(w[l])) ++f; else --l;
        }
        rows[jo].assign(w.begin() + f, w.begin() + l + 1);
        for (double &v : rows[jo]) if (std::abs(v) < cut) v = 0.0;
        first[jo] = f; last[jo] = l;
        W = std::max(W, l - f + 1);
    }
    start.assign(n_out, 0);
    taps.assign((size_t)n_out * W, 0.0);
    for (int jo = 0; jo < n_out; ++jo) {
        const int s = std::min(first[jo], n - W);     // every window lies inside the input: W reads from start[j] are in bounds
        start[jo] = s;
        for (size_t r = 0; r < rows[jo].size(); ++r) taps[(size_t)jo * W + (first[jo] - s) + r] = rows[jo][r];
    }
    return W;
}

// Windows of the transpose of axis_windows' operator: row j (an input node of the forward axis) holds taps[i][j - start[i]] for the contiguous
// range of forward outputs i that touch it.  The range comes from the forward windows' nonzero taps (min and max i per j), not from the
// starts: those are not monotone (edge windows are shifted, taps below the cut are zeroed inside a window, the cap trims one end).  A node no
// output touches gets an all-zero window.  Returns WT (>= 1), HELM_ERR_UNSUPPORTED when it exceeds 64, or axis_windows' error.
int axis_windows_t(int n, double h_in, int n_out, double h_out, std::vector<int> &start_t, std::vector<double> &taps_t) {
    std::vector<int> s;
    std::vector<double> w;
    const int W = axis_windows(n, h_in, n_out, h_out, s, w);
    if (W < 0) return W;
    std::vector<int> lo(n, n_out), hi(n, -1);
    for (int i = 0; i < n_out; ++i)
        for (int t = 0; t < W; ++t)
            if (w[(size_t)i * W + t] != 0.0) { const int j = s[i] + t; lo[j] = std::min(lo[j], i); hi[j] = std::max(hi[j], i); }
    int WT = 1;
    for (int j = 0; j < n; ++j) WT = std::max(WT, hi[j] - lo[j] + 1);
    if (WT > kRegridMaxTaps) return HELM_ERR_UNSUPPORTED;
    start_t.assign(n, 0);
    taps_t.assign((size_t)n * WT, 0.0);
    for (int j = 0; j < n; ++j) {
        if (hi[j] < lo[j]) continue;
        const int st = std::min(lo[j], n_out - WT);   // (WT <= n_out: every window lies inside the forward's outputs)
        start_t[j] = st;
        for (int t = 0; t < WT; ++t) {
            const int i = st + t, tt = j - s[i];
            if (tt >= 0 && tt < W) taps_t[(size_t)j * WT + t] = w[(size_t)i * W + tt];
        }
    }
    // an untouched node (all but every s-th one at an integer scale s) takes the start of its nearest touched neighbour below, the leading ones that of the
    // first touched node: its zero window then lies where its neighbours read, and a column tile's LDS span stays about tile / scale + WT
    int first = 0;
    while (first < n && hi[first] < lo[first]) ++first;
    if (first < n) {
        int near = start_t[first];
        for (int j = 0; j < n; ++j) {
            if (hi[j] >= lo[j]) near = start_t[j];
            else start_t[j] = near;
        }
    }
    return WT;
}

__device__ inline void regrid_put(cplx *out, long long o, long long i, double ar, double ai, bool fin, cplx gain, double beta, const cplx *mul) {
    cplx v = cmake(ar, ai);
    if (fin) {
        v = cmul(gain, v);
        if (mul) v = cmul(mul[i], v);
        if (beta != 0.0) { const cplx b = out[o]; v = cmake(fma(beta, b.x, v.x), fma(beta, b.y, v.y)); }
    }
    out[o] = v;
}

// contracts the row axis: out[f][zo][c] = sum_t w[zo][t] in[f][start[zo] + t][c]; lanes along c
__global__ void __launch_bounds__(256) k_regrid_z(const cplx *in, long long ifs, long long ies, cplx *out, long long ofs, long long oes, int k,
                                                  int nzo, int ncol, const int *start, const double *taps, int W, int fin, cplx gain, double beta,
                                                  const cplx *mul) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int zo = blockIdx.y * 4 + threadIdx.y;
    if (c >= ncol || zo >= nzo) return;
    const int s = start[zo];
    const double *w = taps + (long long)zo * W;
    const long long step = (long long)ncol * ies;
    const long long i = (long long)zo * ncol + c;
    for (int f = blockIdx.z; f < k; f += gridDim.z) {
        const cplx *src = in + f * ifs + ((long long)s * ncol + c) * ies;
        double ar = 0.0, ai = 0.0;
        for (int t = 0; t < W; ++t) {
            const cplx v = src[t * step];
            ar = fma(w[t], v.x, ar);
            ai = fma(w[t], v.y, ai);
        }
        regrid_put(out, f * ofs + i * oes, i, ar, ai, fin != 0, gain, beta, mul);
    }
}

// contracts the contiguous axis: out[f][r][xo] = sum_t w[xo][t] in[f][r][start[xo] + t].  A workgroup owns the output columns of one tile
// (one per lane, taps in registers) and walks rows (f, r); each row's input span [lo, lo + len) of the tile is staged in LDS first.
template <int MW>
__global__ void __launch_bounds__(256) k_regrid_x(const cplx *in, long long ifs, long long ies, cplx *out, long long ofs, long long oes, int k,
                                                  int nrow, int nxi, int nxo, const int *start, const double *taps, int W, const int *tile_lo,
                                                  const int *tile_len, int fin, cplx gain, double beta, const cplx *mul) {
    extern __shared__ cplx seg[];
    const int xo = blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = xo < nxo;
    const int lo = tile_lo[blockIdx.x], len = tile_len[blockIdx.x];
    double w[MW];
    int off = 0;
#pragma unroll
    for (int t = 0; t < MW; ++t) w[t] = (act && t < W) ? taps[(long long)xo * W + t] : 0.0;
    if (act) off = start[xo] - lo;
    const long long rows = (long long)k * nrow;
    for (long long rr = blockIdx.y; rr < rows; rr += gridDim.y) {
        const long long f = rr / nrow, r = rr - f * nrow;
        const cplx *src = in + f * ifs + (r * nxi + lo) * ies;
        __syncthreads();
        for (int j = threadIdx.x; j < len; j += blockDim.x) seg[j] = src[j * ies];
        __syncthreads();
        if (!act) continue;
        double ar = 0.0, ai = 0.0;
#pragma unroll
        for (int t = 0; t < MW; ++t) {
            if (t < W) {
                const cplx v = seg[off + t];
                ar = fma(w[t], v.x, ar);
                ai = fma(w[t], v.y, ai);
            }
        }
        const long long i = r * nxo + xo;
        regrid_put(out, f * ofs + i * oes, i, ar, ai, fin != 0, gain, beta, mul);
    }
}

}  // namespace

struct helm_regrid {
    int device = 0, nz_a = 0, nx_a = 0, nz_b = 0, nx_b = 0;
    int Wz = 0, Wx = 0, tw = 256, xtiles = 0, xspan = 0;
    bool z_first = true;
    int *d_sz = nullptr, *d_sx = nullptr, *d_xlo = nullptr, *d_xlen = nullptr;
    double *d_wz = nullptr, *d_wx = nullptr;
    helm_op io;                       // device and stream of the plan's own work (host arrays staged through the library's pinned chunks)
};

extern "C" int helm_regrid_axis(int n_in, double h_in, int n_out, double h_out, int *start, double *taps, int cap) {
    std::vector<int> s;
    std::vector<double> w;
    const int W = axis_windows(n_in, h_in, n_out, h_out, s, w);
    if (W < 0) { helm_set_error(nullptr, "helm_regrid_axis: needs n_in >= 4, n_out >= 1 and positive spacings"); return W; }
    if (start) std::copy(s.begin(), s.end(), start);
    if (taps) {
        if ((size_t)cap < w.size()) { helm_set_error(nullptr, "helm_regrid_axis: taps holds fewer than n_out * W entries"); return HELM_ERR_ARG; }
        std::copy(w.begin(), w.end(), taps);
    }
    return W;
}

extern "C" int helm_regrid_axis_t(int n_in, double h_in, int n_out, double h_out, int *start, double *taps, int cap) {
    std::vector<int> s;
    std::vector<double> w;
    const int WT = axis_windows_t(n_in, h_in, n_out, h_out, s, w);
    if (WT == HELM_ERR_UNSUPPORTED) { helm_set_error(nullptr, "helm_regrid_axis_t: an input node is touched by more than 64 outputs (an up-sampling axis this dense has no transposed plan)"); return WT; }
    if (WT < 0) { helm_set_error(nullptr, "helm_regrid_axis_t: needs n_in >= 4, n_out >= 1 and positive spacings"); return WT; }
    if (start) std::copy(s.begin(), s.end(), start);
    if (taps) {
        if ((size_t)cap < w.size()) { helm_set_error(nullptr, "helm_regrid_axis_t: taps holds fewer than n_in * WT entries"); return HELM_ERR_ARG; }
        std::copy(w.begin(), w.end(), taps);
    }
    return WT;
}

extern "C" void helm_regrid_destroy(helm_regrid *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->io.stream) { (void)hipStreamSynchronize(p->io.stream); helm_stream_release(p->device, 0, p->io.stream); }
    hipFree(p->d_sz); hipFree(p->d_sx); hipFree(p->d_xlo); hipFree(p->d_xlen); hipFree(p->d_wz); hipFree(p->d_wx);
    delete p;
}

template <class T>
static int upload_small(T **dst, const std::vector<T> &v) {
    if (hipMalloc(dst, v.size() * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); *dst = nullptr; return HELM_ERR_DEVICE; }
    if (hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return HELM_ERR_DEVICE; }
    return HELM_OK;
}

// the plan of windows (sz, wz, Wz) / (sx, wx, Wx) that carry an (nz_a, nx_a) grid to an (nz_b, nx_b) one
static helm_regrid *regrid_plan_from_windows(int device, int nz_a, int nx_a, int nz_b, int nx_b, int Wz, int Wx, const std::vector<int> &sz,
                                             const std::vector<int> &sx, const std::vector<double> &wz, const std::vector<double> &wx) {
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); helm_set_error(nullptr, "helm_regrid_create: hipSetDevice failed"); return nullptr; }
    helm_regrid *p = new helm_regrid();
    p->device = device; p->nz_a = nz_a; p->nx_a = nx_a; p->nz_b = nz_b; p->nx_b = nx_b; p->Wz = Wz; p->Wx = Wx;
    p->io.device = device;
    p->io.stream = helm_stream_acquire(device, 0);
    if (!p->io.stream) { helm_regrid_destroy(p); helm_set_error(nullptr, "helm_regrid_create: no stream"); return nullptr; }
    // FMAs of the two orders: the row axis first leaves an (nz_b, nx_a) intermediate, the contiguous axis first an (nz_a, nx_b) one
    const double zf = (double)nz_b * nx_a * Wz + (double)nz_b * nx_b * Wx, xf = (double)nz_a * nx_b * Wx + (double)nz_b * nx_b * Wz;
    p->z_first = zf <= xf;
    // column tiles of the contiguous pass: as wide as keeps each tile's input span within 64 KB of LDS
    std::vector<int> lo, len;
    for (int tw = 256; tw >= 64; tw /= 2) {
        lo.clear(); len.clear();
        int span = 0;
        for (int c0 = 0; c0 < nx_b; c0 += tw) {
            const int c1 = std::min(c0 + tw, nx_b);
            int a = sx[c0], b = sx[c0] + Wx;
            for (int c = c0; c < c1; ++c) { a = std::min(a, sx[c]); b = std::max(b, sx[c] + Wx); }
            lo.push_back(a); len.push_back(b - a); span = std::max(span, b - a);
        }
        p->tw = tw; p->xspan = span;
        if ((size_t)span * sizeof(cplx) <= ((size_t)64 << 10)) break;
    }
    p->xtiles = (int)lo.size();
    if ((size_t)p->xspan * sizeof(cplx) > ((size_t)64 << 10)) { helm_regrid_destroy(p); helm_set_error(nullptr, "helm_regrid_create: down-scaling factor too large for the LDS tile"); return nullptr; }
    if (upload_small(&p->d_sz, sz) || upload_small(&p->d_sx, sx) || upload_small(&p->d_wz, wz) || upload_small(&p->d_wx, wx) ||
        upload_small(&p->d_xlo, lo) || upload_small(&p->d_xlen, len)) {
        helm_regrid_destroy(p); helm_set_error(nullptr, "helm_regrid_create: upload of the taps failed"); return nullptr;
    }
    return p;
}

extern "C" helm_regrid *helm_regrid_create(int device, int nz_a, int nx_a, double dz_a, double dx_a, int nz_b, int nx_b, double dz_b, double dx_b,
                                           double zorig, double xorig) {
    (void)zorig; (void)xorig;         // (both grids start at the same origin: the transfer depends on the spacings alone)
    helm_tuning_refresh();
    std::vector<int> sz, sx;
    std::vector<double> wz, wx;
    const int Wz = axis_windows(nz_a, dz_a, nz_b, dz_b, sz, wz), Wx = axis_windows(nx_a, dx_a, nx_b, dx_b, sx, wx);
    if (Wz < 0 || Wx < 0) { helm_set_error(nullptr, "helm_regrid_create: grids need at least 4 nodes per axis and positive spacings"); return nullptr; }
    return regrid_plan_from_windows(device, nz_a, nx_a, nz_b, nx_b, Wz, Wx, sz, sx, wz, wx);
}

// The exact transpose of helm_regrid_create's plan for the same arguments: it carries grid B to grid A with the transposed windows of both axes.
// A transposed window of an axis reads forward outputs, so the plan is an ordinary one with the grids' roles exchanged: the pass order from
// the FMA counts with WTz / WTx, the column tiles and their LDS spans from the transposed starts, k_regrid_z / k_regrid_x unchanged.
extern "C" helm_regrid *helm_regrid_create_t(int device, int nz_a, int nx_a, double dz_a, double dx_a, int nz_b, int nx_b, double dz_b, double dx_b,
                                             double zorig, double xorig) {
    (void)zorig; (void)xorig;
    helm_tuning_refresh();
    std::vector<int> sz, sx;
    std::vector<double> wz, wx;
    const int Wz = axis_windows_t(nz_a, dz_a, nz_b, dz_b, sz, wz), Wx = axis_windows_t(nx_a, dx_a, nx_b, dx_b, sx, wx);
    if (Wz == HELM_ERR_UNSUPPORTED || Wx == HELM_ERR_UNSUPPORTED) {
        helm_set_error(nullptr, "helm_regrid_create_t: a node of grid A is touched by more than 64 nodes of grid B along an axis; this up-sampling transfer has no transposed plan");
        return nullptr;
    }
    if (Wz < 0 || Wx < 0) { helm_set_error(nullptr, "helm_regrid_create_t: grids need at least 4 nodes per axis and positive spacings"); return nullptr; }
    return regrid_plan_from_windows(device, nz_b, nx_b, nz_a, nx_a, Wz, Wx, sz, sx, wz, wx);
}

static int regrid_pass_z(const helm_regrid *p, hipStream_t st, const cplx *in, long long ifs, long long ies, cplx *out, long long ofs, long long oes,
                         int k, int ncol, bool fin, cplx gain, double beta, const cplx *mul) {
    dim3 grid((ncol + 63) / 64, (p->nz_b + 3) / 4, std::min(k, 65535));
    HELM_LAUNCH(k_regrid_z, grid, dim3(64, 4), 0, st, in, ifs, ies, out, ofs, oes, k, p->nz_b, ncol, p->d_sz, p->d_wz, p->Wz, fin ? 1 : 0, gain, beta, mul);
    return hipGetLastError() == hipSuccess ? HELM_OK : HELM_ERR_DEVICE;
}

static int regrid_pass_x(const helm_regrid *p, hipStream_t st, const cplx *in, long long ifs, long long ies, cplx *out, long long ofs, long long oes,
                         int k, int nrow, bool fin, cplx gain, double beta, const cplx *mul) {
    const long long rows = (long long)k * nrow;
    dim3 grid(p->xtiles, (unsigned)std::min<long long>(rows, 2048));
    const size_t lds = (size_t)p->xspan * sizeof(cplx);
    if (p->Wx <= 16)
        HELM_LAUNCH(k_regrid_x<16>, grid, dim3(p->tw), lds, st, in, ifs, ies, out, ofs, oes, k, nrow, p->nx_a, p->nx_b, p->d_sx, p->d_wx, p->Wx, p->d_xlo, p->d_xlen, fin ? 1 : 0, gain, beta, mul);
    else if (p->Wx <= 32)
        HELM_LAUNCH(k_regrid_x<32>, grid, dim3(p->tw), lds, st, in, ifs, ies, out, ofs, oes, k, nrow, p->nx_a, p->nx_b, p->d_sx, p->d_wx, p->Wx, p->d_xlo, p->d_xlen, fin ? 1 : 0, gain, beta, mul);
    else
        HELM_LAUNCH(k_regrid_x<64>, grid, dim3(p->tw), lds, st, in, ifs, ies, out, ofs, oes, k, nrow, p->nx_a, p->nx_b, p->d_sx, p->d_wx, p->Wx, p->d_xlo, p->d_xlen, fin ? 1 : 0, gain, beta, mul);
    return hipGetLastError() == hipSuccess ? HELM_OK : HELM_ERR_DEVICE;
}

extern "C" int helm_regrid_apply_device(helm_regrid *p, helm_op *op, int k, const void *dIn, long long in_fstride, long long in_estride, void *dOut,
                                        long long out_fstride, long long out_estride, double gain_re, double gain_im, double beta, const void *dMul) {
    helm_tuning_refresh();
    if (!p || k < 0 || (k > 0 && (!dIn || !dOut)) || in_estride < 1 || out_estride < 1) { helm_set_error(op, "helm_regrid_apply_device: bad arguments"); return HELM_ERR_ARG; }
    if (op && op->device != p->device) { helm_set_error(op, "helm_regrid_apply_device: the operator lives on another device than the plan"); return HELM_ERR_ARG; }
    if (k == 0) return HELM_OK;
    helm_op *eop = op ? op : &p->io;
    HIP_TRY(eop, hipSetDevice(p->device));
    hipStream_t st = eop->stream;
    const long long nmid = p->z_first ? (long long)p->nz_b * p->nx_a : (long long)p->nz_a * p->nx_b;
    const size_t per = (size_t)nmid * sizeof(cplx);
    const int kb = (int)std::max<long long>(1, std::min<long long>(k, (long long)(((size_t)4 << 30) / per)));
    cplx *ws = (cplx *)helm_pool_alloc(p->device, per * kb);
    if (!ws) { helm_set_error(eop, "helm_regrid_apply_device: no memory for the intermediate"); return HELM_ERR_DEVICE; }
    const cplx gain = cmake(gain_re, gain_im), one = cmake(1.0, 0.0);
    const cplx *in = (const cplx *)dIn, *mul = (const cplx *)dMul;
    cplx *out = (cplx *)dOut;
    int rc = HELM_OK;
    for (int f0 = 0; f0 < k && rc == HELM_OK; f0 += kb) {
        const int kk = std::min(kb, k - f0);
        const cplx *src = in + (long long)f0 * in_fstride;
        cplx *dst = out + (long long)f0 * out_fstride;
        if (p->z_first) {
            rc = regrid_pass_z(p, st, src, in_fstride, in_estride, ws, nmid, 1, kk, p->nx_a, false, one, 0.0, nullptr);
            if (!rc) rc = regrid_pass_x(p, st, ws, nmid, 1, dst, out_fstride, out_estride, kk, p->nz_b, true, gain, beta, mul);
        } else {
            rc = regrid_pass_x(p, st, src, in_fstride, in_estride, ws, nmid, 1, kk, p->nz_a, false, one, 0.0, nullptr);
            if (!rc) rc = regrid_pass_z(p, st, ws, nmid, 1, dst, out_fstride, out_estride, kk, p->nx_b, true, gain, beta, mul);
        }
    }
    // (the call returns when the transfer is done: the intermediate goes back to the pool, and the caller may read `out` or reuse `in`)
    const hipError_t e = hipStreamSynchronize(st);
    helm_pool_free(p->device, ws, per * kb);
    if (rc) { (void)hipGetLastError(); helm_set_error(eop, "helm_regrid_apply_device: launch failed"); return rc; }
    if (e != hipSuccess) { (void)hipGetLastError(); helm_set_error(eop, "helm_regrid_apply_device: transfer failed"); return HELM_ERR_DEVICE; }
    return HELM_OK;
}

extern "C" int helm_regrid_apply(helm_regrid *p, int k, const double *in, long long in_fstride, long long in_estride, double *out, long long out_fstride,
                                 long long out_estride, double gain_re, double gain_im, double beta, const double *mul) {
    helm_tuning_refresh();
    if (!p || k < 0 || (k > 0 && (!in || !out))) { helm_set_error(nullptr, "helm_regrid_apply: bad arguments"); return HELM_ERR_ARG; }
    if (k == 0) return HELM_OK;
    const long long na = (long long)p->nz_a * p->nx_a, nb = (long long)p->nz_b * p->nx_b;
    // the host arrays are moved whole: each must be a dense (k, N) or (N, k) block
    auto dense = [](long long n, int kk, long long fs, long long es) { return (es == 1 && (fs == n || kk == 1)) || (fs == 1 && es == kk); };
    if (!dense(na, k, in_fstride, in_estride) || !dense(nb, k, out_fstride, out_estride)) { helm_set_error(nullptr, "helm_regrid_apply: host arrays must be dense (k, N) or (N, k) blocks"); return HELM_ERR_ARG; }
    helm_op *io = &p->io;
    HIP_TRY(io, hipSetDevice(p->device));
    const size_t bi = (size_t)na * k * sizeof(cplx), bo = (size_t)nb * k * sizeof(cplx), bm = (size_t)nb * sizeof(cplx);
    void *din = helm_pool_alloc(p->device, bi), *dout = helm_pool_alloc(p->device, bo), *dmul = mul ? helm_pool_alloc(p->device, bm) : nullptr;
    int rc = (!din || !dout || (mul && !dmul)) ? HELM_ERR_DEVICE : HELM_OK;
    if (rc) helm_set_error(nullptr, "helm_regrid_apply: no device memory");
    if (!rc) rc = helm_upload_staged(io, din, in, bi);
    if (!rc && beta != 0.0) rc = helm_upload_staged(io, dout, out, bo);
    if (!rc && mul) rc = helm_upload_staged(io, dmul, mul, bm);
    if (!rc) rc = helm_regrid_apply_device(p, nullptr, k, din, in_fstride, in_estride, dout, out_fstride, out_estride, gain_re, gain_im, beta, dmul);
    if (!rc) rc = helm_download_staged(io, out, dout, bo);
    if (rc) helm_set_error(nullptr, io->err.empty() ? "helm_regrid_apply failed" : io->err.c_str());
    helm_pool_free(p->device, din, bi); helm_pool_free(p->device, dout, bo);
    if (dmul) helm_pool_free(p->device, dmul, bm);
    return rc;
}
