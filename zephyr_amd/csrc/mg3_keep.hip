// Set-up of the layer-preserving 3-D hierarchy (oversampled grids: >= 20 points per wavelength; cycle_keep of mg3d.hip runs it).
// The standard cycle (mg3d.hip) needs a large shift and a weak layer because (a) point Jacobi DIVERGES where two stretched directions
// overlap (the directional parts of the diagonal have different complex phases and partly cancel: |lambda / d| reaches 4),
// and (b) inside a strongly stretched layer the coupling normal to the boundary is weak, so error that oscillates along the
// normal is neither smoothed nor representable on a grid coarsened in that direction.  Here instead:
//   * coarse grids keep EVERY node of the absorbing layers and halve only the interior: tensor-product grids with
//     non-uniform spacing, rediscretised with the same 27-point formula (the spacing enters the 1-D factors like a stretch),
//     per-axis interpolation / weighting tables;
//   * the smoother is l1-Jacobi (d_i = -sum_j |a_ij|, weight 1.6 = plain 0.8 in the interior);
//   * the preconditioner is the operator itself with its TRUE layer and a small shift (beta = 0.1);
//   * coarsening stops while the interior still has >= 10 points per wavelength and that level is solved directly:
//     block-tridiagonal elimination over the planes normal to the longest axis, dense plane inverses in HBM
//     (8.7 GB in single precision for the 79 x 79 x 47 level of config 5), applied as split-K batched GEMMs.
// numpy prototype (96 x 96 x 64, 40 / 100 points per wavelength): 9 / 7 BiCGSTAB iterations against 219 / 811 for the recipe above.
#include "mg3_internal.hpp"
#include <chrono>

namespace {
// a uniform axis: n nodes at spacing h, npml layer nodes at each end with damping amplitude cpml (the profile of helm3d.hip profile3())
Ax3 uniform_axis(int n, int npml, double h, double cpml) {
    Ax3 a; a.x.resize(n); a.gam.assign(n, 0.0); a.lay.assign(n, 0);
    for (int i = 0; i < n; ++i) a.x[i] = i * h;
    const double Lh = h * (npml - 1);
    for (int k = 0; k < npml && k < n; ++k) {
        a.gam[k] = cpml * cos((M_PI / 2) * (k * h / Lh)); a.lay[k] = 1;
        a.gam[n - npml + k] = cpml * cos((M_PI / 2) * ((npml - 1 - k) * h / Lh)); a.lay[n - npml + k] = 1;
    }
    return a;
}

void coarsen_axis(const Ax3 &a, bool keep_layer, Ax3 &c, std::vector<int> &kept, std::vector<PTab> &pt, std::vector<RTab> &rt) {
    const int n = a.n();
    std::vector<char> keep(n, 0);
    if (keep_layer) {
        for (int i = 0; i < n;) {
            if (a.lay[i]) { keep[i] = 1; ++i; continue; }
            int j = i;
            while (j < n && !a.lay[j]) ++j;
            for (int t = i; t < j; ++t) keep[t] = (char)((t - i) & 1);      // the first node of an interior run is dropped
            i = j;
        }
    } else {
        for (int i = 0; i < n; ++i) keep[i] = (char)!(i & 1);
    }
    keep[0] = keep[n - 1] = 1;
    for (int i = 1; i + 1 < n; ++i) if (!keep[i] && !(keep[i - 1] && keep[i + 1])) keep[i] = 1;   // a dropped node interpolates from kept neighbours
    std::vector<int> cmap(n, -1);
    c = Ax3(); kept.clear();
    for (int i = 0; i < n; ++i) if (keep[i]) {
        cmap[i] = (int)kept.size(); kept.push_back(i);
        c.x.push_back(a.x[i]); c.gam.push_back(a.gam[i]); c.lay.push_back(a.lay[i]);
    }
    pt.resize(n);
    for (int i = 0; i < n; ++i) {
        if (keep[i]) { pt[i].c0 = pt[i].c1 = cmap[i]; pt[i].w0 = 1.0; pt[i].w1 = 0.0; continue; }
        const double da = a.x[i] - a.x[i - 1], db = a.x[i + 1] - a.x[i];
        pt[i].c0 = cmap[i - 1]; pt[i].c1 = cmap[i + 1]; pt[i].w0 = db / (da + db); pt[i].w1 = da / (da + db);
    }
    rt.resize(kept.size());
    for (size_t I = 0; I < kept.size(); ++I) {
        const int f = kept[I];
        double wl = (f > 0 && !keep[f - 1]) ? pt[f - 1].w1 : 0.0, wr = (f + 1 < n && !keep[f + 1]) ? pt[f + 1].w0 : 0.0;
        const double s = 1.0 + wl + wr;
        rt[I].f = f; rt[I].wl = wl / s; rt[I].wc = 1.0 / s; rt[I].wr = wr / s;
    }
}

// 1-D factors L(-1), L(0), L(+1) of d/dx (1/xi) d/dx / xi on a non-uniform axis, 1/h^2 included (for uniform spacing h this is
// profile3() of helm3d.hip divided by h^2)
void lap_from_axis(const Ax3 &a, std::complex<double> om, std::vector<cplx> &Lt) {
    const int n = a.n();
    auto xi = [&](int i) { i = std::min(std::max(i, 0), n - 1); return 1.0 - std::complex<double>(0.0, a.gam[i]) / om; };
    Lt.resize((size_t)3 * n);
    for (int i = 0; i < n; ++i) {
        const double hm = i > 0 ? a.x[i] - a.x[i - 1] : a.x[1] - a.x[0], hp = i + 1 < n ? a.x[i + 1] - a.x[i] : a.x[n - 1] - a.x[n - 2];
        const double hbar = 0.5 * (hm + hp);
        const std::complex<double> c = xi(i);
        const std::complex<double> lm = 1.0 / (c * hbar * (c + xi(i - 1)) * 0.5 * hm), lp = 1.0 / (c * hbar * (c + xi(i + 1)) * 0.5 * hp);
        const std::complex<double> l0 = -(lm + lp);
        Lt[i] = cmake(lm.real(), lm.imag());
        Lt[(size_t)n + i] = cmake(l0.real(), l0.imag());
        Lt[(size_t)2 * n + i] = cmake(lp.real(), lp.imag());
    }
}

// l1-Jacobi: 1 / d with d = -sum_k |a_k| (the centre coefficient of this operator is negative real in the interior); identity rows
// (the box boundary) get 1 / w so that the weighted step is exact
__global__ void k3_l1_dinv(const cplx *__restrict__ planes, cplx *__restrict__ dl1, long long N, double w) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int k = 0; k < 27; ++k) { const cplx v = planes[(long long)k * N + i]; s += sqrt(v.x * v.x + v.y * v.y); }
        const cplx c = planes[13LL * N + i];
        const double ac = sqrt(c.x * c.x + c.y * c.y);
        if (s <= ac * (1.0 + 1e-14)) { const double r = 1.0 / (w * ac * ac); dl1[i] = cmake(c.x * r, -c.y * r); }
        else dl1[i] = cmake(-1.0 / s, 0.0);
    }
}

// Galerkin coarse operator A_c = R A_f P of a 27-point fine operator with the tensor-product transfers of the tables: again 27-point.
// One thread per coarse node (a set-up kernel: the 27 accumulators are indexed dynamically and live in scratch).  Used for the directly
// solved level only: at 5-8 points per wavelength the rediscretised operator carries waves of a different length than the level above
// (numpy prototype, 5 points: 38 instead of 87 iterations).
__global__ __launch_bounds__(256) void k3_galerkin(const cplx *__restrict__ pf, int nzf, int nyf, int nxf, cplx *__restrict__ pc, int nzc, int nyc, int nxc,
                                                   const RTab *__restrict__ rz_, const RTab *__restrict__ ry_, const RTab *__restrict__ rx_,
                                                   const PTab *__restrict__ pz_, const PTab *__restrict__ py_, const PTab *__restrict__ px_) {
    const long long Nc = (long long)nzc * nyc * nxc, Nf = (long long)nzf * nyf * nxf;
    const long long I = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= Nc) return;
    const int X = (int)(I % nxc), Y = (int)((I / nxc) % nyc), Z = (int)(I / ((long long)nxc * nyc));
    cplx acc[27];
    for (int k = 0; k < 27; ++k) acc[k] = cmake(0.0, 0.0);
    const RTab rz = rz_[Z], ry = ry_[Y], rx = rx_[X];
    const double wz[3] = {rz.wl, rz.wc, rz.wr}, wy[3] = {ry.wl, ry.wc, ry.wr}, wx[3] = {rx.wl, rx.wc, rx.wr};
    for (int a = 0; a < 3; ++a) { if (wz[a] == 0.0) continue; const int iz = rz.f + a - 1;
        for (int b = 0; b < 3; ++b) { if (wy[b] == 0.0) continue; const int iy = ry.f + b - 1;
            for (int c = 0; c < 3; ++c) { if (wx[c] == 0.0) continue; const int ix = rx.f + c - 1;
                const double wr = wz[a] * wy[b] * wx[c];
                const long long i = ((long long)iz * nyf + iy) * nxf + ix;
                for (int k = 0; k < 27; ++k) {
                    const cplx cf = pf[(long long)k * Nf + i];
                    if (cf.x == 0.0 && cf.y == 0.0) continue;
                    const int jz = iz + k / 9 - 1, jy = iy + (k / 3) % 3 - 1, jx = ix + k % 3 - 1;
                    if (jz < 0 || jz >= nzf || jy < 0 || jy >= nyf || jx < 0 || jx >= nxf) continue;
                    const PTab qz = pz_[jz], qy = py_[jy], qx = px_[jx];
                    const int cz[2] = {qz.c0, qz.c1}, cy[2] = {qy.c0, qy.c1}, cx[2] = {qx.c0, qx.c1};
                    const double vz[2] = {qz.w0, qz.w1}, vy[2] = {qy.w0, qy.w1}, vx[2] = {qx.w0, qx.w1};
                    for (int ua = 0; ua < 2; ++ua) { if (vz[ua] == 0.0) continue; const int dz = cz[ua] - Z; if (dz < -1 || dz > 1) continue;
                        for (int ub = 0; ub < 2; ++ub) { if (vy[ub] == 0.0) continue; const int dy = cy[ub] - Y; if (dy < -1 || dy > 1) continue;
                            for (int uc = 0; uc < 2; ++uc) { if (vx[uc] == 0.0) continue; const int dx = cx[uc] - X; if (dx < -1 || dx > 1) continue;
                                const double w = wr * vz[ua] * vy[ub] * vx[uc];
                                cplx &t = acc[9 * (dz + 1) + 3 * (dy + 1) + (dx + 1)];
                                t.x += w * cf.x; t.y += w * cf.y;
                            } } }
                }
            } } }
    for (int k = 0; k < 27; ++k) pc[(long long)k * Nc + I] = acc[k];
}

// model of a coarser level: the values at the nodes it keeps (kz / ky / kx: kept node indices per axis)
__global__ void k3_inject_model(const cplx *__restrict__ c, const double *__restrict__ rho, int fny, int fnx, const int *__restrict__ kz, const int *__restrict__ ky,
                                const int *__restrict__ kx, int nzc, int nyc, int nxc, cplx *__restrict__ cc, double *__restrict__ rc) {
    const long long n = (long long)nzc * nyc * nxc;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int X = (int)(e % nxc), Y = (int)((e / nxc) % nyc), Z = (int)(e / ((long long)nxc * nyc));
        const long long src = ((long long)kz[Z] * fny + ky[Y]) * fnx + kx[X];
        cc[e] = c[src]; rc[e] = rho[src];
    }
}

template <typename T> T *upload(Mg3Keep *K, const std::vector<T> &v) {
    const size_t b = v.size() * sizeof(T);
    T *d = (T *)helm_pool_alloc(K->device, b);
    if (!d) return nullptr;
    K->tabs.push_back(std::make_pair((void *)d, b));
    if (hipMemcpy(d, v.data(), b, hipMemcpyHostToDevice) != hipSuccess) return nullptr;      // (the buffer goes back with the others in keep_free)
    return d;
}

}  // namespace

void mg3_keep_free(Mg3Precond *P) {
    Mg3Keep *K = P->keep;
    if (!K) return;
    for (size_t i = 0; i < K->dl1.size(); ++i) helm_pool_free(K->device, K->dl1[i], K->dl1_bytes[i]);
    for (auto &t : K->tabs) helm_pool_free(K->device, t.first, t.second);
    mg3_coarse_free(K);
    delete K;
    P->keep = nullptr;
}

void mg3_keep_level_dims(const helm_op *op, int l, int out[3]) {
    const int dims[3] = {op->nz, op->ny, op->nx};
    for (int a = 0; a < 3; ++a) {
        Ax3 ax = uniform_axis(dims[a], op->nPML, 1.0, 0.0), c;      // (the node counts depend on neither the spacing nor the damping)
        std::vector<int> kept; std::vector<PTab> pt; std::vector<RTab> rt;
        for (int i = 0; i < l; ++i) { coarsen_axis(ax, true, c, kept, pt, rt); ax = c; }
        out[a] = ax.n();
    }
}

// levels 0 .. ncoarsen of the layer-preserving hierarchy + the direct solver of the last one; on failure the caller falls back
int mg3_keep_setup(helm_op *op, Mg3Precond *P, int batch, int ncoarsen, double tauM, const helm_tuning &tune) {
    const bool trace = mg3_trace();
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto tprev = now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        hipStreamSynchronize(op->stream);
        const auto t = now();
        fprintf(stderr, "[helm mg3 set-up] %-34s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(t - tprev).count());
        tprev = t;
    };
    Mg3Keep *K = new Mg3Keep();
    P->keep = K;
    P->fine32 = tune.mg3_f32 != 0;
    K->omega_l1 = 1.6;
    K->device = op->device;
    std::complex<double> om(2.0 * M_PI * op->a_freq_re, 2.0 * M_PI * op->a_freq_im);
    om -= std::complex<double>(0.0, 1.0 / tauM);
    const double cpml = op->a_cpml;
    Ax3 ax[3];
    const int dims[3] = {op->nz, op->ny, op->nx};
    const double hs[3] = {op->dz, op->dy, op->dx};
    for (int a = 0; a < 3; ++a) ax[a] = uniform_axis(dims[a], op->nPML, hs[a], cpml);
    // the levels' models never visit the host: level 0 copies the caller's device arrays, a coarser level takes the values at the nodes it keeps
    std::vector<int> kept[3];
    lap("axes");
    for (int l = 0; l <= ncoarsen; ++l) {
        if (l) lap("level (operator, vectors, tables)");
        Mg3Level L;
        L.nz = ax[0].n(); L.ny = ax[1].n(); L.nx = ax[2].n(); L.N = (long long)L.nz * L.ny * L.nx;
        L.op = helm_create3d(op->device, L.nz, L.ny, L.nx, 1.0, 1.0, 1.0, 2);
        if (!L.op) HELM_FAIL(op, HELM_ERR_DEVICE, "%s", helm_last_error(nullptr));
        P->lv.push_back(L);
        Mg3Level &Lr = P->lv.back();
        if (helm_set_stream(Lr.op, op->stream)) HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: cannot share the stream");
        std::vector<cplx> Lz, Ly, Lx;
        lap_from_axis(ax[0], om, Lz); lap_from_axis(ax[1], om, Ly); lap_from_axis(ax[2], om, Lx);
        Lr.op->lap_override = Lx;
        Lr.op->lap_override.insert(Lr.op->lap_override.end(), Ly.begin(), Ly.end());
        Lr.op->lap_override.insert(Lr.op->lap_override.end(), Lz.begin(), Lz.end());
        int rc = HELM_OK;
        if (l == 0) rc = helm_adopt_model_device(Lr.op, op->d_c, op->d_rho);
        else {
            const Mg3Level &Lf = P->lv[l - 1];
            const size_t kb = (kept[0].size() + kept[1].size() + kept[2].size()) * sizeof(int);
            int *dk = (int *)helm_pool_alloc(op->device, kb);
            if (!dk) HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: transfer tables do not fit");
            size_t off = 0;
            const int *dka[3];
            for (int a = 0; a < 3; ++a) {
                hipMemcpyAsync(dk + off, kept[a].data(), kept[a].size() * sizeof(int), hipMemcpyHostToDevice, op->stream);
                dka[a] = dk + off; off += kept[a].size();
            }
            HELM_LAUNCH(k3_inject_model, dim3((unsigned)std::min<long long>((Lr.N + 255) / 256, 65535)), dim3(256), 0, op->stream, (const cplx *)Lf.op->d_c,
                               (const double *)Lf.op->d_rho, Lf.ny, Lf.nx, dka[0], dka[1], dka[2], Lr.nz, Lr.ny, Lr.nx, Lr.op->d_c, Lr.op->d_rho);
            hipStreamSynchronize(op->stream);                    // (kept[] is overwritten below; the table buffer goes back to the pool)
            helm_pool_free(op->device, dk, kb);
            rc = helm_adopt_model_device(Lr.op, nullptr, nullptr);
        }
        if (!rc) rc = helm_assemble(Lr.op, op->a_freq_re, op->a_freq_im, tauM, 0.0, cpml);
        if (rc) HELM_FAIL(op, rc, "%s", helm_last_error(Lr.op));
        if (!mg3_level_vectors(op, Lr, batch)) HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: level vectors do not fit");
        if (l == ncoarsen) break;
        cplx *dl1 = (cplx *)helm_pool_alloc(op->device, (size_t)Lr.N * sizeof(cplx));
        if (!dl1) HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: level vectors do not fit");
        K->dl1.push_back(dl1); K->dl1_bytes.push_back((size_t)Lr.N * sizeof(cplx));
        HELM_LAUNCH(k3_l1_dinv, dim3((unsigned)std::min<long long>((Lr.N + 255) / 256, 65535)), dim3(256), 0, op->stream, (const cplx *)Lr.op->d_C, dl1, Lr.N, K->omega_l1);
        // next level
        Ax3 cx[3];
        for (int a = 0; a < 3; ++a) {
            std::vector<PTab> pt; std::vector<RTab> rt;
            coarsen_axis(ax[a], true, cx[a], kept[a], pt, rt);
            PTab *dp = upload(K, pt); RTab *dr = upload(K, rt);
            K->pt[a].push_back(dp); K->rt[a].push_back(dr);
            if (!dp || !dr) HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: transfer tables do not fit");
        }
        for (int a = 0; a < 3; ++a) ax[a] = cx[a];
    }
    lap("last level");
    if (ncoarsen > 0 && tune.mg3_galerkin) {        // the directly solved level carries the Galerkin product of the level above it
        const Mg3Level &Lf = P->lv[ncoarsen - 1]; Mg3Level &Lc = P->lv[ncoarsen];
        const int t = ncoarsen - 1;
        Lc.op->otf3 = false;            // (the coarse level's planes are the Galerkin product from here on, not what its c, rho and factor tables would rebuild)
        HELM_LAUNCH(k3_galerkin, dim3((unsigned)((Lc.N + 255) / 256)), dim3(256), 0, op->stream, (const cplx *)Lf.op->d_C, Lf.nz, Lf.ny, Lf.nx,
                           Lc.op->d_C, Lc.nz, Lc.ny, Lc.nx, (const RTab *)K->rt[0][t], (const RTab *)K->rt[1][t], (const RTab *)K->rt[2][t],
                           (const PTab *)K->pt[0][t], (const PTab *)K->pt[1][t], (const PTab *)K->pt[2][t]);
        HIP_TRY(op, hipGetLastError());
    }
    lap("Galerkin product");
    // A transposed handle (helm_set_transposed3d): its preconditioner is the TRANSPOSE of the cycle of A, level by level.  Everything above was built for A --
    // the levels, their l1-Jacobi diagonals (a sweep with the same diagonal on A_l^T is the transpose of the sweep on A_l) and the Galerkin product R A P -- and
    // the planes of every level are now permuted into those of its transpose; the direct solver of the last level factors what it finds there.  The transfers
    // keep their tables: R = D P^T with D the product of the three axes' wc, so the transposed cycle restricts with P^T = D^-1 R and prolongs with R^T = P D
    // (cycle_keep scales the coarse vector, k3_scale_rt).  Re-discretising A^T on the coarse grids and keeping R, P as they are is NOT that cycle: D is 1 in the
    // layers and 1/8 in the interior, and BiCGSTAB needed 34 / 741 / 811 iterations where the cycle of A needs 11 / 16 / 12.
    if (op->transposed)
        for (Mg3Level &Lt : P->lv) {
            const int rct = helm3d_launch_transpose_planes(Lt.op);
            if (rct) HELM_FAIL(op, rct, "%s", helm_last_error(Lt.op));
            Lt.op->transposed = true;
        }
    lap("transposed levels");
    const int rcd = mg3_coarse_setup(op, K, P->lv.back(), batch, tune);
    lap("direct solver of the last level");
    return rcd;
}

// ---- diagnostics exported through the C ABI (host side of the layer-preserving hierarchy, no GPU needed) ----------------
// One axis of n nodes (spacing h, npml layer nodes at each end, damping amplitude cpml), coarsened `level` times.  Returns the number of
// nodes nc of that level and writes, if the pointers are not null: x[nc] node coordinates, lay[nc] layer flags, lap[3 * nc] the factors
// L(-1), L(0), L(+1) (complex, interleaved re / im) for omega = (om_re, om_im); and for the transfer from this level to the next one:
// pc[2 * nc] / pw[2 * nc] the two coarse nodes and weights each node interpolates from, rf[ncn] / rw[3 * ncn] the centre node and the
// three weights of every node of the next level (ncn through *n_next).
extern "C" int helm_mg3_axis(int n, int npml, double h, double cpml, double om_re, double om_im, int level, double *x, int *lay, double *lap,
                             int *pc, double *pw, int *n_next, int *rf, double *rw) {
    if (n < 3 || npml < 2 || 2 * npml > n || level < 0) return -1;
    Ax3 a = uniform_axis(n, npml, h, cpml);
    Ax3 c; std::vector<int> kept; std::vector<PTab> pt; std::vector<RTab> rt;
    for (int l = 0; l < level; ++l) { coarsen_axis(a, true, c, kept, pt, rt); a = c; }
    const int nc = a.n();
    if (x) for (int i = 0; i < nc; ++i) x[i] = a.x[i];
    if (lay) for (int i = 0; i < nc; ++i) lay[i] = a.lay[i];
    if (lap) {
        std::vector<cplx> Lt;
        lap_from_axis(a, std::complex<double>(om_re, om_im), Lt);
        for (size_t i = 0; i < Lt.size(); ++i) { lap[2 * i] = Lt[i].x; lap[2 * i + 1] = Lt[i].y; }
    }
    if (pc || pw || n_next || rf || rw) {
        coarsen_axis(a, true, c, kept, pt, rt);
        if (n_next) *n_next = c.n();
        for (int i = 0; i < nc; ++i) {
            if (pc) { pc[2 * i] = pt[i].c0; pc[2 * i + 1] = pt[i].c1; }
            if (pw) { pw[2 * i] = pt[i].w0; pw[2 * i + 1] = pt[i].w1; }
        }
        for (int i = 0; i < c.n(); ++i) {
            if (rf) rf[i] = rt[i].f;
            if (rw) { rw[3 * i] = rt[i].wl; rw[3 * i + 1] = rt[i].wc; rw[3 * i + 2] = rt[i].wr; }
        }
    }
    return nc;
}
