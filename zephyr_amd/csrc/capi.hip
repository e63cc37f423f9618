// C ABI of libhelm (see include/helm.h): handle lifecycle, model and assembly, apply, and the dispatch of a solve to the direct path
// (solve_direct.hip) or the Krylov drivers (krylov.hip) with the fallback of HELM_AUTO between them.
#include "solve_internal.hpp"
#include <mutex>
#include <map>
#include <algorithm>

// one record per host thread: handles are driven from several threads (bench --streams), and the handle-less error
// is read back by the thread that got the failing return code
static thread_local std::string g_last_error;

void helm_set_error(helm_op *op, const char *msg) {
    if (op) op->err = msg;
    g_last_error = msg;
}

extern "C" const char *helm_last_error(const helm_op *op) { return op ? op->err.c_str() : g_last_error.c_str(); }
extern "C" const char *helm_version(void) { return "libhelm 0.1 (gfx950)"; }

extern "C" int helm_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { helm_set_error(nullptr, hipGetErrorString(e)); return HELM_ERR_DEVICE; }
    return n;
}

// creation failures release everything through helm_destroy (stream, model arrays, planes, the live-handle count)
#define HIP_TRY_NULL(call) do { hipError_t _e = (call); if (_e != hipSuccess) { char _b[256]; \
    snprintf(_b, sizeof(_b), "%s failed: %s", #call, hipGetErrorString(_e)); helm_destroy(op); helm_set_error(nullptr, _b); return nullptr; } } while (0)

static helm_op *create_common(helm_op *op);
namespace { std::mutex g_live_mu; std::map<int, int> g_live_per_device; }      // operators alive per device

extern "C" helm_op *helm_create3d(int device, int nz, int ny, int nx, double dx, double dy, double dz, int nPML) {
    helm_tuning_refresh();
    if (nz < 3 || ny < 3 || nx < 3) { helm_set_error(nullptr, "nz, ny and nx must be >= 3"); return nullptr; }
    if (!(dx > 0) || !(dy > 0) || !(dz > 0)) { helm_set_error(nullptr, "grid spacings must be positive"); return nullptr; }
    helm_op *op = new helm_op();
    op->device = device; op->variant = HELM_3D; op->nz = nz; op->ny = ny; op->nx = nx; op->N = (long long)nz * ny * nx;
    op->dx = dx; op->dy = dy; op->dz = dz; op->nPML = nPML;
    op->nblocks = 1; op->nplanes = 27; op->centre = 13;
    return create_common(op);
}

extern "C" helm_op *helm_create(int device, int variant, int nz, int nx, double dx, double dz, int nPML, const int *freeSurf) {
    helm_tuning_refresh();
    if (nz < 3 || nx < 3) { helm_set_error(nullptr, "nz and nx must be >= 3"); return nullptr; }
    if (variant != HELM_MINIZEPHYR && variant != HELM_EURUS) { helm_set_error(nullptr, "unknown variant"); return nullptr; }
    if (!(dx > 0) || !(dz > 0)) { helm_set_error(nullptr, "dx and dz must be positive"); return nullptr; }
    helm_op *op = new helm_op();
    op->device = device; op->variant = variant; op->nz = nz; op->nx = nx; op->N = (long long)nz * nx;
    op->dx = dx; op->dz = dz; op->nPML = nPML;
    if (freeSurf) for (int i = 0; i < 4; ++i) op->fs[i] = freeSurf[i] ? 1 : 0;
    op->nblocks = variant == HELM_EURUS ? 4 : 1;
    if (nPML < 0) { op->block0_only = true; op->nPML = -nPML; op->nblocks = 1; }   // internal: preconditioner level
    return create_common(op);
}

static helm_op *create_common(helm_op *op) {
    const int device = op->device;
    { std::lock_guard<std::mutex> lk(g_live_mu); g_live_per_device[device] += 1; }      // helm_destroy takes it back on every exit
    HIP_TRY_NULL(hipSetDevice(device));
    {   // first operator of this device in the process: resolve the library's kernels now, not one by one inside the first solves of each kind
        static std::mutex wmu; static std::map<int, bool> warmed;
        bool need = false;
        { std::lock_guard<std::mutex> lk(wmu); if (!warmed[device]) { warmed[device] = true; need = true; } }
        if (need && helm_env_int("HELM_WARM", 1)) (void)helm_warm(device);
    }
    op->stream = helm_stream_acquire(device, 0);
    if (!op->stream) { helm_destroy(op); helm_set_error(nullptr, "hipStreamCreate failed"); return nullptr; }
    op->own_stream = true;
    const size_t N = (size_t)op->N;
    op->Nv = op->N;
    // model arrays come from the size-keyed pool as well: hipMalloc / hipFree of a few MB per operator is a device synchronisation each
    op->d_c = (cplx *)helm_pool_alloc(device, N * sizeof(cplx));
    op->d_rho = (double *)helm_pool_alloc(device, N * sizeof(double));
    if (!op->d_c || !op->d_rho) { helm_destroy(op); helm_set_error(nullptr, "hipMalloc of the model arrays failed"); return nullptr; }
    op->d_C = (cplx *)helm_pool_alloc(device, (size_t)op->nblocks * op->nplanes * N * sizeof(cplx));
    if (!op->d_C) { helm_destroy(op); helm_set_error(nullptr, "hipMalloc of the coefficient planes failed"); return nullptr; }
    return op;
}

extern "C" void helm_destroy(helm_op *op) {
    if (!op) return;
    hipSetDevice(op->device);
    helm_pf_retire(op);
    if (op->stream) hipStreamSynchronize(op->stream);
    helm_pool_free(op->device, op->d_c, (size_t)op->N * sizeof(cplx)); helm_pool_free(op->device, op->d_rho, (size_t)op->N * sizeof(double));
    helm_pool_free(op->device, op->d_theta, (size_t)op->N * sizeof(double)); helm_pool_free(op->device, op->d_eps, (size_t)op->N * sizeof(double)); helm_pool_free(op->device, op->d_delta, (size_t)op->N * sizeof(double));
    helm_eu_params_drop(op);
    helm_pool_free(op->device, op->d_K3, (size_t)op->N * sizeof(cplx)); helm_pool_free(op->device, op->d_b3, (size_t)op->N * sizeof(double));
    helm_pool_free(op->device, op->d_L3, op->l3_elems * sizeof(cplx));
    {
        const size_t pb = (size_t)op->nblocks * op->nplanes * (size_t)op->N * sizeof(cplx);
        helm_pool_free(op->device, op->d_C, pb); helm_pool_free(op->device, op->d_Cs, pb);
        helm_pool_free(op->device, op->d_dinv, (size_t)op->nblocks * (size_t)op->N * sizeof(cplx));
    }
    hipFree(op->d_S); hipFree(op->d_rs);
    if (op->mg || op->mg3) mg_destroy(op);
    for (int b = 0; b < 4; ++b) { nd_free(op->direct[b]); op->direct[b] = nullptr; }
    helm_pool_free(op->device, op->d_ws, op->ws_bytes); helm_pool_free(op->device, op->d_part, op->part_bytes);
    helm_pool_free(op->device, op->sk_buf, op->sk_bytes);
    helm_pool_free(op->device, op->gjp_buf, op->gjp_bytes);
    helm_pool_free(op->device, op->d_scal, (size_t)op->scal_cap * sizeof(RhsScal));
    helm_hostpool_free(op->h_scal, op->h_scal_bytes);
    if (op->pf_done) hipEventDestroy(op->pf_done);
    if (op->pf_t0) hipEventDestroy(op->pf_t0);
    if (op->pf_t1) hipEventDestroy(op->pf_t1);
    if (op->fstream) helm_stream_release(op->device, op->fstream_prio, op->fstream);
    helm_events_release(op);
    if (op->side_stream) helm_stream_release(op->device, -1, op->side_stream);
    if (op->own_stream && op->stream) helm_stream_release(op->device, 0, op->stream);
    const int device = op->device;
    delete op;
    bool last = false;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        int &n = g_live_per_device[device];
        if (n > 0) n -= 1;
        last = n == 0;
    }
    // (auto: the spares of the big size classes are topped up here, when nobody is waiting for this thread -- HELM_POOL_SPARE_AUTO=0 leaves it to helm_pool_spares,
    // for callers that time the region this destroy ends)
    { const int spare = helm_env_int("HELM_POOL_SPARE", 2); if (last && spare > 0 && helm_env_int("HELM_POOL_SPARE_AUTO", 1)) helm_pool_top_up(device, spare); }
}

extern "C" int helm_set_stream(helm_op *op, void *hip_stream) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    helm_pf_retire(op);
    if (op->stream) HIP_TRY(op, hipStreamSynchronize(op->stream));
    // the multigrid level operators launch on the stream they were given at setup (mg.hip assemble_child): they are rebuilt on
    // the new stream by the next solve that needs them
    if (op->mg || op->mg3) mg_destroy(op);
    if (op->own_stream && op->stream) { helm_stream_release(op->device, 0, op->stream); op->own_stream = false; }
    if (hip_stream) { op->stream = (hipStream_t)hip_stream; op->own_stream = false; }
    else { op->stream = helm_stream_acquire(op->device, 0); if (!op->stream) HELM_FAIL(op, HELM_ERR_DEVICE, "hipStreamCreate failed"); op->own_stream = true; }
    return HELM_OK;
}

extern "C" int helm_set_profiling(helm_op *op, int on) {
    helm_tuning_refresh(); if (!op) return HELM_ERR_ARG; op->profiling = on != 0; return HELM_OK; }
extern "C" int helm_last_timing(const helm_op *op, helm_timing *out) { if (!op || !out) return HELM_ERR_ARG; *out = op->timing; return HELM_OK; }
extern "C" int helm_num_blocks(const helm_op *op) { return op ? op->nblocks : HELM_ERR_ARG; }
extern "C" long long helm_num_points(const helm_op *op) { return op ? op->N : HELM_ERR_ARG; }

// The few small kernels of an operator's set-up (default density, assembly) go to a stream of another priority class than the operator's own for the duration of
// the call.  Streams of one priority class share a handful of hardware queues, each of them in order: on the operator's normal-priority stream an 8-us kernel of
// the NEXT operator's set-up sat behind whatever solve had been queued on the same hardware queue -- helm_set_model / helm_assemble took 10-20 ms of the
// pipeline's prepare thread in every other set (tools/pipeline_timeline.py: the call ended when the other thread's helm_solve_device did).  The low class is
// used by nothing else on the 2-D path.  Top-level operators only: a multigrid level's operator shares its parent's stream and must stay in its order.
namespace {
struct SetupStream {
    helm_op *op; hipStream_t keep, tmp = nullptr; int prio;
    explicit SetupStream(helm_op *o) : op(o), keep(o->stream) {
        static const int pr = getenv("HELM_SETUP_PRIO") ? atoi(getenv("HELM_SETUP_PRIO")) : -1;
        prio = pr;
        if (pr == 0 || !o->own_stream || o->block0_only || !keep) return;
        if (hipStreamSynchronize(keep) != hipSuccess) { (void)hipGetLastError(); return; }        // (nothing of this operator is in flight when its model or frequency changes)
        tmp = helm_stream_acquire(o->device, prio);
        if (tmp) o->stream = tmp;
    }
    ~SetupStream() {
        if (!tmp) return;
        (void)hipStreamSynchronize(tmp);
        op->stream = keep;
        helm_stream_release(op->device, prio, tmp);
    }
};
}

extern "C" int helm_set_model(helm_op *op, const double *c, const double *rho, const double *theta, const double *eps, const double *delta) {
    helm_tuning_refresh();
    if (!op || !c) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const size_t N = (size_t)op->N;
    SetupStream setup_stream(op);
    if (helm_upload_staged(op, op->d_c, c, N * sizeof(cplx))) return HELM_ERR_DEVICE;
    if (!rho) {   // Gardner default 310 * Re(c)^0.25  (discretization.py:70), evaluated on the device
        const int rcg = helm_launch_gardner_rho(op);
        if (rcg) return rcg;
    } else {
        if (helm_upload_staged(op, op->d_rho, rho, N * sizeof(double))) return HELM_ERR_DEVICE;
    }
    op->aniso = false;
    bool m3zero = true;
    if (op->variant == HELM_EURUS) {
        auto up = [&](double *&dst, const double *src) -> int {
            if (!src) { if (dst) { helm_pool_free(op->device, dst, N * sizeof(double)); dst = nullptr; } return 0; }
            if (!dst) { dst = (double *)helm_pool_alloc(op->device, N * sizeof(double)); if (!dst) return -1; }
            return helm_upload_staged(op, dst, src, N * sizeof(double)) ? -1 : 0;
        };
        if (up(op->d_theta, theta) || up(op->d_eps, eps) || up(op->d_delta, delta)) HELM_FAIL(op, HELM_ERR_DEVICE, "anisotropy upload failed");
        op->aniso = theta || eps || delta;
        for (size_t i = 0; i < N && m3zero; ++i) {
            const double e = eps ? eps[i] : 0.0, d = delta ? delta[i] : 0.0;
            if (e != d) m3zero = false;
        }
    }
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    // host copies are only needed to build the multigrid levels: fetched back from the device if that ever happens
    op->h_c.clear(); op->h_rho.clear(); op->h_theta.clear(); op->h_eps.clear(); op->h_delta.clear();
    op->block_zero[0] = op->block_zero[1] = op->block_zero[3] = false;
    op->block_zero[2] = m3zero;
    op->has_model = true;
    op->assembled = false;
    return HELM_OK;
}

// The model of an operator that lives on the device already (a multigrid level: the caller's arrays, or values a kernel has put into
// dst->d_c / dst->d_rho -- then both pointers are null): device-to-device, nothing visits the host.  Isotropic operators only.
int helm_adopt_model_device(helm_op *dst, const cplx *d_c, const double *d_rho) {
    if (!dst || (d_c == nullptr) != (d_rho == nullptr)) return HELM_ERR_ARG;
    HIP_TRY(dst, hipSetDevice(dst->device));
    const size_t N = (size_t)dst->N;
    if (d_c) {
        HIP_TRY(dst, hipMemcpyAsync(dst->d_c, d_c, N * sizeof(cplx), hipMemcpyDeviceToDevice, dst->stream));
        HIP_TRY(dst, hipMemcpyAsync(dst->d_rho, d_rho, N * sizeof(double), hipMemcpyDeviceToDevice, dst->stream));
    }
    dst->aniso = false;
    dst->h_c.clear(); dst->h_rho.clear(); dst->h_theta.clear(); dst->h_eps.clear(); dst->h_delta.clear();
    dst->block_zero[0] = dst->block_zero[1] = dst->block_zero[3] = false;
    dst->block_zero[2] = true;
    dst->has_model = true;
    dst->assembled = false;
    return HELM_OK;
}

int helm_ensure_host_model(helm_op *op) {
    if (!op->has_model) HELM_FAIL(op, HELM_ERR_STATE, "model not set");
    if (!op->h_c.empty()) return HELM_OK;
    const size_t N = (size_t)op->N;
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    op->h_c.resize(N); op->h_rho.resize(N);
    HIP_TRY(op, hipMemcpy(op->h_c.data(), op->d_c, N * sizeof(cplx), hipMemcpyDeviceToHost));
    HIP_TRY(op, hipMemcpy(op->h_rho.data(), op->d_rho, N * sizeof(double), hipMemcpyDeviceToHost));
    auto down = [&](std::vector<double> &dst, const double *src) -> int {
        dst.clear();
        if (!src) return 0;
        dst.resize(N);
        return hipMemcpy(dst.data(), src, N * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
    };
    if (down(op->h_theta, op->d_theta) || down(op->h_eps, op->d_eps) || down(op->h_delta, op->d_delta)) HELM_FAIL(op, HELM_ERR_DEVICE, "model download failed");
    return HELM_OK;
}

extern "C" int helm_assemble(helm_op *op, double freq_re, double freq_im, double tau, double ky, double cPML) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    if (!op->has_model) HELM_FAIL(op, HELM_ERR_STATE, "helm_set_model must be called before helm_assemble");
    HIP_TRY(op, hipSetDevice(op->device));
    helm_pf_retire(op);                          // a factorisation still in flight belongs to the operator that is being replaced
    // Eurus with eps == delta is block-triangular and an N-row right-hand side (what the surveys bring, eurus.py:512-533) touches M1 alone: M2 .. M4 -- three
    // quarters of the 604 MB the assembly writes at 1024^2 -- are built when something asks for them (helm_need_all_blocks: a stacked 2N right-hand side,
    // helm_get_diagonals, an apply of another block, the scaled planes of the Krylov paths)
    op->asm_nblk = (op->variant == HELM_EURUS && op->block_zero[2] && !op->block0_only && helm_tuning_now().auto_direct != 0) ? 1 : 4;
    if (op->variant == HELM_EURUS && op->transposed_next && !op->block_zero[2])
        HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "helm_assemble: the handle was asked for M1^T (helm_set_transposed_m1) but its model now has eps != delta: the coupled 2N system has no transposed solve");
    op->transposed = op->transposed_next;        // (helm_set_transposed: in force from here; assemble.hip leaves the planes of A^T in d_C)
    if (op->variant == HELM_EURUS) {
        if (op->transposed) op->asm_nblk = 1;    // (M1^T alone: a transposed Eurus handle serves the direct path and N-row right-hand sides only)
        helm_eu_params_drop(op);                 // (the PML profiles belong to the frequency that is being replaced)
    }
    SetupStream setup_stream(op);
    int rc = op->ny > 0 ? helm3d_launch_assemble(op, freq_re, freq_im, tau, cPML) : helm_launch_assemble(op, freq_re, freq_im, tau, ky, cPML);
    if (rc) return rc;
    op->scaled_ok = false;
    if (op->block0_only) { rc = helm_ensure_scaled(op); if (rc) return rc; }     // multigrid levels always smooth with 1/diag
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    op->assembled = true;
    op->a_freq_re = freq_re; op->a_freq_im = freq_im; op->a_tau = tau; op->a_ky = ky; op->a_cpml = cPML;
    if (op->mg || op->mg3) mg_destroy(op);      // preconditioner belongs to the previous frequency
    op->mg3_no_keep = false;
    for (int b = 0; b < 4; ++b) { nd_free(op->direct[b]); op->direct[b] = nullptr; }   // and so do the direct factors
    op->direct_failed = false;
    return HELM_OK;
}

// The next helm_assemble leaves A^T in the handle (on != 0) or A again (0); what the handle holds until then is unchanged, but what was derived from it
// -- a factorisation in flight or kept, the scaled planes, the preconditioner -- is dropped as a re-assembly drops it.  2-D MiniZephyr handles (the
// single-block 9-point system); Eurus and 3-D handles: HELM_ERR_UNSUPPORTED.
extern "C" int helm_set_transposed(helm_op *op, int on) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    if (op->variant != HELM_MINIZEPHYR || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "helm_set_transposed: the transposed operator exists for 2-D MiniZephyr handles (not Eurus, not 3-D)");
    const bool want = on != 0;
    if (want == op->transposed_next) return HELM_OK;
    HIP_TRY(op, hipSetDevice(op->device));
    helm_pf_retire(op);
    op->transposed_next = want;
    op->scaled_ok = false;
    if (op->mg || op->mg3) mg_destroy(op);
    op->mg3_no_keep = false;
    for (int b = 0; b < 4; ++b) { nd_free(op->direct[b]); op->direct[b] = nullptr; }
    op->direct_failed = false;
    return HELM_OK;
}
// The next helm_assemble leaves M1^T in block 0 of a 2-D Eurus handle (on != 0) or M1 again (0), as helm_set_transposed does for MiniZephyr.  Only where the model
// has eps == delta everywhere: then an N-row right-hand side is solved through M1 alone, and M1^T serves the exact adjoint.  The coupled system has no transposed solve.
extern "C" int helm_set_transposed_m1(helm_op *op, int on) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    if (op->variant != HELM_EURUS || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "helm_set_transposed_m1: M1^T exists for 2-D Eurus handles (MiniZephyr handles take helm_set_transposed)");
    if (!op->has_model) HELM_FAIL(op, HELM_ERR_STATE, "helm_set_transposed_m1: helm_set_model must be called first (whether eps == delta decides)");
    if (on && !op->block_zero[2]) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "helm_set_transposed_m1: the model has eps != delta, so the two fields are coupled: the coupled 2N x 2N system [[M1, M2], [M3, M4]] has no transposed solve");
    const bool want = on != 0;
    if (want == op->transposed_next) return HELM_OK;
    HIP_TRY(op, hipSetDevice(op->device));
    helm_pf_retire(op);
    op->transposed_next = want;
    op->scaled_ok = false;
    if (op->mg || op->mg3) mg_destroy(op);
    op->mg3_no_keep = false;
    for (int b = 0; b < 4; ++b) { nd_free(op->direct[b]); op->direct[b] = nullptr; }
    op->direct_failed = false;
    return HELM_OK;
}
// The same for a 3-D handle (helm_create3d), through an entry point of its own as Eurus has one: the next helm_assemble leaves the 27 planes of A^T in the handle
// (k_transpose_planes3), the levels of both multigrid set-ups are then transposed too and the apply reads stored planes.  Any other handle: HELM_ERR_UNSUPPORTED.
extern "C" int helm_set_transposed3d(helm_op *op, int on) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    if (op->variant != HELM_3D || op->ny <= 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "helm_set_transposed3d: the 27 transposed planes exist for 3-D handles (helm_create3d); 2-D MiniZephyr handles take helm_set_transposed");
    const bool want = on != 0;
    if (want == op->transposed_next) return HELM_OK;
    HIP_TRY(op, hipSetDevice(op->device));
    helm_pf_retire(op);
    op->transposed_next = want;
    op->scaled_ok = false;
    if (op->mg || op->mg3) mg_destroy(op);
    op->mg3_no_keep = false;
    op->direct_failed = false;
    return HELM_OK;
}
// on != 0: helm_stencil_sources[_c64]_device and helm_lag_imaging_accumulate[_c64]_device, which read nothing but nine planes and the grid, serve this 2-D Eurus
// handle (the derivative routes of an Eurus problem run them on the planes of helm_eurus_planes_device); 0, the default: they refuse it as they always did.
extern "C" int helm_set_eurus_derivatives(helm_op *op, int on) {
    if (!op) return HELM_ERR_ARG;
    if (op->variant != HELM_EURUS || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "helm_set_eurus_derivatives: a 2-D Eurus handle is what opts in");
    op->eu_derivatives = on != 0;
    return HELM_OK;
}
extern "C" int helm_get_transposed(const helm_op *op) { return op ? (op->transposed ? 1 : 0) : HELM_ERR_ARG; }

int helm_need_all_blocks(helm_op *op) {
    if (op->variant == HELM_EURUS && op->transposed && op->ny == 0)
        HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the handle holds M1^T (helm_set_transposed_m1): it serves the direct path and N-row right-hand sides only -- M2 .. M4, a stacked 2N right-hand side and the scaled planes of the Krylov paths belong to the untransposed coupled system");
    if (op->variant != HELM_EURUS || op->block0_only || op->ny > 0 || !op->assembled || op->blocks_ready >= op->nblocks) return HELM_OK;
    op->asm_nblk = 4;                            // (M1 is written again with the same values: a factorisation reading it meanwhile sees no change)
    return helm_launch_assemble(op, op->a_freq_re, op->a_freq_im, op->a_tau, op->a_ky, op->a_cpml);
}

int helm_ensure_scaled(helm_op *op) {
    if (op->scaled_ok) return HELM_OK;
    { const int rcb = helm_need_all_blocks(op); if (rcb) return rcb; }
    const size_t N = (size_t)op->N;
    if (!op->d_Cs) op->d_Cs = (cplx *)helm_pool_alloc(op->device, (size_t)op->nblocks * op->nplanes * N * sizeof(cplx));
    if (!op->d_dinv) op->d_dinv = (cplx *)helm_pool_alloc(op->device, (size_t)op->nblocks * N * sizeof(cplx));
    if (!op->d_Cs || !op->d_dinv) HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc of the scaled coefficient planes failed");
    const int rc = helm_launch_scale_planes(op);
    if (rc) return rc;
    op->scaled_ok = true;
    return HELM_OK;
}

extern "C" int helm_get_diagonals(helm_op *op, double *out) {
    helm_tuning_refresh();
    if (!op || !out) return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "operator not assembled");
    HIP_TRY(op, hipSetDevice(op->device));
    { const int rcb = helm_need_all_blocks(op); if (rcb) return rcb; }
    if (helm_download_staged(op, out, op->d_C, (size_t)op->nblocks * op->nplanes * op->N * sizeof(cplx))) return HELM_ERR_DEVICE;
    return HELM_OK;
}

// One block of the planes: what helm_get_diagonals returns for that block alone.  Block 0 of a lazily assembled or transposed Eurus handle needs nothing else.
extern "C" int helm_get_block_diagonals(helm_op *op, int block, double *out) {
    helm_tuning_refresh();
    if (!op || !out || block < 0 || block >= op->nblocks) return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "operator not assembled");
    HIP_TRY(op, hipSetDevice(op->device));
    if (block > 0) { const int rcb = helm_need_all_blocks(op); if (rcb) return rcb; }
    const size_t bb = (size_t)op->nplanes * op->N * sizeof(cplx);
    if (helm_download_staged(op, out, op->d_C + (size_t)block * op->nplanes * op->N, bb)) return HELM_ERR_DEVICE;
    return HELM_OK;
}

static void timing_begin(helm_op *op) {
    if (!op->pf_pending) {       // (the launches of a factorisation started by helm_prefactor are booked with the solve that uses it)
        timing_reset_events(op);
    }
    op->timing.apply_ms = 0; op->timing.apply_launches = 0; op->timing.apply_bytes = 0;
    op->timing.factor_ms = 0; op->timing.gemm_ms = 0; op->timing.gemm_launches = 0; op->timing.gemm_flops = 0; op->timing.gemm_bytes = 0; op->timing.gemm_sol_ms = 0;
    op->timing.gemm_big_ms = 0; op->timing.gemm_big_launches = 0; op->timing.gemm_big_flops = 0;
}
static void timing_collect(helm_op *op) {
    for (auto &pr : op->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, op->ev_pool[pr.first], op->ev_pool[pr.first + 1]) == hipSuccess) {
            op->timing.apply_ms += ms; op->timing.apply_launches += 1; op->timing.apply_bytes += pr.second;
        }
    }
    op->ev_pending.clear();
    static const int gemm_log = getenv("HELM_GEMM_LOG") ? atoi(getenv("HELM_GEMM_LOG")) : 0;
    for (size_t i = 0; i < op->ev_pending_gemm.size(); ++i) {
        const std::pair<int, double> &pr = op->ev_pending_gemm[i];
        const int nl = i < op->ev_pending_gemm_n.size() ? op->ev_pending_gemm_n[i] : 1;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, op->ev_pool[pr.first], op->ev_pool[pr.first + 1]) == hipSuccess) {
            if (gemm_log && 5 * i + 4 < op->ev_pending_gemm_shape.size()) {
                const long long *sh = &op->ev_pending_gemm_shape[5 * i];
                fprintf(stderr, "[gemm log] M %lld N %lld K %lld batch %lld mode %lld : %.1f us, %.2f TFLOP/s, %.0f GB/s of operands\n", sh[0], sh[1], sh[2], sh[3], sh[4],
                        1e3 * ms, pr.second / (ms * 1e-3) / 1e12, (i < op->ev_pending_gemm_bytes.size() ? op->ev_pending_gemm_bytes[i] : 0.0) / (ms * 1e-3) / 1e9);
            }
            op->timing.gemm_ms += ms; op->timing.gemm_launches += nl; op->timing.gemm_flops += pr.second;
            if (i < op->ev_pending_gemm_bytes.size()) { op->timing.gemm_bytes += op->ev_pending_gemm_bytes[i]; op->timing.gemm_sol_ms += op->ev_pending_gemm_sol[i]; }
            if (pr.second >= 1e9 * nl) { op->timing.gemm_big_ms += ms; op->timing.gemm_big_launches += nl; op->timing.gemm_big_flops += pr.second; }
        }
    }
    op->ev_pending_gemm.clear(); op->ev_pending_gemm_n.clear(); op->ev_pending_gemm_bytes.clear(); op->ev_pending_gemm_sol.clear(); op->ev_pending_gemm_shape.clear();
    op->ev_used = 0;
}

// ---- apply -----------------------------------------------------------------------------------
extern "C" int helm_apply_device(helm_op *op, int block, int adjoint, const void *dX, void *dY, int nrhs) {
    helm_tuning_refresh();
    if (!op || !dX || !dY || nrhs < 1 || block < 0 || block >= op->nblocks) return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "operator not assembled");
    HIP_TRY(op, hipSetDevice(op->device));
    if (block > 0) { const int rcb = helm_need_all_blocks(op); if (rcb) return rcb; }
    timing_begin(op);
    ApplyArgs a = ApplyArgs();
    a.planes = op->d_C + (long long)block * op->nplanes * op->N; a.X = (const cplx *)dX; a.Y = (cplx *)dY; a.W = nullptr;
    a.ld = op->N; a.nrhs = nrhs; a.scaled = 0; a.adjoint = adjoint ? 1 : 0; a.epi = EPI_NONE; a.scal = nullptr; a.part = nullptr;
    int rc = helm_launch_apply(op, a);
    if (rc) return rc;
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    timing_collect(op);
    return HELM_OK;
}

extern "C" int helm_apply(helm_op *op, int block, int adjoint, const double *X, double *Y, int nrhs) {
    helm_tuning_refresh();
    if (!op || !X || !Y || nrhs < 1) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const size_t bytes = (size_t)nrhs * op->N * sizeof(cplx);
    void *dX = nullptr, *dY = nullptr;
    HIP_TRY(op, hipMalloc(&dX, bytes));
    if (hipMalloc(&dY, bytes) != hipSuccess) { hipFree(dX); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
    int rc = HELM_OK;
    if (helm_upload_staged(op, dX, X, bytes)) rc = HELM_ERR_DEVICE;
    if (!rc) rc = helm_apply_device(op, block, adjoint, dX, dY, nrhs);
    if (!rc && helm_download_staged(op, Y, dY, bytes)) rc = HELM_ERR_DEVICE;
    hipFree(dX); hipFree(dY);
    return rc;
}

// ---- solve dispatch ---------------------------------------------------------------------------
namespace {
// One block solve of helm_solve_device (arguments as solve_block_direct, solve_internal.hpp): the method the options name; HELM_AUTO is the direct
// path wherever it applies, and the Krylov path for what that path could not do.
int solve_block(helm_op *op, int block, const cplx *dRHS, long long rhs_ld, long long row_off, cplx premul,
                const cplx *sub, cplx *dXout, int nrhs, const helm_solve_opts &o, helm_solve_info *info,
                int sys2 = 0, long long rows_in = 0, cplx *dUconj = nullptr, bool *wrote_u = nullptr) {
    // dUconj / wrote_u: the direct path can leave conj(x) straight in the caller's output (then *wrote_u = true and dXout is
    // untouched); every other path fills dXout
    const long long N = op->N;
    if (wrote_u) *wrote_u = false;
    if (o.method == HELM_DIRECT) {
        if (op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the direct solver is 2-D only");
        const int rcd = solve_block_direct(op, block, dRHS, rhs_ld, row_off, premul, sub, dXout, nrhs, o, info, sys2, rows_in, dUconj);
        if (rcd >= 0 && wrote_u && dUconj && !sys2) *wrote_u = true;
        return rcd;
    }
    // AUTO: the sparse direct path wherever it applies (2-D single-block systems that fit), else / on failure the
    // multigrid-preconditioned Krylov path below
    if (o.method == HELM_AUTO && op->ny == 0 && !op->direct_failed) {
        if (helm_tuning_now().auto_direct != 0) {
            std::vector<helm_solve_info> saved;
            if (info) saved.assign(info, info + nrhs);
            // what THIS call's direct pass found, apart from what earlier blocks of the same solve left in `info` (stacked Eurus: block 3, then 0)
            std::vector<helm_solve_info> cur(nrhs);
            for (helm_solve_info &c : cur) { c.iterations = 0; c.status = 0; c.restarts = 0; c.method = HELM_DIRECT; c.relres = 0.0; }
            const int rc = solve_block_direct(op, block, dRHS, rhs_ld, row_off, premul, sub, dXout, nrhs, o, cur.data(), sys2, rows_in, dUconj);
            auto merge_cur = [&](int b) {
                helm_solve_info &I = info[b];
                I.iterations += cur[b].iterations; I.method = cur[b].method;
                I.relres = std::max(I.relres, cur[b].relres);
                I.status = merge_status(I.status, cur[b].status);
            };
            if (rc >= 0 && info && !(rc > 0 && !sys2 && rc < nrhs)) for (int b = 0; b < nrhs; ++b) merge_cur(b);
            if (rc == 0) { if (wrote_u && dUconj && !sys2) *wrote_u = true; return 0; }
            // the coupled system has no better fallback: row-equilibrated CGNR needs 10^4-10^5 iterations and meets the same
            // fp64 floor of the true residual, so right-hand sides that stalled above rtol are reported as such
            if (rc > 0 && sys2) return rc;
            op->direct_failed = true;
            // the factors are of no further use to this handle: give the (multi-GB) storage back now, not at the next assemble
            { const int slot = sys2 ? 1 : block; nd_free(op->direct[slot]); op->direct[slot] = nullptr; }
            if (rc > 0 && info && !sys2 && rc < nrhs) {
                // some right-hand sides stalled above rtol: only those go to the Krylov path (packed into a narrower batch);
                // the converged ones keep the direct result
                // (status 1 or 2 of the direct pass; those at the fp64 floor -- status 3 -- are solved: no Krylov method gets below it either)
                std::vector<int> bad;
                for (int b = 0; b < nrhs; ++b) { if (cur[b].status == 1 || cur[b].status == 2) bad.push_back(b); else merge_cur(b); }
                const int k = (int)bad.size();
                const size_t colb = (size_t)N * sizeof(cplx);
                cplx *tR = (cplx *)helm_pool_alloc(op->device, (size_t)k * colb), *tX = (cplx *)helm_pool_alloc(op->device, (size_t)k * colb);
                cplx *tS = sub ? (cplx *)helm_pool_alloc(op->device, (size_t)k * colb) : nullptr;
                auto release = [&]() { hipStreamSynchronize(op->stream); helm_pool_free(op->device, tR, (size_t)k * colb); helm_pool_free(op->device, tX, (size_t)k * colb);
                                       helm_pool_free(op->device, tS, (size_t)k * colb); };
                if (!tR || !tX || (sub && !tS)) { release(); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
                for (int j = 0; j < k; ++j) {
                    hipMemcpyAsync(tR + (long long)j * N, dRHS + (long long)bad[j] * rhs_ld + row_off, colb, hipMemcpyDeviceToDevice, op->stream);
                    if (sub) hipMemcpyAsync(tS + (long long)j * N, sub + (long long)bad[j] * N, colb, hipMemcpyDeviceToDevice, op->stream);
                }
                std::vector<helm_solve_info> ki(k);
                for (int j = 0; j < k; ++j) ki[j] = saved[bad[j]];
                const int rck = solve_block(op, block, tR, N, 0, premul, tS, tX, k, o, ki.data());
                if (rck < 0) { release(); return rck; }
                const bool cj = dUconj != nullptr;
                for (int j = 0; j < k; ++j) {
                    info[bad[j]] = ki[j];
                    if (cj) helm_launch_finish(op, tX, N, (long long)j * N, dUconj + (long long)bad[j] * N, N, 0, 1);
                    else hipMemcpyAsync(dXout + (long long)bad[j] * N, tX + (long long)j * N, colb, hipMemcpyDeviceToDevice, op->stream);
                }
                release();
                if (wrote_u && cj) *wrote_u = true;
                return rck;
            }
            if (info) std::copy(saved.begin(), saved.end(), info);
        }
    }
    if (op->variant == HELM_EURUS && op->transposed)
        HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the handle holds M1^T (helm_set_transposed_m1): it is solved by the direct path only -- the Krylov path (method, or the fallback after a failed factorisation) is not served for it");
    return solve_block_krylov(op, block, dRHS, rhs_ld, row_off, premul, sub, dXout, nrhs, o, info, sys2, rows_in);
}
}  // namespace

// Scratch for `concurrent` host-array solves (helm_solve / helm_solve_coo) of nrhs right-hand sides running on this handle's GPU at the
// same time, brought into being NOW: the shared scratch slots of the direct path and the device images of the right-hand sides and
// wavefields (three buffers per call).  Everything here is taken lazily anyway; but a hipMalloc issued while other host threads have
// kernels and copies in flight was measured at 0.7-1.5 s (HELM_ALLOC_TRACE=1), so a dispatcher that knows how many workers it is
// about to start on a GPU asks once, before they run.  A hint: errors other than bad arguments are swallowed.
extern "C" int helm_reserve(helm_op *op, int nrhs, long long rows, int concurrent) {
    helm_tuning_refresh();
    if (!op || nrhs < 1 || rows < 1 || concurrent < 1) return HELM_ERR_ARG;
    if (hipSetDevice(op->device) != hipSuccess) { (void)hipGetLastError(); return HELM_OK; }
    if (concurrent > 64) concurrent = 64;
    const size_t bytes = (size_t)nrhs * rows * sizeof(cplx);
    {   // device images: idle buffers of that size the pool holds already count
        const size_t have = helm_pool_idle_count(op->device, bytes);
        std::vector<void *> got;
        for (size_t k = have; k < (size_t)3 * concurrent; ++k) {
            void *p = nullptr;
            if (helm_malloc_retry(op->device, &p, bytes) != hipSuccess) break;
            got.push_back(p);
        }
        for (void *p : got) helm_pool_free(op->device, p, bytes);
    }
    if (!direct_path_ok(op)) return HELM_OK;
    const helm_tuning tune = helm_tuning_now();
    std::shared_ptr<NdPlanDev> pd;
    if (nd_get_plan(op, tune.nd_leaf, 1, &pd) != HELM_OK || !pd) return HELM_OK;
    const size_t wsb = direct_batch(pd->plan, op->N, nrhs, 0, 0, tune).bytes();      // (what a solve with the default batch option leases once the factors exist)
    const int ready = ws_reserve(op->device, wsb, concurrent);      // this device's own table: booking for one GPU never touches another's
    // more concurrent solves than slots (several workers per GPU): the others fall back to their handle's own workspace, which comes from the
    // size-keyed pool -- put that many buffers there now, as long as they fit beside everything else (half of what is free)
    if (concurrent > ready) {
        size_t freeb = 0, totb = 0;
        const size_t have = helm_pool_idle_count(op->device, wsb);
        if (hipMemGetInfo(&freeb, &totb) != hipSuccess) { (void)hipGetLastError(); freeb = 0; }
        std::vector<void *> got;
        for (size_t k = have; k < (size_t)(concurrent - ready) && (got.size() + 1) * wsb <= freeb / 2; ++k) {
            void *p = nullptr;
            AllocTrace tr("ws fallback", wsb);
            if (hipMalloc(&p, wsb) != hipSuccess) { (void)hipGetLastError(); break; }
            got.push_back(p);
        }
        for (void *p : got) helm_pool_free(op->device, p, wsb);
    }
    return HELM_OK;
}

extern "C" int helm_solve_device(helm_op *op, const void *dRHS, void *dU, int nrhs, long long rows,
                                 double premul_re, double premul_im, const helm_solve_opts *opts, helm_solve_info *info) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    // a declared support (helm_set_rhs_support) belongs to THIS call's right-hand sides and to no later one -- whichever way the call ends, the
    // early returns below included (the bits usually live in a buffer the caller recycles as soon as this returns)
    struct SupportOneShot { helm_op *o; ~SupportOneShot() { o->rhs_bits = nullptr; o->rhs_bits_q = nullptr; o->rhs_bits_violated = 0; } } support_one_shot{op};
    if (!dRHS || !dU || nrhs < 1) return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "operator not assembled");
    const long long N = op->N;
    const bool stacked = (op->variant == HELM_EURUS && rows == 2 * N);
    if (rows != N && !stacked) HELM_FAIL(op, HELM_ERR_ARG, "dimension mismatch: rhs has %lld rows, operator has %lld%s", rows, N,
                                         op->variant == HELM_EURUS ? " (or 2N stacked)" : "");
    HIP_TRY(op, hipSetDevice(op->device));
    if (stacked) { const int rcb = helm_need_all_blocks(op); if (rcb) return rcb; }      // (u = M1^-1 (q1 - M2 M4^-1 q2): M2 and M4 are needed now)
    if (op->rhs_bits && (op->rhs_bits_rows != rows || op->rhs_bits_nrhs != nrhs)) HELM_FAIL(op, HELM_ERR_ARG, "helm_set_rhs_support was given %lld rows x %d right-hand sides, this solve has %lld x %d", op->rhs_bits_rows, op->rhs_bits_nrhs, rows, nrhs);
    op->rhs_bits_q = op->rhs_bits ? dRHS : nullptr;
    helm_solve_opts o;
    if (opts) o = *opts; else { o.method = HELM_AUTO; o.rtol = 1e-10; o.maxit = 200000; o.check_every = 0; o.batch = 0; o.flags = 0; }
    if (!(o.rtol > 0)) o.rtol = 1e-10;
    if (o.maxit < 1) o.maxit = 200000;
    if (!op->direct[0] && !op->pf_pending) { op->rtol_hint = o.rtol; op->rtol_hint_set = true; }      // (factors that exist, or are on their way, were conditioned for the hint they were given)
    if (info) for (int r = 0; r < nrhs; ++r) { info[r].iterations = 0; info[r].status = 0; info[r].restarts = 0; info[r].method = o.method; info[r].relres = 0.0; }
    const cplx premul = cmake(premul_re, premul_im);

    hipEvent_t e0, e1;
    HIP_TRY(op, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); HELM_FAIL(op, HELM_ERR_DEVICE, "hipEventCreate failed"); }
    timing_begin(op);
    HIP_TRY(op, hipEventRecord(e0, op->stream));

    int result = 0;
    const size_t xbytes = (size_t)nrhs * N * sizeof(cplx);
    cplx *dX = (cplx *)helm_pool_alloc(op->device, xbytes);
    if (!dX) { hipEventDestroy(e0); hipEventDestroy(e1); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
    // Buffer layouts (opts.flags): HELM_RHS_NODE_MAJOR / HELM_OUT_NODE_MAJOR = the reference's (rows, nrhs) C-order arrays.  The direct path
    // takes both natively for one batch of a single-block system (no transposes at all); every other combination goes through rhs-major
    // temporaries here, so all paths below see one right-hand side per row.
    const int lay = o.flags & HELM_NODE_MAJOR;
    o.flags &= ~HELM_NODE_MAJOR;
    const void *dRHS_use = dRHS; void *dU_use = dU;
    cplx *tR = nullptr, *tU = nullptr;
    const size_t lbytes = (size_t)nrhs * rows * sizeof(cplx);
    auto cleanup = [&]() { hipStreamSynchronize(op->stream); helm_pool_free(op->device, dX, xbytes); helm_pool_free(op->device, tR, lbytes); helm_pool_free(op->device, tU, lbytes);
                           hipEventDestroy(e0); hipEventDestroy(e1); };
    bool native_done = false;
    if (lay == HELM_NODE_MAJOR && rows == N && (o.method == HELM_AUTO || o.method == HELM_DIRECT) && direct_path_ok(op, o.method == HELM_DIRECT) &&
        !testing_hook("HELM_ND_INJECT_STALL")) {
        helm_solve_opts on = o; on.flags |= HELM_NODE_MAJOR;
        const int rcn = solve_block_direct(op, 0, (const cplx *)dRHS, nrhs, 0, premul, nullptr, nullptr, nrhs, on, info, 0, 0, (cplx *)dU);
        if (op->rhs_bits_violated) { cleanup(); return HELM_ERR_ARG; }          // (HELM_ND_SUPPORT_CHECK: the message is set)
        if (rcn == 0) native_done = true;
        else if (info) for (int r = 0; r < nrhs; ++r) { info[r].iterations = 0; info[r].status = 0; info[r].restarts = 0; info[r].method = o.method; info[r].relres = 0.0; }
        // (anything else -- too many right-hand sides for one batch, a right-hand side above rtol, a failed factorisation: the general path)
    }
    if (lay && !native_done) {
        if (lay & HELM_RHS_NODE_MAJOR) {
            tR = (cplx *)helm_pool_alloc(op->device, lbytes);
            if (!tR) { cleanup(); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
            const int rct = nd_transpose(op, (const cplx *)dRHS, rows, nrhs, tR);
            if (rct) { cleanup(); return rct; }
            dRHS_use = tR;
        }
        if (lay & HELM_OUT_NODE_MAJOR) {
            tU = (cplx *)helm_pool_alloc(op->device, lbytes);
            if (!tU) { cleanup(); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
            dU_use = tU;
        }
    }

    if (native_done) {
    } else if (op->variant == HELM_EURUS && !op->block_zero[2]) {
        // eps != delta: M3 != 0, the two fields are coupled -> Jacobi-BiCGSTAB on the full 2N x 2N system
        // (eurus.py:430-464,512-533); N-row right-hand sides are zero-padded and the result clipped
        cplx *dW = nullptr;
        if (helm_malloc_retry(op->device, (void **)&dW, (size_t)nrhs * 2 * N * sizeof(cplx)) != hipSuccess) { cleanup(); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
        int rc = solve_block(op, 0, (const cplx *)dRHS_use, rows, 0, premul, nullptr, dW, nrhs, o, info, 1, rows);
        if (rc >= 0) {
            result = rc;
            rc = helm_launch_finish(op, dW, 2 * N, 0, (cplx *)dU_use, rows, 0, nrhs);
            if (!rc && stacked) rc = helm_launch_finish(op, dW, 2 * N, N, (cplx *)dU_use, rows, N, nrhs);
            if (!rc && hipStreamSynchronize(op->stream) != hipSuccess) rc = HELM_ERR_DEVICE;
        }
        hipFree(dW);
        if (rc < 0) { cleanup(); return rc; }
    } else if (op->variant == HELM_MINIZEPHYR || !stacked) {
        // Eurus with an N-row right-hand side: zero-padded second field => v = 0 and M1 u = q
        // when M3 == 0 (eurus.py:512-533)
        bool wrote_u = false;        // rows == N here: the direct path writes conj(x) into dU itself
        int rc = solve_block(op, 0, (const cplx *)dRHS_use, rows, 0, premul, nullptr, dX, nrhs, o, info, 0, 0, (cplx *)dU_use, &wrote_u);
        if (rc < 0) { cleanup(); return rc; }
        result = rc;
        if (!wrote_u) {
            rc = helm_launch_finish(op, dX, N, 0, (cplx *)dU_use, rows, 0, nrhs);
            if (rc) { cleanup(); return rc; }
        }
    } else {
        // block-triangular: v = M4^-1 q2 ; u = M1^-1 (q1 - M2 v)
        cplx *dV = nullptr, *dT = nullptr;
        if (helm_malloc_retry(op->device, (void **)&dV, (size_t)nrhs * N * sizeof(cplx)) != hipSuccess || helm_malloc_retry(op->device, (void **)&dT, (size_t)nrhs * N * sizeof(cplx)) != hipSuccess) {
            hipFree(dV); cleanup(); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed");
        }
        int rc = solve_block(op, 3, (const cplx *)dRHS_use, rows, N, premul, nullptr, dV, nrhs, o, info);
        if (rc >= 0) {
            result = rc;
            ApplyArgs a = ApplyArgs();
            a.planes = op->d_C + 1LL * 9 * N; a.X = dV; a.Y = dT; a.W = nullptr; a.ld = N; a.nrhs = nrhs; a.scaled = 0; a.adjoint = 0;
            a.epi = EPI_NONE; a.scal = nullptr; a.part = nullptr;
            rc = helm_launch_apply(op, a);
            if (!rc) rc = solve_block(op, 0, (const cplx *)dRHS_use, rows, 0, premul, dT, dX, nrhs, o, info);
            if (rc >= 0) {
                result = std::max(result, rc);
                rc = helm_launch_finish(op, dX, N, 0, (cplx *)dU_use, rows, 0, nrhs);
                if (!rc) rc = helm_launch_finish(op, dV, N, 0, (cplx *)dU_use, rows, N, nrhs);
            }
        }
        hipFree(dV); hipFree(dT);
        if (rc < 0) { cleanup(); return rc; }
    }
    if (tU) {
        const int rct = nd_transpose(op, tU, nrhs, rows, (cplx *)dU);
        if (rct) { cleanup(); return rct; }
    }
    HIP_TRY(op, hipEventRecord(e1, op->stream));
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    op->timing.solve_ms = ms;
    helm_pf_retire(op);
    timing_collect(op);
    cleanup();
    return result;
}

extern "C" int helm_solve(helm_op *op, const double *RHS, double *U, int nrhs, long long rows,
                          double premul_re, double premul_im, const helm_solve_opts *opts, helm_solve_info *info) {
    helm_tuning_refresh();
    if (!op || !RHS || !U || nrhs < 1) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const size_t bytes = (size_t)nrhs * rows * sizeof(cplx);
    void *dR = helm_pool_alloc(op->device, bytes), *dU = helm_pool_alloc(op->device, bytes);
    if (!dR || !dU) { helm_pool_free(op->device, dR, bytes); helm_pool_free(op->device, dU, bytes); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
    int rc = HELM_OK;
    if (helm_upload_staged(op, dR, RHS, bytes)) rc = HELM_ERR_DEVICE;
    if (!rc) rc = helm_solve_device(op, dR, dU, nrhs, rows, premul_re, premul_im, opts, info);
    if (rc >= 0 && helm_download_staged(op, U, dU, bytes)) rc = HELM_ERR_DEVICE;
    hipStreamSynchronize(op->stream);
    helm_pool_free(op->device, dR, bytes); helm_pool_free(op->device, dU, bytes);
    return rc;
}

// Declared support of right-hand sides (round 4).  The reference hands its sources over as scipy-sparse matrices (survey.py:86-89,162-188): where they are
// nonzero is part of the input, not something to be found.  bits: one byte per row (cell) on the device, bit b set = the right-hand sides of block b of
// 64 columns MAY be nonzero in that row (at most 512 right-hand sides); the caller guarantees zeros everywhere else.  One shot: it applies to the next
// helm_solve_device on this handle (same rows and right-hand-side count, node-major layout) and is forgotten when that call returns.  The direct path then
// sets the leaf flags of its forward pass from the bits instead of reading every right-hand-side row to look for nonzeros (3.2 of 4.3 GB at 1024^2 x 256).
// HELM_ND_SUPPORT_CHECK=1 verifies the guarantee (one pass over q) and fails the solve if it does not hold.
extern "C" int helm_set_rhs_support(helm_op *op, const void *d_bits, long long rows, int nrhs) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    if (!d_bits) { op->rhs_bits = nullptr; op->rhs_bits_q = nullptr; return HELM_OK; }
    if (rows < 1 || nrhs < 1 || nrhs > 512) HELM_FAIL(op, HELM_ERR_ARG, "helm_set_rhs_support: rows >= 1 and 1 <= nrhs <= 512");
    op->rhs_bits = (const unsigned char *)d_bits; op->rhs_bits_rows = rows; op->rhs_bits_nrhs = nrhs; op->rhs_bits_violated = 0;
    return HELM_OK;
}

// Pinned host memory for the caller's result arrays (recycled by size): device-to-host copies into it run at the PCIe rate, into
// pageable memory at a fraction of it.
extern "C" void *helm_host_alloc(size_t bytes) { return bytes ? helm_hostpool_alloc(bytes) : nullptr; }
extern "C" void helm_host_free(void *p, size_t bytes) { helm_hostpool_free(p, bytes); }

// Host-side sparse right-hand sides (the reference's scipy-sparse source matrices, survey.py:162-169): only the triplets cross PCIe,
// the dense right-hand sides exist on the device alone; the wavefields come back into U (host; pinned memory from helm_host_alloc
// makes that copy run at the PCIe rate).  Layout of U and of the implied dense right-hand sides per opts->flags.
extern "C" int helm_solve_coo(helm_op *op, const long long *row, const int *col, const double *val, long long nnz, double *U, int nrhs, long long rows,
                              double premul_re, double premul_im, const helm_solve_opts *opts, helm_solve_info *info) {
    helm_tuning_refresh();
    if (!op || !U || nrhs < 1 || rows < 1 || nnz < 0 || (nnz > 0 && (!row || !col || !val))) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const size_t bytes = (size_t)nrhs * rows * sizeof(cplx);
    // (+ one byte per row behind the triplets: the support of the dense image, see below -- no allocation of its own)
    const size_t tb0 = (((size_t)std::max<long long>(nnz, 1) * (sizeof(long long) + sizeof(int) + sizeof(cplx))) + 15) & ~(size_t)15;
    const size_t bbytes = (size_t)((rows + 3) / 4) * 4;
    const size_t tb = tb0 + bbytes;
    void *dR = helm_pool_alloc(op->device, bytes), *dU = helm_pool_alloc(op->device, bytes), *dT = helm_pool_alloc(op->device, tb);
    auto release = [&]() { hipStreamSynchronize(op->stream); helm_pool_free(op->device, dR, bytes); helm_pool_free(op->device, dU, bytes); helm_pool_free(op->device, dT, tb); };
    if (!dR || !dU || !dT) { release(); HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc failed"); }
    // packed as [val (16-byte entries) | row (8) | col (4)]: every array starts on a multiple of its own element size whatever the parity of nnz
    // (r3 packed row | val | col, which left val on an 8-byte boundary for odd nnz although the expansion kernel reads it as 16-byte vectors)
    cplx *d_val = (cplx *)dT; long long *d_row = (long long *)(d_val + std::max<long long>(nnz, 1)); int *d_col = (int *)(d_row + std::max<long long>(nnz, 1));
    int rc = HELM_OK;
    for (long long k = 0; k < nnz; ++k)              // the scatter trusts its indices: check them where they arrive
        if (row[k] < 0 || row[k] >= rows || col[k] < 0 || col[k] >= nrhs) {
            release();
            HELM_FAIL(op, HELM_ERR_ARG, "sparse right-hand side: entry %lld addresses (row %lld, column %d) outside the %lld x %d right-hand-side matrix", k, row[k], col[k], rows, nrhs);
        }
    if (nnz > 0 && (helm_upload_staged(op, d_row, row, nnz * sizeof(long long)) || helm_upload_staged(op, d_val, val, nnz * sizeof(cplx)) ||
                    helm_upload_staged(op, d_col, col, nnz * sizeof(int)))) rc = HELM_ERR_DEVICE;
    const int flags = opts ? opts->flags : 0;
    if (!rc) rc = helm_launch_rhs_from_coo(op, d_row, d_col, d_val, nnz, (cplx *)dR, nrhs, rows, (flags & HELM_RHS_NODE_MAJOR) ? 1 : 0);
    if (!rc && hipStreamSynchronize(op->stream) != hipSuccess) rc = HELM_ERR_DEVICE;
    // the dense image was made here from the triplets: its support is known exactly, the direct path need not look for it
    void *dBits = (char *)dT + tb0;
    if (!rc && nrhs <= 512 && (flags & HELM_NODE_MAJOR) == HELM_NODE_MAJOR && helm_rhs_support_from_coo(op, d_row, d_col, nnz, dBits, rows, nrhs) == HELM_OK)
        (void)helm_set_rhs_support(op, dBits, rows, nrhs);
    if (!rc) rc = helm_solve_device(op, dR, dU, nrhs, rows, premul_re, premul_im, opts, info);
    (void)helm_set_rhs_support(op, nullptr, 0, 0);          // (the bits live in dT, which goes back to the pool below: never leave a pointer to them behind)
    if (rc >= 0 && helm_download_staged(op, U, dU, bytes)) rc = HELM_ERR_DEVICE;
    release();
    return rc;
}
