// ngf_uv_inverse_train.hip -- C ABI (include/ngf.h: ngf_uv_inverse_trainer_*, ngf_uv_inverse_train_*): NeuTex's inverse gauge with a backward
// pass.  Kernels in ngf_uv_inverse_train.hpp.  A translation unit of its own: ngf_uv.hip, ngf_uv_inverse.hip and ngf_uv_train.hip keep their code.
#include "ngf_host.hpp"
#include "ngf_uv_inverse_train.hpp"

using namespace ngf;

namespace {
constexpr int NL = NGF_UV_INVERSE_LAYERS;
static_assert(NGF_UV_INVERSE_TRAIN_PARAMS == 2 * NL, "weight and bias of every layer");
}  // namespace

struct ngf_uv_inverse_trainer {
    int device = -1;
    int num_cus = 256;
    ngf_uv_inverse_desc desc{};
    UvInvShape shape{};
    int64_t cap = 0;
    DeviceAllocs mem{0, 16};                 // every device buffer of the handle
    float *w = nullptr;                      // the packed sets
    UvitPack pack{};
    UvInverseArgs fwd{};
    UvitDxArgs dx{};
    bool stale = true;                       // the packed sets are older than the caller's tensors
    float *uv = nullptr;                     // the last forward's points [n, D] (linear1's dW reads them)
    float *keep[NL - 1] = {}, *dz[NL - 1] = {};
    float *part = nullptr;
    double *partb = nullptr;
    float *grads = nullptr;
    int64_t grad_off[2 * NL] = {};
    int64_t grad_elems = 0;
    int64_t n = 0;                           // the last forward
    int64_t ticket = 0, next_ticket = 0;
    bool have_grads = false;
};

namespace {

int pack_weights(ngf_uv_inverse_trainer *t, hipStream_t st)
{
    int most = 0;
    for (int s = 0; s < t->pack.nseg; ++s) most = std::max(most, t->pack.seg[s].count);
    NGF_LAUNCH(uvit_pack_kernel, dim3(blocks(most), (unsigned)t->pack.nseg), dim3(256), 0, st, t->pack);
    t->stale = false;
    return NGF_OK;
}

// dW, db of layer l from its dZ and its input: partials over uvit_chunk(n)-row chunks, then the sum in chunk order
int weight_grads(ngf_uv_inverse_trainer *t, int l, const float *dz, int64_t ld_dz, const float *x, int64_t ld_x, hipStream_t st)
{
    UvitDw G{};
    G.dz = dz; G.ld_dz = ld_dz; G.x = x; G.ld_x = ld_x;
    G.part = t->part; G.partb = t->partb;
    G.rows = t->n; G.M = t->shape.out_f[l]; G.N = t->shape.in_f[l];
    G.chunk = (int32_t)uvit_chunk(t->n);
    const int nz = (int)((t->n + G.chunk - 1) / G.chunk);
    const dim3 grid(blocks(G.M, kUvitTile), blocks(G.N, kUvitTile), (unsigned)nz);
    const bool va = (G.M & 3) == 0 && (ld_dz & 3) == 0, vb = (G.N & 3) == 0 && (ld_x & 3) == 0;
    if (va && vb) NGF_LAUNCH((uvit_dw_kernel<true, true>), grid, dim3(256), 0, st, G);
    else if (va) NGF_LAUNCH((uvit_dw_kernel<true, false>), grid, dim3(256), 0, st, G);
    else if (vb) NGF_LAUNCH((uvit_dw_kernel<false, true>), grid, dim3(256), 0, st, G);
    else NGF_LAUNCH((uvit_dw_kernel<false, false>), grid, dim3(256), 0, st, G);
    const int64_t nk = (int64_t)G.M * G.N;
    NGF_LAUNCH(uvit_reduce_kernel, dim3(blocks(std::max<int64_t>(nk, G.M))), dim3(256), 0, st, (const float *)t->part, (const double *)t->partb, nk, G.M, nz,
               t->grads + t->grad_off[2 * l], t->grads + t->grad_off[2 * l + 1]);
    return NGF_OK;
}

}  // namespace

extern "C" {

int64_t ngf_uv_inverse_trainer_bytes(const ngf_uv_inverse_trainer *t) { return t ? t->mem.bytes : 0; }

int ngf_uv_inverse_trainer_destroy(ngf_uv_inverse_trainer *t)
{
    if (!t) return NGF_OK;
    {
        DeviceScope ds(t->device);
        t->mem.free_all();
    }
    delete t;
    return NGF_OK;
}

int ngf_uv_inverse_trainer_create(const ngf_uv_inverse_desc *d, int64_t max_points, ngf_uv_inverse_trainer **out, void *hip_stream)
{
    if (!d || !out) return fail(NGF_E_ARG, "ngf_uv_inverse_trainer_create: null argument");
    *out = nullptr;
    if (int rc = check_inverse_desc("ngf_uv_inverse_trainer_create", d)) return rc;
    if (max_points <= 0 || max_points >= (int64_t)1 << 27)
        return fail(NGF_E_ARG, "ngf_uv_inverse_trainer_create: max_points must be in 1 .. 2^27 - 1, got %lld", (long long)max_points);
    hipStream_t st = (hipStream_t)hip_stream;
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    ngf_uv_inverse_trainer *t = new (std::nothrow) ngf_uv_inverse_trainer();
    if (!t) return fail(NGF_E_HIP, "ngf_uv_inverse_trainer_create: out of host memory");
    t->device = dev;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) t->num_cus = prop.multiProcessorCount;
    t->desc = *d;
    t->cap = max_points;
    const int D = d->input_dim, H = kUvInvHidden;
    t->shape = uv_inverse_shape(D);
    const int *kOut = t->shape.out_f, *kIn = t->shape.in_f;
    int64_t g = 0;
    for (int l = 0; l < NL; ++l) {
        t->grad_off[2 * l] = g; g += (int64_t)kOut[l] * kIn[l];
        t->grad_off[2 * l + 1] = g; g += kOut[l];
        g = (g + 3) & ~(int64_t)3;
    }
    t->grad_elems = g;
    // the packed sets: uvit_pack_kernel's segments read the caller's tensors where they are
    const UvInvPlan P = uv_inverse_plan(D, d->w, d->b);
    const int64_t wfloats = P.floats;
    t->pack.nseg = P.nseg;
    std::copy(P.seg, P.seg + P.nseg, t->pack.seg);
    t->fwd.dim = t->dx.dim = D;
    t->fwd.at = P.fwd;
    t->dx.at = P.dx;
    // chunks of any batch the handle takes: uvit_chunk(n) >= 1024 rows, and at most 64 of them
    const int64_t nzmax = std::min<int64_t>(kUvitMaxChunks, (max_points + kUvitMinChunk - 1) / kUvitMinChunk);
    int rc = NGF_OK;
    auto F = [&](float **p, int64_t n) { if (!rc) rc = t->mem.alloc(p, (size_t)n); };
    F(&t->w, wfloats);
    F(&t->uv, max_points * D);
    for (int l = 0; l < NL - 1; ++l) { F(&t->keep[l], max_points * kOut[l]); F(&t->dz[l], max_points * kOut[l]); }
    F(&t->part, nzmax * H * H);
    if (!rc) rc = t->mem.alloc(&t->partb, (size_t)(nzmax * H));
    F(&t->grads, g);
    if (rc) { t->mem.free_all(); delete t; return rc; }
    if (hipMemsetAsync(t->w, 0, (size_t)wfloats * sizeof(float), st) != hipSuccess) {
        t->mem.free_all(); delete t;
        return fail(NGF_E_HIP, "ngf_uv_inverse_trainer_create: clearing the packed weights failed");
    }
    (void)hipStreamSynchronize(st);      // (the first forward may come on another stream)
    t->pack.dst = t->w;
    t->fwd.w = t->w;
    t->dx.w = t->w;
    for (int l = 0; l < NL - 1; ++l) { t->dx.keep[l] = t->keep[l]; t->dx.dz[l] = t->dz[l]; }
    *out = t;
    return NGF_OK;
}

int ngf_uv_inverse_train_params_changed(ngf_uv_inverse_trainer *t)
{
    if (!t) return fail(NGF_E_ARG, "ngf_uv_inverse_train_params_changed: null handle");
    t->stale = true;          // packed again, on the device, by the next forward
    return NGF_OK;
}

int ngf_uv_inverse_train_forward(ngf_uv_inverse_trainer *t, const float *uv, int64_t n, float *xyz, int64_t *ticket, void *hip_stream)
{
    if (!t || !ticket) return fail(NGF_E_ARG, "ngf_uv_inverse_train_forward: null %s", !t ? "handle" : "ticket");
    if (n < 0) return fail(NGF_E_ARG, "ngf_uv_inverse_train_forward: n=%lld", (long long)n);
    // n == 0 reads and writes nothing, so its pointers may be NULL (an empty tensor has no storage)
    if (n > 0 && (!uv || !xyz)) return fail(NGF_E_ARG, "ngf_uv_inverse_train_forward: null %s", !uv ? "uv" : "xyz");
    if (n > t->cap) return fail(NGF_E_ARG, "ngf_uv_inverse_train_forward: n=%lld exceeds max_points=%lld", (long long)n, (long long)t->cap);
    DeviceScope ds(t->device);
    hipStream_t st = (hipStream_t)hip_stream;
    t->have_grads = false;
    if (n > 0) {
        if (t->stale) {
            if (int rc = pack_weights(t, st)) return rc;
        }
        HIP_TRY(hipMemcpyAsync(t->uv, uv, (size_t)n * t->desc.input_dim * sizeof(float), hipMemcpyDeviceToDevice, st));
        UvitFwdArgs A{};
        A.q = t->fwd;
        A.q.uv = uv; A.q.xyz = xyz; A.q.n = n;
        for (int l = 0; l < NL - 1; ++l) A.keep[l] = t->keep[l];
        if (int rc = launch_inverse_tiles(uvit_forward_kernel, A, n, t->num_cus, st)) return rc;
    }
    t->n = n;
    t->ticket = ++t->next_ticket;
    *ticket = t->ticket;
    return NGF_OK;
}

}  // extern "C"

namespace {
// the backward of the forward named by `ticket`; with_dw = false: the dX chain alone (ngf_debug_uv_inverse_train_dx), no gradients are left
int backward(ngf_uv_inverse_trainer *t, const char *who, int64_t ticket, const float *d_xyz, float *d_uv, bool with_dw, hipStream_t st)
{
    if (!t || !d_xyz) return fail(NGF_E_ARG, "%s: null %s", who, !t ? "handle" : "d_xyz");
    if (ticket <= 0 || ticket != t->ticket)
        return fail(NGF_E_STALE, "%s: ticket %lld is not the trainer's last forward (%lld)", who, (long long)ticket, (long long)t->ticket);
    DeviceScope ds(t->device);
    t->have_grads = false;
    const int64_t n = t->n;
    if (n == 0) {
        if (!with_dw) return NGF_OK;
        HIP_TRY(hipMemsetAsync(t->grads, 0, (size_t)t->grad_elems * sizeof(float), st));
        t->have_grads = true;
        return NGF_OK;
    }
    UvitDxArgs Q = t->dx;
    Q.d_xyz = d_xyz; Q.d_uv = d_uv; Q.n = n;
    if (int rc = launch_inverse_tiles(uvit_dx_kernel, Q, n, t->num_cus, st)) return rc;
    if (!with_dw) return NGF_OK;
    const int D = t->desc.input_dim;
    int rc = weight_grads(t, 4, d_xyz, 3, t->keep[3], kUvInvHidden, st);
    for (int l = 3; l >= 1 && !rc; --l) rc = weight_grads(t, l, t->dz[l], t->shape.out_f[l], t->keep[l - 1], t->shape.out_f[l - 1], st);
    if (!rc) rc = weight_grads(t, 0, t->dz[0], kUvInvMid, t->uv, D, st);
    if (rc) return rc;
    t->have_grads = true;
    return NGF_OK;
}
}  // namespace

extern "C" {

int ngf_uv_inverse_train_backward(ngf_uv_inverse_trainer *t, int64_t ticket, const float *d_xyz, float *d_uv, void *hip_stream)
{
    return backward(t, "ngf_uv_inverse_train_backward", ticket, d_xyz, d_uv, true, (hipStream_t)hip_stream);
}

// profiling aid (include/ngf.h): the dX chain of the backward alone
int ngf_debug_uv_inverse_train_dx(ngf_uv_inverse_trainer *t, int64_t ticket, const float *d_xyz, float *d_uv, void *hip_stream)
{
    return backward(t, "ngf_debug_uv_inverse_train_dx", ticket, d_xyz, d_uv, false, (hipStream_t)hip_stream);
}

int ngf_uv_inverse_train_get_grads(ngf_uv_inverse_trainer *t, float *const out[NGF_UV_INVERSE_TRAIN_PARAMS], void *hip_stream)
{
    if (!t || !out) return fail(NGF_E_ARG, "ngf_uv_inverse_train_get_grads: null argument");
    if (!t->have_grads) return fail(NGF_E_ARG, "ngf_uv_inverse_train_get_grads: no backward since the last forward");
    DeviceScope ds(t->device);
    hipStream_t st = (hipStream_t)hip_stream;
    for (int k = 0; k < NGF_UV_INVERSE_TRAIN_PARAMS; ++k) {
        if (!out[k]) continue;
        const int l = k / 2;
        const int64_t n = (k & 1) ? t->shape.out_f[l] : (int64_t)t->shape.out_f[l] * t->shape.in_f[l];
        HIP_TRY(hipMemcpyAsync(out[k], t->grads + t->grad_off[k], (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return NGF_OK;
}

}  // extern "C"
