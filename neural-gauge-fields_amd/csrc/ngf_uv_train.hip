// ngf_uv_train.hip -- the C ABI of the UV-Mapping (NeuTex) trainer (include/ngf.h: ngf_uv_trainer_*, ngf_uv_train_*); kernels in ngf_uv_train.hpp.
// A translation unit of its own: ngf_uv.hip (the eval kernel, whose assembly tests/test_isa_lint.py lints) stays as it was.
#include "ngf_host.hpp"
#include "ngf_uv_train.hpp"

using namespace ngf;

namespace {

constexpr int L = NGF_UV_LAYERS;
constexpr int kNone = 0, kRelu = 1, kLeaky = 2;

// layer L: inputs, outputs, activation (the order of ngf_uv_desc)
struct LayerShape { int in, out, act; };

void layer_shapes(int sphere, LayerShape s[L])
{
    const int D = sphere ? 3 : 2;
    int i = 0;
    s[i++] = {63, 256, kRelu};
    for (int k = 0; k < 10; ++k) s[i++] = {256, 256, kRelu};
    s[i++] = {256, 1, kNone};
    s[i++] = {63, 64, kRelu};
    s[i++] = {64, 128, kRelu};
    s[i++] = {128, 128, kRelu};
    s[i++] = {128, 128, kRelu};
    s[i++] = {128, D, kNone};
    s[i++] = {D + 20 * D, 256, kLeaky};
    for (int k = 0; k < 5; ++k) s[i++] = {256, 256, kLeaky};
    s[i++] = {256, 3, kNone};
    s[i++] = {295, 256, kLeaky};
    for (int k = 0; k < 3; ++k) s[i++] = {256, 256, kLeaky};
    s[i++] = {256, 3, kNone};
}

}  // namespace

struct ngf_uv_trainer {
    int device = -1;
    ngf_uv_train_desc desc{};
    LayerShape shape[L];
    int64_t cap = 0;                         // max_rays * max_samples
    DeviceAllocs mem{0, 16};                 // every device buffer of the handle
    // per-sample buffers of the last forward (row counts: cap)
    float *seg = nullptr, *opac = nullptr, *acct = nullptr, *xraw = nullptr, *uv = nullptr;
    int32_t *cnt = nullptr, *off = nullptr, *total = nullptr, *list = nullptr, *vid = nullptr;
    float *in[L] = {};                       // layer inputs (post-activation outputs of the layer before, or encodings)
    int64_t in_ld[L] = {};
    float *out[L] = {};                      // layer outputs
    int64_t out_ld[L] = {};
    float *Xga = nullptr, *Xg = nullptr, *Xt = nullptr, *X2 = nullptr;
    // backward
    float *dP = nullptr, *dR = nullptr, *dH = nullptr, *dXt = nullptr, *dRaw = nullptr, *dC1 = nullptr, *dC2 = nullptr, *dQ = nullptr;
    float *part = nullptr, *partb = nullptr;
    float *grads = nullptr;
    int64_t grad_off[2 * L] = {};
    int64_t grad_elems = 0;
    // the last forward
    const float *raydir = nullptr, *bg = nullptr;
    float *ray_pos = nullptr;
    int64_t nrays = 0, R = 0;
    int32_t S = 0;
    int64_t ticket = 0, next_ticket = 0;
    bool have_grads = false;
    // the occupancy mask (ngf_uv_trainer_set_occupancy): an owned copy of the bits, outside `mem` (it is replaced while the handle lives)
    uint8_t *occ = nullptr;
    int32_t occ_n[3] = {0, 0, 0};
    int32_t *cnt_in = nullptr, *off_in = nullptr, *total_in = nullptr;      // in-cube samples per ray, their scan and sum (written with a mask only)
    bool fwd_occ = false;                    // the last forward ran with a mask: total_in holds its in-cube count (else `total` is both counts)
};

namespace {

int launch_gemm(const UvtGemm &G, unsigned gx, unsigned gy, unsigned gz, hipStream_t st)
{
    NGF_LAUNCH(uvt_gemm_kernel, dim3(gx, gy, gz), dim3(256), 0, st, G);
    return NGF_OK;
}

// One Linear as the launch code sees it: caller-owned pointers and leading dimensions.  fwd_layer / bwd_layer fill it from the trainer's buffers,
// ngf_debug_uvt_gemm from its arguments: strides, grid sizes and the chunk count are computed here, once, for both.
struct LayerView {
    int in = 0, out = 0, act = kNone;        // W is [out, in]; the layer's own activation
    const float *w = nullptr, *b = nullptr;
    const float *x = nullptr;                // the layer's input [rows, in] (post-activation output of the producer, or an encoding)
    int64_t ld_x = 0;
    float *z = nullptr;                      // forward: the output [rows, out]
    const float *dz = nullptr;               // backward: the pre-activation gradient [rows, out]
    int64_t ld_z = 0;
    int64_t rows = 0;                        // static row count (sizes the launch)
    const int32_t *rows_dev = nullptr;       // rows on the device (the in-cube count): min(rows, *rows_dev) are computed
    float *dx = nullptr;                     // d input, first n_dx columns
    int64_t ld_dx = 0;
    int n_dx = 0;
    const float *add = nullptr;              // + a second gradient before the mask
    int64_t ld_add = 0;
    int act_prev = kNone;                    // x act'(x) of the producing layer (kNone: no mask)
    float *part = nullptr, *partb = nullptr; // split-K partials [nz][out, in] and [nz][out]
    float *gw = nullptr, *gb = nullptr;      // the reduced gradients
};

int view_nz(const LayerView &v) { return (int)((v.rows + kUvtChunk - 1) / kUvtChunk); }

// Z = act(X W^T + b)
int fwd_view(const LayerView &v, hipStream_t st)
{
    UvtGemm G{};
    G.A = v.x; G.sam = v.ld_x; G.sak = 1;
    G.B = v.w; G.sbk = 1; G.sbn = v.in;
    G.C = v.z; G.ldc = v.ld_z;
    G.bias = v.b; G.act = v.act;
    G.Mdev = v.rows_dev;
    G.M = (int32_t)v.rows; G.N = v.out; G.K = v.in;
    return launch_gemm(G, blocks(v.rows, 64), blocks(v.out, 64), 1, st);
}

// dW, db = dZ^T X over 1024-row chunks -> part / partb, summed in chunk order -> gw, gb
int bwd_weights_view(const LayerView &v, hipStream_t st)
{
    const int nz = view_nz(v);
    UvtGemm G{};
    G.A = v.dz; G.sam = 1; G.sak = v.ld_z;
    G.B = v.x; G.sbk = v.ld_x; G.sbn = 1;
    G.C = v.part; G.ldc = v.in; G.czs = (int64_t)v.out * v.in;
    G.Mdev = v.rows_dev;
    G.M = v.out; G.N = v.in; G.K = (int32_t)v.rows;
    G.split = 1; G.chunk = kUvtChunk; G.partb = v.partb;
    int rc = launch_gemm(G, blocks(v.out, 64), blocks(v.in, 64), (unsigned)std::max(1, nz), st);
    if (rc) return rc;
    const int64_t nk = (int64_t)v.out * v.in;
    NGF_LAUNCH(uvt_reduce_kernel, dim3(blocks(nk)), dim3(256), 0, st, (const float *)v.part, (const float *)v.partb, nk, v.out, (int)v.rows, v.rows_dev,
               v.gw, v.gb);
    return NGF_OK;
}

// dX (first n_dx input columns) = (dZ W + add) x act_prev'(x)
int bwd_input_view(const LayerView &v, hipStream_t st)
{
    UvtGemm G{};
    G.A = v.dz; G.sam = v.ld_z; G.sak = 1;
    G.B = v.w; G.sbk = v.in; G.sbn = 1;
    G.C = v.dx; G.ldc = v.ld_dx;
    G.add = v.add; G.ldadd = v.ld_add;
    if (v.act_prev != kNone) { G.aux = v.x; G.ldaux = v.ld_x; G.act = v.act_prev; }
    G.Mdev = v.rows_dev;
    G.M = (int32_t)v.rows; G.N = v.n_dx; G.K = v.out;
    return launch_gemm(G, blocks(v.rows, 64), blocks(v.n_dx, 64), 1, st);
}

LayerView layer_view(const ngf_uv_trainer *t, int l, int64_t rows, const int32_t *rows_dev)
{
    const LayerShape &s = t->shape[l];
    LayerView v;
    v.in = s.in; v.out = s.out; v.act = s.act;
    v.w = t->desc.w[l]; v.b = t->desc.b[l];
    v.x = t->in[l]; v.ld_x = t->in_ld[l];
    v.rows = rows; v.rows_dev = rows_dev;
    return v;
}

// forward of layer l over `rows` rows (the in-cube count on the device when rows_dev is set)
int fwd_layer(ngf_uv_trainer *t, int l, int64_t rows, const int32_t *rows_dev, hipStream_t st)
{
    LayerView v = layer_view(t, l, rows, rows_dev);
    v.z = t->out[l]; v.ld_z = t->out_ld[l];
    return fwd_view(v, st);
}

// backward of layer l from dZ (its pre-activation gradient, [rows, out] at ld): dW, db -> the gradient slots; dX (first n_dx input columns) ->
// dx (ld_dx), + add (ld_add), x act'(in) of the producing layer (act_prev; kNone: no mask)
int bwd_layer(ngf_uv_trainer *t, int l, const float *dz, int64_t ldz, int64_t rows, const int32_t *rows_dev, float *dx, int64_t ld_dx, int n_dx,
              const float *add, int64_t ld_add, int act_prev, hipStream_t st)
{
    LayerView v = layer_view(t, l, rows, rows_dev);
    v.dz = dz; v.ld_z = ldz;
    v.part = t->part; v.partb = t->partb;
    v.gw = t->grads + t->grad_off[2 * l]; v.gb = t->grads + t->grad_off[2 * l + 1];
    int rc = bwd_weights_view(v, st);
    if (rc || !dx) return rc;
    v.dx = dx; v.ld_dx = ld_dx; v.n_dx = n_dx;
    v.add = add; v.ld_add = ld_add; v.act_prev = act_prev;
    return bwd_input_view(v, st);
}

}  // namespace

extern "C" {

int32_t ngf_sizeof_uv_train_desc(void) { return (int32_t)sizeof(ngf_uv_train_desc); }

int64_t ngf_uv_trainer_bytes(const ngf_uv_trainer *t) { return t ? t->mem.bytes : 0; }

int ngf_uv_trainer_destroy(ngf_uv_trainer *t)
{
    if (!t) return NGF_OK;
    {
        DeviceScope ds(t->device);
        t->mem.free_all();
        if (t->occ) (void)hipFree(t->occ);
    }
    delete t;
    return NGF_OK;
}

int ngf_uv_trainer_create(const ngf_uv_train_desc *desc, ngf_uv_trainer **out, void *hip_stream)
{
    (void)hip_stream;
    if (!desc || !out) return fail(NGF_E_ARG, "ngf_uv_trainer_create: null argument");
    *out = nullptr;
    const ngf_uv_train_desc &d = *desc;
    if (d.max_rays <= 0 || d.max_samples <= 0) return fail(NGF_E_ARG, "ngf_uv_trainer_create: max_rays and max_samples must be > 0");
    if (d.max_rays * (int64_t)d.max_samples >= ((int64_t)1 << 31) / 296)
        return fail(NGF_E_ARG, "ngf_uv_trainer_create: max_rays * max_samples too large (the buffers are indexed with 32-bit rows)");
    if (d.flags != 0) return fail(NGF_E_UNSUPPORTED, "ngf_uv_trainer_create: training is fp32 only (flags must be 0)");
    for (int l = 0; l < L; ++l)
        if (!d.w[l] || !d.b[l]) return fail(NGF_E_ARG, "ngf_uv_trainer_create: layer %d has no weight or bias", l);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    ngf_uv_trainer *t = new (std::nothrow) ngf_uv_trainer();
    if (!t) return fail(NGF_E_ARG, "ngf_uv_trainer_create: out of host memory");
    t->device = dev;
    t->desc = d;
    layer_shapes(d.sphere, t->shape);
    const int64_t cap = d.max_rays * (int64_t)d.max_samples;
    t->cap = cap;
    int rc = NGF_OK;
    auto F = [&](float **p, int64_t n) { if (!rc) rc = t->mem.alloc(p, (size_t)n); };
    auto I = [&](int32_t **p, int64_t n) { if (!rc) rc = t->mem.alloc(p, (size_t)n); };
    F(&t->seg, cap); F(&t->opac, cap); F(&t->acct, cap); F(&t->xraw, d.max_rays * 4); F(&t->uv, cap * 3);
    I(&t->cnt, d.max_rays); I(&t->off, d.max_rays); I(&t->total, 1); I(&t->list, cap); I(&t->vid, cap);
    I(&t->cnt_in, d.max_rays); I(&t->off_in, d.max_rays); I(&t->total_in, 1);
    F(&t->Xga, cap * 64); F(&t->Xg, cap * 64); F(&t->Xt, cap * 64); F(&t->X2, cap * 296);
    for (int l = 0; l < L; ++l) {
        const int o = t->shape[l].out;
        if (l == 22) { t->out[l] = t->X2; t->out_ld[l] = 296; continue; }        // block1's output is block2.0's input, columns 0..255
        const int64_t ld = o == 256 ? 256 : (o == 128 ? 128 : (o == 64 ? 64 : (o == 1 ? 1 : 4)));
        t->out_ld[l] = ld;
        F(&t->out[l], cap * ld);
    }
    if (rc) { t->mem.free_all(); delete t; return rc; }
    for (int l = 0; l < L; ++l) {
        if (l == 0) { t->in[l] = t->Xg; t->in_ld[l] = 64; }
        else if (l == 12) { t->in[l] = t->Xga; t->in_ld[l] = 64; }
        else if (l == 17) { t->in[l] = t->Xt; t->in_ld[l] = 64; }
        else if (l == 23 || l == 24) { t->in[l] = t->X2; t->in_ld[l] = 296; }
        else { t->in[l] = t->out[l - 1]; t->in_ld[l] = t->out_ld[l - 1]; }
    }
    F(&t->dP, cap * 256); F(&t->dR, cap * 256); F(&t->dH, cap * 256); F(&t->dXt, cap * 64);
    F(&t->dRaw, cap); F(&t->dC1, cap * 4); F(&t->dC2, cap * 4); F(&t->dQ, cap * 4);
    const int64_t nz = (cap + kUvtChunk - 1) / kUvtChunk;
    F(&t->part, nz * 256 * 295); F(&t->partb, nz * 256);
    int64_t g = 0;
    for (int l = 0; l < L; ++l) {
        t->grad_off[2 * l] = g; g += (int64_t)t->shape[l].out * t->shape[l].in;
        t->grad_off[2 * l + 1] = g; g += t->shape[l].out;
    }
    t->grad_elems = g;
    F(&t->grads, g);
    if (rc) { t->mem.free_all(); delete t; return rc; }
    *out = t;
    return NGF_OK;
}

int ngf_uv_train_params_changed(ngf_uv_trainer *t)
{
    if (!t) return fail(NGF_E_ARG, "ngf_uv_train_params_changed: null handle");
    return NGF_OK;          // the weights are read in place at every launch: nothing is packed
}

// the contract of ngf_uv_set_occupancy (ngf_uv.hip) on the trainer's own copy.  The forwards after this call read the new bits; the backward of a
// forward before it reads that forward's list and vid, never the mask.
int ngf_uv_trainer_set_occupancy(ngf_uv_trainer *t, const uint8_t *bits_dev, int32_t nx, int32_t ny, int32_t nz, void *hip_stream)
{
    if (!t) return fail(NGF_E_ARG, "ngf_uv_trainer_set_occupancy: null handle");
    if (bits_dev && (nx < 1 || ny < 1 || nz < 1 || nx > kUvOccMaxAxis || ny > kUvOccMaxAxis || nz > kUvOccMaxAxis))
        return fail(NGF_E_ARG, "ngf_uv_trainer_set_occupancy: a grid of %d x %d x %d cells (every axis needs 1 .. %d)", nx, ny, nz, kUvOccMaxAxis);
    DeviceScope ds(t->device);
    uint8_t *fresh = nullptr;
    if (bits_dev) {
        const size_t nbytes = ((size_t)nx * ny * nz + 7) / 8;
        HIP_TRY(hipMalloc((void **)&fresh, nbytes));
        if (hipMemcpyAsync(fresh, bits_dev, nbytes, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream) != hipSuccess) {
            (void)hipFree(fresh);
            return fail(NGF_E_HIP, "ngf_uv_trainer_set_occupancy: copying the bits failed");
        }
    }
    if (t->occ) (void)hipFree(t->occ);          // (waits for the device's work: no launch still reads the old bits)
    t->occ = fresh;
    t->occ_n[0] = fresh ? nx : 0; t->occ_n[1] = fresh ? ny : 0; t->occ_n[2] = fresh ? nz : 0;
    return NGF_OK;
}

int ngf_uv_train_counts(ngf_uv_trainer *t, int64_t out[2], void *hip_stream)
{
    if (!t || !out) return fail(NGF_E_ARG, "ngf_uv_train_counts: null argument");
    if (t->ticket <= 0) return fail(NGF_E_ARG, "ngf_uv_train_counts: the trainer has run no forward");
    DeviceScope ds(t->device);
    hipStream_t st = (hipStream_t)hip_stream;
    int32_t kept = 0, in_cube = 0;
    HIP_TRY(hipMemcpyAsync(&kept, t->total, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (t->fwd_occ) HIP_TRY(hipMemcpyAsync(&in_cube, t->total_in, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out[0] = t->fwd_occ ? in_cube : kept;
    out[1] = kept;
    return NGF_OK;
}

int ngf_uv_train_kept(ngf_uv_trainer *t, uint8_t *out_dev, void *hip_stream)
{
    if (!t || !out_dev) return fail(NGF_E_ARG, "ngf_uv_train_kept: null argument");
    if (t->ticket <= 0) return fail(NGF_E_ARG, "ngf_uv_train_kept: the trainer has run no forward");
    DeviceScope ds(t->device);
    const int64_t M = t->nrays * t->S;
    NGF_LAUNCH(uvt_kept_kernel, dim3(blocks(M)), dim3(256), 0, (hipStream_t)hip_stream, (const int32_t *)t->vid, M, out_dev);
    return NGF_OK;
}

int ngf_uv_train_forward(ngf_uv_trainer *t, const float *campos, const float *raydir, const float *bg, const float *jitter_u, int32_t n_cams,
                         int64_t rays_per_cam, int32_t n_samples, float *color, float *trans, float *uv, float *weight, float *ray_pos, int64_t *ticket,
                         void *hip_stream)
{
    if (!t || !campos || !raydir || !jitter_u || !color || !trans || !uv || !weight || !ray_pos || !ticket)
        return fail(NGF_E_ARG, "ngf_uv_train_forward: null argument");
    if (n_cams <= 0 || rays_per_cam <= 0 || n_samples <= 0) return fail(NGF_E_ARG, "ngf_uv_train_forward: empty batch");
    const int64_t nrays = (int64_t)n_cams * rays_per_cam;
    if (nrays > t->desc.max_rays || n_samples > t->desc.max_samples)
        return fail(NGF_E_ARG, "ngf_uv_train_forward: %lld rays x %d samples exceed the trainer's %lld x %d", (long long)nrays, n_samples,
                    (long long)t->desc.max_rays, t->desc.max_samples);
    DeviceScope ds(t->device);
    hipStream_t st = (hipStream_t)hip_stream;
    const int S = n_samples;
    const int64_t M = nrays * S;
    const int D = t->desc.sphere ? 3 : 2;
    t->have_grads = false;
    // which samples are valid: in-cube, and with a mask in an occupied cell.  Without a mask the launches are the kernels without the look-up.
    UvtOcc O{};
    const bool occ = t->occ != nullptr;
    if (occ) {
        O.bits = t->occ; O.cnt_in = t->cnt_in;
        for (int k = 0; k < 3; ++k) { O.n[k] = t->occ_n[k]; O.h[k] = (float)t->occ_n[k] * 0.5f; }
    }
    {
        UvtRays A{};
        A.cam = campos; A.raydir = raydir; A.U = jitter_u; A.ray_pos = ray_pos; A.seg = t->seg; A.cnt = t->cnt;
        A.nrays = nrays; A.R = (int32_t)rays_per_cam; A.S = S;
        if (occ) NGF_LAUNCH((uvt_rays_kernel<true>), dim3(blocks(nrays)), dim3(256), 0, st, A, O);
        else NGF_LAUNCH((uvt_rays_kernel<false>), dim3(blocks(nrays)), dim3(256), 0, st, A, O);
    }
    NGF_LAUNCH(uvt_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t *)t->cnt, nrays, t->off, t->total);
    if (occ) {
        NGF_LAUNCH(uvt_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t *)t->cnt_in, nrays, t->off_in, t->total_in);
        NGF_LAUNCH((uvt_compact_kernel<true>), dim3(blocks(nrays)), dim3(256), 0, st, (const float *)ray_pos, (const int32_t *)t->off, nrays, S, t->list,
                   t->vid, O);
    } else {
        NGF_LAUNCH((uvt_compact_kernel<false>), dim3(blocks(nrays)), dim3(256), 0, st, (const float *)ray_pos, (const int32_t *)t->off, nrays, S, t->list,
                   t->vid, O);
    }
    t->fwd_occ = occ;
    NGF_LAUNCH(uvt_pe_pos_kernel, dim3(blocks(M)), dim3(256), 0, st, (const float *)ray_pos, M, t->Xga);
    int rc = NGF_OK;
    // gauge network on every sample -> uv
    for (int l = 12; l <= 16 && !rc; ++l) rc = fwd_layer(t, l, M, nullptr, st);
    if (rc) return rc;
    NGF_LAUNCH(uvt_uv_kernel, dim3(blocks(M)), dim3(256), 0, st, (const float *)t->out[16], M, t->desc.sphere, t->uv);
    HIP_TRY(hipMemcpyAsync(uv, t->uv, (size_t)M * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    // geometry network on the in-cube samples
    NGF_LAUNCH(uvt_gather_kernel, dim3(blocks(M * 64)), dim3(256), 0, st, (const float *)t->Xga, (const int32_t *)t->list, (const int32_t *)t->total, M,
               t->Xg);
    for (int l = 0; l <= 11 && !rc; ++l) rc = fwd_layer(t, l, M, t->total, st);
    if (rc) return rc;
    // texture network on the in-cube samples
    NGF_LAUNCH(uvt_tex_in_kernel, dim3(blocks(M)), dim3(256), 0, st, (const float *)t->uv, raydir, (const int32_t *)t->list, (const int32_t *)t->total,
               M, D, S, t->Xt, t->X2);
    for (int l = 17; l <= 28 && !rc; ++l) rc = fwd_layer(t, l, M, t->total, st);
    if (rc) return rc;
    {
        UvtComp A{};
        A.seg = t->seg; A.vid = t->vid; A.raw = t->out[11]; A.c1 = t->out[23]; A.c2 = t->out[28]; A.bg = bg;
        A.color = color; A.trans = trans; A.weight = weight; A.opac = t->opac; A.acct = t->acct; A.xraw = t->xraw;
        A.nrays = nrays; A.R = (int32_t)rays_per_cam; A.S = S;
        NGF_LAUNCH(uvt_composite_kernel, dim3(blocks(nrays)), dim3(256), 0, st, A);
    }
    t->raydir = raydir; t->bg = bg; t->ray_pos = ray_pos;
    t->nrays = nrays; t->R = rays_per_cam; t->S = S;
    t->ticket = ++t->next_ticket;
    *ticket = t->ticket;
    return NGF_OK;
}

int ngf_uv_train_backward(ngf_uv_trainer *t, int64_t ticket, const float *d_color, const float *d_trans, const float *d_uv, const float *d_weight,
                          void *hip_stream)
{
    if (!t || !d_color || !d_trans) return fail(NGF_E_ARG, "ngf_uv_train_backward: null argument");
    if (ticket <= 0 || ticket != t->ticket) return fail(NGF_E_STALE, "ngf_uv_train_backward: ticket %lld is not the trainer's last forward (%lld)",
                                                        (long long)ticket, (long long)t->ticket);
    DeviceScope ds(t->device);
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t nrays = t->nrays, M = nrays * t->S;
    {
        UvtComp A{};
        A.seg = t->seg; A.vid = t->vid; A.raw = t->out[11]; A.c1 = t->out[23]; A.c2 = t->out[28]; A.bg = t->bg;
        A.opac = t->opac; A.acct = t->acct; A.xraw = t->xraw;
        A.d_color = d_color; A.d_trans = d_trans; A.d_weight = d_weight;
        A.d_raw = t->dRaw; A.d_c1 = t->dC1; A.d_c2 = t->dC2;
        A.nrays = nrays; A.R = (int32_t)t->R; A.S = t->S;
        NGF_LAUNCH(uvt_composite_bwd_kernel, dim3(blocks(nrays)), dim3(256), 0, st, A);
    }
    const int32_t *V = t->total;
    int rc = NGF_OK;
    float *pp[2] = {t->dP, t->dR};
    // block2: 28 (dC2) -> 27 -> 26 -> 25 -> 24, whose input gradient (columns 0..255, the block1 output) goes to dH
    rc = bwd_layer(t, 28, t->dC2, 4, M, V, pp[0], 256, 256, nullptr, 0, kLeaky, st);
    int cur = 0;
    for (int l = 27; l >= 25 && !rc; --l, cur ^= 1) rc = bwd_layer(t, l, pp[cur], 256, M, V, pp[cur ^ 1], 256, 256, nullptr, 0, kLeaky, st);
    if (!rc) rc = bwd_layer(t, 24, pp[cur], 256, M, V, t->dH, 256, 256, nullptr, 0, kNone, st);
    // color1: its input gradient + block2.0's, x LeakyReLU'(block1 output)
    if (!rc) rc = bwd_layer(t, 23, t->dC1, 4, M, V, pp[0], 256, 256, t->dH, 256, kLeaky, st);
    cur = 0;
    for (int l = 22; l >= 18 && !rc; --l, cur ^= 1) rc = bwd_layer(t, l, pp[cur], 256, M, V, pp[cur ^ 1], 256, 256, nullptr, 0, kLeaky, st);
    if (!rc) rc = bwd_layer(t, 17, pp[cur], 256, M, V, t->dXt, 64, t->shape[17].in, nullptr, 0, kNone, st);
    if (rc) return rc;
    // d uv -> d q (every sample), gauge network
    NGF_LAUNCH(uvt_uv_bwd_kernel, dim3(blocks(M)), dim3(256), 0, st, (const float *)t->out[16], (const float *)t->uv, (const float *)t->dXt,
               (const int32_t *)t->vid, d_uv, M, t->desc.sphere, t->dQ);
    rc = bwd_layer(t, 16, t->dQ, 4, M, nullptr, pp[0], 128, 128, nullptr, 0, kRelu, st);
    cur = 0;
    for (int l = 15; l >= 13 && !rc; --l, cur ^= 1)
        rc = bwd_layer(t, l, pp[cur], t->out_ld[l], M, nullptr, pp[cur ^ 1], t->in_ld[l], t->shape[l].in, nullptr, 0, kRelu, st);
    if (!rc) rc = bwd_layer(t, 12, pp[cur], 64, M, nullptr, nullptr, 0, 0, nullptr, 0, kNone, st);
    // geometry: 11 (d raw density) -> ... -> 0
    if (!rc) rc = bwd_layer(t, 11, t->dRaw, 1, M, V, pp[0], 256, 256, nullptr, 0, kRelu, st);
    cur = 0;
    for (int l = 10; l >= 1 && !rc; --l, cur ^= 1) rc = bwd_layer(t, l, pp[cur], 256, M, V, pp[cur ^ 1], 256, 256, nullptr, 0, kRelu, st);
    if (!rc) rc = bwd_layer(t, 0, pp[cur], 256, M, V, nullptr, 0, 0, nullptr, 0, kNone, st);
    if (rc) return rc;
    t->have_grads = true;
    return NGF_OK;
}

int ngf_uv_train_get_grads(ngf_uv_trainer *t, float *const out[NGF_UV_TRAIN_PARAMS], void *hip_stream)
{
    if (!t || !out) return fail(NGF_E_ARG, "ngf_uv_train_get_grads: null argument");
    if (!t->have_grads) return fail(NGF_E_ARG, "ngf_uv_train_get_grads: no backward since the last forward");
    DeviceScope ds(t->device);
    hipStream_t st = (hipStream_t)hip_stream;
    for (int k = 0; k < NGF_UV_TRAIN_PARAMS; ++k) {
        if (!out[k]) continue;
        const int l = k / 2;
        const int64_t n = (k & 1) ? t->shape[l].out : (int64_t)t->shape[l].out * t->shape[l].in;
        HIP_TRY(hipMemcpyAsync(out[k], t->grads + t->grad_off[k], (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return NGF_OK;
}

// test aid (include/ngf.h): one layer-sized call on caller-owned buffers through the trainer's own launch code
int ngf_debug_uvt_gemm(const ngf_uvt_gemm_args *a, void *hip_stream)
{
    if (!a) return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: null argument");
    if (a->size != (int32_t)sizeof(ngf_uvt_gemm_args)) return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: ngf_uvt_gemm_args layout mismatch");
    if (a->in <= 0 || a->out <= 0 || a->rows <= 0 || a->rows >= ((int64_t)1 << 31) / 296)
        return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: in, out and rows must be > 0 (rows x 296 below 2^31)");
    if (a->act < kNone || a->act > kLeaky) return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: unknown activation %d", a->act);
    if (!a->z || a->ld_z < a->out) return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: z is null or ld_z < out");
    LayerView v;
    v.in = a->in; v.out = a->out;
    v.w = a->w; v.b = a->b;
    v.x = a->x; v.ld_x = a->ld_x;
    v.rows = a->rows; v.rows_dev = a->rows_dev;
    hipStream_t st = (hipStream_t)hip_stream;
    if (a->form == NGF_UVT_GEMM_FORWARD) {
        if (!a->x || !a->w || !a->b || a->ld_x < a->in) return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: forward needs x (ld_x >= in), w and b");
        v.act = a->act;
        v.z = a->z; v.ld_z = a->ld_z;
        return fwd_view(v, st);
    }
    v.dz = a->z; v.ld_z = a->ld_z;
    if (a->form == NGF_UVT_GEMM_DX) {
        if (!a->w || !a->dx || a->n_dx <= 0 || a->n_dx > a->in || a->ld_dx < a->n_dx)
            return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: dX needs w, dx and 0 < n_dx <= in, ld_dx");
        if (a->add && a->ld_add < a->n_dx) return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: ld_add < n_dx");
        if (a->act != kNone && (!a->x || a->ld_x < a->n_dx)) return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: the mask needs x (ld_x >= n_dx)");
        v.dx = a->dx; v.ld_dx = a->ld_dx; v.n_dx = a->n_dx;
        v.add = a->add; v.ld_add = a->ld_add; v.act_prev = a->act;
        return bwd_input_view(v, st);
    }
    if (a->form == NGF_UVT_GEMM_DW) {
        if (!a->x || a->ld_x < a->in || !a->part || !a->partb || !a->gw || !a->gb)
            return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: dW needs x (ld_x >= in), part, partb, gw and gb");
        const int64_t nz = view_nz(v);
        if (a->part_elems < nz * a->out * a->in || a->partb_elems < nz * a->out)
            return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: part / partb hold fewer than %lld chunks", (long long)nz);
        v.part = a->part; v.partb = a->partb;
        v.gw = a->gw; v.gb = a->gb;
        return bwd_weights_view(v, st);
    }
    return fail(NGF_E_ARG, "ngf_debug_uvt_gemm: unknown form %d", a->form);
}

}  // extern "C"
