// ngf_infoinv_train.hip -- the C ABI of the InfoInv trainer (include/ngf.h: ngf_infoinv_trainer_*, ngf_infoinv_train_*); kernels in
// ngf_infoinv_train.hpp.  A translation unit of its own: ngf_field.hip and the ISA lint's compile of it stay as they were.
#include "ngf_host.hpp"
#include "ngf_infoinv_train.hpp"
#include "ngf_infoinv_fused.hpp"

using namespace ngf;

struct ngf_infoinv_trainer {
    int device = -1;
    ngf_infoinv_train_desc desc{};
    int64_t max_rays = 0;
    int32_t max_samples = 0;
    int64_t cap = 0;                                   // max_rays * max_samples
    DeviceAllocs mem{0, 16};                           // every device buffer of the handle
    float *tex[3] = {nullptr, nullptr, nullptr};       // packed planes
    unsigned long long *gacc[3] = {nullptr, nullptr, nullptr};
    uint8_t *mask = nullptr;
    float *dw1t = nullptr, *cw1t = nullptr;
    IiArgs A{};                                        // buffers of the last forward
    double *part = nullptr;                            // GEMM chunk partials
    int64_t part_elems = 0;
    double *m64 = nullptr;                             // [64][231] colour M in fp64
    float *grads[NGF_INFOINV_TRAIN_PARAMS] = {};       // gradients of the last backward, reference layouts
    int64_t grad_elems[NGF_INFOINV_TRAIN_PARAMS] = {};
    bool packed = false;
    int64_t ticket = 0;                                // last forward's ticket (0 = none)
    bool have_grads = false;
    // the fused step (ngf_infoinv_train_step_backward / _adam_all / _adam_ext / _get_grad)
    float *f_rgb = nullptr, *f_depth = nullptr, *f_drgb = nullptr;     // [max_rays,3], [max_rays], [max_rays,3]
    double *partb = nullptr;                           // bias partials [chunks][64]
    int64_t partb_elems = 0;
    float *exp_avg[NGF_INFOINV_TRAIN_PARAMS] = {}, *exp_avg_sq[NGF_INFOINV_TRAIN_PARAMS] = {};      // the caller's moments (set_moments)
    bool have_moments = false;
    bool have_fused = false;                           // a fused backward's gradients are in the trainer
    bool planes_fixed = false;                         // ... the planes' as fixed point in gacc (one ray chunk); else as floats in grads[0..2]
};

namespace {

// the parameter tensors in `which` order (include/ngf.h) and their element counts
void ii_params(const ngf_infoinv_train_desc &d, const float *p[NGF_INFOINV_TRAIN_PARAMS], int64_t n[NGF_INFOINV_TRAIN_PARAMS])
{
    const float *ps[NGF_INFOINV_TRAIN_PARAMS] = {d.plane[0], d.plane[1], d.plane[2], d.dens_w1, d.dens_b1, d.dens_w2, d.dens_b2, d.dens_w3, d.dens_b3,
                                                 d.basis, d.w1, d.b1, d.w2, d.b2, d.w3, d.b3};
    const int64_t ns[NGF_INFOINV_TRAIN_PARAMS] = {(int64_t)kIiC * d.plane_h[0] * d.plane_w[0], (int64_t)kIiC * d.plane_h[1] * d.plane_w[1],
                                                  (int64_t)kIiC * d.plane_h[2] * d.plane_w[2], kIiDH * kIiDIn, kIiDH, kIiDH * kIiDH, kIiDH, kIiDH, 1,
                                                  kIiCF * kIiCF, kIiCH * kIiCIn, kIiCH, kIiCH * kIiCH, kIiCH, 3 * kIiCH, 3};
    for (int k = 0; k < NGF_INFOINV_TRAIN_PARAMS; ++k) { p[k] = ps[k]; n[k] = ns[k]; }
}

unsigned grid_for(int64_t work, int block = 256, int64_t cap = 1 << 16)
{
    int64_t g = (work + block - 1) / block;
    if (g < 1) g = 1;
    return (unsigned)(g < cap ? g : cap);
}

// Where one weight-gradient product reads its operands' rows and leaves its partials: the trainer fills it from its own buffers (ii_bufs),
// ngf_debug_ii_product from its arguments.  Chunk counts, grid sizes and the reduce launch are computed in ii_xty / ii_mm, once, for both.
struct IiProductBufs {
    int64_t ld;                   // row stride of X and Y
    double *part;                 // chunk partials of the matrix
    int64_t part_elems;
    double *partb;                // ... of the bias column (the MFMA form)
    int64_t partb_elems;
};

// one weight-gradient GEMM (X: M delta rows, Y: N input rows, both [k][ld]) -> gw [M][N], gb [M] (nullable), gw64 (nullable)
int ii_xty(const IiProductBufs &B, const float *X, const float *Y, int64_t rows_cap, const int32_t *rows_dev, int M, int N, float *gw, float *gb,
           double *gw64, hipStream_t st)
{
    IiXty G{};
    G.X = X; G.Y = Y; G.ld = B.ld; G.rows = rows_cap; G.rows_dev = rows_dev; G.M = M; G.N = N; G.NB = N + 1; G.part = B.part;
    const int chunks = (int)((rows_cap + kIiChunk - 1) / kIiChunk);
    const int tiles = ((M + 31) / 32) * ((N + 1 + 31) / 32);
    if ((int64_t)chunks * M * (N + 1) > B.part_elems)
        return fail(NGF_E_ARG, "ngf_infoinv: product scratch too small: part holds %lld doubles, %d chunks of %d x %d need %lld", (long long)B.part_elems,
                    chunks, M, N + 1, (long long)chunks * M * (N + 1));
    NGF_LAUNCH(ii_xty_kernel, dim3(chunks > 0 ? chunks : 1, tiles), dim3(256), 0, st, G);
    NGF_LAUNCH(ii_xty_reduce_kernel, dim3((M * (N + 1) + 255) / 256), dim3(256), 0, st, (const double *)B.part, chunks > 0 ? chunks : 1, M, N, gw, gb,
               gw64);
    return NGF_OK;
}

// the backward up to the per-sample deltas and the fixed-point plane sums (A.d_rgb set)
int ii_backward_deltas(ngf_infoinv_trainer *t, hipStream_t st)
{
    IiArgs &A = t->A;
    const int64_t n = A.n, pairs = n * (int64_t)A.S;
    const unsigned rg = (unsigned)((n + 255) / 256);
    NGF_LAUNCH(ii_composite_bwd_kernel, dim3(rg), dim3(256), 0, st, A);
    NGF_LAUNCH(ii_color_bwd_kernel, dim3(grid_for(pairs)), dim3(256), 0, st, A);
    NGF_LAUNCH(ii_density_bwd_kernel, dim3(grid_for(pairs)), dim3(256), 0, st, A);
    // plane gradients: bound -> scale -> fixed-point scatter
    NGF_LAUNCH(ii_bound_kernel, dim3(kIiBoundBlocks), dim3(256), 0, st, A);
    NGF_LAUNCH(ii_scale_kernel, dim3(1), dim3(64), 0, st, A);
    for (int p = 0; p < 3; ++p)
        HIP_TRY(hipMemsetAsync(t->gacc[p], 0, (size_t)(A.tex[p].H + 2) * (A.tex[p].W + 2) * kIiC * sizeof(unsigned long long), st));
    NGF_LAUNCH(ii_scatter_kernel<true>, dim3(grid_for(pairs * kIiDIn)), dim3(256), 0, st, A);
    NGF_LAUNCH(ii_scatter_kernel<false>, dim3(grid_for(pairs * kIiCF)), dim3(256), 0, st, A);
    return NGF_OK;
}

// one weight-gradient product of the fused step on the matrix pipe (X: M delta rows, Y: N input rows) -> gw [M][N], gb [M], gw64 (nullable)
int ii_mm(const IiProductBufs &B, const float *X, const float *Y, int64_t rows_cap, const int32_t *rows_dev, int M, int N, float *gw, float *gb,
          double *gw64, bool accumulate, hipStream_t st)
{
    IiMm G{};
    G.X = X; G.Y = Y; G.ld = B.ld; G.rows = rows_cap; G.rows_dev = rows_dev; G.M = M; G.N = N; G.part = B.part; G.partb = B.partb;
    const int64_t chunks = (rows_cap + kIiMmChunk - 1) / kIiMmChunk;
    const int tiles = ((M + 63) / 64) * ((N + 63) / 64);
    if (M > kIiCH || chunks > 65535) return fail(NGF_E_ARG, "ngf_infoinv: a product of %d delta rows over %lld chunks is outside the launch", M, (long long)chunks);
    if (chunks * M * N > B.part_elems || chunks * M > B.partb_elems)
        return fail(NGF_E_ARG, "ngf_infoinv: product scratch too small: part / partb hold %lld / %lld doubles, %lld chunks of %d x %d need %lld / %lld",
                    (long long)B.part_elems, (long long)B.partb_elems, (long long)chunks, M, N, (long long)(chunks * M * N), (long long)(chunks * M));
    NGF_LAUNCH(ii_mm_kernel, dim3(tiles, chunks > 0 ? (unsigned)chunks : 1), dim3(256), 0, st, G);
    NGF_LAUNCH(ii_mm_reduce_kernel, dim3((M * N + M + 255) / 256), dim3(256), 0, st, (const double *)B.part, (const double *)B.partb, rows_cap, rows_dev,
               M, N, gw, gb, gw64, accumulate ? 1 : 0);
    return NGF_OK;
}

// grad NULL: the trainer's own gradients of the last fused backward (+ the L1 term on the planes); else the caller's tensors
int ii_adam(ngf_infoinv_trainer *t, const float *const *grad, float *const *m, float *const *v, const int32_t *step_count, const float *lr, float beta1,
            float beta2, float eps, float l1_weight, hipStream_t st)
{
    const ngf_infoinv_train_desc &d = t->desc;
    const float *ps[NGF_INFOINV_TRAIN_PARAMS];
    int64_t ns[NGF_INFOINV_TRAIN_PARAMS];
    ii_params(d, ps, ns);
    auto on = [&](int k) { return step_count[k] > 0 && (!grad || grad[k]); };
    for (int k = 0; k < NGF_INFOINV_TRAIN_PARAMS; ++k)
        if (on(k) && (!m[k] || !v[k])) return fail(NGF_E_ARG, "ngf_infoinv_train_adam: parameter %d has a gradient but no moments", k);
    for (int p = 0; p < 3; ++p) {
        if (!on(p)) continue;
        const int H = d.plane_h[p], W = d.plane_w[p];
        const AdamArgs a = adam_args(step_count[p], lr[p], beta1, beta2, eps, grad ? 0.0f : l1_weight / (float)((int64_t)kIiC * H * W));
        const dim3 g(H * ((W + 63) / 64));
        // a stale packed copy is simply rewritten; its zero border is written whenever the forward packs (t->packed unset)
        if (!grad && t->planes_fixed)
            NGF_LAUNCH(ii_adam_plane_kernel<true>, g, dim3(256), 0, st, d.plane[p], m[p], v[p], H, W, (const unsigned long long *)t->gacc[p],
                       (const double *)t->A.bound, (const float *)nullptr, t->tex[p], a);
        else
            NGF_LAUNCH(ii_adam_plane_kernel<false>, g, dim3(256), 0, st, d.plane[p], m[p], v[p], H, W, (const unsigned long long *)nullptr,
                       (const double *)nullptr, grad ? grad[p] : (const float *)t->grads[p], t->tex[p], a);
    }
    const float *const *g = grad;
    if (!g) g = t->grads;
    HIP_TRY(adam_dense_all<kIiDense>(const_cast<float *const *>(ps) + 3, m + 3, v + 3, g + 3, ns + 3, step_count + 3, lr + 3, beta1, beta2, eps,
                                     [&](int j) { return on(3 + j); }, nullptr, st));
    return NGF_OK;
}

IiProductBufs ii_bufs(const ngf_infoinv_trainer *t) { return IiProductBufs{t->cap, t->part, t->part_elems, t->partb, t->partb_elems}; }

}  // namespace

extern "C" {

int32_t ngf_sizeof_infoinv_train_desc(void) { return (int32_t)sizeof(ngf_infoinv_train_desc); }

int64_t ngf_infoinv_trainer_bytes(const ngf_infoinv_trainer *t) { return t ? t->mem.bytes : 0; }

int ngf_infoinv_trainer_destroy(ngf_infoinv_trainer *t)
{
    if (!t) return NGF_OK;
    {
        DeviceScope ds(t->device);
        t->mem.free_all();
    }
    delete t;
    return NGF_OK;
}

int ngf_infoinv_trainer_create(const ngf_infoinv_train_desc *desc, ngf_infoinv_trainer **out, void *hip_stream)
{
    if (!desc || !out) return fail(NGF_E_ARG, "ngf_infoinv_trainer_create: null argument");
    *out = nullptr;
    const ngf_infoinv_train_desc &d = *desc;
    if (d.max_rays <= 0 || d.max_samples <= 0) return fail(NGF_E_ARG, "ngf_infoinv_trainer_create: max_rays and max_samples must be > 0");
    const float *ps[NGF_INFOINV_TRAIN_PARAMS];
    int64_t ns[NGF_INFOINV_TRAIN_PARAMS];
    ii_params(d, ps, ns);
    for (int k = 0; k < NGF_INFOINV_TRAIN_PARAMS; ++k)
        if (!ps[k]) return fail(NGF_E_ARG, "ngf_infoinv_trainer_create: parameter %d is NULL", k);
    for (int p = 0; p < 3; ++p)
        if (d.plane_h[p] < 2 || d.plane_w[p] < 2 || (int64_t)(d.plane_h[p] + 2) * (d.plane_w[p] + 2) * kIiC >= (1ll << 31))
            return fail(NGF_E_ARG, "ngf_infoinv_trainer_create: plane %d has an unsupported size %d x %d", p, d.plane_h[p], d.plane_w[p]);
    const int64_t cap = d.max_rays * (int64_t)d.max_samples;
    if (cap >= (1ll << 31)) return fail(NGF_E_ARG, "ngf_infoinv_trainer_create: max_rays * max_samples must be < 2^31");
    if (d.mask_bits && (d.mask_d < 1 || d.mask_h < 1 || d.mask_w < 1)) return fail(NGF_E_ARG, "ngf_infoinv_trainer_create: bad mask size");
    hipStream_t st = (hipStream_t)hip_stream;
    ngf_infoinv_trainer *t = new (std::nothrow) ngf_infoinv_trainer();
    if (!t) return fail(NGF_E_HIP, "ngf_infoinv_trainer_create: out of host memory");
    HIP_TRY(hipGetDevice(&t->device));
    t->desc = d;
    t->max_rays = d.max_rays;
    t->max_samples = d.max_samples;
    t->cap = cap;
    IiArgs &A = t->A;
    int rc = 0;
    auto bail = [&](int r) { t->mem.free_all(); delete t; return r; };
    for (int p = 0; p < 3; ++p) {
        const int64_t tex = (int64_t)(d.plane_h[p] + 2) * (d.plane_w[p] + 2);
        if ((rc = t->mem.alloc(&t->tex[p], tex * kIiC)) || (rc = t->mem.alloc(&t->gacc[p], tex * kIiC))) return bail(rc);
        Tex &x = A.tex[p];
        x.p = t->tex[p]; x.W = d.plane_w[p]; x.H = d.plane_h[p]; x.stride = d.plane_w[p] + 2;
        x.fw = (float)(d.plane_w[p] - 1); x.fh = (float)(d.plane_h[p] - 1);
        A.gacc[p] = t->gacc[p];
    }
    if (d.mask_bits) {
        const size_t mb = ((size_t)d.mask_d * d.mask_h * d.mask_w + 7) / 8;
        if ((rc = t->mem.alloc(&t->mask, mb))) return bail(rc);
        if (hipMemcpyAsync(t->mask, d.mask_bits, mb, hipMemcpyDeviceToDevice, st) != hipSuccess) return bail(fail(NGF_E_HIP, "mask copy failed"));
    }
    if ((rc = t->mem.alloc(&t->dw1t, kIiDIn * kIiDH)) || (rc = t->mem.alloc(&t->cw1t, kIiCIn * kIiCH))) return bail(rc);
    const int64_t nr = d.max_rays;
    A.cap = cap;
    if ((rc = t->mem.alloc(&A.et, cap)) || (rc = t->mem.alloc(&A.sg, cap)) || (rc = t->mem.alloc(&A.w, cap)) || (rc = t->mem.alloc(&A.tb, cap)) ||
        (rc = t->mem.alloc(&A.dxs, cap)) || (rc = t->mem.alloc(&A.xn, 3 * cap)) || (rc = t->mem.alloc(&A.valid, cap)) ||
        (rc = t->mem.alloc(&A.d_in, kIiDIn * cap)) || (rc = t->mem.alloc(&A.d_h1, kIiDH * cap)) || (rc = t->mem.alloc(&A.d_h2, kIiDH * cap)) ||
        (rc = t->mem.alloc(&A.d_d1, kIiDH * cap)) || (rc = t->mem.alloc(&A.d_d2, kIiDH * cap)) || (rc = t->mem.alloc(&A.d_g, kIiDIn * cap)) ||
        (rc = t->mem.alloc(&A.count, nr)) || (rc = t->mem.alloc(&A.offset, nr + 1)) || (rc = t->mem.alloc(&A.list, cap)) ||
        (rc = t->mem.alloc(&A.c_in, kIiCIn * cap)) || (rc = t->mem.alloc(&A.c_h1, kIiCH * cap)) || (rc = t->mem.alloc(&A.c_h2, kIiCH * cap)) ||
        (rc = t->mem.alloc(&A.c_rgb, 3 * cap)) || (rc = t->mem.alloc(&A.c_d1, kIiCH * cap)) || (rc = t->mem.alloc(&A.c_d2, kIiCH * cap)) ||
        (rc = t->mem.alloc(&A.c_d3, 3 * cap)) || (rc = t->mem.alloc(&A.c_g, kIiCF * cap)) || (rc = t->mem.alloc(&A.pre, 3 * nr)) ||
        (rc = t->mem.alloc(&A.bound, kIiBoundBlocks + 1)) || (rc = t->mem.alloc(&t->m64, kIiCH * kIiCIn)))
        return bail(rc);
    const int64_t chunks = (cap + kIiChunk - 1) / kIiChunk;
    t->part_elems = chunks * kIiCH * (kIiCIn + 1);
    if ((rc = t->mem.alloc(&t->part, t->part_elems))) return bail(rc);
    t->partb_elems = ((cap + kIiMmChunk - 1) / kIiMmChunk) * kIiCH;
    if ((rc = t->mem.alloc(&t->f_rgb, 3 * nr)) || (rc = t->mem.alloc(&t->f_depth, nr)) || (rc = t->mem.alloc(&t->f_drgb, 3 * nr)) ||
        (rc = t->mem.alloc(&t->partb, t->partb_elems)))
        return bail(rc);
    for (int k = 0; k < NGF_INFOINV_TRAIN_PARAMS; ++k) {
        t->grad_elems[k] = ns[k];
        if ((rc = t->mem.alloc(&t->grads[k], ns[k]))) return bail(rc);
    }
    // the geometry of the desc
    for (int k = 0; k < 3; ++k) {
        A.a0[k] = d.aabb[k]; A.a1[k] = d.aabb[3 + k];
        A.inv[k] = 2.0f / (d.aabb[3 + k] - d.aabb[k]);                 // invaabbSize = 2 / aabbSize (FieldBase.py:66)
        if (d.mask_bits) { A.m_a0[k] = d.mask_aabb[k]; A.m_inv[k] = 1.0f / (d.mask_aabb[3 + k] - d.mask_aabb[k]) * 2.0f; }
    }
    A.near_ = d.near_; A.far_ = d.far_; A.step = d.step; A.dscale = d.distance_scale; A.thr = d.weight_thres;
    A.mask_bits = t->mask; A.mD = d.mask_d; A.mH = d.mask_h; A.mW = d.mask_w;
    A.dw1 = d.dens_w1; A.db1 = d.dens_b1; A.dw2 = d.dens_w2; A.db2 = d.dens_b2; A.dw3 = d.dens_w3; A.db3 = d.dens_b3;
    A.basis = d.basis; A.w1 = d.w1; A.b1 = d.b1; A.w2 = d.w2; A.b2 = d.b2; A.w3 = d.w3; A.b3 = d.b3;
    A.dw1t = t->dw1t; A.cw1t = t->cw1t;
    if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(NGF_E_HIP, "ngf_infoinv_trainer_create: stream synchronisation failed"));
    *out = t;
    return NGF_OK;
}

int ngf_infoinv_train_params_changed(ngf_infoinv_trainer *t)
{
    if (!t) return fail(NGF_E_ARG, "ngf_infoinv_train_params_changed: null trainer");
    t->packed = false;
    return NGF_OK;
}

int ngf_infoinv_train_forward(ngf_infoinv_trainer *t, const float *rays, const float *jitter, int64_t n, int32_t n_samples, int32_t white_bg,
                              int32_t infoinv, float *rgb_map, float *depth_map, int64_t *ticket, void *hip_stream)
{
    if (!t || !rays || !rgb_map || !depth_map || !ticket) return fail(NGF_E_ARG, "ngf_infoinv_train_forward: null argument");
    if (n <= 0 || n > t->max_rays || n_samples <= 0 || n_samples > t->max_samples)
        return fail(NGF_E_ARG, "ngf_infoinv_train_forward: n = %lld, n_samples = %d outside the trainer's 1..%lld x 1..%d", (long long)n, n_samples,
                    (long long)t->max_rays, t->max_samples);
    hipStream_t st = (hipStream_t)hip_stream;
    IiArgs &A = t->A;
    t->ticket = 0;                         // the buffers are overwritten from here on: no earlier ticket stays valid, even if this call fails
    t->have_grads = false;
    t->have_fused = false;
    A.rays = rays; A.jitter = jitter; A.n = n; A.S = n_samples; A.white_bg = white_bg ? 1 : 0; A.infoinv = infoinv ? 1 : 0;
    A.rgb_out = rgb_map; A.depth_out = depth_map; A.d_rgb = nullptr;
    if (!t->packed) {
        for (int p = 0; p < 3; ++p)
            NGF_LAUNCH(ii_pack_kernel, dim3(grid_for((int64_t)(A.tex[p].H + 2) * (A.tex[p].W + 2) * kIiC)), dim3(256), 0, st,
                       (const float *)t->desc.plane[p], A.tex[p].H, A.tex[p].W, t->tex[p]);
        t->packed = true;
    }
    NGF_LAUNCH(ii_prep_kernel, dim3((kIiCIn * kIiCH + 255) / 256), dim3(256), 0, st, A, t->dw1t, t->cw1t);
    const int64_t pairs = n * (int64_t)n_samples;
    NGF_LAUNCH(ii_density_fwd_kernel, dim3(grid_for(pairs)), dim3(256), 0, st, A);
    const unsigned rg = (unsigned)((n + 255) / 256);
    NGF_LAUNCH(ii_scan_kernel, dim3(rg), dim3(256), 0, st, A);
    NGF_LAUNCH(ii_prefix_kernel, dim3(1), dim3(1024), 0, st, (const int32_t *)A.count, n, A.offset);
    NGF_LAUNCH(ii_list_kernel, dim3(rg), dim3(256), 0, st, A);
    NGF_LAUNCH(ii_color_fwd_kernel, dim3(grid_for(pairs)), dim3(256), 0, st, A);       // the active count is read on the device
    NGF_LAUNCH(ii_composite_fwd_kernel, dim3(rg), dim3(256), 0, st, A);
    static int64_t next_ticket = 0;
    t->ticket = __atomic_add_fetch(&next_ticket, 1, __ATOMIC_RELAXED);
    *ticket = t->ticket;
    return NGF_OK;
}

int ngf_infoinv_train_backward_grad(ngf_infoinv_trainer *t, int64_t ticket, const float *d_rgb_map, void *hip_stream)
{
    if (!t || !d_rgb_map) return fail(NGF_E_ARG, "ngf_infoinv_train_backward_grad: null argument");
    if (ticket == 0 || ticket != t->ticket)
        return fail(NGF_E_STALE, "ngf_infoinv_train_backward_grad: ticket %lld is not the trainer's last forward", (long long)ticket);
    hipStream_t st = (hipStream_t)hip_stream;
    IiArgs &A = t->A;
    A.d_rgb = d_rgb_map;
    t->have_fused = false;
    int rc;
    if ((rc = ii_backward_deltas(t, st))) return rc;
    const int64_t n = A.n, pairs = n * (int64_t)A.S;
    for (int p = 0; p < 3; ++p)
        NGF_LAUNCH(ii_plane_grad_kernel, dim3(grid_for((int64_t)kIiC * A.tex[p].H * A.tex[p].W)), dim3(256), 0, st,
                   (const unsigned long long *)t->gacc[p], (const double *)A.bound, A.tex[p].H, A.tex[p].W, t->grads[p]);
    // weight gradients (which: 3..8 density mlp.{0,2,4}.{weight,bias}, 9 basis, 10..15 rgb mlp.{0,2,4}.{weight,bias})
    const int32_t *na = A.offset + n;
    const IiProductBufs B = ii_bufs(t);
    if ((rc = ii_xty(B, A.d_d1, A.d_in, pairs, nullptr, kIiDH, kIiDIn, t->grads[3], t->grads[4], nullptr, st)) ||
        (rc = ii_xty(B, A.d_d2, A.d_h1, pairs, nullptr, kIiDH, kIiDH, t->grads[5], t->grads[6], nullptr, st)) ||
        (rc = ii_xty(B, A.dxs, A.d_h2, pairs, nullptr, 1, kIiDH, t->grads[7], t->grads[8], nullptr, st)) ||
        (rc = ii_xty(B, A.c_d1, A.c_in, pairs, na, kIiCH, kIiCIn, nullptr, t->grads[11], t->m64, st)) ||
        (rc = ii_xty(B, A.c_d2, A.c_h1, pairs, na, kIiCH, kIiCH, t->grads[12], t->grads[13], nullptr, st)) ||
        (rc = ii_xty(B, A.c_d3, A.c_h2, pairs, na, 3, kIiCH, t->grads[14], t->grads[15], nullptr, st)))
        return rc;
    NGF_LAUNCH(ii_unfold_kernel, dim3((kIiCF * kIiCF + 255) / 256), dim3(256), 0, st, (const double *)t->m64, A.basis, A.w1, t->grads[10], t->grads[9]);
    t->have_grads = true;
    return NGF_OK;
}

int ngf_infoinv_train_get_grads(ngf_infoinv_trainer *t, float *const out[NGF_INFOINV_TRAIN_PARAMS], void *hip_stream)
{
    if (!t || !out) return fail(NGF_E_ARG, "ngf_infoinv_train_get_grads: null argument");
    if (!t->have_grads) return fail(NGF_E_ARG, "ngf_infoinv_train_get_grads: no backward since the last forward");
    hipStream_t st = (hipStream_t)hip_stream;
    for (int k = 0; k < NGF_INFOINV_TRAIN_PARAMS; ++k)
        if (out[k]) HIP_TRY(hipMemcpyAsync(out[k], t->grads[k], (size_t)t->grad_elems[k] * sizeof(float), hipMemcpyDeviceToDevice, st));
    return NGF_OK;
}

// ---- the fused step -------------------------------------------------------------------------------------------------------------------------
int ngf_infoinv_train_set_moments(ngf_infoinv_trainer *t, float *const exp_avg[NGF_INFOINV_TRAIN_PARAMS],
                                  float *const exp_avg_sq[NGF_INFOINV_TRAIN_PARAMS])
{
    if (!t || !exp_avg || !exp_avg_sq) return fail(NGF_E_ARG, "ngf_infoinv_train_set_moments: null argument");
    for (int k = 0; k < NGF_INFOINV_TRAIN_PARAMS; ++k)
        if (!exp_avg[k] || !exp_avg_sq[k]) return fail(NGF_E_ARG, "ngf_infoinv_train_set_moments: the moments of parameter %d are NULL", k);
    for (int k = 0; k < NGF_INFOINV_TRAIN_PARAMS; ++k) { t->exp_avg[k] = exp_avg[k]; t->exp_avg_sq[k] = exp_avg_sq[k]; }
    t->have_moments = true;
    return NGF_OK;
}

int ngf_infoinv_train_step_backward(ngf_infoinv_trainer *t, const float *rays, const float *rgb_train, const float *jitter, int64_t n, int32_t n_samples,
                                    int32_t white_bg, int32_t infoinv, double *loss_out, void *hip_stream)
{
    if (!t || !rays || !rgb_train || !loss_out) return fail(NGF_E_ARG, "ngf_infoinv_train_step_backward: null argument");
    if (n <= 0 || n >= (1ll << 31) / 3 || n_samples <= 0 || n_samples > t->max_samples)
        return fail(NGF_E_ARG, "ngf_infoinv_train_step_backward: n = %lld, n_samples = %d outside the trainer's range (n_samples 1..%d)", (long long)n,
                    n_samples, t->max_samples);
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceScope ds(t->device);
    int rc;
    IiArgs &A = t->A;
    const bool one = n <= t->max_rays;              // a batch of more rays than the trainer holds: ray chunks whose gradients add up
    for (int64_t a = 0; a < n; a += t->max_rays) {
        const int64_t nc = n - a < t->max_rays ? n - a : t->max_rays;
        const bool acc = a > 0;
        int64_t ticket = 0;
        if ((rc = ngf_infoinv_train_forward(t, rays + a * 6, jitter ? jitter + a : nullptr, nc, n_samples, white_bg, infoinv, t->f_rgb, t->f_depth, &ticket,
                                            hip_stream)))
            return rc;
        NGF_LAUNCH(ii_loss_kernel, dim3(1), dim3(1024), 0, st, (const float *)t->f_rgb, rgb_train + a * 3, nc * 3, n * 3, t->f_drgb, loss_out, acc ? 1 : 0);
        A.d_rgb = t->f_drgb;
        if ((rc = ii_backward_deltas(t, st))) return rc;
        if (!one)
            for (int p = 0; p < 3; ++p) {
                const unsigned g = grid_for((int64_t)kIiC * A.tex[p].H * A.tex[p].W);
                if (acc)
                    NGF_LAUNCH(ii_plane_grad_add_kernel, dim3(g), dim3(256), 0, st, (const unsigned long long *)t->gacc[p], (const double *)A.bound,
                               A.tex[p].H, A.tex[p].W, t->grads[p]);
                else
                    NGF_LAUNCH(ii_plane_grad_kernel, dim3(g), dim3(256), 0, st, (const unsigned long long *)t->gacc[p], (const double *)A.bound,
                               A.tex[p].H, A.tex[p].W, t->grads[p]);
            }
        const int64_t pairs = nc * (int64_t)n_samples;
        const int32_t *na = A.offset + nc;
        const IiProductBufs B = ii_bufs(t);
        if ((rc = ii_mm(B, A.d_d1, A.d_in, pairs, nullptr, kIiDH, kIiDIn, t->grads[3], t->grads[4], nullptr, acc, st)) ||
            (rc = ii_mm(B, A.d_d2, A.d_h1, pairs, nullptr, kIiDH, kIiDH, t->grads[5], t->grads[6], nullptr, acc, st)) ||
            (rc = ii_mm(B, A.dxs, A.d_h2, pairs, nullptr, 1, kIiDH, t->grads[7], t->grads[8], nullptr, acc, st)) ||
            (rc = ii_mm(B, A.c_d1, A.c_in, pairs, na, kIiCH, kIiCIn, nullptr, t->grads[11], t->m64, acc, st)) ||
            (rc = ii_mm(B, A.c_d2, A.c_h1, pairs, na, kIiCH, kIiCH, t->grads[12], t->grads[13], nullptr, acc, st)) ||
            (rc = ii_mm(B, A.c_d3, A.c_h2, pairs, na, 3, kIiCH, t->grads[14], t->grads[15], nullptr, acc, st)))
            return rc;
    }
    NGF_LAUNCH(ii_unfold_kernel, dim3((kIiCF * kIiCF + 255) / 256), dim3(256), 0, st, (const double *)t->m64, A.basis, A.w1, t->grads[10], t->grads[9]);
    t->ticket = 0;                  // the trainer's own d rgb_map went through: no autograd backward belongs to these forwards
    t->have_grads = false;
    t->have_fused = true;
    t->planes_fixed = one;
    return NGF_OK;
}

int ngf_infoinv_train_get_grad(ngf_infoinv_trainer *t, int32_t which, float *out, void *hip_stream)
{
    if (!t || !out || which < 0 || which >= NGF_INFOINV_TRAIN_PARAMS) return fail(NGF_E_ARG, "ngf_infoinv_train_get_grad: bad argument");
    if (!t->have_fused) return fail(NGF_E_ARG, "ngf_infoinv_train_get_grad: no ngf_infoinv_train_step_backward since the last forward");
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceScope ds(t->device);
    if (which < 3 && t->planes_fixed) {
        const Tex &x = t->A.tex[which];
        NGF_LAUNCH(ii_plane_grad_kernel, dim3(grid_for((int64_t)kIiC * x.H * x.W)), dim3(256), 0, st, (const unsigned long long *)t->gacc[which],
                   (const double *)t->A.bound, x.H, x.W, out);
        return NGF_OK;
    }
    HIP_TRY(hipMemcpyAsync(out, t->grads[which], (size_t)t->grad_elems[which] * sizeof(float), hipMemcpyDeviceToDevice, st));
    return NGF_OK;
}

int ngf_infoinv_train_adam_all(ngf_infoinv_trainer *t, const int32_t step_count[NGF_INFOINV_TRAIN_PARAMS], const float lr[NGF_INFOINV_TRAIN_PARAMS],
                               float beta1, float beta2, float eps, float l1_weight, void *hip_stream)
{
    if (!t || !step_count || !lr) return fail(NGF_E_ARG, "ngf_infoinv_train_adam_all: null argument");
    if (!t->have_moments) return fail(NGF_E_ARG, "ngf_infoinv_train_adam_all: no moments (ngf_infoinv_train_set_moments)");
    if (!t->have_fused) return fail(NGF_E_ARG, "ngf_infoinv_train_adam_all: no ngf_infoinv_train_step_backward since the last forward");
    DeviceScope ds(t->device);
    return ii_adam(t, nullptr, t->exp_avg, t->exp_avg_sq, step_count, lr, beta1, beta2, eps, l1_weight, (hipStream_t)hip_stream);
}

int ngf_infoinv_train_adam_ext(ngf_infoinv_trainer *t, const float *const grad[NGF_INFOINV_TRAIN_PARAMS], float *const exp_avg[NGF_INFOINV_TRAIN_PARAMS],
                               float *const exp_avg_sq[NGF_INFOINV_TRAIN_PARAMS], const int32_t step_count[NGF_INFOINV_TRAIN_PARAMS],
                               const float lr[NGF_INFOINV_TRAIN_PARAMS], float beta1, float beta2, float eps, void *hip_stream)
{
    if (!t || !grad || !exp_avg || !exp_avg_sq || !step_count || !lr) return fail(NGF_E_ARG, "ngf_infoinv_train_adam_ext: null argument");
    DeviceScope ds(t->device);
    return ii_adam(t, grad, exp_avg, exp_avg_sq, step_count, lr, beta1, beta2, eps, 0.0f, (hipStream_t)hip_stream);
}

// test aid (include/ngf.h): the valid and the active count of the rays the trainer's buffers hold
int ngf_debug_ii_counts(ngf_infoinv_trainer *t, int64_t out[2], void *hip_stream)
{
    if (!t || !out) return fail(NGF_E_ARG, "ngf_debug_ii_counts: null argument");
    const IiArgs &A = t->A;
    if (A.n <= 0 || A.S <= 0) return fail(NGF_E_ARG, "ngf_debug_ii_counts: no forward yet");
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceScope ds(t->device);
    const size_t pairs = (size_t)A.n * (size_t)A.S;
    uint8_t *host = (uint8_t *)malloc(pairs);
    if (!host) return fail(NGF_E_HIP, "ngf_debug_ii_counts: out of host memory");
    int32_t active = 0;
    if (hipMemcpyAsync(host, A.valid, pairs, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&active, A.offset + A.n, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        free(host);
        return fail(NGF_E_HIP, "ngf_debug_ii_counts: copy to the host failed");
    }
    int64_t valid = 0;
    for (size_t i = 0; i < pairs; ++i) valid += host[i] ? 1 : 0;
    free(host);
    out[0] = valid;
    out[1] = active;
    return NGF_OK;
}

// test aid (include/ngf.h): one weight-gradient product on caller-owned buffers through the trainer's own launch code
int ngf_debug_ii_product(const ngf_ii_product_args *a, void *hip_stream)
{
    if (!a) return fail(NGF_E_ARG, "ngf_debug_ii_product: null argument");
    if (a->size != (int32_t)sizeof(ngf_ii_product_args)) return fail(NGF_E_ARG, "ngf_debug_ii_product: ngf_ii_product_args layout mismatch");
    if (a->m <= 0 || a->m > kIiCH || a->n <= 0 || a->n > kIiCIn)
        return fail(NGF_E_ARG, "ngf_debug_ii_product: m = %d, n = %d outside 1..%d x 1..%d", a->m, a->n, kIiCH, kIiCIn);
    if (a->rows <= 0 || a->rows >= (1ll << 31) || a->ld < a->rows)
        return fail(NGF_E_ARG, "ngf_debug_ii_product: rows = %lld must be in 1..2^31-1 and ld = %lld at least rows", (long long)a->rows, (long long)a->ld);
    if (!a->x || !a->y || !a->part) return fail(NGF_E_ARG, "ngf_debug_ii_product: x, y and part must not be NULL");
    const IiProductBufs B{a->ld, a->part, a->part_elems, a->partb, a->partb ? a->partb_elems : 0};
    hipStream_t st = (hipStream_t)hip_stream;
    if (a->form == NGF_II_PRODUCT_MFMA) {
        if (!a->partb) return fail(NGF_E_ARG, "ngf_debug_ii_product: the MFMA form needs partb");
        return ii_mm(B, a->x, a->y, a->rows, a->rows_dev, a->m, a->n, a->gw, a->gb, a->gw64, a->accumulate != 0, st);
    }
    if (a->form == NGF_II_PRODUCT_FP64) {
        if (a->accumulate) return fail(NGF_E_ARG, "ngf_debug_ii_product: the fp64 form does not accumulate");
        return ii_xty(B, a->x, a->y, a->rows, a->rows_dev, a->m, a->n, a->gw, a->gb, a->gw64, st);
    }
    return fail(NGF_E_ARG, "ngf_debug_ii_product: unknown form %d", a->form);
}

}  // extern "C"
