// ngf_train.hip -- the C ABI of the TriPlane trainer (include/ngf.h: ngf_trainer_*, ngf_train_*); kernels in ngf_train.hpp, Adam in
// ngf_adam.hpp.  A translation unit of its own like the other trainers: of ngf_field.hip it needs the services of ngf_host.hpp only.
#include <initializer_list>

#include "ngf_host.hpp"
#include "ngf_pack.hpp"
#include "ngf_train.hpp"

using namespace ngf;

// ================================ training step ============================================================
enum { TP_PLANE = 0, TP_GAUGE = 3, TP_DENS_W = 6, TP_DENS_B = 7, TP_BASIS = 8, TP_W1 = 9, TP_B1 = 10, TP_W2 = 11, TP_B2 = 12, TP_W3 = 13,
       TP_B3 = 14, TP_COUNT = 15 };

struct ngf_trainer {
    int dev = 0;                             // the device the trainer's buffers and streams live on
    ngf_train_desc d;
    TrainArgs proto;
    DeviceAllocs mem{64, 0};                 // every device buffer of the handle (64 bytes of slack each, not counted)
    float *tex_d[3] = {}, *tex_a[3] = {}, *tex_g[3] = {};
    float *g_d[3] = {}, *g_a[3] = {}, *g_g[3] = {};
    float *g_gb[3] = {};                     // gauge-plane gradients in the blocked layout the scatter writes (g_g: [texel][2])
    float *q_d[3] = {}, *d_d[3] = {};        // wd-projected density planes, scalar density-gradient images
    float *bwd_image = nullptr, *fwd16_image = nullptr;    // LDS images of the colour MLP (train_fold_kernel): the backward's; the forward's, in the eval pass's layout
    float *dense_p[TP_COUNT] = {};          // the MLP parameters (index TP_*; planes and gauge planes NULL), ...
    float *g_dense[TP_COUNT] = {};          // ... their reference-layout gradient buffers ...
    int64_t dense_n[TP_COUNT] = {};         // ... and element counts
    uint8_t *mask = nullptr;
    uint8_t *mask_cells = nullptr;
    bool tex_fresh[6] = {};                 // the packed copy of plane / gauge plane k holds the parameter's current values
    char *zero_arena = nullptr;             // every buffer a step accumulates into (gradients, M, loss): one memset per step
    size_t zero_bytes = 0;
    int64_t chunk = 0;
    bool speculative = false;               // chunk_samples < 0: `chunk` rows, never a host round trip; a batch with more active samples is flagged on the device
    int32_t *overflow = nullptr;            // device: [0] this step's batch had more active samples than rows (Adam then skips), [1] how often that happened
    int num_cus = 256;
    // after the colour backward the step forks: weight-gradient GEMMs | colour-plane scatter | density / gauge backward are independent
    // chains of kernels none of which fills the device on its own (row transposes, LDS latency, the atomic unit); ngf_train_adam_all
    // updates the three planes side by side
    static constexpr int kAux = 2;
    hipStream_t aux[kAux] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kAux] = {nullptr, nullptr};
    bool has_adam = true;                   // false: built without Adam moments (ngf_train_forward / ngf_train_backward_grad only; ngf_train_adam* refuse)
    // what ngf_train_forward leaves for ngf_train_backward_grad (the two-call form of the step)
    struct Pending {
        bool valid = false;
        TrainArgs T;
        bool fork = false, no_sync = false, single = true;
        int64_t n = 0, list_len = 0;
        int32_t n_samples = 0;
        int64_t ticket = 0;
    } pending;
    int64_t tickets = 0;
};

extern "C" int ngf_trainer_destroy(ngf_trainer *t)
{
    if (!t) return NGF_OK;
    DeviceScope ds(t->dev);              // hipFree / stream teardown on the trainer's device, whatever is current in the calling thread
    t->mem.free_all();
    for (int k = 0; k < ngf_trainer::kAux; ++k) {
        if (t->aux[k]) { (void)hipStreamSynchronize(t->aux[k]); (void)hipStreamDestroy(t->aux[k]); }
        if (t->ev_join[k]) (void)hipEventDestroy(t->ev_join[k]);
    }
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    delete t;
    return NGF_OK;
}

extern "C" int64_t ngf_trainer_bytes(const ngf_trainer *t) { return t ? t->mem.bytes : 0; }
extern "C" int32_t ngf_sizeof_train_desc(void) { return (int32_t)sizeof(ngf_train_desc); }

// parameters -> packed textures where the trainer's copy of plane / gauge plane p is not current (ngf_train_adam* write the copy along with the
// parameter; ngf_train_params_changed marks every copy stale).  A pack writes the copy's zero border too.
static int pack_stale(ngf_trainer *t, int p, hipStream_t st)
{
    const ngf_train_desc &d = t->d;
    if (!t->tex_fresh[p]) {
        NGF_LAUNCH(pack_plane_kernel, dim3(2048), dim3(256), 0, st, d.plane[p], d.plane_h[p], d.plane_w[p], 0, 16, t->tex_d[p]);
        NGF_LAUNCH(pack_plane_kernel, dim3(2048), dim3(256), 0, st, d.plane[p], d.plane_h[p], d.plane_w[p], 16, 48, t->tex_a[p]);
        t->tex_fresh[p] = true;
    }
    if (!t->tex_fresh[3 + p]) {
        NGF_LAUNCH(pack_plane_kernel, dim3(256), dim3(256), 0, st, d.gauge[p], d.gauge_h[p], d.gauge_w[p], 0, 2, t->tex_g[p]);
        t->tex_fresh[3 + p] = true;
    }
    return NGF_OK;
}

extern "C" int ngf_trainer_create(const ngf_train_desc *d, ngf_trainer **out, void *hip_stream)
{
    if (!d || !out) return fail(NGF_E_ARG, "ngf_trainer_create: null argument");
    if (d->max_rays <= 0 || d->max_samples <= 0) return fail(NGF_E_ARG, "ngf_trainer_create: max_rays / max_samples must be positive");
    for (int p = 0; p < 3; ++p) {
        if (!d->plane[p] || d->plane_h[p] < 2 || d->plane_w[p] < 2) return fail(NGF_E_ARG, "plane %d missing or smaller than 2x2", p);
        if (!d->gauge[p] || d->gauge_h[p] < 2 || d->gauge_w[p] < 2) return fail(NGF_E_ARG, "gauge plane %d missing or smaller than 2x2", p);
    }
    if (!d->dens_w || !d->dens_b || !d->basis || !d->w1 || !d->b1 || !d->w2 || !d->b2 || !d->w3 || !d->b3)
        return fail(NGF_E_ARG, "ngf_trainer_create: missing MLP parameter");
    // Adam moments: all fifteen pairs, or none at all (a trainer that only serves ngf_train_forward / ngf_train_backward_grad -- the caller's
    // own optimiser applies the gradients, e.g. torch.optim.Adam in the reference's loop, TriPlane/main.py:241,294-296)
    int moments = 0;
    for (int k = 0; k < TP_COUNT; ++k) moments += (d->exp_avg[k] ? 1 : 0) + (d->exp_avg_sq[k] ? 1 : 0);
    if (moments != 0 && moments != 2 * TP_COUNT) return fail(NGF_E_ARG, "ngf_trainer_create: Adam state must be given for all %d parameters or for none", (int)TP_COUNT);
    ngf_trainer *t = new (std::nothrow) ngf_trainer();
    if (!t) return fail(NGF_E_HIP, "out of host memory");
    t->d = *d;
    t->has_adam = moments != 0;
    auto bail = [&](int rc) { ngf_trainer_destroy(t); return rc; };
    hipStream_t st = (hipStream_t)hip_stream;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) t->num_cus = prop.multiProcessorCount;
    t->dev = dev;
    int rc;
    for (int k = 0; k < ngf_trainer::kAux; ++k)
        if (hipStreamCreateWithFlags(&t->aux[k], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&t->ev_join[k], hipEventDisableTiming) != hipSuccess)
            return bail(fail(NGF_E_HIP, "trainer: stream / event creation failed"));
    if (hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming) != hipSuccess) return bail(fail(NGF_E_HIP, "trainer: event creation failed"));
    TrainArgs &T = t->proto;
    memset(&T, 0, sizeof(T));
    RenderArgs &A = T.R;
    const int64_t dn[TP_COUNT] = {0, 0, 0, 0, 0, 0, 48, 1, 144 * 144, 64 * 159, 64, 64 * 64, 64, 3 * 64, 3};
    // blocked gradient images (ngf_train.hpp, scatter_blocked): 16-float blocks of 4x4 texels (D_p) / 4x2 texels x 2 channels (gauge)
    auto dblk = [&](int p) { return (size_t)((d->plane_w[p] + 2 + 3) / 4) * ((d->plane_h[p] + 2 + 3) / 4) * 16; };
    auto gblk = [&](int p) { return (size_t)((d->gauge_w[p] + 2 + 3) / 4) * ((d->gauge_h[p] + 2 + 1) / 2) * 16; };
    // bins of the colour-plane scatter (ngf_train.hpp section 5b): 8x8 blocks of cells of the padded planes
    int nbins = 0;
    for (int p = 0; p < 3; ++p) {
        T.bin_base[p] = nbins;
        T.bin_nbx[p] = (d->plane_w[p] + 2 + 7) / 8;
        nbins += T.bin_nbx[p] * ((d->plane_h[p] + 2 + 7) / 8);
    }
    T.nbins = nbins;
    {   // the zero arena: [per plane: D_p, gauge gradient] [MLP gradients] [M] [loss] [bin counters], 256-byte aligned pieces
        size_t total = 0;
        auto add = [&](size_t floats) { total += (floats * sizeof(float) + 255) & ~(size_t)255; };
        for (int p = 0; p < 3; ++p) { add(dblk(p)); add(gblk(p)); }
        for (int k = TP_DENS_W; k < TP_COUNT; ++k) add((size_t)dn[k]);
        add((size_t)64 * 144); add(4);
        add((size_t)nbins + 1);
        if ((rc = t->mem.alloc(&t->zero_arena, total))) return bail(rc);
        t->zero_bytes = total;
    }
    size_t carved = 0;
    auto carve = [&](size_t floats) {
        float *q = reinterpret_cast<float *>(t->zero_arena + carved);
        carved += (floats * sizeof(float) + 255) & ~(size_t)255;
        return q;
    };
    for (int p = 0; p < 3; ++p) {
        const int H = d->plane_h[p], W = d->plane_w[p], gh = d->gauge_h[p], gw = d->gauge_w[p];
        const size_t tex = (size_t)(H + 2) * (W + 2), gtex = (size_t)(gh + 2) * (gw + 2);
        if ((rc = t->mem.alloc(&t->tex_d[p], tex * 16)) || (rc = t->mem.alloc(&t->tex_a[p], tex * 48)) || (rc = t->mem.alloc(&t->tex_g[p], gtex * 2)) ||
            (rc = t->mem.alloc(&t->q_d[p], tex)) || (rc = t->mem.alloc(&t->g_d[p], tex * 16)) || (rc = t->mem.alloc(&t->g_g[p], gtex * 2)))
            return bail(rc);
        t->d_d[p] = carve(dblk(p)); t->g_gb[p] = carve(gblk(p));
        // the colour planes' gradients are WRITTEN by train_bin_gather_kernel (every texel): no fill per step
        if ((rc = t->mem.alloc(&t->g_a[p], tex * 48))) return bail(rc);
        if (hipMemsetAsync(t->g_a[p], 0, tex * 48 * sizeof(float), st) != hipSuccess) return bail(fail(NGF_E_HIP, "trainer setup failed"));
        T.d_bw[p] = (W + 2 + 3) / 4; T.g_bw[p] = (gw + 2 + 3) / 4;
        A.dens[p] = Tex{t->tex_d[p], W, H, W + 2, (float)(W - 1), (float)(H - 1)};
        A.app[p] = Tex{t->tex_a[p], W, H, W + 2, (float)(W - 1), (float)(H - 1)};
        A.gau[p] = Tex{t->tex_g[p], gw, gh, gw + 2, (float)(gw - 1), (float)(gh - 1)};
        T.g_dens[p] = t->g_d[p]; T.g_app[p] = t->g_a[p]; T.g_gau[p] = t->g_gb[p];
        T.q_dens[p] = t->q_d[p]; T.d_dens[p] = t->d_d[p];
    }
    float *const dense_p[TP_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d->dens_w, d->dens_b, d->basis, d->w1, d->b1, d->w2, d->b2, d->w3, d->b3};
    for (int k = TP_DENS_W; k < TP_COUNT; ++k) {
        t->dense_p[k] = dense_p[k];
        t->dense_n[k] = dn[k];
        t->g_dense[k] = carve((size_t)dn[k]);
    }
    T.M = carve((size_t)64 * 144);
    T.loss = reinterpret_cast<double *>(carve(4));
    T.bin_count = reinterpret_cast<int32_t *>(carve((size_t)nbins + 1));
    if (carved != t->zero_bytes) return bail(fail(NGF_E_ARG, "trainer: zero arena layout mismatch"));
    T.wd = d->dens_w; T.bd = d->dens_b; T.basis = d->basis; T.w1 = d->w1; T.b1 = d->b1; T.w2 = d->w2; T.b2 = d->b2; T.w3 = d->w3; T.b3 = d->b3;
    T.g_wd = t->g_dense[TP_DENS_W]; T.g_bd = t->g_dense[TP_DENS_B];
    if ((rc = t->mem.alloc(&T.prof, (size_t)16))) return bail(rc);
    if (hipMemsetAsync(T.prof, 0, 16 * sizeof(unsigned long long), st) != hipSuccess) return bail(fail(NGF_E_HIP, "trainer setup failed"));
    T.g_b1 = t->g_dense[TP_B1]; T.g_b2 = t->g_dense[TP_B2]; T.g_b3 = t->g_dense[TP_B3];
    for (int k = 0; k < 3; ++k) {
        A.a0[k] = d->aabb[k];
        A.a1[k] = d->aabb[3 + k];
        A.inv[k] = 2.0f / (d->aabb[3 + k] - d->aabb[k]);
    }
    A.near_ = d->near_; A.far_ = d->far_; A.step = d->step; A.dscale = d->distance_scale; A.thr = d->weight_thres;
    if (d->mask_bits) {
        const size_t nbytes = ((size_t)d->mask_d * d->mask_h * d->mask_w + 7) / 8;
        if ((rc = t->mem.alloc(&t->mask, nbytes))) return bail(rc);
        if (hipMemcpyAsync(t->mask, d->mask_bits, nbytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return bail(fail(NGF_E_HIP, "copying the alpha mask failed"));
        A.mask.bits = t->mask;
        A.mask.D = d->mask_d; A.mask.H = d->mask_h; A.mask.W = d->mask_w;
        const size_t ncells = (size_t)(d->mask_d + 1) * (d->mask_h + 1) * (d->mask_w + 1);
        if (ncells >= ((size_t)1 << 32)) return bail(fail(NGF_E_ARG, "alpha mask of %d x %d x %d cells: the cell image is indexed with 32 bits", d->mask_d, d->mask_h, d->mask_w));
        if ((rc = t->mem.alloc(&t->mask_cells, ncells))) return bail(rc);
        auto cells = [&]() -> int {
            NGF_LAUNCH(mask_cells_kernel, dim3(2048), dim3(256), 0, st, (const uint8_t *)t->mask, d->mask_d, d->mask_h, d->mask_w, t->mask_cells);
            return NGF_OK;
        };
        if ((rc = cells())) return bail(rc);
        A.mask.cells = t->mask_cells;
        for (int k = 0; k < 3; ++k) {
            A.mask.a0[k] = d->mask_aabb[k];
            A.mask.inv[k] = 1.0f / (d->mask_aabb[3 + k] - d->mask_aabb[k]) * 2;
        }
    }
    const size_t cap = (size_t)d->max_rays * d->max_samples;
    // activation rows kept at once: by default the whole batch (1.7 KB per sample -- 6.2 GB for 4096 rays x 884 samples; the MI355X
    // has 288 GB), which also lets the step run without a host round trip; at most ~16 GB unless the caller asks otherwise
    // chunk_samples < 0 (speculative rows): |chunk_samples| rows, the step never waits for the host; a batch with more active samples than that
    // is flagged by the device (Adam skips the step, ngf_train_overflow_count reports it) -- 4096 x 884 pairs with rows for a third of them
    // are 3.4 GiB instead of 9.0
    t->speculative = d->chunk_samples < 0;
    const int64_t want = d->chunk_samples < 0 ? -d->chunk_samples : d->chunk_samples;
    t->chunk = want > 0 ? want : (int64_t)std::min<size_t>(cap, (size_t)9 << 20);
    if ((size_t)t->chunk > cap) t->chunk = (int64_t)((cap + 15) & ~(size_t)15);
    if (want <= 0 && (size_t)t->chunk >= cap) t->chunk = (int64_t)((cap + 15) & ~(size_t)15);
    if (t->speculative) t->chunk = (t->chunk + 15) & ~(int64_t)15;
    if ((rc = t->mem.alloc(&t->overflow, 2))) return bail(rc);
    if (hipMemsetAsync(t->overflow, 0, 2 * sizeof(int32_t), st) != hipSuccess) return bail(fail(NGF_E_HIP, "trainer setup failed"));
    if ((rc = t->mem.alloc(&T.et, cap)) || (rc = t->mem.alloc(&T.sg, cap)) || (rc = t->mem.alloc(&T.w, cap)) || (rc = t->mem.alloc(&T.dx, cap)) || (rc = t->mem.alloc(&T.c, cap * 3)) ||
        (rc = t->mem.alloc(&T.dt, cap * 6)) || (rc = t->mem.alloc(&T.G, (size_t)d->max_rays * 3)) || (rc = t->mem.alloc(&T.count, (size_t)d->max_rays)) ||
        (rc = t->mem.alloc(&T.offset, (size_t)d->max_rays + 1)) || (rc = t->mem.alloc(&T.list, cap * 2)) || (rc = t->mem.alloc(&T.list_w, cap)) ||
        (rc = t->mem.alloc(&t->bwd_image, (size_t)kBwdImage)) || (rc = t->mem.alloc(&t->fwd16_image, (size_t)MlpLayout16<48>::TOTAL)) ||
        (rc = t->mem.alloc(&T.bin_off, (size_t)nbins + 1)) || (rc = t->mem.alloc(&T.bin_unit, (size_t)nbins + 1)) || (rc = t->mem.alloc(&T.unit_total, (size_t)1)))
        return bail(rc);
    // The activation rows (576 floats per sample + the 18 of its scatter pairs).  If the whole-batch default does not fit the free HBM, fall back to round 1's chunked
    // mode (262 144 rows = 453 MB; the colour kernels then run chunk by chunk and the step reads the active count on the host) instead of
    // failing the create -- an explicit chunk_samples is taken as asked.
    for (int attempt = 0;; ++attempt) {
        const size_t ch = (size_t)t->chunk, mark = t->mem.ptrs.size();
        const int64_t bytes_mark = t->mem.bytes;
        T.bin_cap = (int32_t)ch;
        if (!((rc = t->mem.alloc(&T.F, ch * 144)) || (rc = t->mem.alloc(&T.V, ch * 16)) || (rc = t->mem.alloc(&T.H1, ch * 64)) || (rc = t->mem.alloc(&T.H2, ch * 64)) ||
              (rc = t->mem.alloc(&T.D3, ch * 16)) || (rc = t->mem.alloc(&T.D2, ch * 64)) || (rc = t->mem.alloc(&T.D1, ch * 64)) ||
              (rc = t->mem.alloc(&T.DF, ch * 144)) || (rc = t->mem.alloc(&T.pair_cell, ch * 3)) || (rc = t->mem.alloc(&T.pair_rank, ch * 3)) ||
              (rc = t->mem.alloc(&T.pair_w, ch * 12)) || (rc = t->mem.alloc(&T.perm, ch * 3)) ||
              (rc = t->mem.alloc(&T.units, ((size_t)nbins + ch * 3 / kBinChunk + 8) * 3)) ||
              (rc = t->mem.alloc(&T.slab, ((size_t)nbins + ch * 3 / kBinChunk + 8) * kBinTile))))
            break;
        t->mem.free_to(mark, bytes_mark);
        (void)hipGetLastError();
        if (attempt > 0 || d->chunk_samples != 0 || ch <= ((size_t)1 << 18)) return bail(rc);
        t->chunk = (int64_t)1 << 18;
    }
    // the packed copies (every tex_fresh starts false) and defined gradients before the first backward
    for (int p = 0; p < 3; ++p) {
        if ((rc = pack_stale(t, p, st))) return bail(rc);
        if (hipMemsetAsync(t->g_d[p], 0, (size_t)(d->plane_h[p] + 2) * (d->plane_w[p] + 2) * 16 * sizeof(float), st) != hipSuccess ||
            hipMemsetAsync(t->g_g[p], 0, (size_t)(d->gauge_h[p] + 2) * (d->gauge_w[p] + 2) * 2 * sizeof(float), st) != hipSuccess)
            return bail(fail(NGF_E_HIP, "trainer setup failed"));
    }
    if (hipMemsetAsync(t->zero_arena, 0, t->zero_bytes, st) != hipSuccess) return bail(fail(NGF_E_HIP, "trainer setup failed"));
    if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(NGF_E_HIP, "trainer setup failed: %s", hipGetErrorString(hipGetLastError())));
    *out = t;
    return NGF_OK;
}

static int tr_grid(const ngf_trainer *t, int64_t items, int per_block, int waves_per_cu = 8)
{
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t cap = (int64_t)t->num_cus * waves_per_cu;
    if (g > cap) g = cap;
    return g < 1 ? 1 : (int)g;
}

// One fork of a call: the work it has on the trainer's aux streams that the caller's stream `st` has not yet waited for.  begin() sends the
// listed aux streams behind st, done(j) marks the end of aux j's chain (right after its last launch), join() brings st behind every chain
// marked so far.  An error exit between begin() and join() must not leave aux-stream kernels that st never waits for (the next call on st
// would run beside them): the destructor marks and joins what is still open -- best effort, the error being reported stands -- and never
// waits on an event this call did not record.  on == false (ablate bit 1 << 19): aux(j) is st itself and nothing else happens.
struct Fork {
    ngf_trainer *t;
    hipStream_t st;
    bool on;
    bool open[ngf_trainer::kAux] = {};          // aux j was sent behind st and the end of its chain is not recorded yet
    bool recorded[ngf_trainer::kAux] = {};      // ev_join[j] is recorded and st has not waited for it yet
    Fork(ngf_trainer *t_, hipStream_t st_, bool on_) : t(t_), st(st_), on(on_) {}
    Fork(const Fork &) = delete;
    Fork &operator=(const Fork &) = delete;
    hipStream_t aux(int j) const { return on ? t->aux[j] : st; }
    int begin(std::initializer_list<int> js)
    {
        if (!on) return NGF_OK;
        HIP_TRY(hipEventRecord(t->ev_fork, st));
        for (int j : js) {
            HIP_TRY(hipStreamWaitEvent(t->aux[j], t->ev_fork, 0));
            open[j] = true;
        }
        return NGF_OK;
    }
    int done(int j)
    {
        if (!on) return NGF_OK;
        HIP_TRY(hipEventRecord(t->ev_join[j], t->aux[j]));
        open[j] = false;
        recorded[j] = true;
        return NGF_OK;
    }
    int join()
    {
        for (int j = 0; j < ngf_trainer::kAux; ++j)
            if (recorded[j]) {
                HIP_TRY(hipStreamWaitEvent(st, t->ev_join[j], 0));
                recorded[j] = false;
            }
        return NGF_OK;
    }
    ~Fork()
    {
        for (int j = 0; j < ngf_trainer::kAux; ++j)
            if (open[j] && hipEventRecord(t->ev_join[j], t->aux[j]) == hipSuccess) recorded[j] = true;
        for (int j = 0; j < ngf_trainer::kAux; ++j)
            if (recorded[j]) (void)hipStreamWaitEvent(st, t->ev_join[j], 0);
    }
};

// the end of ngf_train_adam_ext / ngf_train_adam_all, which send a plane to each aux stream: stream by stream, the update's end and the caller's wait
static int join_planes(Fork &f)
{
    for (int j = 0; j < ngf_trainer::kAux; ++j) {
        if (int rc = f.done(j)) return rc;
        if (int rc = f.join()) return rc;
    }
    return NGF_OK;
}

// the colour forward of the chunk T.chunk_base / T.chunk_n (activation rows kept when T.store)
static int launch_color_fwd(const ngf_trainer *t, const TrainArgs &T, hipStream_t st)
{
    NGF_LAUNCH(train_color_fwd16_kernel, dim3(tr_grid(t, (T.chunk_n + 15) / 16, kTrainWaves16, 1)), dim3(kTrainWaves16 * 64), kColorFwd16LdsBytes, st, T);
    return NGF_OK;
}

// The step in two parts.  Part A (train_forward_part): everything up to and including the colour forward -- after it the per-sample weights and
// colours of the batch are in the trainer's buffers.  Part B (train_backward_part): compositing backward, colour backward, the three forked
// chains.  The fused entry points run A, the fused compositing kernel <0> and B in one call; ngf_train_forward runs A and the compositing
// kernel <1> (rgb_map / depth_map out), ngf_train_backward_grad the compositing kernel <2> (d loss / d rgb_map in) and B.
static int train_forward_part(ngf_trainer *t, const float *rays, const float *jitter, int64_t n, int32_t n_samples, int32_t white_bg, int32_t gauge_on,
                              int64_t *n_active_host, void *hip_stream, ngf_trainer::Pending &P)
{
    if (n <= 0 || n > t->d.max_rays || n_samples <= 0 || n_samples > t->d.max_samples)
        return fail(NGF_E_ARG, "ngf_train_backward: n=%lld (max %lld), n_samples=%d (max %d)", (long long)n, (long long)t->d.max_rays, n_samples,
                    t->d.max_samples);
    hipStream_t st = (hipStream_t)hip_stream;
    const ngf_train_desc &d = t->d;
    P.valid = false;
    P.T = t->proto;
    TrainArgs &T = P.T;
    RenderArgs &A = T.R;
    A.rays = rays; A.jitter = jitter; A.n = n; A.S = n_samples; A.white_bg = white_bg ? 1 : 0; A.mode = gauge_on ? 1 : 0;
    T.inv_count = 1.0f / (3.0f * (float)n);
    A.ablate = knob(KNOB_ABLATE) > 0 ? knob(KNOB_ABLATE) : 0;      // timing experiments only (profiles/exp_train_ablate.sh)
    if (int prc = poison_lds(st)) return prc;
    // ngf_debug_set("ablate", 1 << 19) keeps the whole step on the caller's stream (see the forks below)
    const bool fork = !(A.ablate & (1 << 19));
    ProjectArgs PJ;
    PJ.wd = d.dens_w;
    // stale packed copies -> re-packed; gradient buffers -> 0
    for (int p = 0; p < 3; ++p) {
        if (int prc = pack_stale(t, p, st)) return prc;
        PJ.tex16[p] = t->tex_d[p]; PJ.texels[p] = (int64_t)(d.plane_h[p] + 2) * (d.plane_w[p] + 2); PJ.q[p] = t->q_d[p];
    }
    NGF_LAUNCH(train_project_density_kernel, dim3(128, 3), dim3(256), 0, st, PJ);
    HIP_TRY(hipMemsetAsync(t->zero_arena, 0, t->zero_bytes, st));
    // the LDS images of the colour MLP are first read by the colour forward: built beside the density kernel and the scan
    T.bwd_image = t->bwd_image; T.fwd16_image = t->fwd16_image;
    Fork fold(t, st, fork);
    if (int frc = fold.begin({0})) return frc;
    NGF_LAUNCH(train_fold_kernel, dim3(48), dim3(256), 0, fold.aux(0), T, t->bwd_image, t->fwd16_image);
    if (int frc = fold.done(0)) return frc;

    const int64_t pairs = n * n_samples;
    NGF_LAUNCH(train_density_kernel, dim3(tr_grid(t, pairs, 256)), dim3(256), 0, st, T);
    const int ray_blocks = (int)((n + 3) / 4);        // sixteen lanes per ray
    NGF_LAUNCH(train_scan_kernel, dim3(ray_blocks), dim3(64), 0, st, T, 0);
    // The overflow flag belongs to the path that cannot cut the list into chunks: speculative rows WITHOUT a host count.  A caller that passes
    // n_active_host gets the chunked path and a complete gradient -- flagging that step would make Adam skip a valid update.
    const bool spec_rows = t->speculative && !n_active_host;
    NGF_LAUNCH(train_prefix_kernel, dim3(1), dim3(1024), 0, st, (const int32_t *)T.count, n, T.offset, spec_rows ? t->chunk : (int64_t)0, t->overflow);
    // The colour kernels walk the active list.  When one chunk of activation rows holds every sample of the batch (the default:
    // HBM is sized for it) they read the active count from the device and run with fixed grids -- the stream never waits for the
    // host.  With a smaller chunk (chunk_samples of the descriptor) the count comes to the host to cut the list into chunks.
    const bool no_sync = (t->chunk >= pairs || t->speculative) && !n_active_host;
    int32_t n_active = 0;
    if (!no_sync) {
        HIP_TRY(hipMemcpyAsync(&n_active, T.offset + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n_active_host) *n_active_host = n_active;
    }
    NGF_LAUNCH(train_scan_kernel, dim3(ray_blocks), dim3(64), 0, st, T, 1);

    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(train_color_fwd16_kernel), kColorFwd16LdsBytes));
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(train_color_bwd_kernel), kColorBwdLdsBytes));
    if (int frc = fold.join()) return frc;          // the images
    const int32_t *cnt = no_sync ? T.offset + n : nullptr;
    T.n_active_dev = cnt;
    // upper bound of the list length the loops below are sized for (speculative rows: what the trainer keeps rows for -- the kernels stop at
    // min(that, the device's count); a longer list is flagged, train_prefix_kernel)
    const int64_t list_len = no_sync ? std::min<int64_t>(pairs, t->chunk) : n_active;
    const bool single = list_len <= t->chunk;
    // colour forward over the whole list (activations kept when the list fits one chunk)
    for (int64_t base = 0; base < list_len; base += t->chunk) {
        T.chunk_base = (int32_t)base;
        T.chunk_n = (int32_t)std::min<int64_t>(t->chunk, list_len - base);
        T.store = single ? 1 : 0;
        if (int lrc = launch_color_fwd(t, T, st)) return lrc;
    }
    P.fork = fork; P.no_sync = no_sync; P.single = single; P.n = n; P.n_samples = n_samples; P.list_len = list_len;
    P.valid = true;
    return NGF_OK;
}

// The four weight-gradient products of one chunk of activation rows, one launch: the step's own call and ngf_debug_train_xty (a test aid)
// both go through here.  gw1 is the whole [64][159] tensor: the product writes its 15 view columns.
static int launch_xty(int num_cus, const float *D1, const float *D2, const float *D3, const float *F, const float *H1, const float *H2,
                      const float *V, float *M, float *gw2, float *gw1, float *gw3, int rows, const int32_t *rows_dev, hipStream_t sx)
{
    int xg = (rows + 31) / 32;                      // 32-sample chunks; at most two workgroups per CU walk them
    if (xg > 2 * num_cus) xg = 2 * num_cus;
    // heaviest first: M = Delta1^T F (train_unfold_kernel turns it into d W1[:, :144] and d basis), d W2, the 15 view columns of d W1, d W3
    XtyAll G;
    G.X[0] = D1; G.ldx[0] = 64; G.Y[0] = F;  G.ldy[0] = 144; G.mvalid[0] = 64; G.nvalid[0] = 144; G.out[0] = M; G.ldo[0] = 144;
    G.X[1] = D2; G.ldx[1] = 64; G.Y[1] = H1; G.ldy[1] = 64;  G.mvalid[1] = 64; G.nvalid[1] = 64;  G.out[1] = gw2; G.ldo[1] = 64;
    G.X[2] = D1; G.ldx[2] = 64; G.Y[2] = V;  G.ldy[2] = 16;  G.mvalid[2] = 64; G.nvalid[2] = 15;  G.out[2] = gw1 + 144; G.ldo[2] = 159;
    G.X[3] = D3; G.ldx[3] = 16; G.Y[3] = H2; G.ldy[3] = 64;  G.mvalid[3] = 3;  G.nvalid[3] = 64;  G.out[3] = gw3; G.ldo[3] = 64;
    G.rows = rows; G.rows_dev = rows_dev;
    NGF_LAUNCH(xty_all_kernel, dim3(xg, 4), dim3(256), 0, sx, G);
    return NGF_OK;
}

extern "C" int ngf_debug_train_xty(const ngf_train_xty_args *a, void *hip_stream)
{
    if (!a) return fail(NGF_E_ARG, "ngf_debug_train_xty: null argument");
    if (a->size != (int32_t)sizeof(ngf_train_xty_args)) return fail(NGF_E_ARG, "ngf_debug_train_xty: ngf_train_xty_args layout mismatch");
    if (a->rows < 1 || a->rows > INT32_MAX) return fail(NGF_E_ARG, "ngf_debug_train_xty: rows = %lld must be in 1..2^31-1", (long long)a->rows);
    const float *in[7] = {a->d1, a->d2, a->d3, a->f, a->h1, a->h2, a->v};
    for (int k = 0; k < 7; ++k) {
        if (!in[k]) return fail(NGF_E_ARG, "ngf_debug_train_xty: operand %d is NULL", k);
        if (reinterpret_cast<uintptr_t>(in[k]) & 15) return fail(NGF_E_ARG, "ngf_debug_train_xty: operand %d is not 16-byte aligned", k);
    }
    if (!a->m || !a->gw2 || !a->gw1 || !a->gw3) return fail(NGF_E_ARG, "ngf_debug_train_xty: m, gw2, gw1 and gw3 must not be NULL");
    int dev = 0, num_cus = 256;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDevice(&dev));
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) num_cus = prop.multiProcessorCount;
    return launch_xty(num_cus, a->d1, a->d2, a->d3, a->f, a->h1, a->h2, a->v, a->m, a->gw2, a->gw1, a->gw3, (int)a->rows, a->rows_dev, (hipStream_t)hip_stream);
}

static inline dim3 comp_grid(int64_t n) { return dim3((unsigned)((n + 64 / kCompLanes - 1) / (64 / kCompLanes))); }

// Part B; the compositing kernel of the calling form has run on hip_stream.  rgb_loss may be NULL (no loss is delivered).
static int train_backward_part(ngf_trainer *t, ngf_trainer::Pending &P, double *rgb_loss, int32_t loss_len, void *hip_stream)
{
    hipStream_t st = (hipStream_t)hip_stream;
    const ngf_train_desc &d = t->d;
    TrainArgs &T = P.T;
    const bool no_sync = P.no_sync, single = P.single;
    const int64_t n = P.n, list_len = P.list_len;
    const int32_t n_samples = P.n_samples;
    Fork chains(t, st, P.fork);
    hipStream_t sx = chains.aux(0), sb = chains.aux(1);
    const int32_t *cnt = no_sync ? T.offset + n : nullptr;
    const dim3 dgrid(tr_grid(t, n * ((n_samples + 63) / 64), 4, knob(KNOB_TRAIN_DWG) > 0 ? knob(KNOB_TRAIN_DWG) : kDensBwdGroupsPerCu + 1));          // knob train_dwg (sweeps): workgroups per CU
    // After the colour backward of a chunk the step forks: the weight-gradient GEMMs (sx) and the colour-plane scatter (sb) leave the
    // caller's stream, which goes on with the density / gauge backward and waits for both before it returns to the caller's order.  None of
    // these chains fills the device alone (LDS transposes, LDS latency, the atomic unit).  (Tried: the density / gauge backward beside the
    // colour backward, with the colour path's d loss / d t scattered into the gauge planes by a kernel of its own -- the active entries of a
    // ray span the whole plane, their scatter cannot be merged in LDS, and the step got 0.17 ms slower.)
    for (int64_t base = 0; base < list_len; base += t->chunk) {
        T.chunk_base = (int32_t)base;
        T.chunk_n = (int32_t)std::min<int64_t>(t->chunk, list_len - base);
        const int passes = (T.chunk_n + 15) / 16;
        if (int jrc = chains.join()) return jrc;              // the previous chunk's chains read the rows this chunk overwrites
        if (!single) {
            T.store = 1;
            if (int lrc = launch_color_fwd(t, T, st)) return lrc;
        }
        T.bin_accumulate = base > 0 ? 1 : 0;
        if (base > 0) HIP_TRY(hipMemsetAsync(T.bin_count, 0, ((size_t)T.nbins + 1) * sizeof(int32_t), st));      // the first chunk's counters: the zero arena
        NGF_LAUNCH(train_color_bwd_kernel, dim3(tr_grid(t, passes, kTrainWavesBwd, 1)), dim3(kTrainWavesBwd * 64), kColorBwdLdsBytes, st, T);
        // colour-plane scatter: order the chunk's (plane, sample) pairs by bin, then one wave per unit (ngf_train.hpp section 5b); the
        // single-workgroup prefix stays on this stream, ahead of the fork (beside three full-device kernels it took 0.13 ms instead of 0.01)
        NGF_LAUNCH(train_bin_prefix_kernel, dim3(1), dim3(1024), 0, st, T);
        if (int frc = chains.begin({1, 0})) return frc;
        NGF_LAUNCH(train_bin_perm_kernel, dim3(tr_grid(t, 3 * (int64_t)T.chunk_n, 256)), dim3(256), 0, sb, T);
#ifdef NGF_EXPERIMENTS
        if (T.R.ablate & (1 << 18)) NGF_LAUNCH(train_bin_scatter_mfma_kernel, dim3(3 * t->num_cus), dim3(256), 0, sb, T);      // the matrix-pipe version (slower)
        else
#endif
        NGF_LAUNCH(train_bin_scatter_kernel, dim3(2 * t->num_cus), dim3(256), 0, sb, T);
        {   // one (texel, channel) per thread and two dependent loads each: as many workgroups as the largest plane has items (a few per thread
            // left the kernel waiting on memory latency: 40 us -> see profiles/r03_train_R1_kernel_stats.txt)
            int64_t items = 0;
            for (int p = 0; p < 3; ++p) items = std::max<int64_t>(items, (int64_t)(d.plane_h[p] + 2) * (d.plane_w[p] + 2) * 48);
            const int gx = (int)std::min<int64_t>((items + 255) / 256, (int64_t)64 * t->num_cus);
            NGF_LAUNCH(train_bin_gather_kernel, dim3(gx, 3), dim3(256), 0, sb, T);
        }
        if (int xrc = launch_xty(t->num_cus, T.D1, T.D2, T.D3, T.F, T.H1, T.H2, T.V, T.M, t->g_dense[TP_W2], t->g_dense[TP_W1], t->g_dense[TP_W3], T.chunk_n, cnt, sx))
            return xrc;
        if (base + t->chunk >= list_len) NGF_LAUNCH(train_unfold_kernel, dim3(96), dim3(256), 0, sx, T, t->g_dense[TP_W1], t->g_dense[TP_BASIS]);
        if (int frc = chains.done(0)) return frc;
        if (int frc = chains.done(1)) return frc;
    }
    if (list_len <= 0) {        // no active sample and the host knows it: nothing wrote the colour planes' gradients
        for (int p = 0; p < 3; ++p) HIP_TRY(hipMemsetAsync(t->g_a[p], 0, (size_t)(d.plane_h[p] + 2) * (d.plane_w[p] + 2) * 48 * sizeof(float), st));
        NGF_LAUNCH(train_unfold_kernel, dim3(96), dim3(256), 0, st, T, t->g_dense[TP_W1], t->g_dense[TP_BASIS]);
    }
    // (Tried: the D_p share <true, false> beside the colour backward and the gauge share <false, true> after it -- each half takes as long
    // as the whole, 0.31 ms: the kernel is bound by the dependent chain of an item, not by what it scatters.)
    NGF_LAUNCH((train_density_bwd_kernel<true, true>), dgrid, dim3(256), 0, st, T);
    UnblockArgs U;
    FinishArgs FA;
    FA.wd = d.dens_w; FA.g_wd = t->g_dense[TP_DENS_W];
    for (int p = 0; p < 3; ++p) {
        FA.D[p] = t->d_d[p]; FA.tex16[p] = t->tex_d[p]; FA.w2[p] = d.plane_w[p] + 2; FA.bw[p] = T.d_bw[p];
        FA.texels[p] = (int64_t)(d.plane_h[p] + 2) * (d.plane_w[p] + 2); FA.g_dens[p] = t->g_d[p];
        U.src[p] = t->g_gb[p]; U.dst[p] = t->g_g[p]; U.w2[p] = d.gauge_w[p] + 2; U.h2[p] = d.gauge_h[p] + 2; U.bw[p] = T.g_bw[p];
    }
    U.g_bd = T.g_bd;
    U.loss_src = T.loss; U.loss_dst = rgb_loss; U.loss_len = loss_len; U.inv_count = 1.0 / (3.0 * (double)n); U.overflow = t->overflow;        // the loss travels with the last kernel of the caller's stream (a copy of 8 bytes is a launch of its own)
    NGF_LAUNCH(train_density_finish_kernel, dim3(128, 3), dim3(256), 0, st, FA);
    NGF_LAUNCH(train_unblock_gauge_kernel, dim3(128, 3), dim3(256), 0, st, U);
    return chains.join();
}

static int train_backward_joined(ngf_trainer *t, const float *rays, const float *rgb_train, const float *jitter, int64_t n, int32_t n_samples,
                                 int32_t white_bg, int32_t gauge_on, double *rgb_loss, int32_t loss_len, int64_t *n_active_host, void *hip_stream)
{
    if (!t || !rays || !rgb_train || !rgb_loss) return fail(NGF_E_ARG, "ngf_train_backward: null argument");
    if (loss_len < 1) return fail(NGF_E_ARG, "ngf_train_backward2: loss_len=%d (1 = the sum of squared residuals, 2 = sum and mean)", loss_len);
    ngf_trainer::Pending P;                 // the fused call keeps its state to itself: a pending ngf_train_forward is not disturbed ...
    t->pending.valid = false;               // ... but the trainer's per-sample buffers are: its backward must re-run the forward
    if (int rc = train_forward_part(t, rays, jitter, n, n_samples, white_bg, gauge_on, n_active_host, hip_stream, P)) return rc;
    P.T.target = rgb_train;
    NGF_LAUNCH(train_composite_bwd_kernel<0>, comp_grid(n), dim3(64), 0, (hipStream_t)hip_stream, P.T);
    return train_backward_part(t, P, rgb_loss, loss_len, hip_stream);
}

// ---- the two-call form: the torch.autograd boundary of Base.forward(is_train=True) (TriPlane/main.py:272-296) -----------------------------
extern "C" int ngf_train_forward(ngf_trainer *t, const float *rays, const float *jitter, int64_t n, int32_t n_samples, int32_t white_bg,
                                 int32_t gauge_on, float *rgb_map, float *depth_map, int64_t *n_active_host, int64_t *ticket, void *hip_stream)
{
    if (!t || !rays || !rgb_map || !depth_map || !ticket) return fail(NGF_E_ARG, "ngf_train_forward: null argument");
    auto body = [&]() -> int {
        if (int rc = train_forward_part(t, rays, jitter, n, n_samples, white_bg, gauge_on, n_active_host, hip_stream, t->pending)) return rc;
        t->pending.T.rgb_out = rgb_map; t->pending.T.depth_out = depth_map;
        NGF_LAUNCH(train_composite_bwd_kernel<1>, comp_grid(n), dim3(64), 0, (hipStream_t)hip_stream, t->pending.T);
        return NGF_OK;
    };
    const int rc = body();
    if (rc == NGF_OK) t->pending.ticket = *ticket = ++t->tickets;
    else t->pending.valid = false;
    return rc;
}

extern "C" int ngf_train_backward_grad(ngf_trainer *t, int64_t ticket, const float *d_rgb_map, void *hip_stream)
{
    if (!t || !d_rgb_map) return fail(NGF_E_ARG, "ngf_train_backward_grad: null argument");
    if (!t->pending.valid || t->pending.ticket != ticket)
        return fail(NGF_E_STALE, "ngf_train_backward_grad: ticket %lld is not the trainer's last forward (%s) -- another forward or a fused step used the "
                    "trainer's buffers since; run ngf_train_forward again", (long long)ticket, t->pending.valid ? "a newer one is pending" : "none is pending");
    ngf_trainer::Pending &P = t->pending;
    P.valid = false;                        // the per-sample state is spent, whatever comes of this call; the gradients go to the trainer's buffers (ngf_train_get_grad)
    P.T.d_rgb = d_rgb_map;
    NGF_LAUNCH(train_composite_bwd_kernel<2>, comp_grid(P.n), dim3(64), 0, (hipStream_t)hip_stream, P.T);
    return train_backward_part(t, P, nullptr, 0, hip_stream);
}

// ABI 3: the loss buffer's length travels with the call (loss_len = 2: [0] the sum of squared residuals, [1] their mean)
extern "C" int ngf_train_backward2(ngf_trainer *t, const float *rays, const float *rgb_train, const float *jitter, int64_t n, int32_t n_samples,
                                   int32_t white_bg, int32_t gauge_on, double *rgb_loss, int32_t loss_len, int64_t *n_active_host, void *hip_stream)
{
    return train_backward_joined(t, rays, rgb_train, jitter, n, n_samples, white_bg, gauge_on, rgb_loss, loss_len, n_active_host, hip_stream);
}

// The ABI-1 entry point keeps the ABI-1 contract: rgb_loss is ONE double (the sum of squared residuals).  (ABI 2 wrote two doubles through
// this symbol: a caller built against ABI 1 got an 8-byte out-of-bounds device write.)
extern "C" int ngf_train_backward(ngf_trainer *t, const float *rays, const float *rgb_train, const float *jitter, int64_t n, int32_t n_samples,
                                  int32_t white_bg, int32_t gauge_on, double *rgb_loss, int64_t *n_active_host, void *hip_stream)
{
    return train_backward_joined(t, rays, rgb_train, jitter, n, n_samples, white_bg, gauge_on, rgb_loss, 1, n_active_host, hip_stream);
}

extern "C" int ngf_train_get_active(ngf_trainer *t, int64_t n, int32_t *out, void *hip_stream)
{
    if (!t || !out || n <= 0 || n > t->d.max_rays) return fail(NGF_E_ARG, "ngf_train_get_active: bad argument");
    HIP_TRY(hipMemcpyAsync(out, t->proto.offset + n, sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    return NGF_OK;
}

extern "C" int ngf_train_get_grad(ngf_trainer *t, int32_t which, float *out, void *hip_stream)
{
    if (!t || !out || which < 0 || which >= TP_COUNT) return fail(NGF_E_ARG, "ngf_train_get_grad: bad argument");
    hipStream_t st = (hipStream_t)hip_stream;
    if (which < 3) {
        const int p = which;
        NGF_LAUNCH(unpack_plane_kernel, dim3(1024), dim3(256), 0, st, (const float *)t->g_d[p], 16, (const float *)t->g_a[p], 64, t->d.plane_h[p],
                   t->d.plane_w[p], out);
    } else if (which < 6) {
        const int p = which - 3;
        NGF_LAUNCH(unpack_plane_kernel, dim3(256), dim3(256), 0, st, (const float *)t->g_g[p], 2, (const float *)nullptr, 2, t->d.gauge_h[p],
                   t->d.gauge_w[p], out);
    } else {
        HIP_TRY(hipMemcpyAsync(out, t->g_dense[which], (size_t)t->dense_n[which] * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return NGF_OK;
}

// ABI 5: every requested gradient in ONE call (out[k] NULL = not wanted): three tiled transposes for the planes, the gauge planes, one launch for
// the nine MLP parameters -- the autograd path (ngf_amd.train.RenderGrad.backward) made fifteen calls of ngf_train_get_grad per step.
extern "C" int ngf_train_get_grads(ngf_trainer *t, float *const *out, void *hip_stream)
{
    if (!t || !out) return fail(NGF_E_ARG, "ngf_train_get_grads: null argument");
    hipStream_t st = (hipStream_t)hip_stream;
    for (int p = 0; p < 3; ++p) {
        if (out[p]) {
            const int H = t->d.plane_h[p], W = t->d.plane_w[p];
            NGF_LAUNCH((unpack_plane_tiled_kernel<64, 16>), dim3(H * ((W + 63) / 64)), dim3(256), 0, st, (const float *)t->g_d[p], (const float *)t->g_a[p], H, W, out[p]);
        }
        if (out[3 + p])
            NGF_LAUNCH(unpack_plane_kernel, dim3(256), dim3(256), 0, st, (const float *)t->g_g[p], 2, (const float *)nullptr, 2, t->d.gauge_h[p], t->d.gauge_w[p], out[3 + p]);
    }
    CopyDenseAll D;
    int32_t at = 0;
    for (int j = 0; j < kDenseParams; ++j) {
        const int k = TP_DENS_W + j;
        D.src[j] = t->g_dense[k]; D.dst[j] = out[k]; D.begin[j] = at;
        if (out[k]) at += (int32_t)t->dense_n[k];
    }
    D.begin[kDenseParams] = at;
    if (at > 0) NGF_LAUNCH(copy_dense_all_kernel, dim3((at + 255) / 256), dim3(256), 0, st, D);
    return NGF_OK;
}

// ABI 5: torch.optim.Adam's update for the trainer's fifteen parameters from the CALLER'S gradient tensors and moments (reference layouts: what
// p.grad, state['exp_avg'], state['exp_avg_sq'] are after total_loss.backward()), planes in one pass that also writes the trainer's packed
// copy -- the next ngf_train_forward reads it without a re-pack.  step_count[k] <= 0 or grad[k] NULL = parameter k is left alone.  The arithmetic
// is ngf_train_adam's (adam_one); no L1 term is added here: the caller's loss put it into the gradient.  Works on trainers with or without
// their own moments.  ngf_amd.optim.Adam is the Python face (TriPlane/main.py:234-242,294-302 unchanged).
extern "C" int ngf_train_adam_ext(ngf_trainer *t, const float *const *grad, float *const *exp_avg, float *const *exp_avg_sq, const int32_t *step_count,
                                  const float *lr, float beta1, float beta2, float eps, void *hip_stream)
{
    if (!t || !grad || !exp_avg || !exp_avg_sq || !step_count || !lr) return fail(NGF_E_ARG, "ngf_train_adam_ext: null argument");
    const ngf_train_desc &d = t->d;
    hipStream_t st = (hipStream_t)hip_stream;
    auto args = [&](int k) { return adam_args(step_count[k], lr[k], beta1, beta2, eps, 0.0f); };
    for (int k = 0; k < TP_COUNT; ++k)
        if (step_count[k] > 0 && grad[k] && (!exp_avg[k] || !exp_avg_sq[k])) return fail(NGF_E_ARG, "ngf_train_adam_ext: parameter %d has a gradient but no moments", k);
    const bool fork = !(knob(KNOB_ABLATE) > 0 && (knob(KNOB_ABLATE) & (1 << 19)));
    const bool big[3] = {step_count[0] > 0 && grad[0], step_count[1] > 0 && grad[1], step_count[2] > 0 && grad[2]};
    Fork planes(t, st, fork && (big[1] || big[2]));
    if (int frc = planes.begin({0, 1})) return frc;
    for (int p : {1, 2, 0}) {
        if (!big[p]) continue;
        const int H = d.plane_h[p], W = d.plane_w[p];
        // a stale packed copy (ngf_train_params_changed since the last forward) is simply rewritten: the kernel stores every interior texel and the
        // zero border was written when the copy was first packed
        NGF_LAUNCH((adam_plane_kernel<64, 16, true>), dim3(H * ((W + 63) / 64)), dim3(256), 0, p > 0 ? planes.aux(p - 1) : st, d.plane[p], exp_avg[p],
                   exp_avg_sq[p], H, W, (const float *)nullptr, (const float *)nullptr, t->tex_d[p], t->tex_a[p], args(p), (const int32_t *)nullptr, grad[p]);
        t->tex_fresh[p] = true;
    }
    for (int p = 0; p < 3; ++p) {
        const int k = 3 + p;
        if (!(step_count[k] > 0 && grad[k])) continue;
        NGF_LAUNCH((adam_plane_kernel<2, 2, true>), dim3(d.gauge_h[p] * ((d.gauge_w[p] + 63) / 64)), dim3(256), 0, st, d.gauge[p], exp_avg[k], exp_avg_sq[k],
                   d.gauge_h[p], d.gauge_w[p], (const float *)nullptr, (const float *)nullptr, t->tex_g[p], (float *)nullptr, args(k), (const int32_t *)nullptr, grad[k]);
        t->tex_fresh[k] = true;
    }
    HIP_TRY(adam_dense_all<kDenseParams>(t->dense_p + TP_DENS_W, exp_avg + TP_DENS_W, exp_avg_sq + TP_DENS_W, grad + TP_DENS_W, t->dense_n + TP_DENS_W,
                                         step_count + TP_DENS_W, lr + TP_DENS_W, beta1, beta2, eps,
                                         [&](int j) { return step_count[TP_DENS_W + j] > 0 && grad[TP_DENS_W + j]; }, nullptr, st));
    return join_planes(planes);
}

// What ngf_train_adam refuses of the trainer's state for parameter `which` (NGF_OK: it would launch).  ngf_train_adam_all asks for every
// parameter before its first launch: a refused call has changed nothing.
static int adam_refused(const ngf_trainer *t, int which)
{
    if (!t->has_adam) return fail(NGF_E_ARG, "ngf_train_adam: the trainer was made without Adam moments (ngf_train_desc.exp_avg / exp_avg_sq all NULL)");
    if (which < 6 && !t->tex_fresh[which]) return fail(NGF_E_ARG, "ngf_train_adam: the planes changed (ngf_train_params_changed) and no backward has re-packed them");
    return NGF_OK;
}

extern "C" int ngf_train_adam(ngf_trainer *t, int32_t which, int32_t step_count, float lr, float beta1, float beta2, float eps, float l1_weight,
                              void *hip_stream)
{
    if (!t || which < 0 || which >= TP_COUNT || step_count < 1) return fail(NGF_E_ARG, "ngf_train_adam: bad argument");
    if (int rc = adam_refused(t, which)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const ngf_train_desc &d = t->d;
    AdamArgs a = adam_args(step_count, lr, beta1, beta2, eps, 0.0f);
    if (which < 3) {
        const int p = which, H = d.plane_h[p], W = d.plane_w[p];
        a.l1 = l1_weight / (float)((int64_t)64 * H * W);             // d/dp of l1_weight * mean(|p|)
        NGF_LAUNCH((adam_plane_kernel<64, 16>), dim3(H * ((W + 63) / 64)), dim3(256), 0, st, d.plane[p], d.exp_avg[which], d.exp_avg_sq[which], H, W,
                   (const float *)t->g_d[p], (const float *)t->g_a[p], t->tex_d[p], t->tex_a[p], a, (const int32_t *)t->overflow);
    } else if (which < 6) {
        const int p = which - 3;
        NGF_LAUNCH((adam_plane_kernel<2, 2>), dim3(d.gauge_h[p] * ((d.gauge_w[p] + 63) / 64)), dim3(256), 0, st, d.gauge[p], d.exp_avg[which],
                   d.exp_avg_sq[which], d.gauge_h[p], d.gauge_w[p], (const float *)t->g_g[p], (const float *)nullptr, t->tex_g[p], (float *)nullptr, a, (const int32_t *)t->overflow);
    } else {
        NGF_LAUNCH(adam_dense_kernel, dim3(64), dim3(256), 0, st, t->dense_p[which], (const float *)t->g_dense[which], d.exp_avg[which], d.exp_avg_sq[which],
                   t->dense_n[which], a, (const int32_t *)t->overflow);
    }
    return NGF_OK;
}

// Speculative rows (ngf_train_desc::chunk_samples < 0): how many steps since the trainer was made had more active samples than activation rows
// (their Adam updates were skipped on the device) and the trainer's row count.  Synchronises the stream.
extern "C" int ngf_train_overflow_count(ngf_trainer *t, int64_t *count_host, int64_t *rows_host, void *hip_stream)
{
    if (!t || !count_host) return fail(NGF_E_ARG, "ngf_train_overflow_count: null argument");
    int32_t v[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(v, t->overflow, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    *count_host = v[1];
    if (rows_host) *rows_host = t->chunk;
    return NGF_OK;
}

// debug: the section clocks of the colour backward (ngf_debug_set("ablate", 1 << 20)), summed over waves since the last call
extern "C" int ngf_train_debug_sections(ngf_trainer *t, uint64_t *out16)
{
    if (!t || !out16) return fail(NGF_E_ARG, "ngf_train_debug_sections: null argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, t->proto.prof, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(t->proto.prof, 0, 16 * sizeof(uint64_t)));
    return NGF_OK;
}

extern "C" int ngf_train_params_changed(ngf_trainer *t)
{
    if (!t) return fail(NGF_E_ARG, "ngf_train_params_changed: null trainer");
    for (bool &f : t->tex_fresh) f = false;
    return NGF_OK;
}

extern "C" int ngf_train_adam_all(ngf_trainer *t, const int32_t *step_count, const float *lr, float beta1, float beta2, float eps, float l1_weight,
                                  void *hip_stream)
{
    if (!t || !step_count || !lr) return fail(NGF_E_ARG, "ngf_train_adam_all: null argument");
    const ngf_train_desc &d = t->d;
    for (int k = 0; k < TP_COUNT; ++k)
        if (step_count[k] > 0)
            if (int rc = adam_refused(t, k)) return rc;
    // the three (plane, gauge plane) pairs are independent streams of reads and writes, none of which reaches the HBM rate alone: planes 1
    // and 2 go to the trainer's own streams (ablate bit 1 << 19: all on the caller's)
    hipStream_t st = (hipStream_t)hip_stream;
    Fork planes(t, st, !(knob(KNOB_ABLATE) > 0 && (knob(KNOB_ABLATE) & (1 << 19))));
    if (int frc = planes.begin({0, 1})) return frc;
    // planes 1 and 2 leave first; the caller's stream takes the small updates (gauge planes, the MLP parameters below) and plane 0
    for (int k : {1, 2, 3, 4, 5})
        if (step_count[k] > 0)
            if (int rc = ngf_train_adam(t, k, step_count[k], lr[k], beta1, beta2, eps, l1_weight, (void *)(k < 3 ? planes.aux(k - 1) : st))) return rc;
    HIP_TRY(adam_dense_all<kDenseParams>(t->dense_p + TP_DENS_W, d.exp_avg + TP_DENS_W, d.exp_avg_sq + TP_DENS_W, t->g_dense + TP_DENS_W, t->dense_n + TP_DENS_W,
                                         step_count + TP_DENS_W, lr + TP_DENS_W, beta1, beta2, eps, [&](int j) { return step_count[TP_DENS_W + j] > 0; },
                                         t->overflow, st));
    if (step_count[0] > 0)
        if (int rc = ngf_train_adam(t, 0, step_count[0], lr[0], beta1, beta2, eps, l1_weight, hip_stream)) return rc;
    return join_planes(planes);
}

