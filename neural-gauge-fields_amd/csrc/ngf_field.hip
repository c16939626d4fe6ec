// ngf_field.hip -- C ABI (include/ngf.h), TriPlane / InfoInv part: field handle, render / march / decode / alpha-mask / ray
// entry points, and the services of ngf_host.hpp (error slot, knobs, LDS poisoning).  The TriPlane training step is ngf_train.hip (it shares
// the plane packing kernels of ngf_pack.hpp).  No torch, no CPU fallback: every entry point runs HIP kernels or fails.  Build: see Makefile
// (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off).
#include <map>
#include <mutex>
#include <utility>

#include "ngf_host.hpp"
#include "ngf_infoinv.hpp"
#include "ngf_mlp_image.hpp"
#include "ngf_pack.hpp"
#include "ngf_render.hpp"
#include "ngf_alpha.hpp"
#include "ngf_query.hpp"
#ifdef NGF_EXPERIMENTS      // libngf_hip_exp.so only (make: second target): kernels that were built, measured and lost -- specialised march / shade
                            // waves, LDS-staged texture strips -- and the tuning variants (8 / 16 waves, two steps per lane, section profile).  The
                            // product library carries only kernels that can be the default; the experiment tests load the other one.
#include "ngf_render_pc.hpp"
#include "ngf_stage.hpp"
#endif

using namespace ngf;

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int ngf::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static std::atomic<int> g_knob[ngf::KNOB_COUNT];
static const char *const g_knob_name[ngf::KNOB_COUNT] = {"tile_w", "split", "waves", "nstep", "profile", "ablate", "uv_tiles", "kernel", "stage", "poison", "grid", "xcd", "tail", "ord_rows", "ord_px", "train_dwg", "pairpack"};
static bool g_knob_init = [] { for (auto &k : g_knob) k.store(-1); return true; }();

int ngf::knob(int id) { return g_knob[id].load(std::memory_order_relaxed); }
static std::atomic<int> g_last_waves{-1};      // waves per workgroup of the last render launch (ngf_debug_get("last_waves"): the tests see which kernel a launch took)

hipError_t ngf::ensure_dynamic_lds(const void *kernel, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> done;         // (device, kernel) -> largest size set so far
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = done[{dev, kernel}];
    if (have >= bytes && have != 0) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

// ---- knob "poison": LDS / allocation poisoning (ngf_host.hpp) ---------------------------------------------------------------------
__global__ void __launch_bounds__(1024) dirty_lds_kernel(unsigned pattern, int words, int spin)
{
    extern __shared__ unsigned dirty_smem[];
    for (int i = threadIdx.x; i < words; i += blockDim.x) dirty_smem[i] = pattern;
    __syncthreads();
    // hold the CU's LDS for a moment so that the other blocks of the grid land on the other CUs (one 160 KB block per CU at a time)
    const unsigned long long t0 = __builtin_readcyclecounter();
    while (__builtin_readcyclecounter() - t0 < (unsigned long long)spin) __builtin_amdgcn_s_sleep(8);
    if (dirty_smem[(threadIdx.x * 97) % words] != pattern) __builtin_trap();
}

int ngf::poison_lds(hipStream_t st)
{
    if (knob(KNOB_POISON) < 0 || !(knob(KNOB_POISON) & 1)) return NGF_OK;
    constexpr int kBytes = 160 * 1024;
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        cus = prop.multiProcessorCount;
    }
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(dirty_lds_kernel), kBytes));
    hipLaunchKernelGGL(dirty_lds_kernel, dim3(2 * cus), dim3(1024), kBytes, st, kPoisonPattern, kBytes / 4, 40000);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

int ngf::poison_alloc(void *p, size_t bytes, hipStream_t st)
{
    if (knob(KNOB_POISON) < 0 || !(knob(KNOB_POISON) & 2) || !p) return NGF_OK;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p, (int)kPoisonPattern, bytes / 4, st));
    return NGF_OK;
}

extern "C" int ngf_debug_dirty_lds(void *hip_stream)
{
    const int old = g_knob[ngf::KNOB_POISON].load();
    g_knob[ngf::KNOB_POISON].store(1);
    const int rc = ngf::poison_lds((hipStream_t)hip_stream);
    g_knob[ngf::KNOB_POISON].store(old);
    return rc;
}

// where do the workgroups of a launch land?  out[x] += 1 per workgroup on XCD x (tests: every XCD id 0..7 is seen, evenly)
__global__ void xcd_histogram_kernel(unsigned *out)
{
    if (threadIdx.x == 0) atomicAdd(out + xcd_id(), 1u);
    const unsigned long long t0 = __builtin_readcyclecounter();
    while (__builtin_readcyclecounter() - t0 < 20000ull) __builtin_amdgcn_s_sleep(8);      // keep the CU busy: one workgroup per CU like the render launches
}
extern "C" int ngf_debug_xcd_histogram(unsigned *out8, int32_t workgroups, void *hip_stream)
{
    if (!out8 || workgroups <= 0) return fail(NGF_E_ARG, "ngf_debug_xcd_histogram: bad argument");
    HIP_TRY(hipMemsetAsync(out8, 0, 8 * sizeof(unsigned), (hipStream_t)hip_stream));
    hipLaunchKernelGGL(xcd_histogram_kernel, dim3(workgroups), dim3(768), 0, (hipStream_t)hip_stream, out8);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

extern "C" int ngf_debug_set(const char *name, int32_t value)
{
    if (!name) return fail(NGF_E_ARG, "ngf_debug_set: null name");
    for (int k = 0; k < ngf::KNOB_COUNT; ++k)
        if (!strcmp(name, g_knob_name[k])) { g_knob[k].store(value); return NGF_OK; }
    return fail(NGF_E_ARG, "ngf_debug_set: unknown knob '%s'", name);
}

extern "C" int32_t ngf_debug_get(const char *name)
{
    if (name)
        for (int k = 0; k < ngf::KNOB_COUNT; ++k)
            if (!strcmp(name, g_knob_name[k])) return g_knob[k].load();
    if (name && !strcmp(name, "last_waves")) return g_last_waves.load();      // read-only
    return -1;
}

struct ngf_field {
    int32_t model = 0, flags = 0, plane_c = 0, dens_dim = 0, app = 0;
    float *tex[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // dens[3], app[3], gau[3]
    float *blob = nullptr;
    float *basis_pack = nullptr;
    double *w1pd_tmp = nullptr;               // create only: the same values as doubles (bake_color_kernel's weights)
    float *w1p_tmp = nullptr;                 // create only: W1' = W1[:, :F] . basis folded on the device (freed before create returns; here so that an error exit frees it)
    uint8_t *mask = nullptr;
    uint8_t *mask_cells = nullptr;            // the mask's corner bytes per trilinear cell (mask_cells_kernel)
    uint8_t *mask_any = nullptr, *mask_clear = nullptr, *mask_clear4 = nullptr;   // blocks of 8^3 (4^3) cells: occupied at all (scratch of the build) / nothing within 8 (4) cells (mask_block_*_kernel)
    unsigned int *counters = nullptr;
    mutable std::atomic<unsigned> next_counter{0};
    RenderArgs proto;
    int64_t bytes = 0;
    int num_cus = 256;
    std::vector<std::pair<void *, size_t>> allocs;      // every device buffer of the handle (pointer, bytes): ngf_field_destroy hands them to the pool
    // round 6: the device the handle lives on and every stream a launch that reads its buffers was put on -- ngf_field_destroy waits for
    // THOSE streams (one event each) on THAT device instead of a hipDeviceSynchronize on whatever device is current in the calling thread
    int dev = 0;
    mutable std::mutex use_mu;
    mutable std::vector<hipStream_t> streams;
    mutable std::atomic<void *> last_stream{(void *)(intptr_t)-1};
};

// every launch that reads the handle's buffers reports its stream (a pointer compare in the steady state)
static inline void field_use(const ngf_field *f, hipStream_t st)
{
    if (f->last_stream.load(std::memory_order_relaxed) == (void *)st) return;
    std::lock_guard<std::mutex> lk(f->use_mu);
    bool known = false;
    for (hipStream_t s : f->streams) known |= s == st;
    if (!known) f->streams.push_back(st);
    f->last_stream.store((void *)st, std::memory_order_relaxed);
}

// ---- packing kernels: pack_plane_kernel, packed_plane_floats, mask_cells_kernel are in ngf_pack.hpp (the TriPlane trainer packs with them too) ----
// tests: the size arithmetic of packed_plane_floats
extern "C" int64_t ngf_debug_packed_plane_floats(int32_t H, int32_t W, int32_t nc, int32_t pair)
{
    if (H < 1 || W < 1 || nc < 1) return -1;
    return (int64_t)packed_plane_floats(H, W, nc, pair != 0);
}

// Alpha mask, block images (round 6): empty-space skipping.  Blocks of B^3 cells, B = 2^LOG, over the cell indices -16 .. size + 16 per axis (block = (cell index + 16) >> LOG).
// Pass 1: any[block] = some cell of the block has an occupied corner (one wave per block, a lane per (z, y) row of B cells).
template <int LOG>
__global__ void __launch_bounds__(64) mask_block_any_kernel(const uint8_t *__restrict__ cells, int D, int H, int W, int bH, int bW, uint8_t *__restrict__ any)
{
    constexpr int B = 1 << LOG;
    const int b = blockIdx.x, X = b % bW, Y = (b / bW) % bH, Z = b / (bW * bH);
    const int z = Z * B - 16 + ((int)threadIdx.x >> LOG), y = Y * B - 16 + ((int)threadIdx.x & (B - 1));
    unsigned acc = 0;
    if ((int)threadIdx.x < B * B && z >= 0 && z <= D && y >= 0 && y <= H) {
        const uint8_t *row = cells + ((size_t)z * (H + 1) + y) * (W + 1);
#pragma unroll
        for (int t = 0; t < B; ++t) {
            const int x = X * B - 16 + t;
            if (x >= 0 && x <= W) acc |= row[x];
        }
    }
    const unsigned long long m = __ballot(acc != 0);
    if (threadIdx.x == 0) any[b] = m ? 1 : 0;
}

// Pass 2: clear[block] = the block and its 26 neighbours hold nothing (blocks outside the grid are empty space).
__global__ void __launch_bounds__(256) mask_block_clear_kernel(const uint8_t *__restrict__ any, int cD, int cH, int cW, uint8_t *__restrict__ clear)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= cD * cH * cW) return;
    const int X = b % cW, Y = (b / cW) % cH, Z = b / (cW * cH);
    unsigned acc = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = X + dx, y = Y + dy, z = Z + dz;
                if (x >= 0 && x < cW && y >= 0 && y < cH && z >= 0 && z < cD) acc |= any[(z * cH + y) * cW + x];
            }
    clear[b] = acc ? 0 : 1;
}

// density_decoder Linear(48,1) pre-composed with the density channels of one plane (fp64 accumulate)
__global__ void bake_density_kernel(const float *__restrict__ src, int H, int W, int nc, const float *__restrict__ wd,
                                    float *__restrict__ dst, int pair)
{
    const size_t total = (size_t)(H + 2) * (W + 2);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % (W + 2)), y = (int)(i / (W + 2));
        double v = 0.0;
        if (x >= 1 && x <= W && y >= 1 && y <= H)
            for (int c = 0; c < nc; ++c) v += (double)wd[c] * (double)src[((size_t)c * H + (y - 1)) * W + (x - 1)];
        if (pair) {          // the row-pair form (pack_plane_kernel)
            dst[i * 2] = (float)v;
            if (y >= 1) dst[(i - (W + 2)) * 2 + 1] = (float)v;
            if (y == H + 1) dst[i * 2 + 1] = 0.0f;
        } else dst[i] = (float)v;
    }
}

// rgb_decoder layer 1 (pre-composed with basis) applied per texel: dst[(y,x)][j] = sum_c wp[j][c] * src[c0+c][y][x]
// (fp64 accumulate); wp = this plane's nc (<= 48) columns of W1' [64][ldw], as doubles (fold_w1_basis_kernel's second output: the fp32-rounded values);
// channel n of a baked texel = unit n.
// Round 5: a workgroup takes 64 consecutive padded texels (one per lane: every channel's read is one 256-byte run of the plane), wave w the outputs
// 16 w .. 16 w + 15 -- sixteen independent fp64 chains per lane whose weights are wave-uniform (scalar loads, SGPR operands of v_fma_f64).  Round 4 had one
// thread per output (48 serial loads of one address per wave): 375 us per 256^2 plane.  Same sums: a product of two floats is exact in fp64, so every
// partial sum is rounded where the one-thread-per-output loop rounded it -- bit-identical planes.
__global__ void __launch_bounds__(256) bake_color_kernel(const float *__restrict__ src, int H, int W, int c0, int nc, const double *__restrict__ wp, int ldw,
                                                         float *__restrict__ dst)
{
    const size_t texels = (size_t)(H + 2) * (W + 2), plane = (size_t)H * W;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double *wr = wp + (size_t)(16 * w) * ldw;            // wave-uniform
    for (size_t t0 = (size_t)blockIdx.x * 64; t0 < texels; t0 += (size_t)gridDim.x * 64) {
        const size_t tx = t0 + lane;
        if (tx >= texels) continue;
        const int x = (int)(tx % (W + 2)), y = (int)(tx / (W + 2));
        const bool inside = x >= 1 && x <= W && y >= 1 && y <= H;
        const float *sp = src + ((size_t)c0 * H + (inside ? y - 1 : 0)) * W + (inside ? x - 1 : 0);
        double acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.0;
#pragma unroll 4
        for (int c = 0; c < nc; ++c) {
            const double v = (double)sp[(size_t)c * plane];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] += wr[(size_t)k * ldw + c] * v;
        }
        f32x4 *o = reinterpret_cast<f32x4 *>(dst + tx * 64 + 16 * w);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = inside ? f32x4{(float)acc[4 * q], (float)acc[4 * q + 1], (float)acc[4 * q + 2], (float)acc[4 * q + 3]} : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

// W1' = W1[:, :F] . basis, [64][F], fp64 accumulate with j ascending, rounded to fp32 once -- what every image builder below places (they used to fold
// on the host: 1.3 M (TriPlane) / 3 M (InfoInv) fp64 multiply-adds of one thread, 0.5 / 1.2 ms of every create; the same sums to the bit: a product of
// two floats is exact in fp64, one rounding per addition, -ffp-contract=off on both sides anyway).  w1p_d (may be NULL): the same fp32 values as doubles,
// what bake_color_kernel multiplies with.  Round 5.
__global__ void __launch_bounds__(256) fold_w1_basis_kernel(const float *__restrict__ w1, const float *__restrict__ basis, int F, float *__restrict__ w1p,
                                                            double *__restrict__ w1p_d)
{
    const int IN = F + 15, total = 64 * F;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int k = i % F, n = i / F;                       // lanes on consecutive k: basis rows are read in runs
        double s = 0.0;
#pragma unroll 8
        for (int j = 0; j < F; ++j) s += (double)w1[(size_t)n * IN + j] * (double)basis[(size_t)j * F + k];
        w1p[i] = (float)s;
        if (w1p_d) w1p_d[i] = (double)(float)s;
    }
}

// get_ray_directions + get_rays (ray_utils.py:24-42, 66-87; blender.py:52)
__global__ void generate_rays_kernel(int H, int W, float focal, float r00, float r01, float r02, float r10, float r11,
                                     float r12, float r20, float r21, float r22, float ox, float oy, float oz, int row0,
                                     int rows, float *__restrict__ rays)
{
    const int64_t total = (int64_t)rows * W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(q % W), row = row0 + (int)(q / W);
        const float i = (float)col + 0.5f, j = (float)row + 0.5f;
        float dx = (i - (float)W / 2) / focal, dy = (j - (float)H / 2) / focal, dz = 1.0f;
        const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);
        dx = dx / nrm; dy = dy / nrm; dz = dz / nrm;
        float *r = rays + q * 6;
        r[0] = ox; r[1] = oy; r[2] = oz;
        r[3] = (dx * r00 + dy * r01) + dz * r02;
        r[4] = (dx * r10 + dy * r11) + dz * r12;
        r[5] = (dx * r20 + dy * r21) + dz * r22;
    }
}

// get_rays_dir on the 'no_crop' pixel grid (UV-Mapping/data/dtu.py:27-37, 160-168): integer pixel coordinates, float32 focal /
// principal point / rotation as the shipped in_cam*.npy hold them; dirs = rot^T (x, y, 1) summed in row order, / (norm + 1e-5)
__global__ void generate_rays_dtu_kernel(int W, float fx, float fy, float cx, float cy, float r00, float r01, float r02, float r10,
                                         float r11, float r12, float r20, float r21, float r22, int row0, int rows, float *__restrict__ raydir)
{
    const int64_t total = (int64_t)rows * W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(q % W), row = row0 + (int)(q / W);
        const float x = ((float)col - cx) / fx, y = ((float)row - cy) / fy;
        float dx = (r00 * x + r10 * y) + r20, dy = (r01 * x + r11 * y) + r21, dz = (r02 * x + r12 * y) + r22;
        const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz) + 1e-5f;
        float *r = raydir + q * 3;
        r[0] = dx / nrm; r[1] = dy / nrm; r[2] = dz / nrm;
    }
}


// ---- buffer pool of the field handles (round 5) ---------------------------------------------------------------------------------
// A handle is rebuilt after every parameter change of an eval field (Base.handle()): same shapes, so the same ten buffer sizes.  hipFree
// synchronises the device and cost 0.7 ms per destroy -- more than the create's own work (0.5 ms) -- and hipMalloc is not free either.
// Destroyed handles therefore park their buffers here (exact-size reuse, per device; at most kPoolEntries buffers / kPoolBytes; the rest
// goes back to the driver), after ONE hipDeviceSynchronize in ngf_field_destroy (what the first hipFree used to do implicitly: kernels
// of any stream may still read the buffers).  ngf_pool_trim() returns everything to the driver.
struct PoolEntry { void *p; size_t bytes; int dev; uint64_t age; };
static std::mutex g_pool_mu;
static std::vector<PoolEntry> g_pool;
static size_t g_pool_bytes = 0;
static uint64_t g_pool_clock = 0;
static size_t g_pool_cap_bytes = (size_t)1 << 30;        // ngf_pool_set_limit; a level-3 TriPlane handle at 256^2 is 52 MB + 67 MB, a 300^2 one 160 MB
constexpr size_t kPoolEntries = 64;

static void pool_release(const std::vector<PoolEntry> &out)          // hipFree outside the lock, each on its own device
{
    for (const PoolEntry &e : out) {
        DeviceScope ds(e.dev);
        (void)hipFree(e.p);
    }
}

// entries of `dev` (or of every device: dev < 0) leave the pool, oldest first, until at most keep_bytes / keep_entries are parked
static void pool_evict_locked(std::vector<PoolEntry> &out, int dev, size_t keep_bytes, size_t keep_entries)
{
    while (!g_pool.empty() && (g_pool_bytes > keep_bytes || g_pool.size() > keep_entries)) {
        size_t oldest = g_pool.size();
        for (size_t i = 0; i < g_pool.size(); ++i)
            if ((dev < 0 || g_pool[i].dev == dev) && (oldest == g_pool.size() || g_pool[i].age < g_pool[oldest].age)) oldest = i;
        if (oldest == g_pool.size()) break;
        out.push_back(g_pool[oldest]);
        g_pool_bytes -= g_pool[oldest].bytes;
        g_pool[oldest] = g_pool.back();
        g_pool.pop_back();
    }
}

// `dev` = the device the buffer is for (the handle's); the caller has made it the current one
static hipError_t pool_malloc(void **p, size_t bytes, int dev)
{
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); ++i)
            if (g_pool[i].bytes == bytes && g_pool[i].dev == dev) {
                *p = g_pool[i].p;
                g_pool_bytes -= bytes;
                g_pool[i] = g_pool.back();
                g_pool.pop_back();
                return hipSuccess;
            }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        // out of memory while this pool sits on parked buffers nobody else can see (torch's caching allocator cannot): give them all back and try once more
        (void)hipGetLastError();
        std::vector<PoolEntry> out;
        {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            pool_evict_locked(out, -1, 0, 0);
        }
        if (out.empty()) return e;
        pool_release(out);
        e = hipMalloc(p, bytes);
    }
    return e;
}

static void pool_free(void *p, size_t bytes, int dev)          // the caller has made sure that nothing on device `dev` still uses p
{
    if (!p) return;
    std::vector<PoolEntry> out;
    bool parked = false;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (bytes <= g_pool_cap_bytes) {
            // full: the OLDEST parked buffers make room (after up_sampling / shrink the old sizes never match again -- round 5 refused the
            // new ones instead and kept the stale ones for the life of the process)
            pool_evict_locked(out, -1, g_pool_cap_bytes - bytes, kPoolEntries - 1);
            g_pool.push_back(PoolEntry{p, bytes, dev, ++g_pool_clock});
            g_pool_bytes += bytes;
            parked = true;
        }
    }
    pool_release(out);
    if (!parked) {
        DeviceScope ds(dev);
        (void)hipFree(p);
    }
}

extern "C" int ngf_pool_trim(void)
{
    std::vector<PoolEntry> out;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        pool_evict_locked(out, -1, 0, 0);
    }
    pool_release(out);
    return NGF_OK;
}

extern "C" int ngf_pool_set_limit(int64_t bytes)
{
    if (bytes < 0) return fail(NGF_E_ARG, "ngf_pool_set_limit: %lld", (long long)bytes);
    std::vector<PoolEntry> out;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pool_cap_bytes = (size_t)bytes;
        pool_evict_locked(out, -1, g_pool_cap_bytes, kPoolEntries);
    }
    pool_release(out);
    return NGF_OK;
}

extern "C" int64_t ngf_pool_bytes(int32_t device)          // parked bytes of one device (device < 0: of all) -- tests, memory reports
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int64_t b = 0;
    for (const PoolEntry &e : g_pool)
        if (device < 0 || e.dev == device) b += (int64_t)e.bytes;
    return b;
}

static int field_alloc(ngf_field *f, void **p, size_t bytes, const char *what)
{
    if (pool_malloc(p, bytes, f->dev) != hipSuccess) { *p = nullptr; return fail(NGF_E_HIP, "hipMalloc(%s, %zu bytes) failed on device %d", what, bytes, f->dev); }
    f->allocs.emplace_back(*p, bytes);
    f->bytes += (int64_t)bytes;
    return NGF_OK;
}

static int alloc_f(float **p, size_t n, ngf_field *f, hipStream_t st)
{
    int rc = field_alloc(f, (void **)p, n * sizeof(float), "texture / image");
    if (rc) return rc;
    return poison_alloc(*p, n * sizeof(float), st);
}

// ------------------------------------------------------------------------------------------------
extern "C" int ngf_abi_version(void) { return NGF_ABI_VERSION; }
extern "C" int ngf_sizeof_field_desc(void) { return (int)sizeof(ngf_field_desc); }
extern "C" const char *ngf_last_error(void) { return g_err; }
extern "C" int64_t ngf_field_bytes(const ngf_field *f) { return f ? f->bytes : 0; }

extern "C" int ngf_field_destroy(ngf_field *f)
{
    if (!f) return NGF_OK;
    if (!f->allocs.empty()) {
        // Launches may still read the buffers: wait for the streams the handle was used on -- on the handle's device, whatever device is
        // current in the calling thread (round 5 synchronised the CURRENT device and parked the buffers under ITS id) -- and for nothing
        // else: no device-wide synchronisation.  A stream the caller has destroyed in the meantime has finished its work (hipStreamDestroy
        // drains it); if the runtime refuses it, or the event cannot be made, the device-wide wait is the fallback.
        DeviceScope ds(f->dev);
        std::vector<hipStream_t> used;
        {
            std::lock_guard<std::mutex> lk(f->use_mu);
            used = f->streams;
        }
        bool waited = true;
        hipEvent_t ev = nullptr;
        if (!used.empty()) {
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; waited = false; }
            for (size_t i = 0; waited && i < used.size(); ++i)
                waited = hipEventRecord(ev, used[i]) == hipSuccess && hipEventSynchronize(ev) == hipSuccess;
            if (ev) (void)hipEventDestroy(ev);
        }
        if (!waited) { (void)hipGetLastError(); (void)hipDeviceSynchronize(); }
        for (const auto &a : f->allocs) pool_free(a.first, a.second, f->dev);
    }
    delete f;
    return NGF_OK;
}

extern "C" int ngf_field_create(const ngf_field_desc *d, ngf_field **out, void *hip_stream)
{
    if (!d || !out) return fail(NGF_E_ARG, "ngf_field_create: null argument");
    *out = nullptr;
    const bool tri = d->model == NGF_MODEL_TRIPLANE;
    if (!tri && d->model != NGF_MODEL_INFOINV) return fail(NGF_E_ARG, "unknown model %d", d->model);
    if (tri && (d->plane_c != 64 || d->dens_dim != 16)) return fail(NGF_E_UNSUPPORTED, "TriPlane expects 64-channel planes with 16 density channels");
    if (!tri && (d->plane_c != 96 || d->dens_dim != 24)) return fail(NGF_E_UNSUPPORTED, "InfoInv expects 96-channel planes with 24 density channels");
    for (int p = 0; p < 3; ++p) {
        if (!d->plane[p] || d->plane_h[p] < 2 || d->plane_w[p] < 2) return fail(NGF_E_ARG, "plane %d missing or smaller than 2x2", p);
        if (tri && (!d->gauge[p] || d->gauge_h[p] < 2 || d->gauge_w[p] < 2)) return fail(NGF_E_ARG, "gauge plane %d missing or smaller than 2x2", p);
    }
    if (!(d->step > 0.0f)) return fail(NGF_E_ARG, "step must be > 0");
    hipStream_t st = (hipStream_t)hip_stream;
#ifdef NGF_EXP_CREATE_TIMES                    // experiment build (profiles/exp_create_phases.py): the phases of a create on stderr
    auto tc0 = std::chrono::steady_clock::now();
#define NGF_CT(label) do { auto t1 = std::chrono::steady_clock::now(); fprintf(stderr, "create %-28s %8.1f us\n", label, std::chrono::duration<double, std::micro>(t1 - tc0).count()); tc0 = t1; } while (0)
#else
#define NGF_CT(label) do { } while (0)
#endif
    ngf_field *f = new (std::nothrow) ngf_field();
    if (!f) return fail(NGF_E_HIP, "out of host memory");
    f->model = d->model; f->flags = d->flags; f->plane_c = d->plane_c; f->dens_dim = d->dens_dim;
    f->app = d->plane_c - d->dens_dim;
    const int F = 3 * f->app;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) f->num_cus = prop.multiProcessorCount;
    f->dev = dev;                   // the caller's current device: where the parameter tensors and the stream live
    field_use(f, st);               // the packing kernels below write the handle's buffers on this stream

    int rc = NGF_OK;
    RenderArgs &A = f->proto;
    memset(&A, 0, sizeof(A));
    auto bail = [&](int code) { ngf_field_destroy(f); return code; };

    const bool bake = tri && (d->flags & NGF_F_BAKE_DENSITY);
    const bool bake_c = tri && (d->flags & NGF_F_BAKE_COLOR);
    const bool no_fold = tri && (d->flags & NGF_F_NO_FOLD);
    const bool split_bf16 = tri && (d->flags & NGF_F_SPLIT_BF16);
    if (no_fold && (bake || bake_c)) return bail(fail(NGF_E_ARG, "NGF_F_NO_FOLD is the un-composed formulation: it excludes the NGF_F_BAKE_* flags"));
    if (split_bf16 && no_fold) return bail(fail(NGF_E_ARG, "NGF_F_SPLIT_BF16 applies to the pre-composed formulations (not with NGF_F_NO_FOLD)"));
    if (split_bf16 && bake_c && !bake) return bail(fail(NGF_E_ARG, "NGF_F_BAKE_COLOR | NGF_F_SPLIT_BF16 (level 3 with layer 2 on the bf16 matrix pipe) is built on top of NGF_F_BAKE_DENSITY"));

    // MLP weights: to the host once, pre-compose, permute, back to HBM as one LDS image
    // W1' = W1[:, :F] . basis comes folded from the device (fold_w1_basis_kernel) for every formulation that pre-composes it; level 0 streams basis itself
    FieldWeights Wt;
    std::vector<float> &basis = Wt.basis, &w1p = Wt.w1p, &w1 = Wt.w1, &b1 = Wt.b1, &w2 = Wt.w2, &b2 = Wt.b2, &w3 = Wt.w3, &b3 = Wt.b3;
    if (!d->basis || !d->w1) return bail(fail(NGF_E_ARG, "missing weight tensor"));
    if (no_fold) {
        if ((rc = d2h(basis, d->basis, (size_t)F * F, st))) return bail(rc);
    } else {
        if ((rc = field_alloc(f, (void **)&f->w1p_tmp, (size_t)64 * F * sizeof(float), "W1'"))) return bail(rc);
        if (bake_c && (rc = field_alloc(f, (void **)&f->w1pd_tmp, (size_t)64 * F * sizeof(double), "W1' (fp64)"))) return bail(rc);
        fold_w1_basis_kernel<<<(64 * F + 255) / 256, 256, 0, st>>>(d->w1, d->basis, F, f->w1p_tmp, f->w1pd_tmp);
        if ((rc = d2h(w1p, f->w1p_tmp, (size_t)64 * F, st))) return bail(rc);
    }
    if ((rc = d2h(w1, d->w1, (size_t)64 * (F + 15), st)) ||
        (rc = d2h(b1, d->b1, 64, st)) || (rc = d2h(w2, d->w2, 64 * 64, st)) || (rc = d2h(b2, d->b2, 64, st)) ||
        (rc = d2h(w3, d->w3, 3 * 64, st)) || (rc = d2h(b3, d->b3, 3, st)))
        return bail(rc);
    std::vector<float> &dw1 = Wt.dw1, &db1 = Wt.db1, &dw2 = Wt.dw2, &db2 = Wt.db2, &dw3 = Wt.dw3, &db3 = Wt.db3;
    if (tri) {
        if ((rc = d2h(dw1, d->dens_w1, 48, st)) || (rc = d2h(db1, d->dens_b1, 1, st))) return bail(rc);
    } else {
        if ((rc = d2h(dw1, d->dens_w1, 32 * 72, st)) || (rc = d2h(db1, d->dens_b1, 32, st)) ||
            (rc = d2h(dw2, d->dens_w2, 32 * 32, st)) || (rc = d2h(db2, d->dens_b2, 32, st)) ||
            (rc = d2h(dw3, d->dens_w3, 32, st)) || (rc = d2h(db3, d->dens_b3, 1, st)))
            return bail(rc);
    }
    if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(NGF_E_HIP, "hipStreamSynchronize failed in ngf_field_create"));
    NGF_CT("fold kernel + D2H + sync");

    std::vector<float> img, bpack;          // the LDS image (colour, then InfoInv's density MLP) and the matrix the shade streams from L2
    build_field_images(d->model, d->flags, Wt, img, bpack);
    NGF_CT("host images");
    if ((rc = alloc_f(&f->blob, img.size(), f, st))) return bail(rc);
    if (hipMemcpyAsync(f->blob, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess)
        return bail(fail(NGF_E_HIP, "uploading the MLP image failed"));
    A.blob = f->blob;
    A.blob_floats = (int)img.size();
    if (!bpack.empty()) {        // the matrix the shade streams from L2 (level-0 basis / lo parts of InfoInv's split layer 1)
        if ((rc = alloc_f(&f->basis_pack, bpack.size(), f, st))) return bail(rc);
        if (hipMemcpyAsync(f->basis_pack, bpack.data(), bpack.size() * sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess)
            return bail(fail(NGF_E_HIP, "uploading the packed basis matrix failed"));
        A.basis_pack = f->basis_pack;
    }
    if (tri) {
        for (int i = 0; i < 48; ++i) A.wd[i] = dw1[i];
        A.bd = db1[0];
    }

    NGF_CT("image upload");
    // textures: channel-last, zero-bordered
    // The march's planes of a baked-density handle (levels 2, 3): the row-pair form (struct Tex) -- the handle is re-packed whenever the parameters change, so
    // the cell's second row is put next to its first once, here.  Level 1 keeps the one-row gauge planes with its 16-channel density texels (its
    // render kernel has no register to spare: bil_setup), and so do the trainer's images, which the optimiser updates in place.
    bool pair = bake;
#ifdef NGF_EXPERIMENTS
    if (knob(KNOB_PAIRPACK) == 0) pair = false;          // A/B: the one-row layout, read by the kernels' RenderArgs::pairpack == 0 path
#else
    if (knob(KNOB_PAIRPACK) == 0) return bail(fail(NGF_E_UNSUPPORTED, "knob pairpack = 0 (the one-row layout of the march's planes) exists in libngf_hip_exp.so only"));
#endif
    A.pairpack = pair ? 1 : 0;
    A.gauge_same = 0;
    if (tri && bake) {
        A.gauge_same = 1;
        for (int p = 0; p < 3; ++p) A.gauge_same &= d->gauge_h[p] == d->gauge_w[0] && d->gauge_w[p] == d->gauge_w[0];
    }
    const int app_c = bake_c ? 64 : f->app;
    for (int p = 0; p < 3; ++p) {
        const int H = d->plane_h[p], W = d->plane_w[p];
        const size_t texels = (size_t)(H + 2) * (W + 2);
        const int dc = bake ? 1 : d->dens_dim;
        if (texels * (size_t)(app_c > 96 ? app_c : 96) * sizeof(float) >= ((size_t)1 << 32)) {     // the kernels address a texture with 32-bit byte offsets (tex_at)
            return bail(fail(NGF_E_UNSUPPORTED, "plane %d: %d x %d texels do not fit a 4 GiB packed texture", p, H, W));
        }
        if ((rc = alloc_f(&f->tex[p], packed_plane_floats(H, W, dc, pair), f, st)) || (rc = alloc_f(&f->tex[3 + p], texels * app_c, f, st))) return bail(rc);
        if (bake) bake_density_kernel<<<1024, 256, 0, st>>>(d->plane[p], H, W, d->dens_dim, d->dens_w1 + p * d->dens_dim, f->tex[p], pair ? 1 : 0);
        else pack_plane_kernel<<<2048, 256, 0, st>>>(d->plane[p], H, W, 0, d->dens_dim, f->tex[p]);
        if (bake_c) bake_color_kernel<<<2048, 256, 0, st>>>(d->plane[p], H, W, d->dens_dim, f->app, f->w1pd_tmp + (size_t)p * f->app, F, f->tex[3 + p]);
        else pack_plane_kernel<<<2048, 256, 0, st>>>(d->plane[p], H, W, d->dens_dim, f->app, f->tex[3 + p], tri ? 0 : 1);
        A.dens[p] = Tex{f->tex[p], W, H, W + 2, (float)(W - 1), (float)(H - 1)};
        A.app[p] = Tex{f->tex[3 + p], W, H, W + 2, (float)(W - 1), (float)(H - 1)};
        if (tri) {
            const int gh = d->gauge_h[p], gw = d->gauge_w[p];
            if ((rc = alloc_f(&f->tex[6 + p], packed_plane_floats(gh, gw, 2, pair), f, st))) return bail(rc);
            pack_plane_kernel<<<256, 256, 0, st>>>(d->gauge[p], gh, gw, 0, 2, f->tex[6 + p], 0, pair ? 1 : 0);
            A.gau[p] = Tex{f->tex[6 + p], gw, gh, gw + 2, (float)(gw - 1), (float)(gh - 1)};
        }
    }
    NGF_CT("texture allocs + launches");
    const bool launch_ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    NGF_CT("sync (pack / bake kernels)");
    f->w1p_tmp = nullptr; f->w1pd_tmp = nullptr;          // (the buffers stay in f->allocs: it goes to the pool with the handle -- the next create of these shapes takes it from there)
    if (!launch_ok) return bail(fail(NGF_E_HIP, "packing kernels failed"));

    for (int k = 0; k < 3; ++k) {
        A.a0[k] = d->aabb[k];
        A.a1[k] = d->aabb[3 + k];
        A.inv[k] = 2.0f / (d->aabb[3 + k] - d->aabb[k]);      // invaabbSize (FieldBase.py:67)
    }
    A.near_ = d->near_; A.far_ = d->far_; A.step = d->step; A.dscale = d->distance_scale; A.thr = d->weight_thres;
    if (d->mask_bits) {
        const size_t nbytes = ((size_t)d->mask_d * d->mask_h * d->mask_w + 7) / 8;
        if ((rc = field_alloc(f, (void **)&f->mask, nbytes, "mask"))) return bail(rc);
        if (hipMemcpyAsync(f->mask, d->mask_bits, nbytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return bail(fail(NGF_E_HIP, "copying the alpha mask failed"));
        A.mask.bits = f->mask;
        A.mask.D = d->mask_d; A.mask.H = d->mask_h; A.mask.W = d->mask_w;
        const size_t ncells = (size_t)(d->mask_d + 1) * (d->mask_h + 1) * (d->mask_w + 1);
        if (ncells >= ((size_t)1 << 32)) return bail(fail(NGF_E_ARG, "alpha mask of %d x %d x %d cells: the cell image is indexed with 32 bits", d->mask_d, d->mask_h, d->mask_w));
        if ((rc = field_alloc(f, (void **)&f->mask_cells, ncells, "mask cells"))) return bail(rc);
        hipLaunchKernelGGL(mask_cells_kernel, dim3(2048), dim3(256), 0, st, (const uint8_t *)f->mask, d->mask_d, d->mask_h, d->mask_w, f->mask_cells);
        if (hipGetLastError() != hipSuccess) return bail(fail(NGF_E_HIP, "mask_cells_kernel failed to launch"));
        A.mask.cells = f->mask_cells;
        const int cD = ((d->mask_d + 32) >> 3) + 1, cH = ((d->mask_h + 32) >> 3) + 1, cW = ((d->mask_w + 32) >> 3) + 1;
        const int fD = ((d->mask_d + 32) >> 2) + 1, fH = ((d->mask_h + 32) >> 2) + 1, fW = ((d->mask_w + 32) >> 2) + 1;
        if ((rc = field_alloc(f, (void **)&f->mask_any, (size_t)fD * fH * fW, "mask blocks"))) return bail(rc);          // scratch of both builds (the finer image is the larger one)
        if ((rc = field_alloc(f, (void **)&f->mask_clear, (size_t)cD * cH * cW, "mask blocks"))) return bail(rc);
        if ((rc = field_alloc(f, (void **)&f->mask_clear4, (size_t)fD * fH * fW, "mask blocks"))) return bail(rc);
        hipLaunchKernelGGL(mask_block_any_kernel<3>, dim3((unsigned)(cD * cH * cW)), dim3(64), 0, st, (const uint8_t *)f->mask_cells, d->mask_d, d->mask_h, d->mask_w, cH, cW, f->mask_any);
        hipLaunchKernelGGL(mask_block_clear_kernel, dim3((unsigned)((cD * cH * cW + 255) / 256)), dim3(256), 0, st, (const uint8_t *)f->mask_any, cD, cH, cW, f->mask_clear);
        hipLaunchKernelGGL(mask_block_any_kernel<2>, dim3((unsigned)(fD * fH * fW)), dim3(64), 0, st, (const uint8_t *)f->mask_cells, d->mask_d, d->mask_h, d->mask_w, fH, fW, f->mask_any);
        hipLaunchKernelGGL(mask_block_clear_kernel, dim3((unsigned)((fD * fH * fW + 255) / 256)), dim3(256), 0, st, (const uint8_t *)f->mask_any, fD, fH, fW, f->mask_clear4);
        if (hipGetLastError() != hipSuccess) return bail(fail(NGF_E_HIP, "mask_block kernels failed to launch"));
        A.mask.fine = f->mask_clear4;
        A.mask.coarse = f->mask_clear; A.mask.cD = cD; A.mask.cH = cH; A.mask.cW = cW;
        for (int k = 0; k < 3; ++k) {
            A.mask.a0[k] = d->mask_aabb[k];
            A.mask.inv[k] = 1.0f / (d->mask_aabb[3 + k] - d->mask_aabb[k]) * 2;   // invgridSize (FieldBase.py:29)
        }
    }
    if ((rc = field_alloc(f, (void **)&f->counters, (size_t)kCounters * kQueueHeads * sizeof(unsigned), "counters"))) return bail(rc);
    if (hipMemsetAsync(f->counters, 0, (size_t)kCounters * kQueueHeads * sizeof(unsigned), st) != hipSuccess) return bail(fail(NGF_E_HIP, "zeroing the queue heads failed"));
    if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(NGF_E_HIP, "packing failed: %s", hipGetErrorString(hipGetLastError())));
    NGF_CT("mask + counters + sync");
    *out = f;
    return NGF_OK;
}

// The tile plan of a render launch (see launch_render): n rays, widest tile `wide`, `resident` waves in the persistent grid, tail16 / 16 narrow
// tiles per resident wave of each narrower width.  Fills up to four (rays, log2 width) segments in ray order, returns their number.  Every
// segment but the last holds whole tiles.  Pure host arithmetic (ngf_debug_tile_plan exposes it to the CPU tests).
static constexpr int kTailDefault16 = 16;
static int make_tile_plan(int64_t n, int wide, int64_t resident, int tail16, int64_t seg_rays[4], int seg_shift[4])
{
    auto shift_of = [](int w) { int sft = 0; while ((1 << sft) < w) ++sft; return sft; };
    // A launch that fits the persistent grid with ONE tile per wave (n <= resident x wide): the narrowest pair of widths (w, w / 2) that does it, as
    // many w / 2-ray tiles as the wave count allows -- the launch then lasts one w-ray tile.  (Round 5.  The tail rule below gave a 4096-ray chunk on
    // 3072 waves 512 two-ray and 3072 one-ray tiles: 512 waves took a second tile behind their first, 0.114 ms; 1024 two-ray + 2048 one-ray tiles are
    // one tile per wave, profiles/r05_shard_latency.txt.)  Knob tail = 0 keeps its meaning: wide tiles only.
    if (tail16 > 0 && resident > 0 && n > 0 && n <= resident * wide) {
        int w = 1;
        while ((int64_t)w * resident < n) w <<= 1;                  // smallest width whose tiles cover n rays with <= resident tiles
        if (w == 1) { seg_rays[0] = n; seg_shift[0] = 0; return 1; }
        const int a = w >> 1;
        auto allowed = [&](int v) { return v == wide || v == 4 || v == 2 || v == 1; };      // the widths the kernels' tile plans are tested with
        if (allowed(w) && allowed(a)) {
        // x tiles of w rays first, then tiles of a rays: x + y <= resident, w x + a y >= n  ->  x = ceil((n - a resident) / a)
        int64_t x = (n - (int64_t)a * resident + a - 1) / a;
        if (x < 0) x = 0;
        if (x * w > n) x = n / w;
        const int64_t rw = x * w, ra = n - rw;
        int nseg = 0;
        if (rw > 0) { seg_rays[nseg] = rw; seg_shift[nseg] = shift_of(w); ++nseg; }
        if (ra > 0) { seg_rays[nseg] = ra; seg_shift[nseg] = shift_of(a); ++nseg; }
        return nseg;
        }
    }
    const int widths[4] = {wide, 4, 2, 1};
    int64_t left = n, want[4] = {0, 0, 0, 0};
    for (int k = 3; k >= 1; --k) {      // the narrow segments are sized from the END of the ray list
        if (widths[k] >= wide) continue;
        // tail16 < 256: the same count for every narrow width; >= 256 (sweeps): one byte per width -- bits 0-7 one-ray, 8-15 two-ray, 16-23 four-ray tiles
        const int tk = tail16 < 256 ? tail16 : (tail16 >> (8 * (3 - k))) & 0xff;
        want[k] = std::min<int64_t>(left, (resident * tk / 16) * widths[k]);
        left -= want[k];
    }
    want[0] = left;
    int nseg = 0;
    int64_t carry = 0;
    for (int k = 0; k < 4; ++k) {       // what does not fill a tile moves to the next narrower segment
        int64_t r = want[k] + carry;
        carry = 0;
        if (k < 3) { carry = r % widths[k]; r -= carry; }
        if (r <= 0) continue;
        if (nseg > 0 && seg_shift[nseg - 1] == shift_of(widths[k])) { seg_rays[nseg - 1] += r; continue; }
        seg_rays[nseg] = r; seg_shift[nseg] = shift_of(widths[k]); ++nseg;
    }
    if (nseg == 0) { seg_rays[0] = n; seg_shift[0] = 0; nseg = 1; }
    return nseg;
}

// the device's queue-position -> tile map of ngf_field_render_image, on the host (CPU test: a bijection of [0, ord_n) for every plan)
extern "C" int ngf_debug_tile_order(const uint32_t *q, int64_t count, uint32_t ord_n, uint32_t tpr, uint32_t bw, uint32_t bh, uint32_t *out)
{
    if (!q || !out || count < 0 || !tpr || !bw || !bh) return fail(NGF_E_ARG, "ngf_debug_tile_order: bad argument");
    for (int64_t i = 0; i < count; ++i) out[i] = tile_order(q[i], ord_n, tpr, bw, bh);
    return NGF_OK;
}

extern "C" int ngf_debug_tile_plan(int64_t n, int32_t wide, int64_t resident, int32_t tail16, int64_t *seg_rays, int32_t *seg_shift)
{
    int64_t r[4] = {0, 0, 0, 0};
    int sh[4] = {0, 0, 0, 0};
    const int nseg = make_tile_plan(n, wide, resident, tail16 >= 0 ? tail16 : kTailDefault16, r, sh);
    for (int k = 0; k < 4; ++k) { seg_rays[k] = k < nseg ? r[k] : 0; seg_shift[k] = k < nseg ? sh[k] : 0; }
    return nseg;
}

// ---- launches ------------------------------------------------------------------------------------
// kernel / kernel_split: the DBG = true instantiations (every feature); kernel_prod: the split kernel's production instantiation (no debug
// outputs, ablation bits, statistics: render_kernel<P, true, false>) or null when the policy has none
template <typename K>
static int launch_render(K kernel, K kernel_split, K kernel_prod, const ngf_field *f, RenderArgs &A, int threads, size_t lds_bytes, hipStream_t st, int wide_tile, int max_split_shift = 6)
{
    // the slot's queue heads are zero: ngf_field_create zeroed all slots, and the last wave of every launch zeroes its slot again (queue_done)
    const unsigned slot = f->next_counter.fetch_add(1) % kCounters;
    A.tile_counter = f->counters + (size_t)slot * kQueueHeads;
    if (int rc = poison_lds(st)) return rc;
    // Split march (render_kernel<P, true>): a tile holds tile_w rays and every ray is marched by 64 / tile_w lanes on
    // consecutive steps (bit-identical results).  Small tiles shorten the critical path of a tile and even out the
    // tiles-per-wave quantisation, which bounds small launches (one rank's shard of a frame, the reference's 4096-ray
    // chunks) and still buys 5 % on a full frame.  Measured in profiles/r01_split_march.txt: tile_w = 8 is best from
    // 160 000 rays to the full frame, tile_w = 4 below (80 000 rays: 1.43-1.49 vs 1.51-1.53 ms; 4000 rays: 0.29 vs 0.51 ms).  ngf_debug_set("tile_w" / "split") override for experiments.
    const int waves = threads / kWave;
    const int cus = knob(KNOB_GRID) > 0 && knob(KNOB_GRID) < f->num_cus ? knob(KNOB_GRID) : f->num_cus;      // knob grid (tests): fewer workgroups
    const int64_t resident = (int64_t)cus * waves;      // waves of the persistent grid
    // ---- tile plan -------------------------------------------------------------------------------------------------------------------
    // Wide tiles are the efficient ones (fewer partial shade passes, finer early termination); but the grid is persistent and a launch ends
    // when its LAST wave is done: with one tile width the waves ran dry one tile duration apart -- ~0.17 ms of every launch, 15 % of one
    // rank's 80 000-ray shard (profiles/r04_timeline.txt).  So the ray list is cut into segments of decreasing width: the widest tiles for the
    // bulk, then about `tail` tiles per resident wave of each narrower width down to one ray per tile (a 1-ray tile is ~1/8 of an 8-ray one).
    // A launch with fewer rays than that starts further down the list: a 4096-ray chunk is all 2-ray tiles on 2048 waves.
    // Knobs: tile_w forces ONE width (bit-identity tests, A/B timing); tail = 16 x the narrow tiles per wave and width (0: none).
    int64_t seg_rays[4] = {0, 0, 0, 0};
    int seg_shift[4] = {0, 0, 0, 0};
    int nseg = 1;
    bool split = kernel_split != nullptr;
    if (knob(KNOB_SPLIT) >= 0) split = knob(KNOB_SPLIT) != 0 && kernel_split;
    const int forced = knob(KNOB_TILE_W);
    auto shift_of = [](int w) { int sft = 0; while ((1 << sft) < w) ++sft; return sft; };
    if (forced >= 0 || !split) {
        int tw = forced >= 0 ? forced : 64;
        if (tw != 64 && tw != 32 && tw != 16 && tw != 8 && tw != 4 && tw != 2 && tw != 1) return fail(NGF_E_ARG, "knob tile_w must be 64, 32, 16, 8, 4, 2 or 1");
        if (knob(KNOB_SPLIT) < 0) split = tw < 64 && kernel_split;
        if (tw < 4 && !split) return fail(NGF_E_ARG, "tiles of 2 or 1 rays exist in the split kernel only");
        seg_rays[0] = A.n; seg_shift[0] = shift_of(tw);
    } else {
        nseg = make_tile_plan(A.n, wide_tile, resident, knob(KNOB_TAIL) >= 0 ? knob(KNOB_TAIL) : kTailDefault16, seg_rays, seg_shift);
    }
    // a split kernel whose collect knows the lane patterns of narrow tiles only (TriPlanePolicy::COLLECT3: 8, 4, 2, 1 rays) must never see a wider one: it would
    // add colours into the wrong lanes without any error.  level3_waves16 keeps such launches on the twelve-wave kernel; this is the check behind it.
    if (split)
        for (int k = 0; k < nseg; ++k)
            if (seg_shift[k] > max_split_shift) return fail(NGF_E_ARG, "this kernel renders split tiles of at most %d rays (plan segment %d has %d)", 1 << max_split_shift, k, 1 << seg_shift[k]);
    A.tile_shift = seg_shift[0];
    A.tile_w = 1 << seg_shift[0];
    int64_t tiles = 0, ray0 = 0;
    for (int k = 0; k < 4; ++k) {
        const int sft = k < nseg ? seg_shift[k] : seg_shift[nseg - 1];
        const int64_t r = k < nseg ? seg_rays[k] : 0;
        A.seg_shift[k] = sft;
        A.seg_ray0[k] = ray0;
        tiles += (r + (1 << sft) - 1) >> sft;
        ray0 += r;
        if (k < 3) {
            if (tiles >= ((int64_t)1 << 32)) return fail(NGF_E_ARG, "render launch of %lld tiles: split the ray list", (long long)tiles);
            A.seg_end[k] = (uint32_t)tiles;
        }
    }
    // Screen-space tile order (ngf_field_render_image): the caller declared the list an image of A.ord_tpr (= row_width here) rays per row.  Blocks of
    // 80 rows x 80 pixels measured best on the MLP-stress frames (profiles/r06_r2_locality.txt: R2 -3.8 %, R2 at S = 884 -6.1 %; R1 and InfoInv
    // within 0.6 %); only whole rows of the widest segment take part, the plan's narrow tail keeps the list's order.
    {
        const int64_t row_w = A.ord_tpr;
        A.ord_n = A.ord_tpr = A.ord_bw = A.ord_bh = 0;
        const int sft0 = seg_shift[0];
        if (split && row_w > 0 && (row_w & ((1 << sft0) - 1)) == 0 && (seg_rays[0] >> sft0) < ((int64_t)1 << 31)) {
            const int64_t tpr = row_w >> sft0, rows = seg_rays[0] / row_w;
            int64_t bh = knob(KNOB_ORD_ROWS) > 0 ? knob(KNOB_ORD_ROWS) : 80;
            int64_t bw = (knob(KNOB_ORD_PX) > 0 ? knob(KNOB_ORD_PX) : 80) >> sft0;
            if (bw < 1) bw = 1;
            if (bw > tpr) bw = tpr;
            if (knob(KNOB_ORD_ROWS) != 0 && tpr > bw && rows >= 2 && bh >= 2) {          // knob ord_rows = 0: the list's order
                if (bh > rows) bh = rows;
                A.ord_tpr = (uint32_t)tpr; A.ord_bw = (uint32_t)bw; A.ord_bh = (uint32_t)bh;
                A.ord_n = (uint32_t)((rows / bh) * bh * tpr);
            }
        }
    }
    K k = split ? kernel_split : kernel;
#if defined(NGF_EXP_DUMP) || defined(NGF_EXP_TIMELINE)      // experiment builds: `stats` is the dump / timeline buffer of the production kernel
    if (split && kernel_prod) k = kernel_prod;
#else
    if (split && kernel_prod && !A.dbg_weight && !A.dbg_sigma && !A.stats && !A.skip_rgb && !A.ablate) k = kernel_prod;
#endif
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(k), lds_bytes));
    if (tiles >= ((int64_t)1 << 32)) return fail(NGF_E_ARG, "render launch of %lld tiles: split the ray list", (long long)tiles);
    A.tiles = (uint32_t)tiles;
    // One tile queue per XCD (knob "xcd" = 1) is built, bit-identical and OFF by default: it cuts the fabric traffic of the MLP-stress frame
    // (R2: profiles/r03_triplane_R2_bd_xcd{0,1}_pmc.txt) but not its time -- these launches are bound by the SIMDs' own MFMA + VALU
    // cycles, not by L2 misses (R1 / R2 / InfoInv within +-0.2 %) -- and the march-only frame loses 8 % to the stealing tail
    // (profiles/r03_xcd_queues.txt).
    A.xcd_queues = knob(KNOB_XCD) > 0 ? 8 : 1;
    // One workgroup per CU as long as there are tiles, and only as many working waves per workgroup as the tiles need: a 4096-ray chunk (1024
    // tiles) used to fill 86 CUs with 12 waves each -- three per SIMD, sharing its matrix pipe -- while 170 CUs idled.
    int64_t grid = tiles < f->num_cus ? tiles : f->num_cus;
    if (knob(KNOB_GRID) > 0 && grid > knob(KNOB_GRID)) grid = knob(KNOB_GRID);      // tests: fewer workgroups -> every wave takes many tiles
    if (grid < 1) grid = 1;
    const int64_t per_wg = (tiles + grid - 1) / grid;
    A.waves_active = per_wg < waves ? (int)per_wg : waves;
    A.queue_waves = (uint32_t)grid;          // one report per workgroup (queue_done)
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(threads), lds_bytes, st, A);
    HIP_TRY(hipGetLastError());
    g_last_waves.store(waves, std::memory_order_relaxed);
    return NGF_OK;
}

template <typename P>
static int launch_policy(const ngf_field *f, RenderArgs &A, hipStream_t st)
{
    if constexpr (shared_gauge<P>::value) {
        if (!A.gauge_same) return launch_policy<GaugeAny<P>>(f, A, st);      // gauge planes of unequal sizes: every plane's cell on its own
    }
    const size_t lds = ((size_t)((A.blob_floats + 3) & ~3) + P::WAVES * wave_lds_floats<P>()) * sizeof(float);
    if (lds > 160 * 1024) return fail(NGF_E_ARG, "this waves-per-CU setting needs %zu bytes of LDS (> 160 KiB)", lds);
    constexpr int wide = P::INFOINV ? 16 : 8;          // measured best full-frame tile width (profiles/r01_split_march.txt; InfoInv: 30.3 vs 29.3 Mray/s)
    using KP = decltype(&render_kernel<P, false>);
    constexpr int max_shift = collect3<P>::value ? 3 : 6;          // COLLECT3: the three-lane collect has the lane patterns of tiles of <= 8 rays
    static_assert(!collect3<P>::value || wide <= 8, "the plan's widest tile must be one the three-lane collect knows");
    if constexpr (P::NSTEP == 1 && P::PROD) return launch_render<KP>(render_kernel<P, false>, render_kernel<P, true>, render_kernel<P, true, false>, f, A, P::WAVES * kWave, lds, st, wide, max_shift);
    else if constexpr (P::NSTEP == 1) return launch_render<KP>(render_kernel<P, false>, render_kernel<P, true>, nullptr, f, A, P::WAVES * kWave, lds, st, wide);
    else return launch_render<KP>(render_kernel<P, false>, nullptr, nullptr, f, A, P::WAVES * kWave, lds, st, wide);
}

#ifdef NGF_EXPERIMENTS
// Specialised march / shade waves (ngf_render_pc.hpp): NM march waves + NS shade waves per CU.
template <typename P, int NM, int NS, int TW>
static int launch_pc(const ngf_field *f, RenderArgs &A, hipStream_t st)
{
    if constexpr (shared_gauge<P>::value) {
        if (!A.gauge_same) return launch_pc<GaugeAny<P>, NM, NS, TW>(f, A, st);
    }
    const size_t lds = ((size_t)((A.blob_floats + 3) & ~3) + PcLds<NM>::TOTAL) * sizeof(float);
    if (lds > 160 * 1024) return fail(NGF_E_ARG, "the specialised kernel needs %zu bytes of LDS (> 160 KiB)", lds);
    const unsigned slot = f->next_counter.fetch_add(1) % kCounters;
    A.tile_counter = f->counters + (size_t)slot * kQueueHeads;
    HIP_TRY(hipMemsetAsync(A.tile_counter, 0, kQueueHeads * sizeof(unsigned), st));
    if (int rc = poison_lds(st)) return rc;
    A.xcd_queues = 1;
    A.tile_w = TW;
    A.tile_shift = TW == 8 ? 3 : 2;
    auto k = render_pc_kernel<P, NM, NS, TW>;
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(k), lds));
    const int64_t tiles = (A.n + TW - 1) / TW;
    int64_t grid = (tiles + NM - 1) / NM;
    if (grid > f->num_cus) grid = f->num_cus;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3((NM + NS) * kWave), lds, st, A);
    HIP_TRY(hipMemsetAsync(A.tile_counter, 0, kQueueHeads * sizeof(unsigned), st));      // this kernel does not zero its slot itself (render_kernel does: queue_done)
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}
#endif

// Level 3 at sixteen waves per CU (TriPlanePolicy::W16: four waves per SIMD, 1024-thread workgroups, the pass in 128 registers; DESIGN.md section
// 4.1, profiles/r09_waves16.txt: the 640 000-ray frame 4.239 -> 4.000 ms).  Which kernel a level-3 launch takes is decided here, per launch, like
// gauge_same:
//   - knob waves = 16 / 12 asks for one of them (the tests and the scripts under profiles/ compare the two in one process);
//   - otherwise sixteen waves from kW16MinRaysPerCu rays per CU on.  A short launch is one narrow tile per wave, and four such waves on a SIMD
//     share its matrix pipe where three did: 4 096 rays 0.107 -> 0.129 ms, 20 000 rays 0.239 -> 0.253 ms, 40 000 rays 0.351 -> 0.362 ms with
//     sixteen waves; 80 000 rays (one rank's shard of an eight-GPU frame) 0.605 -> 0.602 ms, 160 000 rays 1.116 -> 1.075 ms;
//   - a field whose MLP image does not leave room for sixteen waves' queues and view tables in the CU's 160 KiB keeps the twelve-wave kernel
//     whatever was asked for -- never an error.  (The level-3 image is 21.3 KiB for every preset -- the baked planes have 64 channels whatever the
//     appearance width -- so today every level-3 field fits: 21.3 + 16 x 8.25 = 153.3 KiB.)
static constexpr int64_t kW16MinRaysPerCu = 312;      // 80 000 rays on 256 CUs: the smallest launch measured at which sixteen waves do not lose
static bool level3_waves16(const ngf_field *f, const RenderArgs &A)
{
    using P = TriPlanePolicy<true, true, 16, 1>;
    static_assert(P::W16 && P::PROD && P::REC12 && P::VLDS && P::VIEW_FOLD, "the sixteen-wave level-3 policy is the production pass");
    const size_t lds = ((size_t)((A.blob_floats + 3) & ~3) + P::WAVES * wave_lds_floats<P>()) * sizeof(float);
    if (lds > 160 * 1024) return false;
    // COLLECT3: the sixteen-wave split kernel keeps a ray's three colour sums in three of its lanes and knows the lane patterns of the plan's widths
    // (8, 4, 2, 1 rays); split tiles of 16 / 32 / 64 rays (the tile_w knob alone makes them) keep the twelve-wave kernel, like a field that does not
    // fit.  (tile_w = 64 without the split knob is the unsplit kernel, one lane per ray and the v_cmpx collect, at either wave count.)
    const int tw = knob(KNOB_TILE_W);
    if (collect3<P>::value && (tw == 16 || tw == 32 || (tw == 64 && knob(KNOB_SPLIT) > 0))) return false;
    if (knob(KNOB_WAVES) >= 0) return knob(KNOB_WAVES) == 16;
    return A.n >= kW16MinRaysPerCu * f->num_cus;
}

// the fused kernel at W waves per CU; a field with an alpha mask takes the instantiation whose march skips empty space (levels 2 and 3)
template <bool BD, bool BC, int W>
static int launch_fused(const ngf_field *f, RenderArgs &A, hipStream_t st)
{
    if constexpr (BD) {
        if (A.mask.coarse) return launch_policy<MaskSkip<TriPlanePolicy<BD, BC, W, 1>>>(f, A, st);
    }
    return launch_policy<TriPlanePolicy<BD, BC, W, 1>>(f, A, st);
}

template <bool BD, bool BC>
static int launch_triplane(const ngf_field *f, RenderArgs &A, hipStream_t st)
{
#ifndef NGF_EXPERIMENTS
    // product library: the fused kernel, one march step per lane, twelve waves per CU (measured best, profiles/r01_sweep.txt) -- level 3: see level3_waves16
    if (knob(KNOB_KERNEL) > 0 || knob(KNOB_STAGE) > 0 || knob(KNOB_PROFILE) > 0 || knob(KNOB_NSTEP) > 1 ||
        (knob(KNOB_WAVES) >= 0 && knob(KNOB_WAVES) != 12 && !(BD && BC && knob(KNOB_WAVES) == 16)))
        return fail(NGF_E_UNSUPPORTED, "knobs kernel / stage / profile / nstep / waves select experiment kernels: load libngf_hip_exp.so (built with -DNGF_EXPERIMENTS)");
    if constexpr (BD && BC) {
        if (level3_waves16(f, A)) return launch_fused<BD, BC, 16>(f, A, st);
    }
    return launch_fused<BD, BC, 12>(f, A, st);
#else
    // default: the fused kernel (every wave marches and shades).  ngf_debug_set("kernel", 1) selects the specialised march / shade
    // waves of ngf_render_pc.hpp: bit-identical, but SLOWER on gfx950 (R1 frame 10.7-12.7 ms vs 10.0 ms, profiles/r02_pc_kernel.txt),
    // because fp32 MFMA and fp32 VALU execute on the same SIMD datapath and never overlap -- not across waves, not within a wave
    // (profiles/micro/mfma_valu_overlap.hip: 8.7 ms + 3.1 ms run together in 11.6 ms) -- so there is nothing for the split to overlap.
    int kernel = knob(KNOB_KERNEL) >= 0 ? knob(KNOB_KERNEL) : 0;
    if (A.dbg_weight || A.skip_rgb || knob(KNOB_NSTEP) > 1 || (knob(KNOB_PROFILE) > 0 && knob(KNOB_KERNEL) != 1)) kernel = 0;
    if (knob(KNOB_TILE_W) > 8 || knob(KNOB_SPLIT) == 0) kernel = 0;
    if (kernel == 1 && knob(KNOB_PROFILE) > 0) {      // section cycles: stats[4..12] (profiles/exp_sections_pc.py); stats must hold 13 counters
        if constexpr (!BC) {
            using PP = TriPlanePolicy<BD, false, 12, 1, true>;
            return knob(KNOB_WAVES) == 88 ? launch_pc<PP, 8, 8, 8>(f, A, st) : launch_pc<PP, 12, 4, 8>(f, A, st);
        }
    }
    if (kernel == 1) {
        using P = TriPlanePolicy<BD, BC, 12, 1>;
        int tw = A.n < 40 * (int64_t)f->num_cus * 12 ? 4 : 8;
        if (knob(KNOB_TILE_W) == 4 || knob(KNOB_TILE_W) == 8) tw = knob(KNOB_TILE_W);
        const int w = knob(KNOB_WAVES) >= 0 ? knob(KNOB_WAVES) : 124;         // experiment: march waves * 10 + shade waves
        switch (w) {
        case 124: return tw == 8 ? launch_pc<P, 12, 4, 8>(f, A, st) : launch_pc<P, 12, 4, 4>(f, A, st);
        case 88: return tw == 8 ? launch_pc<P, 8, 8, 8>(f, A, st) : launch_pc<P, 8, 8, 4>(f, A, st);
        case 84: return tw == 8 ? launch_pc<P, 8, 4, 8>(f, A, st) : launch_pc<P, 8, 4, 4>(f, A, st);
        case 128: return launch_pc<P, 12, 4, 8>(f, A, st);
        default: return fail(NGF_E_ARG, "specialised kernel: knob waves must be 124, 88 or 84");
        }
    }
    // tuning knobs (measurements in profiles/): waves per CU and march steps in flight per lane
    int w = 12, ns = 1;                   // measured best (profiles/r01_sweep.txt)
    if (knob(KNOB_WAVES) >= 0) w = knob(KNOB_WAVES);
    if (knob(KNOB_NSTEP) >= 0) ns = knob(KNOB_NSTEP);
    if (ns == 2) {
        if (w == 8) return launch_policy<TriPlanePolicy<BD, BC, 8, 2>>(f, A, st);
        return fail(NGF_E_ARG, "knob nstep = 2 is built for waves = 8 only");
    }
    if (knob(KNOB_STAGE) > 0 && !A.dbg_weight && !A.skip_rgb) {      // LDS-staged texture strips (ngf_stage.hpp), faithful layout only; stats[13] += staged iterations
        if constexpr (!BD && !BC) {
            if (w == 8) return launch_policy<TriPlaneStagedPolicy<8>>(f, A, st);
            if (w == 12) return launch_policy<TriPlaneStagedPolicy<12>>(f, A, st);
            return fail(NGF_E_ARG, "knob stage: waves must be 8 (gauge + density strips) or 12 (gauge strips)");
        }
    }
    if (knob(KNOB_PROFILE) > 0) {      // stats[4..9] += section cycles (profiles/exp_sections.py); stats must hold 10 counters
        if constexpr (!BC) return launch_policy<TriPlanePolicy<BD, false, 12, 1, true>>(f, A, st);
    }
    if constexpr (BD && BC) {      // level 3: waves = 16 is the 128-register production pass, waves = 12 the twelve-wave one, no knob the product library's choice
        if (w == 12 || w == 16) return level3_waves16(f, A) ? launch_fused<BD, BC, 16>(f, A, st) : launch_fused<BD, BC, 12>(f, A, st);
    }
    switch (w) {
    case 8: return launch_policy<TriPlanePolicy<BD, BC, 8, 1>>(f, A, st);
    case 12: return launch_fused<BD, BC, 12>(f, A, st);
    case 16: return launch_policy<TriPlanePolicy<BD, BC, 16, 1>>(f, A, st);
    default: return fail(NGF_E_ARG, "knob waves must be 8, 12 or 16");
    }
#endif
}

static int render_common(const ngf_field *f, RenderArgs &A, hipStream_t st)
{
    field_use(f, st);
    if (f->model == NGF_MODEL_INFOINV) {
        const bool wide = knob(KNOB_TILE_W) > 16 || knob(KNOB_SPLIT) == 0;      // debug knobs only: launch_render never picks more than 16 rays per tile
        if (f->flags & NGF_F_SPLIT_BF16) {
            if (wide) return fail(NGF_E_ARG, "InfoInv NGF_F_SPLIT_BF16 renders with split tiles of at most 16 rays");
            return A.mask.coarse ? launch_policy<MaskSkip<InfoInvSplitPolicy>>(f, A, st) : launch_policy<InfoInvSplitPolicy>(f, A, st);
        }
        if (wide) return launch_policy<InfoInvWidePolicy>(f, A, st);
        return A.mask.coarse ? launch_policy<MaskSkip<InfoInvPolicy>>(f, A, st) : launch_policy<InfoInvPolicy>(f, A, st);
    }
    if (f->flags & NGF_F_NO_FOLD) return launch_policy<TriPlaneNoFoldPolicy>(f, A, st);
    if ((f->flags & NGF_F_SPLIT_BF16) && (f->flags & NGF_F_BAKE_COLOR)) return A.mask.coarse ? launch_policy<MaskSkip<TriPlaneBakedBf16Policy>>(f, A, st) : launch_policy<TriPlaneBakedBf16Policy>(f, A, st);
    if (f->flags & NGF_F_SPLIT_BF16) {
        if (knob(KNOB_TILE_W) > 8 || knob(KNOB_SPLIT) == 0) return fail(NGF_E_ARG, "NGF_F_SPLIT_BF16 renders with split tiles of 4 or 8 rays");
        // 8 waves per CU: the pass keeps 48 registers of A fragments next to the gather buffer -- at the 168 registers that 12 waves
        // leave it spills 84 and runs 12.8 ms instead of 8.4 ms (profiles/r02_split_bf16.txt)
#ifdef NGF_EXPERIMENTS
        if (knob(KNOB_WAVES) == 12)
            return (f->flags & NGF_F_BAKE_DENSITY) ? launch_policy<TriPlaneBf16Policy<true, 12>>(f, A, st) : launch_policy<TriPlaneBf16Policy<false, 12>>(f, A, st);
#endif
        return (f->flags & NGF_F_BAKE_DENSITY) ? launch_policy<TriPlaneBf16Policy<true, 8>>(f, A, st) : launch_policy<TriPlaneBf16Policy<false, 8>>(f, A, st);
    }
    const bool bd = f->flags & NGF_F_BAKE_DENSITY, bc = f->flags & NGF_F_BAKE_COLOR;
    if (bd) return bc ? launch_triplane<true, true>(f, A, st) : launch_triplane<true, false>(f, A, st);
    return bc ? launch_triplane<false, true>(f, A, st) : launch_triplane<false, false>(f, A, st);
}

extern "C" int ngf_field_render(const ngf_field *f, const float *rays, int64_t n, int32_t n_samples, int32_t white_bg,
                                int32_t mode, const float *jitter, float *rgb, float *depth, uint64_t *stats, void *hip_stream)
{
    if (!f || !rays || !rgb || !depth) return fail(NGF_E_ARG, "ngf_field_render: null argument");
    if (n < 0 || n_samples <= 0) return fail(NGF_E_ARG, "ngf_field_render: n=%lld n_samples=%d", (long long)n, n_samples);
    if (n == 0) return NGF_OK;
    RenderArgs A = f->proto;
    A.rays = rays; A.jitter = jitter; A.rgb = rgb; A.depth = depth; A.n = n; A.S = n_samples;
    A.white_bg = white_bg ? 1 : 0; A.mode = mode ? 1 : 0; A.stats = (unsigned long long *)stats;
    if (knob(KNOB_ABLATE) > 0) A.ablate = knob(KNOB_ABLATE);          // ngf_debug_set("ablate", bits): A/B timing and bit-identity tests only
    return render_common(f, A, (hipStream_t)hip_stream);
}

// ABI 5: ngf_field_render for a ray list that IS an image -- rays [n,6] row-major, row_width rays per image row (the reference's evaluation hands
// `renderer` exactly that: samples.view(-1, 6) of an H x W frame, TriPlane/main.py:88-94).  Same pixels, bit for bit; the launch walks the image in
// screen-space blocks (RenderArgs::ord_*).  row_width <= 0, or a width the tile plan cannot use (not a multiple of the 8-ray tile): ngf_field_render.
extern "C" int ngf_field_render_image(const ngf_field *f, const float *rays, int64_t n, int32_t row_width, int32_t n_samples, int32_t white_bg,
                                      int32_t mode, const float *jitter, float *rgb, float *depth, uint64_t *stats, void *hip_stream)
{
    if (!f || !rays || !rgb || !depth) return fail(NGF_E_ARG, "ngf_field_render_image: null argument");
    if (n < 0 || n_samples <= 0) return fail(NGF_E_ARG, "ngf_field_render_image: n=%lld n_samples=%d", (long long)n, n_samples);
    if (n == 0) return NGF_OK;
    RenderArgs A = f->proto;
    A.rays = rays; A.jitter = jitter; A.rgb = rgb; A.depth = depth; A.n = n; A.S = n_samples;
    A.white_bg = white_bg ? 1 : 0; A.mode = mode ? 1 : 0; A.stats = (unsigned long long *)stats;
    if (knob(KNOB_ABLATE) > 0) A.ablate = knob(KNOB_ABLATE);
    A.ord_tpr = row_width > 0 && (int64_t)row_width < n && f->model == NGF_MODEL_TRIPLANE ? (uint32_t)row_width : 0u;          // launch_render turns the width into the plan (or drops it); InfoInv: the list's order (its kernels do not re-order)
    return render_common(f, A, (hipStream_t)hip_stream);
}

extern "C" int ngf_field_march(const ngf_field *f, const float *rays, int64_t n, int32_t n_samples, int32_t mode,
                               const float *jitter, float *sigma, float *weight, void *hip_stream)
{
    if (!f || !rays || !sigma || !weight) return fail(NGF_E_ARG, "ngf_field_march: null argument");
    if (n <= 0 || n_samples <= 0) return fail(NGF_E_ARG, "ngf_field_march: n=%lld n_samples=%d", (long long)n, n_samples);
    hipStream_t st = (hipStream_t)hip_stream;
    float *scratch = nullptr;
    HIP_TRY(hipMallocAsync((void **)&scratch, (size_t)n * 4 * sizeof(float), st));
    RenderArgs A = f->proto;
    A.rays = rays; A.jitter = jitter; A.rgb = scratch; A.depth = scratch + 3 * n; A.n = n; A.S = n_samples;
    A.white_bg = 0; A.mode = mode ? 1 : 0; A.skip_rgb = 1; A.dbg_sigma = sigma; A.dbg_weight = weight;
    int rc = render_common(f, A, st);
    (void)hipFreeAsync(scratch, st);
    return rc;
}

extern "C" int ngf_field_decode_rgb(const ngf_field *f, const float *coords, const float *dirs, int64_t n, int32_t mode,
                                    float *rgb, void *hip_stream)
{
    if (!f || !coords || !dirs || !rgb) return fail(NGF_E_ARG, "ngf_field_decode_rgb: null argument");
    if (n <= 0) return fail(NGF_E_ARG, "ngf_field_decode_rgb: n=%lld", (long long)n);
    hipStream_t st = (hipStream_t)hip_stream;
    field_use(f, st);
    RenderArgs A = f->proto;
    A.mode = mode ? 1 : 0;
    const size_t lds = ((size_t)((A.blob_floats + 3) & ~3) + 4 * 32 * kViewFeat) * sizeof(float);
    const int64_t nb = (n + 15) / 16;
    int grid = (int)((nb + 3) / 4);
    if (grid > 4 * f->num_cus) grid = 4 * f->num_cus;
    if (int prc = poison_lds(st)) return prc;
    auto go = [&](auto kern) -> int {
        HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, A, coords, dirs, n, rgb);
        return NGF_OK;
    };
    int rc;
    if (f->model == NGF_MODEL_INFOINV) rc = (f->flags & NGF_F_SPLIT_BF16) ? go(decode_rgb_kernel<InfoInvSplitPolicy>) : go(decode_rgb_kernel<InfoInvPolicy>);
    else if (f->flags & NGF_F_NO_FOLD) rc = go(decode_rgb_kernel<TriPlaneNoFoldPolicy>);
    else if ((f->flags & NGF_F_SPLIT_BF16) && (f->flags & NGF_F_BAKE_COLOR)) rc = go(decode_rgb_kernel<TriPlaneBakedBf16Policy>);
    else if (f->flags & NGF_F_SPLIT_BF16) rc = go(decode_rgb_kernel<TriPlaneBf16Policy<false, 8>>);
    else if (f->flags & NGF_F_BAKE_COLOR) rc = go(decode_rgb_kernel<TriPlanePolicy<false, true, 8, 1>>);
    else rc = go(decode_rgb_kernel<TriPlanePolicy<false, false, 8, 1>>);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

static int launch_alpha(const ngf_field *f, const float *xyz, const Lattice &L, int64_t n, int32_t mode, float length, float *alpha, hipStream_t st)
{
    field_use(f, st);
    RenderArgs A = f->proto;
    A.mode = mode ? 1 : 0;
    if (int rc = poison_lds(st)) return rc;
    int64_t grid = (n + 255) / 256;
    if (grid > 8 * (int64_t)f->num_cus) grid = 8 * (int64_t)f->num_cus;
    if (f->model == NGF_MODEL_INFOINV) {
        const size_t lds = (size_t)((A.blob_floats + 3) & ~3) * sizeof(float);
        if (grid > (int64_t)f->num_cus) grid = f->num_cus;
        if (f->flags & NGF_F_SPLIT_BF16) {        // same density MLP, other offset of its image in the LDS blob
            HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(alpha_kernel<InfoInvSplitPolicy>), lds));
            hipLaunchKernelGGL(alpha_kernel<InfoInvSplitPolicy>, dim3((unsigned)grid), dim3(256), lds, st, A, xyz, L, n, length, alpha);
        } else {
            HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(alpha_kernel<InfoInvPolicy>), lds));
            hipLaunchKernelGGL(alpha_kernel<InfoInvPolicy>, dim3((unsigned)grid), dim3(256), lds, st, A, xyz, L, n, length, alpha);
        }
    } else if (f->flags & NGF_F_BAKE_DENSITY) {
        if (A.gauge_same) hipLaunchKernelGGL((alpha_kernel<TriPlanePolicy<true, false, 8, 1>>), dim3((unsigned)grid), dim3(256), 0, st, A, xyz, L, n, length, alpha);
        else hipLaunchKernelGGL((alpha_kernel<GaugeAny<TriPlanePolicy<true, false, 8, 1>>>), dim3((unsigned)grid), dim3(256), 0, st, A, xyz, L, n, length, alpha);
    } else {
        hipLaunchKernelGGL((alpha_kernel<TriPlanePolicy<false, false, 8, 1>>), dim3((unsigned)grid), dim3(256), 0, st, A, xyz, L, n, length, alpha);
    }
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

extern "C" int ngf_field_alpha(const ngf_field *f, const float *xyz, int64_t n, int32_t mode, float length, float *alpha, void *hip_stream)
{
    if (!f || !xyz || !alpha) return fail(NGF_E_ARG, "ngf_field_alpha: null argument");
    if (n < 0) return fail(NGF_E_ARG, "ngf_field_alpha: n=%lld", (long long)n);
    if (n == 0) return NGF_OK;
    return launch_alpha(f, xyz, Lattice{nullptr, nullptr, nullptr, 0, 0, 0}, n, mode, length, alpha, (hipStream_t)hip_stream);
}

// ---- ngf_field_query: density, colour and plane coordinates at world-space points (ngf_query.hpp) ------------------------------------------------
template <typename PD, typename PC>
static int launch_query_kernel(const ngf_field *f, const RenderArgs &A, const QueryArgs &Q, hipStream_t st)
{
    constexpr bool COLOUR = !std::is_same_v<PC, NoColour>;
    const bool staged = COLOUR || (PD::INFOINV && Q.sigma);          // the kernel's own condition: a coords-only InfoInv call stages nothing
    const size_t lds = staged ? ((size_t)((A.blob_floats + 3) & ~3) + (COLOUR ? 4 * kQueryViewFloats : 0)) * sizeof(float) : 0;
    // the grid-stride loop and its cap follow launch_alpha (8 workgroups per CU; one where the MLP image is staged) and, with a colour stage,
    // ngf_field_decode_rgb (4 per CU)
    int64_t grid = (Q.n + 255) / 256;
    const int64_t cap = (COLOUR ? 4 : staged ? 1 : 8) * (int64_t)f->num_cus;
    if (grid > cap) grid = cap;
    if (knob(KNOB_GRID) > 0 && grid > knob(KNOB_GRID)) grid = knob(KNOB_GRID);      // tests: fewer workgroups -> every wave takes many tiles
    if (lds) HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(query_kernel<PD, PC>), lds));
    hipLaunchKernelGGL((query_kernel<PD, PC>), dim3((unsigned)grid), dim3(256), lds, st, A, Q);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

// the colour side as ngf_field_decode_rgb picks it (BD: the handle has NGF_F_BAKE_DENSITY, which NGF_F_NO_FOLD excludes and level 3's bf16 pass requires)
template <typename PD, bool BD>
static int launch_query_triplane(const ngf_field *f, const RenderArgs &A, const QueryArgs &Q, hipStream_t st)
{
    if (!Q.rgb) return launch_query_kernel<PD, NoColour>(f, A, Q, st);
    if constexpr (!BD) {
        if (f->flags & NGF_F_NO_FOLD) return launch_query_kernel<PD, TriPlaneNoFoldPolicy>(f, A, Q, st);
    } else {
        if ((f->flags & NGF_F_SPLIT_BF16) && (f->flags & NGF_F_BAKE_COLOR)) return launch_query_kernel<PD, TriPlaneBakedBf16Policy>(f, A, Q, st);
    }
    if (f->flags & NGF_F_SPLIT_BF16) return launch_query_kernel<PD, TriPlaneBf16Policy<false, 8>>(f, A, Q, st);
    if (f->flags & NGF_F_BAKE_COLOR) return launch_query_kernel<PD, TriPlanePolicy<false, true, 8, 1>>(f, A, Q, st);
    return launch_query_kernel<PD, TriPlanePolicy<false, false, 8, 1>>(f, A, Q, st);
}

extern "C" int ngf_field_query(const ngf_field *f, const float *xyz, int64_t n, int32_t mode, const float *dirs, int32_t dir_stride, int32_t flags,
                               float *sigma, float *rgb, float *coords, void *hip_stream)
{
    if (!f || !xyz) return fail(NGF_E_ARG, "ngf_field_query: null argument");
    if (n < 0) return fail(NGF_E_ARG, "ngf_field_query: n=%lld", (long long)n);
    if (dir_stride != 0 && dir_stride != 3) return fail(NGF_E_ARG, "ngf_field_query: dir_stride=%d (0: one shared direction, 3: one per point)", dir_stride);
    if (flags & ~NGF_QUERY_NO_MASK) return fail(NGF_E_ARG, "ngf_field_query: unknown flags 0x%x", (unsigned)flags);
    if (rgb && !dirs) return fail(NGF_E_ARG, "ngf_field_query: rgb needs dirs");
    if (!sigma && !rgb && !coords) return fail(NGF_E_ARG, "ngf_field_query: no output requested");
    if (n == 0) return NGF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    field_use(f, st);
    RenderArgs A = f->proto;
    A.mode = mode ? 1 : 0;
    const QueryArgs Q{xyz, rgb ? dirs : nullptr, n, dir_stride, (flags & NGF_QUERY_NO_MASK) ? 0 : 1, sigma, rgb, coords};
    if (int rc = poison_lds(st)) return rc;
    // the density side as launch_alpha picks it
    if (f->model == NGF_MODEL_INFOINV) {
        if (f->flags & NGF_F_SPLIT_BF16)
            return rgb ? launch_query_kernel<InfoInvSplitPolicy, InfoInvSplitPolicy>(f, A, Q, st) : launch_query_kernel<InfoInvSplitPolicy, NoColour>(f, A, Q, st);
        return rgb ? launch_query_kernel<InfoInvPolicy, InfoInvPolicy>(f, A, Q, st) : launch_query_kernel<InfoInvPolicy, NoColour>(f, A, Q, st);
    }
    if (f->flags & NGF_F_BAKE_DENSITY) {
        if (A.gauge_same) return launch_query_triplane<TriPlanePolicy<true, false, 8, 1>, true>(f, A, Q, st);
        return launch_query_triplane<GaugeAny<TriPlanePolicy<true, false, 8, 1>>, true>(f, A, Q, st);
    }
    return launch_query_triplane<TriPlanePolicy<false, false, 8, 1>, false>(f, A, Q, st);
}

extern "C" int ngf_field_alpha_mask_build(const ngf_field *f, int32_t mode, const float *sx, const float *sy, const float *sz, int32_t gx, int32_t gy,
                                          int32_t gz, float length, float thres, float *alpha_zyx, float *volume_zyx, float *new_aabb,
                                          uint64_t *count, void *hip_stream)
{
    if (!f || !sx || !sy || !sz || !alpha_zyx || !volume_zyx || !new_aabb || !count) return fail(NGF_E_ARG, "ngf_field_alpha_mask_build: null argument");
    if (gx < 1 || gy < 1 || gz < 1) return fail(NGF_E_ARG, "ngf_field_alpha_mask_build: grid %dx%dx%d", gx, gy, gz);
    hipStream_t st = (hipStream_t)hip_stream;
    const Lattice L{sx, sy, sz, gx, gy, gz};
    const int64_t n = (int64_t)gx * gy * gz;
    int rc = launch_alpha(f, nullptr, L, n, mode, length, alpha_zyx, st);
    if (rc) return rc;
    // index bounds of the occupied voxels: per-call scratch on the call's stream (concurrent builds on one handle do not share it)
    int *bounds = nullptr;
    HIP_TRY(hipMallocAsync((void **)&bounds, 6 * sizeof(int), st));
    hipLaunchKernelGGL(mask_bounds_init_kernel, dim3(1), dim3(64), 0, st, bounds);
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint64_t), st));
    int64_t grid = (n + 255) / 256;
    if (grid > 16 * (int64_t)f->num_cus) grid = 16 * (int64_t)f->num_cus;
    hipLaunchKernelGGL(mask_pool_kernel, dim3((unsigned)grid), dim3(256), 0, st, (const float *)alpha_zyx, gx, gy, gz, thres, volume_zyx, bounds,
                       (unsigned long long *)count);
    hipLaunchKernelGGL(mask_aabb_kernel, dim3(1), dim3(64), 0, st, f->proto, L, (const int *)bounds, new_aabb);
    const hipError_t launch_err = hipGetLastError();
    (void)hipFreeAsync(bounds, st);
    HIP_TRY(launch_err);
    return NGF_OK;
}

extern "C" int ngf_field_ray_filter(const ngf_field *f, const float *rays, int64_t n, int32_t n_samples, uint8_t *keep, void *hip_stream)
{
    if (!f || !rays || !keep) return fail(NGF_E_ARG, "ngf_field_ray_filter: null argument");
    if (n_samples > 0 && !f->proto.mask.bits) return fail(NGF_E_ARG, "ngf_field_ray_filter: the field has no alpha mask");
    if (n < 0) return fail(NGF_E_ARG, "ngf_field_ray_filter: n=%lld", (long long)n);
    if (n == 0) return NGF_OK;
    field_use(f, (hipStream_t)hip_stream);
    RenderArgs A = f->proto;
    int64_t grid = (n + 255) / 256;
    if (grid > 16 * (int64_t)f->num_cus) grid = 16 * (int64_t)f->num_cus;
    hipLaunchKernelGGL(ray_filter_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)hip_stream, A, rays, n, n_samples, keep);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

extern "C" int ngf_generate_rays(int32_t H, int32_t W, float focal, const float *c, int32_t row0, int32_t rows, float *rays,
                                 void *hip_stream)
{
    if (!c || !rays || H <= 0 || W <= 0 || rows < 0 || row0 < 0 || row0 + rows > H) return fail(NGF_E_ARG, "ngf_generate_rays: bad argument");
    if (rows == 0) return NGF_OK;
    const int64_t total = (int64_t)rows * W;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(generate_rays_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, H, W, focal, c[0], c[1], c[2], c[4],
                       c[5], c[6], c[8], c[9], c[10], c[3], c[7], c[11], row0, rows, rays);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

extern "C" int ngf_generate_rays_dtu(int32_t H, int32_t W, const float *focal, const float *princpt, const float *rot, int32_t row0,
                                     int32_t rows, float *raydir, void *hip_stream)
{
    if (!focal || !princpt || !rot || !raydir || H <= 0 || W <= 0 || rows < 0 || row0 < 0 || row0 + rows > H)
        return fail(NGF_E_ARG, "ngf_generate_rays_dtu: bad argument");
    if (rows == 0) return NGF_OK;
    const int64_t total = (int64_t)rows * W;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(generate_rays_dtu_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, W, focal[0], focal[1], princpt[0],
                       princpt[1], rot[0], rot[1], rot[2], rot[3], rot[4], rot[5], rot[6], rot[7], rot[8], row0, rows, raydir);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}
