// ngf_infoinv_train.hpp -- differentiable training-mode forward + backward of the InfoInv field (InfoInv/models/FieldBase.py:228-282 under
// autograd, as the reference's own loop uses it, InfoInv/main.py:262-330).
//
// The model (InfoInv/models/Field.py:43-89, networks.py:12-54): per sample xyz in [-1,1]^3
//   density: f_d[24 p + c] = bilinear(plane_p[c]) * PE(xyz,4)[c]   (c < 24; PE factor 1 when infoinv=False)  -> 72-32-32-1 ReLU MLP -> softplus(. - 10)
//   colour : f_c[72 p + c] = bilinear(plane_p[24 + c]) * PE(xyz,12)[c] (c < 72)  -> basis (216x216) -> [., view, PE(view,2)] 231-64-64-3 ReLU MLP -> sigmoid
// No gauge: no gradient reaches the coordinates, so the chain is: compositing -> per-sample MLPs -> plane features -> bilinear taps.
//
// The pipeline (one thread per sample or per ray, plain fp32 SIMT; the weights are read at wave-uniform addresses, i.e. through the scalar cache):
//   ii_prep_kernel          W1' = W1[:, :216] . basis (fp64 accumulate; the fold of the eval path) and the transposed layer-1 images
//   ii_pack_kernel          planes [96,H,W] -> channel-last [(H+2)(W+2)][96] with a zero border (grid_sample's zeros padding)
//   ii_density_fwd_kernel   every (ray, step) pair: sample_ray + alpha mask + the density MLP; keeps its input / hidden rows
//   ii_scan_kernel          one thread per ray: raw2alpha's cumprod (fp64 product like ATen's CPU cumprod), weights, active counts
//   ii_prefix_kernel        exclusive prefix of the counts; ii_list_kernel the (ray, step)-ordered active list
//   ii_color_fwd_kernel     every active sample: the colour MLP on the folded layer 1; keeps its input / hidden rows
//   ii_composite_fwd_kernel rgb_map (+ white background, clamp) and depth_map per ray
// backward (d loss / d rgb_map in):
//   ii_composite_bwd_kernel the clamp, then per ray from the END: the closed-form cumprod backward -> d loss / d (pre-softplus density), d colour
//   ii_color_bwd_kernel     the colour MLP's data gradients; d loss / d colour plane feature = W1'^T . Delta1 (x PE)
//   ii_density_bwd_kernel   the density MLP's data gradients; d loss / d density plane feature (x PE)
//   ii_bound_* / ii_scatter_kernel  the plane gradients: every tap adds w * g as a 64-bit FIXED-POINT integer (scale 2^k chosen on the device from
//                           sum |g|, so no sum can overflow): integer addition is associative, so the sums do not depend on the order the atomics
//                           land in and two backwards of one batch give bit-identical gradients
//   ii_xty_kernel / ii_xty_reduce_kernel  weight + bias gradients as sample-reduction GEMMs dW = Delta^T . In over fixed row chunks, fp64
//                           accumulation, chunks summed in chunk order (deterministic; the density bias sums millions of cancelling terms)
//   ii_unfold_kernel        M = Delta1^T [f, view]  ->  dW1[:, :216] = M . basis^T,  d basis = W1[:, :216]^T . M
//
// Row buffers are feature-major: row k of sample s lives at buf[k * cap + s] (coalesced stores by the per-sample kernels, coalesced slabs for the GEMMs).
#pragma once
#include "ngf_device.hpp"

namespace ngf {

constexpr int kIiC = 96, kIiDens = 24, kIiCol = 72;
constexpr int kIiDIn = 72, kIiDH = 32;                 // density MLP 72-32-32-1
constexpr int kIiCF = 216, kIiCIn = 231, kIiCH = 64;   // colour: 216 plane features (+15 view inputs) -> 64 -> 64 -> 3
constexpr int kIiChunk = 4096;                         // rows per GEMM chunk
constexpr int kIiBoundBlocks = 512;

struct IiArgs {
    const float *rays, *jitter;       // [n,6], [n] (NULL = 0)
    int64_t n;
    int32_t S, white_bg, infoinv;
    float a0[3], a1[3], inv[3];
    float near_, far_, step, dscale, thr;
    const uint8_t *mask_bits;         // np.packbits image of [D,H,W] or NULL
    int32_t mD, mH, mW;
    float m_a0[3], m_inv[3];
    Tex tex[3];                       // packed planes: channel-last, 96 channels, one-texel zero border
    // parameters (reference layouts)
    const float *dw1, *db1, *dw2, *db2, *dw3, *db3;    // density_decoder.mlp.{0,2,4}
    const float *basis, *w1, *b1, *w2, *b2, *w3, *b3;  // rgb_decoder
    const float *dw1t;                // [72][32]  density W1^T
    const float *cw1t;                // [231][64] rows 0..215 = (W1[:, :216] . basis)^T, rows 216..230 = the view columns of W1, transposed
    // per-pair buffers (index r * S + i), cap_pairs = max_rays * max_samples
    int64_t cap;
    float *et, *sg, *w, *tb, *dxs;    // exp(-sigma dist), softplus'(xs) (0: invalid), weight, transmittance before the sample, d loss / d xs
    float *xn;                        // [3][cap] normalised position
    uint8_t *valid;                   // [cap]
    float *d_in, *d_h1, *d_h2;        // [72|32|32][cap]
    float *d_d1, *d_d2;               // [32][cap] backward deltas (pre-activation)
    float *d_g;                       // [72][cap] d loss / d density plane feature (PE applied): what the taps scatter
    // active list
    int32_t *count, *offset;          // [n], [n+1]
    int32_t *list;                    // [cap] r * S + i
    float *c_in, *c_h1, *c_h2, *c_rgb;                 // [231|64|64|3][cap]
    float *c_d1, *c_d2, *c_d3;                         // [64|64|3][cap]
    float *c_g;                       // [216][cap]
    float *pre;                       // [n,3] rgb_map before the clamp
    float *rgb_out, *depth_out;       // [n,3], [n]
    const float *d_rgb;               // [n,3]
    unsigned long long *gacc[3];      // [(H+2)(W+2)][96] fixed-point plane gradients
    double *bound;                    // [kIiBoundBlocks + 1]: partial sums of |g|, then [kIiBoundBlocks] = the scale
};

// ---- geometry: Base.sample_ray + alpha mask + normalize_coord (InfoInv/models/FieldBase.py:118-135, 237-249) ----------------------
__device__ __forceinline__ bool ii_mask(const IiArgs &A, const float p[3])
{
    // sign of F.grid_sample(alpha_volume, ., align_corners=True) on a {0,1} volume (FieldBase.py:33-40): > 0 iff a set corner has a positive weight
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = (p[k] - A.m_a0[k]) * A.m_inv[k] - 1.0f;
    const float ix = ((q[0] + 1.0f) / 2.0f) * (float)(A.mW - 1), iy = ((q[1] + 1.0f) / 2.0f) * (float)(A.mH - 1),
                iz = ((q[2] + 1.0f) / 2.0f) * (float)(A.mD - 1);
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    if (!(fx >= -1.0f && fx <= (float)(A.mW - 1) && fy >= -1.0f && fy <= (float)(A.mH - 1) && fz >= -1.0f && fz <= (float)(A.mD - 1))) return false;
    const float wx[2] = {(fx + 1.0f) - ix, ix - fx}, wy[2] = {(fy + 1.0f) - iy, iy - fy}, wz[2] = {(fz + 1.0f) - iz, iz - fz};
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    float acc = 0.0f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = x0 + dx, y = y0 + dy, z = z0 + dz;
                if (x < 0 || y < 0 || z < 0 || x >= A.mW || y >= A.mH || z >= A.mD) continue;
                const size_t idx = ((size_t)z * A.mH + y) * A.mW + x;
                if ((A.mask_bits[idx >> 3] >> (7 - (int)(idx & 7))) & 1) acc += wx[dx] * wy[dy] * wz[dz];
            }
    return acc > 0.0f;
}

__device__ __forceinline__ float ii_tmin(const IiArgs &A, int64_t r)
{
    float tmin = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float o = A.rays[r * 6 + k], d = A.rays[r * 6 + 3 + k];
        const float vec = (d == 0.0f) ? 1e-6f : d;
        const float ra = (A.a1[k] - o) / vec, rb = (A.a0[k] - o) / vec;
        tmin = fmaxf(tmin, fminf(ra, rb));
    }
    return fminf(fmaxf(tmin, A.near_), A.far_);
}

__device__ __forceinline__ float ii_z(const IiArgs &A, float tmin, float jit, int i) { return tmin + A.step * ((float)i + jit); }

// sin / cos (x 2^f), the positional_encoding of networks.py:257-268: channel c of PE(xyz, F) is sin of axis c / F at octave c % F for c < 3F, cos after
__device__ __forceinline__ float ii_pe(const float x[3], int c, int F)
{
    const int s = c < 3 * F ? 0 : 1;
    const int cc = c - s * 3 * F;
    const int ax = cc / F, oct = cc - ax * F;
    const float xa = ax == 0 ? x[0] : (ax == 1 ? x[1] : x[2]);
    const float a = xa * (float)(1 << oct);            // exact: a power of two
    return s ? cosf(a) : sinf(a);
}

// plane coordinates of transform() (Field.py:52-58): xy, yz, xz
__device__ __forceinline__ void ii_uv(const float x[3], int p, float &u, float &v)
{
    u = p == 2 ? x[0] : x[p];
    v = p == 0 ? x[1] : x[2];
}

// ---- 0. weight images ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ii_prep_kernel(const IiArgs A, float *dw1t, float *cw1t)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < kIiDIn * kIiDH) {
        const int k = t / kIiDH, j = t - k * kIiDH;
        dw1t[t] = A.dw1[j * kIiDIn + k];
    }
    if (t < kIiCIn * kIiCH) {
        const int k = t / kIiCH, j = t - k * kIiCH;
        if (k < kIiCF) {
            double s = 0.0;
            for (int i = 0; i < kIiCF; ++i) s += (double)A.w1[j * kIiCIn + i] * (double)A.basis[i * kIiCF + k];
            cw1t[t] = (float)s;
        } else {
            cw1t[t] = A.w1[j * kIiCIn + k];
        }
    }
}

// planes [96][H][W] -> [(H+2)][(W+2)][96], border zero
__global__ void __launch_bounds__(256) ii_pack_kernel(const float *src, int H, int W, float *dst)
{
    const int64_t total = (int64_t)(H + 2) * (W + 2) * kIiC;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % kIiC);
        const int64_t tex = e / kIiC;
        const int x = (int)(tex % (W + 2)) - 1, y = (int)(tex / (W + 2)) - 1;
        dst[e] = (x >= 0 && y >= 0 && x < W && y < H) ? src[((int64_t)c * H + y) * W + x] : 0.0f;
    }
}

// ---- 1. density forward over every (ray, step) pair ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ii_density_fwd_kernel(const IiArgs A)
{
    const int64_t total = A.n * A.S;
    const int64_t cap = A.cap;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = idx / A.S;
        const int i = (int)(idx - r * A.S);
        const float tmin = ii_tmin(A, r);
        const float jit = A.jitter ? A.jitter[r] : 0.0f;
        const float z = ii_z(A, tmin, jit, i);
        const float zn = ii_z(A, tmin, jit, i + 1);
        const float dist = (i < A.S - 1) ? (zn - z) : 0.0f;
        float p[3], x[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = A.rays[r * 6 + k] + A.rays[r * 6 + 3 + k] * z;
            ok = ok & !((A.a0[k] > p[k]) | (p[k] > A.a1[k]));
        }
        if (A.mask_bits && ok) ok = ii_mask(A, p);
#pragma unroll
        for (int k = 0; k < 3; ++k) { x[k] = (p[k] - A.a0[k]) * A.inv[k] - 1.0f; A.xn[k * cap + idx] = x[k]; }
        A.valid[idx] = ok ? 1 : 0;
        if (!ok) {
            A.et[idx] = 1.0f;
            A.sg[idx] = 0.0f;
#pragma unroll 8
            for (int k = 0; k < kIiDIn; ++k) A.d_in[k * cap + idx] = 0.0f;
#pragma unroll
            for (int j = 0; j < kIiDH; ++j) { A.d_h1[j * cap + idx] = 0.0f; A.d_h2[j * cap + idx] = 0.0f; }
            continue;
        }
        float h[kIiDH];
#pragma unroll
        for (int j = 0; j < kIiDH; ++j) h[j] = 0.0f;
        Bil b[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) { float u, v; ii_uv(x, q, u, v); b[q] = bil_setup(u, v, A.tex[q]); }
#pragma unroll 1
        for (int c = 0; c < kIiDens; ++c) {
            const float pe = A.infoinv ? ii_pe(x, c, 4) : 1.0f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const Tex &t = A.tex[q];
                const float *s = t.p + (size_t)b[q].idx * kIiC + c;
                const float f = bil_mix(b[q], s[0], s[kIiC], s[(size_t)t.stride * kIiC], s[((size_t)t.stride + 1) * kIiC]) * pe;
                const int k = q * kIiDens + c;
                A.d_in[k * cap + idx] = f;
                const float *wr = A.dw1t + k * kIiDH;
#pragma unroll
                for (int j = 0; j < kIiDH; ++j) h[j] = fmaf(wr[j], f, h[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < kIiDH; ++j) { h[j] = fmaxf(h[j] + A.db1[j], 0.0f); A.d_h1[j * cap + idx] = h[j]; }
        float o = 0.0f;
#pragma unroll
        for (int j = 0; j < kIiDH; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < kIiDH; ++k) s = fmaf(A.dw2[j * kIiDH + k], h[k], s);
            s = fmaxf(s + A.db2[j], 0.0f);
            A.d_h2[j * cap + idx] = s;
            o = fmaf(A.dw3[j], s, o);
        }
        o = o + A.db3[0];
        const float u = o + (-10.0f);
        A.et[idx] = expf(-softplus_shift(o) * (dist * A.dscale));
        const float e = expf(u);
        A.sg[idx] = u > 20.0f ? 1.0f : e / (e + 1.0f);          // ATen's softplus backward: z / (z + 1), z = exp(u)
    }
}

// ---- 2. raw2alpha per ray (FieldBase.py:12-19): the cumprod in fp64 like ATen's CPU kernel; weights, T_i, active counts ------------
__global__ void __launch_bounds__(256) ii_scan_kernel(const IiArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    double T = 1.0;
    int cnt = 0;
    for (int i = 0; i < A.S; ++i) {
        const int64_t idx = r * A.S + i;
        const float a = 1.0f - A.et[idx];
        const float Ti = (float)T;
        const float w = a * Ti;
        A.w[idx] = w;
        A.tb[idx] = Ti;
        cnt += w > A.thr ? 1 : 0;
        T *= (double)((1.0f - a) + 1e-10f);
    }
    A.count[r] = cnt;
}

__global__ void __launch_bounds__(1024) ii_prefix_kernel(const int32_t *count, int64_t n, int32_t *offset)
{
    __shared__ int32_t sh[1024];
    const int32_t total = block_scan_runs(count, n, offset, sh);
    if (threadIdx.x == 1023) offset[n] = total;
}

__global__ void __launch_bounds__(256) ii_list_kernel(const IiArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    int32_t o = A.offset[r];
    for (int i = 0; i < A.S; ++i) {
        const int64_t idx = r * A.S + i;
        if (A.w[idx] > A.thr) A.list[o++] = (int32_t)idx;
    }
}

// ---- 3. colour forward over the active list ------------------------------------------------------------------------------------
__device__ __forceinline__ void ii_view(const float d[3], float v[15])
{
    // [view_dirs, positional_encoding(view_dirs, 2)] (networks.py:24-28)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = d[k];
        v[3 + 2 * k] = sinf(d[k]); v[4 + 2 * k] = sinf(d[k] * 2.0f);
        v[9 + 2 * k] = cosf(d[k]); v[10 + 2 * k] = cosf(d[k] * 2.0f);
    }
}

__global__ void __launch_bounds__(256) ii_color_fwd_kernel(const IiArgs A)
{
    const int64_t cap = A.cap;
    const int64_t na = A.offset[A.n];
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < na; a += (int64_t)gridDim.x * blockDim.x) {
        const int64_t idx = A.list[a];
        const int64_t r = idx / A.S;
        float x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = A.xn[k * cap + idx];
        float h[kIiCH];
#pragma unroll
        for (int j = 0; j < kIiCH; ++j) h[j] = 0.0f;
        Bil b[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) { float u, v; ii_uv(x, q, u, v); b[q] = bil_setup(u, v, A.tex[q]); }
#pragma unroll 1
        for (int c = 0; c < kIiCol; ++c) {
            const float pe = A.infoinv ? ii_pe(x, c, 12) : 1.0f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const Tex &t = A.tex[q];
                const float *s = t.p + (size_t)b[q].idx * kIiC + kIiDens + c;
                const float f = bil_mix(b[q], s[0], s[kIiC], s[(size_t)t.stride * kIiC], s[((size_t)t.stride + 1) * kIiC]) * pe;
                const int k = q * kIiCol + c;
                A.c_in[k * cap + a] = f;
                const float *wr = A.cw1t + k * kIiCH;
#pragma unroll
                for (int j = 0; j < kIiCH; ++j) h[j] = fmaf(wr[j], f, h[j]);
            }
        }
        float d[3], v[15];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = A.rays[r * 6 + 3 + k];
        ii_view(d, v);
#pragma unroll
        for (int q = 0; q < 15; ++q) {
            A.c_in[(kIiCF + q) * cap + a] = v[q];
            const float *wr = A.cw1t + (kIiCF + q) * kIiCH;
#pragma unroll
            for (int j = 0; j < kIiCH; ++j) h[j] = fmaf(wr[j], v[q], h[j]);
        }
#pragma unroll
        for (int j = 0; j < kIiCH; ++j) { h[j] = fmaxf(h[j] + A.b1[j], 0.0f); A.c_h1[j * cap + a] = h[j]; }
        float o[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int j = 0; j < kIiCH; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < kIiCH; ++k) s = fmaf(A.w2[j * kIiCH + k], h[k], s);
            s = fmaxf(s + A.b2[j], 0.0f);
            A.c_h2[j * cap + a] = s;
#pragma unroll
            for (int m = 0; m < 3; ++m) o[m] = fmaf(A.w3[m * kIiCH + j], s, o[m]);
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) A.c_rgb[m * cap + a] = 1.0f / (1.0f + expf(-(o[m] + A.b3[m])));
    }
}

// ---- 4. compositing (FieldBase.py:261-279) ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ii_composite_fwd_kernel(const IiArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const int64_t cap = A.cap;
    const float tmin = ii_tmin(A, r);
    const float jit = A.jitter ? A.jitter[r] : 0.0f;
    float acc = 0.0f, dep = 0.0f, rgb[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < A.S; ++i) {
        const float w = A.w[r * A.S + i];
        acc += w;
        dep += w * ii_z(A, tmin, jit, i);
    }
    for (int32_t a = A.offset[r]; a < A.offset[r + 1]; ++a) {
        const float w = A.w[A.list[a]];
#pragma unroll
        for (int m = 0; m < 3; ++m) rgb[m] += w * A.c_rgb[m * cap + a];
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const float v = A.white_bg ? rgb[m] + (1.0f - acc) : rgb[m];
        A.pre[r * 3 + m] = v;
        A.rgb_out[r * 3 + m] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
    A.depth_out[r] = dep + (1.0f - acc) * A.rays[r * 6 + 5];
}

// ---- 5. compositing backward: clamp, d w, the closed-form cumprod backward, d xs and d colour ------------------------------------
// d alpha_i = dw_i T_i - S_{i+1} / (1 - alpha_i + 1e-10),  S_m = sum_{k >= m} (dw_k alpha_k) T_k  (ATen: cumprod backward = reversed cumsum of
// grad * output / input for inputs without zeros; the reversed cumsum accumulates in fp64 on the CPU)
__global__ void __launch_bounds__(256) ii_composite_bwd_kernel(const IiArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const int64_t cap = A.cap;
    float G[3];
    float gs = 0.0f;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const float v = A.pre[r * 3 + m];
        G[m] = (v >= 0.0f && v <= 1.0f) ? A.d_rgb[r * 3 + m] : 0.0f;        // clamp backward: the gradient passes where min <= x <= max
        gs += G[m];
    }
    const float tmin = ii_tmin(A, r);
    const float jit = A.jitter ? A.jitter[r] : 0.0f;
    double suf = 0.0;
    int32_t a = A.offset[r + 1] - 1;
    const int32_t a0 = A.offset[r];
    for (int i = A.S - 1; i >= 0; --i) {
        const int64_t idx = r * A.S + i;
        const float w = A.w[idx];
        float dw = A.white_bg ? -gs : 0.0f;                 // d rgb_map / d acc_map = -1 per channel with the white background
        if (a >= a0 && A.list[a] == idx) {
            float cg = 0.0f;
#pragma unroll
            for (int m = 0; m < 3; ++m) { cg += G[m] * A.c_rgb[m * cap + a]; A.c_d3[m * cap + a] = w * G[m]; }       // d colour (sigmoid applied in ii_color_bwd)
            dw = cg + dw;
            --a;
        }
        const float alpha = 1.0f - A.et[idx];
        const float Ti = A.tb[idx];
        const float sfx = (float)suf;                        // S_{i+1}
        const float dalpha = dw * Ti - sfx / ((1.0f - alpha) + 1e-10f);
        suf += (double)((dw * alpha) * Ti);
        const float dd = (i < A.S - 1) ? (ii_z(A, tmin, jit, i + 1) - ii_z(A, tmin, jit, i)) * A.dscale : 0.0f;
        A.dxs[idx] = A.sg[idx] == 0.0f ? 0.0f : ((dalpha * A.et[idx]) * dd) * A.sg[idx];
    }
}

// ---- 6. colour backward over the active list -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ii_color_bwd_kernel(const IiArgs A)
{
    const int64_t cap = A.cap;
    const int64_t na = A.offset[A.n];
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < na; a += (int64_t)gridDim.x * blockDim.x) {
        const int64_t idx = A.list[a];
        float d3[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float y = A.c_rgb[m * cap + a];
            d3[m] = A.c_d3[m * cap + a] * ((1.0f - y) * y);
            A.c_d3[m * cap + a] = d3[m];
        }
        // d h1 = W2^T . Delta2 accumulated one hidden unit of layer 2 at a time (the 64 accumulators stay in registers)
        float d1[kIiCH];
#pragma unroll
        for (int k = 0; k < kIiCH; ++k) d1[k] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < kIiCH; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int m = 0; m < 3; ++m) s = fmaf(A.w3[m * kIiCH + j], d3[m], s);
            const float d2 = A.c_h2[j * cap + a] > 0.0f ? s : 0.0f;
            A.c_d2[j * cap + a] = d2;
            const float *wr = A.w2 + j * kIiCH;
#pragma unroll
            for (int k = 0; k < kIiCH; ++k) d1[k] = fmaf(wr[k], d2, d1[k]);
        }
#pragma unroll
        for (int k = 0; k < kIiCH; ++k) {
            d1[k] = A.c_h1[k * cap + a] > 0.0f ? d1[k] : 0.0f;
            A.c_d1[k * cap + a] = d1[k];
        }
        float x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = A.xn[k * cap + idx];
#pragma unroll 1
        for (int c = 0; c < kIiCol; ++c) {
            const float pe = A.infoinv ? ii_pe(x, c, 12) : 1.0f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int k = q * kIiCol + c;
                const float *wr = A.cw1t + k * kIiCH;
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < kIiCH; ++j) s = fmaf(wr[j], d1[j], s);
                A.c_g[k * cap + a] = s * pe;
            }
        }
    }
}

// ---- 7. density backward over every valid pair --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ii_density_bwd_kernel(const IiArgs A)
{
    const int64_t total = A.n * A.S;
    const int64_t cap = A.cap;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const float g = A.dxs[idx];
        if (!A.valid[idx]) {
#pragma unroll
            for (int j = 0; j < kIiDH; ++j) { A.d_d1[j * cap + idx] = 0.0f; A.d_d2[j * cap + idx] = 0.0f; }
#pragma unroll 8
            for (int k = 0; k < kIiDIn; ++k) A.d_g[k * cap + idx] = 0.0f;
            continue;
        }
        float d2[kIiDH];
#pragma unroll
        for (int j = 0; j < kIiDH; ++j) {
            d2[j] = A.d_h2[j * cap + idx] > 0.0f ? A.dw3[j] * g : 0.0f;
            A.d_d2[j * cap + idx] = d2[j];
        }
        float d1[kIiDH];
#pragma unroll
        for (int k = 0; k < kIiDH; ++k) {
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < kIiDH; ++j) s = fmaf(A.dw2[j * kIiDH + k], d2[j], s);
            d1[k] = A.d_h1[k * cap + idx] > 0.0f ? s : 0.0f;
            A.d_d1[k * cap + idx] = d1[k];
        }
        float x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = A.xn[k * cap + idx];
#pragma unroll 1
        for (int c = 0; c < kIiDens; ++c) {
            const float pe = A.infoinv ? ii_pe(x, c, 4) : 1.0f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int k = q * kIiDens + c;
                const float *wr = A.dw1t + k * kIiDH;
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < kIiDH; ++j) s = fmaf(wr[j], d1[j], s);
                A.d_g[k * cap + idx] = s * pe;
            }
        }
    }
}

// ---- 8. plane gradients: fixed-point scatter ------------------------------------------------------------------------------------------
// sum |g| over every (sample, feature) of both paths -> an upper bound of |any texel's sum| (the four tap weights of a cell add up to <= 1)
__global__ void __launch_bounds__(256) ii_bound_kernel(const IiArgs A)
{
    __shared__ double part[256];
    const int64_t total_d = A.n * A.S, na = A.offset[A.n];
    double s = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total_d * kIiDIn; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / total_d, idx = e - k * total_d;
        s += fabs((double)A.d_g[k * A.cap + idx]);
    }
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < na * kIiCF; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / na, a = e - k * na;
        s += fabs((double)A.c_g[k * A.cap + a]);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) A.bound[blockIdx.x] = part[0];
}

__global__ void __launch_bounds__(64) ii_scale_kernel(const IiArgs A)
{
    if (threadIdx.x != 0) return;
    double b = 0.0;
    for (int k = 0; k < kIiBoundBlocks; ++k) b += A.bound[k];
    // the largest 2^e with b * 2^e <= 2^61 (a margin of 2 bits below int64's range for the per-term rounding); 2^0 when there is nothing to add.
    // A non-finite b (an inf / NaN feature gradient) gives a NaN scale: the scatter then adds nothing and every plane gradient comes out NaN,
    // as the non-finite value would have made them under autograd -- never a silently wrapped integer.
    double sc = 1.0;
    if (!(b < INFINITY)) {
        sc = __builtin_nan("");
    } else if (b > 0.0) {
        int e;
        frexp(b, &e);                    // b < 2^e
        sc = ldexp(1.0, 61 - e);
    }
    A.bound[kIiBoundBlocks] = sc;
}

__device__ __forceinline__ void ii_tap_add(unsigned long long *g, float w, float v, double sc)
{
    if (w == 0.0f) return;
    const long long q = llrint((double)w * (double)v * sc);
    if (q != 0) atomicAdd(g, (unsigned long long)q);
}

// one thread per (sample, feature): the four taps of its cell; DENS = density features of a pair, else colour features of an active sample
template <bool DENS>
__global__ void __launch_bounds__(256) ii_scatter_kernel(const IiArgs A)
{
    constexpr int NF = DENS ? kIiDIn : kIiCF;
    constexpr int PC = DENS ? kIiDens : kIiCol;
    const int64_t rows = DENS ? A.n * A.S : (int64_t)A.offset[A.n];
    const double sc = A.bound[kIiBoundBlocks];
    if (!(sc == sc)) return;                 // non-finite gradients: ii_plane_grad_kernel writes NaN planes
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < rows * NF; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / NF;
        const int k = (int)(e - row * NF);
        const int64_t idx = DENS ? row : (int64_t)A.list[row];
        if (DENS && !A.valid[idx]) continue;
        const float v = DENS ? A.d_g[(int64_t)k * A.cap + row] : A.c_g[(int64_t)k * A.cap + row];
        if (v == 0.0f) continue;
        const int q = k / PC, c = (DENS ? 0 : kIiDens) + (k - q * PC);
        float x[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) x[j] = A.xn[j * A.cap + idx];
        float u, vv;
        ii_uv(x, q, u, vv);
        const Tex &t = A.tex[q];
        const Bil b = bil_setup(u, vv, t);
        unsigned long long *g = A.gacc[q] + (size_t)b.idx * kIiC + c;
        ii_tap_add(g, b.w00, v, sc);
        ii_tap_add(g + kIiC, b.w10, v, sc);
        ii_tap_add(g + (size_t)t.stride * kIiC, b.w01, v, sc);
        ii_tap_add(g + ((size_t)t.stride + 1) * kIiC, b.w11, v, sc);
    }
}

// fixed point -> the reference layout [96][H][W]
__global__ void __launch_bounds__(256) ii_plane_grad_kernel(const unsigned long long *gacc, const double *bound, int H, int W, float *out)
{
    const double inv = 1.0 / bound[kIiBoundBlocks];      // NaN scale (non-finite gradients) -> NaN everywhere
    const int64_t total = (int64_t)kIiC * H * W;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % W);
        const int64_t t = e / W;
        const int y = (int)(t % H), c = (int)(t / H);
        const long long q = (long long)gacc[((size_t)(y + 1) * (W + 2) + (x + 1)) * kIiC + c];
        out[e] = (float)((double)q * inv);
    }
}

// ---- 9. weight gradients: part[chunk][m][n] = sum over the chunk's rows of X[m][row] * Y[n][row]  (column N = 1: the bias) ---------------
// 256 threads own a 32 x 32 output tile (4 outputs each), rows go through LDS 64 at a time; fp64 accumulation.  rows_dev != NULL: the row
// count is min(rows, *rows_dev) (the active count, read on the device).
struct IiXty {
    const float *X, *Y;
    int64_t ld;                   // row stride of both (the buffers' capacity)
    int64_t rows;
    const int32_t *rows_dev;
    int M, N, NB;                 // NB = N + 1 (bias column)
    double *part;                 // [chunks][M][NB]
};

__global__ void __launch_bounds__(256) ii_xty_kernel(const IiXty G)
{
    __shared__ float xs[64][33];
    __shared__ float ys[64][33];
    const int64_t rows = G.rows_dev ? min(G.rows, (int64_t)*G.rows_dev) : G.rows;          // never past the launch, as ii_mm_kernel
    const int tiles_n = (G.NB + 31) / 32;
    const int tm = blockIdx.y / tiles_n, tn = blockIdx.y - tm * tiles_n;
    const int64_t r0 = (int64_t)blockIdx.x * kIiChunk;
    const int t = threadIdx.x;
    const int n = t & 31, mq = (t >> 5) * 4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t rb = r0; rb < r0 + kIiChunk && rb < rows; rb += 64) {
        // stage: 64 rows x 32 columns of X and of Y (8 elements of each per thread); element (k, row): k = e >> 6, row = e & 63
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = t + 256 * u;
            const int k = e >> 6, rr = e & 63;
            const int64_t row = rb + rr;
            const int m = tm * 32 + k, nn = tn * 32 + k;
            const bool rin = row < rows;
            xs[rr][k] = (rin && m < G.M) ? G.X[(int64_t)m * G.ld + row] : 0.0f;
            ys[rr][k] = (rin && nn < G.N) ? G.Y[(int64_t)nn * G.ld + row] : ((rin && nn == G.N) ? 1.0f : 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < 64; ++rr) {
            const double y = (double)ys[rr][n];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (double)xs[rr][mq + j] * y;
        }
        __syncthreads();
    }
    const int nn = tn * 32 + n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = tm * 32 + mq + j;
        if (m < G.M && nn < G.NB) G.part[((int64_t)blockIdx.x * G.M + m) * G.NB + nn] = acc[j];
    }
}

// sum of the chunks in chunk order -> weight gradient [M][N] (float), bias gradient [M] (float), and optionally the fp64 matrix
__global__ void __launch_bounds__(256) ii_xty_reduce_kernel(const double *part, int chunks, int M, int N, float *gw, float *gb, double *gw64)
{
    const int NB = N + 1;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M * NB) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * M * NB + e];
    const int m = e / NB, n = e - m * NB;
    if (n == N) { if (gb) gb[m] = (float)s; }
    else {
        if (gw) gw[m * N + n] = (float)s;
        if (gw64) gw64[m * N + n] = s;
    }
}

// M [64][231] (fp64) -> dW1 [64][231] = [M[:, :216] . basis^T | M[:, 216:]],  d basis [216][216] = W1[:, :216]^T . M[:, :216]
__global__ void __launch_bounds__(256) ii_unfold_kernel(const double *Mm, const float *basis, const float *w1, float *g_w1, float *g_basis)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (g_w1 && e < kIiCH * kIiCIn) {
        const int j = e / kIiCIn, i = e - j * kIiCIn;
        double s = 0.0;
        if (i < kIiCF) {
            for (int k = 0; k < kIiCF; ++k) s += Mm[j * kIiCIn + k] * (double)basis[i * kIiCF + k];
        } else {
            s = Mm[j * kIiCIn + i];
        }
        g_w1[e] = (float)s;
    }
    if (g_basis && e < kIiCF * kIiCF) {
        const int i = e / kIiCF, k = e - i * kIiCF;
        double s = 0.0;
        for (int j = 0; j < kIiCH; ++j) s += (double)w1[j * kIiCIn + i] * Mm[j * kIiCIn + k];
        g_basis[e] = (float)s;
    }
}

}  // namespace ngf
