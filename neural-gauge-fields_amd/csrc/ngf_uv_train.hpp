// ngf_uv_train.hpp -- the differentiable UV-Mapping (NeuTex) forward and its backward on gfx950 (UV-Mapping/model/model.py:27-59,
// renderer.py:79-247, decoder.py:11-78,201-237, gauge_fields.py:8-74); host side in ngf_uv_train.hip.
//
// Layer-wise: every Linear of the three MLPs is one launch of uvt_gemm_kernel, an LDS-tiled GEMM on v_mfma_f32_16x16x4_f32 (exact fp32,
// 64 x 64 block tile, four waves of 32 x 32) with a fused epilogue: bias + activation in the forward, "+ second gradient, x activation
// derivative" in the backward.  The gauge network runs on every sample (uv is an output); the geometry and texture networks run on the
// compacted list of in-cube samples only (their opacity is exactly 0 otherwise, renderer.py:222), whose length stays on the device: those
// launches are sized for the whole batch and their surplus blocks return at once.  With an occupancy mask in the trainer (UvtOcc) the list holds
// the in-cube samples of occupied cells only; everything behind the list is the same code.  Every layer's POST-activation output is kept; for ReLU
// and LeakyReLU(0.2) its sign is the derivative torch uses.  Weight gradients are dZ^T . X over fixed 1024-row chunks, summed in chunk
// order by a second kernel: no float atomics, two backwards of one batch are bit-identical.
#pragma once
#include "ngf_device.hpp"
#include "ngf_uv_occupancy.hpp"

namespace ngf {

constexpr int kUvtChunk = 1024;          // rows per split-K chunk of a weight gradient
constexpr int kUvtLdsPad = 80;           // LDS row of a 64-wide tile: 80 floats puts the four k rows of a fragment read on disjoint banks

#define NGF_UVT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// C = A . B over strided operands: A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn].
//   forward   Z = X W^T:  A = X (sak 1), B(k, n) = W[n K + k]
//   dX        dZ W:       A = dZ (sak 1), B(k, n) = W[k K_in + n]
//   dW        dZ^T X:     A(m, k) = dZ[k ld + m] (sam 1), B = X; split = 1: blockIdx.z takes rows [z chunk, (z + 1) chunk) and writes its
//                         partial to C + z czs
struct UvtGemm {
    const float *A;
    const float *B;
    float *C;
    const float *bias;     // forward: + bias[n] (NULL = none)
    const float *add;      // backward: + add[m ldadd + n] before the mask (NULL = none)
    const float *aux;      // backward: x act'(aux[m ldaux + n]) (NULL = none)
    const int32_t *Mdev;   // rows on the device (split: the K extent) or NULL
    float *partb;          // split: bias-gradient partials [chunk][M] (NULL = none)
    int64_t sam, sak, sbk, sbn, ldc, czs, ldadd, ldaux;
    int32_t M, N, K;
    int32_t act;           // 0 none, 1 ReLU, 2 LeakyReLU(0.2): forward activation, or the derivative applied with `aux`
    int32_t split, chunk;
};

__device__ __forceinline__ float uvt_act(float x, int act)
{
    if (act == 1) return x > 0.0f ? x : 0.0f;
    if (act == 2) return x > 0.0f ? x : 0.2f * x;
    return x;
}

// d act / d x from the post-activation value y: y > 0 iff x > 0 for both (torch: threshold_backward / leaky_relu_backward use x > 0)
__device__ __forceinline__ float uvt_dact(float y, int act)
{
    if (act == 1) return y > 0.0f ? 1.0f : 0.0f;
    if (act == 2) return y > 0.0f ? 1.0f : 0.2f;
    return 1.0f;
}

// one k-step of 16 of both operands, global -> registers (element e = tid + 256 r of the 64 x 16 tiles; the mapping follows the unit stride, so a
// wave's loads are contiguous)
__device__ __forceinline__ void uvt_gload(const UvtGemm &G, int M, int m0, int n0, int k0, int ke, int tid, bool a_kfast, bool b_nfast, float (&ra)[4],
                                          float (&rb)[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = tid + 256 * r;
        const int am = a_kfast ? (e >> 4) : (e & 63), ak = a_kfast ? (e & 15) : (e >> 6);
        const int gm = m0 + am, gk = k0 + ak;
        ra[r] = (gm < M && gk < ke) ? G.A[(int64_t)gm * G.sam + (int64_t)gk * G.sak] : 0.0f;
        const int bn = b_nfast ? (e & 63) : (e >> 4), bk = b_nfast ? (e >> 6) : (e & 15);
        const int gn = n0 + bn, gk2 = k0 + bk;
        rb[r] = (gn < G.N && gk2 < ke) ? G.B[(int64_t)gk2 * G.sbk + (int64_t)gn * G.sbn] : 0.0f;
    }
}

// The next k-step's operands are loaded into registers while the MFMAs of this one run (one LDS buffer, two barriers per step).  Sub-tiles of
// 16 rows / columns that lie wholly outside M / N are skipped (wave-uniform): the 1- to 3-unit layers cost one sub-tile, not a 64-wide tile.
// split = 1 with partb set: the blocks of the first column tile also sum the A tile (dZ^T: row m = unit, column k = sample) over their chunk in
// fp64, in sample order -- the bias gradient partial of the chunk, partb[z M + m].
__global__ void __launch_bounds__(256) uvt_gemm_kernel(const UvtGemm G)
{
    __shared__ float As[16 * kUvtLdsPad];
    __shared__ float Bs[16 * kUvtLdsPad];
    int M = G.M, K = G.K;
    if (G.Mdev) {
        if (G.split) K = min(K, *G.Mdev);
        else M = min(M, *G.Mdev);
    }
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    if (m0 >= M) return;
    int kb = 0, ke = K;
    float *C = G.C;
    if (G.split) {
        kb = blockIdx.z * G.chunk;
        ke = min(K, kb + G.chunk);
        if (kb >= ke) return;
        C += (int64_t)blockIdx.z * G.czs;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
    const int fi = lane & 15, fk = lane >> 4;
    const bool li0 = m0 + wm < M, li1 = m0 + wm + 16 < M, lj0 = n0 + wn < G.N, lj1 = n0 + wn + 16 < G.N;
    const bool bsum = G.split && G.partb && blockIdx.y == 0 && tid < 64;
    double bacc = 0.0;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const bool a_kfast = G.sak == 1, b_nfast = G.sbn == 1;
    float ra[4], rb[4];
    uvt_gload(G, M, m0, n0, kb, ke, tid, a_kfast, b_nfast, ra, rb);
    for (int k0 = kb; k0 < ke; k0 += 16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + 256 * r;
            const int am = a_kfast ? (e >> 4) : (e & 63), ak = a_kfast ? (e & 15) : (e >> 6);
            As[ak * kUvtLdsPad + am] = ra[r];
            const int bn = b_nfast ? (e & 63) : (e >> 4), bk = b_nfast ? (e >> 6) : (e & 15);
            Bs[bk * kUvtLdsPad + bn] = rb[r];
        }
        __syncthreads();
        if (k0 + 16 < ke) uvt_gload(G, M, m0, n0, k0 + 16, ke, tid, a_kfast, b_nfast, ra, rb);
        if (bsum) {
#pragma unroll
            for (int k = 0; k < 16; ++k) bacc += (double)As[k * kUvtLdsPad + tid];
        }
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            const int kr = (k4 * 4 + fk) * kUvtLdsPad;
            const float a0 = As[kr + wm + fi], a1 = As[kr + wm + 16 + fi];
            const float b0 = Bs[kr + wn + fi], b1 = Bs[kr + wn + 16 + fi];
            if (li0 && lj0) acc[0][0] = NGF_UVT_MFMA(a0, b0, acc[0][0]);
            if (li0 && lj1) acc[0][1] = NGF_UVT_MFMA(a0, b1, acc[0][1]);
            if (li1 && lj0) acc[1][0] = NGF_UVT_MFMA(a1, b0, acc[1][0]);
            if (li1 && lj1) acc[1][1] = NGF_UVT_MFMA(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    if (bsum && m0 + tid < M) G.partb[(int64_t)blockIdx.z * M + m0 + tid] = (float)bacc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + fk * 4 + r, col = n0 + wn + j * 16 + fi;
                if (row >= M || col >= G.N) continue;
                float v = acc[i][j][r];
                if (G.bias) v = uvt_act(v + G.bias[col], G.act);
                if (G.add) v = v + G.add[(int64_t)row * G.ldadd + col];
                if (G.aux) v = v * uvt_dact(G.aux[(int64_t)row * G.ldaux + col], G.act);
                C[(int64_t)row * G.ldc + col] = v;
            }
}

// gw[i] = sum over chunks z (in order) of part[z nk + i]; gb[n] likewise from partb
__global__ void __launch_bounds__(256) uvt_reduce_kernel(const float *part, const float *partb, int64_t nk, int N, int rows_static,
                                                         const int32_t *rows_dev, float *gw, float *gb)
{
    const int rows = rows_dev ? min(rows_static, *rows_dev) : rows_static;
    const int nz = (rows + kUvtChunk - 1) / kUvtChunk;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nk) {
        float s = 0.0f;
        for (int z = 0; z < nz; ++z) s += part[(int64_t)z * nk + i];
        gw[i] = s;
    }
    if (i < N) {
        float s = 0.0f;
        for (int z = 0; z < nz; ++z) s += partb[(int64_t)z * N + i];
        gb[i] = s;
    }
}

// ---- rays: cube_ray_generation (renderer.py:79-141), bit-compatible with uv_render_kernel ---------------------------------------------------
struct UvtRays {
    const float *cam;      // [N,3]
    const float *raydir;   // [N,R,3]
    const float *U;        // [N,R,S]
    float *ray_pos;        // [N,R,S,3] (output)
    float *seg;            // [N R S]
    int32_t *cnt;          // [N R] valid samples per ray: the in-cube ones, with a mask (OCC) those of them whose cell is occupied
    int64_t nrays;
    int32_t R, S;
};

// The trainer's occupancy mask (ngf_uv_trainer_set_occupancy; grid and bit order of ngf_uv_occupancy.hpp), read by the OCC instantiations of
// uvt_rays_kernel and uvt_compact_kernel alone.  Both decide a sample by the SAME expression on the SAME floats -- the strict in-cube test, then
// uv_occ_lookup, on the float32 position the rays kernel stores in ray_pos and the compact kernel reads back -- so the count and the list agree.
struct UvtOcc {
    const uint8_t *bits;
    int32_t n[3];
    float h[3];            // (float)n[k] * 0.5f
    int32_t *cnt_in;       // [N R] in-cube samples per ray (rays kernel, OCC only)
};

// p [3] is valid: strictly inside the cube and, with a mask, in an occupied cell (only lanes that passed the in-cube test load a byte)
template <bool OCC>
__device__ __forceinline__ bool uvt_valid(const UvtOcc &O, const float p[3], bool &in_cube)
{
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) valid = valid && (p[k] > -1.0f) && (p[k] < 1.0f);
    in_cube = valid;
    if constexpr (OCC) {
        if (valid) valid = uv_occ_lookup(O.bits, O.n, O.h, p);
    }
    return valid;
}

template <bool OCC>
__global__ void __launch_bounds__(256) uvt_rays_kernel(const UvtRays A, const UvtOcc O)
{
    const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ray >= A.nrays) return;
    const int64_t cam = ray / A.R;
    const int S = A.S;
    float d[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d[k] = A.raydir[ray * 3 + k]; cp[k] = A.cam[cam * 3 + k]; }
    float t1[3], t2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { t1[k] = (-1.0f - cp[k]) / d[k]; t2[k] = (1.0f - cp[k]) / d[k]; }
    const float tmin = fmaxf(fminf(t1[0], t2[0]), fmaxf(fminf(t1[1], t2[1]), fminf(t1[2], t2[2])));
    const float tmax = fminf(fmaxf(t1[0], t2[0]), fminf(fmaxf(t1[1], t2[1]), fmaxf(t1[2], t2[2])));
    const float t0 = fmaxf((tmin < tmax) ? tmin : 0.0f, 0.0f);
    const float dt = (float)(2.0 / S), dtj = (float)((2.0 / S) * 0.05);
    double cum = 0.0;
    int n = 0, n_in = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t m = ray * S + s;
        const float sg = dt + dtj * (A.U[m] - 0.5f);
        const double before = cum;
        cum += (double)sg;
        const float e0 = t0 + (float)before, e1 = t0 + (float)cum;
        const float mid = (e0 + e1) / 2.0f;
        float p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = cp[k] + d[k] * mid;
            A.ray_pos[m * 3 + k] = p[k];
        }
        bool in_cube;
        const bool valid = uvt_valid<OCC>(O, p, in_cube);
        A.seg[m] = sg;
        n += valid ? 1 : 0;
        n_in += in_cube ? 1 : 0;
    }
    A.cnt[ray] = n;
    if constexpr (OCC) O.cnt_in[ray] = n_in;
}

// exclusive scan of cnt [n] -> off [n], total -> *total (one block of 1024)
__global__ void __launch_bounds__(1024) uvt_scan_kernel(const int32_t *cnt, int64_t n, int32_t *off, int32_t *total)
{
    __shared__ int32_t sh[1024];
    const int32_t sum = block_scan_runs(cnt, n, off, sh);
    if (threadIdx.x == 1023) *total = sum;
}

// list[v] = flat sample index of valid sample v (ray-major, sample order); vid[m] = v or -1.  Valid as uvt_rays_kernel<OCC> counted it.
template <bool OCC>
__global__ void __launch_bounds__(256) uvt_compact_kernel(const float *ray_pos, const int32_t *off, int64_t nrays, int S, int32_t *list, int32_t *vid,
                                                          const UvtOcc O)
{
    const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ray >= nrays) return;
    int32_t v = off[ray];
    for (int s = 0; s < S; ++s) {
        const int64_t m = ray * S + s;
        const float p[3] = {ray_pos[m * 3], ray_pos[m * 3 + 1], ray_pos[m * 3 + 2]};
        bool in_cube;
        const bool valid = uvt_valid<OCC>(O, p, in_cube);
        if (valid) list[v] = (int32_t)m;
        vid[m] = valid ? v++ : -1;
    }
}

// kept[m] = 1 where sample m is in the list of the last forward (ngf_uv_train_kept)
__global__ void __launch_bounds__(256) uvt_kept_kernel(const int32_t *vid, int64_t M, uint8_t *kept)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m < M) kept[m] = vid[m] >= 0 ? 1 : 0;
}

// [x (D), sin(x_d 2^f) d-major (D F), cos(same) (D F), zeros up to ld] (util.py:427-438)
template <int D, int F>
__device__ __forceinline__ void uvt_pe_row(float *row, const float x[D], int ld)
{
#pragma unroll
    for (int d = 0; d < D; ++d) row[d] = x[d];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float a = x[d] * (float)(1 << f);
            row[D + d * F + f] = sinf(a);
            row[D + D * F + d * F + f] = cosf(a);
        }
    for (int c = D + 2 * D * F; c < ld; ++c) row[c] = 0.0f;
}

// gauge input of every sample: PE10(p), ld 64
__global__ void __launch_bounds__(256) uvt_pe_pos_kernel(const float *ray_pos, int64_t M, float *X)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float p[3] = {ray_pos[m * 3], ray_pos[m * 3 + 1], ray_pos[m * 3 + 2]};
    uvt_pe_row<3, 10>(X + m * 64, p, 64);
}

// geometry input of in-cube sample v: its gauge input row
__global__ void __launch_bounds__(256) uvt_gather_kernel(const float *Xall, const int32_t *list, const int32_t *total, int64_t cap, float *X)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t v = i >> 6;
    if (v >= min(cap, (int64_t)*total)) return;
    X[i] = Xall[(int64_t)list[v] * 64 + (i & 63)];
}

// uv of every sample from the gauge output q [M, ld 4]: tanh (square) or F.normalize (sphere, eps 1e-12)
__global__ void __launch_bounds__(256) uvt_uv_kernel(const float *Q, int64_t M, int sphere, float *uv)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float *q = Q + m * 4;
    if (sphere) {
        const float nrm = fmaxf(sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]), 1e-12f);
#pragma unroll
    for (int k = 0; k < 3; ++k) uv[m * 3 + k] = q[k] / nrm;
    } else {
        uv[m * 2] = tanhf(q[0]);
        uv[m * 2 + 1] = tanhf(q[1]);
    }
}

// texture inputs of in-cube sample v: PE10(uv) (ld 64) and the view part of block2.0's input, [d, PE6(d)] in columns 256..294 of X2 (ld 296)
__global__ void __launch_bounds__(256) uvt_tex_in_kernel(const float *uv, const float *raydir, const int32_t *list, const int32_t *total, int64_t cap,
                                                         int D, int S, float *Xt, float *X2)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= min(cap, (int64_t)*total)) return;
    const int64_t m = list[v];
    if (D == 3) {
        const float u[3] = {uv[m * 3], uv[m * 3 + 1], uv[m * 3 + 2]};
        uvt_pe_row<3, 10>(Xt + v * 64, u, 64);
    } else {
        const float u[2] = {uv[m * 2], uv[m * 2 + 1]};
        uvt_pe_row<2, 10>(Xt + v * 64, u, 64);
    }
    const int64_t ray = m / S;
    const float d[3] = {raydir[ray * 3], raydir[ray * 3 + 1], raydir[ray * 3 + 2]};
    uvt_pe_row<3, 6>(X2 + v * 296 + 256, d, 40);
}

__device__ __forceinline__ float uvt_softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
// torch softplus_backward (beta 1, threshold 20): z = exp(x), x > 20 ? g : g z / (z + 1)
__device__ __forceinline__ float uvt_dsoftplus(float x)
{
    if (x > 20.0f) return 1.0f;
    const float z = expf(x);
    return z / (z + 1.0f);
}

struct UvtComp {
    const float *seg;
    const int32_t *vid;
    const float *raw;      // [V] raw density (geometry output)
    const float *c1;       // [V, 4] color1 pre-activation
    const float *c2;       // [V, 4] block2 output
    const float *bg;       // [N,3] or NULL
    float *color, *trans, *weight;          // outputs [nrays,3], [nrays], [nrays,S]
    float *opac, *acct;                     // [nrays S]: opacity and the exclusive transmittance in front of each sample
    float *xraw;                            // [nrays, 4]: colour before the tone map, T at the back
    // backward
    const float *d_color, *d_trans, *d_weight;
    float *d_raw, *d_c1, *d_c2;
    int64_t nrays;
    int32_t R, S;
};

// ray_march (renderer.py:176-247) + background + simple_tone_map, one thread per ray, as uv_render_kernel composites
__global__ void __launch_bounds__(256) uvt_composite_kernel(const UvtComp A)
{
    const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ray >= A.nrays) return;
    const int S = A.S;
    float T = 1.0f, rc[3] = {0.0f, 0.0f, 0.0f};
    for (int s = 0; s < S; ++s) {
        const int64_t m = ray * S + s;
        const int v = A.vid[m];
        float sigma = 0.0f, col[3] = {0.0f, 0.0f, 0.0f};
        if (v >= 0) {
            sigma = uvt_softplus(A.raw[v]);
    #pragma unroll
    for (int k = 0; k < 3; ++k) col[k] = fmaxf(uvt_softplus(A.c1[(int64_t)v * 4 + k]) + A.c2[(int64_t)v * 4 + k], 0.0f);
        }
        const float o = 1.0f - expf(-(sigma * (v >= 0 ? 1.0f : 0.0f)) * A.seg[m]);
        const float w = o * T;
        A.opac[m] = o;
        A.acct[m] = T;
        A.weight[m] = w;
        T = T * ((1.0f - o) + 1e-10f);
#pragma unroll
    for (int k = 0; k < 3; ++k) rc[k] += col[k] * w;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float c = rc[k];
        if (A.bg) c += A.bg[(ray / A.R) * 3 + k] * T;
        A.xraw[ray * 4 + k] = c;
        c = powf(c * 1.0f + 1e-5f, (float)(1.0 / 2.2));
        A.color[ray * 3 + k] = fminf(fmaxf(c, 0.0f), 1.0f);
    }
    A.xraw[ray * 4 + 3] = T;
    A.trans[ray] = T;
}

// backward of the above: tone map (clamp passes at the bounds), background, the exclusive cumprod in closed form from the back
// (G_{s-1} = f_s G_s + dw_s o_s, do_s = A_s (dw_s - G_s), f_s = 1 - o_s + 1e-10: no division), opacity, softplus, the colour clamp
__global__ void __launch_bounds__(256) uvt_composite_bwd_kernel(const UvtComp A)
{
    const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ray >= A.nrays) return;
    const int S = A.S;
    float dx[3];
    float dT = A.d_trans ? A.d_trans[ray] : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = A.xraw[ray * 4 + k];
        const float y = powf(x * 1.0f + 1e-5f, (float)(1.0 / 2.2));
        const float g = A.d_color ? A.d_color[ray * 3 + k] : 0.0f;
        const float gy = (y >= 0.0f && y <= 1.0f) ? g : 0.0f;
        dx[k] = gy * ((float)(1.0 / 2.2) * powf(x * 1.0f + 1e-5f, (float)(1.0 / 2.2 - 1.0)));
        if (A.bg) dT += dx[k] * A.bg[(ray / A.R) * 3 + k];
    }
    double G = dT;             // the suffix recurrence in fp64: do_s = A_s (dw_s - G_s) cancels where a sample sits behind an opaque one
    for (int s = S - 1; s >= 0; --s) {
        const int64_t m = ray * S + s;
        const int v = A.vid[m];
        const float o = A.opac[m], acc = A.acct[m], w = o * acc;
        float col[3] = {0.0f, 0.0f, 0.0f}, orig[3] = {0.0f, 0.0f, 0.0f}, c1r[3] = {0.0f, 0.0f, 0.0f};
        float raw = 0.0f, sigma = 0.0f;
        if (v >= 0) {
            raw = A.raw[v];
            sigma = uvt_softplus(raw);
    #pragma unroll
    for (int k = 0; k < 3; ++k) {
                c1r[k] = A.c1[(int64_t)v * 4 + k];
                orig[k] = uvt_softplus(c1r[k]) + A.c2[(int64_t)v * 4 + k];
                col[k] = fmaxf(orig[k], 0.0f);
            }
        }
        double dw = ((double)dx[0] * col[0] + (double)dx[1] * col[1]) + (double)dx[2] * col[2];
        if (A.d_weight) dw += A.d_weight[m];
        const double dop = acc * (dw - G);
        G = (double)((1.0f - o) + 1e-10f) * G + dw * o;
        if (v < 0) continue;
        const float sg = A.seg[m];
        const float e = expf(-sigma * sg);
        A.d_raw[v] = (float)(dop * e * sg * uvt_dsoftplus(raw));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
            const float dorig = orig[k] >= 0.0f ? dx[k] * w : 0.0f;
            A.d_c2[(int64_t)v * 4 + k] = dorig;
            A.d_c1[(int64_t)v * 4 + k] = dorig * uvt_dsoftplus(c1r[k]);
        }
    }
}

// d loss / d q (gauge output) of every sample: the texture PE backward (in-cube samples) + the upstream d uv, through tanh / F.normalize
template <int D>
__device__ __forceinline__ void uvt_uv_bwd(const float *Q, const float *uv, const float *dXt, const int32_t *vid, const float *d_uv, int64_t m, float *dQ)
{
    float du[D];
    const int v = vid[m];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float g = 0.0f;
        if (v >= 0) {
            const float *r = dXt + (int64_t)v * 64;
            const float x = uv[m * D + d];
            float pe = 0.0f;
#pragma unroll
            for (int f = 0; f < 10; ++f) {
                const float fr = (float)(1 << f), a = x * fr;
                pe += (r[D + d * 10 + f] * cosf(a) - r[D + D * 10 + d * 10 + f] * sinf(a)) * fr;
            }
            g = r[d] + pe;
        }
        if (d_uv) g += d_uv[m * D + d];
        du[d] = g;
    }
    const float *q = Q + m * 4;
    float *o = dQ + m * 4;
    if constexpr (D == 3) {
        const float n = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
        if (n >= 1e-12f) {
            const float y0 = q[0] / n, y1 = q[1] / n, y2 = q[2] / n;
            const float yd = (y0 * du[0] + y1 * du[1]) + y2 * du[2];
            o[0] = (du[0] - y0 * yd) / n;
            o[1] = (du[1] - y1 * yd) / n;
            o[2] = (du[2] - y2 * yd) / n;
        } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = du[k] / 1e-12f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float y = uv[m * 2 + k];
            o[k] = du[k] * (1.0f - y * y);
        }
    }
}

__global__ void __launch_bounds__(256) uvt_uv_bwd_kernel(const float *Q, const float *uv, const float *dXt, const int32_t *vid, const float *d_uv, int64_t M,
                                                         int sphere, float *dQ)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    if (sphere) uvt_uv_bwd<3>(Q, uv, dXt, vid, d_uv, m, dQ);
    else uvt_uv_bwd<2>(Q, uv, dXt, vid, d_uv, m, dQ);
}

}  // namespace ngf
