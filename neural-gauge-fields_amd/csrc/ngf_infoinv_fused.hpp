// ngf_infoinv_fused.hpp -- the fused InfoInv training step (include/ngf.h: ngf_infoinv_train_step_backward, ngf_infoinv_train_adam_all,
// ngf_infoinv_train_adam_ext, ngf_infoinv_train_get_grad): the loop body of InfoInv/main.py:262-330 with the loss and the optimiser inside the
// library.  The forward, the per-sample deltas and the fixed-point plane scatter are the autograd path's kernels (ngf_infoinv_train.hpp),
// unchanged; what this file adds runs on this path only:
//   ii_loss_kernel          residual + rgb MSE (fp64 sum and mean) and d rgb_map = 2 (rgb - target) / (3 n), written where the backward reads it
//   ii_mm_kernel            weight gradients dW = Delta^T . In on v_mfma_f32_16x16x4_f32: a 64 x 64 tile per workgroup (four waves of 32 x 32),
//                           fp32 accumulation over kIiMmSub rows, those sums added in row order in fp64 registers; one partial per kIiMmChunk
//                           rows.  The bias column is the fp64 sum of the Delta tile staged in LDS (the density bias is a cancelling sum over
//                           every valid sample: fp32 is not enough for it)
//   ii_mm_reduce_kernel     partials added in chunk order in fp64 (only the chunks that hold rows: the count is read on the device)
//   ii_adam_plane_kernel    torch.optim.Adam on a plane in one pass: fixed-point accumulator and device-side scale in, + the L1 term, parameter,
//                           both moments and the packed channel-last copy out
//   adam_dense_all_kernel   the thirteen decoder tensors in one launch (<kIiDense>, ngf_adam.hpp)
// No float atomics anywhere: two steps from one state give identical bits.
#pragma once
#include "ngf_adam.hpp"
#include "ngf_infoinv_train.hpp"

namespace ngf {

constexpr int kIiMmK = 32;              // rows per k-step
constexpr int kIiMmLd = 40;             // LDS row of a k-step: 32 floats + 8.  Stores: a half-wave writes one row, 32 banks.  Fragment reads
                                        // (ds_read_b128, 16-lane groups {fi 0-3, 12-15 at fk} + {fi 4-11 at fk + 1}): slot (10 fi + fk) mod 16 is
                                        // a permutation of the group, so they are conflict-free too (36 collides on 7 of 8 lanes)
constexpr int kIiMmSub = 1024;          // rows summed in fp32 before the sums move to fp64
constexpr int kIiMmChunk = 8192;        // rows per workgroup = per partial
constexpr int kIiDense = 13;            // decoder tensors (which = 3..15)

#define NGF_II_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// ---- loss -------------------------------------------------------------------------------------------------------------------------------
// one workgroup: n3 = 3 n values of this ray chunk; inv = 1 / (3 n_total) as torch's mean backward has it (a float); loss[0] = sum of squared
// residuals (+= when `accumulate`), loss[1] = loss[0] / (3 n_total)
__global__ void __launch_bounds__(1024) ii_loss_kernel(const float *rgb, const float *tgt, int64_t n3, int64_t n3_total, float *d_rgb, double *loss,
                                                       int accumulate)
{
    __shared__ double part[1024];
    const float inv = 1.0f / (float)n3_total;
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < n3; e += 1024) {
        const float d = rgb[e] - tgt[e];
        d_rgb[e] = (2.0f * d) * inv;
        s += (double)d * (double)d;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double total = (accumulate ? loss[0] : 0.0) + part[0];
        loss[0] = total;
        loss[1] = total / (double)n3_total;
    }
}

// ---- weight gradients on the matrix pipe ------------------------------------------------------------------------------------------------
// part[chunk][m][n] = sum over the chunk's rows of X[m ld + row] * Y[n ld + row];  partb[chunk][m] = sum of X[m ld + row] (fp64)
struct IiMm {
    const float *X, *Y;
    int64_t ld;
    int64_t rows;                 // upper bound of the row count (sizes the launch)
    const int32_t *rows_dev;      // the row count on the device, or NULL
    int M, N;
    double *part, *partb;
};

// one k-step of both operands, global -> registers: element e = tid + 256 r is (row i = e >> 5 of the tile, sample k = e & 31): a wave reads two
// runs of 32 consecutive samples
__device__ __forceinline__ void ii_mm_gload(const IiMm &G, int m0, int n0, int64_t rb, int64_t re, int tid, float (&ra)[8], float (&rbv)[8])
{
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int e = tid + 256 * r;
        const int k = e & 31, i = e >> 5;
        const int64_t row = rb + k;
        const bool in = row < re;
        ra[r] = (in && m0 + i < G.M) ? G.X[(int64_t)(m0 + i) * G.ld + row] : 0.0f;
        rbv[r] = (in && n0 + i < G.N) ? G.Y[(int64_t)(n0 + i) * G.ld + row] : 0.0f;
    }
}

// The operands are sample-fast in memory, and they stay sample-fast in LDS (As[i][k]): the stores of a wave cover whole rows, and a lane fetches
// its four k of a fragment as ONE 16-byte read -- the MFMA of step j takes element j, i.e. the k of one instruction are {4 fk + j}: a
// permutation of the samples that both operands share, which a sum over samples does not see.  The next k-step's loads are in flight while
// the MFMAs of this one run (one LDS buffer, two barriers per step).  16-wide sub-tiles outside M / N are skipped (wave-uniform).
__global__ void __launch_bounds__(256) ii_mm_kernel(const IiMm G)
{
    __shared__ __attribute__((aligned(16))) float As[64 * kIiMmLd];
    __shared__ __attribute__((aligned(16))) float Bs[64 * kIiMmLd];
    int64_t rows = G.rows;
    if (G.rows_dev) rows = min(rows, (int64_t)*G.rows_dev);
    const int tiles_n = (G.N + 63) / 64;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int64_t r0 = (int64_t)blockIdx.y * kIiMmChunk;
    if (r0 >= rows) return;
    const int64_t r1 = min(rows, r0 + (int64_t)kIiMmChunk);
    const int m0 = tm * 64, n0 = tn * 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
    const int fi = lane & 15, fk = lane >> 4;
    const bool li0 = m0 + wm < G.M, li1 = m0 + wm + 16 < G.M, lj0 = n0 + wn < G.N, lj1 = n0 + wn + 16 < G.N;
    const bool bsum = G.partb && tn == 0 && tid < 64;
    double bacc = 0.0;
    double dacc[2][2][4];
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < 4; ++r) dacc[i][j][r] = 0.0;
        }
    float ra[8], rbv[8];
    ii_mm_gload(G, m0, n0, r0, r1, tid, ra, rbv);
    int sub = 0;
    for (int64_t k0 = r0; k0 < r1; k0 += kIiMmK) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int e = tid + 256 * r;
            As[(e >> 5) * kIiMmLd + (e & 31)] = ra[r];
            Bs[(e >> 5) * kIiMmLd + (e & 31)] = rbv[r];
        }
        __syncthreads();
        if (k0 + kIiMmK < r1) ii_mm_gload(G, m0, n0, k0 + kIiMmK, r1, tid, ra, rbv);
        if (bsum) {
#pragma unroll
            for (int k = 0; k < kIiMmK; k += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(&As[tid * kIiMmLd + k]);
                bacc += (double)v[0];
                bacc += (double)v[1];
                bacc += (double)v[2];
                bacc += (double)v[3];
            }
        }
#pragma unroll
        for (int kk = 0; kk < kIiMmK; kk += 16) {
            const int ko = kk + fk * 4;
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(&As[(wm + fi) * kIiMmLd + ko]);
            const f32x4 a1 = *reinterpret_cast<const f32x4 *>(&As[(wm + 16 + fi) * kIiMmLd + ko]);
            const f32x4 b0 = *reinterpret_cast<const f32x4 *>(&Bs[(wn + fi) * kIiMmLd + ko]);
            const f32x4 b1 = *reinterpret_cast<const f32x4 *>(&Bs[(wn + 16 + fi) * kIiMmLd + ko]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (li0 && lj0) acc[0][0] = NGF_II_MFMA(a0[j], b0[j], acc[0][0]);
                if (li0 && lj1) acc[0][1] = NGF_II_MFMA(a0[j], b1[j], acc[0][1]);
                if (li1 && lj0) acc[1][0] = NGF_II_MFMA(a1[j], b0[j], acc[1][0]);
                if (li1 && lj1) acc[1][1] = NGF_II_MFMA(a1[j], b1[j], acc[1][1]);
            }
        }
        __syncthreads();
        sub += kIiMmK;
        if (sub == kIiMmSub) {
            sub = 0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dacc[i][j][r] += (double)acc[i][j][r];
                    acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
        }
    }
    if (bsum && m0 + tid < G.M) G.partb[(int64_t)blockIdx.y * G.M + m0 + tid] = bacc;
    double *C = G.part + (int64_t)blockIdx.y * G.M * G.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + fk * 4 + r, col = n0 + wn + j * 16 + fi;
                if (row < G.M && col < G.N) C[(int64_t)row * G.N + col] = dacc[i][j][r] + (double)acc[i][j][r];
            }
}

// gw [M][N], gb [M] (float, NULL = not wanted) and optionally the fp64 matrix: the partials added in chunk order; `accumulate`: on top of what
// the outputs hold (the ray chunks of one batch)
__global__ void __launch_bounds__(256) ii_mm_reduce_kernel(const double *part, const double *partb, int64_t rows_static, const int32_t *rows_dev, int M,
                                                           int N, float *gw, float *gb, double *gw64, int accumulate)
{
    int64_t rows = rows_static;
    if (rows_dev) rows = min(rows, (int64_t)*rows_dev);
    const int chunks = (int)((rows + kIiMmChunk - 1) / kIiMmChunk);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int mn = M * N;
    if (e < mn) {
        double s = 0.0;
#pragma unroll 8
        for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * mn + e];
        if (gw) gw[e] = accumulate ? gw[e] + (float)s : (float)s;
        if (gw64) gw64[e] = accumulate ? gw64[e] + s : s;
    } else if (e < mn + M) {
        const int m = e - mn;
        double s = 0.0;
#pragma unroll 8
        for (int c = 0; c < chunks; ++c) s += partb[(int64_t)c * M + m];
        if (gb) gb[m] = accumulate ? gb[m] + (float)s : (float)s;
    }
}

// the ray chunks of one batch: the fixed-point sums of this chunk (its own scale) added to the reference-layout gradient
__global__ void __launch_bounds__(256) ii_plane_grad_add_kernel(const unsigned long long *gacc, const double *bound, int H, int W, float *out)
{
    const double inv = 1.0 / bound[kIiBoundBlocks];
    const int64_t total = (int64_t)kIiC * H * W;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % W);
        const int64_t t = e / W;
        const int y = (int)(t % H), c = (int)(t / H);
        const long long q = (long long)gacc[((size_t)(y + 1) * (W + 2) + (x + 1)) * kIiC + c];
        out[e] = out[e] + (float)((double)q * inv);
    }
}

// ---- torch.optim.Adam: the planes (AdamArgs, adam_one and the dense kernel adam_dense_all_kernel<kIiDense>: ngf_adam.hpp) --------------------------
// A plane [96][H][W].  FIXED: the gradient is the fixed-point accumulator [texel][96] times 1 / scale (a NaN scale -- non-finite feature
// gradients -- gives NaN gradients, never wrapped integers); else `gext`, a float gradient in the parameter's own layout.  A workgroup takes
// 64 texels of one row: the accumulator rows go through LDS so that every global access is a contiguous run, and the new values leave
// the same way into the packed copy `tex` -- the next forward packs nothing.
template <bool FIXED>
__global__ void __launch_bounds__(256) ii_adam_plane_kernel(float *p, float *m, float *v, int H, int W, const unsigned long long *gacc, const double *bound,
                                                            const float *gext, float *tex, const AdamArgs a)
{
    constexpr int C = kIiC;
    __shared__ float sg[64 * (C + 1)];
    const int tiles_x = (W + 63) / 64;
    double inv = 0.0;
    if (FIXED) inv = 1.0 / bound[kIiBoundBlocks];
    for (int tile = blockIdx.x; tile < H * tiles_x; tile += gridDim.x) {
        const int y = tile / tiles_x, x0 = (tile - y * tiles_x) * 64, nx = min(64, W - x0);
        const size_t texel0 = (size_t)(y + 1) * (W + 2) + (x0 + 1);
        if (FIXED) {
            for (int e = threadIdx.x; e < nx * C; e += 256)
                sg[(e / C) * (C + 1) + e % C] = (float)((double)(long long)gacc[texel0 * C + e] * inv);
            __syncthreads();
        }
        for (int e = threadIdx.x; e < C * 64; e += 256) {
            const int c = e >> 6, x = e & 63;
            if (x < nx) {
                const size_t i = ((size_t)c * H + y) * W + x0 + x;
                const float pv = p[i];
                const float g = (FIXED ? sg[x * (C + 1) + c] : gext[i]) + a.l1 * (pv > 0.0f ? 1.0f : (pv < 0.0f ? -1.0f : 0.0f));
                float mi = m[i], vi = v[i];
                const float pn = adam_one(pv, g, mi, vi, a);
                p[i] = pn; m[i] = mi; v[i] = vi;
                sg[x * (C + 1) + c] = pn;
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nx * C; e += 256) tex[texel0 * C + e] = sg[(e / C) * (C + 1) + e % C];
        __syncthreads();
    }
}

}  // namespace ngf
