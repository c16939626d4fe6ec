// ngf_uv_inverse_train.hpp -- NeuTex's inverse gauge (ngf_uv_inverse.hpp: uv [n, D] -> 64 -> 512 -> 512 -> 512 -> xyz, ReLU) with a backward
// pass; host side in ngf_uv_inverse_train.hip, DESIGN.md section 4.13.
//
//   uvit_pack_kernel     gathers the caller's ten tensors into the streamed layouts of ngf_uv.hpp's blocks ON THE DEVICE: the forward set (the
//                        segments ngf_uv_inverse_create packs on the host, through the same ngf_uv_pack.hpp) and the transposed set the dX
//                        chain reads.  The weights change every optimiser step; a host round trip per step would cost more than the network.
//   uvit_forward_kernel  uv_inverse_kernel's pass (ngf_uv_inverse.hpp: uv_inverse_pass, the one text of both) -- hence the same bits -- which
//                        also keeps the POST-activation outputs of the four hidden layers (their sign is the derivative torch uses:
//                        relu(z) > 0 iff z > 0; and they are the dW products' right operands as they are).
//   uvit_dx_kernel       the forward mirrored: d_xyz (padded to four k-steps, as linear1 pads uv) -> 512 -> 512 -> 512 -> 64 -> D through dense /
//                        kstep / store_act / dense_out with ACT = kUvActNone, the transposed weights and a zero bias.  Each layer's accumulators
//                        are masked by the kept outputs before they are stored; every layer's dZ also goes to memory for the weight gradients.
//   uvit_dw_kernel       dW = dZ^T H per layer over row chunks (split-K): 128 x 128 output tile per block, both operands staged through LDS, four
//                        waves of 64 x 64 on v_mfma_f32_16x16x4_f32; db = column sums of dZ in fp64.  uvit_reduce_kernel sums the chunks in
//                        chunk order.  No float atomics anywhere: two backwards of one forward are the same bits.
//
// Kept outputs and dZ are ROW-MAJOR [n, width].  In accumulator order lane (point s, quarter kq) holds units mt * 16 + 4 kq + 0..3 of its point in
// one f32x4 per unit tile, so a row-major row takes them as one 16-byte store (64 contiguous bytes per point and tile) and gives them back as one
// 16-byte load -- no shuffle either way -- and it is what the dW product reads with unit stride.  A tile image in accumulator order would save
// nothing and need a transposing read in the dW kernel.
// A tail tile's padding lanes evaluate the last point again (as in the forward) and neither store kept outputs nor dZ: the dW products run over
// rows 0..n-1 only, so they contribute nothing.
#pragma once
#include "ngf_uv_inverse.hpp"

namespace ngf {

constexpr int kUvitHiddenOuts = kUvInvMid + (1 + kUvInvHiddenLayers) * kUvInvHidden;      // 1600 kept floats (and as many of dZ) per point
constexpr int kUvitMinChunk = 1024, kUvitMaxChunks = 64;
// rows per split-K chunk of a weight gradient: a function of n alone (so a batch's sums do not depend on the engine's capacity): 1024 rows up to
// 65 536 points, beyond that n / 64 rounded up to the k-step of the dW kernel -- at most 64 partial images per layer
__host__ __device__ inline int64_t uvit_chunk(int64_t n)
{
    const int64_t c = ((n + kUvitMaxChunks - 1) / kUvitMaxChunks + 15) / 16 * 16;
    return c > kUvitMinChunk ? c : kUvitMinChunk;
}

// ---- device packer -----------------------------------------------------------------------------------------------------------------------
// Every segment of the plan (ngf_uv_pack.hpp: uv_inverse_plan), one grid row each; what a word holds is uv_pack_value's to say.
struct UvitPack {
    float *dst;
    int32_t nseg, pad_;
    UvPackSeg seg[kUvInvSegs];
};

__global__ void __launch_bounds__(256) uvit_pack_kernel(const UvitPack P)
{
    const UvPackSeg &S = P.seg[blockIdx.y];
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < S.count; idx += gridDim.x * 256) P.dst[S.dst + idx] = uv_pack_value(S, idx);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------------
struct UvitFwdArgs {
    UvInverseArgs q;
    float *keep[2 + kUvInvHiddenLayers];      // relu(outputs) of linear1 [n, 64], linear2 and the hidden layers [n, 512]
};

__global__ void __launch_bounds__(64 * kUvInvWaves) uvit_forward_kernel(const UvitFwdArgs A) { uv_inverse_pass<true>(A.q, A.keep); }

// ---- dX chain --------------------------------------------------------------------------------------------------------------------------------
struct UvitDxArgs {
    const float *w;                                  // the packed set (offsets below, floats)
    const float *d_xyz;                              // [n, 3]
    float *d_uv;                                     // [n, D] or NULL
    const float *keep[2 + kUvInvHiddenLayers];       // as the forward left them
    float *dz[2 + kUvInvHiddenLayers];               // d loss / d pre-activation of the same layers
    int64_t n;
    int32_t dim;
    UvInvDxAt at;
};

// acc <- acc where the kept output is positive, else 0 (torch's threshold_backward); a live lane's result to its dZ row.  The sched_barrier keeps
// the compiler from hoisting all NT mask loads in front of the selects (128 more registers at NT = 32).
template <int NT>
__device__ __forceinline__ void uvit_mask_store(const float *krow, float *drow, bool live, f32x4 acc[1][NT])
{
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
        const f32x4 m = *reinterpret_cast<const f32x4 *>(krow + mt * 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[0][mt][r] = m[r] > 0.0f ? acc[0][mt][r] : 0.0f;
        if (live) *reinterpret_cast<f32x4 *>(drow + mt * 16) = acc[0][mt];
        if ((mt & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

__global__ void __launch_bounds__(64 * kUvInvWaves) uvit_dx_kernel(const UvitDxArgs Q)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int lane = threadIdx.x & 63;
    float *act = smem + (threadIdx.x >> 6) * kUvInvWaveLds;
    const int64_t passes = (Q.n + kUvInvTilePoints - 1) / kUvInvTilePoints, stride = (int64_t)gridDim.x * kUvInvWaves;
    for (int64_t p = (int64_t)blockIdx.x * kUvInvWaves + (threadIdx.x >> 6); p < passes; p += stride) {
        int wz = 0;
        asm volatile("" : "+s"(wz), "+v"(lane));
        const float *W = Q.w + wz;
        const int kq = lane >> 4;
        const int64_t idx = p * kUvInvTilePoints + (lane & 15);
        const bool live = idx < Q.n;
        const int64_t i = live ? idx : Q.n - 1;          // padding lanes: the last point again (reads stay in bounds); nothing of theirs is stored
        const int kc = kq < 3 ? kq : 2;
        const float xc = Q.d_xyz[i * 3 + kc];
        const float x = kq < 3 ? xc : 0.0f;
        act[lane] = x;
#pragma unroll
        for (int t = 1; t < 4; ++t) act[t * 64 + lane] = 0.0f;
        f32x4 h4[1][4], h[1][32];
        KStepA<32, 1> pre[4];
        dense<32, 1, true>(W + Q.at.to, W + Q.at.zb, 4, lane, act, h);
        uvit_mask_store<32>(Q.keep[1 + kUvInvHiddenLayers] + i * kUvInvHidden + 4 * kq, Q.dz[1 + kUvInvHiddenLayers] + idx * kUvInvHidden + 4 * kq, live, h);
#pragma unroll 1
        for (int l = 0; l < kUvInvHiddenLayers; ++l) {
            const float *wl = W + Q.at.th + (size_t)l * (kUvInvHidden * kUvInvHidden);
            uv_wprefetch<32, 1>(wl, lane, pre);
            store_act<32, 1, kUvActNone>(act, lane, h);
            dense<32, 1, true>(wl, W + Q.at.zb, kUvInvRows, lane, act, h, 1 << 30, pre, true);
            const int k = kUvInvHiddenLayers - l;        // the layer whose pre-activation gradient this is: 2, 1
            uvit_mask_store<32>(Q.keep[k] + i * kUvInvHidden + 4 * kq, Q.dz[k] + idx * kUvInvHidden + 4 * kq, live, h);
        }
        KStepA<4, 1> pre4[4];
        uv_wprefetch<4, 1>(W + Q.at.t2, lane, pre4);
        store_act<32, 1, kUvActNone>(act, lane, h);
        dense<4, 1, true>(W + Q.at.t2, W + Q.at.zb, kUvInvRows, lane, act, h4, 1 << 30, pre4, true);
        uvit_mask_store<4>(Q.keep[0] + i * kUvInvMid + 4 * kq, Q.dz[0] + idx * kUvInvMid + 4 * kq, live, h4);
        if (Q.d_uv) {          // (uniform)
            UvOutW<kUvInvMid / 4> ow;
            store_act<4, 1, kUvActNone>(act, lane, h4);
            out_prefetch<kUvInvMid / 4>(W + Q.at.t1, lane, ow);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 o[1];
            dense_out<1, kUvInvMid / 4, kUvActNone>(ow, W + Q.at.zb, lane, act, o);
            // the four lanes of a point hold the same values: quarter 0 stores them, plain stores
            if (lane < 16 && live) {
                for (int k = 0; k < Q.dim; ++k) Q.d_uv[idx * Q.dim + k] = k == 0 ? o[0][0] : (k == 1 ? o[0][1] : o[0][2]);
            }
        }
    }
}

// ---- dW, db ------------------------------------------------------------------------------------------------------------------------------------
constexpr int kUvitTile = 128;            // outputs x inputs of a block's tile
constexpr int kUvitLd = kUvitTile + 16;   // LDS row of a k row: 144 floats puts the four k rows of a fragment read on disjoint banks, 16-byte aligned

// part[z][M, N] = sum over rows [z chunk, (z + 1) chunk) of dz[row, m] x[row, n]; partb[z][M] = the same rows' sums of dz[row, m] in fp64
struct UvitDw {
    const float *dz;      // [rows, M] at ld_dz
    const float *x;       // [rows, N] at ld_x
    float *part;
    double *partb;
    int64_t ld_dz, ld_x, rows;
    int32_t M, N, chunk;
};

// 16 rows x 128 columns of one operand, global -> registers: VEC (width a multiple of 4, 16-byte aligned rows) two f32x4 per thread, else eight floats
template <bool VEC>
__device__ __forceinline__ void uvit_gload(const float *src, int64_t ld, int width, int c0, int64_t k0, int64_t ke, int tid, float (&r)[8])
{
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q, row = e >> 5, col = c0 + (e & 31) * 4;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (k0 + row < ke && col < width) v = *reinterpret_cast<const f32x4 *>(src + (k0 + row) * ld + col);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[4 * q + j] = v[j];
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q, row = e >> 7, col = c0 + (e & 127);
            r[q] = (k0 + row < ke && col < width) ? src[(k0 + row) * ld + col] : 0.0f;
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void uvit_lstore(float *dst, int tid, const float (&r)[8])
{
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q;
            *reinterpret_cast<f32x4 *>(dst + (e >> 5) * kUvitLd + (e & 31) * 4) = f32x4{r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]};
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q;
            dst[(e >> 7) * kUvitLd + (e & 127)] = r[q];
        }
    }
}

// The next k-step's operands are loaded into registers while the MFMAs of this one run (one LDS buffer, two barriers per step).  16 x 16 sub-tiles
// wholly outside M / N are skipped (wave-uniform): last_linear's 3 x 512 gradient costs one sub-tile row, not a 128-wide tile.
template <bool VA, bool VB>
__global__ void __launch_bounds__(256) uvit_dw_kernel(const UvitDw G)
{
    __shared__ __attribute__((aligned(16))) float As[16 * kUvitLd];
    __shared__ __attribute__((aligned(16))) float Bs[16 * kUvitLd];
    const int m0 = blockIdx.x * kUvitTile, n0 = blockIdx.y * kUvitTile;
    const int64_t kb = (int64_t)blockIdx.z * G.chunk, ke = kb + G.chunk < G.rows ? kb + G.chunk : G.rows;
    if (kb >= ke) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = (w & 1) * 64, wn = (w >> 1) * 64;
    const int fi = lane & 15, fk = lane >> 4;
    bool li[4], lj[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { li[i] = m0 + wm + i * 16 < G.M; lj[i] = n0 + wn + i * 16 < G.N; }
    const bool bsum = G.partb && blockIdx.y == 0 && tid < kUvitTile;
    double bacc = 0.0;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float ra[8], rb[8];
    uvit_gload<VA>(G.dz, G.ld_dz, G.M, m0, kb, ke, tid, ra);
    uvit_gload<VB>(G.x, G.ld_x, G.N, n0, kb, ke, tid, rb);
    for (int64_t k0 = kb; k0 < ke; k0 += 16) {
        uvit_lstore<VA>(As, tid, ra);
        uvit_lstore<VB>(Bs, tid, rb);
        __syncthreads();
        if (k0 + 16 < ke) {
            uvit_gload<VA>(G.dz, G.ld_dz, G.M, m0, k0 + 16, ke, tid, ra);
            uvit_gload<VB>(G.x, G.ld_x, G.N, n0, k0 + 16, ke, tid, rb);
        }
        if (bsum) {
#pragma unroll
            for (int k = 0; k < 16; ++k) bacc += (double)As[k * kUvitLd + tid];          // in row order
        }
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            const int kr = (k4 * 4 + fk) * kUvitLd;
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[kr + wm + i * 16 + fi]; b[i] = Bs[kr + wn + i * 16 + fi]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (li[i] && lj[j]) acc[i][j] = NGF_UV_MFMA(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
    if (bsum && m0 + tid < G.M) G.partb[(int64_t)blockIdx.z * G.M + m0 + tid] = bacc;
    float *C = G.part + (int64_t)blockIdx.z * G.M * G.N;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + i * 16 + fk * 4 + r, col = n0 + wn + j * 16 + fi;
                if (row < G.M && col < G.N) C[(int64_t)row * G.N + col] = acc[i][j][r];
            }
}

// gw[i] = sum over chunks z = 0, 1, ... (in that order) of part[z nk + i]; gb[m] the same over partb in fp64, rounded once
__global__ void __launch_bounds__(256) uvit_reduce_kernel(const float *part, const double *partb, int64_t nk, int M, int nz, float *gw, float *gb)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nk) {
        float s = 0.0f;
        for (int z = 0; z < nz; ++z) s += part[(int64_t)z * nk + i];
        gw[i] = s;
    }
    if (i < M) {
        double s = 0.0;
        for (int z = 0; z < nz; ++z) s += partb[(int64_t)z * M + i];
        gb[i] = (float)s;
    }
}

}  // namespace ngf
