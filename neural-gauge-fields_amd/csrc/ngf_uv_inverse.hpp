// ngf_uv_inverse.hpp -- NeuTex's inverse gauge (UV-Mapping/model/gauge_fields.py:78-120, a modified AtlasNet core) at explicit template points:
//   uv [n, D] (D = 2 square | 3 sphere) -> linear1 D -> 64 -> linear2 64 -> 512 -> linear_list 2 x (512 -> 512) -> last_linear 512 -> 3, ReLU between.
// 558 592 + 64 D MAC per point, 94 % of them in the two 512 x 512 layers.
//
// The building blocks are ngf_uv.hpp's, unchanged: dense / kstep (the four-k-steps-ahead weight pipeline), store_act (raw accumulator rows to the
// wave's LDS rows, ReLU where the next layer reads them), uv_wprefetch, out_prefetch and dense_out.  All of them are templates over the number of
// 16-unit output tiles NT and take 512 units as NT = 32 at ONE 16-point tile per wave pass (NS = 1): their only fixed width is the row stride
// between the TILES of a pass (kUvActSteps = 80 rows), which a single tile never uses.  So nothing is restated here.
//
// One tile, not two: at fp32 a lane's share of 16 points x 512 outputs is 128 accumulator registers, and a tile's 512 activations are 128 LDS rows
// of 64 lanes = 32 KB.  Two tiles per wave would fit the registers (256 accumulators + 128 of weights in flight + ~35 = ~420 of 512) but not the
// LDS: 64 KB of rows per wave, so two waves per CU and half its SIMDs idle -- and computing a layer in two halves of 256 outputs does not help,
// the rows hold inputs, not outputs.  One tile keeps four waves per CU (128 KB of the 160 KB), one per SIMD, at the price that a 16-byte weight
// load feeds four matrix instructions instead of the eight of the 256-wide two-tile kernels (measured, it costs nothing).
//
// Work split (the texture export's): four waves per block, passes p = wave, wave + n_waves, ... of 16 points each, grid capped at the CU count, no
// queue, no atomics.  A tail's padding lanes evaluate the last point again and store nothing.  A point's three outputs depend on its own inputs
// and the weights alone -- a column of the matrix instructions -- so they are the same bits for every n and every place in the list.
#pragma once
#define NGF_UV_NO_EDIT_KERNEL
#include "ngf_host.hpp"
#include "ngf_uv.hpp"
#include "ngf_uv_pack.hpp"      // kUvInvMid / kUvInvHidden / kUvInvHiddenLayers, the offsets into the packed set

namespace ngf {

constexpr int kUvInvTilePoints = 16;                                          // points per wave pass
constexpr int kUvInvWaves = 4;                                                // waves per block, one per SIMD
constexpr int kUvInvRows = kUvInvHidden / 4;                                  // LDS rows (k-steps) of a wave: 128 x 64 lanes x 4 B = 32 KB
constexpr int kUvInvWaveLds = kUvInvRows * 64;                                // floats per wave
static_assert(kUvInvRows <= 256, "store_act's ds_write2st64 offsets are 8 bits");

struct UvInverseArgs {
    const float *w;        // packed weights / biases (offsets in `at`, floats)
    const float *uv;       // [n, D]
    float *xyz;            // [n, 3]
    int64_t n;
    int32_t dim;           // D
    UvInvFwdAt at;
};

// relu(acc) of a live lane's point to its row-major row (row: the point's row + 4 kq)
template <int NT>
__device__ __forceinline__ void uvit_keep(float *row, bool live, const f32x4 acc[1][NT])
{
    if (live) {
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = act_fn<0>(acc[0][mt][r]);
            *reinterpret_cast<f32x4 *>(row + mt * 16) = v;
        }
    }
}

// The whole pass of a block, for the inference kernel (ngf_uv_inverse.hip: uv_inverse_kernel) and the training forward
// (ngf_uv_inverse_train.hpp: uvit_forward_kernel, KEEP): the latter also stores the POST-activation outputs of the four hidden layers,
// row-major, to keep[0] [n, 64] and keep[1..3] [n, 512].  The arithmetic is one text, so the two kernels give the same bits.
template <bool KEEP>
__device__ __forceinline__ void uv_inverse_pass(const UvInverseArgs &Q, float *const *keep)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int lane = threadIdx.x & 63;
    float *act = smem + (threadIdx.x >> 6) * kUvInvWaveLds;
    const int64_t passes = (Q.n + kUvInvTilePoints - 1) / kUvInvTilePoints, stride = (int64_t)gridDim.x * kUvInvWaves;
    for (int64_t p = (int64_t)blockIdx.x * kUvInvWaves + (threadIdx.x >> 6); p < passes; p += stride) {
        // (opaque zero offset + lane id once per pass: see uv_networks)
        int wz = 0;
        asm volatile("" : "+s"(wz), "+v"(lane));
        const float *W = Q.w + wz;
        const int kq = lane >> 4;
        const int64_t idx = p * kUvInvTilePoints + (lane & 15);
        const bool live = idx < Q.n;
        const int64_t i = live ? idx : Q.n - 1;          // a tail's padding lanes evaluate the last point again; nothing of theirs is stored
        // linear1's inputs in natural order: entry f of a point lives in row f >> 2, lane quarter f & 3.  Quarter kq supplies coordinate kq in
        // row 0; the rest of the layer's 16 padded inputs are zero.  Every lane writes its own slots only.  (No lane-dependent control flow:
        // quarter 3 -- and quarter 2 of a square model -- loads the point's last coordinate and selects the zero.)
        const int kc = kq < Q.dim ? kq : Q.dim - 1;
        const float xc = Q.uv[i * Q.dim + kc];
        const float x = kq < Q.dim ? xc : 0.0f;
        KStepA<32, 1> pre[4];
        uv_wprefetch<32, 1>(W + Q.at.w2, lane, pre);
        act[lane] = x;
#pragma unroll
        for (int t = 1; t < 4; ++t) act[t * 64 + lane] = 0.0f;
        f32x4 h4[1][4], h[1][32];
        dense<4, 1, true>(W + Q.at.w1, W + Q.at.b1, 4, lane, act, h4);
        store_act<4, 1, kUvActNone>(act, lane, h4);
        if constexpr (KEEP) uvit_keep<4>(keep[0] + idx * kUvInvMid + 4 * kq, live, h4);
        dense<32, 1, true, 0>(W + Q.at.w2, W + Q.at.b2, kUvInvMid / 4, lane, act, h, 1 << 30, pre, true);
#pragma unroll 1
        for (int l = 0; l < kUvInvHiddenLayers; ++l) {
            const float *wl = W + Q.at.wh + (size_t)l * (kUvInvHidden * kUvInvHidden);
            uv_wprefetch<32, 1>(wl, lane, pre);
            store_act<32, 1, kUvActNone>(act, lane, h);
            if constexpr (KEEP) uvit_keep<32>(keep[1 + l] + idx * kUvInvHidden + 4 * kq, live, h);
            dense<32, 1, true, 0>(wl, W + Q.at.bh + l * kUvInvHidden, kUvInvRows, lane, act, h, 1 << 30, pre, true);
        }
        UvOutW<kUvInvRows> ow;
        store_act<32, 1, kUvActNone>(act, lane, h);
        out_prefetch<kUvInvRows>(W + Q.at.wo, lane, ow);
        if constexpr (KEEP) uvit_keep<32>(keep[1 + kUvInvHiddenLayers] + idx * kUvInvHidden + 4 * kq, live, h);
        __builtin_amdgcn_sched_barrier(0);
        f32x4 o[1];
        dense_out<1, kUvInvRows, 0, true>(ow, W + Q.at.bo, lane, act, o);
        // the four lanes of a point hold the same values: quarter 0 stores them
        if (lane < 16 && live) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Q.xyz[idx * 3 + k] = o[0][k];
        }
    }
}

// ---- host side, shared by ngf_uv_inverse.hip and ngf_uv_inverse_train.hip ---------------------------------------------------------------------
// `who`: the ABI function the message names
inline int check_inverse_desc(const char *who, const ngf_uv_inverse_desc *d)
{
    if (d->input_dim != 2 && d->input_dim != 3) return fail(NGF_E_ARG, "%s: input_dim must be 2 (square) or 3 (sphere), got %d", who, d->input_dim);
    for (int l = 0; l < NGF_UV_INVERSE_LAYERS; ++l)
        if (!d->w[l] || !d->b[l]) return fail(NGF_E_ARG, "%s: layer %d missing", who, l);
    return NGF_OK;
}

// One of the tile kernels (uv_inverse_kernel, uvit_forward_kernel, uvit_dx_kernel) over n points: four waves per block, one per SIMD, 16 points
// per wave pass; one block per CU (128 KB of activation rows), the grid capped at the CU count.
template <typename Args>
inline int launch_inverse_tiles(void (*kernel)(Args), const Args &args, int64_t n, int num_cus, hipStream_t st)
{
    if (int rc = poison_lds(st)) return rc;
    const int64_t grid = std::min<int64_t>(((n + kUvInvTilePoints - 1) / kUvInvTilePoints + kUvInvWaves - 1) / kUvInvWaves, num_cus);
    const size_t lds = (size_t)kUvInvWaves * kUvInvWaveLds * sizeof(float);
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), lds));
    NGF_LAUNCH(kernel, dim3((unsigned)grid), dim3(64 * kUvInvWaves), lds, st, args);
    return NGF_OK;
}

}  // namespace ngf
