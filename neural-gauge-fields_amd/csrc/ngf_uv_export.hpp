// ngf_uv_export.hpp -- TextureMlpDecoder.forward (UV-Mapping/model/decoder.py:56-121) on an explicit list of texture coordinates: what
// net_texture.export_textures / _export_cube / _export_sphere / _export_square (decoder.py:123-179) evaluate, 6 R^2 points at a time.
//
// The layers are the render kernel's own (ngf_uv.hpp: store_pe, dense, hidden_run, dense_out on v_mfma_f32_16x16x4_f32, two 16-sample tiles per
// wave pass, one wave per SIMD) reading the packed weight images of the same ngf_uv handle; only the march around them is gone.  A wave takes
// the passes p = wave, wave + n_waves, ... of 32 consecutive points: a static split (every point costs the same), no queue head, no atomics.
// A point's result does not depend on the tile or the pass that evaluates it, nor on the launch size.
//   view mode      (color1 + color2).clamp(min=0), softplus on color1 (clamp_texture = False, model.py:22-23); with an edit texture set the
//                  colour goes through uv_texture_edit exactly as in the render
//   diffuse mode   the viewdir=None branch of the exporters: sigmoid(color1(block1(.))); block2 does not run and no edit stage applies
#pragma once
#include "../../include/ngf.h"
#define NGF_UV_NO_EDIT_KERNEL 1
#include "ngf_uv.hpp"

namespace ngf {

struct UvTexArgs {
    UvArgs M;              // the handle's prototype: packed weights, their offsets, sphere / square, the edit texture
    const float *uv;       // [n,3] (z ignored for square models)
    const float *view;     // [3] (view_stride 0) or [n,3] (view_stride 3); unused in diffuse mode
    float *out;            // [n,3]
    int64_t n;
    int32_t view_stride, pad_;
};

// block1 -> color1 [-> block2] for NS x 16 points; uv / v: the coordinates and view direction of the lane's point in each tile.  The texture part
// of uv_networks (fp32, one wave per SIMD), layer for layer: same k-step order, same accumulation order, hence the render's bits for the same inputs.
template <int NS, bool DIFFUSE>
__device__ __forceinline__ void uv_texture_networks(const UvArgs &A, float *act, int lane, const float uv[NS][3], const float v[NS][3], float col[NS][3])
{
    // (opaque zero offset + lane id once per pass: see uv_networks)
    int wz = 0;
    asm volatile("" : "+s"(wz), "+v"(lane));
    const float *W = A.w + wz;
    f32x4 x[NS][16];
    KStepA<16, NS> pre[4];
    // block1: (63|42) -> 256 -> (5x) 256, LeakyReLU(0.2)
    uv_wprefetch<16, NS>(W + A.t1_w0, lane, pre);
    if (A.sphere) {
        store_pe<3, 10, NS>(act, 0, 16, lane, uv);
        dense<16, NS, true>(W + A.t1_w0, W + A.t1_b0, 16, lane, act, x, 1 << 30, pre, true);
    } else {
        store_pe<2, 10, NS>(act, 0, 12, lane, uv);
        dense<16, NS, true>(W + A.t1_w0, W + A.t1_b0, 12, lane, act, x, 1 << 30, pre, true);
    }
    uv_wprefetch<16, NS>(W + A.t1_wh, lane, pre);
    store_act<16, NS, kUvActNone>(act, lane, x);
    f32x4 c1[NS];
    {
        UvOutW<64> ow;
        hidden_run<NS, false, 1, true>(A, W + A.t1_wh, W + A.t1_qh, W + A.t1_bh, 5, lane, act, x, W + A.c1_w, ow, pre, true);
        dense_out<NS, 64, 1, true>(ow, W + A.c1_b, lane, act, c1);
    }
    if constexpr (DIFFUSE) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < 3; ++k) col[s][k] = 1.0f / (1.0f + expf(-c1[s][k]));          // torch.sigmoid (decoder.py:136)
    } else {
        // block2: [h(256), v(3), PE6(v)(36)] -> 256 -> (3x) 256 -> 3
        f32x4 c2[NS];
        uv_wprefetch<16, NS>(W + A.t2_w0, lane, pre);
        store_pe<3, 6, NS>(act, 64, 12, lane, v);
        dense<16, NS, true, 1>(W + A.t2_w0, W + A.t2_b0, 76, lane, act, x, 64, pre, true);
        uv_wprefetch<16, NS>(W + A.t2_wh, lane, pre);
        store_act<16, NS, kUvActNone>(act, lane, x);
        {
            UvOutW<64> ow;
            hidden_run<NS, false, 1, true>(A, W + A.t2_wh, W + A.t2_qh, W + A.t2_bh, 3, lane, act, x, W + A.t2_wo, ow, pre, true);
            dense_out<NS, 64, 1, true>(ow, W + A.t2_bo, lane, act, c2);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float orig[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float s1 = c1[s][k] > 20.0f ? c1[s][k] : log1pf(expf(c1[s][k]));      // softplus(color1)
                orig[k] = s1 + c2[s][k];
                col[s][k] = fmaxf(orig[k], 0.0f);
            }
            if (A.tex) uv_texture_edit(A.tex, A.tex_h, A.tex_w, A.tex_c, A.tex_mode, A.sphere, uv[s], orig, col[s]);
        }
    }
}

constexpr int kUvTexTiles = 2;                         // 16-point tiles per wave pass, as the render kernel at its default
constexpr int kUvTexPass = 16 * kUvTexTiles;           // points per wave pass

template <bool DIFFUSE>
__global__ void __launch_bounds__(256) uv_texture_eval_kernel(const UvTexArgs T)
{
    constexpr int NS = kUvTexTiles;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    float *act = smem + (threadIdx.x >> 6) * (NS * kUvWaveLds);
    const int64_t passes = (T.n + kUvTexPass - 1) / kUvTexPass, stride = (int64_t)gridDim.x * 4;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < passes; p += stride) {
        float q[NS][3], vq[NS][3], col[NS][3];
        int64_t idx[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            idx[s] = p * kUvTexPass + 16 * s + (lane & 15);
            const int64_t i = idx[s] < T.n ? idx[s] : T.n - 1;          // a tail's padding lanes evaluate the last point again; nothing of theirs is stored
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                q[s][k] = T.uv[i * 3 + k];
                vq[s][k] = DIFFUSE ? 0.0f : T.view[i * T.view_stride + k];
            }
        }
        uv_texture_networks<NS, DIFFUSE>(T.M, act, lane, q, vq, col);
        // the four lanes of a point hold the same colour: quarter 0 stores it
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (lane < 16 && idx[s] < T.n) {
#pragma unroll
                for (int k = 0; k < 3; ++k) T.out[idx[s] * 3 + k] = col[s][k];
            }
    }
}

// what this translation unit needs of a handle (struct ngf_uv lives in ngf_uv.hip)
const UvArgs &uv_handle_args(const ::ngf_uv *m, int *num_cus);

}  // namespace ngf
