// ngf_uv_query.hpp -- the UV-Mapping (NeuTex) networks at explicit world points: what the reference's net_geometry_decoder(pts)["density"]
// (decoder.py:219-237), gauge_transform(pts) (gauge_fields.py:60-74) and net_texture(uv, view) (decoder.py:56-121) give, without a ray around them.
//
// The geometry and the gauge network are the render kernel's (uv_networks in ngf_uv.hpp, fp32, one wave per SIMD) restated layer for layer from the
// same building blocks -- store_pe, dense, hidden_run, dense_out, uv_wprefetch, out_prefetch; same k-step order, same accumulation order, same
// softplus / normalise / tanh epilogues -- and the texture network is uv_texture_networks of ngf_uv_export.hpp.  The work split is the texture
// export's: four waves per block, one per SIMD, two 16-point tiles per wave pass, passes p = wave, wave + n_waves, ... (static: every point costs
// the same), no queue head, no atomics.  A tail's padding lanes evaluate the last point again and store nothing.
//
// Three parts, chosen at compile time; a part that is not asked for does not run:
//   GEO    sigma = softplus(geometry(PE10(p)))                 671 744 MAC per point
//   GAUGE  uv = normalize(gauge(PE10(p))) | tanh(..)            45 376 | 45 248 MAC per point (sphere | square)
//   TEX    colour at (uv, view), view or diffuse mode (needs GAUGE), through the edit stage as in uv_texture_networks
// A point's value of an output is the same bits in every instantiation that produces it, whatever the launch size and the point's place in the
// list: each part is one inlined copy of the same source, and no part reads what another left in registers -- the gauge starts from its own copy
// of PE10(p) in LDS rows 64..79, the texture from uv.
//
// Two point sources: a list xyz [n,3], or (GEO only) a lattice the kernel generates itself -- point (i,j,k) of linear index (i ny + j) nz + k is
// lo + float(i,j,k) * step with a separately rounded multiply and add, so a float32 restatement on the host has the same points bit for bit.
// Clip (default): sigma is exactly 0 where not all |p_k| < 1 -- the render's strict in-cube test (renderer.py:137-139); uv and colour never are.
#pragma once
#include "ngf_uv_export.hpp"

namespace ngf {

struct UvQueryArgs {
    UvArgs M;              // the handle's prototype: packed weights, their offsets, sphere / square, the edit texture
    const float *xyz;      // [n,3] (list source)
    const float *view;     // [3] (view_stride 0) or [n,3] (view_stride 3); unused without TEX and in diffuse mode
    float *sigma;          // [n] (GEO)
    float *uv;             // [n,3] (GAUGE; z = 0 for square models) or NULL: the gauge runs for the colour alone
    float *rgb;            // [n,3] (TEX)
    int64_t n;
    int32_t view_stride, clip;
    int32_t ny, nz;        // lattice source: n = nx ny nz
    float lo[3], step[3];
};

constexpr int kUvQueryNoTex = 0, kUvQueryTexView = 1, kUvQueryTexDiffuse = 2;

// geometry and / or gauge for NS x 16 points; p: the position of the lane's point in each tile.  sigma and uv are identical in the 4 lanes of a point.
template <int NS, bool GEO, bool GAUGE>
__device__ __forceinline__ void uv_point_networks(const UvArgs &A, float *act, int lane, const float p[NS][3], float sigma[NS], float uv[NS][3])
{
    // (opaque zero offset + lane id once per pass: see uv_networks)
    int wz = 0;
    asm volatile("" : "+s"(wz), "+v"(lane));
    const float *W = A.w + wz;
    if constexpr (GEO) {
        // geometry: 63 -> 256 -> (10x) 256 -> 1, ReLU.  PE10(p) goes to rows 0..15 and (with GAUGE) to rows 64..79, where the gauge network finds it
        f32x4 x[NS][16];
        KStepA<16, NS> pre[4];
        uv_wprefetch<16, NS>(W + A.geo_w0, lane, pre);
        store_pe<3, 10, NS>(act, 0, 16, lane, p, GAUGE ? 64 : -1);
        dense<16, NS, true>(W + A.geo_w0, W + A.geo_b0, 16, lane, act, x, 1 << 30, pre, true);
        uv_wprefetch<16, NS>(W + A.geo_wh, lane, pre);
        store_act<16, NS, kUvActNone>(act, lane, x);
        UvOutW<64> ow;
        hidden_run<NS, false, 0, true>(A, W + A.geo_wh, W + A.geo_qh, W + A.geo_bh, 10, lane, act, x, W + A.geo_wo, ow, pre, true);
        f32x4 o[NS];
        dense_out<NS, 64, 0, true>(ow, W + A.geo_bo, lane, act, o);
#pragma unroll
        for (int s = 0; s < NS; ++s) sigma[s] = o[s][0] > 20.0f ? o[s][0] : log1pf(expf(o[s][0]));
    } else {
        store_pe<3, 10, NS>(act, 64, 16, lane, p);
    }
    if constexpr (GAUGE) {
        // gauge: 63 -> 64 -> 128 -> 128 -> 128 -> 3|2, ReLU (first layer on PE10(p) in rows 64..79)
        f32x4 g4[NS][4], g[NS][8];
        dense<4, NS, true>(W + A.ga_w0, W + A.ga_b0, 16, lane, act + 64 * 64, g4);
        store_act<4, NS, kUvActNone>(act, lane, g4);
        dense<8, NS, true, 0>(W + A.ga_w1, W + A.ga_b1, 16, lane, act, g);
        store_act<8, NS, kUvActNone>(act, lane, g);
        dense<8, NS, true, 0>(W + A.ga_w2, W + A.ga_b2, 32, lane, act, g);
        store_act<8, NS, kUvActNone>(act, lane, g);
        dense<8, NS, true, 0>(W + A.ga_w3, W + A.ga_b3, 32, lane, act, g);
        store_act<8, NS, kUvActNone>(act, lane, g);
        UvOutW<32> ow;
        out_prefetch<32>(W + A.ga_wo, lane, ow);
        __builtin_amdgcn_sched_barrier(0);
        f32x4 q[NS];
        dense_out<NS, 32, 0, true>(ow, W + A.ga_bo, lane, act, q);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (A.sphere) {
                float nrm = sqrtf((q[s][0] * q[s][0] + q[s][1] * q[s][1]) + q[s][2] * q[s][2]);
                nrm = fmaxf(nrm, 1e-12f);
                uv[s][0] = q[s][0] / nrm; uv[s][1] = q[s][1] / nrm; uv[s][2] = q[s][2] / nrm;
            } else {
                uv[s][0] = tanhf(q[s][0]); uv[s][1] = tanhf(q[s][1]); uv[s][2] = 0.0f;
            }
        }
    }
}

template <bool GEO, bool GAUGE, int TEX, bool LATTICE>
__global__ void __launch_bounds__(256) uv_query_kernel(const UvQueryArgs Q)
{
    static_assert(GEO || GAUGE, "a part must run");
    static_assert(TEX == kUvQueryNoTex || GAUGE, "the texture is evaluated at the gauge's uv");
    static_assert(!LATTICE || (GEO && !GAUGE), "the lattice source serves the density alone");
    constexpr int NS = kUvTexTiles;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    float *act = smem + (threadIdx.x >> 6) * (NS * kUvWaveLds);
    const int64_t passes = (Q.n + kUvTexPass - 1) / kUvTexPass, stride = (int64_t)gridDim.x * 4;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < passes; p += stride) {
        float q[NS][3], vq[NS][3], sg[NS], uv[NS][3], col[NS][3];
        int64_t idx[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            idx[s] = p * kUvTexPass + 16 * s + (lane & 15);
            const int64_t i = idx[s] < Q.n ? idx[s] : Q.n - 1;          // a tail's padding lanes evaluate the last point again; nothing of theirs is stored
            if constexpr (LATTICE) {
                const int64_t ij = i / Q.nz;
                const int c[3] = {(int)(ij / Q.ny), (int)(ij % Q.ny), (int)(i % Q.nz)};
#pragma unroll
                for (int k = 0; k < 3; ++k) q[s][k] = __fadd_rn(Q.lo[k], __fmul_rn((float)c[k], Q.step[k]));
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) q[s][k] = Q.xyz[i * 3 + k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) vq[s][k] = TEX == kUvQueryTexView ? Q.view[i * Q.view_stride + k] : 0.0f;
        }
        uv_point_networks<NS, GEO, GAUGE>(Q.M, act, lane, q, sg, uv);
        if constexpr (TEX != kUvQueryNoTex) uv_texture_networks<NS, TEX == kUvQueryTexDiffuse>(Q.M, act, lane, uv, vq, col);
        // the four lanes of a point hold the same values: quarter 0 stores them
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (lane < 16 && idx[s] < Q.n) {
                if constexpr (GEO) {
                    const bool in = fabsf(q[s][0]) < 1.0f && fabsf(q[s][1]) < 1.0f && fabsf(q[s][2]) < 1.0f;
                    Q.sigma[idx[s]] = (Q.clip && !in) ? 0.0f : sg[s];
                }
                if (GAUGE && Q.uv) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) Q.uv[idx[s] * 3 + k] = uv[s][k];
                }
                if constexpr (TEX != kUvQueryNoTex) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) Q.rgb[idx[s] * 3 + k] = col[s][k];
                }
            }
    }
}

}  // namespace ngf
