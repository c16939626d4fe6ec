// ngf_query.hpp -- point queries (ngf_field_query): density, colour and gauge-shifted plane coordinates of a field at arbitrary world-space points.
// Included by ngf_field.hip only.  The kernel joins the two pieces the library already had -- the density side of alpha_kernel (P::sigma: 64 points
// per wave, one per lane) and the colour side of decode_rgb_kernel (P::shade: 16 samples per matrix pass, four lanes per sample) -- so that the
// coordinates never travel through HBM between them.  DESIGN.md section 4.10.
//
// Two policies, because the two sides of a handle are picked independently (launch_alpha by NGF_F_BAKE_DENSITY / gauge_same, ngf_field_decode_rgb by
// the colour flags): PD supplies sigma(), PC supplies shade().  PC = NoColour is the kernel without a colour stage: no shade code, no view slab,
// and for TriPlane no LDS at all.
//
// Per wave tile of 64 consecutive points:
//   load      p, one point per lane (lanes past n re-read point n - 1 and store nothing)
//   box test  in_box = all(a0 <= p) && all(p <= a1): sample_ray's test (FieldBase.py:134) for every ordered input, and false for NaN
//   sanitise  a lane that is not in the box continues with the box centre (and a zero direction): every texel index and every matrix operand below is
//             then in range by construction, whatever the caller passed (NaN, +-inf, 3e38); its outputs are exact zeros
//   density   sigma = PD::sigma(...), called by all 64 lanes.  TriPlane zeroes t[] for invalid lanes and the coordinates belong to every in-box point,
//             masked or not: sigma is evaluated for in_box and the alpha mask applied to the result.  InfoInv's t[] does not depend on `valid`, so the
//             mask goes into `valid` and a wave whose points are all masked skips the density MLP.
//   colour    four shade passes; in pass k lane (s = lane & 15, kq = lane >> 4) works for point 16 k + s of the tile: its record {0, 1, t[0..5]} and its
//             direction come from lane 16 k + s by __shfl, lanes < 16 write the 16 view inputs of their point to the wave's LDS slab, PC::shade runs
//             with all lanes active and lanes < 16 store sigmoid(logit).  A pass is skipped only when none of its 16 points is in the box (ballot:
//             wave-uniform).  A sample is one column of the pass's matrix products, so its colour depends on its own record and direction only.
// No atomics, no cross-workgroup communication: a point's outputs depend on that point and the handle alone.
#pragma once
#include "ngf_infoinv.hpp"
#include "ngf_render.hpp"

namespace ngf {

struct QueryArgs {
    const float *xyz;      // [n,3]
    const float *dirs;     // [n,3] (dir_stride 3), [3] (dir_stride 0) or NULL (no colour)
    int64_t n;
    int32_t dir_stride;
    int32_t use_mask;      // 0: NGF_QUERY_NO_MASK
    float *sigma;          // [n] or NULL
    float *rgb;            // [n,3] or NULL
    float *coords;         // [n,6] or NULL
};

struct NoColour {};        // PC of the kernels without a colour stage

constexpr int kQueryViewFloats = 32 * kViewFeat;        // the wave's view slab (decode_rgb_kernel's carve)

// Waves per SIMD the register allocation aims at: the residency of the decode_rgb_kernel of the same colour policy -- three waves per SIMD (168
// registers) for the fp32 passes and level 3's bf16 pass, two for the split-bf16 passes of levels 1 / 2 and of InfoInv (~200 registers), one for the
// un-composed level 0.  With plain __launch_bounds__(256) hipcc took 150 + 32 registers for the fp32 passes, two waves per SIMD.  (Measured: the level-3
// query of 2^20 points took 0.494 ms before and 0.493 ms after -- the colour stage's residency is not what makes it 5 % slower than ngf_field_alpha +
// ngf_field_decode_rgb)
template <typename PD, typename PC>
constexpr int query_waves_per_simd()
{
    constexpr bool TAPS16 = std::is_same_v<PD, TriPlanePolicy<false, false, 8, 1>>;      // level 0 / 1 density: 16-channel taps, alpha_kernel's 166 registers
    if (std::is_same_v<PC, NoColour>) return 1;           // no constraint (with 3 the 16-channel taps spill 36 B per lane; the others are far below any limit)
    if (std::is_same_v<PC, TriPlaneNoFoldPolicy>) return 1;
    if (TAPS16) return 2;                                 // at 168 registers the taps next to a colour pass spill ~100 B per lane
    if (std::is_same_v<PC, TriPlaneBf16Policy<false, 8>> || std::is_same_v<PC, InfoInvSplitPolicy> || std::is_same_v<PD, InfoInvSplitPolicy>) return 2;
    return 3;
}

template <typename PD, typename PC>
__global__ void __launch_bounds__(256, (query_waves_per_simd<PD, PC>())) query_kernel(const RenderArgs A, const QueryArgs Q)
{
    constexpr bool COLOUR = !std::is_same_v<PC, NoColour>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    NGF_KARG_CONTRACT((&query_kernel<PD, PC>));
    if (karg_tex(offsetof(RenderArgs, dens)).p != A.dens[0].p) __builtin_trap();      // the RenderArgs must be the first kernel argument (karg_tex)
    if constexpr (COLOUR || PD::INFOINV) {
        if (COLOUR || Q.sigma) {          // an InfoInv coords-only call needs no MLP: nothing is staged (the launch reserves no LDS for it)
            stage_blob(smem, A.blob, A.blob_floats);
            __syncthreads();
        }
    }
    const int lane = threadIdx.x & 63;
    [[maybe_unused]] const int wave = threadIdx.x >> 6;
    const int64_t n = Q.n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < n; base += stride) {
        const int64_t i = base + lane;
        const bool live = i < n;
        const int64_t ii = live ? i : n - 1;
        float p[3] = {Q.xyz[ii * 3], Q.xyz[ii * 3 + 1], Q.xyz[ii * 3 + 2]};
        bool in_box = live;
#pragma unroll
        for (int k = 0; k < 3; ++k) in_box = in_box && (p[k] >= A.a0[k] && p[k] <= A.a1[k]);
        float x[3], t[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = in_box ? p[k] : 0.5f * (A.a0[k] + A.a1[k]);
            x[k] = (p[k] - A.a0[k]) * A.inv[k] - 1.0f;      // normalize_coord, as alpha_kernel
        }
        bool occupied = in_box;
        if (A.mask.bits && Q.use_mask && in_box) occupied = mask_occupied(A.mask, p);
        const bool dens_valid = PD::INFOINV ? (occupied && Q.sigma != nullptr) : in_box;
        float sigma = PD::sigma(A, smem, dens_valid, x, lane, t);
        sigma = occupied ? sigma : 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) t[k] = in_box ? t[k] : 0.0f;
        if (live) {
            if (Q.sigma) Q.sigma[i] = sigma;
            if (Q.coords) {
#pragma unroll
                for (int k = 0; k < 6; ++k) Q.coords[i * 6 + k] = t[k];
            }
        }
        if constexpr (COLOUR) {
            float *vfeat = smem + ((A.blob_floats + 3) & ~3) + wave * kQueryViewFloats;
            const int64_t di = Q.dir_stride ? ii * 3 : 0;
            float d[3] = {Q.dirs[di], Q.dirs[di + 1], Q.dirs[di + 2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = in_box ? d[k] : 0.0f;
            const unsigned long long boxed = __ballot(in_box);
            const int s = lane & 15;
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int src = 16 * k + s;
                float c[3] = {0.0f, 0.0f, 0.0f};
                if ((boxed >> (16 * k)) & 0xffffull) {          // wave-uniform: a pass with no in-box point among its 16 only stores its zeros
                    const float rec[kRecFloats] = {0.0f, 1.0f, __shfl(t[0], src), __shfl(t[1], src), __shfl(t[2], src),
                                                   __shfl(t[3], src), __shfl(t[4], src), __shfl(t[5], src)};
                    const float dq[3] = {__shfl(d[0], src), __shfl(d[1], src), __shfl(d[2], src)};
                    if (lane < 16) {
                        float v[16];
                        view_inputs(dq, v);
                        f32x4 *dst = reinterpret_cast<f32x4 *>(vfeat + s * kViewFeat);
#pragma unroll
                        for (int j = 0; j < 4; ++j) dst[j] = f32x4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    PC::shade(A, smem, rec, vfeat + s * kViewFeat, dq, lane, c);         // logits
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
                const int64_t q = base + src;
                if (lane < 16 && q < n) {
                    const bool qin = (boxed >> src) & 1ull;
#pragma unroll
                    for (int j = 0; j < 3; ++j) Q.rgb[q * 3 + j] = qin ? sigmoid_rcp(c[j]) : 0.0f;
                }
            }
        }
    }
}

}  // namespace ngf
