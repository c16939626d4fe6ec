// ngf_uv_occupancy.hpp -- the occupancy grid of a NeuTex handle: nx x ny x nz cells over the cube [-1,1]^3, one bit per cell (1 = occupied), cell
// (cx,cy,cz) at linear index (cx ny + cy) nz + cz (the C order of ngf_uv_density_lattice), packed like np.packbits -- most significant bit first,
// as ngf_pack_mask_bits packs.  The ONE look-up the render kernel (ngf_uv.hpp, OCC instantiations), ngf_uv_occupancy_lookup and the trainer
// (ngf_uv_train.hpp, the OCC forms of uvt_rays_kernel and uvt_compact_kernel) share.
//
// Nearest cell, not the fields' trilinear alpha test: a sample asks one bit, so that "occupied" is a property of a cell a test can restate and a
// dilated mask is conservative by construction.
#pragma once
#include <cstdint>

#include "ngf_device.hpp"

namespace ngf {

// cell of coordinate p on an axis of n cells, h = (float)n * 0.5f: min(int(floorf((p + 1) * h)), n - 1), the add and the multiply each rounded
// (written with the _rn intrinsics: no contraction whatever the build flags).  For -1 < p < 1 the sum lies in (0, 2] -- it rounds to 2.0 at
// p = 1 - 2^-24, hence the clamp -- so the cell is in 0 .. n - 1.
__device__ __forceinline__ int uv_occ_cell(float p, float h, int n)
{
    const int c = (int)floorf(__fmul_rn(__fadd_rn(p, 1.0f), h));
    return c < n - 1 ? c : n - 1;
}

// the bit of the cell that holds p.  The caller has checked -1 < p_k < 1 on every axis (the render's strict in-cube test, which NaN fails): the
// byte read lies inside the image of (nx ny nz + 7) / 8 bytes for such a point and for no other.  n_k <= 1024: the index fits 31 bits.
__device__ __forceinline__ bool uv_occ_lookup(const uint8_t *bits, const int32_t n[3], const float h[3], const float p[3])
{
    const int cx = uv_occ_cell(p[0], h[0], n[0]), cy = uv_occ_cell(p[1], h[1], n[1]), cz = uv_occ_cell(p[2], h[2], n[2]);
    const unsigned idx = ((unsigned)cx * (unsigned)n[1] + (unsigned)cy) * (unsigned)n[2] + (unsigned)cz;
    return ((bits[idx >> 3] >> (7u - (idx & 7u))) & 1u) != 0;
}

constexpr int kUvOccMaxAxis = 1024, kUvOccMaxDilate = 2;

}  // namespace ngf
