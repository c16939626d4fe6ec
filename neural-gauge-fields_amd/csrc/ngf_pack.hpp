// ngf_pack.hpp -- the kernels that ngf_field.hip (field handles) and ngf_train.hip (the TriPlane trainer) both launch: plane packing and the
// alpha mask's cell image.  `static`: two translation units of one library include this, neither may export the kernels' symbols.
#pragma once
#include "ngf_device.hpp"
#include "ngf_infoinv.hpp"        // infoinv_split_channel

namespace ngf {

// NCHW [C,H,W] channels [c0,c0+nc) -> zero-bordered channel-last [(H+2)][(W+2)][nc]
// perm = 1: the colour channels in the order of infoinv_split_channel (InfoInv NGF_F_SPLIT_BF16, nc = 72)
// pair = 1: the row-pair form (struct Tex, ngf_device.hpp) [(H+2)][(W+2)][2][nc]: slot 0 of padded texel (x, y) holds (x, y), slot 1 holds (x, y + 1) --
// every value is stored twice, as its own texel's slot 0 and as slot 1 of the texel above; the last padded row pairs with zeros.
static __global__ void pack_plane_kernel(const float *__restrict__ src, int H, int W, int c0, int nc, float *__restrict__ dst, int perm = 0, int pair = 0)
{
    const size_t total = (size_t)(H + 2) * (W + 2) * nc;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % nc);
        const size_t tx = i / nc;
        const int x = (int)(tx % (W + 2)), y = (int)(tx / (W + 2));
        float v = 0.0f;
        if (x >= 1 && x <= W && y >= 1 && y <= H) v = src[((size_t)(c0 + (perm ? infoinv_split_channel(c) : c)) * H + (y - 1)) * W + (x - 1)];
        if (pair) {
            dst[tx * 2 * nc + c] = v;
            if (y >= 1) dst[((tx - (W + 2)) * 2 + 1) * nc + c] = v;
            if (y == H + 1) dst[(tx * 2 + 1) * nc + c] = 0.0f;
        } else dst[i] = v;
    }
}

// Rows of a packed plane of H rows as allocated: the padded rows 0 .. H + 1, in both forms (the row-pair form doubles the texel, not the rows).  The march's
// cells start at padded (cx, cy) in [0, W] x [0, H] (bil_setup) and read texels idx, idx + 1 of row cy -- and, in the one-row form, of row cy + 1.
static inline size_t packed_plane_floats(int H, int W, int nc, bool pair) { return (size_t)(H + 2) * (W + 2) * nc * (pair ? 2 : 1); }

// Alpha mask, second image (round 6): per trilinear cell -- base corner (z, y, x) in -1 .. D-1 / H-1 / W-1 -- one byte with the bits of its 8 corners
// (bit dz*4 + dy*2 + dx; corners outside the volume are 0 = grid_sample's zeros padding), so that mask_occupied needs ONE gather per sample.
static __global__ void __launch_bounds__(256) mask_cells_kernel(const uint8_t *__restrict__ bits, int D, int H, int W, uint8_t *__restrict__ cells)
{
    ngf::MaskVol m{};
    m.bits = bits; m.D = D; m.H = H; m.W = W;
    const size_t total = (size_t)(D + 1) * (H + 1) * (W + 1);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % (size_t)(W + 1)) - 1, y = (int)((i / (size_t)(W + 1)) % (size_t)(H + 1)) - 1, z = (int)(i / ((size_t)(W + 1) * (H + 1))) - 1;
        unsigned c = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) c |= (unsigned)ngf::mask_bit(m, z + (k >> 2), y + ((k >> 1) & 1), x + (k & 1)) << k;
        cells[i] = (uint8_t)c;
    }
}

}  // namespace ngf
