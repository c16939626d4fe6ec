// ngf_mlp_layout.hpp -- the LDS images of the decoder MLPs and the two streamed packs: the contract between the host code that fills them
// (ngf_mlp_image.hpp) and the render kernels that read them (ngf_shade16.hpp, ngf_shade_bf16.hpp, ngf_infoinv.hpp; the TriPlane trainer's
// forward pass reads MlpLayout16<48> too).  Plain C++: offsets in floats and one index map, no HIP header, so that the builders and their
// CPU test compile with a host compiler alone.  A new formulation puts its layout HERE, its builder into ngf_mlp_image.hpp and its golden into
// tests/test_mlp_image_cpu.py.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define NGF_LAYOUT_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))      // = __host__ __device__ __forceinline__
#else
#define NGF_LAYOUT_HD inline
#endif

namespace ngf {

// ---- ngf_shade16.hpp: v_mfma_f32_16x16x4_f32, lane (s = l & 15, kq = l >> 4) ---------------------------------------------------------
// The hidden unit of accumulator (mt, r) of lane quarter kq.  A lane's 16 ReLU'd accumulators are the next layer's B operands in place, so the
// next layer's j-th input of lane quarter kq is unit hidden(j >> 2, j & 3, kq).
NGF_LAYOUT_HD int hidden(int mt, int r, int kq) { return mt * 16 + 4 * kq + r; }

template <int APP>
struct MlpLayout16 {                      // floats
    static constexpr int QCH = APP / 4;           // colour channels per plane per lane (12)
    static constexpr int KT = 3 * QCH + 4;        // layer-1 k-steps, 4 inputs each (40)
    static constexpr int W1 = 0;                  // [4 mt][KT][64 lanes]
    static constexpr int W2 = W1 + 4 * KT * 64;   // [4 mt][16][64 lanes]
    static constexpr int B1 = W2 + 4 * 16 * 64;   // [4 kq][16]
    static constexpr int B2 = B1 + 64;
    static constexpr int W3 = B2 + 64;            // [3][4 kq][16]
    static constexpr int B3 = W3 + 192;
    static constexpr int TOTAL = B3 + 4;
};

struct MlpLayout16Baked {                 // NGF_F_BAKE_COLOR: only the view-input k-steps of layer 1 remain
    static constexpr int W1V = 0;                 // [4 mt][4][64 lanes]
    static constexpr int W2 = W1V + 4 * 4 * 64;
    static constexpr int B1 = W2 + 4 * 16 * 64;
    static constexpr int B2 = B1 + 64;
    static constexpr int W3 = B2 + 64;
    static constexpr int B3 = W3 + 192;
    static constexpr int TOTAL = B3 + 4;
};

// NGF_F_BAKE_COLOR | NGF_F_SPLIT_BF16 (round 5, opt-in): level 3 with LAYER 2 on the bf16 matrix pipe as 3-term split products (ngf_shade_bf16.hpp
// mlp_pass16_baked_bf16).  Same front part as MlpLayout16Baked (the view-input k-steps at offset 0), then W2 as bf16 A fragments
// [4 mt][2 k-blocks][3 parts][64 lanes][8 bf16] (= 4 floats per fragment), then the fp32 tables.
struct MlpLayout16BakedBf16 {
    static constexpr int W1V = 0;                 // [4 mt][4][64 lanes] fp32
    static constexpr int W2 = W1V + 4 * 4 * 64;   // bf16 fragments: 4 x 2 x 3 x 64 x 4 floats
    static constexpr int B1 = W2 + 4 * 2 * 3 * 64 * 4;
    static constexpr int B2 = B1 + 64;
    static constexpr int W3 = B2 + 64;
    static constexpr int B3 = W3 + 192;
    static constexpr int TOTAL = B3 + 4;
};

// NGF_F_NO_FOLD (ngf_shade16.hpp, level 0): the basis matrix (83 KB) does not fit LDS next to the layers and is streamed from L2
struct MlpLayout16NoFold {                 // LDS image (floats): layer 1 on [g(144) | view(16)] in accumulator order, then as MlpLayout16
    static constexpr int KT = 40;
    static constexpr int W1 = 0;                  // [4 mt][40][64]
    static constexpr int W2 = W1 + 4 * KT * 64;
    static constexpr int B1 = W2 + 4 * 16 * 64;
    static constexpr int B2 = B1 + 64;
    static constexpr int W3 = B2 + 64;
    static constexpr int B3 = W3 + 192;
    static constexpr int TOTAL = B3 + 4;
};
constexpr int kBasisPackFloats = 36 * 3 * 64 * 4;      // [36 k-steps][3 groups of 4 unit tiles (9 used)][64 lanes][4]

// ---- ngf_shade_bf16.hpp: v_mfma_f32_16x16x32_bf16, A fragments [mt][k-block][part][lane][8 bf16] ---------------------------------------
struct MlpLayoutBf16 {                        // floats (a bf16x8 fragment = 4 floats)
    static constexpr int KB1 = 5, KB2 = 2;
    static constexpr int W1 = 0;                              // [4 mt][5 kb][3 parts][64 lanes][4]
    static constexpr int W2 = W1 + 4 * KB1 * 3 * 64 * 4;      // [4 mt][2 kb][3 parts][64 lanes][4]
    static constexpr int B1 = W2 + 4 * KB2 * 3 * 64 * 4;      // [4 kq][16] fp32, accumulator order
    static constexpr int B2 = B1 + 64;
    static constexpr int W3 = B2 + 64;                        // [3][4 kq][16] fp32
    static constexpr int B3 = W3 + 192;
    static constexpr int TOTAL = B3 + 4;
};

// ---- ngf_infoinv.hpp -------------------------------------------------------------------------------------------------------------------
struct InfoInvDensLayout {                  // floats, relative to MlpLayout16<72>::TOTAL inside the blob
    static constexpr int D1 = 0;                    // [36 k-steps][64 lanes] : W1[l&31][2t + (l>>5)]
    static constexpr int D2 = D1 + 36 * 64;         // [16 k-steps][64 lanes] : W2[l&31][row(t, l>>5)]
    static constexpr int B1 = D2 + 16 * 64;         // [2 hi][16]
    static constexpr int B2 = B1 + 32;              // [2 hi][16]
    static constexpr int W3 = B2 + 32;              // [2 hi][16]
    static constexpr int B3 = W3 + 32;              // [4]
    static constexpr int TOTAL = B3 + 4;
};

// NGF_F_SPLIT_BF16: the density MLP of the march on v_mfma_f32_32x32x16_bf16 with 3-term split operands (ngf_infoinv.hpp sigma_bf16).
// A fragments: lane (i = l & 31, hi = l >> 5), element e of k-block kb holds W[i][16 kb + 8 hi + e] -- layer 1 over the 72 inputs in
// their natural order (plane p, channel c -> 24 p + c; 8 zero pads), layer 2 over the hidden units in the accumulator order of the lane
// half (k = 8 q + e  ->  unit (k & 3) + 8 (k >> 2) + 4 hi), so that a lane's own ReLU'd accumulators are its B fragments.
struct InfoInvDensLayoutBf16 {              // floats (a bf16x8 fragment = 4 floats), relative to MlpLayoutBf16II::TOTAL inside the blob
    static constexpr int KB1 = 5, KB2 = 2;
    static constexpr int D1 = 0;                    // [5 kb][3 parts][64 lanes][4]
    static constexpr int D2 = D1 + KB1 * 3 * 64 * 4;   // [2 kb][3 parts][64 lanes][4]
    static constexpr int B1 = D2 + KB2 * 3 * 64 * 4;   // [2 hi][16]
    static constexpr int B2 = B1 + 32;
    static constexpr int W3 = B2 + 32;
    static constexpr int B3 = W3 + 32;
    static constexpr int TOTAL = B3 + 4;
};

// NGF_F_SPLIT_BF16, the colour MLP (ngf_infoinv.hpp mlp_pass16_bf16_ii): the hi and mid parts of layer 1 in LDS, its lo parts streamed from L2
struct MlpLayoutBf16II {                      // LDS image (floats); a bf16x8 fragment = 4 floats
    static constexpr int KB1 = 8, KB2 = 2;
    static constexpr int W1 = 0;                              // [4 mt][8 kb][2 parts: hi, mid][64 lanes][4]
    static constexpr int W2 = W1 + 4 * KB1 * 2 * 64 * 4;      // [4 mt][2 kb][3 parts][64 lanes][4]
    static constexpr int B1 = W2 + 4 * KB2 * 3 * 64 * 4;      // [4 kq][16] fp32, accumulator order
    static constexpr int B2 = B1 + 64;
    static constexpr int W3 = B2 + 64;                        // [3][4 kq][16]
    static constexpr int B3 = W3 + 192;
    static constexpr int TOTAL = B3 + 4;
};
constexpr int kW1LoPackII = MlpLayoutBf16II::KB1 * 4 * 64 * 4;      // floats of the streamed image: layer 1's lo parts [kb][mt][lane][8 bf16]
// packed position (0..71) of a plane's colour channels -> channel of the reference layout
NGF_LAYOUT_HD int infoinv_split_channel(int pos)
{
    const int kq = pos / 18, r = pos % 18, g = r / 3, j = r % 3;        // g = hi*3 + axis
    return (g / 3) * 36 + (g % 3) * 12 + 3 * kq + j;
}

}  // namespace ngf
