// ngf_mlp_image.hpp -- host code that turns the decoder weights into the LDS images (and the two streamed packs) of ngf_mlp_layout.hpp.
// Host only: the layouts, the public constants of include/ngf.h and the standard library -- no HIP -- so that tests/host/mlp_image_main.cpp
// builds every image on the CPU (tests/test_mlp_image_cpu.py compares them word for word with tests/golden/mlp_images.npz).
//
// Every image is made of the same few blocks, each written by ONE function here: a matrix as fp32 k-steps (ksteps_f32) or as split-bf16 A
// fragments (frags_bf16), and the bias / output-layer tables (mlp_tail).  What differs between the formulations is which column of
// [W1' | view | pad] a lane's j-th layer-1 input is -- the column maps in build_field_images -- and the layout struct that says where the
// blocks go.  A new formulation adds its layout to ngf_mlp_layout.hpp, a column map and a branch of build_field_images, and a configuration
// to tests/host/mlp_image_main.cpp.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ngf.h"      // NGF_MODEL_*, NGF_F_* (plain C)
#include "ngf_mlp_layout.hpp"

namespace ngf {

// The decoder weights on the host, as ngf_field_create reads them back.  w1p = W1' = W1[:, :F] . basis [64][F] (fold_w1_basis_kernel; unused with
// NGF_F_NO_FOLD, which takes basis [F][F] instead); w1 [64][F + 15]; d*: the density MLP (TriPlane: dw1 [48], db1 [1], placed by create itself).
struct FieldWeights {
    std::vector<float> basis, w1p, w1, b1, w2, b2, w3, b3;
    std::vector<float> dw1, db1, dw2, db2, dw3, db3;
};

// ---- NGF_F_SPLIT_BF16 / NGF_UV_F_SPLIT_BF16: bf16 round-to-nearest-even and the 3-term split of a weight, x = hi + mid + lo (the two
// subtractions are exact in fp32).  A NaN stays a (quiet) NaN in every part: also in the InfoInv density image, whose builder used to
// round a NaN like a number (into an infinity or a zero for some payloads).  For finite weights nothing changed.
inline uint16_t f2bf(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf2f(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline void split3(float x, uint16_t out[3])
{
    out[0] = f2bf(x);
    const float r1 = x - bf2f(out[0]);
    out[1] = f2bf(r1);
    const float r2 = r1 - bf2f(out[1]);
    out[2] = f2bf(r2);
}

// hidden(mt, r, kq), the accumulator order of the 16-row tiles, is ngf_mlp_layout.hpp's (the device packer of ngf_uv_pack.hpp calls it too).
// The same for the 32-row tiles of InfoInv's density MLP, lane (i, hi): the unit of the lane half's k-th accumulator
inline int dens_hidden(int k, int hi) { return (k & 3) + 8 * (k >> 2) + 4 * hi; }

// ---- the blocks ------------------------------------------------------------------------------------------------------------------------
// Lane l of a tile of `rows` output units (16: lane (i, kq); 32: lane (i, hi)) holds row n = mt * rows + l % rows and supplies the inputs of
// lane group q = l / rows; w(n, j, q) = the weight of unit n for the j-th input that group supplies.

// fp32 A operands [MT][KT k-steps][64 lanes]: one conflict-free ds_read_b32 per MFMA
template <typename Wt>
inline void ksteps_f32(float *dst, int MT, int rows, int KT, Wt w)
{
    for (int mt = 0; mt < MT; ++mt)
        for (int t = 0; t < KT; ++t)
            for (int l = 0; l < 64; ++l) dst[((size_t)mt * KT + t) * 64 + l] = w(mt * rows + l % rows, t, l / rows);
}

// split-bf16 A fragments [MT][KB k-blocks][parts][64 lanes][8 bf16]: element e of k-block kb is input j = 8 kb + e.  parts = 3, or 2 with the
// lo parts in the streamed image lo [KB][MT][64 lanes][8 bf16] (InfoInv's layer 1: the term that only meets x.hi)
template <typename Wt>
inline void frags_bf16(float *dst, int MT, int rows, int KB, int parts, float *lo, Wt w)
{
    uint16_t *h16 = reinterpret_cast<uint16_t *>(dst), *l16 = reinterpret_cast<uint16_t *>(lo);
    for (int mt = 0; mt < MT; ++mt)
        for (int kb = 0; kb < KB; ++kb)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    uint16_t p3[3];
                    split3(w(mt * rows + l % rows, kb * 8 + e, l / rows), p3);
                    for (int part = 0; part < parts; ++part) h16[((((size_t)mt * KB + kb) * parts + part) * 64 + l) * 8 + e] = p3[part];
                    if (lo) l16[(((size_t)kb * MT + mt) * 64 + l) * 8 + e] = p3[2];
                }
}

// The fp32 tables behind the matrices, in accumulator order: B1, B2 [groups][16], W3 [outs][groups][16], B3 [4] (zero behind the outs).
// unit(k, q) = the unit of lane group q's k-th accumulator; the colour MLP has 4 groups and 3 outputs, the density MLP 2 and 1.
struct TailAt { int B1, B2, W3, B3; };
template <typename L>
constexpr TailAt tail_at() { return {L::B1, L::B2, L::W3, L::B3}; }
template <typename Unit>
inline void mlp_tail(float *img, TailAt at, int groups, int outs, Unit unit, const std::vector<float> &b1, const std::vector<float> &b2,
                     const std::vector<float> &w3, const std::vector<float> &b3)
{
    const int units = groups * 16;
    for (int q = 0; q < groups; ++q)
        for (int k = 0; k < 16; ++k) {
            const int n = unit(k, q);
            img[at.B1 + q * 16 + k] = b1[n];
            img[at.B2 + q * 16 + k] = b2[n];
            for (int c = 0; c < outs; ++c) img[at.W3 + c * units + q * 16 + k] = w3[(size_t)c * units + n];
        }
    for (int c = 0; c < 4; ++c) img[at.B3 + c] = c < outs ? b3[c] : 0.0f;
}

// Row n of [P | view | pad], the inputs of rgb_decoder's layer 1: P = W1' = W1[:, :F] . basis (basis has no bias and no activation,
// networks.py:17,26; folded on the device by fold_w1_basis_kernel) or, with NGF_F_NO_FOLD, W1[:, :F] itself; view = W1[:, F:F+15]; column
// F + 15 is the zero pad that fills the sixteenth view entry.
struct Layer1Rows {
    int F;
    const float *plane;
    int plane_stride;
    const float *w1;
    float at(int n, int col) const { return col < F ? plane[(size_t)n * plane_stride + col] : col < F + 15 ? w1[(size_t)n * (F + 15) + col] : 0.0f; }
};

// A colour image of layout L: sizes img (dens_floats more for what follows the colour image), writes layer 1 at img + w1_at from the column
// map col(j, kq) -- K1 fp32 k-steps (parts1 = 0) or K1 k-blocks of parts1 bf16 parts -- then layer 2 and the tables.  Returns the end of the image.
template <typename L, typename Col>
inline float *colour_image(std::vector<float> &img, int dens_floats, int w1_at, int K1, int parts1, float *lo, bool bf16_layer2,
                           const Layer1Rows &rows, Col col, const FieldWeights &W)
{
    img.assign((size_t)L::TOTAL + dens_floats, 0.0f);
    auto w1 = [&](int n, int j, int kq) { return rows.at(n, col(j, kq)); };
    auto w2 = [&](int n, int j, int kq) { return W.w2[(size_t)n * 64 + hidden(j >> 2, j & 3, kq)]; };
    if (parts1) frags_bf16(img.data() + w1_at, 4, 16, K1, parts1, lo, w1);
    else ksteps_f32(img.data() + w1_at, 4, 16, K1, w1);
    if (bf16_layer2) frags_bf16(img.data() + L::W2, 4, 16, 2, 3, nullptr, w2);
    else ksteps_f32(img.data() + L::W2, 4, 16, 16, w2);
    mlp_tail(img.data(), tail_at<L>(), 4, 3, [](int k, int kq) { return hidden(k >> 2, k & 3, kq); }, W.b1, W.b2, W.w3, W.b3);
    return img.data() + L::TOTAL;
}

// InfoInv's density MLP 72-32-32-1 (ngf_infoinv.hpp: on the matrix cores inside the march), layout D.  fp32 (v_mfma_f32_32x32x2_f32): k-step t of
// lane half hi is input 2 t + hi.  bf16 (v_mfma_f32_32x32x16_bf16): element e of k-block kb is input 16 kb + 8 hi + e, 72 .. 79 zero pads.
// Layer 2 takes the hidden units in the accumulator order of the lane half either way.
template <typename D>
inline void density_image(float *img, bool bf16, const FieldWeights &W)
{
    auto w2 = [&](int n, int j, int hi) { return W.dw2[(size_t)n * 32 + dens_hidden(j, hi)]; };
    if (bf16) {
        frags_bf16(img + D::D1, 1, 32, 5, 3, nullptr, [&](int n, int j, int hi) {
            const int k = 16 * (j >> 3) + 8 * hi + (j & 7);
            return k < 72 ? W.dw1[(size_t)n * 72 + k] : 0.0f;
        });
        frags_bf16(img + D::D2, 1, 32, 2, 3, nullptr, w2);
    } else {
        ksteps_f32(img + D::D1, 1, 32, 36, [&](int n, int t, int hi) { return W.dw1[(size_t)n * 72 + 2 * t + hi]; });
        ksteps_f32(img + D::D2, 1, 32, 16, w2);
    }
    mlp_tail(img, tail_at<D>(), 2, 1, dens_hidden, W.db1, W.db2, W.dw3, W.db3);
}

// NGF_F_NO_FOLD: the basis matrix [F][F] packed for streaming, [36 k-steps][3 groups of 4 unit tiles][64 lanes][4].  k-step t = P*12 + j takes
// colour channel P*48 + 16*(j/4) + 4kq + (j&3) (the gather order of mlp_pass16); output unit tile mt (9 tiles), group mt/4, element mt%4.
inline void basis_pack(int F, const std::vector<float> &basis, std::vector<float> &bpack)
{
    const int APPc = F / 3, QCH = APPc / 4;
    bpack.assign(kBasisPackFloats, 0.0f);
    for (int t = 0; t < 36; ++t)
        for (int mt = 0; mt < 9; ++mt)
            for (int l = 0; l < 64; ++l) {
                const int kq = l >> 4, j = t % QCH;
                const int ch = (t / QCH) * APPc + 16 * (j / 4) + 4 * kq + (j & 3);
                bpack[(((size_t)t * 3 + mt / 4) * 64 + l) * 4 + (mt & 3)] = basis[(size_t)(mt * 16 + (l & 15)) * F + ch];
            }
}

// Sizes and fills img (the colour image, then InfoInv's density image) and pack (NGF_F_NO_FOLD: the level-0 basis pack; InfoInv
// NGF_F_SPLIT_BF16: layer 1's lo parts; empty otherwise) for a (model, flags) pair that ngf_field_create has validated.
inline void build_field_images(int model, int flags, const FieldWeights &W, std::vector<float> &img, std::vector<float> &pack)
{
    const bool tri = model == NGF_MODEL_TRIPLANE, split = flags & NGF_F_SPLIT_BF16;
    const int F = tri ? 144 : 216, APPc = F / 3;
    const Layer1Rows folded{F, W.w1p.data(), F, W.w1.data()}, unfolded{F, W.w1.data(), F + 15, W.w1.data()};
    // The column maps: input j of lane quarter kq -> column of [P | view | pad].  The quarter's four view inputs are entries 4 kq .. 4 kq + 3 of
    // [d, sin, cos, 0] (view_entries16) and always come last.
    auto view = [F](int e, int kq) { return F + 4 * kq + e; };
    // TriPlane, levels 1-2 (fp32 k-steps and bf16 k-blocks alike): 12 channels of each plane, channel 16 q + 4 kq + e -- the gather order of mlp_pass16
    auto tri_col = [=](int j, int kq) { return j < 36 ? (j / 12) * APPc + 16 * ((j % 12) / 4) + 4 * kq + (j & 3) : view(j - 36, kq); };
    // level 3: layer 1's plane part is baked into the textures (bake_color_kernel, natural unit order); only the view inputs remain
    auto baked_col = [=](int j, int kq) { return view(j, kq); };
    // level 0: layer 1 on the 144 outputs of the basis stage, which land in accumulator order
    auto nofold_col = [=](int j, int kq) { return j < 36 ? hidden(j >> 2, j & 3, kq) : view(j - 36, kq); };
    // InfoInv (fp32 k-steps and bf16 k-blocks alike): 18 channels of each plane in the PACKED channel order (infoinv_split_channel), the view inputs,
    // and in the bf16 form 6 zero pads up to the eighth k-block
    auto ii_col = [=](int j, int kq) { return j < 54 ? (j / 18) * APPc + infoinv_split_channel(kq * 18 + j % 18) : j < 58 ? view(j - 54, kq) : F + 15; };

    pack.clear();
    if (!tri && split) {
        using L = MlpLayoutBf16II;
        pack.assign(kW1LoPackII, 0.0f);
        density_image<InfoInvDensLayoutBf16>(colour_image<L>(img, InfoInvDensLayoutBf16::TOTAL, L::W1, L::KB1, 2, pack.data(), true, folded, ii_col, W), true, W);
    } else if (!tri) {
        using L = MlpLayout16<72>;
        density_image<InfoInvDensLayout>(colour_image<L>(img, InfoInvDensLayout::TOTAL, L::W1, L::KT, 0, nullptr, false, folded, ii_col, W), false, W);
    } else if (flags & NGF_F_NO_FOLD) {
        using L = MlpLayout16NoFold;
        colour_image<L>(img, 0, L::W1, L::KT, 0, nullptr, false, unfolded, nofold_col, W);
        basis_pack(F, W.basis, pack);
    } else if (flags & NGF_F_BAKE_COLOR) {      // with NGF_F_SPLIT_BF16: layer 2 as bf16 fragments, the view k-steps stay fp32 where they are
        if (split) colour_image<MlpLayout16BakedBf16>(img, 0, MlpLayout16BakedBf16::W1V, 4, 0, nullptr, true, folded, baked_col, W);
        else colour_image<MlpLayout16Baked>(img, 0, MlpLayout16Baked::W1V, 4, 0, nullptr, false, folded, baked_col, W);
    } else if (split) {
        using L = MlpLayoutBf16;
        colour_image<L>(img, 0, L::W1, L::KB1, 3, nullptr, true, folded, tri_col, W);
    } else {
        using L = MlpLayout16<48>;
        colour_image<L>(img, 0, L::W1, L::KT, 0, nullptr, false, folded, tri_col, W);
    }
}

}  // namespace ngf
