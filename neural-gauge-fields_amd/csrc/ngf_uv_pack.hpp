// ngf_uv_pack.hpp -- the streamed weight images of ngf_uv.hpp's blocks (kload_wg / out_prefetch / load_bias read them from L2) and the plan of
// the packed inverse network: the one definition of both, for the host packers (ngf_uv.hip's UvPacker, ngf_uv_inverse_create) and the device
// packer (ngf_uv_inverse_train.hpp: uvit_pack_kernel).  Plain C++ as ngf_mlp_layout.hpp: no HIP header, so tests/host/uv_pack_main.cpp compiles
// it with a host compiler alone (tests/test_uv_pack_cpu.py).
//
//   dense  [KT k-steps][NT / 4 tile groups][64 lanes][4]   element e of lane l: unit (4 g + e) 16 + (l & 15), input of k-step t, quarter l >> 4
//   out    [KT / 4][64 lanes][4]                          a layer of <= 16 units (3 used): a lane's A operands of four k-steps in one 16-byte load
//   bias   [4 lane quarters][NT tiles][4]                 accumulator order (load_bias)
//   bias4  [4]                                            the output layer's
// Slots whose unit or input lies outside the layer hold zero.
#pragma once
#include <cstdint>

#include "../../include/ngf.h"      // NGF_UV_INVERSE_LAYERS (plain C)
#include "ngf_mlp_layout.hpp"       // NGF_LAYOUT_HD, hidden()

namespace ngf {

// ---- the slot map ----------------------------------------------------------------------------------------------------------------------------
enum { kUvPackDense = 0, kUvPackOut = 1, kUvPackBias = 2, kUvPackBias4 = 3 };

struct UvPackSlot {
    int o;           // output unit
    int t, kq;       // k-step and lane quarter of the input (dense, out)
};

// word idx of an image of `kind` with NT unit tiles -> the unit it belongs to and where its input comes from
NGF_LAYOUT_HD UvPackSlot uv_pack_slot(int kind, int NT, int idx)
{
    const int e = idx & 3, l = (idx >> 2) & 63, rest = idx >> 8;
    if (kind == kUvPackDense) return {(4 * (rest % (NT / 4)) + e) * 16 + (l & 15), rest / (NT / 4), l >> 4};
    if (kind == kUvPackOut) return {l & 15, 4 * rest + e, l >> 4};
    if (kind == kUvPackBias) return {hidden((idx >> 2) % NT, e, idx / (4 * NT)), 0, 0};
    return {idx, 0, 0};
}

// the input behind k-step t of lane quarter kq: natural order (what a kernel writes itself: coordinates, encodings) or the producing layer's
// accumulator order
NGF_LAYOUT_HD int uv_pack_input(int t, int kq, bool accumulator_order) { return accumulator_order ? hidden(t >> 2, t & 3, kq) : 4 * t + kq; }

// ---- one packed image ------------------------------------------------------------------------------------------------------------------------
// Element (o, i) of the layer a segment packs is src[o so + i si] (so = in, si = 1: W as stored; so = 1, si = the stored row length: its
// transpose).
struct UvPackSeg {
    const float *src;
    int32_t dst, count;      // floats
    int32_t kind;
    int32_t out_f, in_f, so, si;
    int32_t NT;              // unit tiles
    int32_t hid;             // input order: 0 natural, 1 accumulator
    int32_t pad_;
};

NGF_LAYOUT_HD float uv_pack_value(const UvPackSeg &S, int idx)
{
    const UvPackSlot s = uv_pack_slot(S.kind, S.NT, idx);
    if (s.o >= S.out_f) return 0.0f;
    if (S.kind >= kUvPackBias) return S.src[s.o];
    const int i = uv_pack_input(s.t, s.kq, S.hid != 0);
    return i < S.in_f ? S.src[(int64_t)s.o * S.so + (int64_t)i * S.si] : 0.0f;
}

// ---- NeuTex's inverse network (ngf_uv_inverse.hpp) -----------------------------------------------------------------------------------------
constexpr int kUvInvMid = 64, kUvInvHidden = 512, kUvInvHiddenLayers = 2;      // fixed, as gauge_fields.py:83 fixes them
static_assert(NGF_UV_INVERSE_LAYERS == 3 + kUvInvHiddenLayers && kUvInvHiddenLayers == 2, "linear1, linear2, two hidden layers, last_linear");

struct UvInvShape { int out_f[NGF_UV_INVERSE_LAYERS], in_f[NGF_UV_INVERSE_LAYERS]; };
inline UvInvShape uv_inverse_shape(int D)
{
    return {{kUvInvMid, kUvInvHidden, kUvInvHidden, kUvInvHidden, 3}, {D, kUvInvMid, kUvInvHidden, kUvInvHidden, kUvInvHidden}};
}

// offsets (floats) into the packed set: what the kernels' argument blocks carry
struct UvInvFwdAt { int32_t w1, b1, w2, b2, wh, bh, wo, bo; };      // wh / bh: the two hidden layers, strides 512 * 512 / 512
struct UvInvDxAt { int32_t to, th, t2, t1, zb; };                   // last_linear^T (3 -> 512), the hidden layers^T LAST FIRST (stride 512 * 512), linear2^T (512 -> 64), linear1^T (64 -> D, output layout), zeros

constexpr int kUvInvSegs = 16;
struct UvInvPlan {
    UvPackSeg seg[kUvInvSegs];
    int nfwd, nseg;                  // the forward set is seg[0 .. nfwd): all an inference handle packs
    int fwd_floats, floats;          // of the forward set; of everything (transposed set and zero block included)
    UvInvFwdAt fwd;
    UvInvDxAt dx;
};

// The forward set first, then the dX chain's layers -- element (o, i) of layer^T is W[i, o] -- then 512 zeros: the chain's bias in accumulator
// order (and its bias4).  Every image is a multiple of four floats, so every offset is 16-byte aligned.
inline UvInvPlan uv_inverse_plan(int D, const float *const *w, const float *const *b)
{
    const int M = kUvInvMid, H = kUvInvHidden;
    UvInvPlan P{};
    int off = 0;
    auto seg = [&](const float *src, int kind, int out_f, int in_f, int so, int si, int KT, int NT, int hid) {
        UvPackSeg &s = P.seg[P.nseg++];
        s.src = src; s.dst = off; s.kind = kind; s.out_f = out_f; s.in_f = in_f; s.so = so; s.si = si; s.NT = NT; s.hid = hid;
        s.count = kind == kUvPackDense ? KT * NT * 64 : (kind == kUvPackOut ? KT * 64 : (kind == kUvPackBias ? NT * 16 : 4));
        off += s.count;
        return s.dst;
    };
    UvInvFwdAt &A = P.fwd;
    A.w1 = seg(w[0], kUvPackDense, M, D, D, 1, 4, M / 16, 0);      A.b1 = seg(b[0], kUvPackBias, M, 0, 0, 0, 0, M / 16, 0);
    A.w2 = seg(w[1], kUvPackDense, H, M, M, 1, M / 4, H / 16, 1);  A.b2 = seg(b[1], kUvPackBias, H, 0, 0, 0, 0, H / 16, 0);
    A.wh = seg(w[2], kUvPackDense, H, H, H, 1, H / 4, H / 16, 1);
    (void)seg(w[3], kUvPackDense, H, H, H, 1, H / 4, H / 16, 1);
    A.bh = seg(b[2], kUvPackBias, H, 0, 0, 0, 0, H / 16, 0);
    (void)seg(b[3], kUvPackBias, H, 0, 0, 0, 0, H / 16, 0);
    A.wo = seg(w[4], kUvPackOut, 3, H, H, 1, H / 4, 0, 1);         A.bo = seg(b[4], kUvPackBias4, 3, 0, 0, 0, 0, 0, 0);
    P.nfwd = P.nseg;
    P.fwd_floats = off;
    UvInvDxAt &X = P.dx;
    X.to = seg(w[4], kUvPackDense, H, 3, 1, H, 4, H / 16, 0);              // d_xyz in natural order, as linear1 takes uv
    X.th = seg(w[3], kUvPackDense, H, H, 1, H, H / 4, H / 16, 1);
    (void)seg(w[2], kUvPackDense, H, H, 1, H, H / 4, H / 16, 1);
    X.t2 = seg(w[1], kUvPackDense, M, H, 1, M, H / 4, M / 16, 1);
    X.t1 = seg(w[0], kUvPackOut, D, M, 1, D, M / 4, 0, 1);
    X.zb = off;
    P.floats = off + (H / 16) * 16;
    return P;
}

}  // namespace ngf
