// ngf_uv_inverse.hip -- C ABI (include/ngf.h), UV-Mapping (NeuTex) inverse gauge: template points uv -> world points xyz through the
// InverseNetwork (gauge_fields.py:78-120).  A handle of its own (the network is not among ngf_uv_desc's 29 render layers) and a translation
// unit of its own: ngf_uv.hip, ngf_uv_export.hip and ngf_uv_query.hip keep their code.
#include "ngf_host.hpp"
#include "ngf_mlp_image.hpp"      // hidden(): the accumulator order of a lane, shared with the field images
#include "ngf_uv_inverse.hpp"

using namespace ngf;

struct ngf_uv_inverse {
    float *w = nullptr;
    UvInverseArgs proto;
    int num_cus = 256;
    int dev = 0;                   // the device the handle's weights live on (the caller's current device at create)
};

extern "C" int ngf_uv_inverse_destroy(ngf_uv_inverse *h)
{
    if (!h) return NGF_OK;
    DeviceScope ds(h->dev);
    if (h->w) (void)hipFree(h->w);
    delete h;
    return NGF_OK;
}

namespace {
// The streamed layouts of ngf_uv.hpp's blocks, as ngf_uv.hip packs them for the render layers.  ngf_mlp_image.hpp supplies the accumulator order
// (hidden); its ksteps_f32 / mlp_tail write the LDS images of the field kernels ([unit tile][k-step][lane], one dword per matrix instruction) and
// ngf_mlp_layout.hpp places those, neither of which is what kload_wg / out_prefetch / load_bias read: [k-step][tile group][lane][4] from L2.
struct InvPacker {
    std::vector<float> buf;
    int align() { while (buf.size() & 3) buf.push_back(0.0f); return (int)buf.size(); }
    // imap(t, kq) -> input index behind k-step t of lane quarter kq; KT k-steps; NT unit tiles (multiple of 4): [KT][NT / 4][64 lanes][4]
    template <typename F>
    int dense(const std::vector<float> &W, int out_f, int in_f, int KT, int NT, F imap)
    {
        const int off = align();
        buf.resize(off + (size_t)KT * NT * 64, 0.0f);
        for (int t = 0; t < KT; ++t)
            for (int g = 0; g < NT / 4; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 4; ++e) {
                        const int o = (4 * g + e) * 16 + (l & 15), i = imap(t, l >> 4);
                        buf[off + (((size_t)t * (NT / 4) + g) * 64 + l) * 4 + e] = (o < out_f && i < in_f) ? W[(size_t)o * in_f + i] : 0.0f;
                    }
        return off;
    }
    // output layer with 3 units: [KT / 4][64 lanes][4] -- a lane's A operands of four k-steps in one 16-byte load (dense_out)
    template <typename F>
    int out_layer(const std::vector<float> &W, int out_f, int in_f, int KT, F imap)
    {
        const int off = align();
        buf.resize(off + (size_t)KT * 64, 0.0f);
        for (int t = 0; t < KT; ++t)
            for (int l = 0; l < 64; ++l) {
                const int o = l & 15, i = imap(t, l >> 4);
                buf[off + ((size_t)(t >> 2) * 64 + l) * 4 + (t & 3)] = (o < out_f && i < in_f) ? W[(size_t)o * in_f + i] : 0.0f;
            }
        return off;
    }
    // [4 lane quarters][NT tiles][4]: accumulator order (load_bias)
    int bias(const std::vector<float> &b, int NT)
    {
        const int off = align();
        buf.resize(off + (size_t)NT * 16, 0.0f);
        for (int kq = 0; kq < 4; ++kq)
            for (int mt = 0; mt < NT; ++mt)
                for (int r = 0; r < 4; ++r) buf[off + kq * (NT * 4) + mt * 4 + r] = b[hidden(mt, r, kq)];
        return off;
    }
    int bias4(const std::vector<float> &b, int out_f)
    {
        const int off = align();
        for (int e = 0; e < 4; ++e) buf.push_back(e < out_f ? b[e] : 0.0f);
        return off;
    }
};
}  // namespace

extern "C" int ngf_uv_inverse_create(const ngf_uv_inverse_desc *d, ngf_uv_inverse **out, void *hip_stream)
{
    if (!d || !out) return fail(NGF_E_ARG, "ngf_uv_inverse_create: null argument");
    *out = nullptr;
    if (d->input_dim != 2 && d->input_dim != 3)
        return fail(NGF_E_ARG, "ngf_uv_inverse_create: input_dim must be 2 (square) or 3 (sphere), got %d", d->input_dim);
    for (int l = 0; l < NGF_UV_INVERSE_LAYERS; ++l)
        if (!d->w[l] || !d->b[l]) return fail(NGF_E_ARG, "ngf_uv_inverse_create: layer %d missing", l);
    hipStream_t st = (hipStream_t)hip_stream;
    const int D = d->input_dim, M = kUvInvMid, H = kUvInvHidden;
    static_assert(NGF_UV_INVERSE_LAYERS == 3 + kUvInvHiddenLayers, "linear1, linear2, the hidden layers, last_linear");
    const int kOut[NGF_UV_INVERSE_LAYERS] = {M, H, H, H, 3}, kIn[NGF_UV_INVERSE_LAYERS] = {D, M, H, H, H};
    std::vector<std::vector<float>> W(NGF_UV_INVERSE_LAYERS), B(NGF_UV_INVERSE_LAYERS);
    for (int l = 0; l < NGF_UV_INVERSE_LAYERS; ++l) {
        int rc;
        if ((rc = d2h(W[l], d->w[l], (size_t)kOut[l] * kIn[l], st)) || (rc = d2h(B[l], d->b[l], kOut[l], st))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    ngf_uv_inverse *h = new (std::nothrow) ngf_uv_inverse();
    if (!h) return fail(NGF_E_HIP, "out of host memory");
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) h->num_cus = prop.multiProcessorCount;
    h->dev = dev;
    UvInverseArgs &A = h->proto;
    memset(&A, 0, sizeof(A));
    A.dim = D;
    InvPacker P;
    auto nat = [](int t, int kq) { return 4 * t + kq; };                      // the template point's coordinates: natural order
    auto hid = [](int t, int kq) { return hidden(t >> 2, t & 3, kq); };       // previous layer's accumulator order
    A.w1 = P.dense(W[0], M, D, 4, M / 16, nat);      A.b1 = P.bias(B[0], M / 16);
    A.w2 = P.dense(W[1], H, M, M / 4, H / 16, hid);  A.b2 = P.bias(B[1], H / 16);
    for (int l = 0; l < kUvInvHiddenLayers; ++l) {
        const int o = P.dense(W[2 + l], H, H, H / 4, H / 16, hid);
        if (l == 0) A.wh = o;
    }
    for (int l = 0; l < kUvInvHiddenLayers; ++l) {
        const int o = P.bias(B[2 + l], H / 16);
        if (l == 0) A.bh = o;
    }
    A.wo = P.out_layer(W[4], 3, H, H / 4, hid);      A.bo = P.bias4(B[4], 3);
    P.align();
    auto bail = [&](int code) { ngf_uv_inverse_destroy(h); return code; };
    if (hipMalloc((void **)&h->w, P.buf.size() * sizeof(float)) != hipSuccess) return bail(fail(NGF_E_HIP, "ngf_uv_inverse_create: hipMalloc(weights) failed"));
    if (hipMemcpyAsync(h->w, P.buf.data(), P.buf.size() * sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return bail(fail(NGF_E_HIP, "ngf_uv_inverse_create: uploading the packed weights failed"));
    A.w = h->w;
    *out = h;
    return NGF_OK;
}

extern "C" int ngf_uv_inverse_map(const ngf_uv_inverse *h, const float *uv, int64_t n, float *xyz, void *hip_stream)
{
    if (!h || !uv || !xyz) return fail(NGF_E_ARG, "ngf_uv_inverse_map: null %s", !h ? "handle" : (!uv ? "uv" : "xyz"));
    if (n < 0 || n >= (int64_t)1 << 40) return fail(NGF_E_ARG, "ngf_uv_inverse_map: n=%lld", (long long)n);
    if (n == 0) return NGF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    UvInverseArgs Q = h->proto;
    Q.uv = uv; Q.xyz = xyz; Q.n = n;
    if (int rc = poison_lds(st)) return rc;
    // four waves per block, one per SIMD, 16 points per wave pass; one block per CU (128 KB of activation rows)
    int64_t grid = ((n + kUvInvTilePoints - 1) / kUvInvTilePoints + kUvInvWaves - 1) / kUvInvWaves;
    if (grid > (int64_t)h->num_cus) grid = h->num_cus;
    const size_t lds = (size_t)kUvInvWaves * kUvInvWaveLds * sizeof(float);
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(uv_inverse_kernel), lds));
    NGF_LAUNCH(uv_inverse_kernel, dim3((unsigned)grid), dim3(64 * kUvInvWaves), lds, st, Q);
    return NGF_OK;
}
