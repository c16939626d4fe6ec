// ngf_uv_inverse.hip -- C ABI (include/ngf.h), UV-Mapping (NeuTex) inverse gauge: template points uv -> world points xyz through the
// InverseNetwork (gauge_fields.py:78-120).  A handle of its own (the network is not among ngf_uv_desc's 29 render layers) and a translation
// unit of its own: ngf_uv.hip, ngf_uv_export.hip and ngf_uv_query.hip keep their code.
#include "ngf_host.hpp"
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

// the one definition of the inference kernel, in the one unit that launches it; the pass itself is ngf_uv_inverse.hpp's
namespace ngf {
__global__ void __launch_bounds__(64 * kUvInvWaves) uv_inverse_kernel(const UvInverseArgs Q) { uv_inverse_pass<false>(Q, nullptr); }
}  // namespace ngf

extern "C" int ngf_uv_inverse_create(const ngf_uv_inverse_desc *d, ngf_uv_inverse **out, void *hip_stream)
{
    if (!d || !out) return fail(NGF_E_ARG, "ngf_uv_inverse_create: null argument");
    *out = nullptr;
    if (int rc = check_inverse_desc("ngf_uv_inverse_create", d)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const UvInvShape shape = uv_inverse_shape(d->input_dim);
    std::vector<float> W[NGF_UV_INVERSE_LAYERS], B[NGF_UV_INVERSE_LAYERS];
    const float *w[NGF_UV_INVERSE_LAYERS], *b[NGF_UV_INVERSE_LAYERS];
    for (int l = 0; l < NGF_UV_INVERSE_LAYERS; ++l) {
        int rc;
        if ((rc = d2h(W[l], d->w[l], (size_t)shape.out_f[l] * shape.in_f[l], st)) || (rc = d2h(B[l], d->b[l], shape.out_f[l], st))) return rc;
        w[l] = W[l].data(); b[l] = B[l].data();
    }
    HIP_TRY(hipStreamSynchronize(st));
    ngf_uv_inverse *h = new (std::nothrow) ngf_uv_inverse();
    if (!h) return fail(NGF_E_HIP, "out of host memory");
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) h->num_cus = prop.multiProcessorCount;
    h->dev = dev;
    // the forward set of the plan, packed on the host from the copies (the trainer packs the same segments on the device, every step)
    const UvInvPlan P = uv_inverse_plan(d->input_dim, w, b);
    std::vector<float> buf(P.fwd_floats);
    for (int s = 0; s < P.nfwd; ++s)
        for (int idx = 0; idx < P.seg[s].count; ++idx) buf[P.seg[s].dst + idx] = uv_pack_value(P.seg[s], idx);
    UvInverseArgs &A = h->proto;
    memset(&A, 0, sizeof(A));
    A.dim = d->input_dim;
    A.at = P.fwd;
    auto bail = [&](int code) { ngf_uv_inverse_destroy(h); return code; };
    if (hipMalloc((void **)&h->w, buf.size() * sizeof(float)) != hipSuccess) return bail(fail(NGF_E_HIP, "ngf_uv_inverse_create: hipMalloc(weights) failed"));
    if (hipMemcpyAsync(h->w, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
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
    return launch_inverse_tiles(uv_inverse_kernel, Q, n, h->num_cus, st);
}
