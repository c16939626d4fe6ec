// ngf_uv_export.hip -- C ABI (include/ngf.h), UV-Mapping (NeuTex) texture export: the texture MLP of an ngf_uv handle on a list of points.
// A translation unit of its own: ngf_uv.hip (the render kernel, whose assembly tests/test_isa_lint.py lints) keeps its code.
#include "ngf_host.hpp"
#include "ngf_uv_export.hpp"

using namespace ngf;

extern "C" int ngf_uv_texture_eval(const ngf_uv *m, const float *uv, const float *view, int32_t view_stride, int64_t n, int32_t flags, float *out,
                                   void *hip_stream)
{
    if (!m || !uv || !out) return fail(NGF_E_ARG, "ngf_uv_texture_eval: null argument");
    if (flags & ~NGF_UV_TEX_DIFFUSE) return fail(NGF_E_ARG, "ngf_uv_texture_eval: unknown bits in flags (0x%x)", flags);
    const bool diffuse = (flags & NGF_UV_TEX_DIFFUSE) != 0;
    if (!diffuse && !view) return fail(NGF_E_ARG, "ngf_uv_texture_eval: a view direction is required unless NGF_UV_TEX_DIFFUSE is set");
    if (!diffuse && view_stride != 0 && view_stride != 3)
        return fail(NGF_E_ARG, "ngf_uv_texture_eval: view_stride must be 0 (one shared direction) or 3 (one per point), got %d", view_stride);
    if (n < 0 || n >= (int64_t)1 << 40) return fail(NGF_E_ARG, "ngf_uv_texture_eval: n=%lld", (long long)n);
    if (n == 0) return NGF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    UvTexArgs T;
    memset(&T, 0, sizeof(T));
    int num_cus = 0;
    T.M = uv_handle_args(m, &num_cus);
    T.uv = uv; T.view = diffuse ? nullptr : view; T.out = out; T.n = n; T.view_stride = diffuse ? 0 : view_stride;
    if (int rc = poison_lds(st)) return rc;
    // four waves per block, one per SIMD, 32 points per wave pass; one block per CU is all that fits (160 KB of activation rows)
    int64_t grid = ((n + kUvTexPass - 1) / kUvTexPass + 3) / 4;
    if (grid > (int64_t)num_cus) grid = num_cus;
    const size_t lds = (size_t)4 * kUvTexTiles * kUvWaveLds * sizeof(float);
    if (diffuse) {
        HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(uv_texture_eval_kernel<true>), lds));
        hipLaunchKernelGGL((uv_texture_eval_kernel<true>), dim3((unsigned)grid), dim3(256), lds, st, T);
    } else {
        HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(uv_texture_eval_kernel<false>), lds));
        hipLaunchKernelGGL((uv_texture_eval_kernel<false>), dim3((unsigned)grid), dim3(256), lds, st, T);
    }
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}
