// ngf_uv_query.hip -- C ABI (include/ngf.h), UV-Mapping (NeuTex) point queries: density, gauge uv and colour of an ngf_uv handle at world points,
// and the density on a lattice the kernel generates itself.  A translation unit of its own: ngf_uv.hip (the render kernel, whose assembly
// tests/test_isa_lint.py lints) and ngf_uv_export.hip keep their code.
#include <cmath>

#include "ngf_host.hpp"
#include "ngf_uv_query.hpp"

using namespace ngf;

namespace {

template <bool GEO, bool GAUGE, int TEX, bool LATTICE>
int launch(const UvQueryArgs &Q, int num_cus, hipStream_t st)
{
    // four waves per block, one per SIMD, 32 points per wave pass; one block per CU is all that fits (160 KB of activation rows)
    int64_t grid = ((Q.n + kUvTexPass - 1) / kUvTexPass + 3) / 4;
    if (grid > (int64_t)num_cus) grid = num_cus;
    const size_t lds = (size_t)4 * kUvTexTiles * kUvWaveLds * sizeof(float);
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(uv_query_kernel<GEO, GAUGE, TEX, LATTICE>), lds));
    hipLaunchKernelGGL((uv_query_kernel<GEO, GAUGE, TEX, LATTICE>), dim3((unsigned)grid), dim3(256), lds, st, Q);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

template <bool GEO>
int launch_tex(const UvQueryArgs &Q, int tex, int num_cus, hipStream_t st)
{
    if (tex == kUvQueryTexView) return launch<GEO, true, kUvQueryTexView, false>(Q, num_cus, st);
    if (tex == kUvQueryTexDiffuse) return launch<GEO, true, kUvQueryTexDiffuse, false>(Q, num_cus, st);
    return launch<GEO, true, kUvQueryNoTex, false>(Q, num_cus, st);
}

}  // namespace

extern "C" int ngf_uv_query(const ngf_uv *m, const float *xyz, int64_t n, const float *view, int32_t view_stride, int32_t flags, float *sigma,
                            float *uv, float *rgb, void *hip_stream)
{
    if (!m || !xyz) return fail(NGF_E_ARG, "ngf_uv_query: null %s", !m ? "model" : "points");
    if (flags & ~(NGF_UV_TEX_DIFFUSE | NGF_UV_QUERY_NO_CLIP)) return fail(NGF_E_ARG, "ngf_uv_query: unknown bits in flags (0x%x)", flags);
    if (!sigma && !uv && !rgb) return fail(NGF_E_ARG, "ngf_uv_query: no output requested (sigma, uv and rgb are all NULL)");
    const bool diffuse = (flags & NGF_UV_TEX_DIFFUSE) != 0;
    if (rgb && !diffuse && !view) return fail(NGF_E_ARG, "ngf_uv_query: rgb needs a view direction unless NGF_UV_TEX_DIFFUSE is set");
    if (rgb && !diffuse && view_stride != 0 && view_stride != 3)
        return fail(NGF_E_ARG, "ngf_uv_query: view_stride must be 0 (one shared direction) or 3 (one per point), got %d", view_stride);
    if (n < 0 || n >= (int64_t)1 << 40) return fail(NGF_E_ARG, "ngf_uv_query: n=%lld", (long long)n);
    if (n == 0) return NGF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    UvQueryArgs Q;
    memset(&Q, 0, sizeof(Q));
    int num_cus = 0;
    Q.M = uv_handle_args(m, &num_cus);
    const int tex = !rgb ? kUvQueryNoTex : (diffuse ? kUvQueryTexDiffuse : kUvQueryTexView);
    Q.xyz = xyz; Q.view = tex == kUvQueryTexView ? view : nullptr; Q.view_stride = tex == kUvQueryTexView ? view_stride : 0;
    Q.sigma = sigma; Q.rgb = rgb; Q.n = n;
    Q.clip = (flags & NGF_UV_QUERY_NO_CLIP) ? 0 : 1;
    Q.uv = uv;          // NULL with rgb alone: the gauge runs for the colour's sake and its coordinates are stored nowhere
    if (int rc = poison_lds(st)) return rc;
    if (!uv && !rgb) return launch<true, false, kUvQueryNoTex, false>(Q, num_cus, st);
    return sigma ? launch_tex<true>(Q, tex, num_cus, st) : launch_tex<false>(Q, tex, num_cus, st);
}

extern "C" int ngf_uv_density_lattice(const ngf_uv *m, const float lo[3], const float step[3], int32_t nx, int32_t ny, int32_t nz, int32_t flags,
                                      float *sigma, void *hip_stream)
{
    if (!m || !lo || !step || !sigma) return fail(NGF_E_ARG, "ngf_uv_density_lattice: null argument");
    if (flags & ~NGF_UV_QUERY_NO_CLIP) return fail(NGF_E_ARG, "ngf_uv_density_lattice: unknown bits in flags (0x%x)", flags);
    // (an axis index must be exact as a float: below 2^24)
    if (nx < 2 || ny < 2 || nz < 2 || nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24) || (int64_t)nx * ny * nz >= (int64_t)1 << 40)
        return fail(NGF_E_ARG, "ngf_uv_density_lattice: a lattice of %d x %d x %d (every axis needs 2 .. 2^24 points, 2^40 in all at the most)", nx, ny, nz);
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(lo[k]) || !std::isfinite(step[k]))
            return fail(NGF_E_ARG, "ngf_uv_density_lattice: lo / step must be finite (axis %d: lo %g, step %g)", k, (double)lo[k], (double)step[k]);
    hipStream_t st = (hipStream_t)hip_stream;
    UvQueryArgs Q;
    memset(&Q, 0, sizeof(Q));
    int num_cus = 0;
    Q.M = uv_handle_args(m, &num_cus);
    Q.sigma = sigma; Q.n = (int64_t)nx * ny * nz; Q.ny = ny; Q.nz = nz;
    Q.clip = (flags & NGF_UV_QUERY_NO_CLIP) ? 0 : 1;
    for (int k = 0; k < 3; ++k) { Q.lo[k] = lo[k]; Q.step[k] = step[k]; }
    if (int rc = poison_lds(st)) return rc;
    return launch<true, false, kUvQueryNoTex, true>(Q, num_cus, st);
}
