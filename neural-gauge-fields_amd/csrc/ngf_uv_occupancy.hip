// ngf_uv_occupancy.hip -- C ABI (include/ngf.h), UV-Mapping (NeuTex) occupancy grid: the reduction of a density lattice to the packed mask and
// the look-up of explicit points.  ngf_uv_set_occupancy lives with the handle (ngf_uv.hip); the render's look-up is ngf_uv_occupancy.hpp's, the same
// function the point kernel below calls.  A translation unit of its own: ngf_uv.hip keeps the render kernels alone.
//
// Reduction, two plain kernels, no atomics, every output a function of the inputs alone:
//   uv_occ_hot_kernel     one thread per cell: hot = some corner c of the cell's 8 has !(c <= threshold) -- the same as !(max of the corners <=
//                         threshold) with a max that propagates NaN, so a NaN corner makes the cell hot -- one byte per cell in the workspace.
//   uv_occ_dilate_kernel  one thread per OUTPUT BYTE: each of its 8 cells (fewer in the last byte: the tail bits stay 0) is occupied iff a cell within
//                         Chebyshev distance `dilate` of it, inside the grid, is hot; the byte is written whole, once, and nothing past the image.
// The (2 dilate + 1)^3 byte reads per cell come from L2; the reduction is noise beside the lattice itself (0.67 M MAC per lattice point).
#include <cmath>

#include "ngf_host.hpp"
#include "ngf_uv_export.hpp"          // UvArgs (the handle's prototype: mask pointer, n, h) and uv_handle_args
#include "ngf_uv_occupancy.hpp"

using namespace ngf;

namespace {

__global__ void __launch_bounds__(256) uv_occ_hot_kernel(const float *sigma, int nx, int ny, int nz, float thr, uint8_t *hot)
{
    const int64_t cells = (int64_t)nx * ny * nz, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t sy = nz + 1, sx = (int64_t)(ny + 1) * (nz + 1);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += stride) {
        const int cz = (int)(i % nz), cy = (int)((i / nz) % ny), cx = (int)(i / ((int64_t)nz * ny));
        const float *c = sigma + cx * sx + cy * sy + cz;
        bool h = false;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int d = 0; d < 2; ++d) h = h || !(c[a * sx + b * sy + d] <= thr);
        hot[i] = h ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) uv_occ_dilate_kernel(const uint8_t *hot, int nx, int ny, int nz, int dilate, uint8_t *bits)
{
    const int64_t cells = (int64_t)nx * ny * nz, nbytes = (cells + 7) / 8, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbytes; b += stride) {
        unsigned byte = 0;
        for (int e = 0; e < 8; ++e) {
            const int64_t i = b * 8 + e;
            if (i >= cells) break;
            const int cz = (int)(i % nz), cy = (int)((i / nz) % ny), cx = (int)(i / ((int64_t)nz * ny));
            const int x0 = max(cx - dilate, 0), x1 = min(cx + dilate, nx - 1), y0 = max(cy - dilate, 0), y1 = min(cy + dilate, ny - 1);
            const int z0 = max(cz - dilate, 0), z1 = min(cz + dilate, nz - 1);
            unsigned any = 0;
            for (int x = x0; x <= x1; ++x)
                for (int y = y0; y <= y1; ++y)
                    for (int z = z0; z <= z1; ++z) any |= hot[((int64_t)x * ny + y) * nz + z];
            byte |= (any ? 1u : 0u) << (7 - e);
        }
        bits[b] = (uint8_t)byte;
    }
}

// xyz [n,3] -> out [n]: 1 where the point passes the render's strict in-cube test and its cell's bit is set; only such points load a byte
__global__ void __launch_bounds__(256) uv_occ_lookup_kernel(const uint8_t *bits, int n0, int n1, int n2, float h0, float h1, float h2, const float *xyz,
                                                            int64_t n, uint8_t *out)
{
    const int32_t nn[3] = {n0, n1, n2};
    const float hh[3] = {h0, h1, h2};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float p[3] = {xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]};
        bool v = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) v = v && (p[k] > -1.0f) && (p[k] < 1.0f);
        if (v) v = uv_occ_lookup(bits, nn, hh, p);
        out[i] = v ? 1 : 0;
    }
}

bool axes_ok(int32_t nx, int32_t ny, int32_t nz)
{
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= kUvOccMaxAxis && ny <= kUvOccMaxAxis && nz <= kUvOccMaxAxis;
}

unsigned grid_for(int64_t items)
{
    int64_t g = (items + 255) / 256;
    return (unsigned)std::min<int64_t>(std::max<int64_t>(g, 1), 8192);
}

}  // namespace

extern "C" int64_t ngf_uv_occupancy_workspace_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    if (!axes_ok(nx, ny, nz)) return -(int64_t)fail(NGF_E_ARG, "ngf_uv_occupancy_workspace_bytes: a grid of %d x %d x %d cells (every axis needs 1 .. %d)", nx, ny, nz, kUvOccMaxAxis);
    return (((int64_t)nx * ny * nz + 255) / 256) * 256;          // one byte per cell
}

extern "C" int ngf_uv_occupancy_from_lattice(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float threshold, int32_t dilate, uint8_t *bits,
                                             void *workspace, int64_t workspace_bytes, void *hip_stream)
{
    if (!sigma || !bits || !workspace)
        return fail(NGF_E_ARG, "ngf_uv_occupancy_from_lattice: null %s", !sigma ? "lattice" : (!bits ? "bits" : "workspace"));
    if (!axes_ok(nx, ny, nz))
        return fail(NGF_E_ARG, "ngf_uv_occupancy_from_lattice: a grid of %d x %d x %d cells (every axis needs 1 .. %d)", nx, ny, nz, kUvOccMaxAxis);
    if (dilate < 0 || dilate > kUvOccMaxDilate) return fail(NGF_E_ARG, "ngf_uv_occupancy_from_lattice: dilate must be 0 .. %d, got %d", kUvOccMaxDilate, dilate);
    if (std::isnan(threshold)) return fail(NGF_E_ARG, "ngf_uv_occupancy_from_lattice: the threshold is NaN");
    const int64_t need = ngf_uv_occupancy_workspace_bytes(nx, ny, nz);
    if (workspace_bytes < need)
        return fail(NGF_E_ARG, "ngf_uv_occupancy_from_lattice: the workspace holds %lld bytes, ngf_uv_occupancy_workspace_bytes asks for %lld", (long long)workspace_bytes,
                    (long long)need);
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t cells = (int64_t)nx * ny * nz;
    uint8_t *hot = (uint8_t *)workspace;
    NGF_LAUNCH(uv_occ_hot_kernel, dim3(grid_for(cells)), dim3(256), 0, st, sigma, nx, ny, nz, threshold, hot);
    NGF_LAUNCH(uv_occ_dilate_kernel, dim3(grid_for((cells + 7) / 8)), dim3(256), 0, st, (const uint8_t *)hot, nx, ny, nz, dilate, bits);
    return NGF_OK;
}

extern "C" int ngf_uv_occupancy_lookup(const ngf_uv *m, const float *xyz, int64_t n, uint8_t *out, void *hip_stream)
{
    if (!m || !xyz || !out) return fail(NGF_E_ARG, "ngf_uv_occupancy_lookup: null %s", !m ? "model" : (!xyz ? "points" : "output"));
    if (n < 0) return fail(NGF_E_ARG, "ngf_uv_occupancy_lookup: n=%lld", (long long)n);
    int num_cus = 0;
    const UvArgs &A = uv_handle_args(m, &num_cus);
    if (!A.occ) return fail(NGF_E_ARG, "ngf_uv_occupancy_lookup: the handle has no occupancy mask (ngf_uv_set_occupancy)");
    if (n == 0) return NGF_OK;
    NGF_LAUNCH(uv_occ_lookup_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)hip_stream, A.occ, A.occ_n[0], A.occ_n[1], A.occ_n[2], A.occ_h[0], A.occ_h[1],
               A.occ_h[2], xyz, n, out);
    return NGF_OK;
}
