// ngf_mesh.hip -- C ABI (include/ngf.h), mesh export: marching cubes over a dense float volume on the device.
// A translation unit of its own: no render or training kernel changes with it.
#include "ngf_host.hpp"
#include "ngf_mesh.hpp"

using namespace ngf;

namespace {

constexpr int64_t kHeaderBytes = 64;
constexpr int kMaxLevels = 4;      // block sums of < 2^31 / 3 points: 2.8M, 2731, 3 pairs

// what count leaves at the head of the workspace and emit compares with its own arguments
struct MeshHeader {
    int64_t nv, nt;
    int32_t dims[3];
    uint32_t level_bits;
};
static_assert(sizeof(MeshHeader) <= kHeaderBytes, "header");

// the header with zero counts (the scan's top level fills them in) and zero totals for the caller: what a volume without cells keeps
__global__ void mesh_header_kernel(MeshHeader *dst, MeshHeader h, int64_t *counts)
{
    *dst = h;
    counts[0] = 0;
    counts[1] = 0;
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// pairs of the scan levels above `n1`: every level's chunk totals, until one chunk holds a level
int64_t upper_pairs(int64_t n1, int64_t *sizes /* [kMaxLevels], sizes[0] = n1 */, int *levels)
{
    int64_t total = 0;
    int l = 0;
    sizes[0] = n1;
    while (sizes[l] > kMeshScanChunk) {
        sizes[l + 1] = cdiv(sizes[l], kMeshScanChunk);
        total += sizes[++l];
    }
    *levels = l + 1;
    return total;
}

struct Layout {
    int64_t n, n1, first, sums, upper, cell, bytes;
};

// header | first vertex per point (u32) | block sums (2 x u32) | upper scan levels | cell words (u16)
Layout layout(int64_t n)
{
    Layout L;
    int64_t sizes[kMaxLevels];
    int levels;
    L.n = n;
    L.n1 = cdiv(n, kMeshBlock);
    L.first = kHeaderBytes;
    L.sums = L.first + ((4 * n + 7) & ~(int64_t)7);
    L.upper = L.sums + 8 * L.n1;
    L.cell = L.upper + 8 * upper_pairs(L.n1, sizes, &levels);
    L.bytes = L.cell + ((2 * n + 7) & ~(int64_t)7);
    return L;
}

// exclusive scan of a[0..n) in place, both components; the totals as int64 pairs to tot0 / tot1 (DEVICE, either may be NULL).
// `upper`: upper_pairs(n) pairs of scratch.
int scan_pairs(uint2 *a, int64_t n, uint2 *upper, int64_t *tot0, int64_t *tot1, hipStream_t st)
{
    int64_t sizes[kMaxLevels];
    int levels;
    (void)upper_pairs(n, sizes, &levels);
    uint2 *at[kMaxLevels];
    at[0] = a;
    for (int l = 1; l < levels; ++l) at[l] = l == 1 ? upper : at[l - 1] + sizes[l - 1];
    for (int l = 0; l < levels; ++l) {
        const bool top = l == levels - 1;
        hipLaunchKernelGGL(mesh_scan_chunks_kernel, dim3((unsigned)cdiv(sizes[l], kMeshScanChunk)), dim3(kMeshBlock), 0, st, at[l], sizes[l],
                           top ? (uint2 *)nullptr : at[l + 1], top ? tot0 : (int64_t *)nullptr, top ? tot1 : (int64_t *)nullptr);
    }
    for (int l = levels - 2; l >= 0; --l)
        hipLaunchKernelGGL(mesh_scan_add_kernel, dim3((unsigned)cdiv(sizes[l], kMeshBlock)), dim3(kMeshBlock), 0, st, at[l], sizes[l], at[l + 1]);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

// the checks count and emit share; *n = lattice points, 0 when a dimension is 1 (no cells: an empty mesh, not an error)
int check_volume(const char *fn, const float *vol, const int32_t *dims, const int64_t *strides, float level, const void *workspace,
                 int64_t workspace_bytes, int64_t *n)
{
    if (!vol || !dims || !strides || !workspace) return fail(NGF_E_ARG, "%s: null argument", fn);
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1) return fail(NGF_E_ARG, "%s: dims[%d] = %d (must be >= 1)", fn, a, dims[a]);
        if (strides[a] == 0) return fail(NGF_E_ARG, "%s: strides[%d] is zero", fn, a);
    }
    if (!std::isfinite(level)) return fail(NGF_E_ARG, "%s: level is not finite", fn);
    const int64_t bytes = ngf_mesh_workspace_bytes(dims[0], dims[1], dims[2]);
    if (bytes < 0) return fail(NGF_E_UNSUPPORTED, "%s: %d x %d x %d lattice points: 3 * points must stay below 2^31", fn, dims[0], dims[1], dims[2]);
    if (workspace_bytes < bytes)
        return fail(NGF_E_ARG, "%s: workspace of %lld bytes, ngf_mesh_workspace_bytes asks for %lld", fn, (long long)workspace_bytes, (long long)bytes);
    *n = dims[0] == 1 || dims[1] == 1 || dims[2] == 1 ? 0 : (int64_t)dims[0] * dims[1] * dims[2];
    return NGF_OK;
}

MeshVol volume_args(const float *vol, const int32_t *dims, const int64_t *strides, float level, int64_t n)
{
    MeshVol V;
    V.v = vol;
    V.gx = dims[0]; V.gy = dims[1]; V.gz = dims[2];
    V.sx = strides[0]; V.sy = strides[1]; V.sz = strides[2];
    V.level = level;
    V.n = n;
    return V;
}

}  // namespace

extern "C" int64_t ngf_mesh_workspace_bytes(int32_t gx, int32_t gy, int32_t gz)
{
    if (gx < 1 || gy < 1 || gz < 1) return -1;
    const int64_t limit = ((int64_t)1 << 31) / 3;      // 3 n < 2^31  <=>  n <= limit
    if ((int64_t)gx * gy > limit || (int64_t)gx * gy * gz > limit) return -1;
    return layout((int64_t)gx * gy * gz).bytes;
}

extern "C" int ngf_mesh_count(const float *vol, const int32_t *dims, const int64_t *strides, float level, void *workspace, int64_t workspace_bytes,
                              int64_t *counts_dev, void *hip_stream)
{
    int64_t n = 0;
    if (!counts_dev) return fail(NGF_E_ARG, "ngf_mesh_count: null argument");
    if (int rc = check_volume("ngf_mesh_count", vol, dims, strides, level, workspace, workspace_bytes, &n)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    char *ws = (char *)workspace;
    MeshHeader h;
    memset(&h, 0, sizeof(h));
    for (int a = 0; a < 3; ++a) h.dims[a] = dims[a];
    memcpy(&h.level_bits, &level, 4);
    if (int rc = poison_lds(st)) return rc;
    hipLaunchKernelGGL(mesh_header_kernel, dim3(1), dim3(1), 0, st, (MeshHeader *)ws, h, counts_dev);
    HIP_TRY(hipGetLastError());
    if (n == 0) return NGF_OK;
    const Layout L = layout(n);
    uint2 *sums = (uint2 *)(ws + L.sums);
    uint16_t *cell = (uint16_t *)(ws + L.cell);
    const MeshVol V = volume_args(vol, dims, strides, level, n);
    if (std::llabs(strides[0]) < std::llabs(strides[2])) {
        const int64_t tiles = cdiv(dims[0], kMeshTile) * dims[1] * cdiv(dims[2], kMeshTile);      // <= n: fits a grid
        hipLaunchKernelGGL(mesh_classify_tiles_kernel, dim3((unsigned)tiles), dim3(kMeshBlock), 0, st, V, cell);
        hipLaunchKernelGGL((mesh_count_kernel<false>), dim3((unsigned)L.n1), dim3(kMeshBlock), 0, st, V, cell, sums);
    } else {
        hipLaunchKernelGGL((mesh_count_kernel<true>), dim3((unsigned)L.n1), dim3(kMeshBlock), 0, st, V, cell, sums);
    }
    if (int rc = scan_pairs(sums, L.n1, (uint2 *)(ws + L.upper), (int64_t *)ws, counts_dev, st)) return rc;
    hipLaunchKernelGGL(mesh_apply_kernel, dim3((unsigned)L.n1), dim3(kMeshBlock), 0, st, (const uint16_t *)cell, n, (const uint2 *)sums,
                       (uint32_t *)(ws + L.first));
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

extern "C" int ngf_mesh_emit(const float *vol, const int32_t *dims, const int64_t *strides, float level, const float *origin, const float *spacing,
                             int32_t flags, const void *workspace, int64_t workspace_bytes, int64_t nv, int64_t nt, float *vertices, float *normals,
                             int32_t *faces, void *hip_stream)
{
    int64_t n = 0;
    if (!origin || !spacing) return fail(NGF_E_ARG, "ngf_mesh_emit: null argument");
    if (int rc = check_volume("ngf_mesh_emit", vol, dims, strides, level, workspace, workspace_bytes, &n)) return rc;
    if (flags & ~(NGF_MESH_FLIP | NGF_MESH_NORMALS)) return fail(NGF_E_ARG, "ngf_mesh_emit: unknown bits in flags (0x%x)", flags);
    const bool want_normals = (flags & NGF_MESH_NORMALS) != 0;
    if (nv < 0 || nt < 0 || nv > 3 * n || nt > kMeshMaxTris * n)
        return fail(NGF_E_ARG, "ngf_mesh_emit: nv = %lld, nt = %lld cannot be the counts of this volume", (long long)nv, (long long)nt);
    if ((nv && !vertices) || (nt && !faces) || (nv && want_normals && !normals)) return fail(NGF_E_ARG, "ngf_mesh_emit: null output");
    if (n == 0) return NGF_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    MeshHeader h;
    HIP_TRY(hipMemcpyAsync(&h, workspace, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t level_bits;
    memcpy(&level_bits, &level, 4);
    if (h.dims[0] != dims[0] || h.dims[1] != dims[1] || h.dims[2] != dims[2] || h.level_bits != level_bits)
        return fail(NGF_E_ARG, "ngf_mesh_emit: the workspace holds the count of another volume or level");
    if (h.nv != nv || h.nt != nt)
        return fail(NGF_E_ARG, "ngf_mesh_emit: nv = %lld, nt = %lld, but ngf_mesh_count left %lld, %lld", (long long)nv, (long long)nt, (long long)h.nv,
                    (long long)h.nt);
    if (nv == 0 && nt == 0) return NGF_OK;
    if (int rc = poison_lds(st)) return rc;
    const Layout L = layout(n);
    const char *ws = (const char *)workspace;
    MeshEmit E;
    for (int a = 0; a < 3; ++a) { E.origin[a] = origin[a]; E.spacing[a] = spacing[a]; }
    E.flip = (flags & NGF_MESH_FLIP) != 0;
    E.cell = (const uint16_t *)(ws + L.cell);
    E.first = (const uint32_t *)(ws + L.first);
    E.sums = (const uint2 *)(ws + L.sums);
    E.vertices = vertices; E.normals = want_normals ? normals : nullptr; E.faces = faces;
    const MeshVol V = volume_args(vol, dims, strides, level, n);
    if (want_normals)
        hipLaunchKernelGGL((mesh_emit_kernel<true>), dim3((unsigned)L.n1), dim3(kMeshBlock), 0, st, V, E);
    else
        hipLaunchKernelGGL((mesh_emit_kernel<false>), dim3((unsigned)L.n1), dim3(kMeshBlock), 0, st, V, E);
    HIP_TRY(hipGetLastError());
    return NGF_OK;
}

extern "C" int ngf_debug_mesh_scan(uint32_t *pairs, int64_t n, uint32_t *scratch, int64_t scratch_pairs, int64_t *totals_dev, void *hip_stream)
{
    if (!pairs || !scratch || !totals_dev) return fail(NGF_E_ARG, "ngf_debug_mesh_scan: null argument");
    if (n < 1 || n > ((int64_t)1 << 31) / 3) return fail(NGF_E_ARG, "ngf_debug_mesh_scan: n = %lld", (long long)n);
    int64_t sizes[kMaxLevels];
    int levels;
    const int64_t want = upper_pairs(n, sizes, &levels);
    if (scratch_pairs < want)
        return fail(NGF_E_ARG, "ngf_debug_mesh_scan: scratch of %lld pairs, %lld needed", (long long)scratch_pairs, (long long)want);
    return scan_pairs((uint2 *)pairs, n, (uint2 *)scratch, totals_dev, nullptr, (hipStream_t)hip_stream);
}
