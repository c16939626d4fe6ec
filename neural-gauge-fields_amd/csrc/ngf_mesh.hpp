// ngf_mesh.hpp -- device code of the mesh export (ngf_mesh.hip): marching cubes over a dense float volume [gx,gy,gz] addressed by three
// element strides.  DESIGN.md section 4.9.
//
// A lattice point is INSIDE iff v >= level (NaN: outside).  Point p = (i * gy + j) * gz + k owns its +x, +y, +z edges; an owned edge carries
// a vertex iff its endpoints differ.  One thread per lattice point everywhere, 256 points per block:
//   count  : per point the owned-edge mask, the case and triangle count of the cell anchored at it (one uint16: case | mask << 8 | ntri << 11),
//            and per block the two sums (vertices, triangles); a volume whose x stride is the small one is classified by tiles first
//   scan   : exclusive scan of the block sums -- chunks of 1024 pairs scanned in place, their totals scanned the same way one level up, then
//            added back (separate launches; no kernel waits for another workgroup)
//   apply  : per point the index of its first vertex
//   emit   : vertices (+ normals) in point order with a point's edges in x, y, z order; faces in cell order then table order
// The case and the counts emit uses are the ones count stored: every index emit writes is below the totals count reported whatever the volume
// holds by then.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngf_mesh_table.hpp"

namespace ngf {

static constexpr int kMeshBlock = 256;            // lattice points per block (count / apply / emit)
static constexpr int kMeshScanItems = 4;          // pairs per thread of a scan block
static constexpr int kMeshScanChunk = kMeshBlock * kMeshScanItems;      // 1024 pairs per scan block

struct MeshVol {
    const float *v;
    int32_t gx, gy, gz;
    int64_t sx, sy, sz;      // element strides
    float level;
    int64_t n;               // gx * gy * gz (3 n < 2^31)
};

struct MeshEmit {
    float origin[3], spacing[3];
    int32_t flip;
    const uint16_t *cell;
    const uint32_t *first;   // per point: index of its first vertex
    const uint2 *sums;       // per block, scanned: (vertices, triangles) before the block
    float *vertices, *normals;
    int32_t *faces;
};

// exclusive scan of one pair per thread over a 256-thread block; *total = the block's sum.  Every thread of the block calls it.
__device__ inline uint2 mesh_block_scan(uint2 v, uint2 *total, uint2 *lds /* [4] */)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint2 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned x = __shfl_up(inc.x, d), y = __shfl_up(inc.y, d);
        if (lane >= d) { inc.x += x; inc.y += y; }
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    uint2 base = make_uint2(0, 0), tot = make_uint2(0, 0);
#pragma unroll
    for (int i = 0; i < kMeshBlock / 64; ++i) {
        const uint2 s = lds[i];
        if (i < w) { base.x += s.x; base.y += s.y; }
        tot.x += s.x; tot.y += s.y;
    }
    __syncthreads();
    *total = tot;
    return make_uint2(base.x + inc.x - v.x, base.y + inc.y - v.y);
}

struct MeshPoint { int32_t i, j, k; int64_t p; bool valid; };

__device__ inline MeshPoint mesh_point(const MeshVol &V)
{
    MeshPoint P;
    P.p = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    P.valid = P.p < V.n;
    const uint32_t p = (uint32_t)P.p, row = p / (uint32_t)V.gz;
    P.k = (int32_t)(p - row * (uint32_t)V.gz);
    P.i = (int32_t)(row / (uint32_t)V.gy);
    P.j = (int32_t)(row - (uint32_t)P.i * (uint32_t)V.gy);
    return P;
}

// the cell word of lattice point (i,j,k): case | owned-edge mask << 8 | triangle count << 11 (case 0 where no cell is anchored at the point)
__device__ inline unsigned mesh_classify(const MeshVol &V, int32_t i, int32_t j, int32_t k)
{
    const float *q = V.v + (i * V.sx + j * V.sy + k * V.sz);
    const bool hx = i + 1 < V.gx, hy = j + 1 < V.gy, hz = k + 1 < V.gz;
    const bool c0 = q[0] >= V.level;
    const bool c1 = hx && q[V.sx] >= V.level, c2 = hy && q[V.sy] >= V.level, c4 = hz && q[V.sz] >= V.level;
    const unsigned mask = (unsigned)(hx && c1 != c0) | (unsigned)(hy && c2 != c0) << 1 | (unsigned)(hz && c4 != c0) << 2;
    unsigned cas = 0;
    if (hx && hy && hz) {
        const bool c3 = q[V.sx + V.sy] >= V.level, c5 = q[V.sx + V.sz] >= V.level, c6 = q[V.sy + V.sz] >= V.level,
                   c7 = q[V.sx + V.sy + V.sz] >= V.level;
        cas = (unsigned)c0 | (unsigned)c1 << 1 | (unsigned)c2 << 2 | (unsigned)c3 << 3 | (unsigned)c4 << 4 | (unsigned)c5 << 5 | (unsigned)c6 << 6 |
              (unsigned)c7 << 7;
    }
    return cas | mask << 8 | (unsigned)kMeshTriCount[cas] << 11;
}

// FromVolume: classify the block's 256 points (k fastest: full lines of a volume whose z stride is the small one) and store their cell words;
// otherwise the words are there already (mesh_classify_tiles_kernel).  Either way: the block's two sums.
template <bool FromVolume>
__global__ __launch_bounds__(kMeshBlock) void mesh_count_kernel(MeshVol V, uint16_t *__restrict__ cell, uint2 *__restrict__ sums)
{
    __shared__ uint2 lds[kMeshBlock / 64];
    const MeshPoint P = mesh_point(V);
    unsigned c = 0;
    if (P.valid) {
        if (FromVolume) {
            c = mesh_classify(V, P.i, P.j, P.k);
            cell[P.p] = (uint16_t)c;
        } else {
            c = cell[P.p];
        }
    }
    uint2 total;
    (void)mesh_block_scan(make_uint2(__popc(c >> 8 & 7u), c >> 11), &total, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// The cell words of a volume whose x stride is the small one ([gz,gy,gx] memory, what updateAlphaMask leaves): a block takes a tile of
// 16 (i) x 16 (k) points of one j, lanes along i, so the volume is read in 64-byte runs and the words are written in 32-byte runs.
static constexpr int kMeshTile = 16;
__global__ __launch_bounds__(kMeshBlock) void mesh_classify_tiles_kernel(MeshVol V, uint16_t *__restrict__ cell)
{
    const uint32_t tiles_k = ((uint32_t)V.gz + kMeshTile - 1) / kMeshTile;
    const uint32_t b = blockIdx.x, rest = b / tiles_k;
    const int32_t k = (int32_t)((b - rest * tiles_k) * kMeshTile + (threadIdx.x >> 4));
    const int32_t ti = (int32_t)(rest / (uint32_t)V.gy), j = (int32_t)(rest - (uint32_t)ti * (uint32_t)V.gy);
    const int32_t i = ti * kMeshTile + (int32_t)(threadIdx.x & 15);
    if (i < V.gx && k < V.gz) cell[((int64_t)i * V.gy + j) * V.gz + k] = (uint16_t)mesh_classify(V, i, j, k);
}

// a[0..n): every chunk of 1024 pairs scanned in place (exclusive); the chunk's total to sums[block] (and, from the single block of the top level,
// to the two int64 pairs tot0 / tot1)
__global__ __launch_bounds__(kMeshBlock) void mesh_scan_chunks_kernel(uint2 *__restrict__ a, int64_t n, uint2 *__restrict__ sums, int64_t *tot0,
                                                                      int64_t *tot1)
{
    __shared__ uint2 lds[kMeshBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kMeshScanChunk + (int64_t)threadIdx.x * kMeshScanItems;
    uint2 v[kMeshScanItems], s = make_uint2(0, 0);
#pragma unroll
    for (int u = 0; u < kMeshScanItems; ++u) {
        v[u] = i0 + u < n ? a[i0 + u] : make_uint2(0, 0);
        s.x += v[u].x; s.y += v[u].y;
    }
    uint2 total, ex = mesh_block_scan(s, &total, lds);
#pragma unroll
    for (int u = 0; u < kMeshScanItems; ++u) {
        if (i0 + u < n) a[i0 + u] = ex;
        ex.x += v[u].x; ex.y += v[u].y;
    }
    if (threadIdx.x == 0) {
        if (sums) sums[blockIdx.x] = total;
        if (tot0) { tot0[0] = total.x; tot0[1] = total.y; }
        if (tot1) { tot1[0] = total.x; tot1[1] = total.y; }
    }
}

__global__ __launch_bounds__(kMeshBlock) void mesh_scan_add_kernel(uint2 *__restrict__ a, int64_t n, const uint2 *__restrict__ sums)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i < n) {
        const uint2 s = sums[i / kMeshScanChunk];
        uint2 x = a[i];
        x.x += s.x; x.y += s.y;
        a[i] = x;
    }
}

__global__ __launch_bounds__(kMeshBlock) void mesh_apply_kernel(const uint16_t *__restrict__ cell, int64_t n, const uint2 *__restrict__ sums,
                                                                uint32_t *__restrict__ first)
{
    __shared__ uint2 lds[kMeshBlock / 64];
    const int64_t p = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const unsigned c = p < n ? cell[p] : 0u;
    uint2 total;
    const uint2 ex = mesh_block_scan(make_uint2(__popc(c >> 8 & 7u), 0), &total, lds);
    if (p < n) first[p] = sums[blockIdx.x].x + ex.x;
}

// central difference along one axis at index x of d (one-sided at the border, 0 for a flat axis), per unit of world length
__device__ inline float mesh_diff(const float *q, int64_t s, int32_t x, int32_t d, float spacing)
{
    if (d == 1) return 0.f;
    if (x == 0) return (q[s] - q[0]) / spacing;
    if (x == d - 1) return (q[0] - q[-s]) / spacing;
    return (q[s] - q[-s]) / (2.f * spacing);
}

template <bool Normals>
__global__ __launch_bounds__(kMeshBlock) void mesh_emit_kernel(MeshVol V, MeshEmit E)
{
    __shared__ uint2 lds[kMeshBlock / 64];
    const MeshPoint P = mesh_point(V);
    const unsigned c = P.valid ? E.cell[P.p] : 0u;
    const unsigned cas = c & 255u, mask = c >> 8 & 7u, ntri = c >> 11;
    uint2 total;
    const uint2 ex = mesh_block_scan(make_uint2(0, ntri), &total, lds);
    if (mask) {
        const float *q = V.v + (P.i * V.sx + P.j * V.sy + P.k * V.sz);
        const float v0 = q[0];
        const float at[3] = {(float)P.i, (float)P.j, (float)P.k};
        const int64_t stride[3] = {V.sx, V.sy, V.sz};
        const int32_t idx[3] = {P.i, P.j, P.k}, dim[3] = {V.gx, V.gy, V.gz};
        float g0[3];
        if (Normals) {
#pragma unroll
            for (int b = 0; b < 3; ++b) g0[b] = mesh_diff(q, stride[b], idx[b], dim[b], E.spacing[b]);
        }
        int64_t o = 3 * (int64_t)E.first[P.p];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(mask >> a & 1u)) continue;
            const float v1 = q[stride[a]];
            float t = (V.level - v0) / (v1 - v0);
            if (!(t >= 0.f && t <= 1.f)) t = 0.5f;
#pragma unroll
            for (int b = 0; b < 3; ++b) E.vertices[o + b] = E.origin[b] + (at[b] + (b == a ? t : 0.f)) * E.spacing[b];
            if (Normals) {
                float g[3];
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const float g1 = mesh_diff(q + stride[a], stride[b], idx[b] + (b == a), dim[b], E.spacing[b]);
                    g[b] = g0[b] + t * (g1 - g0[b]);
                }
                const float len = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
                const bool ok = len > 0.f && len <= 3.402823466e38f;
#pragma unroll
                for (int b = 0; b < 3; ++b) E.normals[o + b] = ok ? -g[b] / len : 0.f;
            }
            o += 3;
        }
    }
    if (ntri) {
        int64_t o = 3 * ((int64_t)E.sums[blockIdx.x].y + ex.y);
        const int64_t plane = (int64_t)V.gy * V.gz;
        for (unsigned tt = 0; tt < ntri; ++tt, o += 3) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = kMeshTris[cas][3 * tt + m];
                const int a = e >> 2, r = e & 3;
                const int corner = a == 0 ? r << 1 : a == 1 ? (r & 1) | (r & 2) << 1 : r;       // the lattice point that owns edge e
                const int64_t owner = P.p + (corner & 1) * plane + (corner >> 1 & 1) * V.gz + (corner >> 2);
                const unsigned before = E.cell[owner] >> 8 & ((1u << a) - 1u);                  // the owner's vertices on lower axes
                E.faces[o + (E.flip ? 2 - m : m)] = (int32_t)(E.first[owner] + __popc(before));
            }
        }
    }
}

}  // namespace ngf
