// ngf_alpha.hpp -- the non-template kernels of the alpha-mask update and of ray filtering (ngf_field.hip launches them; they were the tail of
// ngf_render.hpp).  ngf_render.hpp is included by two translation units of the library (ngf_field.hip, and ngf_train.hip through ngf_train.hpp), and
// a non-template __global__ function with external linkage may be defined in one only: they live here, `static` like the kernels of ngf_pack.hpp.
#pragma once
#include "ngf_render.hpp"

namespace ngf {

// updateAlphaMask (FieldBase.py:180-216) after getDenseAlpha: clamp(0,1), 3x3x3 max-pool (stride 1, padding 1), threshold to a
// {0,1} float volume [gz,gy,gx], and the index bounding box + count of the occupied voxels (integer atomics: deterministic)
static __global__ void __launch_bounds__(256) mask_pool_kernel(const float *__restrict__ alpha, int gx, int gy, int gz, float thres, float *__restrict__ vol,
                                                        int *bounds, unsigned long long *count)
{
    const int64_t n = (int64_t)gx * gy * gz;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    unsigned long long cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int x = (int)(i % gx), y = (int)((i / gx) % gy), z = (int)(i / ((int64_t)gx * gy));
        float m = -INFINITY;
        for (int dz = -1; dz <= 1; ++dz) {
            const int zz = z + dz;
            if (zz < 0 || zz >= gz) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= gy) continue;
                const float *row = alpha + ((int64_t)zz * gy + yy) * gx;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= gx) continue;
                    m = fmaxf(m, fminf(fmaxf(row[xx], 0.0f), 1.0f));
                }
            }
        }
        const bool occ = m >= thres;
        vol[i] = occ ? 1.0f : 0.0f;
        if (occ) {
            ++cnt;
            lo[0] = min(lo[0], x); lo[1] = min(lo[1], y); lo[2] = min(lo[2], z);
            hi[0] = max(hi[0], x); hi[1] = max(hi[1], y); hi[2] = max(hi[2], z);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (hi[k] >= 0) { atomicMin(bounds + k, lo[k]); atomicMax(bounds + 3 + k, hi[k]); }
    }
    if (cnt) atomicAdd(count, cnt);
}

static __global__ void mask_bounds_init_kernel(int *bounds)
{
    if (threadIdx.x < 3) bounds[threadIdx.x] = 0x7fffffff;
    else if (threadIdx.x < 6) bounds[threadIdx.x] = -1;
}

// valid_xyz.amin(0) / amax(0) (FieldBase.py:204-208): coordinates are monotone in their lattice index, so the box of the occupied
// voxels is the lattice point of the index bounds (taken per axis with min/max to stay correct for a flipped aabb)
static __global__ void mask_aabb_kernel(const RenderArgs A, const Lattice L, const int *bounds, float *new_aabb)
{
    const int k = threadIdx.x;
    if (k >= 3) return;
    const float *s = k == 0 ? L.sx : (k == 1 ? L.sy : L.sz);
    const float a = A.a0[k] * (1.0f - s[bounds[k]]) + A.a1[k] * s[bounds[k]];
    const float b = A.a0[k] * (1.0f - s[bounds[3 + k]]) + A.a1[k] * s[bounds[3 + k]];
    new_aabb[k] = fminf(a, b);
    new_aabb[3 + k] = fmaxf(a, b);
}

// ---- filtering_rays (FieldBase.py:218-246): the alpha-mask branch (S > 0) or the bbox_only slab test (S <= 0); one ray per thread --------------------------------------
static __global__ void __launch_bounds__(256) ray_filter_kernel(const RenderArgs A, const float *rays, int64_t n, int S, uint8_t *keep)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        float o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = rays[r * 6 + k]; d[k] = rays[r * 6 + 3 + k]; }
        float tmin = -INFINITY;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float vec = (d[k] == 0.0f) ? 1e-6f : d[k];
            float ra = (A.a1[k] - o[k]) / vec, rb = (A.a0[k] - o[k]) / vec;
            tmin = fmaxf(tmin, fminf(ra, rb));
        }
        if (S <= 0) {
            // bbox_only (FieldBase.py:226-233): keep the ray iff t_max > t_min of the slab test
            float tmax = INFINITY;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float vec = (d[k] == 0.0f) ? 1e-6f : d[k];
                float ra = (A.a1[k] - o[k]) / vec, rb = (A.a0[k] - o[k]) / vec;
                tmax = fminf(tmax, fmaxf(ra, rb));
            }
            keep[r] = tmax > tmin ? 1 : 0;
            continue;
        }
        tmin = fminf(fmaxf(tmin, A.near_), A.far_);
        bool hit = false;
        for (int i = 0; i < S && !hit; ++i) {
            const float z = tmin + A.step * (float)i;
            float p[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = o[k] + d[k] * z;
            hit = mask_occupied(A.mask, p);
        }
        keep[r] = hit ? 1 : 0;
    }
}

}  // namespace ngf
