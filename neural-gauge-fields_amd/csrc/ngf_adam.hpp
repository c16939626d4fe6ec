// ngf_adam.hpp -- torch.optim.Adam (betas, eps, no weight decay, no amsgrad), float32 like the reference, element for element: what the
// TriPlane trainer (ngf_train.hpp, ngf_train.hip) and the fused InfoInv trainer (ngf_infoinv_fused.hpp, ngf_infoinv_train.hip) share.  The plane
// kernels stay with their trainers (packed split layout / fixed-point accumulator) and call adam_one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace ngf {

struct AdamArgs {
    float lr, beta1, beta2, eps;
    float bc1, bc2_sqrt;       // 1 - beta1^t, sqrt(1 - beta2^t)
    float l1;                  // planes: L1_reg_weight / numel, added as l1 * sign(p); 0 otherwise
};

// the bias corrections of step t in fp64, rounded to float once
inline AdamArgs adam_args(int32_t step, float lr, float beta1, float beta2, float eps, float l1)
{
    AdamArgs a;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.l1 = l1;
    a.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    a.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    return a;
}

__device__ __forceinline__ float adam_one(float p, float g, float &m, float &v, const AdamArgs &a)
{
    m = m + (1.0f - a.beta1) * (g - m);                   // exp_avg.lerp_(grad, 1 - beta1)
    v = v * a.beta2 + ((1.0f - a.beta2) * g) * g;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
    const float step = a.lr / a.bc1;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    return p - step * (m / denom);
}

// N dense tensors in one launch: segment k = elements [begin[k], begin[k+1]) of the concatenation, each with its own step count / lr (an empty
// segment's arguments are never read: step 1 is as good as any).  skip (may be NULL): device flag -- non-zero: the step's gradient is incomplete,
// nothing is updated (the TriPlane trainer's overflow[0], see train_prefix_kernel)
template <int N>
struct AdamDense {
    float *p[N], *m[N], *v[N];
    const float *g[N];
    int32_t begin[N + 1];                      // begin[k+1] == begin[k] for a skipped parameter
    AdamArgs a[N];
    const int32_t *skip;
};

template <int N>
__global__ void __launch_bounds__(256) adam_dense_all_kernel(const AdamDense<N> D)
{
    if (D.skip && *D.skip) return;
    const int total = D.begin[N];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int k = 0;
#pragma unroll
        for (int j = 1; j < N; ++j) k += (i >= D.begin[j]) ? 1 : 0;
        const int e = i - D.begin[k];
        float mi = D.m[k][e], vi = D.v[k][e];
        D.p[k][e] = adam_one(D.p[k][e], D.g[k][e], mi, vi, D.a[k]);
        D.m[k][e] = mi; D.v[k][e] = vi;
    }
}

// The host side of that launch, for every trainer: tensor j (parameter p[j], moments m[j] / v[j], gradient g[j], count[j] elements, its own
// step count and learning rate) takes part when on(j); the others become empty segments.  Returns the launch error (no launch when nothing is on).
template <int N, typename On>
inline hipError_t adam_dense_all(float *const *p, float *const *m, float *const *v, const float *const *g, const int64_t *count,
                                 const int32_t *step_count, const float *lr, float beta1, float beta2, float eps, On on, const int32_t *skip,
                                 hipStream_t st)
{
    AdamDense<N> D;
    int32_t at = 0;
    for (int j = 0; j < N; ++j) {
        D.p[j] = p[j]; D.m[j] = m[j]; D.v[j] = v[j]; D.g[j] = g[j];
        D.begin[j] = at;
        D.a[j] = adam_args(step_count[j] > 0 ? step_count[j] : 1, lr[j], beta1, beta2, eps, 0.0f);      // step 1 for an empty segment: never read
        if (on(j)) at += (int32_t)count[j];
    }
    D.begin[N] = at;
    D.skip = skip;
    if (at <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_dense_all_kernel<N>, dim3((at + 255) / 256), dim3(256), 0, st, D);
    return hipGetLastError();
}

}  // namespace ngf
