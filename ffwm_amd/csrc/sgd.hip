// sgd.hip -- one SGD-momentum step over a FLAT parameter range whose elements belong to segments with their own learning rate and
// weight decay.
//
// Reference: lightcnn/finetune.py:74-90 -- torch.optim.SGD(momentum 0.9, dampening 0, no Nesterov) with ONE parameter group per
// tensor: 62 groups in four (lr multiple, weight decay) settings over 32.9 M parameters, which torch's multi-tensor SGD walks group
// by group.  Here the parameters, their gradients (the reducer's flat array, ffwm_amd/dp.py) and the momentum buffer are three
// contiguous arrays and a step is one streaming pass: 3 reads + 2 writes of 4 bytes per parameter, HBM-bound (adam.hip's sibling).
//
// Arithmetic (five roundings per element; the library is built without FMA contraction, the last line is an explicit fma):
//     g'  = g + wd * p
//     buf = momentum * buf + g'             a zero-initialised buffer gives torch's first step: 0.9 * 0 + g' == g'
//     p   = fma(-lr, buf, p)                lr = 0.0 leaves p as it is, bit for bit
// lr and wd are those of the element's segment's group, read from DEVICE memory: a rate the host changes reaches the replays of a
// captured step.  The segment table is staged once per block in LDS (end, lr, wd per segment); a vector's segment is found by binary
// search, a vector that straddles a boundary and the tail go element by element.
#include "common.hpp"

namespace ffwm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSgdMaxSegments = 1024;
constexpr int kSgdMaxGroups = 16;

__device__ __forceinline__ void sgd_one(float& p, float g, float& buf, float lr, float wd, float momentum) {
    const float gd = g + wd * p;
    buf = momentum * buf + gd;
    p = fmaf(-lr, buf, p);
}

// the first segment whose end lies behind element i (the last one for a table that does not cover i)
__device__ __forceinline__ int sgd_segment(const long long* ends, int n_seg, long long i) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kBlock)
sgd_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n,
                const long long* __restrict__ seg_end, const int* __restrict__ seg_group, int n_seg,
                const double* __restrict__ group_lr, const double* __restrict__ group_wd, int n_groups, float momentum) {
    __shared__ long long ends[kSgdMaxSegments];
    __shared__ float lrs[kSgdMaxSegments], wds[kSgdMaxSegments];
    for (int i = threadIdx.x; i < n_seg; i += kBlock) {
        int k = seg_group[i];
        k = k < 0 ? 0 : (k < n_groups ? k : n_groups - 1);          // device data: a group outside the table is never dereferenced
        ends[i] = seg_end[i];
        lrs[i] = static_cast<float>(group_lr[k]);
        wds[i] = static_cast<float>(group_wd[k]);
    }
    __syncthreads();
    const int64_t n4 = n >> 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n4; i += stride) {
        const f32x4 p4 = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 g4 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
        const f32x4 b4 = reinterpret_cast<f32x4*>(buf)[i];
        float pa[4] = {p4.x, p4.y, p4.z, p4.w}, ga[4] = {g4.x, g4.y, g4.z, g4.w}, ba[4] = {b4.x, b4.y, b4.z, b4.w};
        const long long e0 = 4 * i;
        int s = sgd_segment(ends, n_seg, e0);
        if (ends[s] >= e0 + 4 || s == n_seg - 1) {
            const float lr = lrs[s], wd = wds[s];
#pragma unroll
            for (int q = 0; q < 4; ++q) sgd_one(pa[q], ga[q], ba[q], lr, wd, momentum);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                while (s < n_seg - 1 && ends[s] <= e0 + q) ++s;
                sgd_one(pa[q], ga[q], ba[q], lrs[s], wds[s], momentum);
            }
        }
        const f32x4 pp = {pa[0], pa[1], pa[2], pa[3]}, bb = {ba[0], ba[1], ba[2], ba[3]};
        reinterpret_cast<f32x4*>(p)[i] = pp;
        reinterpret_cast<f32x4*>(buf)[i] = bb;
    }
    // tail (n not a multiple of 4)
    const int64_t t = (n4 << 2) + static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (t < n) {
        const int s = sgd_segment(ends, n_seg, t);
        sgd_one(p[t], g[t], buf[t], lrs[s], wds[s], momentum);
    }
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_sgd_step(void* params, const void* grads, void* momentum_buf, int64_t n, const int64_t* seg_end,
                             const int32_t* seg_group, int n_seg, const double* group_lr, const double* group_wd, int n_groups,
                             double momentum, int dtype, void* stream) {
    const char* fn = "ffwm_sgd_step";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(params && grads && momentum_buf, FFWM_ERR_ARG, "%s: NULL pointer (params, grads or momentum_buf)", fn);
    FFWM_REQUIRE(seg_end && seg_group && group_lr && group_wd, FFWM_ERR_ARG, "%s: NULL segment or group table", fn);
    FFWM_REQUIRE(n > 0, FFWM_ERR_ARG, "%s: need n > 0 (n=%lld)", fn, (long long)n);
    FFWM_REQUIRE(n_seg >= 1 && n_seg <= kSgdMaxSegments, FFWM_ERR_ARG, "%s: n_seg must be 1 .. %d, got %d", fn, kSgdMaxSegments, n_seg);
    FFWM_REQUIRE(n_groups >= 1 && n_groups <= kSgdMaxGroups, FFWM_ERR_ARG, "%s: n_groups must be 1 .. %d, got %d", fn, kSgdMaxGroups,
                 n_groups);
    FFWM_REQUIRE((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(momentum_buf))
                 % 16 == 0, FFWM_ERR_ARG, "%s: the three arrays must be 16-byte aligned", fn);
    FFWM_REQUIRE((reinterpret_cast<uintptr_t>(seg_end) | reinterpret_cast<uintptr_t>(group_lr) | reinterpret_cast<uintptr_t>(group_wd))
                 % 8 == 0 && reinterpret_cast<uintptr_t>(seg_group) % 4 == 0, FFWM_ERR_ARG, "%s: a table is not aligned to its element size", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n4 = (n + 3) / 4;
    int64_t blocks = (n4 + kBlock - 1) / kBlock;
    if (blocks > 256 * 16) blocks = 256 * 16;          // grid-stride: 16 workgroups per CU keep the loads in flight
    if (blocks < 1) blocks = 1;
    LaunchScope ls("sgd_flat", st, 20.0 * static_cast<double>(n));
    hipLaunchKernelGGL(sgd_flat_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, (float*)params, (const float*)grads,
                       (float*)momentum_buf, n, (const long long*)seg_end, (const int*)seg_group, n_seg, group_lr, group_wd, n_groups,
                       (float)momentum);
    return check_launch(fn);
}
