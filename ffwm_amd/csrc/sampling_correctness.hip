// sampling_correctness.hip -- the sampling-correctness loss of FlowNet pre-training for one flow scale: warp, cosine
// similarity, exp, mask and both sums in ONE pass over the channels, with the gradient for the flow.
//
// Reference: PerceptualCorrectness.calculate_loss, models/losses.py:341-371 (bilinear branch, :356-357):
//     sample   = F.grid_sample(source_vgg, flow)                       [B, C, H, W]
//     cos      = F.cosine_similarity(sample, target_vgg)               [B, H W]     (each norm clamped at 1e-8)
//     loss_map = exp(-cos / (corr_max + eps))
//     loss     = mean(loss_map) - exp(-1)      or      (sum(mask loss_map) - exp(-1)) / (sum(mask) + eps)
// The composition writes the warped [B, C, H, W] tensor, walks it several times for the cosine, and on the way back forms a
// [B, C, H, W] gradient only to contract it against the bilinear taps again.  The contraction over the channels commutes with
// the bilinear derivative: with s_c the sample of channel c, t_c the target and dx s_c, dy s_c the derivatives of the bilinear
// interpolant at the sampling position, the seven sums
//     D = sum s t    S = sum s^2    T = sum t^2    Px = sum t dx s    Py = sum t dy s    Qx = sum s dx s    Qy = sum s dy s
// give cos = D / (ns nt) (ns = max(sqrt S, 1e-8), nt likewise) and d cos / d px = Px / (ns nt) - [sqrt S > 1e-8] D Qx / (ns^3 nt),
// hence the loss map AND its flow gradient, without any intermediate tensor, atomics or second pass.
//
// Decomposition.  A 256-thread block owns PX consecutive pixels of one image's flattened H W plane and cuts the channels into
// NS contiguous slices: a wave holds PX = 64 / LS pixels x LS lane slices, the block's four waves are four more slices
// (NS = 4 LS).  LS = 1: 64 pixels per block (one 256-byte run of `target` per wave and channel), 4 slices -- calls with many
// pixels.  LS = 4: 16 pixels per block, 16 slices -- calls with few pixels and many channels (the 32 x 32 and 64 x 64 scales),
// where a lane per pixel would leave most of the chip idle.  The source taps are gathered through one buffer resource per
// image (all channels), an out-of-range tap as the offset the range check turns into 0; four channels are in flight per trip.
// The lane slices meet by an xor butterfly, the wave slices through LDS in wave order: a fixed order, so two calls agree bit
// for bit.  The first PX threads finish the pixel; wave 0 adds the block's mask * loss_map and mask in double and stores them
// in the block's slot of the workspace; a one-block launch adds the slots in a fixed order and writes out[0], out[1].
#include "bilinear.hpp"
#include "common.hpp"

namespace ffwm {
namespace {

constexpr int kScWaves = kBlock / kWave;
// LS = 4 below this many 64-pixel blocks, when there are at least kScSliceMinC channels (fixed numbers, not the device's CU
// count: the route, and with it the summation order, is a function of the shape alone)
constexpr int64_t kScFewBlocks = 1024;
constexpr int kScSliceMinC = 32;

inline int sc_lane_slices(int64_t B, int64_t C, int64_t HW) {
    return (C >= kScSliceMinC && B * ((HW + kWave - 1) / kWave) < kScFewBlocks) ? 4 : 1;
}
inline int64_t sc_blocks(int64_t B, int64_t HW, int ls) {
    const int px = kWave / ls;
    return B * ((HW + px - 1) / px);
}

__device__ __forceinline__ float sqrt_t(float v) { return sqrtf(v); }
__device__ __forceinline__ double sqrt_t(double v) { return sqrt(v); }
__device__ __forceinline__ float exp_t(float v) { return expf(v); }
__device__ __forceinline__ double exp_t(double v) { return exp(v); }

template <typename T, int LS>
__global__ void __launch_bounds__(kBlock)
sampling_correctness_kernel(const T* __restrict__ source, const T* __restrict__ target, const T* __restrict__ flow,
                            const T* __restrict__ corr_max, const T* __restrict__ mask, T* __restrict__ loss_map,
                            T* __restrict__ grad_flow, double* __restrict__ partial, int C, int Hi, int Wi, int HW, int tiles, T eps) {
    constexpr int PX = kWave / LS;
    constexpr int NS = LS * kScWaves;
    constexpr unsigned E = sizeof(T);
    __shared__ T red[7][kScWaves][PX];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int p = tile * PX + (lane & (PX - 1));
    const int pc = p < HW ? p : HW - 1;                 // the lanes past the plane shadow its last pixel and store nothing
    const size_t plane = static_cast<size_t>(HW);
    const T* fl = flow + static_cast<size_t>(b) * 2 * plane;
    Corners<T> cn;
    make_corners<T>(cn, fl[pc], fl[plane + pc], Hi, Wi);

    const int slice = wave * LS + lane / PX;
    const int cs = (C + NS - 1) / NS;
    const int c0 = slice * cs < C ? slice * cs : C;
    const int c1 = c0 + cs < C ? c0 + cs : C;
    const size_t iplane = static_cast<size_t>(Hi) * Wi;
    const unsigned istep = static_cast<unsigned>(iplane) * E;
    // one resource for the image's C planes (the host keeps C Hi Wi sizeof(T) below 2^32 - 16): the channel is part of the lane's offset
    const rsrc_t rs = make_rsrc(source + static_cast<size_t>(b) * C * iplane, static_cast<unsigned>(C * iplane * E));
    unsigned off[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) off[q] = cn.valid[q] ? cn.off[q] + static_cast<unsigned>(c0) * istep : kOob;
    const T* tp = target + (static_cast<size_t>(b) * C + c0) * plane + pc;

    T aD = 0, aS = 0, aT = 0, aPx = 0, aPy = 0, aQx = 0, aQy = 0;
    auto one = [&](const T t, const T v0, const T v1, const T v2, const T v3) {
        T s = 0;                                        // the warp kernels' order: bit-identical to WarpNet's sample
        s += v0 * cn.w[0];
        s += v1 * cn.w[1];
        s += v2 * cn.w[2];
        s += v3 * cn.w[3];
        const T dx = cn.dyw[0] * (v1 - v0) + cn.dyw[1] * (v3 - v2);
        const T dy = cn.dxw[0] * (v2 - v0) + cn.dxw[1] * (v3 - v1);
        aD += s * t;
        aS += s * s;
        aT += t * t;
        aPx += t * dx;
        aPy += t * dy;
        aQx += s * dx;
        aQy += s * dy;
    };
    constexpr int U = 4;
    int c = c0;
    for (; c + U <= c1; c += U, tp += U * plane) {
        T t[U], v[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            t[u] = tp[u * plane];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[u][q] = buf_ld<T>(rs, off[q]);
#pragma unroll
            for (int q = 0; q < 4; ++q) off[q] = cn.valid[q] ? off[q] + istep : kOob;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(t[u], v[u][0], v[u][1], v[u][2], v[u][3]);
    }
    for (; c < c1; ++c, tp += plane) {
        const T t = tp[0];
        const T v0 = buf_ld<T>(rs, off[0]), v1 = buf_ld<T>(rs, off[1]), v2 = buf_ld<T>(rs, off[2]), v3 = buf_ld<T>(rs, off[3]);
#pragma unroll
        for (int q = 0; q < 4; ++q) off[q] = cn.valid[q] ? off[q] + istep : kOob;
        one(t, v0, v1, v2, v3);
    }

    T acc[7] = {aD, aS, aT, aPx, aPy, aQx, aQy};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int o = PX; o < kWave; o <<= 1) acc[k] += __shfl_xor(acc[k], o, kWave);
        if (lane < PX) red[k][wave][lane] = acc[k];
    }
    __syncthreads();
    if (wave != 0) return;

    double sum_m = 0, sum_k = 0;
    if (lane < PX && p < HW) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            T s = red[k][0][lane];
#pragma unroll
            for (int w = 1; w < kScWaves; ++w) s += red[k][w][lane];
            acc[k] = s;
        }
        const T tiny = static_cast<T>(1e-8);            // F.cosine_similarity's eps
        const T rs_ = sqrt_t(acc[1]), rt_ = sqrt_t(acc[2]);
        const T ns = rs_ > tiny ? rs_ : tiny, nt = rt_ > tiny ? rt_ : tiny;
        const T inv = 1 / (ns * nt);
        const T cosv = acc[0] * inv;
        const size_t po = static_cast<size_t>(b) * plane + p;
        const T cm = corr_max[po] + eps;
        const T m = exp_t(-cosv / cm);
        const T k2 = rs_ > tiny ? cosv / (ns * ns) : static_cast<T>(0);
        const T cx = acc[3] * inv - k2 * acc[5];
        const T cy = acc[4] * inv - k2 * acc[6];
        const T mk = mask ? mask[po] : static_cast<T>(1);
        if (loss_map) loss_map[po] = m;
        if (grad_flow) {
            const T g = -m / cm;
            T* gp = grad_flow + static_cast<size_t>(b) * 2 * plane + p;
            gp[0] = mk * (g * cx * (static_cast<T>(Wi) / 2));
            gp[plane] = mk * (g * cy * (static_cast<T>(Hi) / 2));
        }
        sum_m = static_cast<double>(mk * m);
        sum_k = static_cast<double>(mk);
    }
    sum_m = wave_sum(sum_m);
    sum_k = wave_sum(sum_k);
    if (lane == 0) {
        partial[2 * static_cast<size_t>(blockIdx.x)] = sum_m;
        partial[2 * static_cast<size_t>(blockIdx.x) + 1] = sum_k;
    }
}

// out[0], out[1] from the blocks' slots: every thread adds its slots in index order, the threads meet in a fixed tree.
template <typename T>
__global__ void __launch_bounds__(kBlock)
sampling_correctness_reduce_kernel(const double* __restrict__ partial, int n, T* __restrict__ out, int masked, double count, double e1,
                                   double eps) {
    __shared__ double r0[kBlock], r1[kBlock];
    double a = 0, k = 0;
    for (int i = threadIdx.x; i < n; i += kBlock) {
        a += partial[2 * static_cast<size_t>(i)];
        k += partial[2 * static_cast<size_t>(i) + 1];
    }
    r0[threadIdx.x] = a;
    r1[threadIdx.x] = k;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (static_cast<int>(threadIdx.x) < s) {
            r0[threadIdx.x] += r0[threadIdx.x + s];
            r1[threadIdx.x] += r1[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (masked) {
            const double den = r1[0] + eps;
            out[0] = static_cast<T>((r0[0] - e1) / den);
            out[1] = static_cast<T>(den);
        } else {
            out[0] = static_cast<T>(r0[0] / count - e1);
            out[1] = static_cast<T>(count);
        }
    }
}

int check_sizes(const char* fn, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int dtype) {
    FFWM_REQUIRE(dtype_ok(dtype), FFWM_ERR_DTYPE, "%s: dtype %d is not FFWM_F32/FFWM_F64", fn, dtype);
    FFWM_REQUIRE(B > 0 && C > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0, FFWM_ERR_ARG,
                 "%s: sizes must be positive (B=%lld C=%lld Hi=%lld Wi=%lld H=%lld W=%lld)", fn, (long long)B, (long long)C,
                 (long long)Hi, (long long)Wi, (long long)H, (long long)W);
    const int64_t esz = dtype == FFWM_F32 ? 4 : 8;
    FFWM_REQUIRE(Hi <= (1LL << 28) / Wi && H <= (1LL << 28) / W && Hi * Wi < (1LL << 28) && H * W < (1LL << 28), FFWM_ERR_SIZE,
                 "%s: a single H*W plane must stay below 2^28 elements", fn);
    FFWM_REQUIRE(C <= ((1LL << 32) - 32) / (Hi * Wi * esz), FFWM_ERR_SIZE,
                 "%s: the C Hi Wi planes of one source image must stay below 4 GiB (32-bit byte offsets)", fn);
    FFWM_REQUIRE(B <= (1LL << 30) / ((H * W + 15) / 16), FFWM_ERR_SIZE, "%s: grid too large", fn);
    return FFWM_OK;
}

template <typename T>
int launch(const T* source, const T* target, const T* flow, const T* corr_max, const T* mask, T* loss_map, T* grad_flow, T* out,
           double* partial, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W, double e1, double eps, hipStream_t st) {
    const int64_t HW = H * W;
    const int ls = sc_lane_slices(B, C, HW);
    const int tiles = static_cast<int>((HW + kWave / ls - 1) / (kWave / ls));
    const int64_t blocks = sc_blocks(B, HW, ls);
    {
        const double pix = static_cast<double>(B) * HW;
        LaunchScope scope("sampling_correctness", st,
                          sizeof(T) * (static_cast<double>(B) * C * Hi * Wi + pix * C + 2 * pix + pix + (mask ? pix : 0.0)
                                       + (grad_flow ? 2 * pix : 0.0) + (loss_map ? pix : 0.0)));
        if (!dispatch<1, 4>(ls, [&](auto LS) {
                hipLaunchKernelGGL((sampling_correctness_kernel<T, LS.value>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st,
                                   source, target, flow, corr_max, mask, loss_map, grad_flow, partial, (int)C, (int)Hi, (int)Wi, (int)HW,
                                   tiles, static_cast<T>(eps));
            }))
            return no_kernel("ffwm_sampling_correctness");
        if (int rc = check_launch("ffwm_sampling_correctness")) return rc;
    }
    LaunchScope scope("sampling_correctness_reduce", st, 16.0 * blocks + 2.0 * sizeof(T));
    hipLaunchKernelGGL((sampling_correctness_reduce_kernel<T>), dim3(1), dim3(kBlock), 0, st, partial, static_cast<int>(blocks), out,
                       mask ? 1 : 0, static_cast<double>(B) * HW, e1, eps);
    return check_launch("ffwm_sampling_correctness(reduce)");
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int64_t ffwm_sampling_correctness_workspace_bytes(int64_t B, int64_t H, int64_t W, int dtype) {
    if (int rc = check_sizes("ffwm_sampling_correctness_workspace_bytes", B, 1, 1, 1, H, W, dtype)) return rc;
    // two doubles per block of the finer decomposition (16 pixels), whichever one the call takes
    return 16 * sc_blocks(B, H * W, 4);
}

extern "C" int ffwm_sampling_correctness(const void* source, const void* target, const void* flow, const void* corr_max,
                                         const void* mask, void* loss_map, void* grad_flow, void* out, void* workspace, int64_t B,
                                         int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W, double e1, double eps, int dtype,
                                         void* stream) {
    const char* fn = "ffwm_sampling_correctness";
    FFWM_REQUIRE(source && target && flow && corr_max && out, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(workspace, FFWM_ERR_ARG, "%s: NULL workspace (ffwm_sampling_correctness_workspace_bytes gives its size)", fn);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, FFWM_ERR_ARG, "%s: the workspace must be 8-byte aligned", fn);
    if (int rc = check_sizes(fn, B, C, Hi, Wi, H, W, dtype)) return rc;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch<T>((const T*)source, (const T*)target, (const T*)flow, (const T*)corr_max, (const T*)mask, (T*)loss_map,
                         (T*)grad_flow, (T*)out, (double*)workspace, B, C, Hi, Wi, H, W, e1, eps, static_cast<hipStream_t>(stream));
    });
}
