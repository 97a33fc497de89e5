// netg_eval.hip -- the layers around the dense convolutions of netG's eval forward (models/base_networks.py:274-347) for gfx950.
//
// With eval-mode BatchNorm folded into the convolutions (ffwm_amd/ffwm_eval.py) what remains of FFWM.forward between the
// dense convolutions is done here, one launch each, float32, forward only:
//   ffwm_shuffle_bias_act_forward       PixelShuffle(2) -> folded BatchNorm shift -> LeakyReLU of a decoder block (:261-272)
//   ffwm_image_head_forward             Conv2d(C, 3, 3, 1, 1) + bias + sigmoid (rec0 / rec1 / rec2), direct, staged through LDS
//   ffwm_upsample2x_bilinear_forward    F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) of the lower reconstruction
//   ffwm_sigmoid_gate_forward_strided   att = sigmoid(a + b), y = x * att (ffwm_sigmoid_gate_forward's arithmetic)
// Every result goes into a DESTINATION VIEW: [B, C, H, W] whose samples are contiguous, sample b at y + b * y_batch_stride -- a
// channel slice of the decoder's concatenation buffer, so cat(skip * att, dec, up(recon)) (:334-340) is never copied.
#include "common.hpp"

namespace ffwm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float lrelu_f(float v, float slope) { return v > 0.f ? v : v * slope; }      // ATen leaky_relu

constexpr int kEwBlocks = 256 * 8;      // grid-stride: 8 workgroups per CU keep the loads in flight

unsigned ew_grid(int64_t n) {
    int64_t blocks = (n + kBlock - 1) / kBlock;
    return static_cast<unsigned>(blocks > kEwBlocks ? kEwBlocks : (blocks < 1 ? 1 : blocks));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- PixelShuffle(2) + bias + LeakyReLU.  A lane owns V adjacent input pixels of the four conv channels 4k .. 4k + 3 of one row:
// V = 4: four 16-byte loads, and 2 V adjacent output pixels of the two output rows as four 16-byte stores; V = 1: scalars.
template <int V>
__global__ void __launch_bounds__(kBlock)
shuffle_bias_act_kernel(const float* __restrict__ h, const float* __restrict__ bias, float* __restrict__ y, int64_t total, int K, int H,
                        int W, int64_t ybs, float slope) {
    const int wv = W / V;
    const int64_t HW = static_cast<int64_t>(H) * W;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int xx = static_cast<int>(i % wv) * V;
        const int64_t row = i / wv;
        const int yy = static_cast<int>(row % H);
        const int64_t plane = row / H;
        const int k = static_cast<int>(plane % K);
        const int64_t b = plane / K;
        const float bk = bias ? bias[k] : 0.f;
        const float* src = h + (plane * 4) * HW + static_cast<int64_t>(yy) * W + xx;          // channel 4k of sample b
        float* dst = y + b * ybs + static_cast<int64_t>(k) * 4 * HW + static_cast<int64_t>(2 * yy) * (2 * W) + 2 * xx;
        if constexpr (V == 4) {
            const f32x4 c0 = *reinterpret_cast<const f32x4*>(src), c1 = *reinterpret_cast<const f32x4*>(src + HW);
            const f32x4 c2 = *reinterpret_cast<const f32x4*>(src + 2 * HW), c3 = *reinterpret_cast<const f32x4*>(src + 3 * HW);
            f32x4 o;
            o.x = lrelu_f(c0.x + bk, slope); o.y = lrelu_f(c1.x + bk, slope); o.z = lrelu_f(c0.y + bk, slope); o.w = lrelu_f(c1.y + bk, slope);
            reinterpret_cast<f32x4*>(dst)[0] = o;
            o.x = lrelu_f(c0.z + bk, slope); o.y = lrelu_f(c1.z + bk, slope); o.z = lrelu_f(c0.w + bk, slope); o.w = lrelu_f(c1.w + bk, slope);
            reinterpret_cast<f32x4*>(dst)[1] = o;
            o.x = lrelu_f(c2.x + bk, slope); o.y = lrelu_f(c3.x + bk, slope); o.z = lrelu_f(c2.y + bk, slope); o.w = lrelu_f(c3.y + bk, slope);
            reinterpret_cast<f32x4*>(dst + 2 * W)[0] = o;
            o.x = lrelu_f(c2.z + bk, slope); o.y = lrelu_f(c3.z + bk, slope); o.z = lrelu_f(c2.w + bk, slope); o.w = lrelu_f(c3.w + bk, slope);
            reinterpret_cast<f32x4*>(dst + 2 * W)[1] = o;
        } else {
            dst[0] = lrelu_f(src[0] + bk, slope);
            dst[1] = lrelu_f(src[HW] + bk, slope);
            dst[2 * W] = lrelu_f(src[2 * HW] + bk, slope);
            dst[2 * W + 1] = lrelu_f(src[3 * HW] + bk, slope);
        }
    }
}

// ---- bilinear x 2, align_corners = False.  Output index d reads source coordinate max((d + 0.5) / 2 - 0.5, 0): neighbours i0 and
// min(i0 + 1, n - 1) with weights (1 - l, l), l in {0, 0.25, 0.75} -- ATen's upsample_bilinear2d arithmetic.
struct Tap {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Tap up2_tap(int d, int n) {
    Tap t;
    const int s = d >> 1;
    if (d & 1) {
        t.i0 = s; t.w0 = 0.75f; t.w1 = 0.25f;
    } else if (s == 0) {
        t.i0 = 0; t.w0 = 1.f; t.w1 = 0.f;
    } else {
        t.i0 = s - 1; t.w0 = 0.25f; t.w1 = 0.75f;
    }
    t.i1 = t.i0 + 1 < n ? t.i0 + 1 : n - 1;
    return t;
}

// A lane owns V adjacent output pixels of one output row (V = 4: one 16-byte store).
template <int V>
__global__ void __launch_bounds__(kBlock)
upsample2x_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total, int C, int H, int W, int64_t ybs) {
    const int Ho = 2 * H, Wo = 2 * W, wv = Wo / V;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int xo = static_cast<int>(i % wv) * V;
        const int64_t row = i / wv;
        const int yo = static_cast<int>(row % Ho);
        const int64_t plane = row / Ho;
        const int c = static_cast<int>(plane % C);
        const int64_t b = plane / C;
        const Tap ty = up2_tap(yo, H);
        const float* r0 = x + plane * H * W + static_cast<int64_t>(ty.i0) * W;
        const float* r1 = x + plane * H * W + static_cast<int64_t>(ty.i1) * W;
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const Tap tx = up2_tap(xo + j, W);
            o[j] = ty.w0 * (tx.w0 * r0[tx.i0] + tx.w1 * r0[tx.i1]) + ty.w1 * (tx.w0 * r1[tx.i0] + tx.w1 * r1[tx.i1]);
        }
        float* dst = y + b * ybs + (static_cast<int64_t>(c) * Ho + yo) * Wo + xo;
        if constexpr (V == 4) {
            const f32x4 v = {o[0], o[1], o[2], o[3]};
            *reinterpret_cast<f32x4*>(dst) = v;
        } else {
            dst[0] = o[0];
        }
    }
}

// ---- att = sigmoid(a + b), y = x * att with y in a destination view (att, optional, contiguous): gate_fwd_kernel of residual.hip,
// sample by sample
template <int V, bool ATT>
__global__ void __launch_bounds__(kBlock)
gate_strided_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ x, float* __restrict__ att,
                    float* __restrict__ y, int64_t total, int64_t chw, int64_t ybs) {
    const int64_t per = chw / V;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t s = i / per;
        const int64_t src = s * chw + (i - s * per) * V, dst = s * ybs + (i - s * per) * V;
        if constexpr (V == 4) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(a + src), bv = *reinterpret_cast<const f32x4*>(b + src);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + src);
            f32x4 g, r;
            g.x = sigmoid_f(av.x + bv.x); g.y = sigmoid_f(av.y + bv.y); g.z = sigmoid_f(av.z + bv.z); g.w = sigmoid_f(av.w + bv.w);
            r.x = xv.x * g.x; r.y = xv.y * g.y; r.z = xv.z * g.z; r.w = xv.w * g.w;
            if constexpr (ATT) *reinterpret_cast<f32x4*>(att + src) = g;
            *reinterpret_cast<f32x4*>(y + dst) = r;
        } else {
            const float g = sigmoid_f(a[src] + b[src]);
            if constexpr (ATT) att[src] = g;
            y[dst] = x[src] * g;
        }
    }
}

// ---- image head: Conv2d(C, 3, 3, 1, 1) + bias + sigmoid, direct.  A workgroup owns a tile of 8 rows x 8 PX pixels of one sample; a
// lane owns PX adjacent pixels of a row and the three output channels.  The input is walked in chunks of kHeadChunk channels staged
// through LDS with their one-pixel halo (zeros outside the image and past channel C); the four waves split a chunk's channels, take
// the 27 weights of a channel as scalar operands, and their partial sums meet in LDS in wave order: no atomics, any H and W.
constexpr int kHeadChunk = 16;
constexpr int kHeadRows = 8;

template <int PX>
struct HeadTile {
    static constexpr int kCols = 8 * PX;                      // output pixels per tile row
    static constexpr int kStride = (kCols + 2 + 3) / 4 * 4 + 1;  // LDS row stride in floats (odd: rows start on different banks)
    static constexpr int kPlane = (kHeadRows + 2) * kStride;
    static constexpr int kStage = kHeadChunk * kPlane;
    static constexpr int kReduce = 4 * 3 * kWave * PX;
    static constexpr int kLds = kStage > kReduce ? kStage : kReduce;
};

template <int PX>
__global__ void __launch_bounds__(kBlock)
image_head_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y, int C,
                  int H, int W, int tiles_x, int tiles_y, int64_t ybs, int vec) {
    using T = HeadTile<PX>;
    __shared__ float lds[T::kLds];
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    unsigned t = blockIdx.x;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int x0 = tx * T::kCols, y0 = ty * kHeadRows;
    const int lx = (lane & 7) * PX, ly = lane >> 3;           // the lane's first pixel inside the tile
    const int64_t HW = static_cast<int64_t>(H) * W;
    const float* xb = x + static_cast<int64_t>(b) * C * HW;
    float acc[3][PX];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int p = 0; p < PX; ++p) acc[k][p] = 0.f;

    constexpr int kHaloCols = T::kCols + 2, kHaloRows = kHeadRows + 2;
    for (int c0 = 0; c0 < C; c0 += kHeadChunk) {
        __syncthreads();                                       // the previous chunk has been read
        for (int e = threadIdx.x; e < kHeadChunk * kHaloRows * kHaloCols; e += kBlock) {
            const int j = e % kHaloCols, r = (e / kHaloCols) % kHaloRows, cl = e / (kHaloCols * kHaloRows);
            const int gx = x0 - 1 + j, gy = y0 - 1 + r, c = c0 + cl;
            float v = 0.f;
            if (c < C && gx >= 0 && gx < W && gy >= 0 && gy < H) v = xb[static_cast<int64_t>(c) * HW + static_cast<int64_t>(gy) * W + gx];
            lds[cl * T::kPlane + r * T::kStride + j] = v;
        }
        __syncthreads();
        for (int cl = wave; cl < kHeadChunk; cl += kBlock / kWave) {
            const int c = c0 + cl;                             // wave-uniform
            if (c >= C) break;
            const float* tile = lds + cl * T::kPlane + ly * T::kStride + lx;
            const float* w0 = w + static_cast<int64_t>(c) * 9;                          // w[0][c][:][:]
            const float* w1 = w + (static_cast<int64_t>(C) + c) * 9;
            const float* w2 = w + (2 * static_cast<int64_t>(C) + c) * 9;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float in[PX + 2];
#pragma unroll
                for (int j = 0; j < PX + 2; ++j) in[j] = tile[r * T::kStride + j];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const float a0 = w0[r * 3 + s], a1 = w1[r * 3 + s], a2 = w2[r * 3 + s];
#pragma unroll
                    for (int p = 0; p < PX; ++p) {
                        acc[0][p] = __builtin_fmaf(a0, in[p + s], acc[0][p]);
                        acc[1][p] = __builtin_fmaf(a1, in[p + s], acc[1][p]);
                        acc[2][p] = __builtin_fmaf(a2, in[p + s], acc[2][p]);
                    }
                }
            }
        }
    }
    __syncthreads();                                           // the staging area becomes the reduction area
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int p = 0; p < PX; ++p) lds[((wave * 3 + k) * kWave + lane) * PX + p] = acc[k][p];
    __syncthreads();
    if (threadIdx.x >= 3 * kWave) return;
    const int k = threadIdx.x / kWave;                         // thread (k, lane) folds the four waves' sums of its PX pixels
    const int gx = x0 + lx, gy = y0 + ly;
    if (gy >= H || gx >= W) return;
    const float bk = bias ? bias[k] : 0.f;
    float o[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        float s = lds[((0 * 3 + k) * kWave + lane) * PX + p];
#pragma unroll
        for (int wv = 1; wv < kBlock / kWave; ++wv) s += lds[((wv * 3 + k) * kWave + lane) * PX + p];
        o[p] = sigmoid_f(s + bk);
    }
    float* dst = y + static_cast<int64_t>(b) * ybs + static_cast<int64_t>(k) * HW + static_cast<int64_t>(gy) * W + gx;
    if constexpr (PX == 4) {
        if (vec) {                                             // W % 4 == 0: the four pixels are inside the row, 16-byte aligned
            const f32x4 v = {o[0], o[1], o[2], o[3]};
            *reinterpret_cast<f32x4*>(dst) = v;
            return;
        }
    }
#pragma unroll
    for (int p = 0; p < PX; ++p)
        if (gx + p < W) dst[p] = o[p];
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

// y[b, k, 2 yy + i, 2 xx + j] = lrelu(h[b, 4 k + 2 i + j, yy, xx] + bias[k]); h [B, 4 K, H, W] contiguous, y a destination view
// [B, K, 2 H, 2 W] with batch stride y_batch_stride >= K * 4 * H * W.  bias may be NULL.
extern "C" int ffwm_shuffle_bias_act_forward(const void* h, const void* bias, void* y, int64_t B, int64_t K, int64_t H, int64_t W,
                                             int64_t y_batch_stride, double negative_slope, int dtype, void* stream) {
    const char* fn = "ffwm_shuffle_bias_act_forward";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(h && y, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(H < (1LL << 15) && W < (1LL << 15), FFWM_ERR_SIZE, "%s: plane too large", fn);
    FFWM_REQUIRE(y_batch_stride >= K * 4 * H * W, FFWM_ERR_ARG, "%s: the destination batch stride is smaller than K * 4 * H * W", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = W % 4 == 0 && aligned16(h) && aligned16(y) && y_batch_stride % 4 == 0;
    const int64_t total = B * K * H * (vec ? W / 4 : W);
    LaunchScope ls("netg_shuffle_bias_act", st, 4.0 * 8.0 * B * K * H * W);
    const bool ok = dispatch<4, 1>(vec ? 4 : 1, [&](auto V) {
        hipLaunchKernelGGL((shuffle_bias_act_kernel<V.value>), dim3(ew_grid(total)), dim3(kBlock), 0, st, (const float*)h, (const float*)bias,
                           (float*)y, total, (int)K, (int)H, (int)W, y_batch_stride, (float)negative_slope);
    });
    return ok ? check_launch(fn) : no_kernel(fn);
}

// y = sigmoid(conv2d(x[B, C, H, W], weight[3, C, 3, 3], stride 1, pad 1) + bias[3]) into a destination view [B, 3, H, W]
// (y_batch_stride >= 3 * H * W).  bias may be NULL.
extern "C" int ffwm_image_head_forward(const void* x, const void* weight, const void* bias, void* y, int64_t B, int64_t C, int64_t H,
                                       int64_t W, int64_t y_batch_stride, int dtype, void* stream) {
    const char* fn = "ffwm_image_head_forward";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(x && weight && y, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(H < (1LL << 15) && W < (1LL << 15) && C < (1LL << 20), FFWM_ERR_SIZE, "%s: plane too large", fn);
    FFWM_REQUIRE(y_batch_stride >= 3 * H * W, FFWM_ERR_ARG, "%s: the destination batch stride is smaller than 3 * H * W", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto blocks = [&](int64_t px) { return B * ((H + kHeadRows - 1) / kHeadRows) * ((W + 8 * px - 1) / (8 * px)); };
    // four pixels per lane once that still gives every CU a workgroup, else one (the 32 x 32 level, small batches)
    const int px = blocks(4) >= device_cus() ? 4 : 1;
    FFWM_REQUIRE(blocks(px) < (1LL << 31), FFWM_ERR_SIZE, "%s: too many tiles", fn);
    const int tiles_x = static_cast<int>((W + 8 * px - 1) / (8 * px)), tiles_y = static_cast<int>((H + kHeadRows - 1) / kHeadRows);
    const int vec = W % 4 == 0 && aligned16(y) && y_batch_stride % 4 == 0;
    LaunchScope ls("netg_image_head", st, 4.0 * (B * C * H * W + 27.0 * C + 3.0 * B * H * W), 2.0 * 27.0 * B * C * H * W);
    const bool ok = dispatch<4, 1>(px, [&](auto PX) {
        hipLaunchKernelGGL((image_head_kernel<PX.value>), dim3(static_cast<unsigned>(blocks(px))), dim3(kBlock), 0, st, (const float*)x,
                           (const float*)weight, (const float*)bias, (float*)y, (int)C, (int)H, (int)W, tiles_x, tiles_y, y_batch_stride, vec);
    });
    return ok ? check_launch(fn) : no_kernel(fn);
}

// F.interpolate(x[B, C, H, W], scale_factor=2, mode="bilinear", align_corners=False) into a destination view [B, C, 2 H, 2 W]
// (y_batch_stride >= C * 4 * H * W).
extern "C" int ffwm_upsample2x_bilinear_forward(const void* x, void* y, int64_t B, int64_t C, int64_t H, int64_t W, int64_t y_batch_stride,
                                                int dtype, void* stream) {
    const char* fn = "ffwm_upsample2x_bilinear_forward";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(x && y, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(H < (1LL << 14) && W < (1LL << 14), FFWM_ERR_SIZE, "%s: plane too large", fn);
    FFWM_REQUIRE(y_batch_stride >= C * 4 * H * W, FFWM_ERR_ARG, "%s: the destination batch stride is smaller than C * 4 * H * W", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = W % 2 == 0 && aligned16(y) && y_batch_stride % 4 == 0;
    const int64_t total = B * C * 2 * H * (vec ? W / 2 : 2 * W);
    LaunchScope ls("netg_upsample2x", st, 4.0 * 5.0 * B * C * H * W);
    const bool ok = dispatch<4, 1>(vec ? 4 : 1, [&](auto V) {
        hipLaunchKernelGGL((upsample2x_kernel<V.value>), dim3(ew_grid(total)), dim3(kBlock), 0, st, (const float*)x, (float*)y, total, (int)C,
                           (int)H, (int)W, y_batch_stride);
    });
    return ok ? check_launch(fn) : no_kernel(fn);
}

// att = sigmoid(a + b), y = x * att: a, b, x (and att, NULL: not written) [B, C, HW] contiguous, y a destination view with batch
// stride y_batch_stride >= C * HW.  ffwm_sigmoid_gate_forward's arithmetic in its order.
extern "C" int ffwm_sigmoid_gate_forward_strided(const void* a, const void* b, const void* x, void* att, void* y, int64_t B, int64_t C,
                                                 int64_t HW, int64_t y_batch_stride, int dtype, void* stream) {
    const char* fn = "ffwm_sigmoid_gate_forward_strided";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(a && b && x && y, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && C > 0 && HW > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(HW < (1LL << 31) && C < (1LL << 31), FFWM_ERR_SIZE, "%s: plane too large", fn);
    FFWM_REQUIRE(y_batch_stride >= C * HW, FFWM_ERR_ARG, "%s: the destination batch stride is smaller than C * HW", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t chw = C * HW;
    const bool vec = chw % 4 == 0 && y_batch_stride % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(x) && aligned16(y) &&
                     (!att || aligned16(att));
    const int64_t total = B * (vec ? chw / 4 : chw);
    LaunchScope ls("netg_sigmoid_gate", st, 4.0 * (att ? 5.0 : 4.0) * B * chw);
    const bool ok = dispatch<4, 1>(vec ? 4 : 1, [&](auto V) {
        return dispatch<false, true>(att != nullptr, [&](auto ATT) {
            hipLaunchKernelGGL((gate_strided_kernel<V.value, ATT.value>), dim3(ew_grid(total)), dim3(kBlock), 0, st, (const float*)a,
                               (const float*)b, (const float*)x, (float*)att, (float*)y, total, chw, y_batch_stride);
        });
    });
    return ok ? check_launch(fn) : no_kernel(fn);
}
