// identity_batch.hip -- the input pipeline of LightCNN fine-tuning (lightcnn/dataset.py with --preload) from a DEVICE-RESIDENT store:
//   ffwm_identity_batch  one launch assembles a whole batch: img [B, 1, Ho, Wo] and target [B] from images uint8 [N, H, W, 3] and
//                        DEVICE vectors of item indices, rotation matrices and flips (a captured launch follows their contents).
// A training item is RandomRotation(5, BICUBIC) -> RandomHorizontalFlip -> ToTensor -> channel mean (-> --crop); the rotation is
// PIL's Image.rotate, restated here operation by operation in float64 ("identity batches"), so the bytes it produces are
// PIL's bytes:
//   xin = m0 (x + .5) + m1 (y + .5) + m2, yin = m3 (x + .5) + m4 (y + .5) + m5; outside [0, W) x [0, H): 0, tested BEFORE any
//   conversion to an integer (so every finite matrix is safe); else the a = -1 cubic over 4 x 4 index-clamped taps around
//   (xin - .5, yin - .5), rows first, clipped to [0, 255] and truncated.
// The build passes -ffp-contract=off: no product-sum below may become an FMA.
// Then byte / 255 (a true division) and ((r + g) + b) / 3 as face_gallery_kernel has them, and with `crop` the slice [28:-2, 15:-15]
// of that plane resized to out_side x out_side as ATen's upsample_bilinear2d (align_corners false) does it in float32.
//
// Ownership: every element of img has one owner thread and is written once by a plain store; target[b] and invalid[b] are written by
// thread 0 of the sample's first block; nothing else is written.
//   * without crop a thread owns one pixel: 16 taps x 3 channels straight from the image (48 KB at 128 x 128: it stays in cache);
//   * with crop a block owns a band of kBandRows output rows of one sample: it works out the rows of the mean plane that the band's
//     bilinear taps read into LDS (each plane pixel pays its 48-tap float64 cubic once, not once per use), then interpolates from LDS.
// A sample whose index is outside [0, N) or whose matrix has an entry that is not finite is never turned into an address: zeros,
// target 0, invalid[b] = 1.
#include "common.hpp"

namespace ffwm {
namespace {

constexpr int kMaxSide = 8192;
constexpr int kBandRows = 8;                                   // output rows of a block of the crop kernel
constexpr int kCropTop = 28, kCropBottom = 2, kCropSide = 15;          // img[:, 28:-2, 15:-15] (dataset.py:64)
constexpr int kMaxPlaneBytes = 64 * 1024;                      // LDS of the crop kernel

struct IdentityArgs {
    const unsigned char* images;          // [N, H, W, 3]
    const long long* targets;             // [N]
    const int* index;                     // [B]
    const double* matrix;                 // [B, 6], augment only
    const unsigned char* flip;            // [B], augment only
    float* img;                           // [B, 1, Ho, Wo]
    long long* target;                    // [B]
    int* invalid;                         // [B]
    long long N;
    int H, W, augment, units;             // units: blocks per sample
    int out_side, in_h, in_w, max_rows;   // crop: the plane slice is in_h x in_w; max_rows: plane rows a band needs at most
    float scale_h, scale_w;               // crop: in / out as ATen computes it (float(in) / out)
};

// What sample b reads, or ok = false.  Every block of a sample decides alike: the inputs are not written during the launch.
struct Sample {
    bool ok, flip;
    long long row;
    double m[6];
};
__device__ __forceinline__ Sample decode_sample(const IdentityArgs& a, int b) {
    Sample s;
    const int i = a.index[b];
    s.ok = i >= 0 && i < a.N;
    s.flip = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) s.m[k] = 0.0;
    if (a.augment) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            s.m[k] = a.matrix[6 * static_cast<long long>(b) + k];
            s.ok = s.ok && fabs(s.m[k]) <= 1.7976931348623157e308;          // false for inf and for NaN
        }
        s.flip = a.flip[b] != 0;
    }
    s.row = s.ok ? i : 0;
    return s;
}

// PIL's BICUBIC macro (a = -1), in its operation order.
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2.0 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

__device__ __forceinline__ int clamp_tap(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// Pixel (x, y) of Image.rotate(..., BICUBIC) of the H x W x 3 image `im` under the matrix m: its three bytes.
__device__ __forceinline__ void rotated_pixel(const unsigned char* __restrict__ im, int H, int W, const double* m, int x, int y, int* rgb) {
    const double xs = x + 0.5, ys = y + 0.5;
    double xin = m[0] * xs + m[1] * ys + m[2];
    double yin = m[3] * xs + m[4] * ys + m[5];
    rgb[0] = rgb[1] = rgb[2] = 0;
    if (!(xin >= 0.0 && xin < static_cast<double>(W) && yin >= 0.0 && yin < static_cast<double>(H))) return;          // (NaN lands here too)
    xin -= 0.5;
    yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);          // in [-1, W - 1] and [-1, H - 1]
    const double dx = xin - fx, dy = yin - fy;
    const int x0 = static_cast<int>(fx) - 1, y0 = static_cast<int>(fy) - 1;
    int xo[4];
    const unsigned char* rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xo[k] = 3 * clamp_tap(x0 + k, W);
        rows[k] = im + 3 * (static_cast<long long>(clamp_tap(y0 + k, H)) * W);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            r[k] = cubic(static_cast<double>(rows[k][xo[0] + c]), static_cast<double>(rows[k][xo[1] + c]),
                         static_cast<double>(rows[k][xo[2] + c]), static_cast<double>(rows[k][xo[3] + c]), dx);
        const double v = cubic(r[0], r[1], r[2], r[3], dy);
        rgb[c] = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : static_cast<int>(v));          // clipped, then truncated
    }
}

// Pixel (x, y) of the item's mean plane [1, H, W]: rotate, flip, / 255, channel mean.
__device__ __forceinline__ float mean_pixel(const IdentityArgs& a, const Sample& s, const unsigned char* __restrict__ im, int x, int y) {
    int rgb[3];
    if (a.augment) {
        rotated_pixel(im, a.H, a.W, s.m, s.flip ? a.W - 1 - x : x, y, rgb);
    } else {
        const unsigned char* p = im + 3 * (static_cast<long long>(y) * a.W + x);
        rgb[0] = p[0];
        rgb[1] = p[1];
        rgb[2] = p[2];
    }
    float v = static_cast<float>(rgb[0]) / 255.0f;
    v += static_cast<float>(rgb[1]) / 255.0f;
    v += static_cast<float>(rgb[2]) / 255.0f;
    return v / 3.0f;
}

__device__ __forceinline__ void write_sample_row(const IdentityArgs& a, const Sample& s, int b) {
    a.invalid[b] = s.ok ? 0 : 1;
    a.target[b] = s.ok ? a.targets[s.row] : 0LL;
}

// Without crop: block `unit` of sample b owns pixels [unit kBlock, unit kBlock + kBlock) of the plane.
__global__ void __launch_bounds__(kBlock) identity_plain_kernel(const IdentityArgs a) {
    const int b = blockIdx.x / a.units, unit = blockIdx.x - b * a.units;
    const Sample s = decode_sample(a, b);
    if (unit == 0 && threadIdx.x == 0) write_sample_row(a, s, b);
    const int HW = a.H * a.W, p = unit * kBlock + static_cast<int>(threadIdx.x);
    if (p >= HW) return;
    float v = 0.f;
    if (s.ok) {
        const int y = p / a.W;
        v = mean_pixel(a, s, a.images + 3 * s.row * HW, p - y * a.W, y);
    }
    a.img[static_cast<long long>(b) * HW + p] = v;
}

// ATen's area_pixel_compute_source_index (align_corners false, not cubic) in float32.
__host__ __device__ inline float source_index(float scale, int dst) {
    const float src = scale * (static_cast<float>(dst) + 0.5f) - 0.5f;
    return src < 0.f ? 0.f : src;
}
// The plane rows [lo, hi] that output rows [y0, y0 + n) read.
__host__ __device__ inline void band_rows(float scale, int y0, int n, int in_h, int* lo, int* hi) {
    *lo = static_cast<int>(source_index(scale, y0));
    const int last = static_cast<int>(source_index(scale, y0 + n - 1)) + 1;
    *hi = last < in_h - 1 ? last : in_h - 1;
    if (*lo > *hi) *lo = *hi;
}

// With crop: block `unit` of sample b owns output rows [unit kBandRows, ...) of the out_side x out_side plane.
__global__ void __launch_bounds__(kBlock) identity_crop_kernel(const IdentityArgs a) {
    extern __shared__ float plane[];          // [rows of the band][in_w]
    const int b = blockIdx.x / a.units, unit = blockIdx.x - b * a.units;
    const Sample s = decode_sample(a, b);
    if (unit == 0 && threadIdx.x == 0) write_sample_row(a, s, b);
    const int S = a.out_side, y0 = unit * kBandRows;
    const int n = kBandRows < S - y0 ? kBandRows : S - y0;
    float* out = a.img + (static_cast<long long>(b) * S + y0) * S;
    if (!s.ok) {
        for (int i = threadIdx.x; i < n * S; i += kBlock) out[i] = 0.f;
        return;
    }
    int lo, hi;
    band_rows(a.scale_h, y0, n, a.in_h, &lo, &hi);
    int rows = hi - lo + 1;
    rows = rows < a.max_rows ? rows : a.max_rows;          // (equal by construction: the host ran band_rows over every band)
    const unsigned char* im = a.images + 3 * s.row * a.H * a.W;
    for (int i = threadIdx.x; i < rows * a.in_w; i += kBlock) {
        const int r = i / a.in_w;
        plane[i] = mean_pixel(a, s, im, kCropSide + (i - r * a.in_w), kCropTop + lo + r);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n * S; i += kBlock) {
        const int oy = i / S, ox = i - oy * S;
        const float h1r = source_index(a.scale_h, y0 + oy), w1r = source_index(a.scale_w, ox);
        int h1 = static_cast<int>(h1r), w1 = static_cast<int>(w1r);
        h1 = h1 < a.in_h - 1 ? h1 : a.in_h - 1;          // (as ATen guards its index)
        w1 = w1 < a.in_w - 1 ? w1 : a.in_w - 1;
        const int h1p = h1 < a.in_h - 1 ? 1 : 0, w1p = w1 < a.in_w - 1 ? 1 : 0;
        const float h1l = h1r - static_cast<float>(h1), h0l = 1.f - h1l, w1l = w1r - static_cast<float>(w1), w0l = 1.f - w1l;
        const int r0 = clamp_tap(h1 - lo, rows), r1 = clamp_tap(h1 + h1p - lo, rows);          // (no clamp acts: the band's rows cover every tap)
        const float* p0 = plane + r0 * a.in_w + w1;
        const float* p1 = plane + r1 * a.in_w + w1;
        out[i] = h0l * (w0l * p0[0] + w1l * p0[w1p]) + h1l * (w0l * p1[0] + w1l * p1[w1p]);
    }
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_identity_batch(const void* images, const void* targets, const void* index, const void* matrix, const void* flip,
                                   void* img, void* target, void* invalid, int64_t N, int64_t H, int64_t W, int64_t B,
                                   int64_t out_side, int augment, int crop, void* stream) {
    const char* fn = "ffwm_identity_batch";
    FFWM_REQUIRE((augment == 0 || augment == 1) && (crop == 0 || crop == 1), FFWM_ERR_ARG, "%s: augment and crop must be 0 or 1", fn);
    FFWM_REQUIRE(images && targets && index && img && target && invalid, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(!augment || (matrix && flip), FFWM_ERR_ARG, "%s: NULL tensor pointer (an augmented batch needs the matrices and the flips)",
                 fn);
    FFWM_REQUIRE(N > 0 && H > 0 && W > 0 && B > 0 && (!crop || out_side > 0), FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(!crop || (H > kCropTop + kCropBottom && W > 2 * kCropSide), FFWM_ERR_ARG,
                 "%s: crop takes [%d:-%d, %d:-%d] of the plane: H and W must exceed 30", fn, kCropTop, kCropBottom, kCropSide, kCropSide);
    FFWM_REQUIRE(H <= kMaxSide && W <= kMaxSide && (!crop || out_side <= kMaxSide), FFWM_ERR_SIZE, "%s: H, W and out_side up to %d", fn,
                 kMaxSide);
    FFWM_REQUIRE(N < (1LL << 31) && B <= 65535, FFWM_ERR_SIZE, "%s: tensor too large", fn);
    IdentityArgs a;
    a.images = static_cast<const unsigned char*>(images);
    a.targets = static_cast<const long long*>(targets);
    a.index = static_cast<const int*>(index);
    a.matrix = augment ? static_cast<const double*>(matrix) : nullptr;
    a.flip = augment ? static_cast<const unsigned char*>(flip) : nullptr;
    a.img = static_cast<float*>(img);
    a.target = static_cast<long long*>(target);
    a.invalid = static_cast<int*>(invalid);
    a.N = N;
    a.H = static_cast<int>(H);
    a.W = static_cast<int>(W);
    a.augment = augment;
    a.out_side = a.in_h = a.in_w = a.max_rows = 0;
    a.scale_h = a.scale_w = 0.f;
    size_t lds = 0;
    if (crop) {
        a.out_side = static_cast<int>(out_side);
        a.in_h = a.H - kCropTop - kCropBottom;
        a.in_w = a.W - 2 * kCropSide;
        a.scale_h = static_cast<float>(a.in_h) / static_cast<float>(a.out_side);
        a.scale_w = static_cast<float>(a.in_w) / static_cast<float>(a.out_side);
        a.units = (a.out_side + kBandRows - 1) / kBandRows;
        for (int u = 0; u < a.units; ++u) {
            int lo, hi;
            const int y0 = u * kBandRows;
            band_rows(a.scale_h, y0, kBandRows < a.out_side - y0 ? kBandRows : a.out_side - y0, a.in_h, &lo, &hi);
            a.max_rows = hi - lo + 1 > a.max_rows ? hi - lo + 1 : a.max_rows;
        }
        lds = static_cast<size_t>(a.max_rows) * a.in_w * sizeof(float);
        FFWM_REQUIRE(lds <= static_cast<size_t>(kMaxPlaneBytes), FFWM_ERR_SIZE,
                     "%s: a band of %d output rows reads %d plane rows of %d pixels: more than %d bytes of LDS", fn, kBandRows, a.max_rows,
                     a.in_w, kMaxPlaneBytes);
    } else {
        a.units = static_cast<int>((H * W + kBlock - 1) / kBlock);
    }
    FFWM_REQUIRE(B * a.units < (1LL << 31), FFWM_ERR_SIZE, "%s: tensor too large", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double px_out = crop ? 1.0 * B * out_side * out_side : 1.0 * B * H * W;
    LaunchScope ls(crop ? "identity_batch_crop" : "identity_batch", st, 3.0 * B * H * W + 4.0 * px_out);
    const dim3 grid(static_cast<unsigned>(B * a.units));
    if (crop)
        hipLaunchKernelGGL(identity_crop_kernel, grid, dim3(kBlock), lds, st, a);
    else
        hipLaunchKernelGGL(identity_plain_kernel, grid, dim3(kBlock), 0, st, a);
    return check_launch(fn);
}
