// lightcnn_eval.hip -- what the reference's identity evaluation needs around the LightCNN convolutions, one pass each.
//
// Reference: test_ffwm.py frontalises a profile, takes the LightCNN-29 feature of the result (models/ffwm_model.py:191-202) and
// ranks it against the gallery's features (util/util.py:141-181).  Around the 29 convolutions of lightcnn/light_cnn.py:82-129 ATen
// runs, per layer, the bias add, the maximum of two strided halves, for a residual block the add, and in front of four layers a
// MaxPool2d(2, 2, ceil_mode=True); in front of the network the channel mean and -- with --crop -- a grid_sample and a bilinear
// resize (models/losses.py:85-90); behind it one cosine_similarity + topk per probe.  Here:
//
//   ffwm_mfm_tail_forward   y = pool(max(h[:, :C] + bias[:C], h[:, C:] + bias[C:]) + residual): every step one rounding or an exact
//                           selection, in ATen's order, so the result equals the PyTorch composition bit for bit.  NaN as ATen:
//                           maximum and max_pool2d propagate it (the pool's own rule: `val > max || isnan(val)`, in window order).
//   ffwm_identity_input     the network's input: the channel mean, or (crop) mean -> WarpNet(build_grid(b, 98)) -> resize to 128 as
//                           one 16-tap gather per output pixel.
//   ffwm_identity_input_backward  its adjoint, for training against the cropped-face identity loss (models/losses.py:76-112 with
//                           crop=True): grad_out / Cin into every channel, or (crop) A_y^T g A_x / Cin as two separable gather passes
//                           through LDS -- no atomics, every element of grad_img written once, exact zeros outside the crop.
//   ffwm_cosine_topk        cosine similarities of B probes against G gallery rows and the k best per probe, without float
//                           atomics: a similarity pass (a wave per gallery row, eight probes per block held in LDS), a selection
//                           per (probe, segment of the gallery), a merge per probe.  Selection is on 64-bit keys (ordered value,
//                           ~index), so ties go to the lower index and every stage is deterministic.
#include "common.hpp"

namespace ffwm {
namespace {

// ATen's maximum: NaN when either operand is (fmaxf alone returns the other operand)
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_isunordered(a, b) ? a + b : fmaxf(a, b); }
// one step of ATen's max_pool2d window scan
__device__ __forceinline__ float pool_step(float m, float v) { return (v > m || v != v) ? v : m; }

constexpr int kEwBlocks = 256 * 8;          // grid cap of the grid-stride kernels: 8 blocks per CU
unsigned ew_grid(int64_t items) {
    const int64_t blocks = (items + kBlock - 1) / kBlock;
    return static_cast<unsigned>(blocks > kEwBlocks ? kEwBlocks : (blocks < 1 ? 1 : blocks));
}

// ------------------------------------------------------------------------------------------------ mfm tail
struct TailArgs {
    const float* h;
    const float* bias;
    const float* res;
    float* y;
    int C, H, W, Ho, Wo;
};

// max(h_a + bias_a, h_b + bias_b) + residual of element `off` of plane (b, c); ha = h + ((b 2C + c) H W), hb = ha + C H W
__device__ __forceinline__ float tail_elem(float a, float b, float ba, float bb, bool has_bias, bool has_res, float r) {
    const float m = has_bias ? max_nan(a + ba, b + bb) : max_nan(a, b);
    return has_res ? m + r : m;
}

// one output element per item, any W
template <bool POOL>
__global__ void __launch_bounds__(kBlock) mfm_tail_kernel(TailArgs p, int64_t total) {
    const int64_t plane = static_cast<int64_t>(p.H) * p.W;
    const bool hb_ = p.bias != nullptr, hr_ = p.res != nullptr;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int ox = static_cast<int>(i % p.Wo);
        int64_t t = i / p.Wo;
        const int oy = static_cast<int>(t % p.Ho);
        t /= p.Ho;
        const int c = static_cast<int>(t % p.C);
        const int64_t b = t / p.C;
        const float* ha = p.h + (b * 2 * p.C + c) * plane;
        const float* hb = ha + static_cast<int64_t>(p.C) * plane;
        const float* r = hr_ ? p.res + (b * p.C + c) * plane : nullptr;
        const float ba = hb_ ? p.bias[c] : 0.f, bb = hb_ ? p.bias[p.C + c] : 0.f;
        if (!POOL) {
            const int64_t o = static_cast<int64_t>(oy) * p.W + ox;
            p.y[i] = tail_elem(ha[o], hb[o], ba, bb, hb_, hr_, hr_ ? r[o] : 0.f);
        } else {
            float m = 0.f;
            bool first = true;
            for (int dy = 0; dy < 2; ++dy) {
                const int iy = 2 * oy + dy;
                if (iy >= p.H) break;
                for (int dx = 0; dx < 2; ++dx) {
                    const int ix = 2 * ox + dx;
                    if (ix >= p.W) break;
                    const int64_t o = static_cast<int64_t>(iy) * p.W + ix;
                    const float v = tail_elem(ha[o], hb[o], ba, bb, hb_, hr_, hr_ ? r[o] : 0.f);
                    m = first ? v : pool_step(m, v);
                    first = false;
                }
            }
            p.y[i] = m;
        }
    }
}

__device__ __forceinline__ float4 tail_elem4(float4 a, float4 b, float ba, float bb, bool has_bias, bool has_res, float4 r) {
    return float4{tail_elem(a.x, b.x, ba, bb, has_bias, has_res, r.x), tail_elem(a.y, b.y, ba, bb, has_bias, has_res, r.y),
                  tail_elem(a.z, b.z, ba, bb, has_bias, has_res, r.z), tail_elem(a.w, b.w, ba, bb, has_bias, has_res, r.w)};
}

// W % 4 == 0, no pool: four outputs per item, 16-byte loads and stores (a float4 never straddles two planes)
__global__ void __launch_bounds__(kBlock) mfm_tail4_kernel(TailArgs p, int64_t total4) {
    const int64_t plane4 = static_cast<int64_t>(p.H) * p.W / 4, half4 = plane4 * p.C;
    const bool hb_ = p.bias != nullptr, hr_ = p.res != nullptr;
    const float4* h4 = reinterpret_cast<const float4*>(p.h);
    const float4* r4 = reinterpret_cast<const float4*>(p.res);
    float4* y4 = reinterpret_cast<float4*>(p.y);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total4; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t b = i / half4, r = i - b * half4;
        const int c = static_cast<int>(r / plane4);
        const float ba = hb_ ? p.bias[c] : 0.f, bb = hb_ ? p.bias[p.C + c] : 0.f;
        const float4 a = h4[b * 2 * half4 + r], s = h4[b * 2 * half4 + half4 + r];
        const float4 rr = hr_ ? r4[i] : float4{0.f, 0.f, 0.f, 0.f};
        y4[i] = tail_elem4(a, s, ba, bb, hb_, hr_, rr);
    }
}

// W % 4 == 0, pool: an item is four input columns of an output row (two outputs); 16-byte loads of up to two input rows of both
// halves and of the residual, one 8-byte store.  Wo = W / 2: a window never hangs over the right edge; the last row's may hang below.
__global__ void __launch_bounds__(kBlock) mfm_tail4_pool_kernel(TailArgs p, int64_t items) {
    const int W4 = p.W / 4;
    const int64_t plane4 = static_cast<int64_t>(p.H) * W4;
    const bool hb_ = p.bias != nullptr, hr_ = p.res != nullptr;
    const float4* h4 = reinterpret_cast<const float4*>(p.h);
    const float4* r4 = reinterpret_cast<const float4*>(p.res);
    float2* y2 = reinterpret_cast<float2*>(p.y);
    const float4 zero = float4{0.f, 0.f, 0.f, 0.f};
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < items; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int xq = static_cast<int>(i % W4);
        int64_t t = i / W4;
        const int oy = static_cast<int>(t % p.Ho);
        t /= p.Ho;
        const int c = static_cast<int>(t % p.C);
        const int64_t b = t / p.C;
        const float ba = hb_ ? p.bias[c] : 0.f, bb = hb_ ? p.bias[p.C + c] : 0.f;
        const int64_t pa = (b * 2 * p.C + c) * plane4, pb = pa + static_cast<int64_t>(p.C) * plane4, pr = (b * p.C + c) * plane4;
        const int64_t o0 = static_cast<int64_t>(2 * oy) * W4 + xq;
        const float4 v0 = tail_elem4(h4[pa + o0], h4[pb + o0], ba, bb, hb_, hr_, hr_ ? r4[pr + o0] : zero);
        float lo = pool_step(v0.x, v0.y), hi = pool_step(v0.z, v0.w);
        if (2 * oy + 1 < p.H) {
            const int64_t o1 = o0 + W4;
            const float4 v1 = tail_elem4(h4[pa + o1], h4[pb + o1], ba, bb, hb_, hr_, hr_ ? r4[pr + o1] : zero);
            lo = pool_step(pool_step(lo, v1.x), v1.y);
            hi = pool_step(pool_step(hi, v1.z), v1.w);
        }
        y2[i] = float2{lo, hi};          // output (b, c, oy, 2 xq .. 2 xq + 1) is float2 number i: Wo / 2 == W4
    }
}

// ------------------------------------------------------------------------------------------------ identity input
__global__ void __launch_bounds__(kBlock) gray_kernel(const float* __restrict__ img, float* __restrict__ out, int64_t total, int Cin, int64_t HW) {
    const float n = static_cast<float>(Cin);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t b = i / HW, o = i - b * HW;
        const float* p = img + b * Cin * HW + o;
        float s = p[0];
        for (int c = 1; c < Cin; ++c) s += p[c * HW];
        out[i] = s / n;
    }
}

__global__ void __launch_bounds__(kBlock) gray4_kernel(const float4* __restrict__ img, float4* __restrict__ out, int64_t total4, int Cin, int64_t HW4) {
    const float n = static_cast<float>(Cin);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total4; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t b = i / HW4, o = i - b * HW4;
        const float4* p = img + b * Cin * HW4 + o;
        float4 s = p[0];
        for (int c = 1; c < Cin; ++c) {
            const float4 v = p[c * HW4];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        out[i] = float4{s.x / n, s.y / n, s.z / n, s.w / n};
    }
}

constexpr int kFace = 128;          // the crop's image and output size
constexpr int kCropPlane = 98;      // build_grid(b, 98)

// Source coordinate of plane sample i along an axis: the grid's linspace(-49, 49, 98)[i] + (centre - 64), over 64, un-normalised by
// grid_sample (align_corners=False): 64 g + 63.5.  Formed in double and rounded once.
__device__ __forceinline__ float crop_coord(int i, double origin) { return static_cast<float>(origin + 98.0 * i / 97.0); }

__device__ __forceinline__ float gray_at(const float* __restrict__ p, int Cin, float n) {
    float s = p[0];
    for (int c = 1; c < Cin; ++c) s += p[c * (kFace * kFace)];
    return s / n;
}

// One thread per output pixel: the bilinear resize (half-pixel centres, scale 98 / 128 -- exact in fp32, as are its coordinates) of
// four plane samples, each a bilinear grid_sample of the channel mean.  Rows 27 .. 126 and columns 14 .. 113: no tap leaves the image.
__global__ void __launch_bounds__(kBlock) crop_kernel(const float* __restrict__ img, float* __restrict__ out, int Cin) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int64_t b = blockIdx.z;
    const float* src = img + b * Cin * (kFace * kFace);
    const float n = static_cast<float>(Cin);
    const float scale = static_cast<float>(kCropPlane) / kFace;
    float ry = scale * (oy + 0.5f) - 0.5f, rx = scale * (ox + 0.5f) - 0.5f;
    ry = ry < 0.f ? 0.f : ry;
    rx = rx < 0.f ? 0.f : rx;
    const int r0 = static_cast<int>(ry), c0 = static_cast<int>(rx);
    const int r1 = r0 + (r0 < kCropPlane - 1 ? 1 : 0), c1 = c0 + (c0 < kCropPlane - 1 ? 1 : 0);
    const float ly1 = ry - r0, ly0 = 1.f - ly1, lx1 = rx - c0, lx0 = 1.f - lx1;
    float row[2];
    const int rs[2] = {r0, r1}, cs[2] = {c0, c1};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float y = crop_coord(rs[a], 27.5);
        const float yf = floorf(y);
        const int y0 = static_cast<int>(yf);
        const float wy1 = y - yf, wy0 = (yf + 1.f) - y;
        float s[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float x = crop_coord(cs[e], 14.5);
            const float xf = floorf(x);
            const int x0 = static_cast<int>(xf);
            const float wx1 = x - xf, wx0 = (xf + 1.f) - x;
            const float* q = src + y0 * kFace + x0;
            const float nw = gray_at(q, Cin, n), ne = gray_at(q + 1, Cin, n), sw = gray_at(q + kFace, Cin, n), se = gray_at(q + kFace + 1, Cin, n);
            s[e] = nw * (wx0 * wy0) + ne * (wx1 * wy0) + sw * (wx0 * wy1) + se * (wx1 * wy1);
        }
        row[a] = lx0 * s[0] + lx1 * s[1];
    }
    out[(b * kFace + oy) * kFace + ox] = ly0 * row[0] + ly1 * row[1];
}

// ---- the input stage's gradient
// crop 0: grad_img[b, c] = grad_out[b, 0] / Cin for every channel (the division the forward makes, one rounding).
__global__ void __launch_bounds__(kBlock) gray_bwd_kernel(const float* __restrict__ go, float* __restrict__ gi, int64_t total, int Cin, int64_t HW) {
    const float n = static_cast<float>(Cin);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t b = i / HW, o = i - b * HW;
        const float v = go[i] / n;
        float* p = gi + b * Cin * HW + o;
        for (int c = 0; c < Cin; ++c) p[c * HW] = v;
    }
}

__global__ void __launch_bounds__(kBlock) gray4_bwd_kernel(const float4* __restrict__ go, float4* __restrict__ gi, int64_t total4, int Cin, int64_t HW4) {
    const float n = static_cast<float>(Cin);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total4; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t b = i / HW4, o = i - b * HW4;
        const float4 g = go[i];
        const float4 v = float4{g.x / n, g.y / n, g.z / n, g.w / n};
        float4* p = gi + b * Cin * HW4 + o;
        for (int c = 0; c < Cin; ++c) p[c * HW4] = v;
    }
}

// The crop is separable: out = A_y gray A_x^T with, per axis, A = R S (S: the two-tap sample of plane index r at crop_coord(r), R: the
// two-tap resize of output index o).  Its adjoint is a gather: input index i along an axis is touched by at most 5 output indices, all
// within kCropCand consecutive ones from crop_first_candidate(i) on (the lowest touching index lies 1 .. 6 past it: one spare on either side).
constexpr int kCropCand = 8;
constexpr int kCropBand = 8;        // input rows per block of crop_bwd_kernel

// twice_origin = 2 origin (55 rows, 29 columns): floor((i - origin) 128 97 / 98^2) - 3, the factor rounded to 331 / 256; all-integer
__device__ __forceinline__ int crop_first_candidate(int i, int twice_origin) { return (((2 * i - twice_origin + 512) * 331) >> 9) - 331 - 3; }

// A[o, i]: the weight of input index i in output index o along an axis, from the forward's own coordinates and weights (resize
// coordinate clamped at 0, upper tap clamped at 97; crop_coord in double, rounded once).  0 when no tap of o is i -- the exact tap test.
__device__ __forceinline__ float crop_axis_weight(int o, int i, double origin) {
    if (o < 0 || o >= kFace) return 0.f;
    const float scale = static_cast<float>(kCropPlane) / kFace;
    float r = scale * (o + 0.5f) - 0.5f;
    r = r < 0.f ? 0.f : r;
    const int r0 = static_cast<int>(r);
    const int r1 = r0 + (r0 < kCropPlane - 1 ? 1 : 0);
    const float l1 = r - r0, l0 = 1.f - l1;
    const int rs[2] = {r0, r1};
    const float ls[2] = {l0, l1};
    float w = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float y = crop_coord(rs[a], origin);
        const float yf = floorf(y);
        const int y0 = static_cast<int>(yf);
        const float w1 = y - yf, w0 = (yf + 1.f) - y;
        if (y0 == i) w += ls[a] * w0;
        if (y0 + 1 == i) w += ls[a] * w1;
    }
    return w;
}

// grad_gray = A_y^T g A_x for a band of kCropBand input rows of one image, then / Cin into every channel.  Pass 1: t[Y][ox] = sum over
// the candidate output rows oy (ascending) of A_y[oy, Y] g[oy][ox], kept in LDS; pass 2: sum over the candidate output columns ox
// (ascending) of A_x[ox, X] t[Y][ox].  A fixed order and no atomics: bit-identical from run to run.  A cell no tap touches (rows
// 0 .. 26 and 127, columns 0 .. 13 and 114 .. 127) adds nothing to 0.f and is stored as that.
__global__ void __launch_bounds__(kBlock) crop_bwd_kernel(const float* __restrict__ go, float* __restrict__ gi, int Cin) {
    __shared__ float wy[kCropBand][kCropCand];
    __shared__ float wx[kCropCand][kFace];
    __shared__ float t[kCropBand][kFace];
    const int tid = threadIdx.x;
    const int band = blockIdx.x * kCropBand;
    const int64_t b = blockIdx.y;
    const float* g = go + b * (kFace * kFace);
    if (tid < kCropBand * kCropCand) {
        const int yl = tid / kCropCand, k = tid % kCropCand;
        wy[yl][k] = crop_axis_weight(crop_first_candidate(band + yl, 55) + k, band + yl, 27.5);
    }
    for (int i = tid; i < kCropCand * kFace; i += kBlock) {
        const int k = i / kFace, X = i % kFace;
        wx[k][X] = crop_axis_weight(crop_first_candidate(X, 29) + k, X, 14.5);
    }
    __syncthreads();
    const int x = tid & (kFace - 1);
    for (int yl = tid / kFace; yl < kCropBand; yl += kBlock / kFace) {
        const int o0 = crop_first_candidate(band + yl, 55);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kCropCand; ++k) {
            const float w = wy[yl][k];          // != 0 only for 0 <= o0 + k < 128
            if (w != 0.f) s += w * g[(o0 + k) * kFace + x];
        }
        t[yl][x] = s;
    }
    __syncthreads();
    const float n = static_cast<float>(Cin);
    const int o0 = crop_first_candidate(x, 29);
    for (int yl = tid / kFace; yl < kCropBand; yl += kBlock / kFace) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kCropCand; ++k) {
            const float w = wx[k][x];
            if (w != 0.f) s += w * t[yl][o0 + k];
        }
        const float v = s / n;
        float* p = gi + (b * Cin * kFace + band + yl) * kFace + x;
        for (int c = 0; c < Cin; ++c) p[c * (kFace * kFace)] = v;
    }
}

// ------------------------------------------------------------------------------------------------ cosine similarity + top-k
constexpr int kProbes = 8;          // probes per block of the similarity pass
constexpr int kSegment = 2048;       // gallery rows per selection block
constexpr int kMaxSegments = 256;
constexpr float kCosEps = 1e-8f;

// sim[b, g] = <p_b, g> / (max(|p_b|, eps) max(|g|, eps)).  Block = (chunk of gallery rows, tile of kProbes probes); the probes sit in
// LDS, a wave owns a gallery row at a time: its lanes stride the row (16 bytes each on the vector route) and keep one partial dot
// product per probe and the row's squared norm, folded by a butterfly (every lane ends with the same sums, in a fixed order).
template <bool VEC>
__global__ void __launch_bounds__(kBlock) cos_sim_kernel(const float* __restrict__ probe, const float* __restrict__ gallery,
                                                         float* __restrict__ sim, int B, int64_t G, int D, int rows_per_block) {
    extern __shared__ float4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    const int Dp = (D + 3) & ~3;
    float* pn = lds + kProbes * Dp;
    const int p0 = blockIdx.y * kProbes;
    const int np = B - p0 < kProbes ? B - p0 : kProbes;
    for (int i = threadIdx.x; i < kProbes * Dp; i += kBlock) {
        const int p = i / Dp, d = i - p * Dp;
        lds[i] = (p < np && d < D) ? probe[static_cast<int64_t>(p0 + p) * D + d] : 0.f;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int p = wave; p < kProbes; p += kBlock / kWave) {
        float s = 0.f;
        for (int d = lane; d < Dp; d += kWave) s += lds[p * Dp + d] * lds[p * Dp + d];
        s = wave_sum(s);
        if (lane == 0) pn[p] = fmaxf(sqrtf(s), kCosEps);
    }
    __syncthreads();
    const int64_t g_begin = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    const int64_t g_end = g_begin + rows_per_block < G ? g_begin + rows_per_block : G;
    for (int64_t g = g_begin + wave; g < g_end; g += kBlock / kWave) {
        float acc[kProbes], gg = 0.f;
#pragma unroll
        for (int p = 0; p < kProbes; ++p) acc[p] = 0.f;
        const float* row = gallery + g * D;
        if (VEC) {
            const float4* row4 = reinterpret_cast<const float4*>(row);
            for (int d4 = lane; d4 < D / 4; d4 += kWave) {
                const float4 v = row4[d4];
                gg += v.x * v.x; gg += v.y * v.y; gg += v.z * v.z; gg += v.w * v.w;
#pragma unroll
                for (int p = 0; p < kProbes; ++p) {
                    const float4 q = lds4[p * (Dp / 4) + d4];
                    acc[p] += v.x * q.x; acc[p] += v.y * q.y; acc[p] += v.z * q.z; acc[p] += v.w * q.w;
                }
            }
        } else {
            for (int d = lane; d < D; d += kWave) {
                const float v = row[d];
                gg += v * v;
#pragma unroll
                for (int p = 0; p < kProbes; ++p) acc[p] += v * lds[p * Dp + d];
            }
        }
        gg = wave_sum(gg);
        float mine = 0.f;
#pragma unroll
        for (int p = 0; p < kProbes; ++p) {
            const float s = wave_sum(acc[p]);
            mine = lane == p ? s : mine;
        }
        if (lane < np) sim[static_cast<int64_t>(p0 + lane) * G + g] = mine / (pn[lane] * fmaxf(sqrtf(gg), kCosEps));
    }
}

// (value, index) as one 64-bit key whose unsigned order is topk's: NaN above everything, then the larger value, then the LOWER index.
// -0 and +0 are one value.  No key is 0 (a NaN never reaches the sign-flip branch), so 0 stands for "nothing".
__device__ __forceinline__ unsigned long long sim_key(float v, unsigned idx) {
    unsigned o = 0xFFFFFFFFu;
    if (v == v) {
        const unsigned bits = __float_as_uint(v == 0.f ? 0.f : v);
        o = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    }
    return (static_cast<unsigned long long>(o) << 32) | static_cast<unsigned>(~idx);
}
__device__ __forceinline__ float key_value(unsigned long long key) {
    const unsigned o = static_cast<unsigned>(key >> 32);
    if (o == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// The k largest keys of a range, largest first: round r finds the largest key below round r - 1's (keys are distinct: they hold
// their index), by a wave butterfly and four LDS cells.  The range is re-read every round (<= 8 KiB of similarities per block in the
// common case: cache-resident); nothing is marked, nothing is atomically updated.
// FROM_KEYS: the range holds candidate keys of the segments (0 = an empty slot) instead of similarities.
// FINAL: write values / indices of the probe; else the segment's k candidate keys.
template <bool FROM_KEYS, bool FINAL>
__global__ void __launch_bounds__(kBlock) topk_kernel(const float* __restrict__ sim, const unsigned long long* __restrict__ keys_in,
                                                      unsigned long long* __restrict__ keys_out, float* __restrict__ values,
                                                      int* __restrict__ indices, int64_t n, int64_t seg_len, int k) {
    __shared__ unsigned long long cell[2][kBlock / kWave];
    const int64_t b = blockIdx.y, s = blockIdx.x;
    const int64_t begin = s * seg_len, end = begin + seg_len < n ? begin + seg_len : n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long prev = 0;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = 0;
        for (int64_t i = begin + threadIdx.x; i < end; i += kBlock) {
            const unsigned long long key = FROM_KEYS ? keys_in[b * n + i] : sim_key(sim[b * n + i], static_cast<unsigned>(i));
            if ((r == 0 || key < prev) && key > best) best = key;
        }
        best = wave_max(best);
        if (lane == 0) cell[r & 1][wave] = best;
        __syncthreads();          // (two cell rows: round r + 1 may write while a slow wave still reads round r)
        best = cell[r & 1][0];
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) best = cell[r & 1][w] > best ? cell[r & 1][w] : best;
        prev = best;
        if (threadIdx.x == 0) {
            if (FINAL) {
                values[b * k + r] = key_value(best);
                indices[b * k + r] = static_cast<int>(~static_cast<unsigned>(best));
            } else {
                keys_out[(b * gridDim.x + s) * k + r] = best;
            }
        }
        if (best == 0) {          // fewer than k keys in this range (a short segment): the remaining slots are empty
            for (int q = r + 1 + threadIdx.x; q < k; q += kBlock)
                if (!FINAL) keys_out[(b * gridDim.x + s) * k + q] = 0;
            break;
        }
    }
}

int64_t align16(int64_t n) { return (n + 15) / 16 * 16; }
int64_t topk_segments(int64_t G) {
    const int64_t s = (G + kSegment - 1) / kSegment;
    return s < 1 ? 1 : (s > kMaxSegments ? kMaxSegments : s);
}
bool topk_dims_ok(int64_t B, int64_t G, int64_t D, int64_t k) {
    return B > 0 && G > 0 && D > 0 && D <= 1024 && k >= 1 && k <= 32 && k <= G && G < (1LL << 31) && B <= 65535 &&
           B * G < (1LL << 40);
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_mfm_tail_forward(const void* h, const void* bias, const void* residual, void* y, int64_t B, int64_t C, int64_t H,
                                     int64_t W, int pool, int dtype, void* stream) {
    const char* fn = "ffwm_mfm_tail_forward";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(h && y, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(pool == 0 || pool == 1, FFWM_ERR_ARG, "%s: pool must be 0 or 1", fn);
    FFWM_REQUIRE(H < (1 << 20) && W < (1 << 20) && C < (1 << 20) && B < (1LL << 40) / (C * H * W), FFWM_ERR_SIZE, "%s: tensor too large", fn);          // (each factor bounded before the product is formed)
    hipStream_t st = static_cast<hipStream_t>(stream);
    TailArgs p;
    p.h = static_cast<const float*>(h);
    p.bias = static_cast<const float*>(bias);
    p.res = static_cast<const float*>(residual);
    p.y = static_cast<float*>(y);
    p.C = static_cast<int>(C);
    p.H = static_cast<int>(H);
    p.W = static_cast<int>(W);
    p.Ho = static_cast<int>(pool ? (H + 1) / 2 : H);
    p.Wo = static_cast<int>(pool ? (W + 1) / 2 : W);
    const int64_t total = B * C * p.Ho * p.Wo;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual)) % 16 == 0;
    LaunchScope ls(pool ? "mfm_tail_pool" : "mfm_tail", st, 4.0 * ((2.0 + (residual ? 1.0 : 0.0)) * B * C * H * W + total));
    if (vec && pool)
        hipLaunchKernelGGL(mfm_tail4_pool_kernel, dim3(ew_grid(total / 2)), dim3(kBlock), 0, st, p, total / 2);
    else if (vec)
        hipLaunchKernelGGL(mfm_tail4_kernel, dim3(ew_grid(total / 4)), dim3(kBlock), 0, st, p, total / 4);
    else if (pool)
        hipLaunchKernelGGL(mfm_tail_kernel<true>, dim3(ew_grid(total)), dim3(kBlock), 0, st, p, total);
    else
        hipLaunchKernelGGL(mfm_tail_kernel<false>, dim3(ew_grid(total)), dim3(kBlock), 0, st, p, total);
    return check_launch(fn);
}

extern "C" int ffwm_identity_input(const void* img, void* out, int64_t B, int64_t Cin, int64_t H, int64_t W, int crop, int dtype,
                                   void* stream) {
    const char* fn = "ffwm_identity_input";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(img && out, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && Cin >= 1 && H > 0 && W > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(crop == 0 || crop == 1, FFWM_ERR_ARG, "%s: crop must be 0 or 1", fn);
    FFWM_REQUIRE(!crop || (H == kFace && W == kFace), FFWM_ERR_ARG, "%s: the centre-face crop is defined for 128 x 128 images only", fn);
    FFWM_REQUIRE(Cin < (1 << 20) && H < (1 << 20) && W < (1 << 20) && B < (1LL << 40) / (Cin * H * W) && (!crop || B <= 65535), FFWM_ERR_SIZE,
                 "%s: tensor too large", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = H * W, total = B * HW;
    LaunchScope ls(crop ? "identity_crop" : "identity_gray", st, 4.0 * (Cin + 1.0) * total);
    if (crop) {
        hipLaunchKernelGGL(crop_kernel, dim3(kFace / 64, kFace / 4, static_cast<unsigned>(B)), dim3(kBlock), 0, st,
                           static_cast<const float*>(img), static_cast<float*>(out), static_cast<int>(Cin));
    } else if (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(out)) % 16 == 0) {
        hipLaunchKernelGGL(gray4_kernel, dim3(ew_grid(total / 4)), dim3(kBlock), 0, st, static_cast<const float4*>(img),
                           static_cast<float4*>(out), total / 4, static_cast<int>(Cin), HW / 4);
    } else {
        hipLaunchKernelGGL(gray_kernel, dim3(ew_grid(total)), dim3(kBlock), 0, st, static_cast<const float*>(img), static_cast<float*>(out),
                           total, static_cast<int>(Cin), HW);
    }
    return check_launch(fn);
}

extern "C" int ffwm_identity_input_backward(const void* grad_out, void* grad_img, int64_t B, int64_t Cin, int64_t H, int64_t W, int crop,
                                            int dtype, void* stream) {
    const char* fn = "ffwm_identity_input_backward";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(grad_out && grad_img, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && Cin >= 1 && H > 0 && W > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(crop == 0 || crop == 1, FFWM_ERR_ARG, "%s: crop must be 0 or 1", fn);
    FFWM_REQUIRE(!crop || (H == kFace && W == kFace), FFWM_ERR_ARG, "%s: the centre-face crop is defined for 128 x 128 images only", fn);
    FFWM_REQUIRE(Cin < (1 << 20) && H < (1 << 20) && W < (1 << 20) && B < (1LL << 40) / (Cin * H * W) && (!crop || B <= 65535), FFWM_ERR_SIZE,
                 "%s: tensor too large", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = H * W, total = B * HW;
    LaunchScope ls(crop ? "identity_crop_bwd" : "identity_gray_bwd", st, 4.0 * (Cin + 1.0) * total);
    if (crop) {
        hipLaunchKernelGGL(crop_bwd_kernel, dim3(kFace / kCropBand, static_cast<unsigned>(B)), dim3(kBlock), 0, st,
                           static_cast<const float*>(grad_out), static_cast<float*>(grad_img), static_cast<int>(Cin));
    } else if (HW % 4 == 0 && (reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(grad_img)) % 16 == 0) {
        hipLaunchKernelGGL(gray4_bwd_kernel, dim3(ew_grid(total / 4)), dim3(kBlock), 0, st, static_cast<const float4*>(grad_out),
                           static_cast<float4*>(grad_img), total / 4, static_cast<int>(Cin), HW / 4);
    } else {
        hipLaunchKernelGGL(gray_bwd_kernel, dim3(ew_grid(total)), dim3(kBlock), 0, st, static_cast<const float*>(grad_out),
                           static_cast<float*>(grad_img), total, static_cast<int>(Cin), HW);
    }
    return check_launch(fn);
}

extern "C" int64_t ffwm_cosine_topk_workspace_bytes(int64_t B, int64_t G, int64_t D, int64_t k) {
    if (!topk_dims_ok(B, G, D, k)) return 0;
    const int64_t segs = topk_segments(G);
    return align16(B * G * 4) + (segs > 1 ? B * segs * k * 8 : 0);
}

extern "C" int ffwm_cosine_topk(const void* probe, const void* gallery, void* values, void* indices, int64_t B, int64_t G, int64_t D,
                                int64_t k, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    const char* fn = "ffwm_cosine_topk";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(probe && gallery && values && indices && workspace, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && G > 0 && D > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(D <= 1024, FFWM_ERR_ARG, "%s: D must be at most 1024", fn);
    FFWM_REQUIRE(k >= 1 && k <= 32 && k <= G, FFWM_ERR_ARG, "%s: k must be in 1 .. min(G, 32)", fn);
    FFWM_REQUIRE(topk_dims_ok(B, G, D, k), FFWM_ERR_SIZE, "%s: problem too large", fn);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, FFWM_ERR_ARG, "%s: the workspace must be 16-byte aligned", fn);
    FFWM_REQUIRE(workspace_bytes >= ffwm_cosine_topk_workspace_bytes(B, G, D, k), FFWM_ERR_ARG, "%s: workspace too small", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* sim = static_cast<float*>(workspace);
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + align16(B * G * 4));
    const int Dp = static_cast<int>((D + 3) / 4 * 4);
    const size_t lds = (static_cast<size_t>(kProbes) * Dp + kProbes) * sizeof(float);
    const int rows = G <= 2048 ? kBlock / kWave : 64;          // a small gallery: one row per wave, a block for every four rows
    const dim3 sim_grid(static_cast<unsigned>((G + rows - 1) / rows), static_cast<unsigned>((B + kProbes - 1) / kProbes));
    {
        LaunchScope ls("cosine_sim", st, 4.0 * (static_cast<double>(G) * D * sim_grid.y + static_cast<double>(B) * G));
        if (D % 4 == 0 && reinterpret_cast<uintptr_t>(gallery) % 16 == 0)
            hipLaunchKernelGGL(cos_sim_kernel<true>, sim_grid, dim3(kBlock), lds, st, static_cast<const float*>(probe),
                               static_cast<const float*>(gallery), sim, static_cast<int>(B), G, static_cast<int>(D), rows);
        else
            hipLaunchKernelGGL(cos_sim_kernel<false>, sim_grid, dim3(kBlock), lds, st, static_cast<const float*>(probe),
                               static_cast<const float*>(gallery), sim, static_cast<int>(B), G, static_cast<int>(D), rows);
        if (int rc = check_launch(fn)) return rc;
    }
    const int64_t segs = topk_segments(G), seg_len = (G + segs - 1) / segs;
    const int kk = static_cast<int>(k);
    float* val = static_cast<float*>(values);
    int* idx = static_cast<int*>(indices);
    if (segs == 1) {
        LaunchScope ls("cosine_topk", st, 4.0 * B * G);
        hipLaunchKernelGGL((topk_kernel<false, true>), dim3(1, static_cast<unsigned>(B)), dim3(kBlock), 0, st, sim, nullptr, nullptr, val, idx, G,
                           seg_len, kk);
        return check_launch(fn);
    }
    {
        LaunchScope ls("cosine_topk", st, 4.0 * B * G);
        hipLaunchKernelGGL((topk_kernel<false, false>), dim3(static_cast<unsigned>(segs), static_cast<unsigned>(B)), dim3(kBlock), 0, st, sim,
                           nullptr, cand, nullptr, nullptr, G, seg_len, kk);
        if (int rc = check_launch(fn)) return rc;
    }
    LaunchScope ls("cosine_topk_merge", st, 8.0 * B * segs * k);
    hipLaunchKernelGGL((topk_kernel<true, true>), dim3(1, static_cast<unsigned>(B)), dim3(kBlock), 0, st, nullptr, cand, nullptr, val, idx, segs * k,
                       segs * k, kk);
    return check_launch(fn);
}
