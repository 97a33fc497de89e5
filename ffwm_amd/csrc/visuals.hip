// visuals.hip -- the reference's result images as ready-to-encode uint8 RGB sheets, every visual of a call in ONE pass (gfx950).
//
// Reference: util/util.py:10-70 (tensor2im / tensor2flow / tensor2mask / tensor2att) and util/flow_util.py:23-153 (flow2img,
// compute_color, make_color_wheel), as util/visualizer.py:102-165 calls them per label and per image: a `.cpu().float().numpy()` of
// the float tensor (four times the bytes of the picture it becomes, and a synchronisation), then numpy passes on the host --
// arctan2, three colour-wheel passes and a dozen full-plane temporaries for a flow.
//
// Here an "item" is one visual: float32 [B, C, H, W] in, uint8 [B, H, W, 3] out.  All items of a call travel in the kernel
// arguments (as the multi-problem warp and L1 launches do); a workgroup finds its item from its index.  A thread owns kVisPix = 4
// consecutive pixels of the item's flat [B*H*W] pixel index: one float4 per plane in, 12 contiguous bytes (three dwords) out.  Every
// output byte is written exactly once, by a plain store, so the launch can sit inside a captured hipGraph.
//
// The arithmetic is the reference's, rounding by rounding (-ffp-contract=off):
//   u8(t)    one rule for every float -> byte conversion: truncate toward zero to int32 and keep the low 8 bits; NaN, +-inf and
//            |t| >= 2^31 give 0.  On [0, 256) that is numpy's astype(uint8); outside it numpy's cast is undefined, this is not.
//   IMAGE    C == 3: u8(x * 255);  C == 1: u8(((x - 0.5) * 2) * 255) on all three channels (tensor2im does map a 1-channel image
//            to [-255, 255])
//   MASK     u8(x * 255), one channel tiled to three
//   PALETTE  palette[u8(x[:, 0] * 255)]: a uint8 [256, 3] RGB table of the caller's (the library ships no colour map)
//   FLOW     g = clamp((f + 1) * (H / 2), 0, H - 1) in float32 -- BOTH axes scale with H, NaN passes the clamp --, motion u = g[0] - x,
//            v = g[1] - y, rad = sqrtf(u u + v v); per IMAGE m = max(rad), NaN if any cell is; maxrad = m > -1 ? m : -1 (Python's
//            max(-1, nan)); u' = (double)(u / maxrad) + DBL_EPSILON: the division is float32, everything after it float64 (NumPy 2
//            promotes the float32 array against finfo(float).eps).  Middlebury wheel of 55 colours indexed by atan2(-v', -u'),
//            saturation by rad'.  A cell whose u' or v' is NaN is black; so is a field without motion (0 / 0).
// The per-image maximum is one workgroup of kFlowBlock threads per image (flow_maxrad_kernel: no float atomics, a fixed reduction
// order) into the caller's workspace, one float per flow image; the colouring pass reads it.  A call without a flow item is one
// launch, a call with one is two.
#include <float.h>

#include "common.hpp"

namespace ffwm {
namespace {

constexpr int kVisMax = 16;                          // items per call
constexpr int kVisPix = 4;                           // pixels per thread
constexpr int kVisPerBlock = kBlock * kVisPix;       // pixels per workgroup of the colouring pass
constexpr int kFlowBlock = 1024;                     // threads of the workgroup that reduces one flow image's maximum
constexpr int kWheelCols = 55;

enum { kImage = 0, kMask = 1, kFlow = 2, kPalette = 3 };

struct VisItem {
    const float* src;
    const unsigned char* pal;
    unsigned char* out;
    unsigned n, hw, W;        // pixels of the item (B*H*W), of a plane, of a row
    int kind, C, planes;      // planes: how many of an image's C planes the kind reads
    int vec;                  // float4 loads: H*W % 4 == 0 and src 16-byte aligned
    float half_h, hi;         // FLOW: H / 2 and H - 1
    unsigned begin;           // first workgroup of the item in the colouring pass
    unsigned fbegin;          // FLOW: first slot of the item in the workspace (= first workgroup in flow_maxrad_kernel)
};
struct VisTable {
    int n;
    VisItem it[kVisMax];
};
static_assert(sizeof(VisTable) <= 4096, "the table travels as a kernel argument");

// The 55-entry Middlebury wheel (flow_util.py:106-153): segments RY 15 / YG 6 / GC 4 / CB 11 / BM 13 / MR 6 with floor-ed ramps,
// stored as value / 255 in double (compute_color divides by 255 in float64 before it mixes; the quotient is folded at compile time).
struct Wheel {
    double c[kWheelCols][3];
};
constexpr Wheel make_wheel() {
    Wheel w{};
    const int seg[6] = {15, 6, 4, 11, 13, 6};
    //               fixed-255 channel, ramp channel, ramp falls (255 - ramp)?
    const int full[6] = {0, 1, 1, 2, 2, 0};
    const int ramp[6] = {1, 0, 2, 1, 0, 2};
    const bool falls[6] = {false, true, false, true, false, true};
    int col = 0;
    for (int s = 0; s < 6; ++s) {
        for (int i = 0; i < seg[s]; ++i) {
            const int r = 255 * i / seg[s];          // floor(255 * i / n) of non-negative integers
            for (int ch = 0; ch < 3; ++ch) w.c[col + i][ch] = 0.0;
            w.c[col + i][full[s]] = 255.0 / 255.0;
            w.c[col + i][ramp[s]] = static_cast<double>(falls[s] ? 255 - r : r) / 255.0;
        }
        col += seg[s];
    }
    return w;
}
__constant__ Wheel kWheel = make_wheel();

__device__ __forceinline__ unsigned u8(float t) {
    if (!(fabsf(t) < 2147483648.f)) return 0u;       // NaN, +-inf, |t| >= 2^31
    return static_cast<unsigned>(static_cast<int>(t)) & 255u;
}
__device__ __forceinline__ unsigned u8(double t) {
    if (!(fabs(t) < 2147483648.0)) return 0u;
    return static_cast<unsigned>(static_cast<int>(t)) & 255u;
}

// torch.clamp(t, 0, hi): NaN compares false twice and stays
__device__ __forceinline__ float clamp_grid(float t, float hi) { return t < 0.f ? 0.f : (t > hi ? hi : t); }

__device__ __forceinline__ void flow_motion(const VisItem& q, float f0, float f1, unsigned rem, float& u, float& v) {
    const unsigned y = rem / q.W, x = rem - y * q.W;
    const float g0 = clamp_grid((f0 + 1.f) * q.half_h, q.hi), g1 = clamp_grid((f1 + 1.f) * q.half_h, q.hi);
    u = g0 - static_cast<float>(x);
    v = g1 - static_cast<float>(y);
}

// packed r | g << 8 | b << 16 of one flow pixel
__device__ __forceinline__ unsigned flow_colour(float u, float v, float m) {
    const float maxrad = (m > -1.f) ? m : -1.f;
    const double ud = static_cast<double>(u / maxrad) + DBL_EPSILON, vd = static_cast<double>(v / maxrad) + DBL_EPSILON;
    if (ud != ud || vd != vd) return 0u;
    const double rad = sqrt(ud * ud + vd * vd);
    const double a = atan2(-vd, -ud) / 3.141592653589793;
    const double fk = (a + 1.0) / 2.0 * (kWheelCols - 1) + 1.0;
    const double k0f = floor(fk);
    // k0 is 1 .. 55 for every atan2 in [-pi, pi]; k1 = k0 + 1 with 56 -> 1.  As indices modulo 55 (what numpy's wheel[k0 - 1] does with
    // k0 = 0): the same colours, and never an address outside the wheel whatever atan2 returns
    const int k0 = static_cast<int>(k0f);
    const int i0 = ((k0 - 1) % kWheelCols + kWheelCols) % kWheelCols, i1 = (k0 % kWheelCols + kWheelCols) % kWheelCols;
    const double f = fk - k0f;
    unsigned rgb = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double col = (1.0 - f) * kWheel.c[i0][ch] + f * kWheel.c[i1][ch];
        if (rad <= 1.0) col = 1.0 - rad * (1.0 - col);
        else col *= 0.75;
        rgb |= u8(floor(255.0 * col)) << (8 * ch);
    }
    return rgb;
}

__device__ __forceinline__ int find_item(const VisTable& tab) {
    int k = 0;
#pragma unroll 1
    for (int i = 1; i < tab.n; ++i)
        if (blockIdx.x >= tab.it[i].begin) k = i;
    return k;
}

// One workgroup per flow image: maxrad[slot] = max over the plane of rad, NaN if any cell's is.  kFlowBlock threads, four cells each
// per pass (one float4 per plane where the item allows it): a 128 x 128 plane is four passes of independent loads.
__device__ __forceinline__ void flow_rad_max(const VisItem& q, float f0, float f1, unsigned rem, float& mx, int& nan) {
    float u, v;
    flow_motion(q, f0, f1, rem, u, v);
    const float rad = sqrtf(u * u + v * v);
    if (rad != rad) nan = 1;
    else mx = rad > mx ? rad : mx;
}

__global__ void __launch_bounds__(kFlowBlock)
flow_maxrad_kernel(const VisTable tab, float* __restrict__ maxrad) {
    __shared__ float red[kFlowBlock / kWave];
    __shared__ int red_nan[kFlowBlock / kWave];
    int k = 0;
#pragma unroll 1
    for (int i = 0; i < tab.n; ++i)
        if (tab.it[i].kind == kFlow && blockIdx.x >= tab.it[i].fbegin) k = i;
    const VisItem& q = tab.it[k];
    const unsigned b = blockIdx.x - q.fbegin;
    const float* f0 = q.src + static_cast<size_t>(b) * q.C * q.hw;
    const float* f1 = f0 + q.hw;
    float mx = 0.f;             // rad >= 0
    int nan = 0;
    if (q.vec) {                // hw % 4 == 0 and both planes 16-byte aligned
        for (unsigned i = threadIdx.x * kVisPix; i < q.hw; i += kFlowBlock * kVisPix) {
            const float4 a = *reinterpret_cast<const float4*>(f0 + i), c = *reinterpret_cast<const float4*>(f1 + i);
            flow_rad_max(q, a.x, c.x, i, mx, nan);
            flow_rad_max(q, a.y, c.y, i + 1, mx, nan);
            flow_rad_max(q, a.z, c.z, i + 2, mx, nan);
            flow_rad_max(q, a.w, c.w, i + 3, mx, nan);
        }
    } else {
        for (unsigned i = threadIdx.x; i < q.hw; i += kFlowBlock) flow_rad_max(q, f0[i], f1[i], i, mx, nan);
    }
    mx = wave_max(mx);
    nan = __any(nan);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
        red[wave] = mx;
        red_nan[wave] = nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kFlowBlock / kWave; ++w) {
            mx = red[w] > mx ? red[w] : mx;
            nan |= red_nan[w];
        }
        maxrad[blockIdx.x] = nan ? __builtin_nanf("") : mx;
    }
}

__global__ void __launch_bounds__(kBlock)
visuals_kernel(const VisTable tab, const float* __restrict__ maxrad) {
    const VisItem& q = tab.it[find_item(tab)];
    const unsigned p0 = (blockIdx.x - q.begin) * kVisPerBlock + threadIdx.x * kVisPix;
    if (p0 >= q.n) return;
    const bool full = q.n - p0 >= kVisPix;
    const unsigned hw = q.hw;
    unsigned img[kVisPix], rem[kVisPix];
    float a[3][kVisPix];
#pragma unroll
    for (int j = 0; j < kVisPix; ++j) {
        const unsigned p = p0 + j < q.n ? p0 + j : q.n - 1;
        img[j] = p / hw;
        rem[j] = p - img[j] * hw;
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c][j] = 0.f;
    }
    if (full && q.vec) {              // the four pixels lie in one image (hw % 4 == 0) and every plane's four floats are 16-byte aligned
        const float* base = q.src + static_cast<size_t>(img[0]) * q.C * hw + rem[0];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < q.planes) {
                const float4 t = *reinterpret_cast<const float4*>(base + static_cast<size_t>(c) * hw);
                a[c][0] = t.x; a[c][1] = t.y; a[c][2] = t.z; a[c][3] = t.w;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kVisPix; ++j) {
            if (p0 + j < q.n) {
                const float* base = q.src + static_cast<size_t>(img[j]) * q.C * hw + rem[j];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c < q.planes) a[c][j] = base[static_cast<size_t>(c) * hw];
            }
        }
    }
    unsigned rgb[kVisPix];        // r | g << 8 | b << 16
#pragma unroll
    for (int j = 0; j < kVisPix; ++j) {
        if (q.kind == kFlow) {
            float u, v;
            flow_motion(q, a[0][j], a[1][j], rem[j], u, v);
            rgb[j] = flow_colour(u, v, maxrad[q.fbegin + img[j]]);
        } else if (q.kind == kPalette) {
            const unsigned char* e = q.pal + 3u * u8(a[0][j] * 255.0f);
            rgb[j] = e[0] | (e[1] << 8) | (e[2] << 16);
        } else if (q.C == 1) {
            const float t = q.kind == kImage ? ((a[0][j] - 0.5f) * 2.0f) * 255.0f : a[0][j] * 255.0f;
            rgb[j] = u8(t) * 0x010101u;
        } else {
            rgb[j] = u8(a[0][j] * 255.0f) | (u8(a[1][j] * 255.0f) << 8) | (u8(a[2][j] * 255.0f) << 16);
        }
    }
    unsigned char* o = q.out + 3 * static_cast<size_t>(p0);           // p0 % 4 == 0 and out is 4-byte aligned: dword stores
    if (full) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        o4[0] = rgb[0] | (rgb[1] << 24);
        o4[1] = (rgb[1] >> 8) | (rgb[2] << 16);
        o4[2] = (rgb[2] >> 16) | (rgb[3] << 8);
    } else {
        for (int j = 0; j < kVisPix; ++j) {
            if (p0 + j < q.n) {
                o[3 * j] = static_cast<unsigned char>(rgb[j]);
                o[3 * j + 1] = static_cast<unsigned char>(rgb[j] >> 8);
                o[3 * j + 2] = static_cast<unsigned char>(rgb[j] >> 16);
            }
        }
    }
}

// The argument checks of both entry points; fills the table when tab != NULL.  -> status, *flow_images = flow items' images.
int plan_visuals(const char* fn, const ffwm_visual_item* items, int n, VisTable* tab, unsigned* blocks, int64_t* flow_images) {
    FFWM_REQUIRE(items, FFWM_ERR_ARG, "%s: NULL item table", fn);
    FFWM_REQUIRE(n >= 1 && n <= kVisMax, FFWM_ERR_ARG, "%s: %d items (1 .. %d are accepted)", fn, n, kVisMax);
    int64_t nblk = 0, nflow = 0;
    for (int i = 0; i < n; ++i) {
        const ffwm_visual_item& it = items[i];
        FFWM_REQUIRE(it.src && it.out, FFWM_ERR_ARG, "%s: item %d: NULL pointer", fn, i);
        FFWM_REQUIRE(it.kind >= kImage && it.kind <= kPalette, FFWM_ERR_ARG, "%s: item %d: kind %d (0 image, 1 mask, 2 flow, 3 palette)", fn,
                     i, it.kind);
        FFWM_REQUIRE(it.B > 0 && it.C > 0 && it.H > 0 && it.W > 0, FFWM_ERR_ARG, "%s: item %d: non-positive size", fn, i);
        const bool c_ok = it.kind == kFlow ? it.C == 2 : (it.kind == kPalette ? true : (it.C == 1 || it.C == 3));
        FFWM_REQUIRE(c_ok, FFWM_ERR_ARG, "%s: item %d: kind %d does not take C = %lld (image, mask: 1 or 3; flow: 2)", fn, i, it.kind,
                     static_cast<long long>(it.C));
        FFWM_REQUIRE(it.kind != kPalette || it.palette, FFWM_ERR_ARG, "%s: item %d: a palette item needs its uint8 [256, 3] palette", fn, i);
        FFWM_REQUIRE((reinterpret_cast<uintptr_t>(it.out) & 3) == 0 && (reinterpret_cast<uintptr_t>(it.src) & 3) == 0, FFWM_ERR_ARG,
                     "%s: item %d: src and out must be 4-byte aligned", fn, i);
        FFWM_REQUIRE(it.H < (1LL << 24) && it.W < (1LL << 24) && it.C < (1LL << 16) && it.H * it.W < (1LL << 31) &&
                     it.B < (1LL << 31) && it.B * it.H * it.W < (1LL << 31), FFWM_ERR_SIZE, "%s: item %d: B*H*W must stay below 2^31", fn, i);
        const int64_t pix = it.B * it.H * it.W;
        if (tab) {
            VisItem& q = tab->it[i];
            q.src = static_cast<const float*>(it.src);
            q.pal = static_cast<const unsigned char*>(it.palette);
            q.out = static_cast<unsigned char*>(it.out);
            q.n = static_cast<unsigned>(pix);
            q.hw = static_cast<unsigned>(it.H * it.W);
            q.W = static_cast<unsigned>(it.W);
            q.kind = it.kind;
            q.C = static_cast<int>(it.C);
            q.planes = it.kind == kFlow ? 2 : (it.kind == kPalette ? 1 : static_cast<int>(it.C));
            q.vec = (q.hw & 3u) == 0 && (reinterpret_cast<uintptr_t>(it.src) & 15) == 0;
            q.half_h = static_cast<float>(static_cast<double>(it.H) / 2.0);
            q.hi = static_cast<float>(it.H - 1);
            q.begin = static_cast<unsigned>(nblk);
            q.fbegin = static_cast<unsigned>(nflow);
        }
        nblk += (pix + kVisPerBlock - 1) / kVisPerBlock;
        if (it.kind == kFlow) nflow += it.B;
    }
    FFWM_REQUIRE(nblk < (1LL << 31) && nflow < (1LL << 31), FFWM_ERR_SIZE, "%s: the call needs 2^31 workgroups or more", fn);
    if (tab) tab->n = n;
    if (blocks) *blocks = static_cast<unsigned>(nblk);
    *flow_images = nflow;
    return FFWM_OK;
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

// One float per image of the flow items (0 without one); a negative ffwm_status for a table ffwm_visuals would refuse.
extern "C" int64_t ffwm_visuals_workspace_bytes(const ffwm_visual_item* items, int n) {
    int64_t nflow = 0;
    if (int rc = plan_visuals("ffwm_visuals_workspace_bytes", items, n, nullptr, nullptr, &nflow)) return rc;
    return 4 * nflow;
}

extern "C" int ffwm_visuals(const ffwm_visual_item* items, int n, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    const char* fn = "ffwm_visuals";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only (bad dtype %d)", fn, dtype);
    VisTable tab;
    unsigned blocks = 0;
    int64_t nflow = 0;
    if (int rc = plan_visuals(fn, items, n, &tab, &blocks, &nflow)) return rc;
    FFWM_REQUIRE(nflow == 0 || (workspace && workspace_bytes >= 4 * nflow && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0), FFWM_ERR_ARG,
                 "%s: the flow items need a 4-byte aligned workspace of %lld bytes (ffwm_visuals_workspace_bytes), got %lld", fn,
                 static_cast<long long>(4 * nflow), static_cast<long long>(workspace ? workspace_bytes : 0));
    hipStream_t st = static_cast<hipStream_t>(stream);
    double in_bytes = 0, flow_bytes = 0;
    for (int i = 0; i < tab.n; ++i) {
        in_bytes += 4.0 * tab.it[i].n * tab.it[i].planes + 3.0 * tab.it[i].n;
        if (tab.it[i].kind == kFlow) flow_bytes += 8.0 * tab.it[i].n;
    }
    if (nflow > 0) {
        LaunchScope ls("visuals_flow_maxrad", st, flow_bytes);
        hipLaunchKernelGGL(flow_maxrad_kernel, dim3(static_cast<unsigned>(nflow)), dim3(kFlowBlock), 0, st, tab, static_cast<float*>(workspace));
        if (int rc = check_launch(fn)) return rc;
    }
    LaunchScope ls("visuals", st, in_bytes);
    hipLaunchKernelGGL(visuals_kernel, dim3(blocks), dim3(kBlock), 0, st, tab, static_cast<const float*>(workspace));
    return check_launch(fn);
}
