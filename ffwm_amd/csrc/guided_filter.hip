// guided_filter.hip -- GuidedFilter(r, eps)(x, y) of FFWM's illumination-adaption path for gfx950.
//
// Reference: /root/reference/models/external_function.py:164-193 (diff_x / diff_y / BoxFilter: box sums
// as cumsum differences, rows first, then columns) and :239-277 (GuidedFilter.forward):
//     N = box(1); mean_x = box(x)/N; mean_y = box(y)/N; cov = box(x*y)/N - mean_x*mean_y;
//     var = box(x*x)/N - mean_x^2; A = cov/(var+eps); b = mean_y - A*mean_x;
//     out = (box(A)/N) * x + box(b)/N
// called by FFWMModel.forward on the generated 128 x 128 image every step and on the 64 / 32 px scales
// after 20000 iterations (models/ffwm_model.py:57-59,81,104-105).  In PyTorch that is ~100 launches
// forward and ~200 backward (cumsum, narrow, cat, sub, div ... per box filter).
//
// Here: four launches forward, four backward, every one over the WHOLE chip.  (Rounds 1-2 kept a plane in the LDS of one
// 1024-thread block: FFWM's call has 24 planes, i.e. 24 of 256 CUs busy for 110 us.)  A box filter is separable and the
// reference evaluates it that way -- cumsum down the columns, window difference, cumsum along the rows, window difference
// -- so the two directions are two kernels:
//   gf_cols_kernel: a block owns a strip of 32 columns of one plane for ONE quantity of the stage (x, y, xy, xx / A, b / ...;
//                   grid = planes x W/32 x quantities = 384 for the first stage of FFWM's call): the pointwise input is formed
//                   on the fly from coalesced 128-byte row segments, transposed through LDS, and a wave scans its eight columns
//                   side by side (two elements per lane, 6 shuffle steps, window difference by two more shuffles per element);
//   gf_rows_kernel: a WAVE owns one row (grid = planes x H / 4 = 768): coalesced row loads, the same register scan, and the
//                   stage's pointwise epilogue (means, cov, var, A, b ... / the quotient-rule terms of the backward) fused
//                   behind it.  No LDS, no barrier.
// The arithmetic (scan shape, order of the operations, N as the closed form of box(1)) is what the one-block kernel did.
// Intermediates live in the `saved` planes / the output (forward) and in grad_x + a two-plane workspace (backward).
// Planes up to 128 x 128 (a line is two elements per lane).  Larger planes, a one-channel guide and the gradient for y: the
// general path further down (gfg_*), behind ffwm_guided_filter_*_general.
#include "common.hpp"

namespace ffwm {
namespace {

constexpr int kGfMaxDim = 128;
constexpr int kGfStrip = 32;          // columns per block of the column pass: a row segment is one 128-byte line

template <typename T>
struct GfArgs {
    const T* x;
    const T* y;
    const T* g;        // grad_output (backward)
    T* saved;          // [5, planes, H, W]  (read-only in the backward)
    T* out;            // output (forward) / grad_x (backward)
    T* ws;             // [2, planes, H, W] workspace (backward)
    int64_t planes;
    int H, W, r;
    T eps;
};

// N = box(1): the window clipped to the image
template <typename T>
__device__ __forceinline__ T box_count(int i, int j, int H, int W, int r) {
    const int h = (i + r < H - 1 ? i + r : H - 1) - (i - r > 0 ? i - r : 0) + 1;
    const int w = (j + r < W - 1 ? j + r : W - 1) - (j - r > 0 ? j - r : 0) + 1;
    return static_cast<T>(h * w);
}

// a, b = elements 2 lane, 2 lane + 1 of a line of L <= 128 values (zero beyond L) held by ONE wave; on return their box sums
// cumsum[min(k + r, L - 1)] - cumsum[k - r - 1]  (diff_x / diff_y of the reference on an inclusive cumsum).
template <typename T>
__device__ __forceinline__ void line_box(T& a, T& b, int lane, int L, int r) {
    b += a;
    T incl = b;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T t = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += t;
    }
    const T excl = incl - b;
    const T ca = a + excl, cb = b + excl;         // inclusive cumsum at 2 lane, 2 lane + 1
    auto at = [&](int k) {                        // every lane takes part in the shuffles
        const T va = __shfl(ca, k >> 1, kWave), vb = __shfl(cb, k >> 1, kWave);
        return (k & 1) ? vb : va;
    };
    const int k0 = 2 * lane, k1 = k0 + 1;
    const int hi0 = k0 + r < L - 1 ? k0 + r : L - 1, hi1 = k1 + r < L - 1 ? k1 + r : L - 1;
    const int lo0 = k0 - r - 1, lo1 = k1 - r - 1;
    const T h0 = at(hi0), h1 = at(hi1);
    const T l0 = at(lo0 > 0 ? lo0 : 0), l1 = at(lo1 > 0 ? lo1 : 0);
    a = lo0 >= 0 ? h0 - l0 : h0;
    b = lo1 >= 0 ? h1 - l1 : h1;
}

// ---- column pass; a block = (plane, strip of 32 columns, ONE quantity q of the stage).
//   STAGE 0: (x, y, xy, xx) -> saved[0..3];  1: (A = saved[2], b = saved[4]) -> (out, saved[4]);
//         2: (g x / N, g / N) -> (grad_x, ws[0]);   3: (grad_x, ws[0], ws[1]) in place.
template <int STAGE>
struct GfStageQ { static constexpr int value = STAGE == 0 ? 4 : (STAGE == 3 ? 3 : 2); };

template <typename T, int STAGE>
__global__ void __launch_bounds__(kBlock)
gf_cols_kernel(const GfArgs<T> a, int strips) {
    constexpr int Q = GfStageQ<STAGE>::value;
    constexpr int NW = kBlock / kWave;
    constexpr int LPW = kGfStrip / NW;                          // lines per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* tile = reinterpret_cast<T*>(smem_raw);                  // [kGfStrip][P], a column is a contiguous line
    const int H = a.H, W = a.W;
    const int P = (H | 1) + 1;                                 // 130 = 2 (mod 64) for H = 128: the transposing writes of a wave (32 columns x 2 rows) hit 64 banks
    unsigned bid = blockIdx.x;
    const int q = bid % Q;
    bid /= Q;
    const int strip = bid % strips;
    const int64_t plane = bid / strips;
    const size_t S = static_cast<size_t>(a.planes) * H * W;    // plane-set stride
    const size_t base = static_cast<size_t>(plane) * H * W;
    const int cc = threadIdx.x & (kGfStrip - 1), rr = threadIdx.x / kGfStrip;
    const int j = strip * kGfStrip + cc;
    const T* src = nullptr;
    T* dst = nullptr;
    if constexpr (STAGE == 0) dst = a.saved + q * S;
    if constexpr (STAGE == 1) { src = a.saved + (q == 0 ? 2 : 4) * S; dst = q == 0 ? a.out : a.saved + 4 * S; }
    if constexpr (STAGE == 2) dst = q == 0 ? a.out : a.ws;
    if constexpr (STAGE == 3) { dst = q == 0 ? a.out : a.ws + (q - 1) * S; src = dst; }

    // all of the thread's loads are issued before the first use (a rolled loop paid one memory round trip per row)
    constexpr int RPP = kBlock / kGfStrip;                      // rows per pass
    constexpr int NIT = kGfMaxDim / RPP;
    T v[NIT], v2[NIT];
    const bool inj = j < W;
    auto load_all = [&](const T* ptr, T (&dstv)[NIT]) {
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int i = rr + k * RPP;
            dstv[k] = (inj && i < H) ? ptr[base + static_cast<size_t>(i) * W + j] : static_cast<T>(0);
        }
    };
    if constexpr (STAGE == 0) {
        if (q == 1) {
            load_all(a.y, v);
        } else {
            load_all(a.x, v);
            if (q == 2) {
                load_all(a.y, v2);
#pragma unroll
                for (int k = 0; k < NIT; ++k) v[k] = v[k] * v2[k];
            } else if (q == 3) {
#pragma unroll
                for (int k = 0; k < NIT; ++k) v[k] = v[k] * v[k];
            }
        }
    } else if constexpr (STAGE == 2) {
        load_all(a.g, v);
        if (q == 0) load_all(a.x, v2);
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const T n = box_count<T>(rr + k * RPP, inj ? j : 0, H, W, a.r);
            v[k] = q == 0 ? v[k] * v2[k] / n : v[k] / n;                             // d mean_A -> d A, d mean_b -> d b
        }
    } else {
        load_all(src, v);
    }
    if (inj) {
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int i = rr + k * RPP;
            if (i < H) tile[cc * P + i] = v[k];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int ncol = (W - strip * kGfStrip) < kGfStrip ? (W - strip * kGfStrip) : kGfStrip;
    const int i0 = 2 * lane;
    T va[LPW], vb[LPW];
#pragma unroll
    for (int k = 0; k < LPW; ++k) {                              // the wave's lines side by side: their shuffle chains interleave
        const T* ln = tile + (wave + k * NW) * P;
        const bool live = wave + k * NW < ncol;
        va[k] = live && i0 < H ? ln[i0] : static_cast<T>(0);
        vb[k] = live && i0 + 1 < H ? ln[i0 + 1] : static_cast<T>(0);
    }
#pragma unroll
    for (int k = 0; k < LPW; ++k) line_box(va[k], vb[k], lane, H, a.r);
#pragma unroll
    for (int k = 0; k < LPW; ++k) {
        T* ln = tile + (wave + k * NW) * P;
        if (wave + k * NW < ncol) {
            if (i0 < H) ln[i0] = va[k];
            if (i0 + 1 < H) ln[i0 + 1] = vb[k];
        }
    }
    __syncthreads();
    if (inj) {
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int i = rr + k * RPP;
            if (i < H) dst[base + static_cast<size_t>(i) * W + j] = tile[cc * P + i];
        }
    }
}

// ---- row pass + the stage's pointwise epilogue; a wave per row.
//   STAGE 0: saved[0..3] (column sums of x, y, xy, xx) -> saved[0..4] = mean_x, mean_y, A, var + eps, b
//         1: (out, saved[4]) (column sums of A, b)      -> saved[4] = mean_A, out = mean_A x + mean_b
//         2: (grad_x, ws[0]) (column sums of g x / N, g / N) -> (grad_x, ws[0], ws[1]) = (d mean_x, d E[xy], d E[xx]) / N
//         3: (grad_x, ws[0], ws[1]) -> grad_x
template <typename T, int STAGE>
__global__ void __launch_bounds__(kBlock)
gf_rows_kernel(const GfArgs<T> a) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int H = a.H, W = a.W;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + wave;
    if (row >= a.planes * H) return;
    const int i = static_cast<int>(row % H);
    const size_t S = static_cast<size_t>(a.planes) * H * W;
    const size_t base = static_cast<size_t>(row) * W;              // (plane * H + i) * W
    const int j0 = 2 * lane, j1 = j0 + 1;
    const bool in0 = j0 < W, in1 = j1 < W;
    const size_t p0 = base + (in0 ? j0 : 0), p1 = base + (in1 ? j1 : 0);
    auto box_of = [&](const T* src, T& s0, T& s1) {
        s0 = in0 ? src[p0] : static_cast<T>(0);
        s1 = in1 ? src[p1] : static_cast<T>(0);
        line_box(s0, s1, lane, W, a.r);
    };
    const T n0 = box_count<T>(i, in0 ? j0 : 0, H, W, a.r), n1 = box_count<T>(i, in1 ? j1 : 0, H, W, a.r);
    if constexpr (STAGE == 0) {
        T bx0, bx1, by0, by1, bxy0, bxy1, bxx0, bxx1;
        box_of(a.saved, bx0, bx1);
        box_of(a.saved + S, by0, by1);
        box_of(a.saved + 2 * S, bxy0, bxy1);
        box_of(a.saved + 3 * S, bxx0, bxx1);
        auto fin = [&](size_t p, T n, T bx, T by, T bxy, T bxx) {
            const T mx = bx / n, my = by / n;
            const T cov = bxy / n - mx * my;
            const T ve = (bxx / n - mx * mx) + a.eps;               // var_x + eps
            const T A = cov / ve;
            a.saved[p] = mx;
            a.saved[S + p] = my;
            a.saved[2 * S + p] = A;
            a.saved[3 * S + p] = ve;
            a.saved[4 * S + p] = my - A * mx;                       // b
        };
        if (in0) fin(p0, n0, bx0, by0, bxy0, bxx0);
        if (in1) fin(p1, n1, bx1, by1, bxy1, bxx1);
    } else if constexpr (STAGE == 1) {
        T bA0, bA1, bb0, bb1;
        box_of(a.out, bA0, bA1);
        box_of(a.saved + 4 * S, bb0, bb1);
        if (in0) { const T mA = bA0 / n0; a.saved[4 * S + p0] = mA; a.out[p0] = mA * a.x[p0] + bb0 / n0; }
        if (in1) { const T mA = bA1 / n1; a.saved[4 * S + p1] = mA; a.out[p1] = mA * a.x[p1] + bb1 / n1; }
    } else if constexpr (STAGE == 2) {
        T q10, q11, q20, q21;
        box_of(a.out, q10, q11);
        box_of(a.ws, q20, q21);
        auto fin = [&](size_t p, T n, T q1, T q2) {
            const T mx = a.saved[p], my = a.saved[S + p], A = a.saved[2 * S + p], ve = a.saved[3 * S + p];
            const T gA = q1 - q2 * mx;                              // b = mean_y - A mean_x
            T gmx = -q2 * A;
            const T gcov = gA / ve;                                 // A = cov / (var + eps)
            const T gvar = -gA * A / ve;
            gmx += -gcov * my - 2 * gvar * mx;                      // cov = E[xy] - mx my ; var = E[xx] - mx^2
            a.out[p] = gmx / n;
            a.ws[p] = gcov / n;
            a.ws[S + p] = gvar / n;
        };
        if (in0) fin(p0, n0, q10, q20);
        if (in1) fin(p1, n1, q11, q21);
    } else {
        T r10, r11, r20, r21, r30, r31;
        box_of(a.out, r10, r11);                                    // -> d x through mean_x
        box_of(a.ws, r20, r21);                                     // -> d (x y)
        box_of(a.ws + S, r30, r31);                                 // -> d (x x)
        auto fin = [&](size_t p, T r1, T r2, T r3) {
            T v = r1 + a.g[p] * a.saved[4 * S + p];                 // + g * mean_A
            v += a.y[p] * r2;
            a.out[p] = v + 2 * a.x[p] * r3;
        };
        if (in0) fin(p0, r10, r20, r30);
        if (in1) fin(p1, r11, r21, r31);
    }
}

template <typename T, int STAGE>
void gf_launch_cols(const GfArgs<T>& a, hipStream_t st) {
    constexpr int Q = GfStageQ<STAGE>::value;
    const int strips = (a.W + kGfStrip - 1) / kGfStrip;
    const int P = (a.H | 1) + 1;
    const size_t lds = static_cast<size_t>(kGfStrip) * P * sizeof(T);
    hipLaunchKernelGGL((gf_cols_kernel<T, STAGE>), dim3(static_cast<unsigned>(a.planes * strips * Q)), dim3(kBlock), lds, st, a, strips);
}
template <typename T, int STAGE>
void gf_launch_rows(const GfArgs<T>& a, hipStream_t st) {
    const int64_t rows = a.planes * a.H;
    const int per = kBlock / kWave;
    hipLaunchKernelGGL((gf_rows_kernel<T, STAGE>), dim3(static_cast<unsigned>((rows + per - 1) / per)), dim3(kBlock), 0, st, a);
}

template <typename T>
void gf_forward(const void* x, const void* y, void* out, void* saved, int64_t planes, int H, int W, int r, double eps, hipStream_t st) {
    GfArgs<T> a{static_cast<const T*>(x), static_cast<const T*>(y), nullptr, static_cast<T*>(saved), static_cast<T*>(out), nullptr,
                planes, H, W, r, static_cast<T>(eps)};
    gf_launch_cols<T, 0>(a, st);
    gf_launch_rows<T, 0>(a, st);
    gf_launch_cols<T, 1>(a, st);
    gf_launch_rows<T, 1>(a, st);
}
template <typename T>
void gf_backward(const void* x, const void* y, const void* saved, const void* g, void* gx, void* ws, int64_t planes, int H, int W, int r,
                 hipStream_t st) {
    GfArgs<T> a{static_cast<const T*>(x), static_cast<const T*>(y), static_cast<const T*>(g), const_cast<T*>(static_cast<const T*>(saved)),
                static_cast<T*>(gx), static_cast<T*>(ws), planes, H, W, r, static_cast<T>(0)};
    gf_launch_cols<T, 2>(a, st);
    gf_launch_rows<T, 2>(a, st);
    gf_launch_cols<T, 3>(a, st);
    gf_launch_rows<T, 3>(a, st);
}

int check_args(const char* fn, int64_t planes, int64_t H, int64_t W, int r, int dtype) {
    FFWM_REQUIRE(dtype_ok(dtype), FFWM_ERR_DTYPE, "%s: dtype %d is not FFWM_F32/FFWM_F64", fn, dtype);
    FFWM_REQUIRE(planes > 0 && H > 0 && W > 0 && r >= 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(H > 2 * r + 1 && W > 2 * r + 1, FFWM_ERR_ARG,
                 "%s: need H > 2r+1 and W > 2r+1 (H=%lld W=%lld r=%d), as the reference asserts", fn, (long long)H,
                 (long long)W, r);
    FFWM_REQUIRE(H <= kGfMaxDim && W <= kGfMaxDim, FFWM_ERR_SIZE,
                 "%s: planes up to %d x %d (a wave holds a line as two elements per lane), got %lld x %lld; larger planes: %s_general", fn,
                 kGfMaxDim, kGfMaxDim, (long long)H, (long long)W, fn);
    FFWM_REQUIRE(planes < (1LL << 31), FFWM_ERR_SIZE, "%s: too many planes", fn);
    return FFWM_OK;
}


// ================================================================================================ the general path
// Planes of any size (a side up to kGfgMaxSide, H W < 2^28), a guide x of one channel broadcast over the channels of y (Px planes
// of x, Py = Px * cdiv planes of y), and the gradient for y.  The eight-launch structure of the kernels above stays -- a column pass
// and a row pass with the pointwise stage fused behind it, twice per direction, plus one more row pass forward so that mean_x and
// var_x + eps are formed once per x plane -- but a line no longer has to fit one wave:
//   gfg_cols_kernel: a WAVE owns 64 columns x `rc` rows of ONE quantity (work units = quantity-planes x row chunks x 64-column strips;
//                    no LDS, no barrier).  A lane walks down its column with a sliding-window sum S(i) = S(i-1) + in[i+r] - in[i-r-1]
//                    (rows outside the image contribute nothing: that is the reference's clipped window), seeded with the
//                    window of the row above the chunk, read from the chunk's own halo.  Every load is a coalesced row segment.
//   gfg_rows_kernel: a WAVE owns kGfgRowChunk = 256 consecutive outputs of one row: the seed is a wave reduction over the halo,
//                    then four 64-wide segments, each an inclusive wave scan of in[k+r] - in[k-r-1] on top of the carried sum; all
//                    quantities of the stage side by side, the pointwise epilogue behind them.  No LDS, no barrier.
// Registers and LDS (none) do not depend on H, W or r; a window may cross any number of chunk or segment boundaries, only the seed
// loop gets longer (2r + 1 loads per chunk).  Every pass reads planes that the passes of the same launch do not write (chunks read
// each other's halo), hence the workspace.  A sum runs over at most `rc` / 256 steps before it is seeded afresh, so the rounding error
// does not grow with the line as a cumsum's does.  Sums over the channels of a broadcast guide are taken in registers, channel 0 first.
constexpr int kGfgMaxSide = 8192;
constexpr int64_t kGfgMaxPlane = 1LL << 28;
constexpr int kGfgSegs = 4;
constexpr int kGfgRowChunk = kGfgSegs * kWave;
constexpr int kGfgWaves = kBlock / kWave;
enum { kGfgRows0X = 0, kGfgRows0Y = 1, kGfgRows1 = 2, kGfgRows2 = 3, kGfgRows3 = 4 };
enum { kGfgWantX = 1, kGfgWantY = 2 };

template <typename T>
struct GfgArgs {
    const T* x;        // [Px, H, W]
    const T* y;        // [Py, H, W]
    const T* g;        // grad_output [Py, H, W] (backward)
    T* mx;             // saved: mean_x [Px], mean_y [Py], A [Py], var_x + eps [Px], mean_A [Py] -- for Px == Py the [5, planes, H, W]
    T* my;             //        layout of the kernels above
    T* A;
    T* ve;
    T* mA;
    T* out;            // output (forward)
    T* gx;             // grad_x / grad_y (backward), NULL = not wanted
    T* gy;
    T* wa;             // workspace: column sums
    T* wb;             // workspace: the planes between the two halves of the backward
    int64_t Px, Py;
    int cdiv;          // Py / Px: channels of y per channel of x
    int H, W, r;
    int rc;            // rows per work unit of the column pass
    T eps;
};

// the pointwise input of a column pass, formed on the fly: p0, p0 p1, p0^2, p0 / N, p0 p1 / N
template <typename T>
struct GfgSrc {
    const T* p0;
    const T* p1;
    int kind;
};
template <typename T>
__device__ __forceinline__ T gfg_in(const GfgSrc<T>& s, int i, int j, int H, int W, int r) {
    const int idx = i * W + j;
    T v = s.p0[idx];
    if (s.kind == 1 || s.kind == 4) v = v * s.p1[idx];
    else if (s.kind == 2) v = v * v;
    if (s.kind >= 3) v = v / box_count<T>(i, j, H, W, r);
    return v;
}

// ---- column pass.  Quantity-planes ("jobs") of a stage, in the order of the workspace planes they fill:
//   STAGE 0: x [Px], x x [Px], y [Py], x y [Py]              1: A [Py], b (in the mean_A plane) [Py]
//         2: g x / N [Py], g / N [Py]
//         3: wb -> wa, plane for plane: d E[xy] / N [Py], d mean_y / N [Py] (if grad_y), d mean_x / N [Px], d E[xx] / N [Px] (if grad_x)
template <typename T, int STAGE>
__global__ void __launch_bounds__(kBlock)
gfg_cols_kernel(const GfgArgs<T> a, int strips, int chunks, int64_t units, int want) {
    const int lane = threadIdx.x & (kWave - 1);
    int64_t u = static_cast<int64_t>(blockIdx.x) * kGfgWaves + threadIdx.x / kWave;
    if (u >= units) return;
    const int strip = static_cast<int>(u % strips);
    u /= strips;
    const int chunk = static_cast<int>(u % chunks);
    int64_t job = u / chunks;
    const int H = a.H, W = a.W, r = a.r;
    const size_t HW = static_cast<size_t>(H) * W;
    GfgSrc<T> s{nullptr, nullptr, 0};
    if constexpr (STAGE == 0) {
        if (job < 2 * a.Px) {
            s.p0 = a.x + (job % a.Px) * HW;
            s.kind = job < a.Px ? 0 : 2;
        } else {
            const int64_t k = job - 2 * a.Px, pl = k % a.Py;
            s.p1 = a.y + pl * HW;
            s.p0 = k < a.Py ? s.p1 : a.x + (pl / a.cdiv) * HW;
            s.kind = k < a.Py ? 0 : 1;
        }
    } else if constexpr (STAGE == 1) {
        s.p0 = job < a.Py ? a.A + job * HW : a.mA + (job - a.Py) * HW;
    } else if constexpr (STAGE == 2) {
        const int64_t pl = job % a.Py;
        s.p0 = a.g + pl * HW;
        s.p1 = a.x + (pl / a.cdiv) * HW;
        s.kind = job < a.Py ? 4 : 3;
    } else {
        if (job >= a.Py && !(want & kGfgWantY)) job += a.Py;
        s.p0 = a.wb + job * HW;
    }
    T* dst = a.wa + job * HW;
    const int j = strip * kWave + lane;
    if (j >= W) return;
    const int i0 = chunk * a.rc, i1 = i0 + a.rc < H ? i0 + a.rc : H;
    int lo = i0 - 1 - r, hi = i0 - 1 + r;
    lo = lo > 0 ? lo : 0;
    hi = hi < H - 1 ? hi : H - 1;
    T sum = static_cast<T>(0);
#pragma unroll 4
    for (int i = lo; i <= hi; ++i) sum += gfg_in(s, i, j, H, W, r);
#pragma unroll 4
    for (int i = i0; i < i1; ++i) {
        const int ia = i + r, is = i - r - 1;
        const T add = ia < H ? gfg_in(s, ia, j, H, W, r) : static_cast<T>(0);
        const T sub = is >= 0 ? gfg_in(s, is, j, H, W, r) : static_cast<T>(0);
        sum += add - sub;
        dst[i * W + j] = sum;
    }
}

template <typename T>
__device__ __forceinline__ T gfg_wave_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T t = __shfl_up(v, o, kWave);
        if (lane >= o) v += t;
    }
    return v;
}

// Box sums of the outputs [s, e) (e - s <= kGfgRowChunk) of Q rows, by ONE wave: f(segment, k, S[Q]) for the wave's element k of
// every 64-wide segment (k may lie beyond e in the last one).
template <typename T, int Q, class F>
__device__ __forceinline__ void gfg_row_boxes(const T* const (&rows)[Q], int s, int e, int W, int r, int lane, F&& f) {
    T carry[Q];
    int lo = s - 1 - r, hi = s - 1 + r;
    lo = lo > 0 ? lo : 0;
    hi = hi < W - 1 ? hi : W - 1;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        T acc = static_cast<T>(0);
        for (int m = lo + lane; m <= hi; m += kWave) acc += rows[q][m];
        carry[q] = wave_sum(acc);                              // the same bits in every lane: a + b and b + a at every step
    }
#pragma unroll
    for (int sg = 0; sg < kGfgSegs; ++sg) {
        const int k0 = s + sg * kWave;
        if (k0 < e) {                                          // wave-uniform
            const int k = k0 + lane, ia = k + r, is = k - r - 1;
            T S[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const T add = ia < W ? rows[q][ia] : static_cast<T>(0);
                const T sub = (is >= 0 && is < W) ? rows[q][is] : static_cast<T>(0);
                S[q] = carry[q] + gfg_wave_scan(add - sub, lane);
                carry[q] = __shfl(S[q], kWave - 1, kWave);
            }
            f(sg, k, S);
        }
    }
}

// ---- row pass + pointwise epilogue; a wave = (plane, row, chunk of 256 outputs); the planes are x planes except in 0Y and 1.
//   0X: wa (x, x x)            -> mean_x, var_x + eps                      0Y: wa (y, x y) -> mean_y, A, b (in the mean_A plane)
//   1 : wa (A, b)              -> mean_A, out = mean_A x + mean_b
//   2 : wa (g x / N, g / N)    -> wb: the four planes of column stage 3 (d mean_x and d E[xx] summed over the channels of the x plane)
//   3 : wa (those, column sums) -> grad_x (summed over the channels), grad_y
template <typename T, int ROWS>
__global__ void __launch_bounds__(kBlock)
gfg_rows_kernel(const GfgArgs<T> a, int rchunks, int64_t units, int want) {
    const int lane = threadIdx.x & (kWave - 1);
    int64_t u = static_cast<int64_t>(blockIdx.x) * kGfgWaves + threadIdx.x / kWave;
    if (u >= units) return;
    const int chunk = static_cast<int>(u % rchunks);
    u /= rchunks;
    const int H = a.H, W = a.W, r = a.r;
    const int i = static_cast<int>(u % H);
    const int64_t plane = u / H;
    const size_t HW = static_cast<size_t>(H) * W, ro = static_cast<size_t>(i) * W;
    const int s = chunk * kGfgRowChunk, e = s + kGfgRowChunk < W ? s + kGfgRowChunk : W;
    if constexpr (ROWS == kGfgRows0X) {
        const T* rows[2] = {a.wa + plane * HW + ro, a.wa + (a.Px + plane) * HW + ro};
        gfg_row_boxes<T, 2>(rows, s, e, W, r, lane, [&](int, int k, const T (&S)[2]) {
            if (k >= e) return;
            const T n = box_count<T>(i, k, H, W, r);
            const T mx = S[0] / n;
            a.mx[plane * HW + ro + k] = mx;
            a.ve[plane * HW + ro + k] = (S[1] / n - mx * mx) + a.eps;
        });
    } else if constexpr (ROWS == kGfgRows0Y) {
        const T* rows[2] = {a.wa + (2 * a.Px + plane) * HW + ro, a.wa + (2 * a.Px + a.Py + plane) * HW + ro};
        const size_t px = (plane / a.cdiv) * HW + ro, py = plane * HW + ro;
        gfg_row_boxes<T, 2>(rows, s, e, W, r, lane, [&](int, int k, const T (&S)[2]) {
            if (k >= e) return;
            const T n = box_count<T>(i, k, H, W, r);
            const T mx = a.mx[px + k], my = S[0] / n;
            const T A = (S[1] / n - mx * my) / a.ve[px + k];
            a.my[py + k] = my;
            a.A[py + k] = A;
            a.mA[py + k] = my - A * mx;                                    // b
        });
    } else if constexpr (ROWS == kGfgRows1) {
        const T* rows[2] = {a.wa + plane * HW + ro, a.wa + (a.Py + plane) * HW + ro};
        const size_t px = (plane / a.cdiv) * HW + ro, py = plane * HW + ro;
        gfg_row_boxes<T, 2>(rows, s, e, W, r, lane, [&](int, int k, const T (&S)[2]) {
            if (k >= e) return;
            const T n = box_count<T>(i, k, H, W, r);
            const T mA = S[0] / n;
            a.mA[py + k] = mA;
            a.out[py + k] = mA * a.x[px + k] + S[1] / n;
        });
    } else if constexpr (ROWS == kGfgRows2) {
        const size_t px = plane * HW + ro;
        T amx[kGfgSegs], avar[kGfgSegs];
#pragma unroll
        for (int sg = 0; sg < kGfgSegs; ++sg) amx[sg] = avar[sg] = static_cast<T>(0);
        for (int c = 0; c < a.cdiv; ++c) {
            const int64_t yp = plane * a.cdiv + c;
            const size_t py = yp * HW + ro;
            const T* rows[2] = {a.wa + py, a.wa + a.Py * HW + py};
            gfg_row_boxes<T, 2>(rows, s, e, W, r, lane, [&](int sg, int k, const T (&S)[2]) {
                if (k >= e) return;
                const T n = box_count<T>(i, k, H, W, r);
                const T mx = a.mx[px + k], ve = a.ve[px + k], my = a.my[py + k], A = a.A[py + k];
                const T q1 = S[0], q2 = S[1];
                const T gA = q1 - q2 * mx;                                  // b = mean_y - A mean_x
                T gmx = -q2 * A;
                const T gcov = gA / ve;                                     // A = cov / (var + eps)
                const T gvar = -gA * A / ve;
                gmx += -gcov * my - 2 * gvar * mx;                          // cov = E[xy] - mx my ; var = E[xx] - mx^2
                amx[sg] += gmx;
                avar[sg] += gvar;
                a.wb[py + k] = gcov / n;
                if (want & kGfgWantY) a.wb[a.Py * HW + py + k] = (q2 - gcov * mx) / n;     // d mean_y
            });
        }
        if (want & kGfgWantX) {
#pragma unroll
            for (int sg = 0; sg < kGfgSegs; ++sg) {
                const int k = s + sg * kWave + lane;
                if (k < e) {
                    const T n = box_count<T>(i, k, H, W, r);
                    a.wb[2 * a.Py * HW + px + k] = amx[sg] / n;
                    a.wb[(2 * a.Py + a.Px) * HW + px + k] = avar[sg] / n;
                }
            }
        }
    } else {
        const size_t px = plane * HW + ro;
        T v[kGfgSegs];
#pragma unroll
        for (int sg = 0; sg < kGfgSegs; ++sg) v[sg] = static_cast<T>(0);
        if (want & kGfgWantX) {
            const T* rows[2] = {a.wa + 2 * a.Py * HW + px, a.wa + (2 * a.Py + a.Px) * HW + px};
            gfg_row_boxes<T, 2>(rows, s, e, W, r, lane, [&](int sg, int k, const T (&S)[2]) {
                if (k < e) v[sg] = S[0] + 2 * a.x[px + k] * S[1];           // through mean_x and E[xx]
            });
        }
        for (int c = 0; c < a.cdiv; ++c) {
            const size_t py = (plane * a.cdiv + c) * HW + ro;
            auto fin = [&](int sg, int k, T r2, T r4) {
                if (k >= e) return;
                if (want & kGfgWantX) v[sg] += a.g[py + k] * a.mA[py + k] + a.y[py + k] * r2;
                if (want & kGfgWantY) a.gy[py + k] = a.x[px + k] * r2 + r4;
            };
            if (want & kGfgWantY) {
                const T* rows[2] = {a.wa + py, a.wa + a.Py * HW + py};
                gfg_row_boxes<T, 2>(rows, s, e, W, r, lane, [&](int sg, int k, const T (&S)[2]) { fin(sg, k, S[0], S[1]); });
            } else {
                const T* rows[1] = {a.wa + py};
                gfg_row_boxes<T, 1>(rows, s, e, W, r, lane, [&](int sg, int k, const T (&S)[1]) { fin(sg, k, S[0], static_cast<T>(0)); });
            }
        }
        if (want & kGfgWantX) {
#pragma unroll
            for (int sg = 0; sg < kGfgSegs; ++sg) {
                const int k = s + sg * kWave + lane;
                if (k < e) a.gx[px + k] = v[sg];
            }
        }
    }
}

inline int64_t gfg_cdiv(int64_t n, int64_t d) { return (n + d - 1) / d; }
// Rows per work unit of the column pass: 128, halved while the smallest launch (two quantities) has fewer than 2048 waves.  A function
// of the shape alone, so that a gradient has the same bits whichever other gradient is asked for.
inline int gfg_col_rows(int64_t Py, int64_t H, int64_t W) {
    int rc = 128;
    while (rc > 32 && 2 * Py * gfg_cdiv(W, kWave) * gfg_cdiv(H, rc) < 2048) rc /= 2;
    return rc;
}

template <typename T, int STAGE>
void gfg_launch_cols(const GfgArgs<T>& a, int64_t jobs, int want, hipStream_t st) {
    const int strips = static_cast<int>(gfg_cdiv(a.W, kWave)), chunks = static_cast<int>(gfg_cdiv(a.H, a.rc));
    const int64_t units = jobs * strips * chunks;
    hipLaunchKernelGGL((gfg_cols_kernel<T, STAGE>), dim3(static_cast<unsigned>(gfg_cdiv(units, kGfgWaves))), dim3(kBlock), 0, st, a, strips,
                       chunks, units, want);
}
template <typename T, int ROWS>
void gfg_launch_rows(const GfgArgs<T>& a, int64_t planes, int want, hipStream_t st) {
    const int rchunks = static_cast<int>(gfg_cdiv(a.W, kGfgRowChunk));
    const int64_t units = planes * a.H * rchunks;
    hipLaunchKernelGGL((gfg_rows_kernel<T, ROWS>), dim3(static_cast<unsigned>(gfg_cdiv(units, kGfgWaves))), dim3(kBlock), 0, st, a, rchunks,
                       units, want);
}

template <typename T>
GfgArgs<T> gfg_args(const void* x, const void* y, const void* g, const void* saved, void* out, void* gx, void* gy, void* ws, int64_t Px,
                    int64_t Py, int H, int W, int r, double eps) {
    const size_t HW = static_cast<size_t>(H) * W;
    T* sv = const_cast<T*>(static_cast<const T*>(saved));
    GfgArgs<T> a;
    a.x = static_cast<const T*>(x);
    a.y = static_cast<const T*>(y);
    a.g = static_cast<const T*>(g);
    a.mx = sv;
    a.my = a.mx + Px * HW;
    a.A = a.my + Py * HW;
    a.ve = a.A + Py * HW;
    a.mA = a.ve + Px * HW;
    a.out = static_cast<T*>(out);
    a.gx = static_cast<T*>(gx);
    a.gy = static_cast<T*>(gy);
    a.wa = static_cast<T*>(ws);
    a.wb = a.wa + 2 * (Px + Py) * HW;
    a.Px = Px;
    a.Py = Py;
    a.cdiv = static_cast<int>(Py / Px);
    a.H = H;
    a.W = W;
    a.r = r;
    a.rc = gfg_col_rows(Py, H, W);
    a.eps = static_cast<T>(eps);
    return a;
}

template <typename T>
void gfg_forward(const GfgArgs<T>& a, hipStream_t st) {
    gfg_launch_cols<T, 0>(a, 2 * (a.Px + a.Py), 0, st);
    gfg_launch_rows<T, kGfgRows0X>(a, a.Px, 0, st);
    gfg_launch_rows<T, kGfgRows0Y>(a, a.Py, 0, st);
    gfg_launch_cols<T, 1>(a, 2 * a.Py, 0, st);
    gfg_launch_rows<T, kGfgRows1>(a, a.Py, 0, st);
}
template <typename T>
void gfg_backward(const GfgArgs<T>& a, hipStream_t st) {
    const int want = (a.gx ? kGfgWantX : 0) | (a.gy ? kGfgWantY : 0);
    gfg_launch_cols<T, 2>(a, 2 * a.Py, want, st);
    gfg_launch_rows<T, kGfgRows2>(a, a.Px, want, st);
    gfg_launch_cols<T, 3>(a, a.Py + (a.gy ? a.Py : 0) + (a.gx ? 2 * a.Px : 0), want, st);
    gfg_launch_rows<T, kGfgRows3>(a, a.Px, want, st);
}

inline bool gfg_fast(int64_t Px, int64_t Py, int64_t H, int64_t W) { return Px == Py && H <= kGfMaxDim && W <= kGfMaxDim; }

int check_args_general(const char* fn, int64_t Px, int64_t Py, int64_t H, int64_t W, int r, int dtype) {
    FFWM_REQUIRE(dtype_ok(dtype), FFWM_ERR_DTYPE, "%s: dtype %d is not FFWM_F32/FFWM_F64", fn, dtype);
    FFWM_REQUIRE(Px > 0 && Py > 0 && H > 0 && W > 0 && r >= 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(Py % Px == 0, FFWM_ERR_ARG,
                 "%s: planes_y (%lld) must be a multiple of planes_x (%lld): the guide has one channel or as many as y (Cx in {1, Cy})",
                 fn, (long long)Py, (long long)Px);
    FFWM_REQUIRE(H > 2 * (int64_t)r + 1 && W > 2 * (int64_t)r + 1, FFWM_ERR_ARG,
                 "%s: need H > 2r+1 and W > 2r+1 (H=%lld W=%lld r=%d), as the reference asserts", fn, (long long)H, (long long)W, r);
    FFWM_REQUIRE(H <= kGfgMaxSide && W <= kGfgMaxSide && H * W < kGfgMaxPlane, FFWM_ERR_SIZE,
                 "%s: H and W up to %d (and H W < 2^28 elements), got H=%lld W=%lld", fn, kGfgMaxSide, (long long)H, (long long)W);
    // the largest launch: four quantities per plane, 32-row chunks, 64-column strips, four waves per workgroup
    FFWM_REQUIRE(Py < (1LL << 31) && 4 * Py * gfg_cdiv(H, 32) * gfg_cdiv(W, kWave) < (1LL << 32) && Py * H * gfg_cdiv(W, kGfgRowChunk) < (1LL << 32),
                 FFWM_ERR_SIZE, "%s: too many planes (planes_y=%lld of %lld x %lld)", fn, (long long)Py, (long long)H, (long long)W);
    return FFWM_OK;
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_guided_filter_forward(const void* x, const void* y, void* output, void* saved, int64_t planes,
                                          int64_t H, int64_t W, int r, double eps, int dtype, void* stream) {
    const char* fn = "ffwm_guided_filter_forward";
    FFWM_REQUIRE(x && y && output && saved, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    if (int rc = check_args(fn, planes, H, W, r, dtype)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t esz = dtype == FFWM_F32 ? 4 : 8;
    LaunchScope ls("guided_filter_fwd", st, static_cast<double>(esz) * planes * H * W * 8.0);   // x, y in; out + 5 saved planes
    if (dtype == FFWM_F32)
        gf_forward<float>(x, y, output, saved, planes, (int)H, (int)W, r, eps, st);
    else
        gf_forward<double>(x, y, output, saved, planes, (int)H, (int)W, r, eps, st);
    return check_launch(fn);
}

extern "C" int ffwm_guided_filter_backward(const void* x, const void* y, const void* saved, const void* grad_output,
                                           void* grad_x, void* workspace, int64_t planes, int64_t H, int64_t W, int r, int dtype,
                                           void* stream) {
    const char* fn = "ffwm_guided_filter_backward";
    FFWM_REQUIRE(x && y && saved && grad_output && grad_x && workspace, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    if (int rc = check_args(fn, planes, H, W, r, dtype)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t esz = dtype == FFWM_F32 ? 4 : 8;
    LaunchScope ls("guided_filter_bwd", st, static_cast<double>(esz) * planes * H * W * 9.0);   // x, y, g, 5 saved in; grad out
    if (dtype == FFWM_F32)
        gf_backward<float>(x, y, saved, grad_output, grad_x, workspace, planes, (int)H, (int)W, r, st);
    else
        gf_backward<double>(x, y, saved, grad_output, grad_x, workspace, planes, (int)H, (int)W, r, st);
    return check_launch(fn);
}

// ---- the reference's whole contract: any plane size, a one-channel guide, the gradient for y
extern "C" int64_t ffwm_guided_filter_workspace_bytes(int64_t planes_x, int64_t planes_y, int64_t H, int64_t W, int dtype, int backward) {
    if (int rc = check_args_general("ffwm_guided_filter_workspace_bytes", planes_x, planes_y, H, W, 0, dtype)) return rc;
    const int64_t esz = dtype == FFWM_F32 ? 4 : 8;
    if (!backward && gfg_fast(planes_x, planes_y, H, W)) return 0;
    return (backward ? 4 : 2) * (planes_x + planes_y) * H * W * esz;
}

extern "C" int ffwm_guided_filter_forward_general(const void* x, const void* y, void* output, void* saved, void* workspace,
                                                  int64_t planes_x, int64_t planes_y, int64_t H, int64_t W, int r, double eps, int dtype,
                                                  void* stream) {
    const char* fn = "ffwm_guided_filter_forward_general";
    FFWM_REQUIRE(x && y && output && saved, FFWM_ERR_ARG, "%s: NULL tensor pointer (x, y, output, saved)", fn);
    if (int rc = check_args_general(fn, planes_x, planes_y, H, W, r, dtype)) return rc;
    const bool fast = gfg_fast(planes_x, planes_y, H, W);
    FFWM_REQUIRE(fast || workspace, FFWM_ERR_ARG, "%s: NULL workspace (ffwm_guided_filter_workspace_bytes gives its size)", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double esz = dtype == FFWM_F32 ? 4 : 8;
    if (fast) {
        LaunchScope ls("guided_filter_fwd", st, esz * planes_y * H * W * 8.0);
        by_dtype(dtype, [&](auto t) {
            gf_forward<decltype(t)>(x, y, output, saved, planes_y, (int)H, (int)W, r, eps, st);
            return 0;
        });
        return check_launch(fn);
    }
    // x, y in; out, mean_y, A, mean_A per y plane and mean_x, var_x + eps per x plane out
    LaunchScope ls("guided_filter_fwd_general", st, esz * H * W * (3.0 * planes_x + 5.0 * planes_y));
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        gfg_forward<T>(gfg_args<T>(x, y, nullptr, saved, output, nullptr, nullptr, workspace, planes_x, planes_y, (int)H, (int)W, r, eps), st);
        return 0;
    });
    return check_launch(fn);
}

extern "C" int ffwm_guided_filter_backward_general(const void* x, const void* y, const void* saved, const void* grad_output, void* grad_x,
                                                   void* grad_y, void* workspace, int64_t planes_x, int64_t planes_y, int64_t H, int64_t W,
                                                   int r, int dtype, void* stream) {
    const char* fn = "ffwm_guided_filter_backward_general";
    FFWM_REQUIRE(x && y && saved && grad_output, FFWM_ERR_ARG, "%s: NULL tensor pointer (x, y, saved, grad_output)", fn);
    FFWM_REQUIRE(grad_x || grad_y, FFWM_ERR_ARG, "%s: grad_x and grad_y are both NULL: nothing to compute", fn);
    FFWM_REQUIRE(workspace, FFWM_ERR_ARG, "%s: NULL workspace (ffwm_guided_filter_workspace_bytes gives its size)", fn);
    if (int rc = check_args_general(fn, planes_x, planes_y, H, W, r, dtype)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double esz = dtype == FFWM_F32 ? 4 : 8;
    if (gfg_fast(planes_x, planes_y, H, W) && !grad_y) {
        LaunchScope ls("guided_filter_bwd", st, esz * planes_y * H * W * 9.0);
        by_dtype(dtype, [&](auto t) {
            gf_backward<decltype(t)>(x, y, saved, grad_output, grad_x, workspace, planes_y, (int)H, (int)W, r, st);
            return 0;
        });
        return check_launch(fn);
    }
    // x, y, g and the saved planes in; the gradients asked for out
    LaunchScope ls("guided_filter_bwd_general", st,
                   esz * H * W * (3.0 * planes_x + 5.0 * planes_y + (grad_x ? planes_x : 0) + (grad_y ? planes_y : 0)));
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        gfg_backward<T>(gfg_args<T>(x, y, grad_output, saved, nullptr, grad_x, grad_y, workspace, planes_x, planes_y, (int)H, (int)W, r, 0.0), st);
        return 0;
    });
    return check_launch(fn);
}
