// conv_winograd_gemm_split.hip -- the batched-GEMM Winograd route of conv_winograd_gemm.hip with its 16 GEMMs on the bf16 matrix
// instruction: the forward of a FROZEN Conv2d(C, K, 3, 1, 1), float32 tensors in and out, opt-in (precision="bf16x3" of the inference
// classes).  v_mfma_f32_32x32x16_bf16 runs at 16 x the rate of the fp32 MFMA; every operand entry is split in two bf16 terms as
// csrc/correlation.hip's corr_colmax_split_kernel does it,  hi = bf16_rn(x),  lo = bf16_rn(x - hi)  (x - hi is exact in fp32), and a
// product sum is taken as  sum_c (U_lo V_hi + U_hi V_lo + U_hi V_hi)  in ONE fp32 accumulator: three MFMAs per 16 channels.
//
//   wgs_weights          w [K, C, 3, 3]  ->  U [16][Cp / 8][2][K][8] bf16    U = G w Gt in fp32 as wg_weights_kernel, then split
//   wgs_input_transform  x [B, C, H, W]  ->  V [16][Cp / 8][2][Tp][8] bf16   V = Bt d B in fp32 as wg_input_transform_kernel, then split
//   wgs_batched_gemm     M_p [Kp x Tp] = U_p [K x Cp] V_p [Cp x Tp]           p = 0 .. 15, fp32 M
//   wgs_output_transform M [16][Kp][Tp]  ->  y [B, K, H, W]                   y = At M A (wg_tile_of), then bias / bias + LeakyReLU
//
// The frozen loss networks of the train step take the same GEMM through ffwm_conv3x3_wg_split_apply (loss_precision="bf16x3"): the
// data gradient reads U made from the layer's own weight transposed and rotated (wgs_weights, mode 1) and the ReLU mask inside the
// input transform, exactly as conv_winograd_gemm.hip does it; the output transform has that route's epilogues (bias, bias + ReLU,
// bias + max-feature-map).  Bounds of those: tests/wino_split_train_cases.py.
//
// Layout.  Eight consecutive channels of one row (output channel k, or tile t) are one 16-byte line, the operand of one lane of the
// MFMA (lane & 31 = row, lane >> 5 selects k 0-7 / 8-15); index [2] is the hi line, then the lo line.  hi and lo together take the 4
// bytes per entry fp32 takes.  Cp = C rounded up to 32 (one LDS stage), zero filled on both sides; Tp / Kp = T / K rounded up to the
// GEMM tile.  The padded columns of V hold zeros, the padded rows of U are zero filled in LDS.
//
// Error per output element (derivation: tests/wino_split_cases.py):
//   |y - ref| <= 16 (2^-16 MAG + SAFETY (3 C + 11) u MAG) mag_patch + (SAFETY + post) u |ref| + eta,    MAG = 1 + 2^-6.
// Non-finite: an infinite entry of U or V has hi = inf and lo = bf16(inf - inf) = NaN, so an infinity in the input or the weight
// behaves as a NaN over the reach of its 4 x 4 patch.  Finite |x| >= 2^125 is outside the contract (V sums four inputs, hi may round
// to infinity).  No atomics, no split of the reduction: two calls agree bit for bit.
#include "conv_winograd_gemm.hpp"

namespace ffwm {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

enum { kWgsNone = FFWM_WGS_NONE, kWgsBias = FFWM_WGS_BIAS, kWgsBiasLrelu = FFWM_WGS_BIAS_LRELU };
constexpr int kWgsStage = 32;            // input channels per LDS stage of the GEMM: four groups of eight, two MFMA k-steps

// x = hi + lo + e, |e| <= 2^-18 |x|: hi = bf16_rn(x), lo = bf16_rn(x - hi) (the difference is exact in fp32; inf - inf = NaN)
__device__ __forceinline__ void wgs_split(float x, __bf16& hi, __bf16& lo) {
    hi = static_cast<__bf16>(x);
    lo = static_cast<__bf16>(x - static_cast<float>(hi));
}

// ---------------------------------------------------------------------------------------------------- weights
// One thread = one (k, c), c < Cp: (G w Gt)[p] with the arithmetic of wg_weights_kernel, zero for C <= c, then the split.  mode 0: w
// is [K][C][3][3]; mode 1 (data gradient): w is the layer's own [C][K][3][3], read transposed and rotated by 180 degrees.
__global__ void __launch_bounds__(kBlock)
wgs_weights_kernel(const float* __restrict__ w, __bf16* __restrict__ U, int K, int C, int Cp, int mode) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= static_cast<int64_t>(K) * Cp) return;
    const int k = static_cast<int>(e / Cp), c = static_cast<int>(e - static_cast<int64_t>(k) * Cp);
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            float v = 0.f;
            if (c < C) v = mode == 0 ? w[(static_cast<size_t>(k) * C + c) * 9 + r * 3 + s]
                                     : w[(static_cast<size_t>(c) * K + k) * 9 + (2 - r) * 3 + (2 - s)];
            g[r][s] = v;
        }
    float t[4][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        t[0][s] = g[0][s];
        t[1][s] = 0.5f * (g[0][s] + g[1][s] + g[2][s]);
        t[2][s] = 0.5f * (g[0][s] - g[1][s] + g[2][s]);
        t[3][s] = g[2][s];
    }
    const size_t pstride = static_cast<size_t>(Cp / 8) * 2 * K * 8;          // bf16 per position
    const size_t lo_off = static_cast<size_t>(K) * 8;
    __bf16* dst = U + (static_cast<size_t>(c >> 3) * 2 * K + k) * 8 + (c & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float u[4] = {t[i][0], 0.5f * (t[i][0] + t[i][1] + t[i][2]), 0.5f * (t[i][0] - t[i][1] + t[i][2]), t[i][2]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __bf16 h, l;
            wgs_split(u[j], h, l);
            dst[(i * 4 + j) * pstride] = h;
            dst[(i * 4 + j) * pstride + lo_off] = l;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- input transform
// One thread = one tile x eight channels (blockIdx.y = the channel group): per channel 16 bounds-checked loads (the zero padding, odd
// H / W, the tile tail and the channel tail all read 0) and Bt d B as wg_input_transform_kernel has it; the 16 entries are split and
// packed, and the thread stores one hi and one lo line per position, lanes along the tiles.  MASK: mask is a tensor of x's shape and
// x is taken as `mask <= 0 ? 0 : x` (aten::threshold_backward(x, mask, 0): a NaN in the mask lets the value pass, a masked-out
// infinity is a zero), read with x's own index: both loads run along the tiles as x's does.
template <bool MASK>
__global__ void __launch_bounds__(kBlock)
wgs_input_transform_kernel(const float* __restrict__ x, const float* __restrict__ mask, bf16x8* __restrict__ V, const WgGeo g) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.Tp) return;
    const int c8 = blockIdx.y;
    const bool tv = t < g.T;
    const int per = g.TH * g.TW;
    const int b = tv ? t / per : 0;
    const int rem = tv ? t - b * per : 0;
    const int ty = rem / g.TW, tx = rem - ty * g.TW;
    const size_t HW = static_cast<size_t>(g.H) * g.W;
    bf16x8 vh[16], vl[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c8 * 8 + j;
        const bool cv = tv && c < g.C;
        const size_t plane = (static_cast<size_t>(b) * g.C + (cv ? c : 0)) * HW;
        float d[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int iy = 2 * ty - 1 + i, ix = 2 * tx - 1 + q;
                float e = 0.f;
                if (cv && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) {
                    const size_t o = plane + static_cast<size_t>(iy) * g.W + ix;
                    e = x[o];
                    if (MASK) e = mask[o] <= 0.f ? 0.f : e;
                }
                d[i * 4 + q] = e;
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // row i of Bt d: (d0 - d2, d1 + d2, d2 - d1, d1 - d3), then the same along the columns
            float r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                r[q] = i == 0 ? d[0 + q] - d[8 + q] : i == 1 ? d[4 + q] + d[8 + q] : i == 2 ? d[8 + q] - d[4 + q] : d[4 + q] - d[12 + q];
            const float v[4] = {r[0] - r[2], r[1] + r[2], r[2] - r[1], r[1] - r[3]};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __bf16 h, l;
                wgs_split(v[q], h, l);
                vh[i * 4 + q][j] = h;
                vl[i * 4 + q][j] = l;
            }
        }
    }
    const size_t pstride = static_cast<size_t>(g.C4) * g.Tp;          // 16-byte lines per position: Cp / 8 groups x (hi, lo) x Tp
    bf16x8* dst = V + static_cast<size_t>(c8) * 2 * g.Tp + t;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        dst[p * pstride] = vh[p];
        dst[p * pstride + g.Tp] = vl[p];
    }
}

// ---------------------------------------------------------------------------------------------------- 16 GEMMs
// The workgroup and wave tiling of wg_batched_gemm_kernel: 4 waves, 2 x 2, own a TILE x TILE block of M_p, a wave NB x NB accumulators
// of 32 x 32.  A stage is 32 input channels: [4 channel groups][hi, lo][TILE rows] 16-byte lines per operand, copied global ->
// registers -> LDS by all 256 threads (TILE / 32 lines per thread and operand), double buffered: the loads of stage n + 1 are in
// flight while the MFMAs of stage n issue, one barrier per stage.  One MFMA takes 16 channels: lanes 0-31 the even group's line,
// lanes 32-63 the odd group's.  Per 16 channels and 32 x 32 block: lo hi, hi lo, hi hi, in that order, into one accumulator.
// Consecutive lanes read / write consecutive 16-byte lines: no LDS bank conflict.  Rows of U past K are zero filled in LDS; V and M are
// padded to the tile, so nothing else needs a bounds check.  blockIdx: the tile column fastest, then the k tile, then the position.
template <int TILE>
__global__ void __launch_bounds__(kBlock)
wgs_batched_gemm_kernel(const f32x4* __restrict__ U, const f32x4* __restrict__ V, float* __restrict__ M, int K, int L, int Tp, int Kp,
                        int KT, int TTn) {
    constexpr int WT = TILE / 2, NB = WT / 32, NL = TILE / 32;
    __shared__ f32x4 As[2][8][TILE];
    __shared__ f32x4 Bs[2][8][TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    unsigned bid = blockIdx.x;
    const int tt = static_cast<int>(bid % static_cast<unsigned>(TTn));
    bid /= static_cast<unsigned>(TTn);
    const int kt = static_cast<int>(bid % static_cast<unsigned>(KT));
    const int p = static_cast<int>(bid / static_cast<unsigned>(KT));
    const int k0 = kt * TILE, t0 = tt * TILE;
    const f32x4* Up = U + static_cast<size_t>(p) * L * K;              // L = Cp / 4 lines per row and position
    const f32x4* Vp = V + static_cast<size_t>(p) * L * Tp;

    f32x4 ra[NL], rb[NL];
    auto gload = [&](int stage) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = threadIdx.x + kBlock * i;
            const int line = stage * 8 + idx / TILE, n = idx % TILE;
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (k0 + n < K) a = Up[static_cast<size_t>(line) * K + k0 + n];
            ra[i] = a;
            rb[i] = Vp[static_cast<size_t>(line) * Tp + t0 + n];
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = threadIdx.x + kBlock * i;
            As[buf][idx / TILE][idx % TILE] = ra[i];
            Bs[buf][idx / TILE][idx % TILE] = rb[i];
        }
    };

    f32x16 acc[NB][NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int stages = L / 8;
    gload(0);
    sstore(0);
    __syncthreads();
    int buf = 0;
    for (int st = 0; st < stages; ++st) {
        const bool more = st + 1 < stages;
        if (more) gload(st + 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 ah[NB], al[NB], bh[NB], bl[NB];
            const int line = (2 * s + half) * 2;
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                ah[i] = __builtin_bit_cast(bf16x8, As[buf][line][wm * WT + i * 32 + l31]);
                al[i] = __builtin_bit_cast(bf16x8, As[buf][line + 1][wm * WT + i * 32 + l31]);
                bh[i] = __builtin_bit_cast(bf16x8, Bs[buf][line][wn * WT + i * 32 + l31]);
                bl[i] = __builtin_bit_cast(bf16x8, Bs[buf][line + 1][wn * WT + i * 32 + l31]);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
        if (more) sstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // C/D layout: column = lane & 31 (tile), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel)
    float* Mp = M + (static_cast<size_t>(p) * Kp + k0 + wm * WT) * Tp + t0 + wn * WT + l31;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                Mp[static_cast<size_t>(row) * Tp + j * 32] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------------------------------------------- output transform
// One thread = one tile x one output channel (blockIdx.y): y = At (M A) + bias by wg_tile_of, LeakyReLU, the 2 x 2 store.
__global__ void __launch_bounds__(kBlock)
wgs_output_transform_kernel(const float* __restrict__ M, const float* __restrict__ bias, float* __restrict__ out, const WgGeo g, int epi,
                            float slope, int vec) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.T) return;
    const int ko = blockIdx.y;
    const size_t pstride = static_cast<size_t>(g.Kp) * g.Tp;
    const bool use_bias = bias != nullptr && epi != kWgsNone;
    float y[4];
    wg_tile_of(M + static_cast<size_t>(ko) * g.Tp + t, pstride, use_bias ? bias[ko] : 0.f, y);
    if (epi == kWgsBiasLrelu) {
#pragma unroll
        for (int v = 0; v < 4; ++v) y[v] = y[v] > 0.f ? y[v] : y[v] * slope;
    }
    wg_store_tile(out, g, t, ko, g.K, y, vec);
}

// The output transform of the loss networks: the epilogues of wg_output_transform_kernel (conv_winograd_gemm.hip).  One thread = one
// tile x one output channel; under the max-feature-map epilogue two rows of M, k and k + K / 2, both read with the lanes along the tiles.
__global__ void __launch_bounds__(kBlock)
wgs_output_apply_kernel(const float* __restrict__ M, const float* __restrict__ bias, float* __restrict__ out, const WgGeo g, int epi,
                        int vec) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.T) return;
    const int ko = blockIdx.y;
    const int Kout = epi == FFWM_WG_BIAS_MFM ? g.K / 2 : g.K;
    const size_t pstride = static_cast<size_t>(g.Kp) * g.Tp;
    const bool use_bias = bias != nullptr && epi != FFWM_WG_NONE;
    float y[4];
    wg_tile_of(M + static_cast<size_t>(ko) * g.Tp + t, pstride, use_bias ? bias[ko] : 0.f, y);
    if (epi == FFWM_WG_BIAS_RELU) {
#pragma unroll
        for (int v = 0; v < 4; ++v) y[v] = wg_relu_nan(y[v]);
    } else if (epi == FFWM_WG_BIAS_MFM) {
        float y2[4];
        wg_tile_of(M + static_cast<size_t>(ko + Kout) * g.Tp + t, pstride, use_bias ? bias[ko + Kout] : 0.f, y2);
#pragma unroll
        for (int v = 0; v < 4; ++v) y[v] = wg_max_nan(y[v], y2[v]);
    }
    wg_store_tile(out, g, t, ko, Kout, y, vec);
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

// The route of one call, decided once: the workspace query and the three launches read this plan.
struct WgsPlan {
    int tile;                // GEMM tile: 64 or 128
    int64_t T, Tp, Kp, Cp;
    int64_t KT, TTn;         // tiles of output channels / of Winograd tiles
    int64_t v_bytes, m_floats;
};
static WgsPlan wgs_plan(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int force_tile) {
    WgsPlan p;
    p.T = B * ((H + 1) / 2) * ((W + 1) / 2);
    p.Cp = wg_round_up(C, kWgsStage);
    // the plan rule of the fp32 route: the 128 x 128 tile when it still gives every compute unit a workgroup, else 64 x 64
    const int64_t n128 = 16 * ((K + 127) / 128) * ((p.T + 127) / 128);
    p.tile = force_tile ? force_tile : (n128 >= device_cus() ? 128 : 64);
    p.Tp = wg_round_up(p.T, p.tile);
    p.Kp = wg_round_up(K, p.tile);
    p.KT = p.Kp / p.tile;
    p.TTn = p.Tp / p.tile;
    p.v_bytes = 16 * p.Cp * p.Tp * 4;          // a hi and a lo bf16 per entry
    p.m_floats = 16 * p.Kp * p.Tp;
    return p;
}

extern "C" int64_t ffwm_conv3x3_wg_split_weights_bytes(int64_t K, int64_t C) {
    if (K <= 0 || C <= 0) return 0;
    return 16 * wg_round_up(C, kWgsStage) * K * 4;
}

extern "C" int64_t ffwm_conv3x3_wg_split_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    // V and M of the larger tile's padding: enough for either plan
    const int64_t T = wg_round_up(B * ((H + 1) / 2) * ((W + 1) / 2), 128);
    return 16 * T * (wg_round_up(C, kWgsStage) + wg_round_up(K, 128)) * 4;
}

// weight -> the split U of one direction.  K / C in the GEMM's terms: U has K rows and reduces over C.
static int wgs_weights_call(const char* fn, const void* weight, void* U, int64_t K, int64_t C, int mode, int dtype, void* stream) {
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only (split into bf16 terms for the bf16 MFMA)", fn);
    FFWM_REQUIRE(weight && U, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(K > 0 && C > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(U) % 16 == 0, FFWM_ERR_ARG, "%s: U must be 16-byte aligned", fn);
    const int64_t Cp = wg_round_up(C, kWgsStage);
    FFWM_REQUIRE(K * Cp < (1LL << 31) - kBlock && K * C * 9 < (1LL << 31), FFWM_ERR_SIZE, "%s: weight beyond 2^31 elements", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LaunchScope ls("conv_wgs_weights", st, 4.0 * (9.0 * K * C + 16.0 * K * Cp));
    hipLaunchKernelGGL(wgs_weights_kernel, dim3(static_cast<unsigned>((K * Cp + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       static_cast<const float*>(weight), static_cast<__bf16*>(U), static_cast<int>(K), static_cast<int>(C),
                       static_cast<int>(Cp), mode);
    return check_launch(fn);
}

extern "C" int ffwm_conv3x3_wg_split_weights(const void* weight, void* U, int64_t K, int64_t C, int dtype, void* stream) {
    return wgs_weights_call("ffwm_conv3x3_wg_split_weights", weight, U, K, C, 0, dtype, stream);
}

extern "C" int ffwm_conv3x3_wg_split_weights_dgrad(const void* weight, void* U, int64_t K, int64_t C, int dtype, void* stream) {
    // the data gradient of a Conv2d(C, K) is a convolution with C output rows that reduces over K
    return wgs_weights_call("ffwm_conv3x3_wg_split_weights_dgrad", weight, U, C, K, 1, dtype, stream);
}

extern "C" int ffwm_conv3x3_wg_split_tile(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    return wgs_plan(B, C, H, W, K, 0).tile;
}

// What the two entry points share: the checks that do not depend on the epilogue's code, then the three launches.  apply: the
// epilogue codes of the fp32 route (FFWM_WG_*) and the ReLU mask; else FFWM_WGS_* with its LeakyReLU slope.
static int wgs_call(const char* fn, bool apply, const void* input, const void* U, const void* bias, void* output, void* workspace,
                    int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epi, double negative_slope, const void* relu_mask,
                    int tile, void* stream) {
    FFWM_REQUIRE(tile == 0 || tile == 64 || tile == 128, FFWM_ERR_ARG, "%s: tile must be 0 (the plan's), 64 or 128", fn);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(U) % 16 == 0, FFWM_ERR_ARG,
                 "%s: U and the workspace must be 16-byte aligned", fn);
    FFWM_REQUIRE(B * C * H * W < (1LL << 31) && B * K * H * W < (1LL << 31), FFWM_ERR_SIZE, "%s: a tensor beyond 2^31 elements", fn);
    const WgsPlan p = wgs_plan(B, C, H, W, K, tile);
    const int64_t Kout = apply && epi == FFWM_WG_BIAS_MFM ? K / 2 : K;
    FFWM_REQUIRE(p.Tp < (1LL << 30) && p.Cp / 8 <= 65535 && Kout <= 65535 && 16 * p.KT * p.TTn < (1LL << 31), FFWM_ERR_SIZE,
                 "%s: too many tiles or channels", fn);
    WgGeo g;
    g.C = static_cast<int>(C); g.C4 = static_cast<int>(p.Cp / 4);
    g.H = static_cast<int>(H); g.W = static_cast<int>(W); g.K = static_cast<int>(K);
    g.TH = static_cast<int>((H + 1) / 2); g.TW = static_cast<int>((W + 1) / 2); g.T = static_cast<int>(p.T);
    g.Tp = static_cast<int>(p.Tp); g.Kp = static_cast<int>(p.Kp);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* V = static_cast<char*>(workspace);
    float* M = reinterpret_cast<float*>(V + p.v_bytes);
    const double act = static_cast<double>(B) * H * W;
    {
        LaunchScope ls("conv_wgs_in", st, 4.0 * act * C * (relu_mask ? 2.0 : 1.0) + static_cast<double>(p.v_bytes));
        const dim3 grid(static_cast<unsigned>((p.Tp + kBlock - 1) / kBlock), static_cast<unsigned>(p.Cp / 8));
        if (relu_mask)
            hipLaunchKernelGGL(wgs_input_transform_kernel<true>, grid, dim3(kBlock), 0, st, static_cast<const float*>(input),
                               static_cast<const float*>(relu_mask), reinterpret_cast<bf16x8*>(V), g);
        else
            hipLaunchKernelGGL(wgs_input_transform_kernel<false>, grid, dim3(kBlock), 0, st, static_cast<const float*>(input),
                               static_cast<const float*>(nullptr), reinterpret_cast<bf16x8*>(V), g);
    }
    if (int rc = check_launch(fn)) return rc;
    {
        // flops = the multiplications the RESULT needs (16 per tile and channel pair): not those of the padding, not three times that
        LaunchScope ls("conv_wgs_gemm", st, 4.0 * 16.0 * K * p.Cp + static_cast<double>(p.v_bytes) + 4.0 * static_cast<double>(p.m_floats),
                       2.0 * 16.0 * static_cast<double>(p.T) * K * C);
        const unsigned grid = static_cast<unsigned>(16 * p.KT * p.TTn);
        const bool ok = dispatch<64, 128>(p.tile, [&](auto TILE) {
            hipLaunchKernelGGL(wgs_batched_gemm_kernel<TILE.value>, dim3(grid), dim3(kBlock), 0, st, static_cast<const f32x4*>(U),
                               reinterpret_cast<const f32x4*>(V), M, g.K, g.C4, g.Tp, g.Kp, static_cast<int>(p.KT), static_cast<int>(p.TTn));
        });
        if (!ok) return no_kernel(fn);
    }
    if (int rc = check_launch(fn)) return rc;
    {
        LaunchScope ls("conv_wgs_out", st, 4.0 * (16.0 * K * p.T + act * Kout));
        const int vec = W % 2 == 0 && reinterpret_cast<uintptr_t>(output) % 8 == 0;
        const dim3 grid(static_cast<unsigned>((p.T + kBlock - 1) / kBlock), static_cast<unsigned>(Kout));
        if (apply)
            hipLaunchKernelGGL(wgs_output_apply_kernel, grid, dim3(kBlock), 0, st, M, static_cast<const float*>(bias),
                               static_cast<float*>(output), g, epi, vec);
        else
            hipLaunchKernelGGL(wgs_output_transform_kernel, grid, dim3(kBlock), 0, st, M, static_cast<const float*>(bias),
                               static_cast<float*>(output), g, epi, static_cast<float>(negative_slope), vec);
    }
    return check_launch(fn);
}

extern "C" int ffwm_conv3x3_wg_split_forward(const void* input, const void* U, const void* bias, void* output, void* workspace,
                                             int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, double negative_slope,
                                             int tile, int dtype, void* stream) {
    const char* fn = "ffwm_conv3x3_wg_split_forward";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only (split into bf16 terms for the bf16 MFMA)", fn);
    FFWM_REQUIRE(input && U && output && workspace, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && K > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    const int epi = epilogue;
    FFWM_REQUIRE(epi >= kWgsNone && epi <= kWgsBiasLrelu, FFWM_ERR_ARG,
                 "%s: epilogue must be 0 (none), 1 (bias) or 2 (bias, LeakyReLU)", fn);
    FFWM_REQUIRE(epi == kWgsNone || bias, FFWM_ERR_ARG, "%s: the bias epilogues need a bias", fn);
    return wgs_call(fn, false, input, U, bias, output, workspace, B, C, H, W, K, epi, negative_slope, nullptr, tile, stream);
}

extern "C" int ffwm_conv3x3_wg_split_apply(const void* input, const void* U, const void* bias, void* output, void* workspace,
                                           int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, const void* relu_mask,
                                           int tile, int dtype, void* stream) {
    const char* fn = "ffwm_conv3x3_wg_split_apply";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only (split into bf16 terms for the bf16 MFMA)", fn);
    FFWM_REQUIRE(input && U && output && workspace, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && K > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    const int epi = epilogue;
    FFWM_REQUIRE(epi >= FFWM_WG_NONE && epi <= FFWM_WG_BIAS_MFM, FFWM_ERR_ARG,
                 "%s: epilogue must be 0 (none), 1 (bias), 2 (bias, relu) or 3 (bias, max-feature-map)", fn);
    FFWM_REQUIRE(epi == FFWM_WG_NONE || bias, FFWM_ERR_ARG, "%s: the bias epilogues need a bias", fn);
    FFWM_REQUIRE(epi != FFWM_WG_BIAS_MFM || K % 2 == 0, FFWM_ERR_ARG, "%s: the max-feature-map epilogue needs an even K", fn);
    return wgs_call(fn, true, input, U, bias, output, workspace, B, C, H, W, K, epi, 0.0, relu_mask, tile, stream);
}
