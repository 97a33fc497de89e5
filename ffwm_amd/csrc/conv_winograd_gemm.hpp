// conv_winograd_gemm.hpp -- what the two batched-GEMM Winograd routes share (conv_winograd_gemm.hip: fp32 MFMA;
// conv_winograd_gemm_split.hip: bf16 MFMA on hi / lo operand halves): the geometry of a call, the accumulator types, the output
// transform of one tile and the rounding helper of the plans.  M [16][Kp][Tp] fp32 has the same layout in both routes.
#pragma once
#include "common.hpp"

namespace ffwm {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WgGeo {
    int C, C4;               // input channels; 16-byte lines per operand row (fp32 route: groups of four channels of the padded Cp;
                             // split route: groups of eight channels, a hi and a lo line each -- Cp / 4 in both)
    int H, W, K;
    int TH, TW, T;           // 2 x 2 output tiles per column / row / in total (B TH TW)
    int Tp, Kp;              // T and K rounded up to the GEMM tile
};

// ATen's NaN rule, as csrc/mfm.hip has it: maximum(a, b) is NaN when either operand is, relu(NaN) is NaN
__device__ __forceinline__ float wg_max_nan(float a, float b) { return __builtin_isunordered(a, b) ? a + b : fmaxf(a, b); }
__device__ __forceinline__ float wg_relu_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// y = At (M A) of one tile and output channel, + bv: M points at position 0, the positions are pstride floats apart
__device__ __forceinline__ void wg_tile_of(const float* __restrict__ M, size_t pstride, float bv, float (&y)[4]) {
    float z[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float m0 = M[(i * 4 + 0) * pstride], m1 = M[(i * 4 + 1) * pstride], m2 = M[(i * 4 + 2) * pstride], m3 = M[(i * 4 + 3) * pstride];
        z[i][0] = (m0 + m1) + m2;
        z[i][1] = (m1 - m2) - m3;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        y[j] = ((z[0][j] + z[1][j]) + z[2][j]) + bv;
        y[2 + j] = ((z[1][j] - z[2][j]) - z[3][j]) + bv;
    }
}

// the 2 x 2 store of one tile (odd H / W: the pixels that exist); vec: W even and an 8-byte aligned output
__device__ __forceinline__ void wg_store_tile(float* __restrict__ out, const WgGeo& g, int t, int ko, int Kout, const float (&y)[4], int vec) {
    const int per = g.TH * g.TW;
    const int b = t / per, rem = t - b * per;
    const int ty = rem / g.TW, tx = rem - ty * g.TW;
    const int oy = 2 * ty, ox = 2 * tx;
    const bool row1 = oy + 1 < g.H, col1 = ox + 1 < g.W;
    float* o = out + ((static_cast<size_t>(b) * Kout + ko) * g.H + oy) * g.W + ox;
    if (vec) {               // W even, 8-byte aligned output: every tile has both columns
        *reinterpret_cast<float2*>(o) = make_float2(y[0], y[1]);
        if (row1) *reinterpret_cast<float2*>(o + g.W) = make_float2(y[2], y[3]);
    } else {
        o[0] = y[0];
        if (col1) o[1] = y[1];
        if (row1) {
            o[g.W] = y[2];
            if (col1) o[g.W + 1] = y[3];
        }
    }
}

inline int64_t wg_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

}  // namespace
}  // namespace ffwm
