// conv_winograd_gemm.hip -- fp32 Winograd F(2x2, 3x3) in its classic three-launch form, for the FROZEN 3x3 / stride 1 / pad 1
// layers of the loss networks on small planes (VGG19 from relu3 on, LightCNN's 32 x 32 and 16 x 16 stages: models/losses.py:398-519,
// lightcnn/light_cnn.py:59-112).
//
// conv_winograd.hip gives a workgroup 64 channels x 64 tiles for ALL 16 Winograd positions; 512 -> 512 at 16 x 16, batch 8 is then 64
// work units for 256 CUs.  Here the 16 positions are 16 independent GEMMs, which is 16 times the parallelism:
//
//   wg_input_transform   x [B, C, H, W]  ->  V [16][Cp / 4][Tp][4]     V = Bt d B per tile t = (b, ty, tx) and channel
//   wg_batched_gemm      M_p [Kp x Tp] = U_p [K x Cp] V_p [Cp x Tp]    p = 0 .. 15, v_mfma_f32_32x32x2_f32
//   wg_output_transform  M [16][Kp][Tp]  ->  y [B, K, H, W]            y = At M A, then the epilogue (bias, ReLU, max-feature-map)
//
// U = G w Gt [16][Cp / 4][K][4] is made ONCE per layer and direction (wg_weights): the weights are frozen.  U and V keep four
// consecutive input channels of one row / tile side by side, so a GEMM workgroup copies both operands global -> LDS as straight
// 16-byte lines and a lane's ds_read_b128 feeds four MFMAs.  Cp = C rounded up to 16 (one LDS stage), zero filled on both sides;
// Tp / Kp = T / K rounded up to the GEMM tile.  A column of M depends on the same column of V alone, so the columns past T hold
// zeros that nobody reads.  V and M are 4-17 MB on these planes and stay in L2 / MALL between the launches; on large planes they
// are 4 x the activations and conv_winograd.hip's fused form wins.
//
// No atomics, no split of the reduction: one fma chain over C per M entry, bit-reproducible.  The roundings per entry are those of
// conv_winograd.hip (two in V, four in U, the chain, four in the output transform): tests/conv_bounds.py rho_winograd, splits = 1.
#include "conv_winograd_gemm.hpp"

namespace ffwm {
namespace {

enum { kWgNone = FFWM_WG_NONE, kWgBias = FFWM_WG_BIAS, kWgBiasRelu = FFWM_WG_BIAS_RELU, kWgBiasMfm = FFWM_WG_BIAS_MFM };
constexpr int kWgStage = 16;             // input channels per LDS stage of the GEMM: four groups of four

// ---------------------------------------------------------------------------------------------------- weights
// U[p][c / 4][k][c % 4] = (G w Gt)[p] of output channel k and input channel c; zero for C <= c < Cp.  mode 0: w is [K][C][3][3];
// mode 1 (data gradient): w is the layer's own [C][K][3][3], read transposed and rotated by 180 degrees.
__global__ void __launch_bounds__(kBlock)
wg_weights_kernel(const float* __restrict__ w, float* __restrict__ U, int K, int C, int Cp, int mode) {
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
    // rows: G g  (G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]), then the same along the columns
    float t[4][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        t[0][s] = g[0][s];
        t[1][s] = 0.5f * (g[0][s] + g[1][s] + g[2][s]);
        t[2][s] = 0.5f * (g[0][s] - g[1][s] + g[2][s]);
        t[3][s] = g[2][s];
    }
    const size_t pstride = static_cast<size_t>(Cp / 4) * K * 4;
    float* dst = U + (static_cast<size_t>(c >> 2) * K + k) * 4 + (c & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dst[(i * 4 + 0) * pstride] = t[i][0];
        dst[(i * 4 + 1) * pstride] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);
        dst[(i * 4 + 2) * pstride] = 0.5f * (t[i][0] - t[i][1] + t[i][2]);
        dst[(i * 4 + 3) * pstride] = t[i][2];
    }
}

// ---------------------------------------------------------------------------------------------------- input transform
// One thread = one tile x four channels (blockIdx.y = the channel group): 64 bounds-checked loads (the zero padding, odd H / W, the
// tile tail and the channel tail all read 0), 16 float4 stores, lanes along the tiles.  mask (or NULL): a tensor of x's shape,
// x is taken as `mask <= 0 ? 0 : x` -- aten::threshold_backward(x, mask, 0), the gradient through a ReLU whose OUTPUT is mask.
__global__ void __launch_bounds__(kBlock)
wg_input_transform_kernel(const float* __restrict__ x, const float* __restrict__ mask, float* __restrict__ V, const WgGeo g) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.Tp) return;
    const int c4 = blockIdx.y;
    const bool tv = t < g.T;
    const int per = g.TH * g.TW;
    const int b = tv ? t / per : 0;
    const int rem = tv ? t - b * per : 0;
    const int ty = rem / g.TW, tx = rem - ty * g.TW;
    const size_t HW = static_cast<size_t>(g.H) * g.W;
    f32x4 v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c4 * 4 + j;
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
                    if (mask != nullptr) e = mask[o] <= 0.f ? 0.f : e;
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
            v[i * 4 + 0][j] = r[0] - r[2];
            v[i * 4 + 1][j] = r[1] + r[2];
            v[i * 4 + 2][j] = r[2] - r[1];
            v[i * 4 + 3][j] = r[1] - r[3];
        }
    }
    const size_t pstride = static_cast<size_t>(g.C4) * g.Tp;          // float4 units
    f32x4* dst = reinterpret_cast<f32x4*>(V) + static_cast<size_t>(c4) * g.Tp + t;
#pragma unroll
    for (int p = 0; p < 16; ++p) dst[p * pstride] = v[p];
}

// ---------------------------------------------------------------------------------------------------- 16 GEMMs
// A workgroup (4 waves, 2 x 2) owns a TILE x TILE block of M_p; a wave TILE / 2 x TILE / 2 = NB x NB accumulators of 32 x 32.
// A stage is 16 input channels: [4 channel groups][TILE rows][4 channels] per operand, one 16-byte line per row and group, copied
// global -> registers -> LDS by all 256 threads (TILE / 64 lines per thread and operand), double buffered: the loads of stage
// n + 1 are in flight while the MFMAs of stage n issue, one barrier per stage.
// An MFMA takes A[k][c] and B[c][t] for TWO channels: lanes 0-31 feed channel j of the even group, lanes 32-63 channel j of the odd
// group, so ONE ds_read_b128 per 32 rows feeds four MFMAs.  128 x 128: 4 reads for 16 MFMAs; 64 x 64: 2 reads for 4 MFMAs.
// Consecutive lanes read / write consecutive 16-byte lines: no LDS bank conflict.  Rows of U past K are zero filled in LDS; V and M
// are padded to the tile, so nothing else needs a bounds check.  blockIdx: the tile column fastest, then the k tile, then the position
// -- the workgroups that run together share their U rows and V columns in L2.
template <int TILE>
__global__ void __launch_bounds__(kBlock)
wg_batched_gemm_kernel(const float* __restrict__ U, const float* __restrict__ V, float* __restrict__ M, int K, int C4, int Tp, int Kp,
                       int KT, int TTn) {
    constexpr int WT = TILE / 2, NB = WT / 32, NL = TILE / 64;
    __shared__ f32x4 As[2][4][TILE];
    __shared__ f32x4 Bs[2][4][TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    unsigned bid = blockIdx.x;
    const int tt = static_cast<int>(bid % static_cast<unsigned>(TTn));
    bid /= static_cast<unsigned>(TTn);
    const int kt = static_cast<int>(bid % static_cast<unsigned>(KT));
    const int p = static_cast<int>(bid / static_cast<unsigned>(KT));
    const int k0 = kt * TILE, t0 = tt * TILE;
    const f32x4* Up = reinterpret_cast<const f32x4*>(U) + static_cast<size_t>(p) * C4 * K;
    const f32x4* Vp = reinterpret_cast<const f32x4*>(V) + static_cast<size_t>(p) * C4 * Tp;

    f32x4 ra[NL], rb[NL];
    auto gload = [&](int stage) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = threadIdx.x + kBlock * i;
            const int grp = stage * 4 + idx / TILE, n = idx % TILE;
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (k0 + n < K) a = Up[static_cast<size_t>(grp) * K + k0 + n];
            ra[i] = a;
            rb[i] = Vp[static_cast<size_t>(grp) * Tp + t0 + n];
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

    const int stages = C4 / 4;
    gload(0);
    sstore(0);
    __syncthreads();
    int buf = 0;
    for (int st = 0; st < stages; ++st) {
        const bool more = st + 1 < stages;
        if (more) gload(st + 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f32x4 a[NB], b[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                a[i] = As[buf][2 * s + half][wm * WT + i * 32 + l31];
                b[i] = Bs[buf][2 * s + half][wn * WT + i * 32 + l31];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < NB; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[j][q], acc[i][j], 0, 0, 0);
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
// One thread = one tile x one output channel (blockIdx.y; two channels, k and k + K / 2, under the max-feature-map epilogue): 16
// loads per channel with the lanes along the tiles, y = At (M A), the epilogue, a 2 x 2 store (odd H / W: the pixels that exist).
__global__ void __launch_bounds__(kBlock)
wg_output_transform_kernel(const float* __restrict__ M, const float* __restrict__ bias, float* __restrict__ out, const WgGeo g, int epi,
                           int vec) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.T) return;
    const int ko = blockIdx.y;
    const int Kout = epi == kWgBiasMfm ? g.K / 2 : g.K;
    const size_t pstride = static_cast<size_t>(g.Kp) * g.Tp;
    const bool use_bias = bias != nullptr && epi != kWgNone;
    float y[4];
    wg_tile_of(M + static_cast<size_t>(ko) * g.Tp + t, pstride, use_bias ? bias[ko] : 0.f, y);
    if (epi == kWgBiasRelu) {
#pragma unroll
        for (int v = 0; v < 4; ++v) y[v] = wg_relu_nan(y[v]);
    } else if (epi == kWgBiasMfm) {
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
struct WgPlan {
    int tile;                // GEMM tile: 64 or 128
    int64_t T, Tp, Kp, Cp;
    int64_t KT, TTn;         // tiles of output channels / of Winograd tiles
    int64_t v_floats, m_floats;
};
static WgPlan wg_plan(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int force_tile) {
    WgPlan p;
    p.T = B * ((H + 1) / 2) * ((W + 1) / 2);
    p.Cp = wg_round_up(C, kWgStage);
    // the 128 x 128 tile (4 LDS reads per 16 MFMAs) when it still gives every compute unit a workgroup, else 64 x 64 (4 x the workgroups)
    const int64_t n128 = 16 * ((K + 127) / 128) * ((p.T + 127) / 128);
    p.tile = force_tile ? force_tile : (n128 >= device_cus() ? 128 : 64);
    p.Tp = wg_round_up(p.T, p.tile);
    p.Kp = wg_round_up(K, p.tile);
    p.KT = p.Kp / p.tile;
    p.TTn = p.Tp / p.tile;
    p.v_floats = 16 * p.Cp * p.Tp;
    p.m_floats = 16 * p.Kp * p.Tp;
    return p;
}

extern "C" int64_t ffwm_conv3x3_wg_weights_bytes(int64_t K, int64_t C) {
    if (K <= 0 || C <= 0) return 0;
    return 16 * wg_round_up(C, kWgStage) * K * 4;
}

extern "C" int64_t ffwm_conv3x3_wg_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    // V and M of the larger tile's padding: enough for either plan
    const int64_t T = wg_round_up(B * ((H + 1) / 2) * ((W + 1) / 2), 128);
    return 16 * T * (wg_round_up(C, kWgStage) + wg_round_up(K, 128)) * 4;
}

extern "C" int ffwm_conv3x3_wg_weights(const void* weight, void* U, int64_t K, int64_t C, int data_gradient, int dtype, void* stream) {
    const char* fn = "ffwm_conv3x3_wg_weights";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(weight && U, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(K > 0 && C > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(data_gradient == 0 || data_gradient == 1, FFWM_ERR_ARG, "%s: data_gradient must be 0 or 1", fn);
    const int64_t Cp = wg_round_up(C, kWgStage);
    FFWM_REQUIRE(K * Cp < (1LL << 31) - kBlock && K * C * 9 < (1LL << 31), FFWM_ERR_SIZE, "%s: weight beyond 2^31 elements", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LaunchScope ls("conv_wg_weights", st, 4.0 * (9.0 * K * C + 16.0 * K * Cp));
    hipLaunchKernelGGL(wg_weights_kernel, dim3(static_cast<unsigned>((K * Cp + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       static_cast<const float*>(weight), static_cast<float*>(U), static_cast<int>(K), static_cast<int>(C),
                       static_cast<int>(Cp), data_gradient);
    return check_launch(fn);
}

extern "C" int ffwm_conv3x3_wg_tile(int64_t B, int64_t C, int64_t H, int64_t W, int64_t K) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    return wg_plan(B, C, H, W, K, 0).tile;
}

extern "C" int ffwm_conv3x3_wg_forward(const void* input, const void* U, const void* bias, void* output, void* workspace,
                                       int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, const void* relu_mask,
                                       int dtype, void* stream) {
    return ffwm_conv3x3_wg_forward_tiled(input, U, bias, output, workspace, B, C, H, W, K, epilogue, relu_mask, 0, dtype, stream);
}

extern "C" int ffwm_conv3x3_wg_forward_tiled(const void* input, const void* U, const void* bias, void* output, void* workspace,
                                             int64_t B, int64_t C, int64_t H, int64_t W, int64_t K, int epilogue, const void* relu_mask,
                                             int tile, int dtype, void* stream) {
    const char* fn = "ffwm_conv3x3_wg_forward";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(input && U && output && workspace, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && K > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    const int epi = epilogue;
    FFWM_REQUIRE(epi >= kWgNone && epi <= kWgBiasMfm, FFWM_ERR_ARG,
                 "%s: epilogue must be 0 (none), 1 (bias), 2 (bias, relu) or 3 (bias, max-feature-map)", fn);
    FFWM_REQUIRE(tile == 0 || tile == 64 || tile == 128, FFWM_ERR_ARG, "%s: tile must be 0 (the plan's), 64 or 128", fn);
    FFWM_REQUIRE(epi != kWgBiasMfm || K % 2 == 0, FFWM_ERR_ARG, "%s: the max-feature-map epilogue needs an even K", fn);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(U) % 16 == 0, FFWM_ERR_ARG,
                 "%s: U and the workspace must be 16-byte aligned", fn);
    FFWM_REQUIRE(B * C * H * W < (1LL << 31) && B * K * H * W < (1LL << 31), FFWM_ERR_SIZE, "%s: a tensor beyond 2^31 elements", fn);
    const WgPlan p = wg_plan(B, C, H, W, K, tile);
    const int64_t Kout = epi == kWgBiasMfm ? K / 2 : K;
    FFWM_REQUIRE(p.Tp < (1LL << 30) && p.Cp / 4 <= 65535 && Kout <= 65535 && 16 * p.KT * p.TTn < (1LL << 31), FFWM_ERR_SIZE,
                 "%s: too many tiles or channels", fn);
    WgGeo g;
    g.C = static_cast<int>(C); g.C4 = static_cast<int>(p.Cp / 4);
    g.H = static_cast<int>(H); g.W = static_cast<int>(W); g.K = static_cast<int>(K);
    g.TH = static_cast<int>((H + 1) / 2); g.TW = static_cast<int>((W + 1) / 2); g.T = static_cast<int>(p.T);
    g.Tp = static_cast<int>(p.Tp); g.Kp = static_cast<int>(p.Kp);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* V = static_cast<float*>(workspace);
    float* M = V + p.v_floats;
    const double act = static_cast<double>(B) * H * W;
    {
        LaunchScope ls("conv_wg_in", st, 4.0 * (act * C * (relu_mask ? 2.0 : 1.0) + static_cast<double>(p.v_floats)));
        hipLaunchKernelGGL(wg_input_transform_kernel, dim3(static_cast<unsigned>((p.Tp + kBlock - 1) / kBlock), static_cast<unsigned>(g.C4)),
                           dim3(kBlock), 0, st, static_cast<const float*>(input), static_cast<const float*>(relu_mask), V, g);
    }
    if (int rc = check_launch(fn)) return rc;
    {
        // flops = the multiplications the result needs (16 per tile and channel pair), not those of the padding
        LaunchScope ls("conv_wg_gemm", st, 4.0 * (16.0 * K * p.Cp + static_cast<double>(p.v_floats) + static_cast<double>(p.m_floats)),
                       2.0 * 16.0 * static_cast<double>(p.T) * K * C);
        const unsigned grid = static_cast<unsigned>(16 * p.KT * p.TTn);
        const bool ok = dispatch<64, 128>(p.tile, [&](auto TILE) {
            hipLaunchKernelGGL(wg_batched_gemm_kernel<TILE.value>, dim3(grid), dim3(kBlock), 0, st, static_cast<const float*>(U), V, M, g.K,
                               g.C4, g.Tp, g.Kp, static_cast<int>(p.KT), static_cast<int>(p.TTn));
        });
        if (!ok) return no_kernel(fn);
    }
    if (int rc = check_launch(fn)) return rc;
    {
        LaunchScope ls("conv_wg_out", st, 4.0 * (16.0 * K * p.T + act * Kout));
        const int vec = W % 2 == 0 && reinterpret_cast<uintptr_t>(output) % 8 == 0;
        hipLaunchKernelGGL(wg_output_transform_kernel, dim3(static_cast<unsigned>((p.T + kBlock - 1) / kBlock), static_cast<unsigned>(Kout)),
                           dim3(kBlock), 0, st, M, static_cast<const float*>(bias), static_cast<float*>(output), g, epi, vec);
    }
    return check_launch(fn);
}
