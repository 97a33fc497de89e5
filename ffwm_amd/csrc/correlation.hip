// correlation.hip -- max_i <source_i, target_j> over all source positions, for every target position,
// on the matrix cores (fp32-in / fp32-accumulate MFMA).
//
// Reference: PerceptualCorrectness.calculate_loss, /root/reference/models/losses.py:347-353 --
//     correction = torch.bmm(source_norm [B,N,C], target_norm [B,C,N])      # [B, N, N]
//     correction_max, _ = torch.max(correction, dim=1)                      # [B, N]
// with N = h*w of a VGG feature map: 16384 at relu1_1, i.e. a 1 GiB matrix PER SAMPLE that is written,
// read back once for the max and (in the reference) kept for a backward pass nobody needs.
//
// This is a genuine contraction (2 N^2 C flop per sample: 34 GFLOP at relu1_1), so it runs on MFMA;
// the N x N matrix never exists.  A workgroup owns 128 target columns of one sample, one 64-lane wave per
// 32 columns.  The wave keeps its B operands (the 32 target columns, all of K = C) in registers for the
// whole kernel, walks the source rows in tiles of 32 (staged through LDS once per workgroup, double
// buffered), issues C/2 v_mfma_f32_32x32x2_f32 per tile -- 64 cycles each, back to back on its SIMD: the
// f32 MFMA peak from one wave per SIMD -- and folds the 32 x 32 products into 16 running maxima per
// lane.  v_mfma_f32_32x32x2_f32 is an exact k-ordered fp32 fma chain, so the values are those of an
// fp32 GEMM (different summation order than rocBLAS: ~1e-7).
//
// K is permuted so that lanes 0-31 take k in [0, 32) of every 64-chunk and lanes 32-63 take [32, 64):
// every lane then loads 32 CONTIGUOUS floats of its row (the sum over k does not care about the order,
// and A and B use the same permutation).
//
// Second precision route, opt-in (ffwm_correlation_colmax_split, corr_colmax_split_kernel): the same contraction on
// v_mfma_f32_32x32x16_bf16 -- 32 cycles per SIMD for 16 k, 16 x the fp32 MFMA rate -- with every operand element split in two bf16
// terms,  hi = bf16_rn(x),  lo = bf16_rn(x - hi)  (x - hi is exact in fp32), and the product sum taken as
//     lo.hi + hi.lo + hi.hi        (source term first; lo.lo is dropped)
// in ONE fp32 accumulator, k-block by k-block, in that order: three MFMAs per 16 k instead of eight fp32 MFMAs of twice the
// cycles, an MFMA-time ceiling of 16/3.  Error per product sum (derivation: tests/colmax_split_bounds.py):
//     |prod - ref| <= (2^-16 + 3 C roundings) sum_k |s_ik t_kj|;      measured 1-3e-6 on normalised features.
// Staging.  The source tile is split ONCE, when it is committed to LDS: a hi plane and a lo plane of 32 rows x C bf16 (together the
//   bytes of the fp32 tile), each thread converting 8 consecutive floats of a row and storing them with one ds_write_b128 per
//   plane.  The wave's B operand is split once, when it is loaded: C/4 hi dwords + C/4 lo dwords, the register count of the fp32
//   kernel.  Operand lane map of the instruction: lane (r = l & 31, h = l >> 5) holds A[r][8h + j] and B[8h + j][r], j = 0..7, so
//   a fragment is one ds_read_b128 at  row r, k = 16 kb + 8h  (natural k order: A and B agree).
// LDS row pitch = C + 8 bf16 = 2C + 16 bytes = an ODD number of 16-byte slots (9 / 17 / 33).  ds_read_b128 is served in four
//   groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- over 64 banks of 4 bytes, i.e. 16 slots of
//   16 bytes.  All lanes of a group share h and kb, their rows are pairwise different mod 16, and row * odd mod 16 is a bijection:
//   every group covers the 16 slots once, the reads are conflict-free.  The stores (ds_write_b128: groups of 8 consecutive lanes,
//   32 banks) put 8 consecutive lanes on 128 consecutive bytes of one row: conflict-free as well.
// Source traffic and the column tile.  Every workgroup streams its sample's whole source from L2.  A tile of 32 rows is 128 C
//   bytes and feeds (C/16) x 3 MFMAs of 32 cycles per wave = 6 C cycles, so a CU that runs at the MFMA ceiling pulls 128 C / 6 C =
//   21.3 bytes per clock whatever C is: x 256 CUs x 2.4 GHz = 13 TB/s, 38 % of the 34.5 TB/s the per-XCD L2s deliver together
//   (the source of one sample, 4 MiB at N = 16384, C = 64, is shared by all column tiles of that sample, which run side by side).
//   A 256-column workgroup would halve that, but at (B, N, C) = (6, 16384, 64) it leaves 384 workgroups for 256 CUs -- 1.5 per CU,
//   a quarter of the chip idle in the second half -- where 128 columns give 768 = exactly 3 per CU, resident together (18 KiB of
//   LDS each), so that one workgroup's split + commit + barrier runs under the MFMA chains of the other two.  L2 is not the limit at
//   either width; the tail is.  The column tile therefore stays 128 for every (B, N, C): no route to choose, and the gate of
//   PerceptualCorrectness counts workgroups as before.
// Non-finite contract (DIFFERS from the fp32 kernel's in one point).  A NaN in source row i makes out[b, :] NaN, a NaN in target
//   column j makes out[b, j] NaN alone -- as before.  An INFINITE operand has hi = inf and lo = bf16(inf - inf) = NaN: it behaves as
//   a NaN in its row or column (the fp32 kernel gives +-inf products there; a column of -inf is no longer -inf).  Finite inputs
//   with |x| >= 2^127 may round to an infinite hi and are outside the contract.  lo terms below 2^-126 may be flushed by the matrix
//   core: an absolute error of the order of 2^-126 |operand| per product, stated in the bound (ETA).
// No atomics, fixed summation order (two calls agree bit for bit), out-of-range rows and columns are clamped copies.
#include "common.hpp"

namespace ffwm {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCorRows = 32;          // source rows per tile
constexpr int kCorCols = 128;         // target columns per workgroup (4 waves x 32)

// max that propagates NaN, as torch.max does: a NaN candidate replaces the running value, and a NaN running value is never replaced
// (every comparison with it is false)
__device__ __forceinline__ float nan_max(float m, float a) { return (a > m || a != a) ? a : m; }

template <int KC>                     // KC = C / 64
__global__ void __launch_bounds__(kBlock)
corr_colmax_kernel(const float* __restrict__ src, const float* __restrict__ tgt, float* __restrict__ out, int N,
                   int col_tiles) {
    constexpr int C = KC * 64;
    constexpr int PITCH = C + 4;      // floats; rows 272 B apart (C = 64): conflict-free ds_read_b128 across 32 rows
    constexpr int F4_PER_THREAD = kCorRows * C / 4 / kBlock;      // float4 loads per thread per tile = 2 KC
    extern __shared__ __attribute__((aligned(16))) float tile_mem[];      // 2 x 32 x PITCH floats
    const int b = blockIdx.x / col_tiles;
    const int j0 = (blockIdx.x % col_tiles) * kCorCols;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int half = lane >> 5, l31 = lane & 31;
    const float* sb = src + static_cast<size_t>(b) * N * C;
    const float* tb = tgt + static_cast<size_t>(b) * C * N;

    // B operands: column j0 + 32 wave + l31 (clamped: out-of-range columns are computed and not stored)
    const int col = min(j0 + wave * 32 + l31, N - 1);
    float breg[KC * 32];
#pragma unroll
    for (int ch = 0; ch < KC; ++ch)
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) breg[ch * 32 + kk] = tb[static_cast<size_t>(ch * 64 + half * 32 + kk) * N + col];

    // cooperative staging: float4 index f of the tile -> row f / (C/4), 4 floats at (f % (C/4)) * 4
    f32x4 stage[F4_PER_THREAD];
    auto fetch = [&](int i0) {
#pragma unroll
        for (int q = 0; q < F4_PER_THREAD; ++q) {
            const int f = threadIdx.x + q * kBlock;
            const int r = f / (C / 4), c4 = (f - r * (C / 4)) * 4;
            const int row = min(i0 + r, N - 1);
            stage[q] = *reinterpret_cast<const f32x4*>(sb + static_cast<size_t>(row) * C + c4);
        }
    };
    auto commit = [&](float* buf) {
#pragma unroll
        for (int q = 0; q < F4_PER_THREAD; ++q) {
            const int f = threadIdx.x + q * kBlock;
            const int r = f / (C / 4), c4 = (f - r * (C / 4)) * 4;
            *reinterpret_cast<f32x4*>(buf + r * PITCH + c4) = stage[q];
        }
    };

    float m[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
    const int ntiles = (N + kCorRows - 1) / kCorRows;
    fetch(0);
    commit(tile_mem);
    __syncthreads();
    int p = 0;
    for (int t = 0; t < ntiles; ++t, p ^= 1) {
        if (t + 1 < ntiles) fetch((t + 1) * kCorRows);           // lands during the MFMA chain
        const float* arow = tile_mem + p * (kCorRows * PITCH) + l31 * PITCH + half * 32;
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int ch = 0; ch < KC; ++ch) {
            float areg[32];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(arow + ch * 64 + q * 4);
                areg[q * 4] = v.x; areg[q * 4 + 1] = v.y; areg[q * 4 + 2] = v.z; areg[q * 4 + 3] = v.w;
            }
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[kk], breg[ch * 32 + kk], acc, 0, 0, 0);
        }
        // (rows past N in a ragged last tile are clamped copies of row N-1: harmless for a max)
        // torch.max semantics: a NaN product sticks (fmaxf would drop it), and the maxima start at -inf so that a column of -inf stays -inf
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = nan_max(m[r], acc[r]);
        if (t + 1 < ntiles) commit(tile_mem + (p ^ 1) * (kCorRows * PITCH));
        __syncthreads();
    }
    // C/D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): the two halves hold
    // disjoint rows of the same column
    float best = m[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) best = nan_max(best, m[r]);
    best = nan_max(best, __shfl_xor(best, 32, kWave));
    const int jc = j0 + wave * 32 + l31;
    if (half == 0 && jc < N) out[static_cast<size_t>(b) * N + jc] = best;
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// x = hi + lo + e, |e| <= 2^-18 |x|: hi = bf16_rn(x), lo = bf16_rn(x - hi) (the difference is exact in fp32; inf - inf = NaN)
__device__ __forceinline__ void split_bf16(float x, __bf16& hi, __bf16& lo) {
    hi = static_cast<__bf16>(x);
    lo = static_cast<__bf16>(x - static_cast<float>(hi));
}

template <int KC>                     // KC = C / 64
__global__ void __launch_bounds__(kBlock)
corr_colmax_split_kernel(const float* __restrict__ src, const float* __restrict__ tgt, float* __restrict__ out, int N,
                         int col_tiles) {
    constexpr int C = KC * 64;
    constexpr int KB = C / 16;                        // k-blocks of one v_mfma_f32_32x32x16_bf16
    constexpr int PITCH = C + 8;                      // bf16; 2C + 16 bytes = an odd number of 16-byte slots (file header)
    constexpr int PLANE = kCorRows * PITCH;           // bf16 per plane; a buffer = hi plane, lo plane
    constexpr int U8_PER_THREAD = kCorRows * C / 8 / kBlock;      // units of 8 floats per thread per tile = KC
    extern __shared__ __attribute__((aligned(16))) __bf16 split_mem[];    // 2 buffers x 2 planes x 32 x PITCH bf16
    const int b = blockIdx.x / col_tiles;
    const int j0 = (blockIdx.x % col_tiles) * kCorCols;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int half = lane >> 5, l31 = lane & 31;
    const float* sb = src + static_cast<size_t>(b) * N * C;
    const float* tb = tgt + static_cast<size_t>(b) * C * N;

    // B operands: column j0 + 32 wave + l31 (clamped: out-of-range columns are computed and not stored), k = 16 kb + 8 half + j
    const int col = min(j0 + wave * 32 + l31, N - 1);
    bf16x8 bhi[KB], blo[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 h, l;
            split_bf16(tb[static_cast<size_t>(kb * 16 + half * 8 + j) * N + col], h, l);
            bhi[kb][j] = h;
            blo[kb][j] = l;
        }

    // cooperative staging: unit e of the tile -> row e / (C/8), 8 floats at (e % (C/8)) * 8
    f32x4 stage[U8_PER_THREAD][2];
    auto fetch = [&](int i0) {
#pragma unroll
        for (int q = 0; q < U8_PER_THREAD; ++q) {
            const int e = threadIdx.x + q * kBlock;
            const int r = e / (C / 8), c8 = (e - r * (C / 8)) * 8;
            const float* p = sb + static_cast<size_t>(min(i0 + r, N - 1)) * C + c8;
            stage[q][0] = *reinterpret_cast<const f32x4*>(p);
            stage[q][1] = *reinterpret_cast<const f32x4*>(p + 4);
        }
    };
    auto commit = [&](__bf16* buf) {
#pragma unroll
        for (int q = 0; q < U8_PER_THREAD; ++q) {
            const int e = threadIdx.x + q * kBlock;
            const int r = e / (C / 8), c8 = (e - r * (C / 8)) * 8;
            bf16x8 h, l;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 hj, lj;
                split_bf16(stage[q][j >> 2][j & 3], hj, lj);
                h[j] = hj;
                l[j] = lj;
            }
            *reinterpret_cast<bf16x8*>(buf + r * PITCH + c8) = h;
            *reinterpret_cast<bf16x8*>(buf + PLANE + r * PITCH + c8) = l;
        }
    };

    float m[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
    const int ntiles = (N + kCorRows - 1) / kCorRows;
    fetch(0);
    commit(split_mem);
    __syncthreads();
    int p = 0;
    for (int t = 0; t < ntiles; ++t, p ^= 1) {
        if (t + 1 < ntiles) fetch((t + 1) * kCorRows);           // lands during the MFMA chain
        const __bf16* ahi = split_mem + p * (2 * PLANE) + l31 * PITCH + half * 8;
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int ch = 0; ch < KC; ++ch) {                        // 64 k at a time: 8 ds_read_b128 in flight, then 12 MFMAs
            bf16x8 ah[4], al[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ah[q] = *reinterpret_cast<const bf16x8*>(ahi + (ch * 4 + q) * 16);
                al[q] = *reinterpret_cast<const bf16x8*>(ahi + PLANE + (ch * 4 + q) * 16);
            }
            __builtin_amdgcn_sched_barrier(0);                   // keep the reads ahead of the chain (the scheduler sinks each to its use)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int kb = ch * 4 + q;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[q], bhi[kb], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[q], blo[kb], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[q], bhi[kb], acc, 0, 0, 0);
            }
        }
        // the fold, the cross-half shuffle and the store are those of corr_colmax_kernel: the C/D layout is the same
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = nan_max(m[r], acc[r]);
        if (t + 1 < ntiles) commit(split_mem + (p ^ 1) * (2 * PLANE));
        __syncthreads();
    }
    float best = m[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) best = nan_max(best, m[r]);
    best = nan_max(best, __shfl_xor(best, 32, kWave));
    const int jc = j0 + wave * 32 + l31;
    if (half == 0 && jc < N) out[static_cast<size_t>(b) * N + jc] = best;
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_correlation_colmax(const void* source, const void* target, void* out, int64_t B, int64_t N,
                                       int64_t C, int dtype, void* stream) {
    const char* fn = "ffwm_correlation_colmax";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only (fp32 MFMA)", fn);
    FFWM_REQUIRE(source && target && out, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && N > 0 && (C == 64 || C == 128 || C == 256), FFWM_ERR_ARG,
                 "%s: need B, N > 0 and C in {64, 128, 256} (VGG relu1_1 / relu2_1 / relu3_1), got B=%lld N=%lld C=%lld", fn,
                 (long long)B, (long long)N, (long long)C);
    const int64_t col_tiles = (N + kCorCols - 1) / kCorCols;
    FFWM_REQUIRE(N < (1LL << 30) && B * col_tiles < (1LL << 31), FFWM_ERR_SIZE, "%s: tensor too large", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = static_cast<unsigned>(B * col_tiles);
    // "bytes" of this compute-bound kernel: operands read once + result (the roofline that matters is MFMA)
    LaunchScope ls("correlation_colmax", st, 4.0 * B * (2.0 * N * C + N), 2.0 * B * N * N * C);
    const size_t lds = 2 * static_cast<size_t>(kCorRows) * (C + 4) * sizeof(float);
    allow_large_lds(reinterpret_cast<const void*>(corr_colmax_kernel<4>));
    if (C == 64)
        hipLaunchKernelGGL((corr_colmax_kernel<1>), dim3(grid), dim3(kBlock), lds, st, (const float*)source, (const float*)target,
                           (float*)out, (int)N, (int)col_tiles);
    else if (C == 128)
        hipLaunchKernelGGL((corr_colmax_kernel<2>), dim3(grid), dim3(kBlock), lds, st, (const float*)source, (const float*)target,
                           (float*)out, (int)N, (int)col_tiles);
    else
        hipLaunchKernelGGL((corr_colmax_kernel<4>), dim3(grid), dim3(kBlock), lds, st, (const float*)source, (const float*)target,
                           (float*)out, (int)N, (int)col_tiles);
    return check_launch(fn);
}

extern "C" int ffwm_correlation_colmax_split(const void* source, const void* target, void* out, int64_t B, int64_t N,
                                             int64_t C, int dtype, void* stream) {
    const char* fn = "ffwm_correlation_colmax_split";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only (split into bf16 terms for the bf16 MFMA)", fn);
    FFWM_REQUIRE(source && target && out, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(B > 0 && N > 0 && (C == 64 || C == 128 || C == 256), FFWM_ERR_ARG,
                 "%s: need B, N > 0 and C in {64, 128, 256} (VGG relu1_1 / relu2_1 / relu3_1), got B=%lld N=%lld C=%lld", fn,
                 (long long)B, (long long)N, (long long)C);
    const int64_t col_tiles = (N + kCorCols - 1) / kCorCols;
    FFWM_REQUIRE(N < (1LL << 30) && B * col_tiles < (1LL << 31), FFWM_ERR_SIZE, "%s: tensor too large", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = static_cast<unsigned>(B * col_tiles);
    // the algorithmic bytes and flops of the fp32 row: the two rows compare as times
    LaunchScope ls("correlation_colmax_split", st, 4.0 * B * (2.0 * N * C + N), 2.0 * B * N * N * C);
    const size_t lds = 2 * 2 * static_cast<size_t>(kCorRows) * (C + 8) * sizeof(__bf16);
    allow_large_lds(reinterpret_cast<const void*>(corr_colmax_split_kernel<4>));
    if (C == 64)
        hipLaunchKernelGGL((corr_colmax_split_kernel<1>), dim3(grid), dim3(kBlock), lds, st, (const float*)source,
                           (const float*)target, (float*)out, (int)N, (int)col_tiles);
    else if (C == 128)
        hipLaunchKernelGGL((corr_colmax_split_kernel<2>), dim3(grid), dim3(kBlock), lds, st, (const float*)source,
                           (const float*)target, (float*)out, (int)N, (int)col_tiles);
    else
        hipLaunchKernelGGL((corr_colmax_split_kernel<4>), dim3(grid), dim3(kBlock), lds, st, (const float*)source,
                           (const float*)target, (float*)out, (int)N, (int)col_tiles);
    return check_launch(fn);
}
