// landmark_loss.hip -- the landmark term of FlowNet pre-training for ALL flow scales of a batch in one call: the loss, the loss of
// every scale and the gradient for every flow, without float atomics.
//
// Reference: LandmarkLoss / MultiScaleLDLoss, models/losses.py:61-74,114-126.  Per scale (side s, integer divisor q, weight):
//     cell   (X, Y) = (lm_F[b,l,0] div q, lm_F[b,l,1] div q)                      div = floor division
//     wanted w_c    = (lm_S[b,l,c] div q) * (2 / s) - 1
//     e[b,l,c]      = (flow[b,c,Y,X] - w_c) * gate[b,l,c]
//     mse           = sum e^2 / (2 B L)
// The composition reaches this through two floor divisions, an index build, gather, a transpose, a cast, a scale, two gate products
// and mse_loss per scale, and on the way back through gather's scatter-add: float atomics on cells that several landmarks share
// (1024 landmarks on at most 32 x 32 cells), so the flow gradient depends on the order the hardware happened to serve them in.
//
// Here: OWNER SCAN.  A thread owns one cell (b, Y, X) of one scale, both channels; a 256-thread block owns 256 consecutive cells
// of one sample's plane.  The block walks the landmarks of sample b 256 at a time, one per thread (loaded one trip ahead): a
// landmark is range-checked on the undivided 64-bit value -- outside the plane it is never turned into an index -- and the ones
// that fall on the block's own cells are packed into LDS IN LANDMARK ORDER (ballot and prefix count within a wave, the waves'
// counts in wave order): the cell counted from the block's first, the two targets and the two gates.  Every thread then walks
// the packed cells (16-byte LDS reads of four landmarks each, the same address in every lane: a broadcast; the four are tested at
// once before any is looked at singly) and adds the landmarks that fall on its own cell, still in landmark order:
//     acc_c += (gate_c * gate_c) * (flow_c - w_c)            loss += double(e_c) * double(e_c),   e_c = (flow_c - w_c) * gate_c
// Every in-range landmark has exactly one owner, so the owners' loss terms are the whole sum; each cell is written once, by its
// owner, with a plain store (grad = coef * acc, coef = weight / (B L); 0 where no landmark fell): the destination is overwritten
// completely and needs no zero-fill.  The block's loss terms meet in double in a fixed order (xor butterfly, then the four waves
// in wave order) and go to the block's slot of the workspace; a one-block launch adds the slots of each scale in a fixed order and
// writes out[0 .. n_scales] and the count of the landmarks that one scale or more skipped.  The order of every sum is a function
// of the shapes alone: two calls on the same inputs agree bit for bit.
#include "common.hpp"

namespace ffwm {
namespace {

constexpr int kLmMaxScales = 4;
constexpr int kLmChunk = kBlock;              // landmarks staged per trip: one per thread
constexpr int kLmWaves = kBlock / kWave;
constexpr int64_t kLmMaxSide = 4096;          // s^2 cells stay far inside an int

template <typename T>
struct LmScale {
    const T* flow;
    T* grad;                // NULL: no gradient for this scale
    long long range;        // s * q: lm_F components in [0, range) are inside the plane
    int s, q, tiles;        // side, divisor, 256-cell tiles per sample
    unsigned block0;        // first block of this scale
    T two_over_s, coef;     // 2 / s and weight / (B L), rounded to T
};
template <typename T>
struct LmArgs {
    LmScale<T> sc[kLmMaxScales];
    long long min_range;    // the smallest range of the call: a landmark outside it is skipped by one scale or more
    int n;
};
struct LmReduceArgs {
    unsigned block0[kLmMaxScales + 1];      // the slots of scale i are [block0[i], block0[i + 1])
    double weight[kLmMaxScales];
    int n;
};

// a div q toward minus infinity, q >= 1
__device__ __forceinline__ long long floor_div(long long a, int q) {
    if (a == static_cast<int>(a)) {                   // the usual case: a 32-bit division
        const int n = static_cast<int>(a);
        int d = n / q;
        if (n < 0 && d * q != n) --d;
        return d;
    }
    long long d = a / q;
    if (a < 0 && d * q != a) --d;
    return d;
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
landmark_loss_kernel(const LmArgs<T> a, const long long* __restrict__ lm_S, const long long* __restrict__ lm_F,
                     const T* __restrict__ gate, double* __restrict__ partial, int L) {
    __shared__ __attribute__((aligned(16))) int cell_s[kLmChunk + 4];
    __shared__ T w_s[2][kLmChunk], g_s[2][kLmChunk];
    __shared__ double red[kLmWaves];
    __shared__ int redn[kLmWaves], taken[kLmWaves];
    LmScale<T> sc = a.sc[0];
    int which = 0;
#pragma unroll
    for (int k = 1; k < kLmMaxScales; ++k)
        if (k < a.n && blockIdx.x >= a.sc[k].block0) {
            sc = a.sc[k];
            which = k;
        }
    const unsigned rel = blockIdx.x - sc.block0;
    const int b = static_cast<int>(rel / sc.tiles), tile = static_cast<int>(rel - static_cast<unsigned>(b) * sc.tiles);
    const int cells = sc.s * sc.s;
    const int mine = tile * kBlock + static_cast<int>(threadIdx.x);
    const bool live = mine < cells;
    // every block of a sample stages the same landmarks: tile 0 of scale 0 alone counts the ones a scale skips
    const bool counts = which == 0 && tile == 0;
    const int key = live ? static_cast<int>(threadIdx.x) : -2;      // staged indices are 0 .. 255 or -1: a thread past the plane matches nothing
    const size_t plane = static_cast<size_t>(cells);
    const T* fp = sc.flow + static_cast<size_t>(b) * 2 * plane;
    const T f0 = live ? fp[mine] : static_cast<T>(0), f1 = live ? fp[plane + mine] : static_cast<T>(0);

    T acc0 = 0, acc1 = 0;
    double loss = 0;
    int skipped = 0;
    auto hit = [&](const int k) {
        const T d0 = f0 - w_s[0][k], d1 = f1 - w_s[1][k];
        const T g0 = g_s[0][k], g1 = g_s[1][k];
        acc0 += (g0 * g0) * d0;
        acc1 += (g1 * g1) * d1;
        const T e0 = d0 * g0, e1 = d1 * g1;
        loss += static_cast<double>(e0) * static_cast<double>(e0);
        loss += static_cast<double>(e1) * static_cast<double>(e1);
    };
    // the raw values of landmark l0 + threadIdx.x: loaded one trip ahead, so that the loads are in flight during the scan
    struct Raw {
        long long fx, fy, sx, sy;
        T g0, g1;
    };
    auto fetch = [&](const int l0) {
        Raw r = {-1, -1, 0, 0, static_cast<T>(0), static_cast<T>(0)};          // past the last landmark: outside every plane
        const int l = l0 + static_cast<int>(threadIdx.x);
        if (l < L) {
            const size_t o = (static_cast<size_t>(b) * L + l) * 2;
            r.fx = lm_F[o];
            r.fy = lm_F[o + 1];
            r.sx = lm_S[o];
            r.sy = lm_S[o + 1];
            r.g0 = gate[o];
            r.g1 = gate[o + 1];
        }
        return r;
    };
    Raw raw = fetch(0);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int base = tile * kBlock;                   // the block's cells are [base, base + kBlock)
    for (int l0 = 0; l0 < L; l0 += kLmChunk) {
        // the range check on the undivided 64-bit values: only a landmark inside the plane becomes an index
        const bool inside = raw.fx >= 0 && raw.fx < sc.range && raw.fy >= 0 && raw.fy < sc.range;
        int local = -1;                               // the cell of the landmark, counted from the block's first
        if (inside) local = (static_cast<int>(raw.fy) / sc.q) * sc.s + static_cast<int>(raw.fx) / sc.q - base;
        const bool take = inside && local >= 0 && local < kBlock;
        if (counts && l0 + static_cast<int>(threadIdx.x) < L
            && !(raw.fx >= 0 && raw.fx < a.min_range && raw.fy >= 0 && raw.fy < a.min_range))
            ++skipped;
        // the block keeps the landmarks on its own cells, packed in landmark order: ballot and prefix count within a wave, the
        // waves' counts in wave order
        const unsigned long long votes = __ballot(take);
        if (lane == 0) taken[wave] = __popcll(votes);
        __syncthreads();                              // (the previous trip's readers are done, too: they passed their scan)
        int pos = __popcll(votes & ((1ull << lane) - 1)), total = 0;
#pragma unroll
        for (int k = 0; k < kLmWaves; ++k) {
            if (k < wave) pos += taken[k];
            total += taken[k];
        }
        if (take) {
            cell_s[pos] = local;
            w_s[0][pos] = static_cast<T>(floor_div(raw.sx, sc.q)) * sc.two_over_s - 1;
            w_s[1][pos] = static_cast<T>(floor_div(raw.sy, sc.q)) * sc.two_over_s - 1;
            g_s[0][pos] = raw.g0;
            g_s[1][pos] = raw.g1;
        }
        if (threadIdx.x < 4) cell_s[total + threadIdx.x] = -1;           // pads the last 16-byte read (cell_s has four slots to spare)
        __syncthreads();
        if (l0 + kLmChunk < L) raw = fetch(l0 + kLmChunk);
        // four kept landmarks per trip: one 16-byte broadcast read, one test whether any of them is this thread's, and only then
        // the four tests in landmark order
        const int4* c4 = reinterpret_cast<const int4*>(cell_s);
        for (int j = 0; 4 * j < total; ++j) {
            const int4 c = c4[j];
            if (!((c.x == key) | (c.y == key) | (c.z == key) | (c.w == key))) continue;
            if (c.x == key) hit(4 * j);
            if (c.y == key) hit(4 * j + 1);
            if (c.z == key) hit(4 * j + 2);
            if (c.w == key) hit(4 * j + 3);
        }
    }
    if (live && sc.grad) {
        T* gp = sc.grad + static_cast<size_t>(b) * 2 * plane;
        gp[mine] = sc.coef * acc0;
        gp[plane + mine] = sc.coef * acc1;
    }
    loss = wave_sum(loss);
    skipped = wave_sum(skipped);
    if (lane == 0) {
        red[wave] = loss;
        redn[wave] = skipped;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        int n = redn[0];
#pragma unroll
        for (int k = 1; k < kLmWaves; ++k) {
            s += red[k];
            n += redn[k];
        }
        partial[2 * static_cast<size_t>(blockIdx.x)] = s;
        partial[2 * static_cast<size_t>(blockIdx.x) + 1] = static_cast<double>(n);      // at most 256 per block: exact
    }
}

// out[1 + i] = mse_i, out[0] = sum_i weight_i mse_i, *skipped: every thread adds its slots in index order, the threads meet in a
// fixed tree, scale after scale.
template <typename T>
__global__ void __launch_bounds__(kBlock)
landmark_loss_reduce_kernel(const LmReduceArgs a, const double* __restrict__ partial, T* __restrict__ out, int* __restrict__ skipped,
                            double denom) {
    __shared__ double r0[kBlock], r1[kBlock];
    double total = 0, count = 0;
    for (int i = 0; i < a.n; ++i) {
        double s = 0, k = 0;
        for (unsigned j = a.block0[i] + threadIdx.x; j < a.block0[i + 1]; j += kBlock) {
            s += partial[2 * static_cast<size_t>(j)];
            k += partial[2 * static_cast<size_t>(j) + 1];
        }
        __syncthreads();
        r0[threadIdx.x] = s;
        r1[threadIdx.x] = k;
        __syncthreads();
        for (int h = kBlock / 2; h > 0; h >>= 1) {
            if (static_cast<int>(threadIdx.x) < h) {
                r0[threadIdx.x] += r0[threadIdx.x + h];
                r1[threadIdx.x] += r1[threadIdx.x + h];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const double mse = r0[0] / denom;
            out[1 + i] = static_cast<T>(mse);
            total += a.weight[i] * mse;
            count += r1[0];
        }
    }
    if (threadIdx.x == 0) {
        out[0] = static_cast<T>(total);
        if (skipped) *skipped = static_cast<int>(count);
    }
}

// Sizes of one call; `blocks` (may be NULL) receives the launch's block count.
int check_sizes(const char* fn, const int64_t* sides, const int64_t* divisors, int n_scales, int64_t B, int64_t L, int dtype,
                int64_t* blocks) {
    FFWM_REQUIRE(dtype_ok(dtype), FFWM_ERR_DTYPE, "%s: dtype %d is not FFWM_F32/FFWM_F64", fn, dtype);
    FFWM_REQUIRE(n_scales >= 1 && n_scales <= kLmMaxScales, FFWM_ERR_ARG, "%s: n_scales must be 1 .. %d, got %d", fn, kLmMaxScales,
                 n_scales);
    FFWM_REQUIRE(sides, FFWM_ERR_ARG, "%s: NULL array of sides", fn);
    FFWM_REQUIRE(B > 0 && L > 0, FFWM_ERR_ARG, "%s: B and L must be positive (B=%lld L=%lld)", fn, (long long)B, (long long)L);
    FFWM_REQUIRE(L <= (1LL << 30) && B <= (1LL << 30), FFWM_ERR_SIZE, "%s: B and L must stay within 2^30", fn);
    int64_t total = 0;
    for (int i = 0; i < n_scales; ++i) {
        const int64_t s = sides[i], q = divisors ? divisors[i] : 1;
        FFWM_REQUIRE(s >= 1 && q >= 1, FFWM_ERR_ARG, "%s: scale %d needs a side >= 1 and a divisor >= 1 (s=%lld q=%lld)", fn, i,
                     (long long)s, (long long)q);
        FFWM_REQUIRE(s <= kLmMaxSide && q < (1LL << 31) / s, FFWM_ERR_SIZE,
                     "%s: scale %d: the side must stay within %lld and side * divisor below 2^31", fn, i, (long long)kLmMaxSide);
        total += B * ((s * s + kBlock - 1) / kBlock);
        FFWM_REQUIRE(total < (1LL << 31), FFWM_ERR_SIZE, "%s: grid too large", fn);
    }
    if (blocks) *blocks = total;
    return FFWM_OK;
}

template <typename T>
int launch(const void* const* flows, void* const* grads, const int64_t* sides, const int64_t* divisors, const double* weights,
           int n_scales, const long long* lm_S, const long long* lm_F, const T* gate, T* out, int* skipped, double* partial, int64_t B,
           int64_t L, int64_t blocks, hipStream_t st) {
    LmArgs<T> a;
    LmReduceArgs r;
    a.n = r.n = n_scales;
    a.min_range = sides[0] * divisors[0];
    for (int i = 1; i < n_scales; ++i)
        if (sides[i] * divisors[i] < a.min_range) a.min_range = sides[i] * divisors[i];
    unsigned block0 = 0;
    double cells = 0;
    for (int i = 0; i < kLmMaxScales; ++i) {
        const int k = i < n_scales ? i : 0;              // the unused entries repeat scale 0 and are never selected
        LmScale<T>& sc = a.sc[i];
        sc.flow = static_cast<const T*>(flows[k]);
        sc.grad = grads ? static_cast<T*>(grads[k]) : nullptr;
        sc.s = static_cast<int>(sides[k]);
        sc.q = static_cast<int>(divisors[k]);
        sc.range = static_cast<long long>(sides[k]) * divisors[k];
        sc.tiles = static_cast<int>((sides[k] * sides[k] + kBlock - 1) / kBlock);
        sc.block0 = block0;
        sc.two_over_s = static_cast<T>(2.0 / static_cast<double>(sides[k]));
        sc.coef = static_cast<T>(weights[k] / (static_cast<double>(B) * static_cast<double>(L)));
        r.block0[i] = block0;
        r.weight[i] = weights[k];
        if (i < n_scales) {
            block0 += static_cast<unsigned>(B * sc.tiles);
            cells += static_cast<double>(B) * sides[k] * sides[k] * (sc.grad ? 4.0 : 2.0);
        }
    }
    for (int i = n_scales; i <= kLmMaxScales; ++i) r.block0[i] = block0;
    {
        LaunchScope scope("landmark_loss", st, sizeof(T) * (cells + 2.0 * B * L) + 32.0 * B * L + 16.0 * blocks);
        hipLaunchKernelGGL((landmark_loss_kernel<T>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, a, lm_S, lm_F, gate, partial,
                           static_cast<int>(L));
        if (int rc = check_launch("ffwm_landmark_loss")) return rc;
    }
    LaunchScope scope("landmark_loss_reduce", st, 16.0 * blocks + (n_scales + 1.0) * sizeof(T) + 4.0);
    hipLaunchKernelGGL((landmark_loss_reduce_kernel<T>), dim3(1), dim3(kBlock), 0, st, r, partial, out, skipped,
                       2.0 * static_cast<double>(B) * static_cast<double>(L));
    return check_launch("ffwm_landmark_loss(reduce)");
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int64_t ffwm_landmark_loss_workspace_bytes(const int64_t* sides, int n_scales, int64_t B, int64_t L, int dtype) {
    int64_t blocks = 0;
    if (int rc = check_sizes("ffwm_landmark_loss_workspace_bytes", sides, nullptr, n_scales, B, L, dtype, &blocks)) return rc;
    return 16 * blocks;                     // two doubles per block
}

extern "C" int ffwm_landmark_loss(const void* const* flows, void* const* grads, const int64_t* sides, const int64_t* divisors,
                                  const double* weights, int n_scales, const void* lm_S, const void* lm_F, const void* gate, void* out,
                                  void* skipped, void* workspace, int64_t B, int64_t L, int dtype, void* stream) {
    const char* fn = "ffwm_landmark_loss";
    FFWM_REQUIRE(flows && sides && divisors && weights, FFWM_ERR_ARG, "%s: NULL array of flows, sides, divisors or weights", fn);
    FFWM_REQUIRE(lm_S && lm_F && gate && out && skipped, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(workspace, FFWM_ERR_ARG, "%s: NULL workspace (ffwm_landmark_loss_workspace_bytes gives its size)", fn);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, FFWM_ERR_ARG, "%s: the workspace must be 8-byte aligned", fn);
    int64_t blocks = 0;
    if (int rc = check_sizes(fn, sides, divisors, n_scales, B, L, dtype, &blocks)) return rc;
    for (int i = 0; i < n_scales; ++i) FFWM_REQUIRE(flows[i], FFWM_ERR_ARG, "%s: NULL flow of scale %d", fn, i);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch<T>(flows, grads, sides, divisors, weights, n_scales, (const long long*)lm_S, (const long long*)lm_F,
                         (const T*)gate, (T*)out, (int*)skipped, (double*)workspace, B, L, blocks, static_cast<hipStream_t>(stream));
    });
}
