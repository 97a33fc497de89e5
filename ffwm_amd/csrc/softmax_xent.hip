// softmax_xent.hip -- the classifier loss of LightCNN fine-tuning in one call: mean cross entropy, its gradient for the logits,
// every row's rank of the target and prec@1 / prec@5, without float atomics.
//
// Reference: lightcnn/finetune.py:109,152-159 -- nn.CrossEntropyLoss over 79 077 classes and accuracy(output, target, (1, 5)),
// a topk over the same [10, 79077] matrix; in ATen about 15 launches forward and backward.
//
// B = 10 rows cannot fill the chip, so a row is cut into chunks of kXeChunk elements and the grid is (chunks, B):
//   pass 1  every block reduces its chunk: the maximum m (NaN left out), sum exp(x - m) -- each term in T, accumulated in double: per
//           thread, xor butterfly, the four waves in wave order --, the elements greater than the target's logit and the equal ones
//           in front of it.  One 24-byte slot per (row, chunk).
//   pass 2  every block combines ALL slots of its row in index order (each thread its slots in ascending order, then a fixed tree),
//           so that every block of a row holds the same bits of
//               M = max m_c,   S = sum_c s_c exp(m_c - M),   lse = M + log S          (double)
//           and writes its chunk of grad = (exp(x - T(lse)) - [j == t]) / B.  Chunk 0 writes the row's loss lse - x_t and its rank.
//   pass 3  one block adds the rows' losses (double, fixed order) and counts the hits and the rows that were skipped.
// A row whose target lies outside [0, N) is never dereferenced with it: loss 0, gradient row 0, rank N (no valid row reaches N).
// The order of every sum is a function of the shapes alone: two calls on the same input agree bit for bit.
#include "common.hpp"

namespace ffwm {
namespace {

constexpr int kXePerThread = 4;
constexpr int kXeChunk = kBlock * kXePerThread;       // elements of a row that one block reduces
constexpr int kXeWaves = kBlock / kWave;
constexpr int64_t kXeMaxN = 1LL << 24;                // ranks and chunk counts stay far inside an int
constexpr int64_t kXeMaxB = 65535;                    // gridDim.y

struct XeSlot {
    double m, s;            // chunk maximum (NaN left out; -inf when nothing finite), sum of exp(x - m)
    int gt, eq;             // elements that rank above the target, equal elements in front of it
};

__device__ __forceinline__ float exp_t(float v) { return expf(v); }
__device__ __forceinline__ double exp_t(double v) { return exp(v); }

template <typename T>
struct XeVec {
    typedef T type __attribute__((ext_vector_type(4)));
};

// The block's elements of a row: four consecutive ones per thread when the chunk starts on a vector boundary (one 16 / 32-byte
// access), else element q * 256 + thread (coalesced scalars).  idx[q] is the position in the row; positions past N read as -inf,
// which adds nothing to the maximum, the sum or the counts.
template <typename T>
__device__ __forceinline__ void xe_load(const T* __restrict__ row, int64_t base, int64_t N, bool vec, T v[4], int64_t idx[4]) {
    const T ninf = -__builtin_huge_val();
    if (vec) {
        const int64_t j0 = base + 4 * static_cast<int64_t>(threadIdx.x);
#pragma unroll
        for (int q = 0; q < 4; ++q) idx[q] = j0 + q;
        if (j0 + 4 <= N) {
            const typename XeVec<T>::type w = *reinterpret_cast<const typename XeVec<T>::type*>(row + j0);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
            return;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) idx[q] = base + q * kBlock + static_cast<int64_t>(threadIdx.x);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = idx[q] < N ? row[idx[q]] : ninf;
}

template <typename T>
__device__ __forceinline__ bool xe_vec_ok(const T* p) {
    return reinterpret_cast<uintptr_t>(p) % (4 * sizeof(T)) == 0;
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
xent_partial_kernel(const T* __restrict__ x, const long long* __restrict__ target, XeSlot* __restrict__ slots, int64_t N) {
    __shared__ double red_m[kXeWaves], red_s[kXeWaves];
    __shared__ int red_g[kXeWaves], red_e[kXeWaves];
    const int b = blockIdx.y, chunks = gridDim.x;
    const long long t = target[b];
    if (t < 0 || t >= N) return;                       // (the whole block: pass 2 never reads this row's slots)
    const T* row = x + static_cast<size_t>(b) * static_cast<size_t>(N);
    const T xt = row[t];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kXeChunk;
    T v[4];
    int64_t idx[4];
    xe_load(row, base, N, xe_vec_ok(row + base), v, idx);
    const T ninf = -__builtin_huge_val();
    T m = ninf;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (v[q] > m) m = v[q];                        // a NaN is never taken
    m = wave_max(m);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) red_m[wave] = static_cast<double>(m);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kXeWaves; ++k) {
        const T u = static_cast<T>(red_m[k]);
        if (u > m) m = u;
    }
    double s = 0;
    int gt = 0, eq = 0;
    const bool tnan = xt != xt;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const T a = v[q];
        if (a != ninf) s += static_cast<double>(exp_t(a - m));          // a NaN goes through: the sum becomes NaN
        const bool anan = a != a;
        gt += (anan ? !tnan : a > xt) ? 1 : 0;                          // NaN ranks above everything, equal to another NaN
        eq += ((a == xt || (anan && tnan)) && idx[q] < t) ? 1 : 0;
    }
    s = wave_sum(s);
    gt = wave_sum(gt);
    eq = wave_sum(eq);
    if (lane == 0) {
        red_s[wave] = s;
        red_g[wave] = gt;
        red_e[wave] = eq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        XeSlot o;
        o.m = static_cast<double>(m);
        o.s = red_s[0];
        o.gt = red_g[0];
        o.eq = red_e[0];
#pragma unroll
        for (int k = 1; k < kXeWaves; ++k) {
            o.s += red_s[k];
            o.gt += red_g[k];
            o.eq += red_e[k];
        }
        slots[static_cast<size_t>(b) * chunks + blockIdx.x] = o;
    }
}

// `chunks`: the slots per row (pass 1's gridDim.x); this launch has one block per row when no gradient is wanted.
template <typename T>
__global__ void __launch_bounds__(kBlock)
xent_finish_kernel(const T* __restrict__ x, const long long* __restrict__ target, const XeSlot* __restrict__ slots,
                   T* __restrict__ grad, T* __restrict__ row_loss, int* __restrict__ rank, double* __restrict__ loss_ws,
                   int* __restrict__ rank_ws, int64_t N, int chunks, T Bt) {
    __shared__ double r0[kBlock];
    __shared__ int r1[kBlock], r2[kBlock];
    const int b = blockIdx.y;
    const long long t = target[b];
    const bool valid = t >= 0 && t < N;
    const T* row = x + static_cast<size_t>(b) * static_cast<size_t>(N);
    double lse = 0;
    int rk = static_cast<int>(N);
    if (valid) {                                        // (uniform over the block)
        const XeSlot* sl = slots + static_cast<size_t>(b) * chunks;
        double M = -__builtin_huge_val();
        for (int i = threadIdx.x; i < chunks; i += kBlock) {
            const double u = sl[i].m;
            if (u > M) M = u;
        }
        r0[threadIdx.x] = M;
        __syncthreads();
        for (int h = kBlock / 2; h > 0; h >>= 1) {
            if (static_cast<int>(threadIdx.x) < h && r0[threadIdx.x + h] > r0[threadIdx.x]) r0[threadIdx.x] = r0[threadIdx.x + h];
            __syncthreads();
        }
        M = r0[0];
        __syncthreads();
        double S = 0;
        int gt = 0, eq = 0;
        for (int i = threadIdx.x; i < chunks; i += kBlock) {
            const XeSlot o = sl[i];
            if (o.s != 0) S += o.s * exp(o.m - M);      // (a chunk of -inf alone: s = 0, m = -inf; a NaN sum goes through)
            gt += o.gt;
            eq += o.eq;
        }
        r0[threadIdx.x] = S;
        r1[threadIdx.x] = gt;
        r2[threadIdx.x] = eq;
        __syncthreads();
        for (int h = kBlock / 2; h > 0; h >>= 1) {
            if (static_cast<int>(threadIdx.x) < h) {
                r0[threadIdx.x] += r0[threadIdx.x + h];
                r1[threadIdx.x] += r1[threadIdx.x + h];
                r2[threadIdx.x] += r2[threadIdx.x + h];
            }
            __syncthreads();
        }
        lse = M + log(r0[0]);
        rk = r1[0] + r2[0];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double loss = valid ? lse - static_cast<double>(row[t]) : 0.0;
        loss_ws[b] = loss;
        rank_ws[b] = rk;
        if (row_loss) row_loss[b] = static_cast<T>(loss);
        if (rank) rank[b] = rk;
    }
    if (!grad) return;
    T* grow = grad + static_cast<size_t>(b) * static_cast<size_t>(N);
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kXeChunk;
    const bool vec = xe_vec_ok(row + base) && xe_vec_ok(grow + base);
    T v[4];
    int64_t idx[4];
    if (valid) {
        xe_load(row, base, N, vec, v, idx);
        const T lse_t = static_cast<T>(lse);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            T p = exp_t(v[q] - lse_t);                  // exp(-inf) = 0 exactly
            if (idx[q] == t) p = p - 1;
            v[q] = p / Bt;
        }
    } else {
        if (vec) {
#pragma unroll
            for (int q = 0; q < 4; ++q) idx[q] = base + 4 * static_cast<int64_t>(threadIdx.x) + q;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) idx[q] = base + q * kBlock + static_cast<int64_t>(threadIdx.x);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = 0;
    }
    if (vec && idx[3] < N) {
        const typename XeVec<T>::type w = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<typename XeVec<T>::type*>(grow + idx[0]) = w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (idx[q] < N) grow[idx[q]] = v[q];
    }
}

// out[0] = mean loss, out[1] / out[2] = prec@1 / prec@5 in percent, *skipped = rows with a target outside [0, N) (their rank is N).
template <typename T>
__global__ void __launch_bounds__(kBlock)
xent_reduce_kernel(const double* __restrict__ loss_ws, const int* __restrict__ rank_ws, T* __restrict__ out, int* __restrict__ skipped,
                   int B, int N) {
    __shared__ double r0[kBlock];
    __shared__ int r1[kBlock], r2[kBlock], r3[kBlock];
    double s = 0;
    int c1 = 0, c5 = 0, sk = 0;
    for (int i = threadIdx.x; i < B; i += kBlock) {
        const int rk = rank_ws[i];
        s += loss_ws[i];
        c1 += rk < 1 ? 1 : 0;
        c5 += rk < 5 ? 1 : 0;
        sk += rk == N ? 1 : 0;
    }
    r0[threadIdx.x] = s;
    r1[threadIdx.x] = c1;
    r2[threadIdx.x] = c5;
    r3[threadIdx.x] = sk;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (static_cast<int>(threadIdx.x) < h) {
            r0[threadIdx.x] += r0[threadIdx.x + h];
            r1[threadIdx.x] += r1[threadIdx.x + h];
            r2[threadIdx.x] += r2[threadIdx.x + h];
            r3[threadIdx.x] += r3[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const T per = static_cast<T>(100.0 / static_cast<double>(B));          // accuracy(): correct_k.mul_(100.0 / batch_size)
        out[0] = static_cast<T>(r0[0] / static_cast<double>(B));
        out[1] = static_cast<T>(r1[0]) * per;
        out[2] = static_cast<T>(r2[0]) * per;
        if (skipped) *skipped = r3[0];
    }
}

int check_sizes(const char* fn, int64_t B, int64_t N, int dtype) {
    FFWM_REQUIRE(dtype_ok(dtype), FFWM_ERR_DTYPE, "%s: dtype %d is not FFWM_F32/FFWM_F64", fn, dtype);
    FFWM_REQUIRE(B >= 1 && N >= 1, FFWM_ERR_ARG, "%s: B and N must be positive (B=%lld N=%lld)", fn, (long long)B, (long long)N);
    FFWM_REQUIRE(N <= kXeMaxN, FFWM_ERR_SIZE, "%s: N must stay within 2^24, got %lld", fn, (long long)N);
    FFWM_REQUIRE(B <= kXeMaxB, FFWM_ERR_SIZE, "%s: B must stay within %lld, got %lld", fn, (long long)kXeMaxB, (long long)B);
    return FFWM_OK;
}

inline int64_t xe_chunks(int64_t N) { return (N + kXeChunk - 1) / kXeChunk; }
inline int64_t xe_slot_bytes(int64_t B, int64_t N) { return static_cast<int64_t>(sizeof(XeSlot)) * B * xe_chunks(N); }

template <typename T>
int launch(const T* x, const long long* target, T* out, T* row_loss, int* rank, T* grad, int* skipped, char* ws, int64_t B, int64_t N,
           hipStream_t st) {
    const int chunks = static_cast<int>(xe_chunks(N));
    XeSlot* slots = reinterpret_cast<XeSlot*>(ws);
    double* loss_ws = reinterpret_cast<double*>(ws + xe_slot_bytes(B, N));
    int* rank_ws = reinterpret_cast<int*>(loss_ws + B);
    const double logits = static_cast<double>(sizeof(T)) * B * N, slot_bytes = static_cast<double>(xe_slot_bytes(B, N));
    {
        LaunchScope scope("softmax_xent_partial", st, logits + slot_bytes + 8.0 * B);
        hipLaunchKernelGGL((xent_partial_kernel<T>), dim3(chunks, static_cast<unsigned>(B)), dim3(kBlock), 0, st, x, target, slots, N);
        if (int rc = check_launch("ffwm_softmax_xent(partial)")) return rc;
    }
    {
        const int blocks = grad ? chunks : 1;
        LaunchScope scope("softmax_xent_finish", st, (grad ? 2.0 * logits : 0.0) + slot_bytes * blocks + 32.0 * B);
        hipLaunchKernelGGL((xent_finish_kernel<T>), dim3(blocks, static_cast<unsigned>(B)), dim3(kBlock), 0, st, x, target, slots, grad,
                           row_loss, rank, loss_ws, rank_ws, N, chunks, static_cast<T>(B));
        if (int rc = check_launch("ffwm_softmax_xent(finish)")) return rc;
    }
    LaunchScope scope("softmax_xent_reduce", st, 12.0 * B + 3.0 * sizeof(T) + 4.0);
    hipLaunchKernelGGL((xent_reduce_kernel<T>), dim3(1), dim3(kBlock), 0, st, loss_ws, rank_ws, out, skipped, static_cast<int>(B),
                       static_cast<int>(N));
    return check_launch("ffwm_softmax_xent(reduce)");
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_softmax_xent_chunk(void) { return kXeChunk; }

extern "C" int64_t ffwm_softmax_xent_workspace_bytes(int64_t B, int64_t N, int dtype) {
    if (int rc = check_sizes("ffwm_softmax_xent_workspace_bytes", B, N, dtype)) return rc;
    return xe_slot_bytes(B, N) + 16 * B;               // the slots, then a double and an int per row
}

extern "C" int ffwm_softmax_xent(const void* logits, const int64_t* target, void* out, void* row_loss, int* rank, void* grad_logits,
                                 int* skipped, void* workspace, int64_t B, int64_t N, int dtype, void* stream) {
    const char* fn = "ffwm_softmax_xent";
    FFWM_REQUIRE(logits && target && out, FFWM_ERR_ARG, "%s: NULL tensor pointer (logits, target or out)", fn);
    FFWM_REQUIRE(skipped, FFWM_ERR_ARG, "%s: NULL pointer for the count of skipped rows", fn);
    FFWM_REQUIRE(workspace, FFWM_ERR_ARG, "%s: NULL workspace (ffwm_softmax_xent_workspace_bytes gives its size)", fn);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, FFWM_ERR_ARG, "%s: the workspace must be 8-byte aligned", fn);
    if (int rc = check_sizes(fn, B, N, dtype)) return rc;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch<T>((const T*)logits, (const long long*)target, (T*)out, (T*)row_loss, rank, (T*)grad_logits, skipped,
                         (char*)workspace, B, N, static_cast<hipStream_t>(stream));
    });
}
