// grad_health.hip -- gradient health of a FLAT gradient range, per segment: sum g^2 and max |g| over the finite elements, the count
// of non-finite ones (NaN, +inf, -inf) and the element count.
//
// A captured train step runs no Python: between two loss_values() calls nothing looks at a gradient, and a non-finite gradient that
// reaches the Adam kernel is written into the parameter and both moments for good.  The gradients of one optimizer are one contiguous
// range of the reducer's flat array (ffwm_amd/dp.py: every parameter 16-byte aligned, zero padding), so looking at all of them is one
// streaming read: 4 n bytes, HBM-bound.  The record this file writes is what adam.hip's guarded step decides on, in device memory.
//
// Two launches, no atomics, no dependence on the grid size or on timing:
//   chunk pass    a segment is cut, from ITS start, into chunks of FFWM_GRAD_HEALTH_CHUNK elements (the last one shorter), so a chunk
//                 never straddles a segment; chunk c of the whole table is summed by ONE workgroup into workspace[4 c .. 4 c + 3] =
//                 (sum, max, non-finite count, element count).  The grid strides over the chunks; which workgroup takes a chunk does
//                 not change what it computes.
//   segment pass  workgroup s adds the partials of segment s into record[4 s .. 4 s + 3].
//
// Order of summation (all in double; the square of a float is exact in double, so no term is rounded before it is added):
//   1. thread t of the 256 adds, into its own accumulator starting at 0, the float4 vectors t, t + 256, t + 512, ... of the chunk, the
//      four lanes of a vector in the order x, y, z, w; then, for t < (length mod 4), the tail element (4 * vectors + t).
//   2. the 64 lanes of a wave meet in the xor butterfly of wave_sum: offsets 32, 16, 8, 4, 2, 1.
//   3. the four waves meet through LDS, added left to right: ((w0 + w1) + w2) + w3.
//   4. segment pass: thread t adds the partials t, t + 256, ... of its segment in that order, then steps 2 and 3 again.
// The maximum and the counts are exact in any order.  A non-finite element adds 0 to the sum, takes no part in the maximum and counts
// once; -0.0 and denormals are finite values like any other.
//
// The table of segment ends is read from DEVICE memory by both kernels (a captured launch holds its address).  Each kernel reads it
// through the same sanitising walk -- an end is clamped into [previous end, n], every end but the last is rounded down to a multiple
// of 4 and the last one is n -- so that no table, whatever it holds, makes a load leave [grads, grads + n).  The entry point refuses
// a table that would need any of that (see there).
#include "common.hpp"

namespace ffwm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kGhChunk = FFWM_GRAD_HEALTH_CHUNK;
constexpr int kGhMaxSegments = FFWM_GRAD_HEALTH_MAX_SEGMENTS;
static_assert(kGhChunk % (4 * kBlock) == 0, "a full chunk is a whole number of float4 per thread");

// The sanitised end of segment s, given the sanitised end of the one before (see the head of the file).
__device__ __forceinline__ long long gh_end(const long long* __restrict__ seg_end, int s, int n_seg, long long prev, long long n) {
    if (s == n_seg - 1) return n;
    long long e = seg_end[s];
    e = e < prev ? prev : (e > n ? n : e);
    return e & ~3LL;
}

__device__ __forceinline__ long long gh_chunks(long long len) { return (len + kGhChunk - 1) / kGhChunk; }

__device__ __forceinline__ void gh_one(float x, double& sum, float& mx, int& bad) {
    const float a = fabsf(x);
    const bool fin = (__float_as_uint(x) & 0x7fffffffu) < 0x7f800000u;
    const double d = static_cast<double>(x);
    sum += fin ? d * d : 0.0;
    mx = fin && a > mx ? a : mx;
    bad += fin ? 0 : 1;
}

// (sum, max, count) of the workgroup's 256 threads -> thread 0, in the order of steps 2 and 3.  Called by every thread.
__device__ __forceinline__ void gh_block_reduce(double& sum, double& mx, double& cnt, double* s_sum, double* s_max, double* s_cnt) {
    sum = wave_sum(sum);
    mx = wave_max(mx);
    cnt = wave_sum(cnt);
    const int wave = threadIdx.x / kWave;
    __syncthreads();                                  // the cells of the chunk before have been read
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_sum[wave] = sum;
        s_max[wave] = mx;
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = s_sum[0];
        mx = s_max[0];
        cnt = s_cnt[0];
        for (int w = 1; w < kBlock / kWave; ++w) {
            sum += s_sum[w];
            mx = s_max[w] > mx ? s_max[w] : mx;
            cnt += s_cnt[w];
        }
    }
}

__global__ void __launch_bounds__(kBlock)
grad_health_chunk_kernel(const float* __restrict__ g, long long n, const long long* __restrict__ seg_end, int n_seg,
                         double* __restrict__ workspace) {
    __shared__ double s_sum[kBlock / kWave], s_max[kBlock / kWave], s_cnt[kBlock / kWave];
    // chunks of the whole table (wave-uniform: the compiler keeps the walk on the scalar unit)
    long long total = 0, prev = 0;
    for (int s = 0; s < n_seg; ++s) {
        const long long e = gh_end(seg_end, s, n_seg, prev, n);
        total += gh_chunks(e - prev);
        prev = e;
    }
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        // chunk c -> its segment and its element range [a, b)
        long long first = 0, begin = 0, end = 0;
        prev = 0;
        for (int s = 0; s < n_seg; ++s) {
            const long long e = gh_end(seg_end, s, n_seg, prev, n);
            const long long k = gh_chunks(e - prev);
            if (c < first + k) {
                begin = prev;
                end = e;
                break;
            }
            first += k;
            prev = e;
        }
        const long long a = begin + (c - first) * kGhChunk;               // a multiple of 4: 16-byte aligned
        const long long b = a + kGhChunk < end ? a + kGhChunk : end;
        const int len = static_cast<int>(b - a), nv = len >> 2, tail = len & 3;
        const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + a);
        double sum = 0.0;
        float mx = 0.f;
        int bad = 0;
        if (len == kGhChunk) {
            f32x4 v[kGhChunk / (4 * kBlock)];
#pragma unroll
            for (int j = 0; j < kGhChunk / (4 * kBlock); ++j) v[j] = __builtin_nontemporal_load(g4 + j * kBlock + threadIdx.x);
#pragma unroll
            for (int j = 0; j < kGhChunk / (4 * kBlock); ++j) {
                gh_one(v[j].x, sum, mx, bad);
                gh_one(v[j].y, sum, mx, bad);
                gh_one(v[j].z, sum, mx, bad);
                gh_one(v[j].w, sum, mx, bad);
            }
        } else {
            for (int j = threadIdx.x; j < nv; j += kBlock) {
                const f32x4 v = __builtin_nontemporal_load(g4 + j);
                gh_one(v.x, sum, mx, bad);
                gh_one(v.y, sum, mx, bad);
                gh_one(v.z, sum, mx, bad);
                gh_one(v.w, sum, mx, bad);
            }
            if (static_cast<int>(threadIdx.x) < tail) gh_one(g[a + 4 * nv + threadIdx.x], sum, mx, bad);
        }
        double m = static_cast<double>(mx), cnt = static_cast<double>(bad);
        gh_block_reduce(sum, m, cnt, s_sum, s_max, s_cnt);
        if (threadIdx.x == 0) {
            f64x2* out = reinterpret_cast<f64x2*>(workspace + 4 * c);
            const f64x2 lo = {sum, m}, hi = {cnt, static_cast<double>(len)};
            out[0] = lo;
            out[1] = hi;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
grad_health_segment_kernel(const double* __restrict__ workspace, long long n, const long long* __restrict__ seg_end, int n_seg,
                           double* __restrict__ record) {
    __shared__ double s_sum[kBlock / kWave], s_max[kBlock / kWave], s_cnt[kBlock / kWave];
    const int seg = blockIdx.x;
    long long first = 0, prev = 0, count = 0, len = 0;
    for (int s = 0; s <= seg; ++s) {
        const long long e = gh_end(seg_end, s, n_seg, prev, n);
        first += count;
        len = e - prev;
        count = gh_chunks(len);
        prev = e;
    }
    double sum = 0.0, mx = 0.0, cnt = 0.0;
    for (long long i = threadIdx.x; i < count; i += kBlock) {
        const f64x2* in = reinterpret_cast<const f64x2*>(workspace + 4 * (first + i));
        const f64x2 lo = in[0], hi = in[1];
        sum += lo.x;
        mx = lo.y > mx ? lo.y : mx;
        cnt += hi.x;
    }
    gh_block_reduce(sum, mx, cnt, s_sum, s_max, s_cnt);
    if (threadIdx.x == 0) {
        f64x2* out = reinterpret_cast<f64x2*>(record + 4 * seg);
        const f64x2 lo = {sum, mx}, hi = {cnt, static_cast<double>(len)};
        out[0] = lo;
        out[1] = hi;
    }
}

// Chunks a table of n_seg segments over n elements can have at most: every segment rounds up once.
inline int64_t gh_max_chunks(int64_t n, int n_seg) { return n / kGhChunk + n_seg; }

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" size_t ffwm_grad_health_workspace_bytes(int64_t n, int n_seg) {
    if (n <= 0 || n_seg < 1 || n_seg > kGhMaxSegments) return 0;
    return static_cast<size_t>(gh_max_chunks(n, n_seg)) * 4 * sizeof(double);
}

extern "C" int ffwm_grad_health(const void* grads, int64_t n, const int64_t* seg_end, int n_seg, void* workspace,
                                size_t workspace_bytes, void* record, int dtype, void* stream) {
    const char* fn = "ffwm_grad_health";
    FFWM_REQUIRE(dtype == FFWM_F32, FFWM_ERR_DTYPE, "%s: float32 only", fn);
    FFWM_REQUIRE(grads && seg_end && workspace && record, FFWM_ERR_ARG, "%s: NULL pointer (grads, seg_end, workspace or record)", fn);
    FFWM_REQUIRE(n > 0, FFWM_ERR_ARG, "%s: need n > 0 (n=%lld)", fn, (long long)n);
    FFWM_REQUIRE(n_seg >= 1 && n_seg <= kGhMaxSegments, FFWM_ERR_ARG, "%s: n_seg must be 1 .. %d, got %d", fn, kGhMaxSegments, n_seg);
    FFWM_REQUIRE(reinterpret_cast<uintptr_t>(grads) % 16 == 0, FFWM_ERR_ARG, "%s: grads must be 16-byte aligned", fn);
    FFWM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(record)) % 16 == 0 &&
                 reinterpret_cast<uintptr_t>(seg_end) % 8 == 0, FFWM_ERR_ARG,
                 "%s: workspace and record must be 16-byte aligned, seg_end 8-byte aligned", fn);
    FFWM_REQUIRE(workspace_bytes >= ffwm_grad_health_workspace_bytes(n, n_seg), FFWM_ERR_ARG,
                 "%s: workspace of %llu bytes, ffwm_grad_health_workspace_bytes asks for %llu", fn, (unsigned long long)workspace_bytes,
                 (unsigned long long)ffwm_grad_health_workspace_bytes(n, n_seg));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The table lives in device memory.  On a stream that is being captured the host cannot read it (and a replay would not come by
    // here again): the kernels' sanitising walk keeps every load inside the array.  Anywhere else it is read back and checked -- the one
    // place where this library waits for a stream; 128 bytes behind whatever the stream still holds.
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
        (void)hipGetLastError();
        cs = hipStreamCaptureStatusActive;          // (the null stream beside a capture elsewhere: reading would break that capture)
    }
    if (cs == hipStreamCaptureStatusNone) {
        int64_t ends[kGhMaxSegments];
        if (hipMemcpyAsync(ends, seg_end, sizeof(int64_t) * n_seg, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: the segment table could not be read from the device", fn);
            return FFWM_ERR_LAUNCH;
        }
        int64_t prev = 0;
        for (int s = 0; s < n_seg; ++s) {
            FFWM_REQUIRE(ends[s] >= prev && ends[s] <= n, FFWM_ERR_ARG, "%s: seg_end[%d] = %lld is not ascending within [0, n = %lld]", fn, s,
                         (long long)ends[s], (long long)n);
            FFWM_REQUIRE(s == n_seg - 1 || ends[s] % 4 == 0, FFWM_ERR_ARG,
                         "%s: seg_end[%d] = %lld is not a multiple of 4 (only the last end may be)", fn, s, (long long)ends[s]);
            prev = ends[s];
        }
        FFWM_REQUIRE(prev == n, FFWM_ERR_ARG, "%s: the last segment ends at %lld, not at n = %lld", fn, (long long)prev, (long long)n);
    }
    const int64_t chunks = gh_max_chunks(n, n_seg);
    const unsigned grid = capped_grid(chunks, static_cast<int64_t>(device_cus()) * 8);          // 8 workgroups = 32 waves per CU
    {
        LaunchScope ls("grad_health", st, 4.0 * static_cast<double>(n));
        hipLaunchKernelGGL(grad_health_chunk_kernel, dim3(grid), dim3(kBlock), 0, st, static_cast<const float*>(grads), (long long)n,
                           reinterpret_cast<const long long*>(seg_end), n_seg, static_cast<double*>(workspace));
    }
    LaunchScope ls("grad_health_segments", st, 32.0 * static_cast<double>(chunks));
    hipLaunchKernelGGL(grad_health_segment_kernel, dim3(static_cast<unsigned>(n_seg)), dim3(kBlock), 0, st,
                       static_cast<const double*>(workspace), (long long)n, reinterpret_cast<const long long*>(seg_end), n_seg,
                       static_cast<double*>(record));
    return check_launch(fn);
}
