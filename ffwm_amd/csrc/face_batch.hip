// face_batch.hip -- the input pipeline of the reference (data/face_dataset.py with --preload) from a DEVICE-RESIDENT store of bytes:
//   ffwm_face_batch    one launch gathers a whole training (or test) batch: img_S / img_F [B, 3, H, W], mask_S / mask_F [B, 1, H, W] as
//                      byte / 255 (a true division, as torch's .div(255)), flipped along W for an index >= P, lm_S / lm_F int64 [B, L, 2]
//                      from the plain or the flipped landmark table, gate [B, L, 1], invalid [B]
//   ffwm_face_gallery  the gallery planes: the channel mean ((r + g) + b) / 3 of byte / 255 (ffwm_identity_input's arithmetic, crop 0)
// The batch's indices are read from device memory: a captured launch follows the index vector it was captured on.
//
// One block of ffwm_face_batch owns one UNIT of one sample: a group of whole image rows of one side (S or F), or a chunk of landmarks.
//   * the rows of a group are contiguous in [N, H, W, 3] and in [N, H, W]: the block copies them as aligned dwords (bytes at the two
//     ragged ends: a row of 3 W bytes starts anywhere) into LDS at the same offset modulo 4, then every thread writes consecutive
//     floats of one CHW row group -- both sides of the transpose are coalesced;
//   * every output element has one owner thread and is written once, by a plain store; nothing else is written;
//   * an index outside [0, n_items), or a table row outside its table, is never turned into an address: that sample's outputs are zeros
//     and invalid[b] = 1.
#include "common.hpp"

namespace ffwm {
namespace {

constexpr int kGroupPixels = 1024;          // pixels of a row group (whole rows; one row when W is larger)
constexpr int kLmChunk = 1024;              // landmarks of a landmark unit
constexpr int kMaxSide = 8192;

struct FaceArgs {
    const unsigned char* images;            // [N, H, W, 3]
    const unsigned char* masks;             // [N, H, W], train only
    const int* pairs;                       // [P, 2]: rows of S and F in images / masks
    const int* pair_lm;                     // [P, 3]: rows of lm_S, lm_F in the landmark tables, row of the gate table; train only
    const int* lm;                          // [K, L, 2]
    const int* lm_flip;                     // [K, L, 2]
    const float* gate;                      // [KG, L]
    const int* index;                       // [B]
    float* img[2];                          // [B, 3, H, W]
    float* mask[2];                         // [B, 1, H, W]
    long long* lm_out[2];                   // [B, L, 2]
    float* gate_out;                        // [B, L, 1]
    int* invalid;                           // [B]
    long long N, K, KG;
    int P, n_items, H, W, L, train;
    int rows, groups, lm_chunks, units;     // rows per group, groups per plane, landmark units and all units per sample
};

// What sample b reads, or ok = false.  Every block of a sample decides alike: the inputs are not written during the launch.
struct Sample {
    bool ok, flip;
    int pair;
};
__device__ __forceinline__ Sample decode_sample(const FaceArgs& a, int b) {
    Sample s;
    const int i = a.index[b];
    s.ok = i >= 0 && i < a.n_items;
    s.flip = s.ok && i >= a.P;
    s.pair = s.ok ? (s.flip ? i - a.P : i) : 0;          // (train: n_items = 2 P, so i - P = i % P)
    return s;
}

// `len` bytes from src into LDS at dst + (src mod 4): whole aligned dwords, single bytes at the ragged ends.  Returns that shift.
__device__ __forceinline__ int stage_bytes(unsigned char* dst, const unsigned char* src, int len) {
    const int shift = static_cast<int>(reinterpret_cast<uintptr_t>(src) & 3u);
    int head = (4 - shift) & 3;
    head = head < len ? head : len;
    const int words = (len - head) >> 2, tail = len - head - 4 * words;
    const unsigned* src4 = reinterpret_cast<const unsigned*>(src + head);
    unsigned* dst4 = reinterpret_cast<unsigned*>(dst + shift + head);          // dst is 16-byte aligned and shift + head is 0 or 4
    for (int i = threadIdx.x; i < words; i += kBlock) dst4[i] = src4[i];
    if (static_cast<int>(threadIdx.x) < head) dst[shift + threadIdx.x] = src[threadIdx.x];
    if (static_cast<int>(threadIdx.x) < tail) dst[shift + head + 4 * words + threadIdx.x] = src[head + 4 * words + threadIdx.x];
    return shift;
}

__global__ void __launch_bounds__(kBlock) face_batch_kernel(const FaceArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const int b = blockIdx.x / a.units, unit = blockIdx.x - b * a.units;
    Sample s = decode_sample(a, b);
    int row_S = 0, row_F = 0, lm_rows[2] = {0, 0}, gate_row = 0;
    if (s.ok) {
        row_S = a.pairs[2 * s.pair];
        row_F = a.pairs[2 * s.pair + 1];
        s.ok = row_S >= 0 && row_S < a.N && row_F >= 0 && row_F < a.N;
        if (a.train) {
            lm_rows[0] = a.pair_lm[3 * s.pair];
            lm_rows[1] = a.pair_lm[3 * s.pair + 1];
            gate_row = a.pair_lm[3 * s.pair + 2];
            s.ok = s.ok && lm_rows[0] >= 0 && lm_rows[0] < a.K && lm_rows[1] >= 0 && lm_rows[1] < a.K && gate_row >= 0 && gate_row < a.KG;
        }
    }
    if (unit == 0 && threadIdx.x == 0) a.invalid[b] = s.ok ? 0 : 1;

    if (unit < 2 * a.groups) {
        // ---- a group of image rows of one side, and the same rows of its mask
        const int side = unit / a.groups, y0 = (unit - side * a.groups) * a.rows;
        const int rows = a.rows < a.H - y0 ? a.rows : a.H - y0;
        const int W = a.W, pixels = rows * W;
        const long long HW = static_cast<long long>(a.H) * W;
        float* img = a.img[side] + (static_cast<long long>(b) * 3 * a.H + y0) * W;          // channel c: + c HW
        float* mask = a.train ? a.mask[side] + (static_cast<long long>(b) * a.H + y0) * W : nullptr;
        if (!s.ok) {
            for (int i = threadIdx.x; i < pixels; i += kBlock) {
                img[i] = 0.f;
                img[HW + i] = 0.f;
                img[2 * HW + i] = 0.f;
                if (mask) mask[i] = 0.f;
            }
            return;
        }
        const long long first = (static_cast<long long>(side ? row_F : row_S) * a.H + y0) * W;          // first pixel of the group
        unsigned char* mstage = stage + 3 * pixels + 8;          // (behind the image bytes and their shift; rounded up below)
        mstage += (16 - (reinterpret_cast<uintptr_t>(mstage) & 15u)) & 15u;
        const unsigned char* px = stage + stage_bytes(stage, a.images + 3 * first, 3 * pixels);
        const unsigned char* mx = mask ? mstage + stage_bytes(mstage, a.masks + first, pixels) : nullptr;
        __syncthreads();
        for (int i = threadIdx.x; i < pixels; i += kBlock) {
            int p = i;
            if (s.flip) {
                const int r = i / W;
                p = r * W + (W - 1 - (i - r * W));
            }
            img[i] = static_cast<float>(px[3 * p]) / 255.0f;
            img[HW + i] = static_cast<float>(px[3 * p + 1]) / 255.0f;
            img[2 * HW + i] = static_cast<float>(px[3 * p + 2]) / 255.0f;
            if (mask) mask[i] = static_cast<float>(mx[p]) / 255.0f;
        }
        return;
    }

    // ---- a chunk of landmarks: lm_S, lm_F (int32 table -> int64) and the gate
    const int l0 = (unit - 2 * a.groups) * kLmChunk;
    const int n = kLmChunk < a.L - l0 ? kLmChunk : a.L - l0;
    const int* table = s.flip ? a.lm_flip : a.lm;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        long long* out = a.lm_out[side] + (static_cast<long long>(b) * a.L + l0) * 2;
        const int* src = table + (static_cast<long long>(lm_rows[side]) * a.L + l0) * 2;
        for (int i = threadIdx.x; i < 2 * n; i += kBlock) out[i] = s.ok ? static_cast<long long>(src[i]) : 0LL;
    }
    float* gout = a.gate_out + static_cast<long long>(b) * a.L + l0;
    const float* gsrc = a.gate + static_cast<long long>(gate_row) * a.L + l0;
    for (int i = threadIdx.x; i < n; i += kBlock) gout[i] = s.ok ? gsrc[i] : 0.f;
}

// One thread per output pixel; the three bytes of consecutive pixels are consecutive.
__global__ void __launch_bounds__(kBlock) face_gallery_kernel(const unsigned char* __restrict__ images, const int* __restrict__ rows,
                                                              float* __restrict__ out, long long N, long long HW, long long total) {
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * kBlock) {
        const long long g = i / HW, o = i - g * HW;
        const int row = rows[g];
        float v = 0.f;
        if (row >= 0 && row < N) {
            const unsigned char* p = images + 3 * (row * HW + o);
            float s = static_cast<float>(p[0]) / 255.0f;
            s += static_cast<float>(p[1]) / 255.0f;
            s += static_cast<float>(p[2]) / 255.0f;
            v = s / 3.0f;
        }
        out[i] = v;
    }
}

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_face_batch(const void* images, const void* masks, const void* pairs, const void* pair_lm, const void* lm,
                               const void* lm_flip, const void* gate, const void* index, void* img_S, void* img_F, void* mask_S,
                               void* mask_F, void* lm_S, void* lm_F, void* gate_out, void* invalid, int64_t N, int64_t H, int64_t W,
                               int64_t P, int64_t K, int64_t KG, int64_t L, int64_t B, int train, void* stream) {
    const char* fn = "ffwm_face_batch";
    FFWM_REQUIRE(train == 0 || train == 1, FFWM_ERR_ARG, "%s: train must be 0 or 1", fn);
    FFWM_REQUIRE(images && pairs && index && img_S && img_F && invalid, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(!train || (masks && pair_lm && lm && lm_flip && gate && mask_S && mask_F && lm_S && lm_F && gate_out), FFWM_ERR_ARG,
                 "%s: NULL tensor pointer (a training batch needs the masks, the landmark tables and their outputs)", fn);
    FFWM_REQUIRE(N > 0 && H > 0 && W > 0 && P > 0 && B > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(!train || (K > 0 && KG > 0 && L > 0), FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(H <= kMaxSide && W <= kMaxSide, FFWM_ERR_SIZE, "%s: H and W up to %d", fn, kMaxSide);
    FFWM_REQUIRE(N < (1LL << 31) && P < (1LL << 30) && B <= 65535 && (!train || (K < (1LL << 31) && KG < (1LL << 31) && L <= (1 << 20))),
                 FFWM_ERR_SIZE, "%s: tensor too large", fn);
    FaceArgs a;
    a.images = static_cast<const unsigned char*>(images);
    a.masks = static_cast<const unsigned char*>(masks);
    a.pairs = static_cast<const int*>(pairs);
    a.pair_lm = static_cast<const int*>(pair_lm);
    a.lm = static_cast<const int*>(lm);
    a.lm_flip = static_cast<const int*>(lm_flip);
    a.gate = static_cast<const float*>(gate);
    a.index = static_cast<const int*>(index);
    a.img[0] = static_cast<float*>(img_S);
    a.img[1] = static_cast<float*>(img_F);
    a.mask[0] = static_cast<float*>(mask_S);
    a.mask[1] = static_cast<float*>(mask_F);
    a.lm_out[0] = static_cast<long long*>(lm_S);
    a.lm_out[1] = static_cast<long long*>(lm_F);
    a.gate_out = static_cast<float*>(gate_out);
    a.invalid = static_cast<int*>(invalid);
    a.N = N;
    a.K = K;
    a.KG = KG;
    a.P = static_cast<int>(P);
    a.n_items = static_cast<int>(train ? 2 * P : P);
    a.H = static_cast<int>(H);
    a.W = static_cast<int>(W);
    a.L = train ? static_cast<int>(L) : 0;
    a.train = train;
    a.rows = static_cast<int>(W >= kGroupPixels ? 1 : (kGroupPixels / W < H ? kGroupPixels / W : H));
    a.groups = (a.H + a.rows - 1) / a.rows;
    a.lm_chunks = train ? (a.L + kLmChunk - 1) / kLmChunk : 0;
    a.units = 2 * a.groups + a.lm_chunks;
    // image bytes + their shift, the mask bytes + theirs, each region rounded up to 16 bytes: at most 4 * 8192 + 64 bytes
    const size_t lds = static_cast<size_t>(a.rows) * a.W * 4 + 64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double px = 2.0 * B * H * W;
    LaunchScope ls(train ? "face_batch" : "face_batch_test", st, px * (train ? 4.0 + 16.0 : 3.0 + 12.0) + (train ? 1.0 * B * L * (2 * 12.0 + 8.0) : 0.0));
    hipLaunchKernelGGL(face_batch_kernel, dim3(static_cast<unsigned>(B * a.units)), dim3(kBlock), lds, st, a);
    return check_launch(fn);
}

extern "C" int ffwm_face_gallery(const void* images, const void* rows, void* out, int64_t N, int64_t H, int64_t W, int64_t G,
                                 void* stream) {
    const char* fn = "ffwm_face_gallery";
    FFWM_REQUIRE(images && rows && out, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(N > 0 && H > 0 && W > 0 && G > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(H <= kMaxSide && W <= kMaxSide, FFWM_ERR_SIZE, "%s: H and W up to %d", fn, kMaxSide);
    FFWM_REQUIRE(N < (1LL << 31) && G < (1LL << 31) / (H * W), FFWM_ERR_SIZE, "%s: tensor too large", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = H * W, total = G * HW;
    LaunchScope ls("face_gallery", st, 7.0 * total);
    const int64_t blocks = (total + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(face_gallery_kernel, dim3(capped_grid(blocks, 1 << 16)), dim3(kBlock), 0, st,
                       static_cast<const unsigned char*>(images), static_cast<const int*>(rows), static_cast<float*>(out),
                       static_cast<long long>(N), static_cast<long long>(HW), static_cast<long long>(total));
    return check_launch(fn);
}
