// face_batch.hip -- the input pipeline of the reference (data/face_dataset.py with --preload) from a DEVICE-RESIDENT store of bytes:
//   ffwm_face_batch    one launch gathers a whole training (or test) batch: img_S / img_F [B, 3, H, W], mask_S / mask_F [B, 1, H, W] as
//                      byte / 255 (a true division, as torch's .div(255)), flipped along W for an index >= P, lm_S / lm_F int64 [B, L, 2]
//                      from the plain or the flipped landmark table, gate [B, L, 1], invalid [B]
//   ffwm_face_batch_aug  the same training batch with the S side rotated by a whole angle per sample (the rotation of --aug, stated as
//                      cv2.warpAffine's fixed-point bilinear path; see the second half of this file)
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
#include <algorithm>

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

// The table rows of sample s (clears s.ok where one lies outside its table).
struct Rows {
    int img_S, img_F, lm_S, lm_F, gate;
};
__device__ __forceinline__ Rows sample_rows(const FaceArgs& a, Sample& s) {
    Rows r = {0, 0, 0, 0, 0};
    if (s.ok) {
        r.img_S = a.pairs[2 * s.pair];
        r.img_F = a.pairs[2 * s.pair + 1];
        s.ok = r.img_S >= 0 && r.img_S < a.N && r.img_F >= 0 && r.img_F < a.N;
        if (a.train) {
            r.lm_S = a.pair_lm[3 * s.pair];
            r.lm_F = a.pair_lm[3 * s.pair + 1];
            r.gate = a.pair_lm[3 * s.pair + 2];
            s.ok = s.ok && r.lm_S >= 0 && r.lm_S < a.K && r.lm_F >= 0 && r.lm_F < a.K && r.gate >= 0 && r.gate < a.KG;
        }
    }
    return r;
}

// ---- a group of image rows of one side, and the same rows of its mask
__device__ __forceinline__ void copy_row_group(const FaceArgs& a, const Sample& s, const Rows& r, int b, int side, int group,
                                               unsigned char* stage) {
    const int y0 = group * a.rows;
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
    const long long first = (static_cast<long long>(side ? r.img_F : r.img_S) * a.H + y0) * W;          // first pixel of the group
    unsigned char* mstage = stage + 3 * pixels + 8;          // (behind the image bytes and their shift; rounded up below)
    mstage += (16 - (reinterpret_cast<uintptr_t>(mstage) & 15u)) & 15u;
    const unsigned char* px = stage + stage_bytes(stage, a.images + 3 * first, 3 * pixels);
    const unsigned char* mx = mask ? mstage + stage_bytes(mstage, a.masks + first, pixels) : nullptr;
    __syncthreads();
    for (int i = threadIdx.x; i < pixels; i += kBlock) {
        int p = i;
        if (s.flip) {
            const int row = i / W;
            p = row * W + (W - 1 - (i - row * W));
        }
        img[i] = static_cast<float>(px[3 * p]) / 255.0f;
        img[HW + i] = static_cast<float>(px[3 * p + 1]) / 255.0f;
        img[2 * HW + i] = static_cast<float>(px[3 * p + 2]) / 255.0f;
        if (mask) mask[i] = static_cast<float>(mx[p]) / 255.0f;
    }
}

// ---- a chunk of landmarks: lm_S, lm_F (int32 table -> int64; the sides from kFirstSide on) and the gate
template <int kFirstSide>
__device__ __forceinline__ void copy_landmark_chunk(const FaceArgs& a, const Sample& s, const Rows& r, int b, int l0, int n) {
    const int* table = s.flip ? a.lm_flip : a.lm;
#pragma unroll
    for (int side = kFirstSide; side < 2; ++side) {
        long long* out = a.lm_out[side] + (static_cast<long long>(b) * a.L + l0) * 2;
        const int* src = table + (static_cast<long long>(side ? r.lm_F : r.lm_S) * a.L + l0) * 2;
        for (int i = threadIdx.x; i < 2 * n; i += kBlock) out[i] = s.ok ? static_cast<long long>(src[i]) : 0LL;
    }
    float* gout = a.gate_out + static_cast<long long>(b) * a.L + l0;
    const float* gsrc = a.gate + static_cast<long long>(r.gate) * a.L + l0;
    for (int i = threadIdx.x; i < n; i += kBlock) gout[i] = s.ok ? gsrc[i] : 0.f;
}

__global__ void __launch_bounds__(kBlock) face_batch_kernel(const FaceArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const int b = blockIdx.x / a.units, unit = blockIdx.x - b * a.units;
    Sample s = decode_sample(a, b);
    const Rows r = sample_rows(a, s);
    if (unit == 0 && threadIdx.x == 0) a.invalid[b] = s.ok ? 0 : 1;
    if (unit < 2 * a.groups) {
        const int side = unit / a.groups;
        copy_row_group(a, s, r, b, side, unit - side * a.groups, stage);
        return;
    }
    const int l0 = (unit - 2 * a.groups) * kLmChunk;
    copy_landmark_chunk<0>(a, s, r, b, l0, kLmChunk < a.L - l0 ? kLmChunk : a.L - l0);
}

// ---------------------------------------------------------------------------------------------------------------- the rotation of --aug
// ffwm_face_batch_aug: the same batch with the S side rotated by a whole angle per sample, as cv2.warpAffine's bilinear path states
// it (ffwm_amd/data.py: rotation_tables, warp_affine_linear, rotate_landmarks).  Everything that needs floating point on the image
// half -- the four fixed-point tables of an angle -- is made on the host once per angle and image size; the kernel is integer
// arithmetic up to the exact float(S) / 1024 and the division by 255.  The F side, lm_F and the gate are the units above, unchanged.
struct FaceAugArgs {
    FaceArgs f;
    const float* lm_raw;                    // [K, L, 2]: the landmark rows before .long(), as float32
    const float* lm_raw_flip;               // [K, L, 2]
    const int* slot;                        // [B]: angle slot of every sample
    const int* xtab;                        // [A, 2, W]: adelta, bdelta
    const int* ytab;                        // [A, 2, H]: X0, Y0
    const float* cs;                        // [A, 2]: float32 cos and sin of -angle
    int A, load_size;
    int lds_bytes;                          // dynamic LDS of the launch: a window of source rows up to this size is staged
};

__device__ __forceinline__ int wrap_add(int x, int y) {          // (tables are the caller's: no overflow is undefined)
    return static_cast<int>(static_cast<unsigned>(x) + static_cast<unsigned>(y));
}

// Output rows [y0, y0 + rows) of the rotated S side.  px / mx: the image and mask bytes of source rows [ry0, ry1] (in LDS, or the
// whole planes in global memory with ry0 = 0, ry1 = H - 1); a tap outside them or outside [0, W) counts 0 and is not read.  The
// flip comes BEFORE the rotation: column tx of the flipped image is column W - 1 - tx of the stored one.
__device__ __forceinline__ void rotate_rows(const FaceArgs& a, bool flip, int y0, int pixels, const int* __restrict__ xt,
                                            const int* __restrict__ yt, const unsigned char* px, const unsigned char* mx, int ry0, int ry1,
                                            float* __restrict__ img, float* __restrict__ mask) {
    const int W = a.W, H = a.H;
    const long long HW = static_cast<long long>(H) * W;
    for (int i = threadIdx.x; i < pixels; i += kBlock) {
        const int row = i / W, x = i - row * W, y = y0 + row;
        const int X = wrap_add(yt[y], xt[x]) >> 5, Y = wrap_add(yt[H + y], xt[W + x]) >> 5;
        const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
        const int w[4] = {(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy};          // sum to 1024
        int S[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ty = sy + (t >> 1), tx = sx + (t & 1);
            if (tx >= 0 && tx < W && ty >= ry0 && ty <= ry1) {
                const int o = (ty - ry0) * W + (flip ? W - 1 - tx : tx);
                S[0] += w[t] * px[3 * o];
                S[1] += w[t] * px[3 * o + 1];
                S[2] += w[t] * px[3 * o + 2];
                S[3] += w[t] * mx[o];
            }
        }
        // S <= 255 * 1024 < 2^24: float(S) and S / 1024 are exact; the division by 255 is a true one
        img[i] = static_cast<float>(S[0]) * 0.0009765625f / 255.0f;
        img[HW + i] = static_cast<float>(S[1]) * 0.0009765625f / 255.0f;
        img[2 * HW + i] = static_cast<float>(S[2]) * 0.0009765625f / 255.0f;
        mask[i] = S[3] > 0 ? 1.f : 0.f;          // mask_aug[mask_aug > 0] = 255, then / 255
    }
}

__global__ void __launch_bounds__(kBlock) face_batch_aug_kernel(const FaceAugArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char stage[];
    const FaceArgs& a = g.f;
    const int b = blockIdx.x / a.units, unit = blockIdx.x - b * a.units;
    Sample s = decode_sample(a, b);
    const Rows r = sample_rows(a, s);
    const int slot = g.slot[b];
    s.ok = s.ok && slot >= 0 && slot < g.A;
    if (unit == 0 && threadIdx.x == 0) a.invalid[b] = s.ok ? 0 : 1;

    if (unit >= a.groups && unit < 2 * a.groups) {          // the F side
        copy_row_group(a, s, r, b, 1, unit - a.groups, stage);
        return;
    }
    if (unit < a.groups) {
        if (!s.ok) {
            copy_row_group(a, s, r, b, 0, unit, stage);          // (zeros)
            return;
        }
        // ---- a group of rows of the rotated S side
        const int H = a.H, W = a.W, y0 = unit * a.rows;
        const int rows = a.rows < H - y0 ? a.rows : H - y0, y1 = y0 + rows - 1;
        const int* xt = g.xtab + static_cast<long long>(slot) * 2 * W;
        const int* yt = g.ytab + static_cast<long long>(slot) * 2 * H;
        float* img = a.img[0] + (static_cast<long long>(b) * 3 * H + y0) * W;
        float* mask = a.mask[0] + (static_cast<long long>(b) * H + y0) * W;
        const long long plane = static_cast<long long>(r.img_S) * H * W;
        // Y0[y] + bdelta[x] is a sum of two monotone tables: over the group it lies between its values at the four corners, and so
        // do the source rows sy = that >> 10 (+ 1 for the lower taps).  Tables that are not monotone cost pixels, never an address.
        const int ya = yt[H + y0], yb = yt[H + y1], ba = xt[W], bb = xt[W + W - 1];
        const int lo = wrap_add(ya < yb ? ya : yb, ba < bb ? ba : bb) >> 10, hi = wrap_add(ya > yb ? ya : yb, ba > bb ? ba : bb) >> 10;
        const int ry0 = lo > 0 ? lo : 0, ry1 = hi < H - 2 ? hi + 1 : H - 1;
        const long long window = ry1 >= ry0 ? static_cast<long long>(ry1 - ry0 + 1) * W : 0;          // pixels of the source rows
        if (window > 0 && 4 * window + 64 <= g.lds_bytes) {
            // whole source rows are contiguous: staged as the plain copy stages its rows
            const int wp = static_cast<int>(window);
            const long long first = plane + static_cast<long long>(ry0) * W;
            unsigned char* mstage = stage + 3 * wp + 8;
            mstage += (16 - (reinterpret_cast<uintptr_t>(mstage) & 15u)) & 15u;
            const unsigned char* px = stage + stage_bytes(stage, a.images + 3 * first, 3 * wp);
            const unsigned char* mx = mstage + stage_bytes(mstage, a.masks + first, wp);
            __syncthreads();
            rotate_rows(a, s.flip, y0, rows * W, xt, yt, px, mx, ry0, ry1, img, mask);
        } else {
            // a window beyond the LDS of the launch (very wide images, large angles): the taps come from global memory
            rotate_rows(a, s.flip, y0, rows * W, xt, yt, a.images + 3 * plane, a.masks + plane, 0, H - 1, img, mask);
        }
        return;
    }

    // ---- a chunk of landmarks: lm_S by the reference's float32 chain (every product and sum rounded on its own), lm_F and the gate
    const int l0 = (unit - 2 * a.groups) * kLmChunk;
    const int n = kLmChunk < a.L - l0 ? kLmChunk : a.L - l0;
    copy_landmark_chunk<1>(a, s, r, b, l0, n);
    long long* out = a.lm_out[0] + (static_cast<long long>(b) * a.L + l0) * 2;
    if (!s.ok) {
        for (int i = threadIdx.x; i < 2 * n; i += kBlock) out[i] = 0LL;
        return;
    }
    const float* raw = (s.flip ? g.lm_raw_flip : g.lm_raw) + (static_cast<long long>(r.lm_S) * a.L + l0) * 2;
    const float c = g.cs[2 * slot], sn = g.cs[2 * slot + 1], h = static_cast<float>(g.load_size / 2), top = static_cast<float>(g.load_size);
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const float x0 = __fsub_rn(raw[2 * i], h), y0 = __fsub_rn(raw[2 * i + 1], h);
        const float v[2] = {__fadd_rn(__fsub_rn(__fmul_rn(x0, c), __fmul_rn(y0, sn)), h),
                            __fadd_rn(__fadd_rn(__fmul_rn(x0, sn), __fmul_rn(y0, c)), h)};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float clipped = fminf(fmaxf(v[k], 0.f), top);          // np.clip(lm_aug, 0, load_size): in [0, load_size], never NaN
            const long long t = static_cast<long long>(clipped);         // .long()
            out[2 * i + k] = t < g.load_size - 1 ? t : g.load_size - 1;  // clamp(0, load_size - 1)
        }
    }
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

// The argument checks both batch entry points share, then the arguments and the unit geometry of the launch.
int face_args(const char* fn, FaceArgs& a, const void* images, const void* masks, const void* pairs, const void* pair_lm, const void* lm,
              const void* lm_flip, const void* gate, const void* index, void* img_S, void* img_F, void* mask_S, void* mask_F, void* lm_S,
              void* lm_F, void* gate_out, void* invalid, int64_t N, int64_t H, int64_t W, int64_t P, int64_t K, int64_t KG, int64_t L,
              int64_t B, int train) {
    FFWM_REQUIRE(train == 0 || train == 1, FFWM_ERR_ARG, "%s: train must be 0 or 1", fn);
    FFWM_REQUIRE(images && pairs && index && img_S && img_F && invalid, FFWM_ERR_ARG, "%s: NULL tensor pointer", fn);
    FFWM_REQUIRE(!train || (masks && pair_lm && lm && lm_flip && gate && mask_S && mask_F && lm_S && lm_F && gate_out), FFWM_ERR_ARG,
                 "%s: NULL tensor pointer (a training batch needs the masks, the landmark tables and their outputs)", fn);
    FFWM_REQUIRE(N > 0 && H > 0 && W > 0 && P > 0 && B > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(!train || (K > 0 && KG > 0 && L > 0), FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(H <= kMaxSide && W <= kMaxSide, FFWM_ERR_SIZE, "%s: H and W up to %d", fn, kMaxSide);
    FFWM_REQUIRE(N < (1LL << 31) && P < (1LL << 30) && B <= 65535 && (!train || (K < (1LL << 31) && KG < (1LL << 31) && L <= (1 << 20))),
                 FFWM_ERR_SIZE, "%s: tensor too large", fn);
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
    return FFWM_OK;
}

// image bytes + their shift, the mask bytes + theirs, each region rounded up to 16 bytes: at most 4 * 8192 + 64 bytes
size_t row_group_lds(const FaceArgs& a) { return static_cast<size_t>(a.rows) * a.W * 4 + 64; }

// The LDS of a rotated launch: room for a window of 8192 source pixels (image and mask bytes), which is the most a plain row group
// takes as well.  At 128 x 128 a group of 8 rows under +-5 degrees reads about 22 rows, 11 KiB; a window that does not fit takes the
// global-tap route, block by block: a large angle, or a wide image, where a group is one row whose taps under any angle but 0 span
// many source rows (8 x 2048: all 8 rows, 64 KiB; at angle 0 two rows, staged).  Measured at batch 8, 128 x 128, +-5 degrees, device
// time in a captured graph, builds that differ in this constant only: 32 KiB 6.86 us, 16 KiB 6.84 us (the LDS a block reserves costs
// nothing measurable: the grid is about one block per CU), 0 -- every rotated block on global taps -- 7.18 us.  So windows are
// staged, and the budget is the larger one, which serves angles up to about 25 degrees at 128 x 128.
constexpr size_t kAugLds = 4 * 8192 + 64;

}  // namespace
}  // namespace ffwm

using namespace ffwm;

extern "C" int ffwm_face_batch(const void* images, const void* masks, const void* pairs, const void* pair_lm, const void* lm,
                               const void* lm_flip, const void* gate, const void* index, void* img_S, void* img_F, void* mask_S,
                               void* mask_F, void* lm_S, void* lm_F, void* gate_out, void* invalid, int64_t N, int64_t H, int64_t W,
                               int64_t P, int64_t K, int64_t KG, int64_t L, int64_t B, int train, void* stream) {
    const char* fn = "ffwm_face_batch";
    FaceArgs a;
    const int rc = face_args(fn, a, images, masks, pairs, pair_lm, lm, lm_flip, gate, index, img_S, img_F, mask_S, mask_F, lm_S, lm_F,
                             gate_out, invalid, N, H, W, P, K, KG, L, B, train);
    if (rc != FFWM_OK) return rc;
    const size_t lds = row_group_lds(a);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double px = 2.0 * B * H * W;
    LaunchScope ls(train ? "face_batch" : "face_batch_test", st, px * (train ? 4.0 + 16.0 : 3.0 + 12.0) + (train ? 1.0 * B * L * (2 * 12.0 + 8.0) : 0.0));
    hipLaunchKernelGGL(face_batch_kernel, dim3(static_cast<unsigned>(B * a.units)), dim3(kBlock), lds, st, a);
    return check_launch(fn);
}

extern "C" int ffwm_face_batch_aug(const void* images, const void* masks, const void* pairs, const void* pair_lm, const void* lm,
                                   const void* lm_flip, const void* gate, const void* index, const void* lm_raw, const void* lm_raw_flip,
                                   const void* slot, const void* xtab, const void* ytab, const void* cs, void* img_S, void* img_F,
                                   void* mask_S, void* mask_F, void* lm_S, void* lm_F, void* gate_out, void* invalid, int64_t N, int64_t H,
                                   int64_t W, int64_t P, int64_t K, int64_t KG, int64_t L, int64_t B, int64_t A, int64_t load_size,
                                   int train, void* stream) {
    const char* fn = "ffwm_face_batch_aug";
    FFWM_REQUIRE(train == 1, FFWM_ERR_ARG, "%s: train must be 1 (only a training batch is rotated)", fn);
    FFWM_REQUIRE(lm_raw && lm_raw_flip && slot && xtab && ytab && cs, FFWM_ERR_ARG,
                 "%s: NULL tensor pointer (a rotated batch needs the raw landmark tables, the angle slots and the angle tables)", fn);
    FFWM_REQUIRE(load_size > 0, FFWM_ERR_ARG, "%s: sizes must be positive", fn);
    FFWM_REQUIRE(A >= 1 && A <= 64, FFWM_ERR_ARG, "%s: A (angle slots) must be 1 to 64", fn);
    FFWM_REQUIRE(load_size <= (1 << 24), FFWM_ERR_SIZE, "%s: load_size up to 2^24 (exact in float32)", fn);
    FaceAugArgs g;
    const int rc = face_args(fn, g.f, images, masks, pairs, pair_lm, lm, lm_flip, gate, index, img_S, img_F, mask_S, mask_F, lm_S, lm_F,
                             gate_out, invalid, N, H, W, P, K, KG, L, B, train);
    if (rc != FFWM_OK) return rc;
    g.lm_raw = static_cast<const float*>(lm_raw);
    g.lm_raw_flip = static_cast<const float*>(lm_raw_flip);
    g.slot = static_cast<const int*>(slot);
    g.xtab = static_cast<const int*>(xtab);
    g.ytab = static_cast<const int*>(ytab);
    g.cs = static_cast<const float*>(cs);
    g.A = static_cast<int>(A);
    g.load_size = static_cast<int>(load_size);
    const size_t whole = static_cast<size_t>(H) * W * 4 + 64, plain = row_group_lds(g.f);
    const size_t lds = std::max(plain, std::min(whole, kAugLds));          // (no window is larger than the whole plane)
    g.lds_bytes = static_cast<int>(lds);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LaunchScope ls("face_batch_aug", st, 2.0 * B * H * W * (4.0 + 16.0) + 1.0 * B * L * (2 * 12.0 + 8.0));
    hipLaunchKernelGGL(face_batch_aug_kernel, dim3(static_cast<unsigned>(B * g.f.units)), dim3(kBlock), lds, st, g);
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
