// bilinear.hpp -- the four taps of ATen's grid_sampler_2d (bilinear / zeros / align_corners=False) for one sampling position:
// shared by the warp kernels (warp.hip) and the fused sampling-correctness loss (sampling_correctness.hip).
#pragma once
#include "common.hpp"

namespace ffwm {

constexpr unsigned kOob = 0xFFFFFFF0u;

template <typename T>
struct Corners {
    unsigned off[4];   // nw, ne, sw, se byte offsets (kOob when outside the image)
    T w[4];            // matching weights (0 when outside)
    T dxw[2], dyw[2];  // (x1 - ix), (ix - x0), (y1 - iy), (iy - y0): for d(flow)
    bool valid[4];
};

// ATen grid_sampler_2d, bilinear / zeros / align_corners=False:
//   ix = ((gx + 1) * W_in - 1) / 2, corner weights from the opposite corner.
template <typename T>
__device__ __forceinline__ void make_corners(Corners<T>& c, T gx, T gy, int Hi, int Wi) {
    const T ix = ((gx + 1) * static_cast<T>(Wi) - 1) / 2;
    const T iy = ((gy + 1) * static_cast<T>(Hi) - 1) / 2;
    const T fx = floor_t(ix), fy = floor_t(iy);
    // corner indices as floats are exact for |f| < 2^24 (2^53); anything outside [-1, size] is
    // out of range on both corners anyway, so clamp before converting (NaN -> out of range).
    const T lim_x = static_cast<T>(Wi), lim_y = static_cast<T>(Hi);
    const bool okx = (fx >= static_cast<T>(-1)) && (fx <= lim_x);
    const bool oky = (fy >= static_cast<T>(-1)) && (fy <= lim_y);
    const int x0 = okx ? static_cast<int>(fx) : -2;
    const int y0 = oky ? static_cast<int>(fy) : -2;
    const int x1 = x0 + 1, y1 = y0 + 1;
    const T x1f = fx + 1, y1f = fy + 1;     // == (T)x1, (T)y1 whenever a corner is valid
    const bool finite = okx && oky;         // otherwise every corner is outside: all terms drop out
    c.dxw[0] = finite ? x1f - ix : static_cast<T>(0);
    c.dxw[1] = finite ? ix - fx : static_cast<T>(0);
    c.dyw[0] = finite ? y1f - iy : static_cast<T>(0);
    c.dyw[1] = finite ? iy - fy : static_cast<T>(0);
    const bool vx0 = x0 >= 0 && x0 < Wi, vx1 = x1 >= 0 && x1 < Wi;
    const bool vy0 = y0 >= 0 && y0 < Hi, vy1 = y1 >= 0 && y1 < Hi;
    c.valid[0] = vy0 && vx0;
    c.valid[1] = vy0 && vx1;
    c.valid[2] = vy1 && vx0;
    c.valid[3] = vy1 && vx1;
    const T w[4] = {c.dxw[0] * c.dyw[0], c.dxw[1] * c.dyw[0], c.dxw[0] * c.dyw[1], c.dxw[1] * c.dyw[1]};
    const int xs[4] = {x0, x1, x0, x1};
    const int ys[4] = {y0, y0, y1, y1};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        c.off[q] = c.valid[q] ? static_cast<unsigned>(ys[q] * Wi + xs[q]) * static_cast<unsigned>(sizeof(T)) : kOob;
        c.w[q] = c.valid[q] ? w[q] : static_cast<T>(0);
    }
}

}  // namespace ffwm
