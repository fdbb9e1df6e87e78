// Deformable convolution (DCNv1, mmcv.ops.DeformConv2dPack restricted to 3x3 / pad 1 / dilation 1 / deform_groups 1 / groups 1 /
// stride 1 | 2) of the ResNet bottleneck's conv2 (mmdet/models/backbones/resnet.py:174-197): the SAMPLING half.  The contraction with the
// weight is a 1x1 convolution over the 9 * C sampled columns and runs on the package's GEMM launches (kernels.deform_conv3x3_*).
//
//   erd_deform_cols      (x [N,IH,IW,C], offset [N,OH,OW,18]) -> col [N,OH,OW,9,C]
//   erd_deform_cols_bwd  (dcol, x, offset) -> dx += ..., doffset [N,OH,OW,18]
//
// The operator (mmcv is not pinned: DESIGN 8).  Tap t = 3 i + j of output pixel (oy, ox) samples x at
//   h = (float)(oy * s - 1 + i) + offset[2 t]        w = (float)(ox * s - 1 + j) + offset[2 t + 1]        (one fp32 addition each)
// The sample is 0 unless h > -1 && w > -1 && h < IH && w < IW, decided ON THE FLOATS (an offset of 3e9, an infinity or a NaN never
// becomes an index).  Inside: h0 = floor(h), ly = h - h0, hy = 1 - ly (w0, lx, hx alike); a corner whose row or column is outside the
// map contributes 0.  This file is compiled with -ffp-contract=off: the inside / floor decisions and the order below do not depend on
// contraction.
//
// Operation order, sampling (every product and sum rounds once, 7 roundings on the longest path):
//   w00 = hy * hx   w01 = hy * lx   w10 = ly * hx   w11 = ly * lx
//   col = ((w00 * x[h0][w0] + w01 * x[h0][w0+1]) + w10 * x[h0+1][w0]) + w11 * x[h0+1][w0+1]
// Operation order, backward (g = dcol[c]):
//   dx[corner][c] += g * w_corner                                               (one fp32 global atomic add per in-range corner)
//   d offset_y = sum_c g * (hx * (x10 - x00) + lx * (x11 - x01))                d offset_x = sum_c g * (hy * (x01 - x00) + ly * (x11 - x10))
//   each lane sums its channels c = lane, lane + 64, ... ascending, then the 64 lanes are folded by the xor butterfly 32, 16, .. 1.
//
// A wave owns one output pixel at a time; lanes run along the channels, so every corner load, every store and every atomic
// wave-instruction touches one contiguous 256-byte run of one pixel's channels.  The pixel index comes from the wave's number, so
// the position, the weights and the four corner offsets of a (pixel, tap) are wave-uniform: computed once per wave, branches on them
// are scalar.  col and doffset are written in full (outside samples store zeros) and depend on the shape alone: the same bits under
// any grid or CU reserve.  dx is a data-dependent scatter: float atomics, whose sums depend on the arrival order -- THE ONE PLACE IN
// THE PACKAGE where the last bits may differ from run to run.  dx accumulates onto what the buffer holds.
#include "erd_common.h"

#include <algorithm>

namespace {

constexpr int NT = 256, WAVES = NT / 64;

struct Geo {
    int N, IH, IW, OH, OW, C, stride;
};

// wave-uniform description of one (pixel, tap)
struct Tap {
    bool inside;
    bool ok00, ok01, ok10, ok11;
    float ly, lx, hy, hx;
    unsigned o00, o01, o10, o11;      // element offsets of the four corner pixels' channel 0 (< 2^31: the entry points check)
};

__device__ __forceinline__ Tap tap_of(const Geo& g, int n, int oy, int ox, int t, float offy, float offx) {
    Tap r;
    const float h = (float)(oy * g.stride - 1 + t / 3) + offy;
    const float w = (float)(ox * g.stride - 1 + t % 3) + offx;
    r.inside = h > -1.f && w > -1.f && h < (float)g.IH && w < (float)g.IW;
    r.ok00 = r.ok01 = r.ok10 = r.ok11 = false;
    r.ly = r.lx = r.hy = r.hx = 0.f;
    r.o00 = r.o01 = r.o10 = r.o11 = 0u;
    if (r.inside) {
        const float hf = floorf(h), wf = floorf(w);
        r.ly = h - hf;
        r.lx = w - wf;
        r.hy = 1.f - r.ly;
        r.hx = 1.f - r.lx;
        const int h0 = (int)hf, w0 = (int)wf;      // in [-1, IH - 1] x [-1, IW - 1]
        const bool r0 = h0 >= 0, r1 = h0 + 1 <= g.IH - 1, c0 = w0 >= 0, c1 = w0 + 1 <= g.IW - 1;
        r.ok00 = r0 && c0, r.ok01 = r0 && c1, r.ok10 = r1 && c0, r.ok11 = r1 && c1;
        const unsigned C = (unsigned)g.C, row = (unsigned)g.IW * C;
        const unsigned base = ((unsigned)n * g.IH + (unsigned)(r0 ? h0 : 0)) * row + (unsigned)(c0 ? w0 : 0) * C;
        r.o00 = base;
        r.o01 = base + (c0 ? C : 0u);
        r.o10 = base + (r0 ? row : 0u);
        r.o11 = r.o10 + (c0 ? C : 0u);
    }
    return r;
}

__device__ __forceinline__ void pixel_of(const Geo& g, unsigned p, int& n, int& oy, int& ox) {
    const unsigned r = p / (unsigned)g.OW;
    ox = (int)(p % (unsigned)g.OW);
    oy = (int)(r % (unsigned)g.OH);
    n = (int)(r / (unsigned)g.OH);
}

__global__ __launch_bounds__(NT) void deform_cols_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                         float* __restrict__ col, Geo g, unsigned npix) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)erd::uniform_int((int)(threadIdx.x >> 6));
    const unsigned step = gridDim.x * WAVES;
    for (unsigned p = blockIdx.x * WAVES + wave; p < npix; p += step) {
        int n, oy, ox;
        pixel_of(g, p, n, oy, ox);
        const float* op = offset + (size_t)p * 18;
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const Tap tp = tap_of(g, n, oy, ox, t, op[2 * t], op[2 * t + 1]);
            float* out = col + ((size_t)p * 9 + t) * g.C;
            if (!tp.inside) {
                for (int c = lane; c < g.C; c += 64) out[c] = 0.f;
                continue;
            }
            const float w00 = tp.hy * tp.hx, w01 = tp.hy * tp.lx, w10 = tp.ly * tp.hx, w11 = tp.ly * tp.lx;
            for (int c = lane; c < g.C; c += 64) {
                const float v00 = tp.ok00 ? x[tp.o00 + c] : 0.f;
                const float v01 = tp.ok01 ? x[tp.o01 + c] : 0.f;
                const float v10 = tp.ok10 ? x[tp.o10 + c] : 0.f;
                const float v11 = tp.ok11 ? x[tp.o11 + c] : 0.f;
                out[c] = ((w00 * v00 + w01 * v01) + w10 * v10) + w11 * v11;
            }
        }
    }
}

__global__ __launch_bounds__(NT) void deform_cols_bwd_kernel(const float* __restrict__ dcol, const float* __restrict__ x,
                                                             const float* __restrict__ offset, float* __restrict__ dx,
                                                             float* __restrict__ doffset, Geo g, unsigned npix) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)erd::uniform_int((int)(threadIdx.x >> 6));
    const unsigned step = gridDim.x * WAVES;
    for (unsigned p = blockIdx.x * WAVES + wave; p < npix; p += step) {
        int n, oy, ox;
        pixel_of(g, p, n, oy, ox);
        const float* op = offset + (size_t)p * 18;
        float mine = 0.f;      // lane l < 18 ends up with d offset[l] of this pixel
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const Tap tp = tap_of(g, n, oy, ox, t, op[2 * t], op[2 * t + 1]);
            if (!tp.inside) continue;      // no sample: no gradient to x, zero to the offsets
            const float w00 = tp.hy * tp.hx, w01 = tp.hy * tp.lx, w10 = tp.ly * tp.hx, w11 = tp.ly * tp.lx;
            const float* gp = dcol + ((size_t)p * 9 + t) * g.C;
            float gy = 0.f, gx = 0.f;
            for (int c = lane; c < g.C; c += 64) {
                const float gv = gp[c];
                const float v00 = tp.ok00 ? x[tp.o00 + c] : 0.f;
                const float v01 = tp.ok01 ? x[tp.o01 + c] : 0.f;
                const float v10 = tp.ok10 ? x[tp.o10 + c] : 0.f;
                const float v11 = tp.ok11 ? x[tp.o11 + c] : 0.f;
                if (tp.ok00) atomicAdd(dx + tp.o00 + c, gv * w00);
                if (tp.ok01) atomicAdd(dx + tp.o01 + c, gv * w01);
                if (tp.ok10) atomicAdd(dx + tp.o10 + c, gv * w10);
                if (tp.ok11) atomicAdd(dx + tp.o11 + c, gv * w11);
                gy += gv * (tp.hx * (v10 - v00) + tp.lx * (v11 - v01));
                gx += gv * (tp.hy * (v01 - v00) + tp.ly * (v11 - v10));
            }
            const float sy = erd::wave_sum(gy), sx = erd::wave_sum(gx);
            if (lane == 2 * t) mine = sy;
            if (lane == 2 * t + 1) mine = sx;
        }
        if (lane < 18) doffset[(size_t)p * 18 + lane] = mine;
    }
}

int num_cus_deform() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// shape rules shared by the two entries; 0 when the launch is in scope
int check_shape(const char* what, int N, int IH, int IW, int C, int stride, Geo& g) {
    if (N <= 0 || IH <= 0 || IW <= 0 || C <= 0) {
        erd::set_error("%s: empty map (N %d, %d x %d, C %d)", what, N, IH, IW, C);
        return ERD_EINVAL;
    }
    if (C % 4 != 0) {
        erd::set_error("%s: C = %d is not a multiple of 4 (16-byte pixel rows)", what, C);
        return ERD_EUNSUPPORTED;
    }
    if (stride != 1 && stride != 2) {
        erd::set_error("%s: stride %d; supported: 1, 2", what, stride);
        return ERD_EUNSUPPORTED;
    }
    g = Geo{N, IH, IW, (IH - 1) / stride + 1, (IW - 1) / stride + 1, C, stride};
    // element offsets are 32-bit in the kernels: x, col (the largest) and offset; IH and IW convert to fp32 exactly
    const int64_t npix = (int64_t)N * g.OH * g.OW;
    if ((int64_t)N * IH * IW * C >= (1ll << 31) || npix * 9 * C >= (1ll << 31) || IH >= (1 << 24) || IW >= (1 << 24)) {
        erd::set_error("%s: map too large for 32-bit element offsets (N %d, %d x %d, C %d)", what, N, IH, IW, C);
        return ERD_EUNSUPPORTED;
    }
    return 0;
}

// a persistent grid: at most eight workgroups (32 waves) per usable CU, each wave striding over the pixels
unsigned grid_of(unsigned npix) {
    const unsigned want = (npix + WAVES - 1) / WAVES, cap = 8u * (unsigned)erd::usable_cus(num_cus_deform());
    return std::max(1u, std::min(want, cap));
}

}  // namespace

// replaces: the sampling (deformable im2col) of mmcv.ops.DeformConv2dPack.forward as built by resnet.py:174-197 (conv2 of a Bottleneck with dcn=...)
extern "C" int erd_deform_cols(const float* x, const float* offset, float* col, int N, int IH, int IW, int C, int stride,
                               erd_stream_t stream) {
    const char* what = "erd_deform_cols";
    Geo g;
    const int rc = check_shape(what, N, IH, IW, C, stride, g);
    if (rc) return rc;
    ERD_REQUIRE(x && offset && col, "%s: null x / offset / col", what);
    ERD_REQUIRE(aligned16(x) && aligned16(col) && aligned16(offset), "%s: pointers must be 16-byte aligned", what);
    const unsigned npix = (unsigned)((int64_t)N * g.OH * g.OW);
    hipLaunchKernelGGL(deform_cols_kernel, dim3(grid_of(npix)), dim3(NT), 0, (hipStream_t)stream, x, offset, col, g, npix);
    return erd::check_launch(what);
}

// replaces: the backward of that call site (deformable col2im and col2im_coord of mmcv's DeformConv2dFunction.backward)
extern "C" int erd_deform_cols_bwd(const float* dcol, const float* x, const float* offset, float* dx, float* doffset, int N, int IH,
                                   int IW, int C, int stride, erd_stream_t stream) {
    const char* what = "erd_deform_cols_bwd";
    Geo g;
    const int rc = check_shape(what, N, IH, IW, C, stride, g);
    if (rc) return rc;
    ERD_REQUIRE(dcol && x && offset && dx && doffset, "%s: null dcol / x / offset / dx / doffset", what);
    ERD_REQUIRE(aligned16(dcol) && aligned16(x) && aligned16(offset) && aligned16(dx) && aligned16(doffset),
                "%s: pointers must be 16-byte aligned", what);
    ERD_REQUIRE(dx != x, "%s: dx must not alias x", what);
    const unsigned npix = (unsigned)((int64_t)N * g.OH * g.OW);
    hipLaunchKernelGGL(deform_cols_bwd_kernel, dim3(grid_of(npix)), dim3(NT), 0, (hipStream_t)stream, dcol, x, offset, dx, doffset, g,
                       npix);
    return erd::check_launch(what);
}
