// IoULoss / DIoULoss / CIoULoss of one box pair (mmdet/models/losses/iou_loss.py:16-54, 130-181, 185-246): the loss value, its
// gradient w.r.t. the predicted box (x1, y1, x2, y2) as torch autograd forms it, and the plain bbox_overlaps IoU (the QFL score).
// Shared by the fused step kernel (losses.hip, gfl_losses_kernel) and the stand-alone operator (leaf_ops.hip, erd_iou_loss); both
// files are built with -ffp-contract=off, so the expressions below are evaluated operation by operation in fp32.
//
// Gradient rules (torch autograd): max / min split the gradient 1/2 : 1/2 on ties; clamp(min=0) and ious.clamp(min=eps) pass it
// where the argument is >= the bound; clamp(-1, 1) passes it inside the closed interval; CIoU's alpha is detached.
// No guard is added where the reference's own fp32 evaluation is not finite (CIoU on two identical boxes: alpha = 0 / 0).
#ifndef ERD_BOX_LOSS_H_
#define ERD_BOX_LOSS_H_
#include "erd_common.h"

namespace erd {
namespace box {

__device__ __forceinline__ float gmax_a(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }   // d max(a, b) / da
__device__ __forceinline__ float gmin_a(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }   // d min(a, b) / da

// overlap, the raw union ap + ag - overlap and their partials w.r.t. the predicted box
struct Inter {
    float ov, uni0;
    float dov[4], da1[4];
};

__device__ __forceinline__ Inter intersect(const float4 p, const float4 t) {
    Inter r;
    const float pw = p.z - p.x, ph = p.w - p.y;
    const float area1 = pw * ph, area2 = (t.z - t.x) * (t.w - t.y);
    const float w0 = fminf(p.z, t.z) - fmaxf(p.x, t.x), h0 = fminf(p.w, t.w) - fmaxf(p.y, t.y);
    const float w = fmaxf(w0, 0.f), h = fmaxf(h0, 0.f);
    r.ov = w * h;
    r.uni0 = area1 + area2 - r.ov;
    const float cw = w0 >= 0.f ? 1.f : 0.f, ch = h0 >= 0.f ? 1.f : 0.f;            // clamp(min=0) passes the gradient at >=
    r.dov[0] = -gmax_a(p.x, t.x) * cw * h;
    r.dov[1] = -gmax_a(p.y, t.y) * ch * w;
    r.dov[2] = gmin_a(p.z, t.z) * cw * h;
    r.dov[3] = gmin_a(p.w, t.w) * ch * w;
    r.da1[0] = -ph; r.da1[1] = -pw; r.da1[2] = ph; r.da1[3] = pw;
    return r;
}

// bbox_overlaps(pred, target, is_aligned=True): the union is clamped at the function's own 1e-6 (bbox_overlaps.py:151-199)
__device__ __forceinline__ float plain_iou(const Inter& it) { return it.ov / fmaxf(it.uni0, 1e-6f); }

// IoULoss: ious = bbox_overlaps(...).clamp(min=eps); MODE 0: -log(ious), 1: 1 - ious, 2: 1 - ious^2
template <int MODE>
__device__ __forceinline__ float iou_loss_grad(const float4 p, const float4 t, float eps, float* g /*[4] or null*/, float* iou_out) {
    const Inter it = intersect(p, t);
    const float uni = fmaxf(it.uni0, 1e-6f);
    const float iou = it.ov / uni;
    const float ic = fmaxf(iou, eps);
    if (iou_out) *iou_out = iou;
    if (g) {
        const float cu = it.uni0 > 1e-6f ? 1.f : (it.uni0 == 1e-6f ? 0.5f : 0.f);
        const float pass = iou >= eps ? 1.f : 0.f;
        // d loss / d ious
        const float dl = MODE == 0 ? -1.0f / ic : (MODE == 1 ? -1.0f : -2.0f * ic);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float duni = (it.da1[q] - it.dov[q]) * cu;
            const float diou = it.dov[q] / uni - it.ov / (uni * uni) * duni;
            g[q] = dl * pass * diou;
        }
    }
    return MODE == 0 ? -logf(ic) : (MODE == 1 ? 1.0f - ic : 1.0f - ic * ic);
}

// DIoULoss (CIOU == false) and CIoULoss (CIOU == true): eps is ADDED to the union, to c2 and (CIoU) to both heights
template <bool CIOU>
__device__ __forceinline__ float diou_loss_grad(const float4 p, const float4 t, float eps, float* g /*[4] or null*/, float* iou_out) {
    const Inter it = intersect(p, t);
    if (iou_out) *iou_out = plain_iou(it);
    const float uni = it.uni0 + eps;
    const float ious = it.ov / uni;
    const float ew0 = fmaxf(p.z, t.z) - fminf(p.x, t.x), eh0 = fmaxf(p.w, t.w) - fminf(p.y, t.y);
    const float cw = fmaxf(ew0, 0.f), ch = fmaxf(eh0, 0.f);
    const float c2 = cw * cw + ch * ch + eps;
    const float sx = (t.x + t.z) - (p.x + p.z), sy = (t.y + t.w) - (p.y + p.w);
    const float rho2 = sx * sx / 4.0f + sy * sy / 4.0f;
    float v = 0.f, alpha = 0.f, dat = 0.f, w1 = 0.f, h1 = 1.f, r1 = 0.f;
    if (CIOU) {
        w1 = p.z - p.x;
        h1 = p.w - p.y + eps;
        const float w2 = t.z - t.x, h2 = t.w - t.y + eps;
        r1 = w1 / h1;
        dat = atanf(w2 / h2) - atanf(r1);
        v = 0.40528473456935109f * (dat * dat);                                        // 4 / pi^2
        alpha = (ious > 0.5f ? 1.f : 0.f) * v / (1.0f - ious + v);                     // detached
    }
    const float cious = ious - (rho2 / c2 + alpha * v);
    if (g) {
        const float pew = ew0 >= 0.f ? 1.f : 0.f, peh = eh0 >= 0.f ? 1.f : 0.f;
        const float dcw[4] = {-gmin_a(p.x, t.x) * pew, 0.f, gmax_a(p.z, t.z) * pew, 0.f};
        const float dch[4] = {0.f, -gmin_a(p.y, t.y) * peh, 0.f, gmax_a(p.w, t.w) * peh};
        const float drho[4] = {-sx / 2.0f, -sy / 2.0f, -sx / 2.0f, -sy / 2.0f};
        const float pass = CIOU ? ((cious >= -1.0f && cious <= 1.0f) ? 1.f : 0.f) : 1.f;
        // d v / d (w1 / h1) = -2 factor (atan(w2/h2) - atan(w1/h1)) / (1 + (w1/h1)^2)
        const float dvr = CIOU ? -(0.40528473456935109f * (2.0f * dat)) / (1.0f + r1 * r1) : 0.f;
        const float dr1[4] = {-1.0f / h1, w1 / (h1 * h1), 1.0f / h1, -(w1 / (h1 * h1))};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float duni = it.da1[q] - it.dov[q];
            const float diou = it.dov[q] / uni - it.ov / (uni * uni) * duni;
            const float dc2 = 2.0f * cw * dcw[q] + 2.0f * ch * dch[q];
            float pen = drho[q] / c2 - rho2 / (c2 * c2) * dc2;
            if (CIOU) pen += alpha * (dvr * dr1[q]);
            g[q] = -(pass * (diou - pen));
        }
    }
    // clamp(-1, 1) as torch evaluates it: a NaN stays a NaN (fminf / fmaxf would return the bound)
    return CIOU ? 1.0f - (cious < -1.0f ? -1.0f : (cious > 1.0f ? 1.0f : cious)) : 1.0f - cious;
}

// kind: enum erd_box_loss (include/erd_hip.h), ERD_BOX_IOU_LOG .. ERD_BOX_CIOU
template <int KIND>
__device__ __forceinline__ float loss_grad(const float4 p, const float4 t, float eps, float* g, float* iou_out) {
    static_assert(KIND >= ERD_BOX_IOU_LOG && KIND <= ERD_BOX_CIOU, "box-loss kind");
    if (KIND == ERD_BOX_IOU_LOG) return iou_loss_grad<0>(p, t, eps, g, iou_out);
    if (KIND == ERD_BOX_IOU_LINEAR) return iou_loss_grad<1>(p, t, eps, g, iou_out);
    if (KIND == ERD_BOX_IOU_SQUARE) return iou_loss_grad<2>(p, t, eps, g, iou_out);
    if (KIND == ERD_BOX_DIOU) return diou_loss_grad<false>(p, t, eps, g, iou_out);
    return diou_loss_grad<true>(p, t, eps, g, iou_out);
}

}  // namespace box
}  // namespace erd
#endif  // ERD_BOX_LOSS_H_
