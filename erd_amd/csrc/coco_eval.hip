// COCO bounding-box evaluation on the device (erd_amd/evaluation.py: CocoBBoxEvalGPU), gfx950 only.
//
// The same precision [T][R][K][A][M] / recall [T][K][A][M] arrays as the host restatement CocoBBoxEval.evaluate(), bit for
// bit.  What it relies on:
//   - greedy matching of the i-th detection of an (image, category) pair depends only on the detections before it, so the
//     matchings for maxDet 1 and 10 are prefixes of the one for maxDet 100: ONE matching per (pair, area range, IoU
//     threshold) over the first 100 detections, and the per-maxDet lists are those with rank < maxDet;
//   - numpy's stable mergesort of a concatenation orders ties by position: every sort here is a sort of unique keys
//     (key, original position), done as a merge sort whose passes place each element by binary search in its sibling run;
//   - cumulative tp / fp counts are small integers: the fp64 cumsum of the host is exact, so integer scans give its bits.
// All IoU / area arithmetic is fp64 in the host's operation order; the file is compiled with -ffp-contract=off.
//
// Pipeline of erd_coco_eval (one stream, no host synchronisation):
//   1. keys by (pair = image * K + label, score descending, slot) -> merge sort          => pair-contiguous, score order
//   2. pair bounds; one wave per pair: lane = area range * 10 + threshold, greedy matching => flag per (slot, lane), rank
//   3. keys by (label, score descending, step-1 position) for rank < 100 -> merge sort    => category-contiguous, score order
//   4. one workgroup per (category, area range, maxDet, threshold): two scans of the category's segment (totals, then a
//      reverse pass with the running suffix maximum of precision) sample the envelope at the 101 recall thresholds.
#include "erd_common.h"

#include <utility>

namespace {

constexpr int NA = 4, NT = 10, NM = 3, NR = 101, NL = NA * NT;   // area ranges, IoU thresholds, maxDets, recall points
constexpr int MAX_DET = 100;                                    // max(MAX_DETS)
constexpr uint64_t SENT = ~0ull;                                // sorts after every real key
constexpr int FLAG_FP = 0, FLAG_TP = 1, FLAG_IGN = 2;
constexpr int SCAN_T = 256;

// larger score -> smaller key; 0.0 == -0.0; NaN after every number (numpy's argsort of -s puts NaN last)
__device__ __forceinline__ uint64_t score_key(double s) {
    if (s != s) return SENT;
    if (s == 0.0) s = 0.0;
    uint64_t b = __builtin_bit_cast(uint64_t, s);
    b = (b >> 63) ? ~b : (b | (1ull << 63));                    // ascending order of s
    return ~b;                                                  // descending; a number never maps to SENT
}

__device__ __forceinline__ bool key_less(uint64_t a0, uint64_t b0, uint32_t i0, uint64_t a1, uint64_t b1, uint32_t i1) {
    return a0 < a1 || (a0 == a1 && (b0 < b1 || (b0 == b1 && i0 < i1)));
}

__global__ void dets_append_kernel(const float* __restrict__ dets, const int64_t* __restrict__ labels,
                                   const int32_t* __restrict__ num, const int32_t* __restrict__ img_index, int N, int P,
                                   double* __restrict__ box, double* __restrict__ score, int32_t* __restrict__ img,
                                   int32_t* __restrict__ lab) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * P) return;
    const int n = (int)(i / P), j = (int)(i % P);
    const bool ok = j < num[n];
    const float* d = dets + i * 5;
    const double x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];     // fp32 -> fp64, then w / h in fp64 (add_predictions)
    box[i * 4 + 0] = x1;
    box[i * 4 + 1] = y1;
    box[i * 4 + 2] = x2 - x1;
    box[i * 4 + 3] = y2 - y1;
    score[i] = (double)d[4];
    img[i] = ok ? img_index[n] : -1;
    lab[i] = ok ? (int32_t)labels[i] : -1;
}

__global__ void pair_keys_kernel(const double* __restrict__ score, const int32_t* __restrict__ img,
                                 const int32_t* __restrict__ lab, int64_t D, int I, int K, uint64_t* __restrict__ ka,
                                 uint64_t* __restrict__ kb, uint32_t* __restrict__ ix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    const int g = img[i], k = lab[i];
    const bool ok = g >= 0 && g < I && k >= 0 && k < K;          // an image outside gt["images"] is never counted
    ka[i] = ok ? (uint64_t)g * K + k : SENT;
    kb[i] = score_key(score[i]);
    ix[i] = (uint32_t)i;
}

// one merge pass: runs of `width` sorted elements pairwise into runs of 2 * width; each element's place is its index in its
// own run plus the number of elements of the sibling run before it (keys are unique: (a, b, index))
__global__ void merge_pass_kernel(const uint64_t* __restrict__ a_in, const uint64_t* __restrict__ b_in,
                                  const uint32_t* __restrict__ i_in, int64_t n, int64_t width, uint64_t* __restrict__ a_out,
                                  uint64_t* __restrict__ b_out, uint32_t* __restrict__ i_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t base = (i / (2 * width)) * (2 * width);
    const bool left = i - base < width;
    const int64_t own0 = left ? base : base + width;
    const int64_t oth0 = left ? base + width : base;
    const int64_t oth1 = left ? min(base + 2 * width, n) : base + width;
    const uint64_t a = a_in[i], b = b_in[i];
    const uint32_t x = i_in[i];
    int64_t lo = oth0, hi = max(oth0, oth1);
    while (lo < hi) {                                            // first element of the sibling run that is not before ours
        const int64_t mid = (lo + hi) >> 1;
        if (key_less(a_in[mid], b_in[mid], i_in[mid], a, b, x)) lo = mid + 1;
        else hi = mid;
    }
    const int64_t dst = base + (i - own0) + (lo - oth0);
    a_out[dst] = a;
    b_out[dst] = b;
    i_out[dst] = x;
}

// [start, end) of every group id < ngroups in a sorted key array (the arrays were zeroed: absent groups stay empty)
__global__ void bounds_kernel(const uint64_t* __restrict__ ka, int64_t n, int64_t ngroups, int32_t* __restrict__ start,
                              int32_t* __restrict__ end) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t g = ka[i];
    if (g >= (uint64_t)ngroups) return;
    if (i == 0 || ka[i - 1] != g) start[g] = (int32_t)i;
    if (i == n - 1 || ka[i + 1] != g) end[g] = (int32_t)(i + 1);
}

__device__ __forceinline__ double iou_xywh(const double* d, double da, const double* g, bool crowd) {
    const double dx2 = d[0] + d[2], dy2 = d[1] + d[3];
    const double gx2 = g[0] + g[2], gy2 = g[1] + g[3];
    double iw = (dx2 < gx2 ? dx2 : gx2) - (d[0] > g[0] ? d[0] : g[0]);
    double ih = (dy2 < gy2 ? dy2 : gy2) - (d[1] > g[1] ? d[1] : g[1]);
    iw = iw < 0.0 ? 0.0 : iw;
    ih = ih < 0.0 ? 0.0 : ih;
    const double inter = iw * ih;
    const double ga = g[2] * g[3];
    const double uni = crowd ? da : da + ga - inter;
    return inter / (uni > 1e-12 ? uni : 1e-12);
}

// one wave per (image, category) pair; lane = area range * 10 + IoU threshold.  gtm: one byte per (ground truth, lane)
__global__ __launch_bounds__(64) void match_kernel(
        const uint32_t* __restrict__ order, const int32_t* __restrict__ pstart,
        const int32_t* __restrict__ pend, const double* __restrict__ dbox, const double* __restrict__ gbox,
        const double* __restrict__ garea, const int32_t* __restrict__ gflag, const int32_t* __restrict__ goff,
        const double* __restrict__ area_rng, const double* __restrict__ iou_start, int npairs,
        uint8_t* __restrict__ gtm, uint8_t* __restrict__ flags, int32_t* __restrict__ rank) {
    const int p = blockIdx.x;
    if (p >= npairs) return;
    const int d0 = pstart[p], nd = pend[p] - d0;
    if (nd <= 0) return;
    const int lane = threadIdx.x;
    for (int r = lane; r < nd; r += 64) rank[d0 + r] = r;       // every detection of the pair, kept or not
    const int D = min(nd, MAX_DET);
    if (lane >= NL) return;
    const int a = lane / NT, t = lane % NT;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = iou_start[t];
    const int g0 = goff[p], G = goff[p + 1] - g0;
    uint8_t* used = gtm + (int64_t)g0 * NL + lane;
    for (int g = 0; g < G; ++g) used[(int64_t)g * NL] = 0;
    for (int di = 0; di < D; ++di) {
        const double* d = dbox + (int64_t)order[d0 + di] * 4;
        const double da = d[2] * d[3];
        double best = thr;
        int m = -1;
        bool m_ig = false;
        // ground truth in the host's order: the non-ignored first, then the ignored (both in annotation order); once a
        // non-ignored one has matched, the scan stops at the first ignored one -- nothing after it can change the match
        for (int pass = 0; pass < 2 && !(pass == 1 && m >= 0); ++pass) {
            for (int g = 0; g < G; ++g) {
                const int f = gflag[g0 + g];
                const double ar = garea[g0 + g];
                const bool ig = (f & 1) || !(lo <= ar && ar <= hi);
                if (ig != (pass == 1)) continue;
                const bool crowd = (f & 2) != 0;
                if (used[(int64_t)g * NL] && !crowd) continue;
                const double iou = iou_xywh(d, da, gbox + (int64_t)(g0 + g) * 4, crowd);
                if (iou < best) continue;
                best = iou;
                m = g;
                m_ig = ig;
            }
        }
        int fl;
        if (m >= 0) {
            used[(int64_t)m * NL] = 1;
            fl = m_ig ? FLAG_IGN : FLAG_TP;
        } else {
            fl = (lo <= da && da <= hi) ? FLAG_FP : FLAG_IGN;
        }
        flags[(int64_t)(d0 + di) * NL + lane] = (uint8_t)fl;
    }
}

// category keys over the pair-sorted positions: (label, score descending, position); position order within one label and
// one score is (image, rank) order, the concatenation order of the host
__global__ void cat_keys_kernel(const uint64_t* __restrict__ ka1, const uint64_t* __restrict__ kb1,
                                const int32_t* __restrict__ rank, int64_t D, int K, uint64_t* __restrict__ ka,
                                uint64_t* __restrict__ kb, uint32_t* __restrict__ ix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    const bool ok = ka1[i] != SENT && rank[i] >= 0 && rank[i] < MAX_DET;
    ka[i] = ok ? ka1[i] % (uint64_t)K : SENT;
    kb[i] = kb1[i];
    ix[i] = (uint32_t)i;
}

template <typename T, typename Op>
__device__ T block_scan(T v, T* sh, Op op, bool reverse) {       // inclusive scan over the 256 threads (forward or reverse)
    const int tid = threadIdx.x;
    const int me = reverse ? SCAN_T - 1 - tid : tid;
    sh[me] = v;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {
        T w = v;
        if (me >= o) w = op(sh[me - o], v);
        __syncthreads();
        sh[me] = w;
        v = w;
        __syncthreads();
    }
    return v;
}

struct Cnt {
    int tp, fp, n;
};

// one workgroup per (category k, area range a, maxDet m, threshold t)
__global__ __launch_bounds__(SCAN_T) void accumulate_kernel(
        const uint32_t* __restrict__ ord2, const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend,
        const int32_t* __restrict__ rank, const uint8_t* __restrict__ flags, const int32_t* __restrict__ n_gt,
        const int32_t* __restrict__ max_dets, const double* __restrict__ rec_thrs, int K, double* __restrict__ precision,
        double* __restrict__ recall) {
    __shared__ Cnt sc[SCAN_T];
    __shared__ double sd[SCAN_T];
    __shared__ double q[NR];
    __shared__ double rt[NR];
    __shared__ Cnt tot;
    const int bid = blockIdx.x;
    const int t = bid % NT, m = (bid / NT) % NM, a = (bid / (NT * NM)) % NA, k = bid / (NT * NM * NA);
    const int tid = threadIdx.x;
    const int ngt = n_gt[k * NA + a];
    const int64_t rstride = (int64_t)K * NA * NM;
    double* prec = precision + (int64_t)t * NR * rstride + ((int64_t)k * NA + a) * NM + m;   // + r * rstride
    double* rec = recall + (((int64_t)t * K + k) * NA + a) * NM + m;
    if (ngt == 0) {                                              // no ground truth in the range: -1 (the host skips it)
        for (int r = tid; r < NR; r += SCAN_T) prec[r * rstride] = -1.0;
        if (tid == 0) *rec = -1.0;
        return;
    }
    for (int r = tid; r < NR; r += SCAN_T) {
        q[r] = 0.0;
        rt[r] = rec_thrs[r];
    }
    const int s0 = cstart[k], s1 = cend[k];
    const int md = max_dets[m];
    const int lane = a * NT + t;
    auto load = [&](int e, int& tpf, int& fpf, int& inc) {
        tpf = fpf = inc = 0;
        if (e < s1) {
            const uint32_t pos = ord2[e];
            if (rank[pos] < md) {
                inc = 1;
                const int f = flags[(int64_t)pos * NL + lane];
                tpf = f == FLAG_TP;
                fpf = f == FLAG_FP;
            }
        }
    };
    auto add = [](Cnt x, Cnt y) { return Cnt{x.tp + y.tp, x.fp + y.fp, x.n + y.n}; };
    // pass 1: totals
    Cnt mine{0, 0, 0};
    for (int e = s0 + tid; e < s1; e += SCAN_T) {
        int tpf, fpf, inc;
        load(e, tpf, fpf, inc);
        mine = add(mine, Cnt{tpf, fpf, inc});
    }
    mine = block_scan(mine, sc, add, false);
    if (tid == SCAN_T - 1) tot = mine;
    __syncthreads();
    const Cnt total = tot;
    if (tid == 0) *rec = (double)total.tp / (double)ngt;       // rc[-1], or 0 without detections
    // pass 2: chunks from the right; cum = counts up to and including the element, env = max precision from it to the end
    Cnt after{0, 0, 0};                                          // counts right of the current chunk
    double env_right = -1.0;
    const int nchunk = (s1 - s0 + SCAN_T - 1) / SCAN_T;
    for (int c = nchunk - 1; c >= 0; --c) {
        const int e = s0 + c * SCAN_T + tid;
        int tpf, fpf, inc;
        load(e, tpf, fpf, inc);
        const Cnt pre = block_scan(Cnt{tpf, fpf, inc}, sc, add, false);
        const Cnt chunk = sc[SCAN_T - 1];
        const Cnt before{total.tp - after.tp - chunk.tp, total.fp - after.fp - chunk.fp, total.n - after.n - chunk.n};
        const Cnt cum = add(before, pre);
        double pr = -1.0;
        if (inc) {
            const double tp = cum.tp, den = (double)(cum.tp + cum.fp);
            pr = tp / (den > 2.220446049250313e-16 ? den : 2.220446049250313e-16);
        }
        __syncthreads();
        double env = block_scan(pr, sd, [](double x, double y) { return x > y ? x : y; }, true);
        env = env > env_right ? env : env_right;
        if (inc && (tpf || cum.n == 1)) {                        // recall moves here (or the array starts here)
            const double rc = (double)cum.tp / (double)ngt;
            int r = 0;
            if (cum.n > 1) {
                const double rc_prev = (double)(cum.tp - tpf) / (double)ngt;
                while (r < NR && !(rt[r] > rc_prev)) ++r;
            }
            for (; r < NR && rt[r] <= rc; ++r) q[r] = env;       // searchsorted(rc, r, 'left') lands on this element
        }
        __syncthreads();
        const double first = sd[SCAN_T - 1];                     // the reverse scan's total (the chunk's maximum)
        env_right = first > env_right ? first : env_right;
        after = add(after, chunk);
        __syncthreads();
    }
    for (int r = tid; r < NR; r += SCAN_T) prec[r * rstride] = q[r];
}

struct Ws {
    uint64_t *ka[2], *kb[2];
    uint32_t* ix[2];
    int32_t *pstart, *pend, *cstart, *cend, *rank;
    uint8_t *flags, *gtm;
};

size_t carve(Ws* w, char* base, int64_t D, int64_t npairs, int K, int64_t ngt) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    for (int s = 0; s < 2; ++s) {
        w->ka[s] = (uint64_t*)take(D * 8);
        w->kb[s] = (uint64_t*)take(D * 8);
        w->ix[s] = (uint32_t*)take(D * 4);
    }
    w->pstart = (int32_t*)take(npairs * 4);
    w->pend = (int32_t*)take(npairs * 4);
    w->cstart = (int32_t*)take((size_t)K * 4);
    w->cend = (int32_t*)take((size_t)K * 4);
    w->rank = (int32_t*)take(D * 4);
    w->flags = (uint8_t*)take(D * NL);
    w->gtm = (uint8_t*)take((ngt > 0 ? ngt : 1) * NL);
    return off;
}

// sorts (ka, kb, ix)[0] in place (the result lands in buffer 0); returns a launch error or 0
int merge_sort(Ws& w, int64_t D, hipStream_t st) {
    int cur = 0;
    const dim3 grid((unsigned)((D + 255) / 256));
    for (int64_t width = 1; width < D; width *= 2) {
        hipLaunchKernelGGL(merge_pass_kernel, grid, dim3(256), 0, st, w.ka[cur], w.kb[cur], w.ix[cur], D, width,
                           w.ka[cur ^ 1], w.kb[cur ^ 1], w.ix[cur ^ 1]);
        cur ^= 1;
    }
    if (cur) {
        const hipError_t e = hipMemcpyAsync(w.ka[0], w.ka[1], D * 8, hipMemcpyDeviceToDevice, st);
        const hipError_t e2 = hipMemcpyAsync(w.kb[0], w.kb[1], D * 8, hipMemcpyDeviceToDevice, st);
        const hipError_t e3 = hipMemcpyAsync(w.ix[0], w.ix[1], D * 4, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
            erd::set_error("coco_eval: hipMemcpyAsync failed");
            return (int)(e != hipSuccess ? e : e2 != hipSuccess ? e2 : e3);
        }
    }
    return erd::check_launch("coco_eval merge sort");
}

}  // namespace

extern "C" int erd_coco_dets_append(const float* dets, const int64_t* labels, const int32_t* num, const int32_t* img_index,
                                    int N, int P, double* box, double* score, int32_t* img, int32_t* label,
                                    erd_stream_t stream) {
    ERD_REQUIRE(dets && labels && num && img_index && box && score && img && label, "coco_dets_append: null");
    ERD_REQUIRE(N > 0 && P > 0 && (int64_t)N * P < (1ll << 31), "coco_dets_append: bad sizes");
    const int64_t n = (int64_t)N * P;
    hipLaunchKernelGGL(dets_append_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dets, labels,
                       num, img_index, N, P, box, score, img, label);
    return erd::check_launch("coco_dets_append");
}

extern "C" size_t erd_coco_eval_ws_bytes(int64_t D, int npairs, int K, int64_t ngt) {
    Ws w;
    return carve(&w, nullptr, D, npairs, K, ngt);
}

extern "C" int erd_coco_eval(const double* dt_box, const double* dt_score, const int32_t* dt_img, const int32_t* dt_label,
                             int64_t D, const double* gt_box, const double* gt_area, const int32_t* gt_flag,
                             const int32_t* gt_off, int I, int K, int64_t ngt, const int32_t* n_gt, const double* area_rng,
                             const double* iou_start, const double* rec_thrs, const int32_t* max_dets, double* precision,
                             double* recall, void* ws, size_t ws_bytes, erd_stream_t stream) {
    ERD_REQUIRE(gt_off && n_gt && area_rng && iou_start && rec_thrs && max_dets && precision && recall && ws,
                "coco_eval: null");
    ERD_REQUIRE(I > 0 && K > 0 && (int64_t)I * K < (1ll << 31) && D >= 0 && D < (1ll << 31) && ngt >= 0,
                "coco_eval: bad sizes");
    ERD_REQUIRE(D == 0 || (dt_box && dt_score && dt_img && dt_label), "coco_eval: null detections");
    ERD_REQUIRE(ngt == 0 || (gt_box && gt_area && gt_flag), "coco_eval: null ground truth");
    const int npairs = I * K;
    ERD_REQUIRE(ws_bytes >= erd_coco_eval_ws_bytes(D, npairs, K, ngt), "coco_eval: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    Ws w;
    carve(&w, (char*)ws, D, npairs, K, ngt);
    ERD_ZERO_ASYNC(w.cstart, (size_t)K * 4, st);
    ERD_ZERO_ASYNC(w.cend, (size_t)K * 4, st);
    if (D > 0) {
        const dim3 grid((unsigned)((D + 255) / 256));
        ERD_ZERO_ASYNC(w.pstart, (size_t)npairs * 4, st);
        ERD_ZERO_ASYNC(w.pend, (size_t)npairs * 4, st);
        const hipError_t e = hipMemsetAsync(w.rank, 0xFF, D * 4, st);      // -1: no pair
        if (e != hipSuccess) {
            erd::set_error("hipMemsetAsync: %s", hipGetErrorString(e));
            return (int)e;
        }
        hipLaunchKernelGGL(pair_keys_kernel, grid, dim3(256), 0, st, dt_score, dt_img, dt_label, D, I, K, w.ka[0], w.kb[0],
                           w.ix[0]);
        int rc = merge_sort(w, D, st);
        if (rc) return rc;
        hipLaunchKernelGGL(bounds_kernel, grid, dim3(256), 0, st, w.ka[0], D, (int64_t)npairs, w.pstart, w.pend);
        hipLaunchKernelGGL(match_kernel, dim3((unsigned)npairs), dim3(64), 0, st, w.ix[0], w.pstart, w.pend, dt_box,
                           gt_box, gt_area, gt_flag, gt_off, area_rng, iou_start, npairs, w.gtm, w.flags, w.rank);
        // the category keys go to buffer 1 and are sorted from there: buffer 0 keeps the pair order the flags index
        hipLaunchKernelGGL(cat_keys_kernel, grid, dim3(256), 0, st, w.ka[0], w.kb[0], w.rank, D, K, w.ka[1], w.kb[1], w.ix[1]);
        rc = erd::check_launch("coco_eval match");
        if (rc) return rc;
        std::swap(w.ka[0], w.ka[1]);
        std::swap(w.kb[0], w.kb[1]);
        std::swap(w.ix[0], w.ix[1]);
        rc = merge_sort(w, D, st);
        if (rc) return rc;
        hipLaunchKernelGGL(bounds_kernel, grid, dim3(256), 0, st, w.ka[0], D, (int64_t)K, w.cstart, w.cend);
    }
    // rank / flags are indexed by pair-sorted position, which is what the category sort carries in ix
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)(K * NA * NM * NT)), dim3(SCAN_T), 0, st, w.ix[0], w.cstart, w.cend,
                       w.rank, w.flags, n_gt, max_dets, rec_thrs, K, precision, recall);
    return erd::check_launch("coco_eval");
}
