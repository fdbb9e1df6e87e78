// Grouped 3x3 convolutions of the ResNeXt bottleneck (conv2: `cardinality` independent convolutions of cg = C / cardinality channels
// each, mmdet/models/backbones/resnext.py:55-64) on the fp32 vector pipe: forward, input gradient and weight-gradient partial slabs.
//
// Why not the matrix cores: with cg = 4 .. 32 the contraction of one output is 9 * cg products, and a dense GEMM tile would multiply the
// zeros of the block-diagonal weight `cardinality` times over.  Every conv2 of a ResNeXt-101 32x4d is the same 0.62 GFLOP per image;
// measured (profiles/r10_conv_grouped.txt) the launches reach neither the HBM nor the vector roofline.
//
// Arithmetic (all three kernels): every output is ONE fp32 fma chain whose order is fixed by the shape alone --
//   forward         the group's input-channel quads ascending, per quad the taps (kh, kw) ascending, per tap the quad's four channels;
//   input gradient  the same over the group's output channels, with the taps whose parity reaches the pixel;
//   weight gradient every PL-th pixel of its split ascending per pixel lane, then the lanes in order (PL fixed by the shape).
// A tap outside the map contributes an operand of 0.  Nothing depends on the grid size: forward and input gradient give the same
// bits under any CU reserve.  The compute modes "f32" and "f32x3" share these kernels.
//
// Forward / input gradient: a workgroup takes a block of CB = min(C, max(cg, 512 / cg)) channels (whole groups), stages that block's weights in
// LDS ONCE (the input gradient applies the folded BN row scale and transposes while staging: it reads the parameter's own layout
// [C][3][3][cg]) and then walks pixel tiles persistently.  A thread owns four adjacent output channels of two pixels; the lanes of a wave
// run along the channels, so a wave's loads and stores of a pixel are contiguous.  LDS layout [tap][cg / 4][CB][4]: a thread's four
// weight vectors of a step are 64 contiguous bytes, neighbouring lanes read neighbouring 64 bytes.
#include "erd_common.h"

#include <algorithm>

namespace {

constexpr int NT = 256;
// channels per workgroup of the forward / input-gradient kernels: whole groups, 18 KB of staged weights (36 KB at cg = 32)
constexpr int cb_max(int cg) { return cg == 32 ? 32 : 512 / cg; }

struct Geo {
    int N, IH, IW, OH, OW, C, stride;
};

__device__ __forceinline__ void dot4(float& acc, const float4 x, const float4 w) {
    acc = fmaf(x.x, w.x, acc);
    acc = fmaf(x.y, w.y, acc);
    acc = fmaf(x.z, w.z, acc);
    acc = fmaf(x.w, w.w, acc);
}

struct ClassStart {
    int v[4];
};

// acc[i][j] += sum over the NTAP taps packed in `taps` (4 bits each, ascending) and the group's channels of in * w for the thread's two
// pixels i and four channels j.  Order of every chain: channel quads of the group ascending, then the taps ascending, then the four
// channels of the quad.  All loads of a quad step are issued before its multiplications; a tap outside the map contributes in = 0.
template <int CG, bool DGRAD, int NTAP>
__device__ __forceinline__ void accumulate(float (&acc)[2][4], const float* __restrict__ in, const float4* wl, int CB, int q, int gbase, int C,
                                           int s, int QH, int QW, const int (&n)[2], const int (&y)[2], const int (&x)[2],
                                           const bool (&on)[2], unsigned long long taps) {
    constexpr int Q = CG / 4;
    unsigned off[2][NTAP];      // element offsets (< 2^31: the entry point checks)
    bool ok[2][NTAP];
#pragma unroll
    for (int k = 0; k < NTAP; ++k) {
        const int t = (int)((taps >> (4 * k)) & 15), kh = t / 3, kw = t % 3;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int iy, ix;
            bool v;
            if (!DGRAD) {
                iy = y[i] * s + kh - 1;
                ix = x[i] * s + kw - 1;
                v = on[i] && iy >= 0 && iy < QH && ix >= 0 && ix < QW;
            } else {
                const int ny = y[i] + 1 - kh, nx = x[i] + 1 - kw;      // (stride 2: the class's taps divide)
                iy = ny / s;
                ix = nx / s;
                v = on[i] && ny >= 0 && nx >= 0 && iy < QH && ix < QW;
            }
            ok[i][k] = v;
            off[i][k] = v ? (((unsigned)n[i] * QH + iy) * QW + ix) * (unsigned)C + gbase : 0u;
        }
    }
    int nq = Q;
    asm volatile("" : "+s"(nq));      // (an opaque trip count: also the one-quad case keeps the shape of the loop, 232 registers)
#pragma unroll 1
    for (int c4 = 0; c4 < nq; ++c4) {      // (not unrolled: the loads of ALL quads hoisted to the top would not fit the register file)
        float4 xv[2][NTAP];
#pragma unroll
        for (int k = 0; k < NTAP; ++k)
#pragma unroll
            for (int i = 0; i < 2; ++i) xv[i][k] = ok[i][k] ? erd::ld4(in + off[i][k] + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < NTAP; ++k) {
            const int t = (int)((taps >> (4 * k)) & 15);
            const float4* wp = wl + (t * Q + c4) * CB + 4 * q;
            const float4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                dot4(acc[i][0], xv[i][k], w0);
                dot4(acc[i][1], xv[i][k], w1);
                dot4(acc[i][2], xv[i][k], w2);
                dot4(acc[i][3], xv[i][k], w3);
            }
        }
    }
}

// DGRAD = false: out = epi(conv_g(in = x, w)); iterates the OH x OW map, tap (kh, kw) reads x[oy * s + kh - 1][ox * s + kw - 1]
// DGRAD = true:  out = dx = epi(conv_g^T(in = dz, w * rowscale)); iterates the IH x IW map, tap (kh, kw) reads
//                dz[(y + 1 - kh) / s][(x + 1 - kw) / s] where both divide
template <int CG, bool DGRAD>
__global__ __launch_bounds__(NT, 2) void conv_grouped_kernel(erd_conv_grouped_desc d, int CB, int ncb, int Gc, int ntiles, ClassStart cls_start) {
    __shared__ float4 wl[9 * CG * cb_max(CG) / 4];
    __shared__ float red[1024];
    constexpr int Q = CG / 4;
    const int tid = threadIdx.x;
    const int L = erd::xcd_contiguous(blockIdx.x, gridDim.x);
    const int cb = L / Gc, j0 = L % Gc;
    const int C = d.C, s = d.stride;
    const int c_base = cb * CB;

    // ---- stage the channel block's weights
    if (!DGRAD) {
        // global order (cob, t, c4): coalesced reads
        for (int e = tid; e < CB * 9 * Q; e += NT) {
            const int c4 = e % Q, t = (e / Q) % 9, cob = e / (9 * Q);
            const int co = c_base + cob;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < C) v = erd::ld4(d.w + ((int64_t)co * 9 + t) * CG + c4 * 4);
            wl[(t * Q + c4) * CB + cob] = v;
        }
    } else {
        for (int e = tid; e < CB * 9 * Q; e += NT) {
            const int cib = e % CB, c4 = (e / CB) % Q, t = e / (CB * Q);
            const int ci = c_base + cib;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (ci < C) {
                const int g = ci / CG, cil = ci % CG;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int co = g * CG + c4 * 4 + a;
                    const float wv = d.w[((int64_t)co * 9 + t) * CG + cil];
                    v[a] = d.scale ? d.scale[co] * wv : wv;
                }
            }
            wl[(t * Q + c4) * CB + cib] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    __syncthreads();

    const int QB = CB / 4, PP = NT / QB;
    const int q = tid % QB, pl = tid / QB;
    const int c0 = c_base + 4 * q;                 // this thread's four channels
    const bool lane_on = pl < PP && c0 < C;
    const int gbase = (c0 / CG) * CG;              // first channel of their group
    const int PH = DGRAD ? d.IH : d.OH, PW = DGRAD ? d.IW : d.OW;      // the map this launch writes
    const int QH = DGRAD ? d.OH : d.IH, QW = DGRAD ? d.OW : d.IW;      // the map it reads
    const int step = (DGRAD && s == 2) ? 2 : 1;    // stride-2 input gradient: four parity classes of pixels, each with its own taps
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);

#pragma unroll 1
    for (int tile = j0; tile < ntiles; tile += Gc) {
        asm volatile("" ::: "memory");      // (the staged weights are re-read per tile: kept across tiles they cost the second resident workgroup)
        // the tile's parity class (uniform): tiles never straddle classes
        int cls = 0;
        if (step == 2) cls = tile >= cls_start.v[3] ? 3 : (tile >= cls_start.v[2] ? 2 : (tile >= cls_start.v[1] ? 1 : 0));
        const int py = step == 2 ? (cls == 0 || cls == 2) : 0, px = step == 2 ? (cls == 0 || cls == 1) : 0;      // (1,1) (0,1) (1,0) (0,0)
        const int Hc = (PH - py + step - 1) / step, Wc = (PW - px + step - 1) / step;
        const unsigned npix_c = (unsigned)d.N * Hc * Wc;
        const unsigned lt = (unsigned)(tile - (step == 2 ? cls_start.v[cls] : 0));
        unsigned p[2];
        int n[2], y[2], x[2];
        bool on[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned pc = lt * 2 * PP + i * PP + pl;
            on[i] = lane_on && pc < npix_c;
            const unsigned pp = on[i] ? pc : 0, r = pp / (unsigned)Wc;
            x[i] = (int)(pp % (unsigned)Wc) * step + px;
            y[i] = (int)(r % (unsigned)Hc) * step + py;
            n[i] = (int)(r / (unsigned)Hc);
            p[i] = ((unsigned)n[i] * PH + y[i]) * PW + x[i];
        }
        float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (step == 1) accumulate<CG, DGRAD, 9>(acc, d.in, wl, CB, q, gbase, C, s, QH, QW, n, y, x, on, 0x876543210ull);
        else if (cls == 0) accumulate<CG, DGRAD, 4>(acc, d.in, wl, CB, q, gbase, C, s, QH, QW, n, y, x, on, 0x8620ull);
        else if (cls == 1) accumulate<CG, DGRAD, 2>(acc, d.in, wl, CB, q, gbase, C, s, QH, QW, n, y, x, on, 0x53ull);
        else if (cls == 2) accumulate<CG, DGRAD, 2>(acc, d.in, wl, CB, q, gbase, C, s, QH, QW, n, y, x, on, 0x71ull);
        else accumulate<CG, DGRAD, 1>(acc, d.in, wl, CB, q, gbase, C, s, QH, QW, n, y, x, on, 0x4ull);
        // ---- epilogue
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (!on[i]) continue;
            const int64_t o = (int64_t)p[i] * C + c0;
            float v[4] = {acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
            if (!DGRAD) {
                if (d.scale) {
                    const float4 sc = erd::ld4(d.scale + c0);
                    v[0] *= sc.x, v[1] *= sc.y, v[2] *= sc.z, v[3] *= sc.w;
                }
                if (d.shift) {
                    const float4 sh = erd::ld4(d.shift + c0);
                    v[0] += sh.x, v[1] += sh.y, v[2] += sh.z, v[3] += sh.w;
                }
            }
            if (d.res) {
                const float4 r = erd::ld4(d.res + o);
                v[0] += r.x, v[1] += r.y, v[2] += r.z, v[3] += r.w;
            }
            if (!DGRAD && d.relu) {
#pragma unroll
                for (int b = 0; b < 4; ++b) v[b] = fmaxf(v[b], 0.f);
            }
            if (d.mask) {
                const float4 m = erd::ld4(d.mask + o);
                v[0] = m.x > 0.f ? v[0] : 0.f;
                v[1] = m.y > 0.f ? v[1] : 0.f;
                v[2] = m.z > 0.f ? v[2] : 0.f;
                v[3] = m.w > 0.f ? v[3] : 0.f;
            }
            erd::st4(d.out + o, make_float4(v[0], v[1], v[2], v[3]));
            cs.x += v[0], cs.y += v[1], cs.z += v[2], cs.w += v[3];
        }
    }

    // ---- column sums of what this workgroup stored: folded over its pixel lanes in LDS, one atomic per channel into the workgroup's
    // replicated row (the consumer folds the rows, erd_bn_dgamma)
    if (d.colsum) {
        if (pl < PP) *reinterpret_cast<float4*>(red + (pl * QB + q) * 4) = cs;
        __syncthreads();
        if (tid < CB && c_base + tid < C) {
            float sum = 0.f;
            for (int r = 0; r < PP; ++r) sum += red[r * CB + tid];
            const int row = d.colsum_copies > 1 ? (int)(blockIdx.x & (unsigned)(d.colsum_copies - 1)) : 0;
            atomicAdd(d.colsum + (int64_t)row * C + c_base + tid, sum);
        }
    }
}

// Weight-gradient partial slabs part[s][co][t][cil] = sum over the pixels of split s of dz[p][co] * x[p shifted by tap t][group(co) * cg + cil].
// A workgroup = (split, block of CBW channels = whole groups).  A thread owns a PAIR (four output channels, four input channels of
// their group) at all nine taps -- 144 accumulators fed by ten 16-byte loads per pixel -- and every PL-th pixel of the split (PL = 256 /
// pairs of the block pixel lanes; two workgroups per CU hide each other's load latency).  A tap outside the map
// contributes x = 0.  The pixel lanes are folded through LDS in lane order and the block stores its slab: no atomics, the sums depend on
// the shape and the split count alone.  Lanes run (group, output quad, input quad): a wave's x loads cover whole groups.
struct WgOperands {
    float4 dz;
    float4 x[9];
};

template <int CG>
__device__ __forceinline__ void wg_load(WgOperands& o, const float* __restrict__ x, const float* __restrict__ dz, const Geo& g, unsigned p,
                                        int co, int xc) {
    const unsigned ox = p % (unsigned)g.OW, r = p / (unsigned)g.OW;
    const unsigned oy = r % (unsigned)g.OH, n = r / (unsigned)g.OH;
    o.dz = erd::ld4(dz + (int64_t)p * g.C + co);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = (int)oy * g.stride + t / 3 - 1, ix = (int)ox * g.stride + t % 3 - 1;
        const bool ok = iy >= 0 && iy < g.IH && ix >= 0 && ix < g.IW;
        o.x[t] = ok ? erd::ld4(x + (((int64_t)n * g.IH + iy) * g.IW + ix) * g.C + xc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <int CG>
__global__ __launch_bounds__(NT) void conv_grouped_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                               float* __restrict__ part, Geo g, int PAIRS, int ncb, unsigned chunk) {
    __shared__ float red[NT * 16];
    constexpr int Q = CG / 4;                      // quads per group; a group has Q * Q pairs
    const int tid = threadIdx.x;
    const int cb = blockIdx.x % ncb, sp = blockIdx.x / ncb;
    const int PL = NT / PAIRS;
    const int pair = tid % PAIRS, pl = tid / PAIRS;
    const int gpair = cb * PAIRS + pair;           // pair index over the whole layer: (group, output quad, input quad)
    const int grp = gpair / (Q * Q), qo = (gpair / Q) % Q, qi = gpair % Q;
    const int co = grp * CG + qo * 4, xc = grp * CG + qi * 4;
    const bool on = pl < PL && co < g.C;
    const unsigned npix = (unsigned)g.N * g.OH * g.OW;
    const unsigned p_begin = sp * chunk, p_end = p_begin + chunk < npix ? p_begin + chunk : npix;
    float acc[9][16];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
    if (on) {
        for (unsigned p = p_begin + pl; p < p_end; p += PL) {
            WgOperands cur;
            wg_load<CG>(cur, x, dz, g, p, co, xc);
            const float dv[4] = {cur.dz.x, cur.dz.y, cur.dz.z, cur.dz.w};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    acc[t][a * 4 + 0] = fmaf(dv[a], cur.x[t].x, acc[t][a * 4 + 0]);
                    acc[t][a * 4 + 1] = fmaf(dv[a], cur.x[t].y, acc[t][a * 4 + 1]);
                    acc[t][a * 4 + 2] = fmaf(dv[a], cur.x[t].z, acc[t][a * 4 + 2]);
                    acc[t][a * 4 + 3] = fmaf(dv[a], cur.x[t].w, acc[t][a * 4 + 3]);
                }
            }
        }
    }
    // fold the pixel lanes, tap by tap: red[pl][pair][16] -> part[sp][co + a][t][qi * 4 + b]
    const int nout = PAIRS * 16;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        if (pl < PL) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<float4*>(red + (pl * PAIRS + pair) * 16 + j * 4) =
                    make_float4(acc[t][j * 4], acc[t][j * 4 + 1], acc[t][j * 4 + 2], acc[t][j * 4 + 3]);
        }
        __syncthreads();
        for (int o = tid; o < nout; o += NT) {
            float sum = 0.f;
            for (int r = 0; r < PL; ++r) sum += red[r * nout + o];
            const int pr = cb * PAIRS + o / 16, a = (o / 4) % 4, b = o % 4;
            const int pg = pr / (Q * Q), pqo = (pr / Q) % Q, pqi = pr % Q;
            const int oc = pg * CG + pqo * 4 + a;
            if (oc < g.C) part[(((int64_t)sp * g.C + oc) * 9 + t) * CG + pqi * 4 + b] = sum;
        }
        __syncthreads();
    }
}

// pairs per workgroup and channel blocks of a weight-gradient launch
void wgrad_blocks(int C, int cg, int& pairs, int& ncb) {
    const int total = (C / 4) * (cg / 4);
    pairs = std::min(64, total);
    ncb = (total + pairs - 1) / pairs;
}

int num_cus_grouped() {
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

// shape rules shared by the three entries; 0 when the launch is in scope
int check_shape(const char* what, int N, int IH, int IW, int C, int cg, int stride) {
    if (N <= 0 || IH <= 0 || IW <= 0 || C <= 0) {
        erd::set_error("%s: empty map (N %d, %d x %d, C %d)", what, N, IH, IW, C);
        return ERD_EINVAL;
    }
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32) {
        erd::set_error("%s: %d channels per group; supported: 4, 8, 16, 32", what, cg);
        return ERD_EUNSUPPORTED;
    }
    if (C % cg != 0 || C / cg < 2) {
        erd::set_error("%s: C = %d is not cardinality >= 2 times cg = %d", what, C, cg);
        return ERD_EUNSUPPORTED;
    }
    if (stride != 1 && stride != 2) {
        erd::set_error("%s: stride %d; supported: 1, 2", what, stride);
        return ERD_EUNSUPPORTED;
    }
    return 0;
}

template <bool DGRAD>
int launch_conv(const erd_conv_grouped_desc* d, hipStream_t st) {
    const char* what = DGRAD ? "erd_conv_grouped_dgrad" : "erd_conv_grouped_fwd";
    ERD_REQUIRE(d != nullptr, "%s: null descriptor", what);
    const int rc = check_shape(what, d->N, d->IH, d->IW, d->C, d->cg, d->stride);
    if (rc) return rc;
    ERD_REQUIRE(d->OH == (d->IH - 1) / d->stride + 1 && d->OW == (d->IW - 1) / d->stride + 1,
                "%s: output %d x %d does not belong to input %d x %d at stride %d (3x3, pad 1)", what, d->OH, d->OW, d->IH, d->IW, d->stride);
    ERD_REQUIRE(d->in && d->out && d->w, "%s: null in / out / w", what);
    ERD_REQUIRE(aligned16(d->in) && aligned16(d->out) && aligned16(d->w) && aligned16(d->scale) && aligned16(d->shift) && aligned16(d->res) &&
                    aligned16(d->mask),
                "%s: pointers must be 16-byte aligned", what);
    ERD_REQUIRE(d->colsum_copies >= 0 && (d->colsum_copies & (d->colsum_copies - 1)) == 0, "%s: colsum_copies %d is not a power of two", what,
                d->colsum_copies);
    if (DGRAD) ERD_REQUIRE(!d->shift && !d->relu, "%s: no shift / relu in an input gradient", what);
    else ERD_REQUIRE(!d->mask && !d->colsum, "%s: no mask / colsum in a forward launch", what);
    const int CB = std::min(d->C, cb_max(d->cg)), ncb = (d->C + CB - 1) / CB;
    const int PP = NT / (CB / 4);
    ERD_REQUIRE((int64_t)d->N * d->IH * d->IW * d->C < (1ll << 31), "%s: map too large", what);
    // pixel tiles of 2 * PP pixels; a stride-2 input gradient lists them by output-parity class (1,1) (0,1) (1,0) (0,0): 4 + 2 + 2 + 1 taps
    ClassStart cls_start = {{0, 0, 0, 0}};
    int64_t nt = 0;
    if (DGRAD && d->stride == 2) {
        const int pys[4] = {1, 0, 1, 0}, pxs[4] = {1, 1, 0, 0};
        for (int c = 0; c < 4; ++c) {
            cls_start.v[c] = (int)nt;
            const int64_t npc = (int64_t)d->N * ((d->IH - pys[c] + 1) / 2) * ((d->IW - pxs[c] + 1) / 2);
            nt += (npc + 2 * PP - 1) / (2 * PP);
        }
    } else {
        const int64_t npix = (int64_t)d->N * (DGRAD ? (int64_t)d->IH * d->IW : (int64_t)d->OH * d->OW);
        nt = (npix + 2 * PP - 1) / (2 * PP);
    }
    // two workgroups per CU (a quad step keeps its 18 operand and 36 weight vectors in registers: up to 256 of them), both resident: the
    // persistent grid of one dispatch round
    const int slots = 2 * erd::usable_cus(num_cus_grouped());
    const int Gc = (int)std::max<int64_t>(1, std::min<int64_t>(nt, slots / ncb));
    const dim3 grid(ncb * Gc), block(NT);
#define ERD_GC_LAUNCH(CG_)                                                                                        \
    case CG_:                                                                                                     \
        hipLaunchKernelGGL((conv_grouped_kernel<CG_, DGRAD>), grid, block, 0, st, *d, CB, ncb, Gc, (int)nt, cls_start);     \
        break;
    switch (d->cg) {
        ERD_GC_LAUNCH(4)
        ERD_GC_LAUNCH(8)
        ERD_GC_LAUNCH(16)
        ERD_GC_LAUNCH(32)
    }
#undef ERD_GC_LAUNCH
    return erd::check_launch(what);
}

}  // namespace

// replaces: the F.conv2d dispatch of conv2 with groups = cardinality, resnext.py:55-64 (+ fused frozen-statistics BN / ReLU)
extern "C" int erd_conv_grouped_fwd(const erd_conv_grouped_desc* d, erd_stream_t stream) {
    return launch_conv<false>(d, (hipStream_t)stream);
}

// replaces: the input-gradient half of that call site's convolution_backward (+ the ReLU mask of conv1's output and the column sums for
// its d beta, which the reference computes in separate threshold_backward / sum dispatches)
extern "C" int erd_conv_grouped_dgrad(const erd_conv_grouped_desc* d, erd_stream_t stream) {
    return launch_conv<true>(d, (hipStream_t)stream);
}

// replaces: the weight-gradient half of that call site's convolution_backward
extern "C" int erd_conv_grouped_wgrad(const float* x, const float* dz, float* part, int N, int IH, int IW, int C, int cg, int stride,
                                      int nsplit, erd_stream_t stream) {
    const char* what = "erd_conv_grouped_wgrad";
    const int rc = check_shape(what, N, IH, IW, C, cg, stride);
    if (rc) return rc;
    ERD_REQUIRE(x && dz && part, "%s: null x / dz / part", what);
    ERD_REQUIRE(aligned16(x) && aligned16(dz) && aligned16(part), "%s: pointers must be 16-byte aligned", what);
    ERD_REQUIRE(nsplit >= 1 && nsplit <= 4096, "%s: nsplit %d outside 1 .. 4096", what, nsplit);
    Geo g = {N, IH, IW, (IH - 1) / stride + 1, (IW - 1) / stride + 1, C, stride};
    const int64_t npix = (int64_t)N * g.OH * g.OW;
    ERD_REQUIRE(npix < (1ll << 31) && (int64_t)N * IH * IW < (1ll << 31), "%s: map too large", what);
    int pairs, ncb;
    wgrad_blocks(C, cg, pairs, ncb);
    const unsigned chunk = (unsigned)((npix + nsplit - 1) / nsplit);      // (splits past the last pixel write zero slabs)
    const dim3 grid(nsplit * ncb), block(NT);
    hipStream_t st = (hipStream_t)stream;
    switch (cg) {
        case 4: hipLaunchKernelGGL((conv_grouped_wgrad_kernel<4>), grid, block, 0, st, x, dz, part, g, pairs, ncb, chunk); break;
        case 8: hipLaunchKernelGGL((conv_grouped_wgrad_kernel<8>), grid, block, 0, st, x, dz, part, g, pairs, ncb, chunk); break;
        case 16: hipLaunchKernelGGL((conv_grouped_wgrad_kernel<16>), grid, block, 0, st, x, dz, part, g, pairs, ncb, chunk); break;
        case 32: hipLaunchKernelGGL((conv_grouped_wgrad_kernel<32>), grid, block, 0, st, x, dz, part, g, pairs, ncb, chunk); break;
    }
    return erd::check_launch(what);
}

// the split count of erd_conv_grouped_wgrad that makes ONE dispatch round of erd_usable_cus(): two workgroups per CU (144 accumulators per
// thread) over the launch's channel blocks, at least 64 pixels per split, at most 512 splits; < 0 on a shape out of scope
extern "C" int erd_conv_grouped_wgrad_splits(int N, int IH, int IW, int C, int cg, int stride) {
    const int rc = check_shape("erd_conv_grouped_wgrad_splits", N, IH, IW, C, cg, stride);
    if (rc) return rc;
    int pairs, ncb;
    wgrad_blocks(C, cg, pairs, ncb);
    const int64_t npix = (int64_t)N * ((IH - 1) / stride + 1) * ((IW - 1) / stride + 1);
    const int64_t s = std::min<int64_t>(std::min<int64_t>(2 * erd::usable_cus(num_cus_grouped()) / ncb, npix / 64), 512);
    return (int)std::max<int64_t>(1, s);
}
