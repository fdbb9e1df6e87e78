// HBM-bound kernels around the convolutions: stem, max-pool, frozen-BN helpers, GroupNorm(32)+ReLU
// forward/backward over level-concatenated [N][A][C] maps, FPN top-down add, bias/scale helpers, SGD.
// All activations NHWC fp32; 16-byte (float4) accesses, channels fastest => fully coalesced rows.
#include "erd_common.h"
#include <vector>

namespace erd {
thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace erd

extern "C" int erd_abi_version(void) { return ERD_ABI_VERSION; }
#ifndef ERD_CSRC_SHA
#define ERD_CSRC_SHA "unknown"
#endif
extern "C" const char* erd_csrc_sha(void) { return ERD_CSRC_SHA; }
// 1 when any translation unit of this library was compiled with a probe of erd_probes.h (a timing / accuracy / trace variant)
extern "C" __attribute__((weak)) int erd_probe_build_marker;
extern "C" int erd_probe_build(void) { return &erd_probe_build_marker != nullptr ? erd_probe_build_marker : 0; }
extern "C" const char* erd_last_error(void) { return erd::g_err; }
namespace erd {
static int g_cu_reserve = 0;
int usable_cus(int physical) { return physical - g_cu_reserve >= 8 ? physical - g_cu_reserve : (physical < 8 ? physical : 8); }
}  // namespace erd
// ABI v6: CUs every later launch leaves free (persistent Winograd grids, stream-K grids, the activation-stationary kernel's grid, and --
// through erd_usable_cus -- the caller's one-round weight-gradient splits); n < 0 only queries.  Returns the previous reserve.
extern "C" int erd_set_cu_reserve(int n) {
    const int prev = erd::g_cu_reserve;
    if (n >= 0) erd::g_cu_reserve = n;
    return prev;
}
extern "C" int erd_usable_cus(void) {
    int dev = 0, n = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) n = prop.multiProcessorCount;
    return erd::usable_cus(n);
}

namespace {

// ------------------------------------------------------------------------------------------------
// stem: conv 7x7 stride 2 pad 3, 3->64, input NCHW (the detector's public input layout), output NHWC,
// frozen BN + ReLU fused (resnet.py:636-638).  Implicit GEMM on the fp32 matrix cores: M = 8x32 output pixels per
// block (one 32-pixel row per MFMA row block, two per wave), N = 64 channels, K = 7*7*3 = 147 (+1 zero row) in
// the weights' own (kh, kw, c) order.  The 21x69x3 input patch and the [148][64] weight image live in LDS; the A
// operand is gathered straight from the patch (lane = pixel, the k-th patch offset is a compile-time constant per
// lane half), the B operand is a conflict-free row read.
// ------------------------------------------------------------------------------------------------
constexpr int ST_TH = 8, ST_TW = 32;
constexpr int ST_PH = ST_TH * 2 + 5, ST_PW = ST_TW * 2 + 5;  // 21 x 69
constexpr int ST_PWP = ST_PW + 1;                             // padded row
constexpr int ST_K = 148;

__host__ __device__ constexpr int stem_patch_off(int k) {     // (kh, kw, c) -> offset inside patch[3][21][70]
    return k >= 147 ? 0 : (k % 3) * ST_PH * ST_PWP + (k / 21) * ST_PWP + (k / 3) % 7;
}

__global__ __launch_bounds__(256, 2) void stem_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* __restrict__ out, int N, int H, int W, int OH, int OW) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    constexpr int WLD = 65;                    // padded weight row: conflict-free transposing store and row reads
    constexpr int PATCH = 3 * ST_PH * ST_PWP, NLOAD = (3 * ST_PH * ST_PW + 255) / 256;
    __shared__ float wl[ST_K * WLD];           // [(kh,kw,c)][co], row 147 = 0
    __shared__ float patch[2][PATCH];
    // scale / shift in LDS: as global loads inside the store loop each of them sat between two stores, and gfx950 retires loads and
    // stores through one in-order counter -- every store waited for the previous one's acknowledgement (EXPERIMENTS 7f); registers
    // do not hold them either (the kernel sits at 256)
    __shared__ __attribute__((aligned(16))) float ssl[128];
    const int tid = threadIdx.x;
    if (tid < 128) ssl[tid] = tid < 64 ? scale[tid] : shift[tid - 64];
    // weights arrive as [co][kh][kw][c] (OHWI); LDS wants [(kh,kw,c)][co].  Loaded ONCE: the grid is persistent.
    for (int i = tid; i < 147 * 64; i += 256) {
        const int co = i / 147, k = i - co * 147;
        wl[k * WLD + co] = w[i];
    }
    if (tid < 64) wl[147 * WLD + tid] = 0.f;
    const int tx_n = (OW + ST_TW - 1) / ST_TW, ty_n = (OH + ST_TH - 1) / ST_TH;
    const int total = tx_n * ty_n * N;

    float pv[NLOAD];
    auto fetch = [&](int t) {                  // the 21x69x3 input patch of tile t -> registers
        const int n = t / (tx_n * ty_n), rem = t - n * tx_n * ty_n;
        const int ih0 = (rem / tx_n) * ST_TH * 2 - 3, iw0 = (rem % tx_n) * ST_TW * 2 - 3;
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int i = tid + q * 256;
            const int c = i / (ST_PH * ST_PW);
            const int r = (i / ST_PW) % ST_PH;
            const int col = i % ST_PW;
            const int ih = ih0 + r, iw = iw0 + col;
            float v = 0.f;
            if (i < 3 * ST_PH * ST_PW && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                v = x[((int64_t)(n * 3 + c) * H + ih) * W + iw];
            pv[q] = v;
        }
    };
    auto stash = [&](float* dst) {
#pragma unroll
        for (int q = 0; q < NLOAD; ++q) {
            const int i = tid + q * 256;
            if (i < 3 * ST_PH * ST_PW) dst[(i / ST_PW) * ST_PWP + i % ST_PW] = pv[q];     // (c*PH + r) rows of PWP
        }
    };

    const int wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    int t = blockIdx.x;
    if (t < total) { fetch(t); stash(patch[0]); }
    __syncthreads();
    for (int it = 0; t < total; t += gridDim.x, ++it) {
        const float* pc = patch[it & 1];
        const bool more = t + (int)gridDim.x < total;
        if (more) fetch(t + gridDim.x);        // in flight behind the MFMAs of this tile
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        // pixel (row 2*wave + i, column li) of the tile -> patch origin (2*row, 2*col)
        const float* pa = pc + (2 * (2 * wave)) * ST_PWP + 2 * li;
        const float* pb = wl + h * WLD + li;
        // software pipeline: the operands of step ks+1 are read while the four MFMAs of step ks run; the scheduling
        // barrier keeps the compiler from hoisting all 296 LDS reads to the top (256 VGPRs + spills otherwise)
        const int off0 = h ? stem_patch_off(1) : stem_patch_off(0);
        float a0 = pa[off0], a1 = pa[off0 + 2 * ST_PWP], b0 = pb[0], b1 = pb[32];
#pragma unroll
        for (int ks = 0; ks < ST_K / 2; ++ks) {
            float na0 = 0.f, na1 = 0.f, nb0 = 0.f, nb1 = 0.f;
            if (ks + 1 < ST_K / 2) {
                const int off = h ? stem_patch_off(2 * ks + 3) : stem_patch_off(2 * ks + 2);
                na0 = pa[off]; na1 = pa[off + 2 * ST_PWP];
                nb0 = pb[(ks + 1) * 2 * WLD]; nb1 = pb[(ks + 1) * 2 * WLD + 32];
            }
            // weights are the A operand (rows = channels), pixels the B operand (columns): a lane then owns four
            // CONSECUTIVE channels of its pixel per accumulator quad -> 16-byte stores
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a0, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a1, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a1, acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
        }
        if (more) stash(patch[(it & 1) ^ 1]);  // that buffer was last read one tile ago (barrier in between)
        // acc[cb][pr][4g + q] of lane (li, h): channel cb*32 + 8g + 4h + q of pixel (row 2*wave + pr, column li)
        const int n = t / (tx_n * ty_n), rem = t - n * tx_n * ty_n;
        const int oh0 = (rem / tx_n) * ST_TH, ow0 = (rem % tx_n) * ST_TW;
        const int ow = ow0 + li;
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const int oh = oh0 + 2 * wave + pr;
            if (oh >= OH || ow >= OW) continue;
            float* o = out + ((int64_t)(n * OH + oh) * OW + ow) * 64 + 4 * h;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = cb * 32 + 8 * g;
                    const float4 sc = *reinterpret_cast<const float4*>(ssl + ch + 4 * h);
                    const float4 sh = *reinterpret_cast<const float4*>(ssl + 64 + ch + 4 * h);
                    float4 v;
                    v.x = fmaxf(acc[cb][pr][4 * g + 0] * sc.x + sh.x, 0.f);
                    v.y = fmaxf(acc[cb][pr][4 * g + 1] * sc.y + sh.y, 0.f);
                    v.z = fmaxf(acc[cb][pr][4 * g + 2] * sc.z + sh.z, 0.f);
                    v.w = fmaxf(acc[cb][pr][4 * g + 3] * sc.w + sh.w, 0.f);
                    *reinterpret_cast<float4*>(o + ch) = v;
                }
        }
        __syncthreads();
    }
}

template <typename T>      // T: storage cell of the output map (float | erd::bf16s)
__global__ __launch_bounds__(256) void maxpool_kernel(const float4* __restrict__ in, T* __restrict__ out, int N,
                                                      int H, int W, int C4, int OH, int OW) {
    const int64_t total = (int64_t)N * OH * OW * C4;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = i % C4;
        int64_t r = i / C4;
        const int ow = r % OW; r /= OW;
        const int oh = r % OH;
        const int n = r / OH;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int ih = oh * 2 - 1 + dy;
            if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iw = ow * 2 - 1 + dx;
                if ((unsigned)iw >= (unsigned)W) continue;
                const float4 v = in[((int64_t)(n * H + ih) * W + iw) * C4 + c];
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        erd::st4(out + i * 4, m);
    }
}

__global__ void bn_fold_kernel(const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ m,
                               const float* __restrict__ v, float eps, float* __restrict__ scale,
                               float* __restrict__ shift, int64_t n) {
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n) {
        const float s = g[i] * (1.0f / sqrtf(v[i] + eps));
        scale[i] = s;
        shift[i] = b[i] - m[i] * s;
    }
}

// dz = dy * (y>0) (dz may alias dy); colsum[c] += sum over rows of dz.  rows are [npix][C] with an image
// stride (level views of [N][A][C] buffers): row r -> img r / rows_per_img.
// Block (x = row range, y = column group of C4w float4s): thread (column c4 = tid % C4w, row lane = tid / C4w) streams
// float4s down its column, 4 rows in flight; the block combines its row lanes through LDS and issues ONE atomic per
// channel.  Same-address float atomics retire at ~6 per microsecond, so the grid is cut into 64-channel column groups
// x long row ranges (a few hundred adds per channel) rather than into many short full-width row ranges.
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_colsum_kernel(const T* __restrict__ y, const T* dy, T* dz,
                                                               int64_t npix, int C, int64_t nstride,
                                                               int64_t rows_per_img, float* __restrict__ colsum,
                                                               int use_relu, int rows_per_block, int C4w) {
    __shared__ float4 red[256];
    const int lanes = 256 / C4w;
    const int rl = threadIdx.x / C4w;
    const bool dense = nstride == rows_per_img * C;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r_end = min(npix, r_begin + rows_per_block);
    {
        const int c4 = blockIdx.y * C4w + threadIdx.x % C4w;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rl < lanes) {
            auto offset = [&](int64_t r) -> int64_t {
                if (dense) return r * C + c4 * 4;
                const int64_t img = r / rows_per_img;
                return img * nstride + (r - img * rows_per_img) * C + c4 * 4;
            };
            int64_t r = r_begin + rl;
            for (; r + 3 * lanes < r_end; r += 4 * lanes) {
                int64_t o[4];
                float4 g[4], yy[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    o[q] = offset(r + q * lanes);
                    g[q] = erd::ld4(dy + o[q]);
                    if (use_relu) yy[q] = erd::ld4(y + o[q]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (use_relu) {
                        g[q].x = yy[q].x > 0.f ? g[q].x : 0.f; g[q].y = yy[q].y > 0.f ? g[q].y : 0.f;
                        g[q].z = yy[q].z > 0.f ? g[q].z : 0.f; g[q].w = yy[q].w > 0.f ? g[q].w : 0.f;
                        erd::st4(dz + o[q], g[q]);
                    }
                    s.x += g[q].x; s.y += g[q].y; s.z += g[q].z; s.w += g[q].w;
                }
            }
            for (; r < r_end; r += lanes) {
                const int64_t o = offset(r);
                float4 g = erd::ld4(dy + o);
                if (use_relu) {
                    const float4 yy = erd::ld4(y + o);
                    g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f;
                    g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
                    erd::st4(dz + o, g);
                }
                s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
            }
        }
        if (colsum) {
            __syncthreads();
            red[threadIdx.x] = s;
            __syncthreads();
            if (threadIdx.x < C4w) {
                float4 t = red[threadIdx.x];
                for (int j = 1; j < lanes; ++j) {
                    const float4 v = red[threadIdx.x + j * C4w];
                    t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
                }
                atomicAdd(colsum + c4 * 4 + 0, t.x);
                atomicAdd(colsum + c4 * 4 + 1, t.y);
                atomicAdd(colsum + c4 * 4 + 2, t.z);
                atomicAdd(colsum + c4 * 4 + 3, t.w);
            }
        }
    }
}

// dbeta: [copies][C] replicated column sums (the input-gradient epilogues add into row blockIdx & (copies - 1)).  32 channels per
// workgroup, eight row lanes each: lane g folds rows g, g + 8, ... with four loads in flight (a single thread per channel walking 64
// rows is a chain of dependent L2 round trips: 20 us per launch on the trailing stream), then thread (0, c) adds the eight shares in
// row-lane order -- for copies <= 8 the sum order of the one-thread loop this replaces.
__global__ void __launch_bounds__(256) bn_dgamma_kernel(const float* __restrict__ rowdot, const float* __restrict__ dbeta, int copies,
                                                        const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta_out, int accumulate, int C) {
    __shared__ float part[8][32];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + c;
    float s = 0.f;
    if (i < C) {
        int r = g;
        for (; r + 24 < copies; r += 32) {
            const float a0 = dbeta[(int64_t)r * C + i], a1 = dbeta[(int64_t)(r + 8) * C + i];
            const float a2 = dbeta[(int64_t)(r + 16) * C + i], a3 = dbeta[(int64_t)(r + 24) * C + i];
            s += (a0 + a1) + (a2 + a3);
        }
        for (; r < copies; r += 8) s += dbeta[(int64_t)r * C + i];
    }
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && i < C) {
        float db = part[0][c];
#pragma unroll
        for (int j = 1; j < 8; ++j) db += part[j][c];
        if (dbeta_out) dbeta_out[i] = db;
        const float v = (1.0f / sqrtf(var[i] + eps)) * (rowdot[i] - mean[i] * db);
        dgamma[i] = accumulate ? dgamma[i] + v : v;
    }
}

// ------------------------------------------------------------------------------------------------
// GroupNorm(G groups) + ReLU over [N][A][C] with per-(image, level, group) statistics.
// stats_ws: double [N][nseg][G][2] (sum, sumsq) accumulated with f64 atomics, then folded to
// mean_rstd float [N][nseg][G][2].
// ------------------------------------------------------------------------------------------------
constexpr int GN_ROWS = 128;       // rows per block of the streaming (apply) kernels
constexpr int GN_STAT_ROWS = 512;  // rows per block of the statistics kernels (fewer atomics per byte)
// Rows each thread of a streaming kernel has in flight per tensor.  One 16-byte load per thread and tensor is ~11 KB per CU on the
// head's maps (712 workgroups on 256 CUs), which holds 3.8 TB/s; four are ~45 KB per CU, past the 20-40 KB that the copy rate needs
// at 0.75-1.5 us of loaded latency.  The apply kernels' 4 row lanes cover 16 rows per unrolled pass, eight passes per 128-row chunk,
// and the head's launch keeps 11 waves per CU.
constexpr int GN_FLIGHT = 4;
// The loads of an unrolled pass as the registers they fill (four floats, or four bf16 in two dwords), all handed through ONE empty asm
// statement before the first is used: left alone, the optimizer sinks each load to its first use and the scheduler then keeps one or
// two in flight to save registers (a scheduling fence does not stop the first).  No instruction of its own; the values are untouched.
typedef float raw_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned raw_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ raw_f32x4 ld4_raw(const float* p) { return *reinterpret_cast<const raw_f32x4*>(p); }
__device__ __forceinline__ raw_u32x2 ld4_raw(const erd::bf16s* p) { return *reinterpret_cast<const raw_u32x2*>(p); }
__device__ __forceinline__ float4 cooked(raw_f32x4 v) { return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ float4 cooked(raw_u32x2 v) { return erd::unpack4_bf16(make_uint2(v.x, v.y)); }
template <typename R>
__device__ __forceinline__ void loads_first(R (&a)[4]) {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));
}
template <typename R>
__device__ __forceinline__ void loads_first(R (&a)[4], R (&b)[4]) {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}

__device__ __forceinline__ int find_level(const erd_levels& lv, int64_t a) {
    int s = 0;
#pragma unroll 1
    for (; s < lv.nseg - 1; ++s)
        if (a < lv.off[s] + lv.cnt[s]) break;
    return s;
}

// grid: (chunks over A rows, N).  Each chunk of GN_ROWS rows lies inside one level (host pads the
// chunk table per level: blockIdx.x -> (level, first row) through cumulative chunk counts).
struct GnChunks {
    int nseg;
    int start[ERD_MAX_SEG + 1];
};
__device__ __forceinline__ void gn_chunk(const erd_levels& lv, const GnChunks& ch, int bx, int& s, int64_t& r0,
                                         int64_t& r1, int rows = GN_ROWS) {
    s = 0;
#pragma unroll 1
    for (; s < ch.nseg - 1; ++s)
        if (bx < ch.start[s + 1]) break;
    r0 = lv.off[s] + (int64_t)(bx - ch.start[s]) * rows;
    r1 = min(lv.off[s] + lv.cnt[s], r0 + rows);
}

// Statistics kernels: grid (row chunks, N, 4 column groups).  A block owns 16 float4 columns (64 channels = 8 groups)
// and 16 row lanes over a long row range: the same bytes in flight as a full-width block over a quarter of the rows,
// but a quarter of the same-address atomics (those retire at ~6 per microsecond and were the limiter).
template <int C, int G, typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ c, double* __restrict__ stats,
                                                       int64_t A, erd_levels lv, GnChunks ch) {
    constexpr int CPG = C / G;         // channels per group (8)
    static_assert(CPG == 8 && C == 256, "tuned for C=256, G=32");
    const int n = blockIdx.y;
    int s; int64_t r0, r1;
    gn_chunk(lv, ch, blockIdx.x, s, r0, r1, GN_STAT_ROWS);
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;  // 16 columns x 16 row lanes
    const int c4 = blockIdx.z * 16 + cl;
    float sum = 0.f, sq = 0.f;
    int64_t r = r0 + rl;
    for (; r + 48 < r1; r += 64) {
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = erd::ld4(c + ((int64_t)n * A + r + 16 * q) * C + c4 * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sum += v[q].x + v[q].y + v[q].z + v[q].w;
            sq += v[q].x * v[q].x + v[q].y * v[q].y + v[q].z * v[q].z + v[q].w * v[q].w;
        }
    }
    for (; r < r1; r += 16) {
        const float4 v = erd::ld4(c + ((int64_t)n * A + r) * C + c4 * 4);
        sum += v.x + v.y + v.z + v.w;
        sq += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    // a group = 2 adjacent float4 columns -> combine lane pairs
    sum += __shfl_xor(sum, 1, 64);
    sq += __shfl_xor(sq, 1, 64);
    __shared__ float red[16][8][2];
    if ((cl & 1) == 0) { red[rl][cl >> 1][0] = sum; red[rl][cl >> 1][1] = sq; }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int g = threadIdx.x >> 1, k = threadIdx.x & 1;
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += (double)red[q][g][k];
        atomicAdd(stats + (((int64_t)n * lv.nseg + s) * G + blockIdx.z * 8 + g) * 2 + k, t);
    }
}

__global__ void gn_finalize_kernel(const double* __restrict__ stats, float* __restrict__ mean_rstd, int N, int G,
                                   erd_levels lv, int cpg, float eps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int total = N * lv.nseg * G;
    if (i < total) {
        const int s = (i / G) % lv.nseg;
        const double m = (double)lv.cnt[s] * cpg;
        const double mean = stats[i * 2] / m;
        double var = stats[i * 2 + 1] / m - mean * mean;
        if (var < 0) var = 0;
        mean_rstd[i * 2] = (float)mean;
        mean_rstd[i * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

template <int C, int G, typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ c, T* __restrict__ y,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean_rstd, int64_t A, erd_levels lv,
                                                       GnChunks ch) {
    const int n = blockIdx.y;
    int s; int64_t r0, r1;
    gn_chunk(lv, ch, blockIdx.x, s, r0, r1);
    const int c4 = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int g = c4 >> 1;
    const float2 mr = *reinterpret_cast<const float2*>(mean_rstd + (((int64_t)n * lv.nseg + s) * G + g) * 2);
    const float4 ga = reinterpret_cast<const float4*>(gamma)[c4];
    const float4 be = reinterpret_cast<const float4*>(beta)[c4];
#define GN_ROW(V, OFF)                                                     \
        {                                                                  \
            const float4 v = V;                                            \
            float4 o;                                                      \
            o.x = fmaxf((v.x - mr.x) * mr.y * ga.x + be.x, 0.f);           \
            o.y = fmaxf((v.y - mr.x) * mr.y * ga.y + be.y, 0.f);           \
            o.z = fmaxf((v.z - mr.x) * mr.y * ga.z + be.z, 0.f);           \
            o.w = fmaxf((v.w - mr.x) * mr.y * ga.w + be.w, 0.f);           \
            erd::st4(y + (OFF), o);                                        \
        }
    int64_t r = r0 + rl;
#pragma unroll 1
    for (; r + 4 * (GN_FLIGHT - 1) < r1; r += 4 * GN_FLIGHT) {      // GN_FLIGHT rows in flight per thread
        const int64_t off = ((int64_t)n * A + r) * C + c4 * 4;
        decltype(ld4_raw(c)) vv[GN_FLIGHT];
#pragma unroll
        for (int q = 0; q < GN_FLIGHT; ++q) vv[q] = ld4_raw(c + off + (int64_t)q * 4 * C);
        loads_first(vv);
#pragma unroll
        for (int q = 0; q < GN_FLIGHT; ++q) GN_ROW(cooked(vv[q]), off + (int64_t)q * 4 * C)
    }
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (; r < r1; r += 4) {
        const int64_t off = ((int64_t)n * A + r) * C + c4 * 4;
        GN_ROW(erd::ld4(c + off), off)
    }
#undef GN_ROW
}

// backward pass 1: per (n,level,group) s1 = sum dyh, s2 = sum dyh*xhat (dyh = dy*mask*gamma);
// per channel dgamma += sum dy*mask*xhat, dbeta += sum dy*mask
template <int C, int G, typename T>
__global__ __launch_bounds__(256) void gn_bwd_stats_kernel(const T* __restrict__ c, const T* __restrict__ dy,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ mean_rstd,
                                                           double* __restrict__ stats, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int64_t A, erd_levels lv,
                                                           GnChunks ch) {
    const int n = blockIdx.y;
    int s; int64_t r0, r1;
    gn_chunk(lv, ch, blockIdx.x, s, r0, r1, GN_STAT_ROWS);
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;  // 16 columns x 16 row lanes (see gn_stats_kernel)
    const int c4 = blockIdx.z * 16 + cl;
    const int g = c4 >> 1;
    static_assert(GN_FLIGHT == 4, "the unrolled loop below steps 4 x 16 rows");
    const float2 mr = *reinterpret_cast<const float2*>(mean_rstd + (((int64_t)n * lv.nseg + s) * G + g) * 2);
    const float4 ga = reinterpret_cast<const float4*>(gamma)[c4];
    const float4 be = reinterpret_cast<const float4*>(beta)[c4];
    float s1 = 0.f, s2 = 0.f;
    float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = make_float4(0.f, 0.f, 0.f, 0.f);
#define GN_ONE(F)                                                          \
        {                                                                  \
            const float xh = (v.F - mr.x) * mr.y;                          \
            const float dm = (xh * ga.F + be.F > 0.f) ? d.F : 0.f;         \
            dg.F += dm * xh;                                               \
            db.F += dm;                                                    \
            {   /* the group sums feed dc: no product fused into them */   \
                _Pragma("clang fp contract(off)")                          \
                const float dh = dm * ga.F;                                \
                s1 += dh;                                                  \
                s2 += dh * xh;                                             \
            }                                                              \
        }
    // (s1 and s2 reach dc through the group sums.  The fp32 instantiation's two-row loop always compiled them as rounded products and
    // plain additions; left to the compiler, the four-row loop fuses one row's dm * gamma into s1 and its dh * xh into s2, and dc
    // moves in the last bit.  So both are spelled unfused, for every loop.)
    int64_t r = r0 + rl;
    // four rows of both tensors in flight per thread, then two, then one: every lane adds its rows in the order r, r + 16, ... whatever
    // the step, so s1, s2, dg and db are the sums they were
#pragma unroll 1
    for (; r + 48 < r1; r += 64) {
        const int64_t off = ((int64_t)n * A + r) * C + c4 * 4;
        decltype(ld4_raw(c)) vv[GN_FLIGHT], dd[GN_FLIGHT];
#pragma unroll
        for (int q = 0; q < GN_FLIGHT; ++q) {
            vv[q] = ld4_raw(c + off + (int64_t)q * 16 * C);
            dd[q] = ld4_raw(dy + off + (int64_t)q * 16 * C);
        }
        loads_first(vv, dd);
#pragma unroll
        for (int q = 0; q < GN_FLIGHT; ++q) { const float4 v = cooked(vv[q]), d = cooked(dd[q]); GN_ONE(x) GN_ONE(y) GN_ONE(z) GN_ONE(w) }
    }
    for (; r + 16 < r1; r += 32) {          // two rows in flight per thread
        const int64_t off0 = ((int64_t)n * A + r) * C + c4 * 4, off1 = off0 + (int64_t)16 * C;
        const float4 v0 = erd::ld4(c + off0), d0 = erd::ld4(dy + off0);
        const float4 v1 = erd::ld4(c + off1), d1 = erd::ld4(dy + off1);
        { const float4 v = v0, d = d0; GN_ONE(x) GN_ONE(y) GN_ONE(z) GN_ONE(w) }
        { const float4 v = v1, d = d1; GN_ONE(x) GN_ONE(y) GN_ONE(z) GN_ONE(w) }
    }
    for (; r < r1; r += 16) {
        const int64_t off = ((int64_t)n * A + r) * C + c4 * 4;
        const float4 v = erd::ld4(c + off);
        const float4 d = erd::ld4(dy + off);
        GN_ONE(x) GN_ONE(y) GN_ONE(z) GN_ONE(w)
    }
#undef GN_ONE
    s1 += __shfl_xor(s1, 1, 64);
    s2 += __shfl_xor(s2, 1, 64);
    __shared__ float red[16][8][2];
    __shared__ float4 redc[16][16][2];
    __shared__ __attribute__((aligned(16))) float outc[2][64];
    if ((cl & 1) == 0) { red[rl][cl >> 1][0] = s1; red[rl][cl >> 1][1] = s2; }
    redc[rl][cl][0] = dg;
    redc[rl][cl][1] = db;
    __syncthreads();
#ifdef ERD_GN_BWD_NOATOMICS     // timing probe (tools/build_probe.sh): what the 16 double and 128 float atomics of a workgroup cost -- only a
                                // workgroup whose first sum is a value no data gives issues them (results are wrong)
    if (red[0][0][0] != -1.2345e33f) return;
#endif
    if (threadIdx.x < 16) {
        const int gg = threadIdx.x >> 1, k = threadIdx.x & 1;
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += (double)red[q][gg][k];
        atomicAdd(stats + (((int64_t)n * lv.nseg + s) * G + blockIdx.z * 8 + gg) * 2 + k, t);
    } else if (threadIdx.x >= 64 && threadIdx.x < 80) {
        const int cc = threadIdx.x - 64;
        float4 a = redc[0][cc][0], b = redc[0][cc][1];
#pragma unroll
        for (int q = 1; q < 16; ++q) {
            a.x += redc[q][cc][0].x; a.y += redc[q][cc][0].y; a.z += redc[q][cc][0].z; a.w += redc[q][cc][0].w;
            b.x += redc[q][cc][1].x; b.y += redc[q][cc][1].y; b.z += redc[q][cc][1].z; b.w += redc[q][cc][1].w;
        }
        *reinterpret_cast<float4*>(&outc[0][cc * 4]) = a;
        *reinterpret_cast<float4*>(&outc[1][cc * 4]) = b;
    }
    // the workgroup's 64 dgamma and 64 dbeta shares as two wave-wide adds of 256 contiguous bytes each (one lane per channel), not eight
    // of 16 lanes at a 16-byte stride: the same sums in a quarter of the 64-byte atomic requests, all of which queue on 2 KB of addresses
    __syncthreads();
    if (threadIdx.x < 128) atomicAdd((threadIdx.x < 64 ? dgamma : dbeta) + blockIdx.z * 64 + (threadIdx.x & 63), outc[threadIdx.x >> 6][threadIdx.x & 63]);
}

// backward pass 2: dc = rstd * (dyh - (s1 + xhat*s2)/m)
template <int C, int G, typename T>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const T* __restrict__ c, const T* __restrict__ dy,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ mean_rstd,
                                                           const double* __restrict__ stats, T* __restrict__ dc,
                                                           int64_t A, erd_levels lv, GnChunks ch) {
    const int n = blockIdx.y;
    int s; int64_t r0, r1;
    gn_chunk(lv, ch, blockIdx.x, s, r0, r1);
    const int c4 = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int g = c4 >> 1;
    const int64_t si = ((int64_t)n * lv.nseg + s) * G + g;
    const float2 mr = *reinterpret_cast<const float2*>(mean_rstd + si * 2);
    const float inv_m = (float)(1.0 / ((double)lv.cnt[s] * (C / G)));
    const float m1 = (float)stats[si * 2] * inv_m, m2 = (float)stats[si * 2 + 1] * inv_m;
    const float4 ga = reinterpret_cast<const float4*>(gamma)[c4];
    const float4 be = reinterpret_cast<const float4*>(beta)[c4];
#define GN_ONE(F)                                                          \
        {                                                                  \
            const float xh = (v.F - mr.x) * mr.y;                          \
            const float dh = (xh * ga.F + be.F > 0.f) ? d.F * ga.F : 0.f;  \
            o.F = mr.y * (dh - m1 - xh * m2);                              \
        }
#define GN_ROW(V, D, OFF)                                                  \
        {                                                                  \
            const float4 v = V, d = D;                                     \
            float4 o;                                                      \
            GN_ONE(x) GN_ONE(y) GN_ONE(z) GN_ONE(w)                        \
            erd::st4(dc + (OFF), o);                                       \
        }
    int64_t r = r0 + rl;
#pragma unroll 1
    for (; r + 4 * (GN_FLIGHT - 1) < r1; r += 4 * GN_FLIGHT) {      // GN_FLIGHT rows of both tensors in flight per thread
        const int64_t off = ((int64_t)n * A + r) * C + c4 * 4;
        decltype(ld4_raw(c)) vv[GN_FLIGHT], dd[GN_FLIGHT];
#pragma unroll
        for (int q = 0; q < GN_FLIGHT; ++q) {
            vv[q] = ld4_raw(c + off + (int64_t)q * 4 * C);
            dd[q] = ld4_raw(dy + off + (int64_t)q * 4 * C);
        }
        loads_first(vv, dd);
#pragma unroll
        for (int q = 0; q < GN_FLIGHT; ++q) GN_ROW(cooked(vv[q]), cooked(dd[q]), off + (int64_t)q * 4 * C)
    }
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (; r < r1; r += 4) {
        const int64_t off = ((int64_t)n * A + r) * C + c4 * 4;
        GN_ROW(erd::ld4(c + off), erd::ld4(dy + off), off)
    }
#undef GN_ROW
#undef GN_ONE
}

GnChunks make_chunks(const erd_levels* lv, int rows = GN_ROWS) {
    GnChunks ch;
    ch.nseg = lv->nseg;
    int acc = 0;
    for (int s = 0; s < lv->nseg; ++s) {
        ch.start[s] = acc;
        acc += (int)((lv->cnt[s] + rows - 1) / rows);
    }
    ch.start[lv->nseg] = acc;
    for (int s = lv->nseg + 1; s <= ERD_MAX_SEG; ++s) ch.start[s] = acc;
    return ch;
}

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void upsample_add_kernel(T* __restrict__ fine, const T* __restrict__ coarse,
                                                           int N, int H, int W, int C4, int h, int w, int64_t fns,
                                                           int64_t cns) {
    const int64_t total = (int64_t)N * H * W * C4;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = i % C4;
        int64_t r = i / C4;
        const int x = r % W; r /= W;
        const int y = r % H;
        const int n = r / H;
        // F.interpolate(mode='nearest', size=(H,W)): src = floor(dst * (h/H)); exact 2x => dst>>1
        const int sy = min((int)((int64_t)y * h / H), h - 1), sx = min((int)((int64_t)x * w / W), w - 1);
        T* f = fine + n * fns + (((int64_t)y * W + x) * C4 + c) * 4;
        const float4 cv = erd::ld4(coarse + n * cns + (((int64_t)sy * w + sx) * C4 + c) * 4);
        float4 v = erd::ld4(f);
        v.x += cv.x; v.y += cv.y; v.z += cv.z; v.w += cv.w;
        erd::st4(f, v);
    }
}

// adjoint: dcoarse[sy,sx] += sum of dfine over the pixels that map to it
template <typename T>
__global__ __launch_bounds__(256) void upsample_add_bwd_kernel(const T* __restrict__ dfine,
                                                               T* __restrict__ dcoarse, int N, int H, int W,
                                                               int C4, int h, int w, int64_t fns, int64_t cns) {
    const int64_t total = (int64_t)N * h * w * C4;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = i % C4;
        int64_t r = i / C4;
        const int sx = r % w; r /= w;
        const int sy = r % h;
        const int n = r / h;
        // fine rows y with floor(y*h/H) == sy
        const int y0 = (int)(((int64_t)sy * H + h - 1) / h), y1 = (int)((((int64_t)sy + 1) * H + h - 1) / h);
        const int x0 = (int)(((int64_t)sx * W + w - 1) / w), x1 = (int)((((int64_t)sx + 1) * W + w - 1) / w);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int y = y0; y < min(y1, H); ++y)
            for (int x = x0; x < min(x1, W); ++x) {
                const float4 v = erd::ld4(dfine + n * fns + (((int64_t)y * W + x) * C4 + c) * 4);
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
        T* d = dcoarse + n * cns + (((int64_t)sy * w + sx) * C4 + c) * 4;
        float4 o = erd::ld4(d);
        o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
        erd::st4(d, o);
    }
}

// out[c] += sum over rows of x[r][c] for C % 4 == 0, in the shape of relu_bwd_colsum_kernel: block (x = row range, y = group of cw4
// float4 columns), thread (column tid % cw4, row lane tid / cw4) with four rows in flight, one combine through LDS, one atomic per
// channel and workgroup.  cw4 need not divide 256 (17 columns at the 68-channel head: 15 row lanes, one thread idle).  Adds to one
// address retire at ~40 per microsecond, so the grid is COLSUM_WGS long row ranges: the one-thread-per-channel form below, with a
// workgroup per 64 rows, spent its 36 us on 1 400 adds per channel.
#ifndef COLSUM_WGS
#define COLSUM_WGS 128
#endif
template <typename T>
__global__ __launch_bounds__(256) void colsum_vec_kernel(const T* __restrict__ x, int64_t rows, int C4, float* __restrict__ out,
                                                         int64_t rows_per_block, int cw4) {
    __shared__ float4 red[256];
    const int lanes = 256 / cw4;
    const int cl = threadIdx.x % cw4, rl = threadIdx.x / cw4;
    const int c4 = blockIdx.y * cw4 + cl;
    const int64_t r_begin = blockIdx.x * rows_per_block, r_end = min(rows, r_begin + rows_per_block);
    const int64_t C = (int64_t)C4 * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rl < lanes && c4 < C4) {
        const T* xc = x + c4 * 4;
        int64_t r = r_begin + rl;
        for (; r + 3 * lanes < r_end; r += 4 * lanes) {
            float4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = erd::ld4(xc + (r + q * lanes) * C);
#pragma unroll
            for (int q = 0; q < 4; ++q) { s.x += v[q].x; s.y += v[q].y; s.z += v[q].z; s.w += v[q].w; }
        }
        for (; r < r_end; r += lanes) {
            const float4 v = erd::ld4(xc + r * C);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    __shared__ __attribute__((aligned(16))) float sums[256];
    if (rl == 0) {
        float4 t = red[cl];
        for (int j = 1; j < lanes; ++j) {
            const float4 v = red[cl + j * cw4];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        *reinterpret_cast<float4*>(&sums[cl * 4]) = t;
    }
    __syncthreads();
    // one lane per channel: the adds of a workgroup are contiguous bytes (they all queue on the same C addresses)
    const int ch = blockIdx.y * cw4 * 4 + threadIdx.x;
    if (threadIdx.x < cw4 * 4 && ch < C) atomicAdd(out + ch, sums[threadIdx.x]);
}

// any C, 4-byte loads: the path of a channel count that is no multiple of 4 (a 70-class head) or of rows that are not 16-byte aligned
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, int64_t rows, int C,
                                                     float* __restrict__ out, int rows_per_block) {
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int64_t r = r0; r < r1; ++r) s += erd::ld1(x + r * C + c);
        atomicAdd(out + c, s);
    }
}

// dst[r][c] = c < C ? src[r][c] : 0 over [rows][Cp]: a channel count that is not a multiple of 4 brought to the GEMM kernels'
// 4-channel groups (the gfl_cls backward of a 70-class head runs at 80 channels)
__global__ __launch_bounds__(256) void pad_channels_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           int64_t rows, int C, int Cp) {
    const int64_t n = rows * Cp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / Cp;
        const int c = (int)(i - r * Cp);
        dst[i] = c < C ? src[r * C + c] : 0.f;
    }
}

// y = x * alpha[level]  over [N][A][C] (gfl_head.py:229 `scale(self.gfl_reg(reg_feat))`, one Scale per level)
__global__ __launch_bounds__(256) void level_scale_kernel(const float* __restrict__ x, const float* __restrict__ alphas,
                                                          float* __restrict__ y, int64_t A, int C, erd_levels lv,
                                                          GnChunks ch) {
    const int n = blockIdx.y;
    int s; int64_t r0, r1;
    gn_chunk(lv, ch, blockIdx.x, s, r0, r1);
    const float a = alphas[s];
    const int64_t base = ((int64_t)n * A + r0) * C, cnt = (r1 - r0) * C;
    for (int64_t i = threadIdx.x; i < cnt; i += 256) y[base + i] = x[base + i] * a;
}

// VEC (C % 4 == 0 and 16-byte aligned buffers: a chunk then starts and ends on a float4): 16-byte accesses, four in flight per thread.
// (The forward above keeps its 4-byte form: with float4s it measured 13.3 us against 13.0 on the head's 49 MB, a launch of that size
// being mostly ramp and tail.)
template <bool VEC>
__global__ __launch_bounds__(256) void level_scale_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const float* __restrict__ alphas, float* __restrict__ dx,
                                                              float* __restrict__ dalphas, int64_t A, int C,
                                                              erd_levels lv, GnChunks ch) {
    const int n = blockIdx.y;
    int s; int64_t r0, r1;
    gn_chunk(lv, ch, blockIdx.x, s, r0, r1);
    const float a = alphas[s];
    const int64_t base = ((int64_t)n * A + r0) * C, cnt = (r1 - r0) * C;
    float acc = 0.f;
    if constexpr (VEC) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x + base);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(dy + base);
        float4* __restrict__ dx4 = reinterpret_cast<float4*>(dx + base);
        const int64_t cnt4 = cnt >> 2;
#define LS_ONE(G, X, I)                                                                        \
        {                                                                                      \
            const float4 g = G, v = X;                                                         \
            acc += g.x * v.x; acc += g.y * v.y; acc += g.z * v.z; acc += g.w * v.w;            \
            dx4[I] = make_float4(g.x * a, g.y * a, g.z * a, g.w * a);                          \
        }
        int64_t i = threadIdx.x;
        for (; i + 3 * 256 < cnt4; i += 4 * 256) {
            raw_f32x4 gg[4], vv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { gg[q] = ld4_raw(dy + base + 4 * (i + q * 256)); vv[q] = ld4_raw(x + base + 4 * (i + q * 256)); }
            loads_first(gg, vv);
#pragma unroll
            for (int q = 0; q < 4; ++q) LS_ONE(cooked(gg[q]), cooked(vv[q]), i + q * 256)
        }
        for (; i < cnt4; i += 256) LS_ONE(g4[i], x4[i], i)
#undef LS_ONE
    } else {
        for (int64_t i = threadIdx.x; i < cnt; i += 256) {
            const float g = dy[base + i];
            acc += g * x[base + i];
            dx[base + i] = g * a;
        }
    }
    acc = erd::wave_sum(acc);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dalphas + s, red[0] + red[1] + red[2] + red[3]);
}

// ---- optimizer update with parameter groups, gradient clipping, gradient accumulation ---------------------------------
// The segment table: entry s covers the elements [seg[s].begin, seg[s + 1].begin) of the flat buffers (absolute offsets; `base`
// is where p / g / buf start), with the learning-rate multiplier and the ABSOLUTE weight decay of its parameter.  A block's 256
// float4 are contiguous: the table is searched once per tile for the tile's first element (block-uniform loads), each lane then
// walks forward to its own segment -- at most a few entries, segments start on multiples of 4 floats (in the trainer: of 64).
// -> the last entry whose begin <= e0 (the launcher checked seg[0].begin <= base)
__device__ __forceinline__ int seg_of_tile(const erd_sgd_seg* __restrict__ seg, int nseg, int64_t e0) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].begin <= e0) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// torch.optim.SGD (momentum, weight decay) over [base, base + 4 * n4) of the flat buffers, a tile of 256 float4 per block and sweep.
// GROUPS: lr0 * lr_mult and the weight decay of each element's table entry (wd0 is not read), `coef` an optional device float
// that multiplies gs0 (the clip coefficient); otherwise lr0 and wd0 for every element, and neither table nor coef is touched.
template <bool GROUPS>
__global__ __launch_bounds__(256) void sgd_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                  float4* __restrict__ buf, int64_t n4, int64_t base,
                                                  const erd_sgd_seg* __restrict__ seg, int nseg, float lr0, float mom, float wd0,
                                                  float gs0, const float* __restrict__ coef, int first) {
    const float gs = GROUPS && coef ? gs0 * coef[0] : gs0;
    for (int64_t t0 = blockIdx.x * 256ll; t0 < n4; t0 += (int64_t)gridDim.x * 256) {
        const int lo = GROUPS ? seg_of_tile(seg, nseg, base + t0 * 4) : 0;
        const int64_t i = t0 + threadIdx.x;
        if (i >= n4) continue;
        float lr = lr0, wd = wd0;
        if (GROUPS) {
            const int64_t e = base + i * 4;
            int s = lo;
            while (s + 1 < nseg && seg[s + 1].begin <= e) ++s;
            lr = lr0 * seg[s].lr_mult;
            wd = seg[s].weight_decay;
        }
        float4 pp = p[i];
        const float4 gg = g[i];
        float4 d;
        d.x = gg.x * gs + wd * pp.x; d.y = gg.y * gs + wd * pp.y;
        d.z = gg.z * gs + wd * pp.z; d.w = gg.w * gs + wd * pp.w;
        float4 b;
        if (first) {
            b = d;
        } else {
            b = buf[i];
            b.x = mom * b.x + d.x; b.y = mom * b.y + d.y; b.z = mom * b.z + d.z; b.w = mom * b.w + d.w;
        }
        buf[i] = b;
        pp.x -= lr * b.x; pp.y -= lr * b.y; pp.z -= lr * b.z; pp.w -= lr * b.w;
        p[i] = pp;
    }
}

// torch.optim.AdamW (decoupled != 0) / torch.optim.Adam (decay joins the gradient) over the same flat buffers with the same segment
// table, tile search and clip coefficient as sgd_kernel<true>; `seg` null: one learning rate lr0 and one decay wd0.  m / v: first and
// second moment.  omb1 = 1 - beta1 and omb2 = 1 - beta2 are rounded from the host's doubles (1 - float(0.999) is 1.3e-5 off 0.001);
// ib1 = 1 / (1 - beta1^t), isb2 = 1 / sqrt(1 - beta2^t).  28 B per element, no reuse: an HBM pass like the SGD one.  Divide and
// square root are the compiler's correctly rounded ones, the fused multiply-adds are written out (the bits do not hang on what
// the compiler contracts).  Zero padding stays zero (0 / (0 + eps)).
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float wd, float decay, float beta2,
                                          float omb1, float omb2, float eps, float step, float isb2, int decoupled) {
    if (decoupled) p *= decay; else g = fmaf(wd, p, g);
    m = fmaf(g - m, omb1, m);
    v = fmaf(beta2, v, (omb2 * g) * g);
    p = fmaf(-step, m / fmaf(sqrtf(v), isb2, eps), p);
}

__global__ __launch_bounds__(256) void adam_groups_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                          float4* __restrict__ m, float4* __restrict__ v, int64_t n4, int64_t base,
                                                          const erd_sgd_seg* __restrict__ seg, int nseg, float lr0, float wd0,
                                                          float beta2, float omb1, float omb2, float eps, float ib1, float isb2,
                                                          float gs0, const float* __restrict__ coef, int decoupled) {
    const float gs = coef ? gs0 * coef[0] : gs0;
    for (int64_t t0 = blockIdx.x * 256ll; t0 < n4; t0 += (int64_t)gridDim.x * 256) {
        const int lo = seg ? seg_of_tile(seg, nseg, base + t0 * 4) : 0;
        const int64_t i = t0 + threadIdx.x;
        if (i >= n4) continue;
        float lr = lr0, wd = wd0;
        if (seg) {
            const int64_t e = base + i * 4;
            int s = lo;
            while (s + 1 < nseg && seg[s + 1].begin <= e) ++s;
            lr = lr0 * seg[s].lr_mult;
            wd = seg[s].weight_decay;
        }
        const float decay = 1.f - lr * wd, step = lr * ib1;
        float4 pp = p[i], mm = m[i], vv = v[i];
        float4 gg = g[i];
        gg.x *= gs; gg.y *= gs; gg.z *= gs; gg.w *= gs;
        adam_elem(pp.x, gg.x, mm.x, vv.x, wd, decay, beta2, omb1, omb2, eps, step, isb2, decoupled);
        adam_elem(pp.y, gg.y, mm.y, vv.y, wd, decay, beta2, omb1, omb2, eps, step, isb2, decoupled);
        adam_elem(pp.z, gg.z, mm.z, vv.z, wd, decay, beta2, omb1, omb2, eps, step, isb2, decoupled);
        adam_elem(pp.w, gg.w, mm.w, vv.w, wd, decay, beta2, omb1, omb2, eps, step, isb2, decoupled);
        m[i] = mm;
        v[i] = vv;
        p[i] = pp;
    }
}

// sum of squares of g[0, n) as ERD_SQNORM_PARTS fp64 partials: workgroup b owns the float4 b*256 + t + k*PARTS*256 (a partition
// that depends on n alone), every lane accumulates the exact fp64 squares of its elements in index order, the lanes fold through
// the wave butterfly and the four waves in order.  No float atomics: the same gradient gives the same bits on every run.
__device__ __forceinline__ double block_sum_d(double acc) {
    acc = erd::wave_sum_d(acc);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float4* __restrict__ g, int64_t n4, double* __restrict__ part) {
    double acc = 0.0;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)ERD_SQNORM_PARTS * 256) {
        const float4 v = g[i];
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    const double s = block_sum_d(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ part, int64_t nparts, float gs, float max_norm,
                                                        float* __restrict__ out) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) acc += part[i];
    const double s = block_sum_d(acc);
    if (threadIdx.x == 0) {
        const float total = (float)((double)gs * sqrt(s));
        const float c = max_norm / (total + 1e-6f);
        out[0] = total;
        out[1] = c < 1.f ? c : 1.f;
    }
}

__global__ __launch_bounds__(256) void grad_accumulate_kernel(float4* __restrict__ acc, const float4* __restrict__ g, int64_t n4,
                                                              int first) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 a = g[i];
        if (!first) {
            const float4 o = acc[i];
            a.x = o.x + a.x; a.y = o.y + a.y; a.z = o.z + a.z; a.w = o.w + a.w;
        }
        acc[i] = a;
    }
}

// ---- weight averaging (EMAHook) over a range of two flat buffers -----------------------------------------------------------
// ema = fmaf(p, c, ema * d) per element -- the multiply rounded on its own, then ONE fused multiply-add: what
// `averaged.mul_(1 - c).add_(src, alpha=c)` computes on an FMA host; c and d = 1 - c are rounded from the host's doubles.  COPY:
// ema = p.  12 B per element (8 B copying), no reuse: an HBM pass.  Whole float4 lanes grid-stride, the n % 4 elements behind the
// last whole lane go to the first lanes of block 0 one by one; nothing outside [0, n) is read or written.
__device__ __forceinline__ float ema_elem(float e, float p, float c, float d) { return fmaf(p, c, __fmul_rn(e, d)); }

template <bool COPY>
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n, float c, float d) {
    const int64_t n4 = n >> 2;
    float4* __restrict__ e4 = reinterpret_cast<float4*>(ema);
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 s = p4[i];
        if (!COPY) {
            const float4 a = e4[i];
            s.x = ema_elem(a.x, s.x, c, d); s.y = ema_elem(a.y, s.y, c, d);
            s.z = ema_elem(a.z, s.z, c, d); s.w = ema_elem(a.w, s.w, c, d);
        }
        e4[i] = s;
    }
    const int64_t t = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < n) ema[t] = COPY ? p[t] : ema_elem(ema[t], p[t], c, d);
}

// a[0, n) <-> b[0, n): every element is read and written by one lane, so no third buffer and no ordering between lanes
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
    const int64_t n4 = n >> 2;
    float4* __restrict__ a4 = reinterpret_cast<float4*>(a);
    float4* __restrict__ b4 = reinterpret_cast<float4*>(b);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    const int64_t t = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && t < n) {
        const float x = a[t], y = b[t];
        a[t] = y;
        b[t] = x;
    }
}

inline int grid_for(int64_t n, int cap = 2048) {
    int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// the grid of a streaming pass over n4 float4: one block per 256 lanes up to eight blocks per usable CU, the rest grid-strides
// (the physical CU count is asked once: hipGetDeviceProperties is no per-launch call; the reserve is read every time)
inline int stream_grid(int64_t n4) {
    static int physical = 0;
    if (physical == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        physical = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0
                       ? prop.multiProcessorCount : 256;
    }
    return grid_for(n4, 8 * erd::usable_cus(physical));
}

inline bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }
inline bool disjoint(const float* a, const float* b, int64_t n) { return a + n <= b || b + n <= a; }

}  // namespace

extern "C" int erd_stem_conv7x7_bn_relu(const float* x, const float* w, const float* scale, const float* shift,
                                        float* out, int N, int H, int W, erd_stream_t stream) {
    ERD_REQUIRE(x && w && scale && shift && out && N > 0, "stem: bad args");
    const int OH = (H + 6 - 7) / 2 + 1, OW = (W + 6 - 7) / 2 + 1;
    const int64_t tiles = (int64_t)((OW + ST_TW - 1) / ST_TW) * ((OH + ST_TH - 1) / ST_TH) * N;
    ERD_REQUIRE(tiles < (1ll << 31), "stem: too many tiles");
    hipLaunchKernelGGL(stem_kernel, dim3((unsigned)(tiles < 512 ? tiles : 512)), dim3(256), 0,       // persistent: 2 per CU
                       (hipStream_t)stream, x, w, scale, shift, out, N, H, W, OH, OW);
    return erd::check_launch("stem");
}

// map_type dispatch of the templated kernels: ERD_MAP(T, statement using T)
#define ERD_MAP(map_type, ...)                                   \
    do {                                                         \
        if ((map_type) == ERD_BF16) { using T = erd::bf16s; __VA_ARGS__; } \
        else { using T = float; __VA_ARGS__; }                   \
    } while (0)
#define ERD_MAP_OK(map_type) ((map_type) == ERD_F32 || (map_type) == ERD_BF16)

extern "C" int erd_maxpool3x3s2(const float* in, void* out, int N, int H, int W, int C, int out_type, erd_stream_t stream) {
    ERD_REQUIRE(in && out && C % 4 == 0 && ERD_MAP_OK(out_type), "maxpool: bad args");
    const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
    const int64_t total = (int64_t)N * OH * OW * (C / 4);
    ERD_MAP(out_type, hipLaunchKernelGGL(maxpool_kernel<T>, dim3(grid_for(total, 8192)), dim3(256), 0, (hipStream_t)stream,
                                         reinterpret_cast<const float4*>(in), reinterpret_cast<T*>(out), N, H, W, C / 4, OH, OW));
    return erd::check_launch("maxpool");
}

namespace {
// DetDataPreprocessor (data_preprocessor.py:110-183 + mmengine ImgDataPreprocessor): one image [3][h][w] (uint8 or
// fp32, CHW) -> its slot [3][H][W] of the batch: optional channel flip, float, (x - mean) / std, pad_value beyond
// (h, w).  The subtraction and the division stay two IEEE operations (no reciprocal, no fma), so the result is
// bit-identical to the host arithmetic.
template <typename T>
__global__ __launch_bounds__(256) void preprocess_kernel(const T* __restrict__ img, int h, int w, float* __restrict__ out,
                                                         int H, int W, float m0, float m1, float m2, float s0, float s1,
                                                         float s2, int flip, float pad_value) {
    const int64_t plane = (int64_t)H * W;
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= plane) return;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    const bool inside = y < h && x < w;
    const int64_t src = (int64_t)y * w + x;
    const int64_t sp = (int64_t)h * w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = pad_value;
        if (inside) {
            const float px = (float)img[(flip ? 2 - c : c) * sp + src];
            const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
            v = __fdiv_rn(__fsub_rn(px, mean), sd);
        }
        out[c * plane + i] = v;
    }
}
}  // namespace

namespace {
__global__ __launch_bounds__(256) void to_bf16_kernel(const float4* __restrict__ src, uint2* __restrict__ dst, int64_t n4,
                                                      const float* __restrict__ tail_src, unsigned short* __restrict__ tail_dst,
                                                      int ntail) {
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = src[i];
        const f2 a = {v.x, v.y}, b = {v.z, v.w};
        uint2 o;
        o.x = __builtin_bit_cast(unsigned, __builtin_convertvector(a, bf2));
        o.y = __builtin_bit_cast(unsigned, __builtin_convertvector(b, bf2));
        dst[i] = o;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) {
        const f2 a = {tail_src[threadIdx.x], 0.f};
        tail_dst[threadIdx.x] = (unsigned short)(__builtin_bit_cast(unsigned, __builtin_convertvector(a, bf2)) & 0xffffu);
    }
}
}  // namespace

extern "C" int erd_to_bf16(const float* src, void* dst, int64_t n, erd_stream_t stream) {
    ERD_REQUIRE(src && dst && n >= 0, "to_bf16: bad args");
    if (n == 0) return 0;
    const int64_t n4 = n / 4;
    const int ntail = (int)(n - n4 * 4);
    hipLaunchKernelGGL(to_bf16_kernel, dim3(grid_for(n4 > 0 ? n4 : 1, 4096)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(src), reinterpret_cast<uint2*>(dst), n4, src + n4 * 4,
                       reinterpret_cast<unsigned short*>(dst) + n4 * 4, ntail);
    return erd::check_launch("to_bf16");
}

extern "C" int erd_preprocess_image(const void* img, int is_uint8, int h, int w, float* out, int H, int W,
                                    const float* mean3, const float* std3, int flip_channels, float pad_value,
                                    erd_stream_t stream) {
    ERD_REQUIRE(img && out && mean3 && std3, "preprocess: null");
    ERD_REQUIRE(h > 0 && w > 0 && H >= h && W >= w, "preprocess: image %dx%d does not fit the %dx%d slot", h, w, H, W);
    const int64_t plane = (int64_t)H * W;
    const dim3 grid((unsigned)((plane + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    if (is_uint8)
        hipLaunchKernelGGL(preprocess_kernel<uint8_t>, grid, dim3(256), 0, st, reinterpret_cast<const uint8_t*>(img), h, w,
                           out, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], flip_channels, pad_value);
    else
        hipLaunchKernelGGL(preprocess_kernel<float>, grid, dim3(256), 0, st, reinterpret_cast<const float*>(img), h, w, out,
                           H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], flip_channels, pad_value);
    return erd::check_launch("preprocess");
}

namespace {
// Resize(keep_ratio) + RandomFlip + DetDataPreprocessor fused: one thread per OUTPUT pixel of the
// padded [3][H][W] slot.  The 8-bit bilinear resize follows OpenCV's fixed-point two-pass scheme (coefficient tables are
// built on the host exactly as the test oracle builds them): rows = S[x0]*a0 + S[x1]*a1 (int, x2048), then
// u8 = (((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2, and only then float, (v - mean) / std.
__global__ __launch_bounds__(256) void resize_normalize_kernel(const uint8_t* __restrict__ src, int sh, int sw,
                                                               const int* __restrict__ xofs, const short* __restrict__ xco,
                                                               const int* __restrict__ yofs, const short* __restrict__ yco,
                                                               int nh, int nw, float* __restrict__ out, int H, int W, float m0,
                                                               float m1, float m2, float s0, float s1, float s2, int flip,
                                                               int swap_rb, float pad_value) {
    const int64_t plane = (int64_t)H * W;
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= plane) return;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    if (y >= nh || x >= nw) {
        out[i] = pad_value; out[plane + i] = pad_value; out[2 * plane + i] = pad_value;
        return;
    }
    const int xs = flip ? nw - 1 - x : x;                       // flipping the resized image == reading it mirrored
    const int x0 = xofs[xs], x1 = min(x0 + 1, sw - 1);
    const int y0 = yofs[y], y1 = min(y0 + 1, sh - 1);
    const int a0 = xco[2 * xs], a1 = xco[2 * xs + 1], b0 = yco[2 * y], b1 = yco[2 * y + 1];
    const uint8_t* r0 = src + (int64_t)y0 * sw * 3;
    const uint8_t* r1 = src + (int64_t)y1 * sw * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int cs = swap_rb ? 2 - c : c;
        const int t0 = r0[x0 * 3 + cs] * a0 + r0[x1 * 3 + cs] * a1;
        const int t1 = r1[x0 * 3 + cs] * a0 + r1[x1 * 3 + cs] * a1;
        int v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
        v = min(max(v, 0), 255);
        const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
        out[c * plane + i] = __fdiv_rn(__fsub_rn((float)v, mean), sd);
    }
}
}  // namespace

extern "C" int erd_resize_normalize(const void* src_hwc_u8, int sh, int sw, const int* xofs, const short* xcoef,
                                    const int* yofs, const short* ycoef, int nh, int nw, float* out, int H, int W,
                                    const float* mean3, const float* std3, int flip, int swap_rb, float pad_value,
                                    erd_stream_t stream) {
    ERD_REQUIRE(src_hwc_u8 && xofs && xcoef && yofs && ycoef && out && mean3 && std3, "resize_normalize: null");
    ERD_REQUIRE(sh > 0 && sw > 0 && nh > 0 && nw > 0 && H >= nh && W >= nw, "resize_normalize: bad sizes");
    const int64_t plane = (int64_t)H * W;
    hipLaunchKernelGGL(resize_normalize_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint8_t*>(src_hwc_u8), sh, sw, xofs, xcoef, yofs, ycoef, nh, nw, out, H, W,
                       mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], flip, swap_rb, pad_value);
    return erd::check_launch("resize_normalize");
}

namespace {
// One axis of datasets.linear_coeffs for ONE output index d, bit for bit: scale = 1.0 / (double(dst) / double(src)) as the caller
// formed it, f = float((d + 0.5) * scale - 0.5) with the product and the difference rounded SEPARATELY in double (numpy evaluates
// them as two array operations; a contracted v_fma_f64 is a different function), floor, the two clamps, then the 11-bit weights
// c1 = rint(double(f) * 2048), c0 = rint(double(float(1.0f - f)) * 2048) (round half to even, as np.rint).
// The product and the difference are written as OPERATORS under `fp contract(off)`: __dmul_rn / __dsub_rn are inline `x * y` / `x - y`
// in this toolchain's headers, compiled there with contraction allowed, and came out of this function fused (v_fma_f64 in the ISA).
__device__ __forceinline__ void linear_coeff(int d, double scale, int src, int& ofs, int& c0, int& c1) {
#pragma clang fp contract(off)
    const double t = ((double)d + 0.5) * scale;
    float f = (float)(t - 0.5);
    int s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    ofs = s;
    c1 = (int)rint((double)f * 2048.0);
    c0 = (int)rint((double)__fsub_rn(1.0f, f) * 2048.0);
}

__device__ __forceinline__ double linear_scale(int src, int dst) {
    return __ddiv_rn(1.0, __ddiv_rn((double)dst, (double)src));
}

// resize_normalize_kernel over a whole batch in one launch, without host-built tables: blockIdx.y is the image, a thread owns four
// consecutive x of one row of the padded [3][H][W] slot and computes its own coefficients (one y set, four x sets).  The pixel
// arithmetic is resize_normalize_kernel's.  VEC: W % 4 == 0 and a 16-byte aligned output, so each plane gets one float4 store;
// otherwise scalar stores with the row end checked.  A record that does not fit the source buffer reads nothing (its slot is padding).
template <bool VEC>
__global__ __launch_bounds__(256) void resize_normalize_batch_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                     const erd_resize_item* __restrict__ items,
                                                                     float* __restrict__ out, int H, int W, float m0, float m1,
                                                                     float m2, float s0, float s1, float s2, int swap_rb,
                                                                     float pad_value) {
    const int W4 = (W + 3) >> 2;
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (int64_t)H * W4) return;
    const int y = (int)(i / W4), x = (int)(i - (int64_t)y * W4) * 4;
    const erd_resize_item it = items[blockIdx.y];
    const int sh = it.sh, sw = it.sw, nh = it.nh, nw = it.nw;
    const bool ok = sh > 0 && sw > 0 && nh > 0 && nw > 0 && it.offset >= 0 && it.offset + (int64_t)sh * sw * 3 <= src_bytes;
    const int64_t plane = (int64_t)H * W;
    float* o = out + (int64_t)blockIdx.y * 3 * plane + (int64_t)y * W + x;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[c][j] = pad_value;
    if (ok && y < nh && x < nw) {
        int y0, b0, b1;
        linear_coeff(y, linear_scale(sh, nh), sh, y0, b0, b1);
        const int y1 = min(y0 + 1, sh - 1);
        const uint8_t* r0 = src + it.offset + (int64_t)y0 * sw * 3;
        const uint8_t* r1 = src + it.offset + (int64_t)y1 * sw * 3;
        const double xscale = linear_scale(sw, nw);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x + j >= nw) continue;
            const int xs = it.flip ? nw - 1 - (x + j) : x + j;          // flipping the resized image == reading it mirrored
            int x0, a0, a1;
            linear_coeff(xs, xscale, sw, x0, a0, a1);
            const int x1 = min(x0 + 1, sw - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cs = swap_rb ? 2 - c : c;
                const int t0 = r0[x0 * 3 + cs] * a0 + r0[x1 * 3 + cs] * a1;
                const int t1 = r1[x0 * 3 + cs] * a0 + r1[x1 * 3 + cs] * a1;
                int u = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
                u = min(max(u, 0), 255);
                const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
                v[c][j] = __fdiv_rn(__fsub_rn((float)u, mean), sd);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (VEC) {
            *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) o[c * plane + j] = v[c][j];
        }
    }
}
}  // namespace

extern "C" int erd_resize_normalize_batch(const void* src_u8, int64_t src_bytes, const erd_resize_item* items_dev, int n,
                                          float* out, int H, int W, const float* mean3, const float* std3, int swap_rb,
                                          float pad_value, erd_stream_t stream) {
    ERD_REQUIRE(src_u8 && items_dev && out && mean3 && std3, "resize_normalize_batch: null");
    ERD_REQUIRE(src_bytes > 0 && n > 0 && n <= 65535 && H > 0 && W > 0, "resize_normalize_batch: bad sizes");
    const int64_t work = (int64_t)H * ((W + 3) / 4);
    const dim3 grid((unsigned)((work + 255) / 256), (unsigned)n);
    const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(src_u8);
    if (vec)
        hipLaunchKernelGGL(resize_normalize_batch_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, s, src_bytes, items_dev,
                           out, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], swap_rb, pad_value);
    else
        hipLaunchKernelGGL(resize_normalize_batch_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, s, src_bytes, items_dev,
                           out, H, W, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], swap_rb, pad_value);
    return erd::check_launch("resize_normalize_batch");
}

extern "C" int erd_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                           float* scale, float* shift, int64_t n, erd_stream_t stream) {
    ERD_REQUIRE(gamma && beta && mean && var && scale && shift, "bn_fold: null");
    if (n == 0) return 0;
    hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gamma,
                       beta, mean, var, eps, scale, shift, n);
    return erd::check_launch("bn_fold");
}

namespace {
__global__ __launch_bounds__(256) void bn_fold_batch_kernel(const erd_bn_fold_item* __restrict__ items) {
    const erd_bn_fold_item it = items[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < it.n) {
        const float s = it.gamma[i] * (1.0f / sqrtf(it.var[i] + it.eps));      // (the arithmetic of bn_fold_kernel)
        it.scale[i] = s;
        it.shift[i] = it.beta[i] - it.mean[i] * s;
    }
}
}  // namespace

extern "C" int erd_bn_fold_batch(const erd_bn_fold_item* items_dev, int nitems, int max_n, erd_stream_t stream) {
    ERD_REQUIRE(items_dev && nitems >= 0 && max_n >= 0, "bn_fold_batch: bad args");
    if (nitems == 0 || max_n == 0) return 0;
    hipLaunchKernelGGL(bn_fold_batch_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)nitems), dim3(256), 0,
                       (hipStream_t)stream, items_dev);
    return erd::check_launch("bn_fold_batch");
}

extern "C" int erd_relu_bwd_colsum(const void* y, const void* dy, void* dz, int64_t npix, int C,
                                   int64_t nstride_rows, int64_t rows_per_img, float* colsum, int use_relu,
                                   int map_type, erd_stream_t stream) {
    ERD_REQUIRE(dy && C % 4 == 0 && (!use_relu || (y && dz)) && ERD_MAP_OK(map_type), "relu_bwd: bad args");
    if (npix == 0) return 0;
    const int C4 = C / 4;
    ERD_REQUIRE(C4 % 16 == 0 || 256 % C4 == 0, "relu_bwd: C=%d unsupported", C);
    const int cw4 = C4 % 16 == 0 ? 16 : C4, gy = C4 / cw4, lanes = 256 / cw4;
    static const int blocks_env = getenv("ERD_RELU_BLOCKS") ? atoi(getenv("ERD_RELU_BLOCKS")) : 0;   // tuning aid
    const int want = blocks_env > 0 ? blocks_env : 512;
    const int unit = 4 * lanes;                                     // rows one pass of the unrolled loop covers
    int64_t rpb = (npix + (want / gy > 0 ? want / gy : 1) - 1) / (want / gy > 0 ? want / gy : 1);
    rpb = (rpb + unit - 1) / unit * unit;
    ERD_MAP(map_type, hipLaunchKernelGGL(relu_bwd_colsum_kernel<T>, dim3((unsigned)((npix + rpb - 1) / rpb), gy), dim3(256), 0,
                                         (hipStream_t)stream, (const T*)y, (const T*)dy, (T*)dz, npix, C, nstride_rows,
                                         rows_per_img, colsum, use_relu, (int)rpb, cw4));
    return erd::check_launch("relu_bwd_colsum");
}

extern "C" int erd_bn_dgamma(const float* rowdot, const float* dbeta, int copies, const float* mean, const float* var,
                             float eps, float* dgamma, float* dbeta_out, int accumulate, int C, erd_stream_t stream) {
    ERD_REQUIRE(rowdot && dbeta && mean && var && dgamma && copies >= 1, "bn_dgamma: bad args");
    hipLaunchKernelGGL(bn_dgamma_kernel, dim3((C + 31) / 32), dim3(256), 0, (hipStream_t)stream, rowdot, dbeta, copies,
                       mean, var, eps, dgamma, dbeta_out, accumulate, C);
    return erd::check_launch("bn_dgamma");
}

extern "C" int erd_gn_relu_fwd(const void* c, void* y, const float* gamma, const float* beta, double* stats_ws,
                               float* mean_rstd, int N, int64_t A, int C, int G, const erd_levels* lv, float eps,
                               int map_type, erd_stream_t stream) {
    ERD_REQUIRE(c && y && gamma && beta && stats_ws && mean_rstd && lv && ERD_MAP_OK(map_type), "gn_fwd: bad args");
    ERD_REQUIRE(C == 256 && G == 32, "gn_fwd: only C=256,G=32 (gfl_head.py:109-110) is built");
    hipStream_t st = (hipStream_t)stream;
    const GnChunks ch = make_chunks(lv);
    const GnChunks chs = make_chunks(lv, GN_STAT_ROWS);
    const int nst = N * lv->nseg * G;
    ERD_ZERO_ASYNC(stats_ws, sizeof(double) * 2 * nst, st);
#ifndef ERD_GN_NOSTATS      // timing probe (tools/build_probe.sh): the upper bound of what statistics fused into the producing
                            // convolution's output stage could save -- the pass is simply not run (results are wrong)
    ERD_MAP(map_type, hipLaunchKernelGGL((gn_stats_kernel<256, 32, T>), dim3(chs.start[lv->nseg], N, 4), dim3(256), 0, st,
                                         (const T*)c, stats_ws, A, *lv, chs));
#endif
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((nst + 255) / 256), dim3(256), 0, st, stats_ws, mean_rstd, N, G, *lv,
                       C / G, eps);
    ERD_MAP(map_type, hipLaunchKernelGGL((gn_apply_kernel<256, 32, T>), dim3(ch.start[lv->nseg], N), dim3(256), 0, st,
                                         (const T*)c, (T*)y, gamma, beta, mean_rstd, A, *lv, ch));
    return erd::check_launch("gn_relu_fwd");
}

// the normalisation pass alone: mean_rstd[N][nseg][G][2] comes from the producing convolution (erd_wino_conv3x3_x3_gn)
extern "C" int erd_gn_relu_apply(const void* c, void* y, const float* gamma, const float* beta, const float* mean_rstd, int N,
                                 int64_t A, int C, int G, const erd_levels* lv, int map_type, erd_stream_t stream) {
    ERD_REQUIRE(c && y && gamma && beta && mean_rstd && lv && ERD_MAP_OK(map_type), "gn_apply: bad args");
    ERD_REQUIRE(C == 256 && G == 32, "gn_apply: only C=256,G=32 (gfl_head.py:109-110) is built");
    const GnChunks ch = make_chunks(lv);
    ERD_MAP(map_type, hipLaunchKernelGGL((gn_apply_kernel<256, 32, T>), dim3(ch.start[lv->nseg], N), dim3(256), 0, (hipStream_t)stream,
                                         (const T*)c, (T*)y, gamma, beta, mean_rstd, A, *lv, ch));
    return erd::check_launch("gn_relu_apply");
}

extern "C" int erd_gn_relu_bwd(const void* c, const void* dy, const float* gamma, const float* beta,
                               const float* mean_rstd, double* stats_ws, void* dc, float* dgamma, float* dbeta, int N,
                               int64_t A, int C, int G, const erd_levels* lv, int map_type, erd_stream_t stream) {
    ERD_REQUIRE(c && dy && gamma && beta && mean_rstd && stats_ws && dc && dgamma && dbeta && lv && ERD_MAP_OK(map_type),
                "gn_bwd: bad args");
    ERD_REQUIRE(C == 256 && G == 32, "gn_bwd: only C=256,G=32 is built");
    hipStream_t st = (hipStream_t)stream;
    const GnChunks ch = make_chunks(lv);
    const GnChunks chs = make_chunks(lv, GN_STAT_ROWS);
    const int nst = N * lv->nseg * G;
    ERD_ZERO_ASYNC(stats_ws, sizeof(double) * 2 * nst, st);
    ERD_MAP(map_type, hipLaunchKernelGGL((gn_bwd_stats_kernel<256, 32, T>), dim3(chs.start[lv->nseg], N, 4), dim3(256), 0, st,
                                         (const T*)c, (const T*)dy, gamma, beta, mean_rstd, stats_ws, dgamma, dbeta, A, *lv, chs));
    ERD_MAP(map_type, hipLaunchKernelGGL((gn_bwd_apply_kernel<256, 32, T>), dim3(ch.start[lv->nseg], N), dim3(256), 0, st,
                                         (const T*)c, (const T*)dy, gamma, beta, mean_rstd, stats_ws, (T*)dc, A, *lv, ch));
    return erd::check_launch("gn_relu_bwd");
}

extern "C" int erd_upsample2x_add(void* fine, const void* coarse, int N, int H, int W, int C, int h, int w,
                                  int64_t fns, int64_t cns, int map_type, erd_stream_t stream) {
    ERD_REQUIRE(fine && coarse && C % 4 == 0 && fns % 4 == 0 && cns % 4 == 0 && ERD_MAP_OK(map_type), "upsample_add: bad args");
    const int64_t total = (int64_t)N * H * W * (C / 4);
    ERD_MAP(map_type, hipLaunchKernelGGL(upsample_add_kernel<T>, dim3(grid_for(total, 4096)), dim3(256), 0, (hipStream_t)stream,
                                         (T*)fine, (const T*)coarse, N, H, W, C / 4, h, w, fns, cns));
    return erd::check_launch("upsample_add");
}

extern "C" int erd_upsample2x_add_bwd(const void* dfine, void* dcoarse, int N, int H, int W, int C, int h, int w,
                                      int64_t fns, int64_t cns, int map_type, erd_stream_t stream) {
    ERD_REQUIRE(dfine && dcoarse && C % 4 == 0 && fns % 4 == 0 && cns % 4 == 0 && ERD_MAP_OK(map_type), "upsample_add_bwd: bad args");
    const int64_t total = (int64_t)N * h * w * (C / 4);
    ERD_MAP(map_type, hipLaunchKernelGGL(upsample_add_bwd_kernel<T>, dim3(grid_for(total, 4096)), dim3(256), 0, (hipStream_t)stream,
                                         (const T*)dfine, (T*)dcoarse, N, H, W, C / 4, h, w, fns, cns));
    return erd::check_launch("upsample_add_bwd");
}

extern "C" int erd_colsum(const void* x, int64_t rows, int C, float* out, int accumulate, int map_type, erd_stream_t stream) {
    ERD_REQUIRE(x && out && C > 0 && ERD_MAP_OK(map_type), "colsum: bad args");
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) ERD_ZERO_ASYNC(out, sizeof(float) * C, st);
    if (rows == 0) return 0;
    if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & (map_type == ERD_BF16 ? 7 : 15)) == 0) {
        const int C4 = C / 4, cw4 = C4 < 64 ? C4 : 64, gy = (C4 + cw4 - 1) / cw4, lanes = 256 / cw4;
        const int ranges = COLSUM_WGS / gy > 0 ? COLSUM_WGS / gy : 1;
        const int64_t unit = 4 * lanes;                                 // rows one pass of the unrolled loop covers
        const int64_t rpb = ((rows + ranges - 1) / ranges + unit - 1) / unit * unit;
        ERD_MAP(map_type, hipLaunchKernelGGL(colsum_vec_kernel<T>, dim3((unsigned)((rows + rpb - 1) / rpb), gy), dim3(256), 0, st,
                                             (const T*)x, rows, C4, out, rpb, cw4));
        return erd::check_launch("colsum");
    }
    int rpb = 64;
    while ((rows + rpb - 1) / rpb > 2048) rpb *= 2;
    ERD_MAP(map_type, hipLaunchKernelGGL(colsum_kernel<T>, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, st,
                                         (const T*)x, rows, C, out, rpb));
    return erd::check_launch("colsum");
}

extern "C" int erd_pad_channels(const float* src, float* dst, int64_t rows, int C, int Cp, erd_stream_t stream) {
    ERD_REQUIRE(src && dst && rows >= 0 && C > 0 && Cp >= C, "pad_channels: bad args");
    if (rows == 0) return 0;
    const int64_t blocks = std::min<int64_t>((rows * Cp + 255) / 256, 8192);
    hipLaunchKernelGGL(pad_channels_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, rows, C, Cp);
    return erd::check_launch("pad_channels");
}

extern "C" int erd_level_scale(const float* x, const float* alphas, float* y, int N, int64_t A, int C,
                               const erd_levels* lv, erd_stream_t stream) {
    ERD_REQUIRE(x && alphas && y && lv, "level_scale: null");
    const GnChunks ch = make_chunks(lv);
    hipLaunchKernelGGL(level_scale_kernel, dim3(ch.start[lv->nseg], N), dim3(256), 0, (hipStream_t)stream, x, alphas, y,
                       A, C, *lv, ch);
    return erd::check_launch("level_scale");
}

extern "C" int erd_level_scale_bwd(const float* x, const float* dy, const float* alphas, float* dx, float* dalphas,
                                   int N, int64_t A, int C, const erd_levels* lv, erd_stream_t stream) {
    ERD_REQUIRE(x && dy && alphas && dx && dalphas && lv, "level_scale_bwd: null");
    hipStream_t st = (hipStream_t)stream;
    const GnChunks ch = make_chunks(lv);
    ERD_ZERO_ASYNC(dalphas, sizeof(float) * lv->nseg, st);
    if (C % 4 == 0 && aligned16(x, dy) && aligned16(dx, dx))
        hipLaunchKernelGGL(level_scale_bwd_kernel<true>, dim3(ch.start[lv->nseg], N), dim3(256), 0, st, x, dy, alphas, dx,
                           dalphas, A, C, *lv, ch);
    else
        hipLaunchKernelGGL(level_scale_bwd_kernel<false>, dim3(ch.start[lv->nseg], N), dim3(256), 0, st, x, dy, alphas, dx,
                           dalphas, A, C, *lv, ch);
    return erd::check_launch("level_scale_bwd");
}

extern "C" int erd_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float momentum,
                                float weight_decay, float grad_scale, int first_step, erd_stream_t stream) {
    ERD_REQUIRE(p && g && buf && n % 4 == 0, "sgd: bad args (n must be a multiple of 4)");
    if (n == 0) return 0;
    hipLaunchKernelGGL(sgd_kernel<false>, dim3(grid_for(n / 4, 4096)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(buf), n / 4,
                       (int64_t)0, (const erd_sgd_seg*)nullptr, 0, lr, momentum, weight_decay, grad_scale, (const float*)nullptr,
                       first_step);
    return erd::check_launch("sgd");
}

// torch.optim.SGD with parameter groups (the reference builds them through mmengine's OptimWrapper / paramwise_cfg): validates a
// host segment table and writes its device form, nseg + 1 entries (the last one is the end of the buffers)
extern "C" int erd_sgd_groups_table(const int64_t* seg_off, const float* lr_mult, const float* weight_decay, int nseg,
                                    erd_sgd_seg* table_dev, erd_stream_t stream) {
    ERD_REQUIRE(seg_off && lr_mult && weight_decay && table_dev && nseg >= 1, "sgd_groups_table: bad args");
    std::vector<erd_sgd_seg> host((size_t)nseg + 1);
    for (int s = 0; s <= nseg; ++s) {
        ERD_REQUIRE(seg_off[s] >= 0 && seg_off[s] % 4 == 0, "sgd_groups_table: segment %d starts at element %lld, not a multiple of 4 "
                    "floats (a float4 would straddle two segments)", s, (long long)seg_off[s]);
        ERD_REQUIRE(s == 0 || seg_off[s] > seg_off[s - 1], "sgd_groups_table: offsets must increase (segment %d)", s);
        host[s].begin = seg_off[s];
        host[s].lr_mult = s < nseg ? lr_mult[s] : 0.f;
        host[s].weight_decay = s < nseg ? weight_decay[s] : 0.f;
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(table_dev, host.data(), host.size() * sizeof(erd_sgd_seg), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);        // (`host` dies with this call; tables are built once per trainer)
    if (e != hipSuccess) {
        erd::set_error("sgd_groups_table: %s", hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// torch.optim.SGD with parameter groups over [base, base + n) of the flat buffers (p, g, buf point AT element `base`): segments
// [seg0, seg0 + nseg) of the device table cover the range.  clip_coef: optional device float that multiplies grad_scale
// (torch.nn.utils.clip_grad_norm_'s coefficient, erd_clip_coef)
extern "C" int erd_sgd_momentum_groups(float* p, const float* g, float* buf, int64_t base, int64_t n, const erd_sgd_seg* table_dev,
                                       int seg0, int nseg, int64_t seg0_begin, int64_t seg_end, float lr, float momentum,
                                       float grad_scale, const float* clip_coef, int first_step, erd_stream_t stream) {
    ERD_REQUIRE(p && g && buf && table_dev && n % 4 == 0 && base % 4 == 0 && n >= 0, "sgd_groups: bad args (base and n must be "
                "multiples of 4)");
    ERD_REQUIRE(seg0 >= 0 && nseg >= 1 && seg0_begin <= base && base + n <= seg_end, "sgd_groups: segments [%lld, %lld) do not cover "
                "the range [%lld, %lld)", (long long)seg0_begin, (long long)seg_end, (long long)base, (long long)(base + n));
    if (n == 0) return 0;
    hipLaunchKernelGGL(sgd_kernel<true>, dim3(grid_for(n / 4, 4096)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(buf), n / 4, base,
                       table_dev + seg0, nseg, lr, momentum, 0.f, grad_scale, clip_coef, first_step);
    return erd::check_launch("sgd_groups");
}

// torch.optim.AdamW / torch.optim.Adam (amsgrad=False, maximize=False) over [base, base + n) of the flat buffers, one launch: the
// arguments of erd_sgd_momentum_groups with two moment buffers.  table_dev null: lr and weight_decay for every element (seg0, nseg,
// seg0_begin, seg_end are not read); otherwise lr * lr_mult[s] and weight_decay[s] of the table (weight_decay is not read)
extern "C" int erd_adam_groups(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t base, int64_t n,
                               const erd_sgd_seg* table_dev, int seg0, int nseg, int64_t seg0_begin, int64_t seg_end, float lr,
                               float weight_decay, double beta1, double beta2, float eps, float inv_bias1, float inv_sqrt_bias2,
                               float grad_scale, const float* clip_coef, int decoupled, erd_stream_t stream) {
    ERD_REQUIRE(((p && g && exp_avg && exp_avg_sq) || n == 0) && n % 4 == 0 && base % 4 == 0 && n >= 0 && base >= 0, "adam_groups: "
                "bad args (base and n must be multiples of 4)");
    ERD_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f, "adam_groups: betas (%g, %g) must lie in "
                "[0, 1) and eps %g must not be negative", beta1, beta2, (double)eps);
    ERD_REQUIRE(!table_dev || (seg0 >= 0 && nseg >= 1 && seg0_begin <= base && base + n <= seg_end), "adam_groups: segments [%lld, "
                "%lld) do not cover the range [%lld, %lld)", (long long)seg0_begin, (long long)seg_end, (long long)base,
                (long long)(base + n));
    if (n == 0) return 0;
    hipLaunchKernelGGL(adam_groups_kernel, dim3(grid_for(n / 4, 4096)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(exp_avg),
                       reinterpret_cast<float4*>(exp_avg_sq), n / 4, base, table_dev ? table_dev + seg0 : nullptr, nseg, lr,
                       weight_decay, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, inv_bias1, inv_sqrt_bias2,
                       grad_scale, clip_coef, decoupled);
    return erd::check_launch("adam_groups");
}

// torch.nn.utils.clip_grad_norm_ (norm_type 2; the reference: OptimWrapper clip_grad), first half: the sum of squares of g[0, n) as
// ERD_SQNORM_PARTS fp64 partials in the caller's slot (every entry of the slot is written)
extern "C" int erd_grad_sqnorm(const float* g, int64_t n, double* partials, erd_stream_t stream) {
    ERD_REQUIRE((g || n == 0) && partials && n >= 0 && n % 4 == 0, "grad_sqnorm: bad args (n must be a multiple of 4)");
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(ERD_SQNORM_PARTS), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(g), n / 4, partials);
    return erd::check_launch("grad_sqnorm");
}

// ... second half: folds nslots slots in a fixed order, out[0] = total_norm = grad_scale * sqrt(sum) (the norm of the MEAN gradient),
// out[1] = min(1, max_norm / (total_norm + 1e-6)); both stay on the device
extern "C" int erd_clip_coef(const double* partials, int nslots, float grad_scale, float max_norm, float* out, erd_stream_t stream) {
    ERD_REQUIRE(partials && out && nslots >= 1 && max_norm > 0.f, "clip_coef: bad args");
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (int64_t)nslots * ERD_SQNORM_PARTS,
                       grad_scale, max_norm, out);
    return erd::check_launch("clip_coef");
}

// OptimWrapper accumulative_counts: acc = g (first micro-step of a window) or acc += g, plain fp32 adds
extern "C" int erd_grad_accumulate(float* acc, const float* g, int64_t n, int first, erd_stream_t stream) {
    ERD_REQUIRE(acc && g && n >= 0 && n % 4 == 0, "grad_accumulate: bad args (n must be a multiple of 4)");
    if (n == 0) return 0;
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(grid_for(n / 4, 4096)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(acc), reinterpret_cast<const float4*>(g), n / 4, first);
    return erd::check_launch("grad_accumulate");
}

// mmengine's EMAHook / ExponentialMovingAverage (mmdet ExpMomentumEMA: the coefficient is the host's) over [0, n) of two flat
// buffers, one launch: ema = p (copy != 0) or ema = fmaf(p, c, ema * one_minus_c).  ema and p point AT the range's start,
// 16-byte aligned; n is any count (a scalar tail behind the float4 lanes)
extern "C" int erd_ema_update(float* ema, const float* p, int64_t n, float c, float one_minus_c, int copy, erd_stream_t stream) {
    ERD_REQUIRE(n >= 0 && ((ema && p) || n == 0), "ema_update: bad args (null buffer or n = %lld < 0)", (long long)n);
    if (n == 0) return 0;
    ERD_REQUIRE(aligned16(ema, p) && disjoint(ema, p, n), "ema_update: the ranges must start on 16-byte boundaries and not overlap");
    const dim3 grid(stream_grid(n >> 2));
    if (copy) hipLaunchKernelGGL(ema_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, ema, p, n, c, one_minus_c);
    else hipLaunchKernelGGL(ema_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, ema, p, n, c, one_minus_c);
    return erd::check_launch("ema_update");
}

// a[0, n) <-> b[0, n) in one launch (parameters <-> their average around a validation pass: no third buffer of the flat size)
extern "C" int erd_swap_f32(float* a, float* b, int64_t n, erd_stream_t stream) {
    ERD_REQUIRE(n >= 0 && ((a && b) || n == 0), "swap_f32: bad args (null buffer or n = %lld < 0)", (long long)n);
    if (n == 0) return 0;
    ERD_REQUIRE(aligned16(a, b) && disjoint(a, b, n), "swap_f32: the ranges must start on 16-byte boundaries and not overlap");
    hipLaunchKernelGGL(swap_kernel, dim3(stream_grid(n >> 2)), dim3(256), 0, (hipStream_t)stream, a, b, n);
    return erd::check_launch("swap_f32");
}
