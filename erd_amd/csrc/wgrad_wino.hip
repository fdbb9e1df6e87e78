// Weight gradient of a 3x3 / stride 1 / pad 1 convolution in the Winograd domain, F(3x3, 2x2), three-limb form ("f32x3").
//
// Per 2x2 tile of the gradient map and channel pair:   V = Bt x Bt^T   (x: the 4x4 input patch around the tile, the forward kernel's input
// transform),   M = G dz G^T   (dz: the 2x2 tile, playing the filter),   dU[xi] += M[xi] * V[xi]   for the 16 positions xi, summed over all
// tiles of all maps;  dW (3x3) = At dU At^T  once, in the reduce kernel.  16 multiplications per tile where the direct form
// (conv_wgrad_row3_x3_kernel) counts 36.
//     Bt = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,-1,0,1]]      G = [[1,0],[.5,.5],[.5,-.5],[0,1]]      At = [[1,1,1,0],[0,1,-1,0],[0,1,1,1]]
// Both GEMM dimensions are channels and the contraction runs over tiles: every transformed and limb-split operand value feeds 128 MFMA
// columns.  The transforms add and halve only; products are the six limb products of the direct kernel in its order.
//
//   * A workgroup of 512 threads owns (transform row r of 4, 128 output channels, 128 input channels) of one split of the tile axis.
//     Wave w multiplies position 4 r + (w & 3) for output-channel half w >> 2: 2 x 4 accumulator blocks of 32 x 32.
//   * A K-step is 16 consecutive tiles of the concatenated tile axis (segments, images, tile rows follow each other without gaps; the last
//     tile row / column of an odd map is half outside, and out-of-map entries are loaded from past the buffer extent: exact zeros).
//   * Staging: a thread owns 2 channels x 2 tiles of BOTH operands.  It loads the two patch rows transform row r needs (x: 2 x 4 entries per
//     tile) and the tile's rows (dz: 2 entries per row; one row for r = 0 and r = 3) as 8-byte pieces, runs the row pass and the column pass,
//     splits the four positions' values of its tile pair into limbs and stores one dword per (position, limb, channel) into
//     [position][limb][operand][128 channel rows][16 tiles] bf16 rows of 32 B -- the dz planes of the direct kernel with "pixel" read as "tile":
//     channel 2 cg + c lives in row cg + 64 c, the 16-byte half of a row is swizzled by (row >> 3) & 1 (a store instruction of a wave -- 16
//     channel pairs x 4 tile pairs -- then touches all 64 banks once), and a lane's MFMA fragment is one 16-byte read.
//     16 consecutive lanes load 16 consecutive channel pairs, one 128-byte line of a pixel.  (First form: 8 lanes per pixel, neighbouring
//     lanes on different pixels -- every lane its own line request: 586 us on the head towers' launch against 380, EXPERIMENTS 7q.)
//   * One operand buffer (98 KB; two do not fit), run in phases: the raw loads of step g + 1 are issued, the MFMAs of step g run on the
//     buffer, a barrier, the transform of step g + 1 is written, a barrier.
//   * The row permutation makes accumulator blocks j and j + 2 of a lane two CONSECUTIVE input channels: the partial slab
//     part[split][position][Cout][Cin] is written straight from the accumulators as 8-byte pieces, 256 contiguous bytes per half wave.
//   * Where Cin and Cout are multiples of 256 the launch takes wgrad_wino_pos_kernel below instead: one position and 256 x 256 channels per
//     workgroup, half the vector work per MFMA, the same slabs bit for bit.
#include <stdlib.h>
#include "erd_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));

constexpr int WT = 512;                          // threads of a workgroup
constexpr int KT = 16;                           // tiles per K-step
constexpr int BC = 128;                          // channels per workgroup, either side
constexpr int ROWB = 2 * KT;                     // bytes of an LDS row: 16 tiles of one channel, one limb, one position
constexpr int PLANE = BC * ROWB;                 // one operand's rows
constexpr int LIMB = 2 * PLANE;                  // dz rows, then x rows
constexpr int POS = 3 * LIMB;                    // the three limbs of a position
constexpr int OPER_BYTES = 4 * POS;              // the four positions of a transform row: 98 304
constexpr int TAB_U = 8, NSLOT = 4;              // table: words per tile, ring slots of 16 tiles
constexpr size_t LDS_BYTES = OPER_BYTES + NSLOT * KT * TAB_U * sizeof(unsigned);
constexpr unsigned INV = 0x80000000u;            // byte offset of an entry that does not exist: past the extent of any buffer (< 2^31 bytes)

__device__ __forceinline__ float2 buf_load8(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    const u2v v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0);
    return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
}
__device__ __forceinline__ float2 buf_load8(__amdgpu_buffer_rsrc_t r, unsigned byte_off, unsigned uniform_off) {
    const u2v v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, uniform_off, 0);
    return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
}
__device__ __forceinline__ float comp(const float2& v, int c) { return c == 0 ? v.x : v.y; }

struct WinoMap { int xb, zb, IH, IW, OH, OW; };      // image n of a segment: element offsets of its x / dz maps, their sizes

__device__ __forceinline__ int tiles_w(const erd_wgrad_seg& g) { return (g.GW + 1) >> 1; }
__device__ __forceinline__ int tiles_h(const erd_wgrad_seg& g) { return (g.GH + 1) >> 1; }

// Transform row r: patch rows (A, B) with T = A + sx B -- (0,2,-) (1,2,+) (2,1,-) (3,1,-) --, dz rows R = cz (A + sz B) -- r = 0: row 0,
// r = 3: row 1 (B is never loaded and stays zero), r = 1, 2: half the sum / difference of rows 0 and 1.  The COLUMN pass of the
// position kernel selects patch and tile columns by the same table.
struct Sel {
    int xa, xb, za;
    float sx, sz, cz;
    bool z_two;
    __device__ __forceinline__ explicit Sel(int r)
        : xa(r), xb(r < 2 ? 2 : 1), za(r == 3 ? 1 : 0), sx(r == 1 ? 1.f : -1.f), sz(r == 2 ? -1.f : 1.f), cz(r == 1 || r == 2 ? 0.5f : 1.f),
          z_two(r == 1 || r == 2) {}
};

// Table of a K-step, by the first 16 lanes of wave 0: per tile the byte offsets of its two x rows (at patch column 0, channel 0) and its
// two dz rows (at the tile's first column), INV for a row outside the map, and the masks of the columns inside.  The position (segment
// sl, image sn, tile row sa, tile sb) of a step's first tile is wave-uniform: decoded once, then stepped by 16 on the scalar side.  A
// lane walks from there by row wraps; a lane whose tile lies past the image of the first one decodes its tile index itself.
struct TileTable {
    const erd_wgrad_desc& p;
    const Sel& rs;
    const Sel& cs;      // (the position kernel's column selectors)
    unsigned* tab;      // [NSLOT][KT][TAB_U]
    int lane, ntiles;
    int sl, sn = 0, sa = 0, sb = 0;
    __device__ __forceinline__ TileTable(const erd_wgrad_desc& p_, const Sel& rs_, const Sel& cs_, unsigned* tab_, int lane_, int ntiles_)
        : p(p_), rs(rs_), cs(cs_), tab(tab_), lane(lane_), ntiles(ntiles_), sl(p_.nseg) {}

    __device__ __forceinline__ void tile_entry(const WinoMap& m, int ty, int tx, unsigned (&ent)[5]) const {
        const int ra = 2 * ty - 1 + rs.xa, rb = 2 * ty - 1 + rs.xb, c0 = 2 * tx - 1;
        if ((unsigned)ra < (unsigned)m.IH) ent[0] = (unsigned)(m.xb + (ra * m.IW + c0) * p.Cin) * 4u;
        if ((unsigned)rb < (unsigned)m.IH) ent[1] = (unsigned)(m.xb + (rb * m.IW + c0) * p.Cin) * 4u;
        const int qa = 2 * ty + rs.za, qb = 2 * ty + 1;
        if (qa < m.OH) ent[2] = (unsigned)(m.zb + (qa * m.OW + 2 * tx) * p.Cout) * 4u;
        if (rs.z_two && qb < m.OH) ent[3] = (unsigned)(m.zb + (qb * m.OW + 2 * tx) * p.Cout) * 4u;
        unsigned mask = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) mask |= (unsigned)(c0 + b) < (unsigned)m.IW ? 1u << b : 0u;
        mask |= (2 * tx < m.OW ? 16u : 0u) | (2 * tx + 1 < m.OW ? 32u : 0u);
        ent[4] = mask;
    }
    // The position kernel's entry: rows AND columns are the workgroup's, so the table holds the byte offset of every entry a thread loads
    // (at channel 0) -- x [row A, B][column a, b], dz [row A, B][column a, b] -- or INV: a load costs its thread one addition.
    __device__ __forceinline__ void tile_entry_pos(const WinoMap& m, int ty, int tx, unsigned (&ent)[8]) const {
        const int ra = 2 * ty - 1 + rs.xa, rb = 2 * ty - 1 + rs.xb, ca = 2 * tx - 1 + cs.xa, cb = 2 * tx - 1 + cs.xb;
        const bool ra_in = (unsigned)ra < (unsigned)m.IH, rb_in = (unsigned)rb < (unsigned)m.IH;
        const bool ca_in = (unsigned)ca < (unsigned)m.IW, cb_in = (unsigned)cb < (unsigned)m.IW;
        if (ra_in && ca_in) ent[0] = (unsigned)(m.xb + (ra * m.IW + ca) * p.Cin) * 4u;
        if (ra_in && cb_in) ent[1] = (unsigned)(m.xb + (ra * m.IW + cb) * p.Cin) * 4u;
        if (rb_in && ca_in) ent[2] = (unsigned)(m.xb + (rb * m.IW + ca) * p.Cin) * 4u;
        if (rb_in && cb_in) ent[3] = (unsigned)(m.xb + (rb * m.IW + cb) * p.Cin) * 4u;
        const int qa = 2 * ty + rs.za, qb = 2 * ty + 1, ka = 2 * tx + cs.za, kb = 2 * tx + 1;
        const bool qb_in = rs.z_two && qb < m.OH, kb_in = cs.z_two && kb < m.OW;
        if (qa < m.OH && ka < m.OW) ent[4] = (unsigned)(m.zb + (qa * m.OW + ka) * p.Cout) * 4u;
        if (qa < m.OH && kb_in) ent[5] = (unsigned)(m.zb + (qa * m.OW + kb) * p.Cout) * 4u;
        if (qb_in && ka < m.OW) ent[6] = (unsigned)(m.zb + (qb * m.OW + ka) * p.Cout) * 4u;
        if (qb_in && kb_in) ent[7] = (unsigned)(m.zb + (qb * m.OW + kb) * p.Cout) * 4u;
    }
    static __device__ __forceinline__ WinoMap map_of(const erd_wgrad_seg& g, int n) {
        return WinoMap{(int)(g.x_off + n * g.x_nstride), (int)(g.dz_off + n * g.dz_nstride), g.IH, g.IW, g.OH, g.OW};
    }
    __device__ __forceinline__ void locate(int u, int& l, int& n, int& a, int& b) const {      // tile u < ntiles of the concatenated axis (the only divisions)
        l = 0;
#pragma unroll 1
        for (; l < p.nseg - 1; ++l) {
            const int cnt = p.seg[l].N * tiles_h(p.seg[l]) * tiles_w(p.seg[l]);
            if (u < cnt) break;
            u -= cnt;
        }
        const int TW = tiles_w(p.seg[l]), THW = tiles_h(p.seg[l]) * TW;
        n = u / THW;
        const int rem = u - n * THW;
        a = rem / TW;
        b = rem - a * TW;
    }
    __device__ __forceinline__ void start(int g) {      // the walker at the first tile of step g
        if (g * KT < ntiles) locate(g * KT, sl, sn, sa, sb);
    }
    // SPAN tiles from the first tile of step g on, which is at the walker's position, into the slots from `slot` on; then the walker moves on
    template <bool POS, int SPAN = KT>
    __device__ __forceinline__ void build(int g, int slot) {
        sl = __builtin_amdgcn_readfirstlane(sl);
        sn = __builtin_amdgcn_readfirstlane(sn);
        sa = __builtin_amdgcn_readfirstlane(sa);
        sb = __builtin_amdgcn_readfirstlane(sb);
        if (lane < SPAN) {
            unsigned ent[8] = {INV, INV, INV, INV, POS ? INV : 0u, INV, INV, INV};
            auto entry = [&](const WinoMap& m, int a, int b) {
                if constexpr (POS) tile_entry_pos(m, a, b, ent);
                else tile_entry(m, a, b, reinterpret_cast<unsigned (&)[5]>(ent));
            };
            if (sl < p.nseg) {
                const erd_wgrad_seg& sg = p.seg[sl];
                const int TW = tiles_w(sg);
                int a = sa, b = sb + lane;
                while (b >= TW) { b -= TW; ++a; }
                if (a < tiles_h(sg)) entry(map_of(sg, sn), a, b);
                else if (g * KT + lane < ntiles) {
                    int l, n;
                    locate(g * KT + lane, l, n, a, b);
                    entry(map_of(p.seg[l], n), a, b);
                }
            }
            unsigned* e = tab + (slot * KT + lane) * TAB_U;
            *reinterpret_cast<u4v*>(e) = u4v{ent[0], ent[1], ent[2], ent[3]};
            if constexpr (POS) *reinterpret_cast<u4v*>(e + 4) = u4v{ent[4], ent[5], ent[6], ent[7]};
            else e[4] = ent[4];
        }
        sb += SPAN;
        while (sl < p.nseg && sb >= tiles_w(p.seg[sl])) {      // one tile row on; a row is never split between images or segments
            sb -= tiles_w(p.seg[sl]);
            const bool img = sa + 1 == tiles_h(p.seg[sl]);
            sa = img ? 0 : sa + 1;
            const bool seg = img && sn + 1 == p.seg[sl].N;
            sn = seg ? 0 : sn + (img ? 1 : 0);
            sl += seg ? 1 : 0;
        }
    }
};

__global__ __launch_bounds__(WT) void conv_wgrad_wino_kernel(const erd_wgrad_desc p, const int ntiles, const int nsteps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* tab = reinterpret_cast<unsigned*>(smem + OPER_BYTES);      // [NSLOT][KT][TAB_U]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);

    // ---- work: the grid lists, fastest first, the transform rows, the ci tiles, the co tiles and the splits; in XCD-contiguous order the
    // workgroups of one split (which read the same maps at the same time) share an L2
    const int nci = p.Cin / BC, nco = p.Cout / BC, ncomb = 4 * nci * nco;
    const int wg = erd::xcd_contiguous(blockIdx.x, gridDim.x);
    const int split = wg / ncomb, comb = wg - split * ncomb;
    const int r = comb & 3, ct = comb >> 2;
    const int ci0 = (ct % nci) * BC, co0 = (ct / nci) * BC;
    const int per = (nsteps + p.nsplit - 1) / p.nsplit;
    const int g_begin = split * per, g_end = min(nsteps, g_begin + per);

    const Sel rs(r);
    const float sx = rs.sx, sz = rs.sz, cz = rs.cz;
    const bool z_two = rs.z_two;
    TileTable tt{p, rs, rs, tab, lane, ntiles};

    // ---- staging: every thread owns 2 channels x 2 tiles of BOTH operands
    // (16 consecutive lanes read 16 consecutive channel pairs, one 128-byte line of a pixel: the texture unit merges neighbouring lanes only)
    const int cg = (wave & 3) * 16 + (lane & 15), tp = (wave >> 2) * 4 + (lane >> 4);      // channel pair, tile pair
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)(p.x_elems * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dz), 0, (int)(p.dz_elems * 4), 0x00020000);
    const unsigned chan_x = (unsigned)(ci0 + 2 * cg) * 4u, chan_z = (unsigned)(co0 + 2 * cg) * 4u;
    const unsigned step_x = (unsigned)p.Cin * 4u, step_z = (unsigned)p.Cout * 4u;      // bytes from a pixel to the next one of its row
    float2 rx[16], rz[8];      // [tile of the pair][row A, B][patch column 0..3 | tile column 0..1]
#pragma unroll
    for (int i = 0; i < 8; ++i) rz[i] = make_float2(0.f, 0.f);
    auto load_global = [&](int slot) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const unsigned* e = tab + (slot * KT + 2 * tp + q) * TAB_U;
            const u4v o = *reinterpret_cast<const u4v*>(e);
            const unsigned mask = e[4];
#pragma unroll
            for (int w = 0; w < 2; ++w)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const bool ok = o[w] != INV && ((mask >> b) & 1u);
                    rx[q * 8 + w * 4 + b] = buf_load8(rs_x, ok ? o[w] + (unsigned)b * step_x + chan_x : INV);
                }
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                if (w == 1 && !z_two) continue;      // (uniform over the workgroup: the registers keep their zeros)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const bool ok = o[2 + w] != INV && ((mask >> (4 + b)) & 1u);
                    rz[q * 4 + w * 2 + b] = buf_load8(rs_z, ok ? o[2 + w] + (unsigned)b * step_z + chan_z : INV);
                }
            }
        }
    };
    // the thread's dwords: rows cg and cg + 64 of an operand's plane, tile pair tp of the row (16-byte halves swizzled by (row >> 3) & 1 = (cg >> 3) & 1)
    char* const st_base = smem + cg * ROWB + ((((tp >> 2) ^ (cg >> 3)) & 1) << 4) + ((tp & 3) << 2);
    auto store_limbs = [&](char* dst, const float (&v)[2][4]) {      // the four positions of a tile pair, one channel
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned hi, mid, lo;
            erd::limbs3_pair(v[0][j], v[1][j], hi, mid, lo);
            *reinterpret_cast<unsigned*>(dst + j * POS) = hi;
            *reinterpret_cast<unsigned*>(dst + j * POS + LIMB) = mid;
            *reinterpret_cast<unsigned*>(dst + j * POS + 2 * LIMB) = lo;
        }
    };
    auto store_lds = [&]() {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float v[2][4];      // [tile][position of the transform row]
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float t[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) t[b] = __builtin_fmaf(sx, comp(rx[q * 8 + 4 + b], c), comp(rx[q * 8 + b], c));
                v[q][0] = t[0] - t[2];
                v[q][1] = t[1] + t[2];
                v[q][2] = t[2] - t[1];
                v[q][3] = t[3] - t[1];
            }
            store_limbs(st_base + PLANE + c * (64 * ROWB), v);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float t[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) t[b] = cz * __builtin_fmaf(sz, comp(rz[q * 4 + 2 + b], c), comp(rz[q * 4 + b], c));
                v[q][0] = t[0];
                v[q][1] = 0.5f * (t[0] + t[1]);
                v[q][2] = 0.5f * (t[0] - t[1]);
                v[q][3] = t[1];
            }
            store_limbs(st_base + c * (64 * ROWB), v);
        }
    };

    // ---- MFMA roles
    const int pj = wave & 3, half = wave >> 2;
    const int li = lane & 31, h = lane >> 5;
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if (g_begin < g_end) {
        if (wave_u == 0) {
            tt.start(g_begin);
            tt.build<false>(g_begin, 0);
            tt.build<false>(g_begin + 1, 1);
        }
        __syncthreads();
        load_global(0);
        store_lds();
        __syncthreads();
        // fragment addresses: dz rows (half * 2 + i) * 32 + li, x rows j * 32 + li, the 16-byte half h (tiles 8 h .. 8 h + 7)
        const char* const fr = smem + pj * POS + li * ROWB + (((h ^ (li >> 3)) & 1) << 4);
        for (int g = g_begin; g < g_end; ++g) {
            const int k = g - g_begin;
            const bool more = g + 1 < g_end;
#ifndef ERD_WW_NOLOAD
            if (more) load_global((k + 1) & (NSLOT - 1));
#endif
#ifndef ERD_WW_NOTABLE
            if (wave_u == 0 && g + 2 < g_end) tt.build<false>(g + 2, (k + 2) & (NSLOT - 1));
#endif
#ifndef ERD_WW_NOMFMA
            u4v fa[2][3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i][pl] = *reinterpret_cast<const u4v*>(fr + pl * LIMB + (half * 2 + i) * (32 * ROWB));
#pragma unroll
            for (int jh = 0; jh < 2; ++jh) {      // (two column blocks at a time: their x fragments are 24 registers)
                u4v fb[2][3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                    for (int j = 0; j < 2; ++j) fb[j][pl] = *reinterpret_cast<const u4v*>(fr + pl * LIMB + PLANE + (jh * 2 + j) * (32 * ROWB));
#define ERD_W3(APL, BPL)                                                                                                                     \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) _Pragma("unroll") for (int i = 0; i < 2; ++i) acc[i][jh * 2 + j] =                         \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i][APL]), __builtin_bit_cast(bf16x8, fb[j][BPL]), acc[i][jh * 2 + j], 0, 0, 0);
                ERD_W3(0, 2) ERD_W3(0, 1) ERD_W3(1, 1) ERD_W3(2, 0) ERD_W3(1, 0) ERD_W3(0, 0)
#undef ERD_W3
            }
#endif
            __syncthreads();      // every wave has read its fragments of step g
#ifndef ERD_WW_NOSPLIT
            if (more) store_lds();
#endif
            __syncthreads();
        }
    }

    // ---- partial slab [split][position][Cout][Cin]: row R of a plane is channel 2 (R % 64) + R / 64, so block (i, j), register e, lane (li, h)
    // holds output channel co0 + 2 (32 i + (e & 3) + 8 (e >> 2) + 4 h) + half and input channel ci0 + 64 (j & 1) + 2 li + (j >> 1)
    float* __restrict__ part = p.part + ((int64_t)(split * 16 + 4 * r + pj) * p.Cout) * p.Cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = co0 + 2 * (32 * i + (e & 3) + 8 * (e >> 2) + 4 * h) + half;
            float* row = part + (int64_t)co * p.Cin + ci0 + 2 * li;
            *reinterpret_cast<float2*>(row) = make_float2(acc[i][0][e], acc[i][2][e]);
            *reinterpret_cast<float2*>(row + 64) = make_float2(acc[i][1][e], acc[i][3][e]);
        }
}

// ---- one position per workgroup ------------------------------------------------------------------------------------------------------------
// The same product with another ownership: a workgroup of 512 threads owns (position xi = 4 r + c of 16, 256 output channels, 256 input
// channels) of one split.  The accumulators (half the register file) allow positions x couts x cins = 65 536 either way; the values to
// transform and limb-split per K-step go as positions x (couts + cins): 4 x 256 above, 1 x 512 here, for the same 384 MFMAs -- half the
// vector work per MFMA.  What is the same: walker, K-step of 16 tiles, the three limbs and six products in their order, the slab layout,
// the reduce kernel.  Every accumulator sums the same products in the same order as above: the slabs are bit-equal on any data.
//   * Wave w multiplies output-channel quarter w >> 1 (2 row blocks of 32) with input-channel half w & 1 (4 column blocks): 2 x 4 accumulator
//     blocks, 6 + 12 fragment reads per K-step.  The x fragments are read one column block at a time: 12 registers live instead of 24.
//   * Staging: a thread owns 2 channels x 4 tiles of BOTH operands.  Row AND column selectors are workgroup-uniform, so the table holds
//     the offset of every entry a thread loads (TileTable::tile_entry_pos): per tile the 2 x 2 patch entries the position needs (x: 16
//     eight-byte loads, one addition each) and 1, 2 or 4 entries of the tile (dz: 4 .. 16 loads).  The thread forms T = A + s B per needed
//     column and the ONE column combination of the position (the operations of the column pass above, value for value), splits 8 + 8
//     values and stores one 8-byte piece per (limb, operand, channel): 12 LDS stores where the row form has 48.
//   * [limb][operand][256 channel rows][16 tiles] bf16 rows of 32 B, 48 KB: channel 2 cg + c lives in row cg + 128 c, halves swizzled by
//     (row >> 3) & 1 as above.  TWO such buffers, 64 KB apart (a thread changes buffers by one XOR on its offsets): the transform of step
//     g + 1 is written into the buffer the MFMAs of step g do not read, so a K-step has ONE barrier and no wave waits between its MFMAs
//     and its vector work -- the two waves of a SIMD drift apart and one's transform runs beside the other's MFMAs (head launch: 388 us
//     with one buffer and two barriers, 375 with two buffers, profiles/r12_wgrad_wino_pos.txt).
//   * The table is built for FOUR K-steps at a time, by the 64 lanes of wave 0 every fourth step (ring of 8 step slots, between the
//     buffers).  Its chain of dependent scalar loads of the segment geometry lies on the workgroup's critical path -- the other waves
//     wait for wave 0 at the barrier: 38 us of the head launch when built per step (timing probe ERD_WW_NOTABLE), 10 us per four steps.
constexpr int BP = 256;                          // channels per workgroup, either side
constexpr int PPLANE = BP * ROWB;                // one operand's rows
constexpr int PLIMB = 2 * PPLANE;                // dz rows, then x rows
constexpr int POPER_BYTES = 3 * PLIMB;           // the three limbs of the position: 49 152
constexpr unsigned PBUF_XOR = 65536;              // the second buffer's offset: a thread's addresses change buffers by one XOR
constexpr int PSPAN = 4 * KT, PNSLOT = 8;        // table: built for four K-steps at a time by the 64 lanes of wave 0, ring slots of 16 tiles
constexpr size_t PTAB_BYTES = PNSLOT * KT * TAB_U * sizeof(unsigned);      // (behind the first buffer)
constexpr size_t PLDS_BYTES = PBUF_XOR + POPER_BYTES;
static_assert(POPER_BYTES + PTAB_BYTES <= PBUF_XOR, "the table lies between the buffers");

__global__ __launch_bounds__(WT) void wgrad_wino_pos_kernel(const erd_wgrad_desc p, const int ntiles, const int nsteps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* tab = reinterpret_cast<unsigned*>(smem + POPER_BYTES);      // [PNSLOT][KT][TAB_U]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);

    // ---- work: the grid lists, fastest first, the positions, the ci tiles, the co tiles and the splits (XCD-contiguous, as above)
    const int nci = p.Cin / BP, nco = p.Cout / BP, ncomb = 16 * nci * nco;
    const int wg = erd::xcd_contiguous(blockIdx.x, gridDim.x);
    const int split = wg / ncomb, comb = wg - split * ncomb;
    const int xi = comb & 15, ct = comb >> 4;
    const int ci0 = (ct % nci) * BP, co0 = (ct / nci) * BP;
    const int per = (nsteps + p.nsplit - 1) / p.nsplit;
    const int g_begin = split * per, g_end = min(nsteps, g_begin + per);

    // rows by r, columns by c: x column pass t[ca] + sxc t[cb] -- (0,2,-) (1,2,+) (2,1,-) (3,1,-): a product with +-1 is exact, so the
    // fma is the subtraction / addition of the row form bit for bit --, dz column pass t[za], or half the sum / difference of both columns
    const Sel rs(xi >> 2), cs(xi & 3);
    const float sx = rs.sx, sz = rs.sz, cz = rs.cz;
    const bool z_two = rs.z_two, zc_two = cs.z_two;
    const float sxc = cs.sx, szc = cs.sz;
    TileTable tt{p, rs, cs, tab, lane, ntiles};

    // ---- staging: every thread owns 2 channels x 4 tiles of BOTH operands (16 consecutive lanes: one 128-byte line of a pixel)
    const int cg = wave * 16 + (lane & 15), tq = lane >> 4;      // channel pair, tile quad
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, (int)(p.x_elems * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.dz), 0, (int)(p.dz_elems * 4), 0x00020000);
    const unsigned chan = (unsigned)cg * 8u, tile_x = (unsigned)ci0 * 4u, tile_z = (unsigned)co0 * 4u;      // the pair in its tile; the tile: uniform
    float2 rx[16], rz[16];      // [tile of the quad][row A, B][column a, b]
#pragma unroll
    for (int i = 0; i < 16; ++i) rz[i] = make_float2(0.f, 0.f);
    // (an entry that does not exist is INV, and INV + the channel offset is still past the extent: zeros)
    auto load_global = [&](int slot) {
        u4v ox[4], oz[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned* e = tab + (slot * KT + 4 * tq + q) * TAB_U;
            ox[q] = *reinterpret_cast<const u4v*>(e);
            oz[q] = *reinterpret_cast<const u4v*>(e + 4);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) rx[q * 4 + i] = buf_load8(rs_x, ox[q][i] + chan, tile_x);
        // (the conditions are uniform over the workgroup: each branch skips a whole group of loads, whose registers keep their zeros)
#pragma unroll
        for (int q = 0; q < 4; ++q) rz[q * 4] = buf_load8(rs_z, oz[q][0] + chan, tile_z);
        if (zc_two) {
#pragma unroll
            for (int q = 0; q < 4; ++q) rz[q * 4 + 1] = buf_load8(rs_z, oz[q][1] + chan, tile_z);
        }
        if (z_two) {
#pragma unroll
            for (int q = 0; q < 4; ++q) rz[q * 4 + 2] = buf_load8(rs_z, oz[q][2] + chan, tile_z);
            if (zc_two) {
#pragma unroll
                for (int q = 0; q < 4; ++q) rz[q * 4 + 3] = buf_load8(rs_z, oz[q][3] + chan, tile_z);
            }
        }
    };
    // the thread's 8-byte pieces: rows cg and cg + 128 of an operand's plane, tile quad tq of the row (halves swizzled by (cg >> 3) & 1)
    unsigned st_off = cg * ROWB + ((((tq >> 1) ^ (cg >> 3)) & 1) << 4) + ((tq & 1) << 3);
    auto store_limbs = [&](char* dst, const float (&v)[4]) {      // the four tiles of one channel
        unsigned hi[2], mid[2], lo[2];
        erd::limbs3_pair(v[0], v[1], hi[0], mid[0], lo[0]);
        erd::limbs3_pair(v[2], v[3], hi[1], mid[1], lo[1]);
        *reinterpret_cast<u2v*>(dst) = u2v{hi[0], hi[1]};
        *reinterpret_cast<u2v*>(dst + PLIMB) = u2v{mid[0], mid[1]};
        *reinterpret_cast<u2v*>(dst + 2 * PLIMB) = u2v{lo[0], lo[1]};
    };
    auto store_lds = [&]() {
        char* const st = smem + st_off;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float ta = __builtin_fmaf(sx, comp(rx[q * 4 + 2], c), comp(rx[q * 4], c));
                const float tb = __builtin_fmaf(sx, comp(rx[q * 4 + 3], c), comp(rx[q * 4 + 1], c));
                v[q] = __builtin_fmaf(sxc, tb, ta);
            }
            store_limbs(st + PPLANE + c * (128 * ROWB), v);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float ta = cz * __builtin_fmaf(sz, comp(rz[q * 4 + 2], c), comp(rz[q * 4], c));
                const float tb = cz * __builtin_fmaf(sz, comp(rz[q * 4 + 3], c), comp(rz[q * 4 + 1], c));
                v[q] = zc_two ? 0.5f * __builtin_fmaf(szc, tb, ta) : ta;
            }
            store_limbs(st + c * (128 * ROWB), v);
        }
    };

    // ---- MFMA roles
    const int zq = wave >> 1, hx = wave & 1;
    const int li = lane & 31, h = lane >> 5;
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if (g_begin < g_end) {
        if (wave_u == 0) {
            tt.start(g_begin);
            tt.build<true, PSPAN>(g_begin, 0);
            tt.build<true, PSPAN>(g_begin + 4, 4);
        }
        __syncthreads();
        load_global(0);
        store_lds();
        __syncthreads();
        st_off ^= PBUF_XOR;
        // fragment addresses: dz rows (zq * 2 + i) * 32 + li, x rows (2 hx + (j & 1) + 4 (j >> 1)) * 32 + li -- column blocks j and j + 2 are
        // the two channels of a pair --, the 16-byte half h (tiles 8 h .. 8 h + 7)
        unsigned fr_off = li * ROWB + (((h ^ (li >> 3)) & 1) << 4);
        for (int g = g_begin; g < g_end; ++g) {
            const int k = g - g_begin;
            const bool more = g + 1 < g_end;
            const char* const fr = smem + fr_off;
#ifndef ERD_WW_NOLOAD
            if (more) load_global((k + 1) & (PNSLOT - 1));
#endif
#ifndef ERD_WW_NOTABLE
            // (steps k + 5 .. k + 8 take the slots of steps k - 3 .. k, last read by the load_global of the iteration before)
            if (wave_u == 0 && (k & 3) == 3 && g + 5 < g_end) tt.build<true, PSPAN>(g + 5, (k + 5) & (PNSLOT - 1));
#endif
#ifndef ERD_WW_NOMFMA
            u4v fa[2][3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i][pl] = *reinterpret_cast<const u4v*>(fr + pl * PLIMB + (zq * 2 + i) * (32 * ROWB));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u4v fb[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    fb[pl] = *reinterpret_cast<const u4v*>(fr + pl * PLIMB + PPLANE + (2 * hx + (j & 1) + 4 * (j >> 1)) * (32 * ROWB));
#define ERD_W3(APL, BPL)                                                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) acc[i][j] =                                                                                \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i][APL]), __builtin_bit_cast(bf16x8, fb[BPL]), acc[i][j], 0, 0, 0);
                ERD_W3(0, 2) ERD_W3(0, 1) ERD_W3(1, 1) ERD_W3(2, 0) ERD_W3(1, 0) ERD_W3(0, 0)
#undef ERD_W3
            }
#endif
#ifndef ERD_WW_NOSPLIT
            if (more) store_lds();
#endif
            __syncthreads();
            fr_off ^= PBUF_XOR;
            st_off ^= PBUF_XOR;
        }
    }

    // ---- partial slab [split][position][Cout][Cin]: row R of a plane is channel 2 (R % 128) + R / 128, so block (i, j), register e, lane (li, h)
    // holds output channel co0 + 2 (32 (2 (zq & 1) + i) + (e & 3) + 8 (e >> 2) + 4 h) + (zq >> 1) and input channel
    // ci0 + 2 (64 hx + 32 (j & 1) + li) + (j >> 1)
    float* __restrict__ part = p.part + ((int64_t)(split * 16 + xi) * p.Cout) * p.Cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = co0 + 2 * (32 * (2 * (zq & 1) + i) + (e & 3) + 8 * (e >> 2) + 4 * h) + (zq >> 1);
            float* row = part + (int64_t)co * p.Cin + ci0 + 2 * (64 * hx + li);
            *reinterpret_cast<float2*>(row) = make_float2(acc[i][0][e], acc[i][2][e]);
            *reinterpret_cast<float2*>(row + 64) = make_float2(acc[i][1][e], acc[i][3][e]);
        }
}

// dW[co][3 a + b][ci] (+)= sum_{i, j} At[a][i] At[b][j] sum_s part[s][4 i + j][co][ci]: slabs in order s = 0, 1, ..., then the column pass,
// then the row pass -- one summation order for any grid.  A block takes one output channel and 64 input channels: thread (position, four
// input channels) sums its column of the slabs, the 16 positions meet in LDS, 9 x 16 threads write the taps.
__global__ __launch_bounds__(256) void wgrad_wino_reduce_kernel(const float* __restrict__ part, int nsplit, int Cout, int Cin,
                                                                 float* __restrict__ dW, int accumulate) {
    __shared__ float4 du[16][16];
    const int co = blockIdx.x, xi = threadIdx.x >> 4, c4 = threadIdx.x & 15;
    const int ci = blockIdx.y * 64 + c4 * 4;
    const int64_t slab = (int64_t)16 * Cout * Cin;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ci < Cin) {
        const float* src = part + ((int64_t)xi * Cout + co) * Cin + ci;
        for (int k = 0; k < nsplit; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(src + k * slab);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    du[xi][c4] = s;
    __syncthreads();
    if (threadIdx.x >= 9 * 16 || ci >= Cin) return;
    const int a = xi / 3, b = xi - 3 * a;      // (xi < 9 here: the tap)
    auto col = [&](int i) {      // (dU At^T)[i][b]
        const float4 u1 = du[4 * i + 1][c4], u2 = du[4 * i + 2][c4];
        if (b == 1) return make_float4(u1.x - u2.x, u1.y - u2.y, u1.z - u2.z, u1.w - u2.w);
        const float4 u0 = du[4 * i + (b == 0 ? 0 : 3)][c4];
        return make_float4((u1.x + u2.x) + u0.x, (u1.y + u2.y) + u0.y, (u1.z + u2.z) + u0.z, (u1.w + u2.w) + u0.w);
    };
    const float4 e1 = col(1), e2 = col(2);
    float4 o;
    if (a == 1) o = make_float4(e1.x - e2.x, e1.y - e2.y, e1.z - e2.z, e1.w - e2.w);
    else {
        const float4 e0 = col(a == 0 ? 0 : 3);
        o = make_float4((e1.x + e2.x) + e0.x, (e1.y + e2.y) + e0.y, (e1.z + e2.z) + e0.z, (e1.w + e2.w) + e0.w);
    }
    float* dst = dW + ((int64_t)co * 9 + xi) * Cin + ci;
    if (accumulate) {
        const float4 old = *reinterpret_cast<const float4*>(dst);
        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
    }
    *reinterpret_cast<float4*>(dst) = o;
}

int64_t wino_tiles(const erd_wgrad_desc* d) {
    int64_t n = 0;
    for (int l = 0; l < d->nseg; ++l) n += (int64_t)d->seg[l].N * ((d->seg[l].GH + 1) / 2) * ((d->seg[l].GW + 1) / 2);
    return n;
}

// Channels per workgroup and side of the kernel a launch takes: 256 (one position per workgroup) where both channel counts are multiples
// of 256, else 128 (a transform row per workgroup).  ERD_WGRAD_WINO_TILE=128|256 forces either where the shape allows it (A/B aid, read
// per call: tests/test_gpu_wgrad_wino_pos.py flips it inside one process to compare the slabs bit for bit).
int wino_tile(const erd_wgrad_desc* d) {
    const bool can = d->Cin % BP == 0 && d->Cout % BP == 0;
    const char* const e = getenv("ERD_WGRAD_WINO_TILE");
    const int force = e ? atoi(e) : 0;
    if (force == BC || !can) return BC;
    return BP;
}

}  // namespace

// 128 | 256: the kernel erd_conv_wgrad_wino would launch for this descriptor now (see wino_tile), 0 where it refuses the descriptor
extern "C" int erd_conv_wgrad_wino_tile(const erd_wgrad_desc* d) { return erd_conv_wgrad_wino_ok(d) ? wino_tile(d) : 0; }

// 1: erd_conv_wgrad_wino takes this descriptor (the routing predicate of the host): a 3x3 / stride 1 / pad 1 layer in tap order with fp32
// maps, one group, Cin and Cout multiples of 128
extern "C" int erd_conv_wgrad_wino_ok(const erd_wgrad_desc* d) {
    if (!d || d->bf16_multiplicands || d->x_bf16 || d->dz_bf16 || d->ngroups != 1) return 0;
    if (d->nseg < 1 || d->nseg > ERD_MAX_SEG || d->Cin < BC || d->Cout < BC || d->Cin % BC || d->Cout % BC) return 0;
    if (d->x_elems <= 0 || d->dz_elems <= 0 || d->x_elems >= (1ll << 29) || d->dz_elems >= (1ll << 29)) return 0;
    for (int l = 0; l < d->nseg; ++l)
        if (d->seg[l].N < 1 || d->seg[l].GH < 1 || d->seg[l].GW < 1) return 0;
    return erd_wgrad_row3_slices(d) > 0 && wino_tiles(d) < (1ll << 30);      // (the geometry test of the three-tap kernels)
}

// Partial slabs part[nsplit][16][Cout][Cin] of the Winograd-domain weight gradient (erd_wgrad_wino_reduce folds them into dW); the
// descriptor is erd_conv_wgrad's, with `part` holding nsplit * 16 * Cout * Cin floats.  Every slab is written whole (an empty split: zeros).
extern "C" int erd_conv_wgrad_wino(const erd_wgrad_desc* d, erd_stream_t stream) {
    ERD_REQUIRE(d != nullptr && d->part && d->x && d->dz, "wgrad_wino: null pointer");
    ERD_REQUIRE(!d->bf16_multiplicands && !d->x_bf16 && !d->dz_bf16, "wgrad_wino: fp32 maps and the three-limb form only");
    ERD_REQUIRE(d->ngroups == 1, "wgrad_wino: ngroups=%d", d->ngroups);
    ERD_REQUIRE(d->Cin >= BC && d->Cout >= BC && d->Cin % BC == 0 && d->Cout % BC == 0, "wgrad_wino: Cin=%d Cout=%d must be multiples of %d", d->Cin,
                d->Cout, BC);
    ERD_REQUIRE(d->in_stride == 1 && d->out_stride == 1, "wgrad_wino: stride 1 only");
    ERD_REQUIRE(erd_conv_wgrad_wino_ok(d), "wgrad_wino: not a 3x3 / stride 1 / pad 1 layer over 1 .. %d non-empty maps below 2 GiB", ERD_MAX_SEG);
    const int64_t grid = (int64_t)4 * (d->Cin / BC) * (d->Cout / BC) * d->nsplit;      // (= 16 x (Cin / 256) x (Cout / 256) x nsplit)
    ERD_REQUIRE(d->nsplit >= 1 && grid < (1 << 20), "wgrad_wino: nsplit=%d", d->nsplit);
    const int ntiles = (int)wino_tiles(d), nsteps = (ntiles + KT - 1) / KT;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_wgrad_wino_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_wino_pos_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PLDS_BYTES);
        attr_done = true;
    }
    if (wino_tile(d) == BP) hipLaunchKernelGGL(wgrad_wino_pos_kernel, dim3((unsigned)grid), dim3(WT), PLDS_BYTES, (hipStream_t)stream, *d, ntiles, nsteps);
    else hipLaunchKernelGGL(conv_wgrad_wino_kernel, dim3((unsigned)grid), dim3(WT), LDS_BYTES, (hipStream_t)stream, *d, ntiles, nsteps);
    return erd::check_launch("conv_wgrad_wino");
}

extern "C" int erd_wgrad_wino_reduce(const float* part, int nsplit, int Cout, int Cin, float* dW, int accumulate, erd_stream_t stream) {
    ERD_REQUIRE(part && dW && nsplit >= 1 && Cout >= 1 && Cin >= 4 && Cin % 4 == 0, "wgrad_wino_reduce: bad args");
    hipLaunchKernelGGL(wgrad_wino_reduce_kernel, dim3(Cout, (Cin + 63) / 64), dim3(256), 0, (hipStream_t)stream, part, nsplit, Cout, Cin, dW,
                       accumulate & 1);
    return erd::check_launch("wgrad_wino_reduce");
}
