// mrts_conv.hip -- the first encoder stage of a GridNet policy on the packed observation words:
// Conv2d(P, C, 3, padding = 1) -> MaxPool2d(3, 2, 1) -> ReLU, forward and the backward to the
// parameters, straight from one 32-bit one-hot word per cell (bit i = plane i, mrts_rules.h
// cell_onehot).  Over a one-hot input the convolution has no multiplies: an output is the bias
// plus, per tap, the sum of the weights the neighbour's set bits select (include/microrts_amd.h
// states the order of the adds, which the kernels keep).  Nothing dense is ever written: 4 bytes a
// cell in, the pooled [N, C, Ho, Wo] out; the backward recomputes the forward from the words.
//
// A workgroup owns a slice of CL = 32 output channels (grid.y) and walks tiles of Ti x Tj pooled
// outputs of one image (grid.x strides over N * tiles).  Its LDS holds
//   tbl  [tap][plane][CL]  the slice's weights, read 16 bytes (four channels) a lane
//   te   [tap][CL]         the tap sums of the empty cell's word (most cells: one read per tap)
//   w    the tile's words with a halo of 2 (zero outside the map: a zero word adds nothing)
//   conv [2 Ti + 1][2 Tj + 1][CL + 1]  the tile's conv outputs, -inf outside the map
// and a tile is three phases: stage the words; a lane per (four channels, conv cell) sums its nine taps;
// a lane per (channel, pooled output), column fastest, takes the window's maximum.  The backward
// adds per pooled output the first maximum's position and its gradient (zero when the maximum is
// not positive), then a lane per (channel, tap) keeps one accumulator per plane in registers over
// all of the workgroup's tiles.  Each workgroup writes its partial sums as a row of the workspace; k_obs_conv_reduce adds the rows in index order.  No float atomics:
// the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "mrts_engine.h"

namespace mrts {
namespace oconv {

constexpr int CL = 32;        // channel lanes: a workgroup's channel slice (a short last slice idles lanes)
constexpr int CG = CL / 4;    // a lane of the conv phase takes four channels: 16-byte reads of the table
constexpr int CP = CL + 1;    // the conv tile's channel stride: lanes over cells of one channel hit distinct banks
constexpr int FT = 512;       // forward workgroup
constexpr int BT = 512;       // backward workgroup (its accumulating lanes: CL channels x 9 taps)
constexpr int PMAX = 31;
constexpr int FWD_BLOCKS = 1024, BWD_BLOCKS = 512;   // grid.x caps: a workgroup loads its weight table once
constexpr int TJ_MAX = 8, TI_MAX = 8;
// the empty cell's word (hp 0, resources 0, no owner, no unit, no action, free terrain); with fog also "not seen by the opponent"
constexpr uint32_t EMPTY = 1u | (1u << 5) | (1u << 10) | (1u << 13) | (1u << 21) | (1u << 27);

struct Args {
    const uint32_t* packed;   // [N][H][W]
    const float* weight;      // [C][P][3][3]
    const float* bias;        // [C]
    int N, H, W, P, C, Ho, Wo;
    int Ti, Tj, nbi, nbj;     // pooled outputs per tile, tiles per image
};

struct Lds {
    float *tbl, *te, *bias, *conv, *g;
    uint32_t* w;
    int* pos;
};
// the one LDS layout of both kernels; its end offset is the launch's dynamic LDS
__host__ __device__ inline size_t carve(Carver& cv, Lds& L, int P, int Ti, int Tj, bool bwd) {
    L.tbl = cv.take<float>((size_t)9 * (P + 1) * CL);
    L.te = cv.take<float>(9 * CL);
    L.bias = cv.take<float>(CL);
    L.w = cv.take<uint32_t>((size_t)(2 * Ti + 3) * (2 * Tj + 3));
    L.conv = cv.take<float>((size_t)(2 * Ti + 1) * (2 * Tj + 1) * CP);
    L.g = bwd ? cv.take<float>((size_t)Ti * Tj * CP) : nullptr;
    L.pos = bwd ? cv.take<int>((size_t)Ti * Tj * CP) : nullptr;
    return cv.o;
}
inline size_t lds_bytes(int P, int Ti, int Tj, bool bwd) {
    Carver cv{lds_any_base()};
    Lds L;
    return carve(cv, L, P, Ti, Tj, bwd);
}

// t of the contract for a lane's four channels: the selected weights of one tap in ascending plane order, from the
// first one.  The next TB set planes' rows are read together -- a one-hot word's whole rest, so one LDS round trip
// instead of one per plane -- and added in order; a plane that is not there reads the table's row P, which holds
// -0.0: x + -0.0 is x for every x, signed zeros included, so those adds change no bit and nothing branches.  A zero
// word returns that row, -0.0: adding it is skipping the tap.
constexpr int TB = 6;
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void add4(float4& t, const float4& v) {
    t.x += v.x;
    t.y += v.y;
    t.z += v.z;
    t.w += v.w;
}
__device__ __forceinline__ float4 tap_sum(const float* __restrict__ tb, uint32_t w, int P) {
    float4 t = ld4(tb + (w ? __ffs((int)w) - 1 : P) * CL);
    w &= w - 1;
    while (w) {
        float4 v[TB];
#pragma unroll
        for (int i = 0; i < TB; i++) {
            v[i] = ld4(tb + (w ? __ffs((int)w) - 1 : P) * CL);
            w &= w - 1;
        }
#pragma unroll
        for (int i = 0; i < TB; i++) add4(t, v[i]);
    }
    return t;
}

// tbl [tap][P + 1][CL]: the slice's weights and per tap the -0.0 row; te [tap][CL]: the empty word's tap sums
template <int NT>
__device__ __forceinline__ void load_table(const Lds& L, const Args& a, int c0, int CS) {
    const int P = a.P, n = 9 * (P + 1) * CL;
    for (int l = threadIdx.x; l < n; l += NT) {
        const int c = l % CL, tp = l / CL, p = tp % (P + 1), tap = tp / (P + 1);
        L.tbl[l] = p == P ? -0.0f : c < CS ? a.weight[((size_t)(c0 + c) * P + p) * 9 + tap] : 0.0f;
    }
    if (threadIdx.x < CL) L.bias[threadIdx.x] = (int)threadIdx.x < CS ? a.bias[c0 + threadIdx.x] : 0.0f;
    __syncthreads();
    const uint32_t E = EMPTY | (P == 31 ? 1u << 29 : 0u);
    if (threadIdx.x < 9 * CG) {
        const int tap = threadIdx.x / CG, c4 = (threadIdx.x % CG) * 4;
        *reinterpret_cast<float4*>(L.te + tap * CL + c4) = tap_sum(L.tbl + tap * (P + 1) * CL + c4, E, P);
    }
    // (the tile's first barrier orders te)
}

struct Tile {
    int n, i0, j0, ti, tj;
};
__device__ __forceinline__ Tile tile_of(const Args& a, long long t) {
    const int per = a.nbi * a.nbj, r = (int)(t % per);
    Tile q;
    q.n = (int)(t / per);
    q.i0 = (r / a.nbj) * a.Ti;
    q.j0 = (r % a.nbj) * a.Tj;
    q.ti = min(a.Ti, a.Ho - q.i0);
    q.tj = min(a.Tj, a.Wo - q.j0);
    return q;
}

// A tile: conv cell (cy, cx) of the tile is map cell (2 i0 - 1 + cy, 2 j0 - 1 + cx), word (wy, wx) is map cell
// (2 i0 - 2 + wy, 2 j0 - 2 + wx): tap (ky, kx) of conv cell (cy, cx) is word (cy + ky, cx + kx).
// A tile has at most NT words, one per thread: a thread reads the next tile's word while this tile computes.
static_assert((2 * TI_MAX + 3) * (2 * TJ_MAX + 3) <= FT && FT <= BT && 9 * CL <= BT, "a word per thread; the accumulating lanes");
__device__ __forceinline__ uint32_t fetch_word(const Args& a, const Tile& q) {
    const int ww = 2 * q.tj + 3, k = threadIdx.x, wy = k / ww, wx = k - wy * ww, y = 2 * q.i0 - 2 + wy, x = 2 * q.j0 - 2 + wx;
    if (wy >= 2 * q.ti + 3 || (unsigned)y >= (unsigned)a.H || (unsigned)x >= (unsigned)a.W) return 0u;   // zero outside the map
    return a.packed[((size_t)q.n * a.H + y) * a.W + x] & ((1u << a.P) - 1u);
}
// phase 1: stage the tile's words (`word`: this thread's, from fetch_word)
__device__ __forceinline__ void stage_words(const Lds& L, const Args& a, const Tile& q, uint32_t word) {
    const int ww = 2 * q.tj + 3, k = threadIdx.x, wy = k / ww, wx = k - wy * ww;
    __syncthreads();   // the previous tile's readers are done
    if (wy < 2 * q.ti + 3) L.w[wy * (2 * a.Tj + 3) + wx] = word;
}
// phase 2: the tile's conv outputs
template <int NT>
__device__ __forceinline__ void conv_tile(const Lds& L, const Args& a, const Tile& q) {
    const int WS = 2 * a.Tj + 3, CWS = 2 * a.Tj + 1;
    const uint32_t E = EMPTY | (a.P == 31 ? 1u << 29 : 0u);
    __syncthreads();
    const int ch = 2 * q.ti + 1, cw = 2 * q.tj + 1, c4 = (threadIdx.x % CG) * 4, TR = (a.P + 1) * CL;
    const float4 b = ld4(L.bias + c4);
    for (int k = threadIdx.x / CG; k < ch * cw; k += NT / CG) {
        const int cy = k / cw, cx = k - cy * cw, y = 2 * q.i0 - 1 + cy, x = 2 * q.j0 - 1 + cx;
        float4 acc = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);   // outside the map: never a window's maximum
        if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
            acc = b;
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const uint32_t w = L.w[(cy + tap / 3) * WS + cx + tap % 3];
                add4(acc, w == E ? ld4(L.te + tap * CL + c4) : tap_sum(L.tbl + tap * TR + c4, w, a.P));
            }
        }
        float* o = L.conv + (cy * CWS + cx) * CP + c4;   // (CP is odd: four 4-byte stores)
        o[0] = acc.x;
        o[1] = acc.y;
        o[2] = acc.z;
        o[3] = acc.w;
    }
    __syncthreads();
}

__global__ __launch_bounds__(FT) void k_obs_conv_fwd(Args a, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Carver cv{smem};
    Lds L;
    carve(cv, L, a.P, a.Ti, a.Tj, false);
    const int c0 = blockIdx.y * CL, CS = min(CL, a.C - c0), CWS = 2 * a.Tj + 1;
    load_table<FT>(L, a, c0, CS);
    const long long tiles = (long long)a.N * a.nbi * a.nbj;
    Tile q = tile_of(a, blockIdx.x);   // (the grid has no more workgroups than tiles)
    uint32_t word = fetch_word(a, q);
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        stage_words(L, a, q, word);
        const Tile cur = q;
        if (t + gridDim.x < tiles) {
            q = tile_of(a, t + gridDim.x);
            word = fetch_word(a, q);
        }
        conv_tile<FT>(L, a, cur);
        const int per = cur.ti * cur.tj;
        for (int k = threadIdx.x; k < CS * per; k += FT) {
            const int c = k / per, r = k - c * per, li = r / cur.tj, lj = r - li * cur.tj;
            const float* cv0 = L.conv + ((2 * li) * CWS + 2 * lj) * CP + c;
            float m = -INFINITY;
#pragma unroll
            for (int d = 0; d < 9; d++) {
                const float v = cv0[((d / 3) * CWS + d % 3) * CP];
                if (v > m) m = v;
            }
            out[(((size_t)cur.n * a.C + c0 + c) * a.Ho + cur.i0 + li) * a.Wo + cur.j0 + lj] = m > 0.0f ? m : 0.0f;
        }
    }
}

// ws: [gridDim.x][rowlen] partial sums, a row = grad_weight's [C][P][3][3] then grad_bias's [C]
__global__ __launch_bounds__(BT) void k_obs_conv_bwd(Args a, const float* __restrict__ gout, float* __restrict__ ws, int rowlen) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Carver cv{smem};
    Lds L;
    carve(cv, L, a.P, a.Ti, a.Tj, true);
    const int c0 = blockIdx.y * CL, CS = min(CL, a.C - c0), CWS = 2 * a.Tj + 1, WS = 2 * a.Tj + 3;
    load_table<BT>(L, a, c0, CS);
    const int c = threadIdx.x % CL, tap = threadIdx.x / CL;   // tap >= 9: no accumulating lane
    const int tapoff = (tap / 3) * WS + tap % 3;
    float acc[PMAX], accb = 0.0f;
#pragma unroll
    for (int p = 0; p < PMAX; p++) acc[p] = 0.0f;
    const long long tiles = (long long)a.N * a.nbi * a.nbj;
    Tile q = tile_of(a, blockIdx.x);   // (the grid has no more workgroups than tiles)
    uint32_t word = fetch_word(a, q);
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        stage_words(L, a, q, word);
        const Tile cur = q;
        if (t + gridDim.x < tiles) {
            q = tile_of(a, t + gridDim.x);
            word = fetch_word(a, q);
        }
        conv_tile<BT>(L, a, cur);
        const int per = cur.ti * cur.tj;
        for (int k = threadIdx.x; k < CS * per; k += BT) {
            const int cc = k / per, r = k - cc * per, li = r / cur.tj, lj = r - li * cur.tj;
            const float* cv0 = L.conv + ((2 * li) * CWS + 2 * lj) * CP + cc;
            float m = -INFINITY;
            int arg = 0;
#pragma unroll
            for (int d = 0; d < 9; d++) {   // row-major, strict >: the first maximum
                const float v = cv0[((d / 3) * CWS + d % 3) * CP];
                if (v > m) { m = v; arg = d; }
            }
            const bool on = m > 0.0f;
            L.g[r * CP + cc] = on ? gout[(((size_t)cur.n * a.C + c0 + cc) * a.Ho + cur.i0 + li) * a.Wo + cur.j0 + lj] : 0.0f;
            L.pos[r * CP + cc] = on ? (2 * li + arg / 3) * WS + 2 * lj + arg % 3 : 0;
        }
        __syncthreads();
        if (c < CS && tap < 9) {
            for (int r = 0; r < per; r++) {
                const float g = L.g[r * CP + c];
                const uint32_t w = L.w[L.pos[r * CP + c] + tapoff];
#pragma unroll
                for (int p = 0; p < PMAX; p++) acc[p] += (w >> p) & 1u ? g : 0.0f;
                accb += g;
            }
        }
    }
    if (c < CS && tap < 9) {
        float* row = ws + (size_t)blockIdx.x * rowlen;
#pragma unroll
        for (int p = 0; p < PMAX; p++)
            if (p < a.P) row[((size_t)(c0 + c) * a.P + p) * 9 + tap] = acc[p];
        if (tap == 0) row[(size_t)a.C * a.P * 9 + c0 + c] = accb;
    }
}

__global__ __launch_bounds__(256) void k_obs_conv_reduce(const float* __restrict__ ws, int rows, int rowlen, int nw,
                                                          float* __restrict__ gw, float* __restrict__ gb) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= rowlen) return;
    float s = ws[e];
    for (int r = 1; r < rows; r++) s += ws[(size_t)r * rowlen + e];
    if (e < nw) gw[e] = s;
    else gb[e - nw] = s;
}

// The tile of a shape: the widest Tj <= TJ_MAX, then the tallest Ti whose carve fits 64 KB, evened out over
// the image's row bands.  false: not even one pooled output fits.
static bool tiling(Args& a, bool bwd) {
    a.Ho = (a.H - 1) / 2 + 1;
    a.Wo = (a.W - 1) / 2 + 1;
    a.nbj = (a.Wo + TJ_MAX - 1) / TJ_MAX;
    a.Tj = (a.Wo + a.nbj - 1) / a.nbj;
    int Ti = std::min(a.Ho, TI_MAX);
    while (Ti >= 1 && lds_bytes(a.P, Ti, a.Tj, bwd) > MRTS_LDS_CAP) Ti--;
    if (Ti < 1) return false;
    a.nbi = (a.Ho + Ti - 1) / Ti;
    a.Ti = (a.Ho + a.nbi - 1) / a.nbi;
    a.nbi = (a.Ho + a.Ti - 1) / a.Ti;
    a.nbj = (a.Wo + a.Tj - 1) / a.Tj;
    return true;
}
static Args make_args(const int32_t* packed, int n, int h, int w, int planes, const float* weight, const float* bias, int channels) {
    Args a{};
    a.packed = reinterpret_cast<const uint32_t*>(packed);
    a.weight = weight;
    a.bias = bias;
    a.N = n; a.H = h; a.W = w; a.P = planes; a.C = channels;
    return a;
}
static int bwd_blocks(const Args& a) { return (int)std::min<long long>((long long)a.N * a.nbi * a.nbj, BWD_BLOCKS); }

}  // namespace oconv
}  // namespace mrts

// The launchers take the caller's stream, allocate nothing and synchronise nothing (mrts_capi.cpp has checked
// the arguments: planes 29 / 31, channels 1..64, the map within MRTS_MAX_HW cells, n * h * w within 32 bits).
extern "C" {
using namespace mrts::oconv;
// bytes of the backward's workspace (0 for n == 0), or -1 for a shape whose tile does not fit
long long mrts_engine_obs_conv_workspace(int n, int h, int w, int planes, int channels) {
    if (n == 0) return 0;
    Args a = make_args(nullptr, n, h, w, planes, nullptr, nullptr, channels);
    if (!tiling(a, true)) return -1;
    return (long long)bwd_blocks(a) * ((long long)channels * planes * 9 + channels) * (long long)sizeof(float);
}
hipError_t mrts_engine_obs_conv_fwd(const int32_t* packed, int n, int h, int w, int planes, const float* weight, const float* bias,
                                    int channels, float* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    Args a = make_args(packed, n, h, w, planes, weight, bias, channels);
    if (!tiling(a, false)) return hipErrorInvalidValue;
    const long long tiles = (long long)n * a.nbi * a.nbj;
    const dim3 grid((unsigned)std::min<long long>(tiles, FWD_BLOCKS), (unsigned)((channels + CL - 1) / CL));
    hipLaunchKernelGGL(k_obs_conv_fwd, grid, dim3(FT), lds_bytes(planes, a.Ti, a.Tj, false), s, a, out);
    return hipGetLastError();
}
hipError_t mrts_engine_obs_conv_bwd(const int32_t* packed, int n, int h, int w, int planes, const float* weight, const float* bias,
                                    int channels, const float* grad_out, float* ws, float* grad_weight, float* grad_bias, hipStream_t s) {
    Args a = make_args(packed, n, h, w, planes, weight, bias, channels);
    const int nw = channels * planes * 9, rowlen = nw + channels;
    if (n == 0) return hipSuccess;
    if (!tiling(a, true)) return hipErrorInvalidValue;
    const int blocks = bwd_blocks(a);
    hipLaunchKernelGGL(k_obs_conv_bwd, dim3(blocks, (channels + CL - 1) / CL), dim3(BT), lds_bytes(planes, a.Ti, a.Tj, true), s, a,
                       grad_out, ws, rowlen);
    hipLaunchKernelGGL(k_obs_conv_reduce, dim3((rowlen + 255) / 256), dim3(256), 0, s, ws, blocks, rowlen, nw, grad_weight, grad_bias);
    return hipGetLastError();
}
}
