// realToComplex / complexToReal (Liquid.chs:503-546): liquid's firhilbf half-band Hilbert transform, 2:1 decimator and 1:2
// interpolator.
//   k_firhilb_decim  : 2n reals -> n complex      k_firhilb_interp : n complex -> 2n reals                  time-parallel
// Both directions are one memory operation.  With the float stream E = history ++ input taken in pairs (E[2p], E[2p + 1]) --
// (x0, x1) of the decimator, (re, im) of the interpolator -- the even floats are what liquid pushes into w1 and the odd ones what
// it pushes into w0, and pair p of the call yields the two floats
//     out[2p]     = w0[m - 1]              = E[2 (p + m) + 1]                            (the delay branch)
//     out[2p + 1] = sum_j hq[j] w1[j]      = sum_j hq[j] E[2 (p + 1 + j)], j = 0 .. 2m-1 (the quadrature branch)
// which are (re, im) of the decimator's output and (y[0], y[1]) of the interpolator's.  The history is the last 2m pairs of E,
// kept in the handle pair-interleaved (w1[j], w0[j]) in two copies used in turn, so no workgroup reads what another writes.
// A workgroup stages a tile of TILE pairs plus 2m pairs in front through LDS, even and odd floats apart; a thread owns two
// consecutive output pairs: one 16-byte load, one 16-byte store, LDS reads at a lane stride of 8 bytes.
// Arithmetic contract: plain f32, no contraction, the sum taken j = 0 .. 2m-1 starting from the first product.  The output is
// the same for every chunking of the stream, bit for bit, and tests/firhilb_restatement.py restates it exactly.
#include "../../include/csdr.h"
#include "csdr_internal.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr int FT = 256;             // threads per workgroup
constexpr int TILE = 2 * FT;        // output pairs per tile
constexpr uint32_t MAX_GRID = 2048;

__device__ __forceinline__ void firhilb_body(const float *__restrict__ X, float *__restrict__ Y, const float *__restrict__ hin,
                                             float *__restrict__ hout, const FirhilbLaunch &l)
{
    __shared__ __attribute__((aligned(16))) float ev[TILE + 2 * FIRHILB_MAX_M], od[TILE + 2 * FIRHILB_MAX_M];
    const uint32_t t = threadIdx.x, m = l.m, H = 2 * m;          // H pairs of history
    const size_t n = l.n, nf = 2 * n;
    // float e of E: the history for e < 2H, the call's input behind it
    auto ext = [&](size_t e) { return e < 2 * H ? hin[e] : X[e - 2 * H]; };
    if (blockIdx.x == 0 && t < 2 * H) hout[t] = ext(nf + t);      // the next call's history: the last H pairs of E
    const size_t ntiles = (n + TILE - 1) / TILE;
    // the tile's own 2 TILE floats, four per thread: X[2 p0 + 4 t ..]
    auto load = [&](size_t tile) {
        const size_t f = 2 * tile * TILE + 4 * (size_t)t;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l.vec && f + 4 <= nf) v = *reinterpret_cast<const float4 *>(X + f);
        else {
            if (f < nf) v.x = X[f];
            if (f + 1 < nf) v.y = X[f + 1];
            if (f + 2 < nf) v.z = X[f + 2];
            if (f + 3 < nf) v.w = X[f + 3];
        }
        return v;
    };
    float4 cur = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x < ntiles) cur = load(blockIdx.x);
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t p0 = tile * TILE;                            // first output pair of the tile = first E pair of its window
        if (t < 2 * H) {                                          // the H pairs in front of the tile's own input
            const float v = ext(2 * p0 + t);
            if (t & 1) od[t >> 1] = v; else ev[t >> 1] = v;
        }
        *reinterpret_cast<float2 *>(ev + H + 2 * t) = make_float2(cur.x, cur.z);
        *reinterpret_cast<float2 *>(od + H + 2 * t) = make_float2(cur.y, cur.w);
        __syncthreads();
        if (tile + gridDim.x < ntiles) cur = load(tile + gridDim.x);     // in flight while this tile is computed
        const uint32_t i = 2 * t;                                 // local pairs i, i + 1
        const float *w = ev + i + 1;
        float nx = w[1];
        float a0 = l.hq[0] * w[0], a1 = l.hq[0] * nx;
        for (uint32_t j = 1; j < H; j++) {
            const float c = nx;
            nx = w[j + 1];
            a0 = a0 + l.hq[j] * c;
            a1 = a1 + l.hq[j] * nx;
        }
        const float4 o = make_float4(od[i + m], a0, od[i + m + 1], a1);
        const size_t p = p0 + i;
        if (l.vec && p + 2 <= n) *reinterpret_cast<float4 *>(Y + 2 * p) = o;
        else {
            if (p < n) { Y[2 * p] = o.x; Y[2 * p + 1] = o.y; }
            if (p + 1 < n) { Y[2 * p + 2] = o.z; Y[2 * p + 3] = o.w; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(FT) void k_firhilb_decim(const float *__restrict__ X, float *__restrict__ Y, const float *__restrict__ hin,
                                                      float *__restrict__ hout, FirhilbLaunch l)
{
    firhilb_body(X, Y, hin, hout, l);
}

__global__ __launch_bounds__(FT) void k_firhilb_interp(const float *__restrict__ X, float *__restrict__ Y, const float *__restrict__ hin,
                                                       float *__restrict__ hout, FirhilbLaunch l)
{
    firhilb_body(X, Y, hin, hout, l);
}

}  // namespace

int launch_firhilb(bool interp, const float *x, float *y, const float *hist_in, float *hist_out, FirhilbLaunch l, hipStream_t s)
{
    if (!l.n) return 0;
    l.vec = (((uintptr_t)x | (uintptr_t)y) & 15u) == 0;
    const uint64_t ntiles = ((uint64_t)l.n + TILE - 1) / TILE;
    const dim3 grid((uint32_t)(ntiles < MAX_GRID ? ntiles : MAX_GRID));
    if (interp) hipLaunchKernelGGL(k_firhilb_interp, grid, dim3(FT), 0, s, x, y, hist_in, hist_out, l);
    else hipLaunchKernelGGL(k_firhilb_decim, grid, dim3(FT), 0, s, x, y, hist_in, hist_out, l);
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr
