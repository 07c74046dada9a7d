// firFilterC / firFilterR / firFilterCKaiser (Liquid.chs:868-916, 955-957): liquid's firfilt_crcf / firfilt_rrrf on C independent
// rows of CF32 or F32 samples with real taps.
//   k_firfilt<CPLX> : 2048 consecutive outputs of one row per workgroup, 8 consecutive outputs per thread     direct form, no recurrence
// A workgroup stages its 2048 samples and the L - 1 in front of them (from the row, or from the history buffer at the row's
// start) into LDS: 16-byte global loads where the alignment allows.  A thread then walks the taps once: at tap i it reads the
// one sample x[t0 - i] it has not seen yet, keeps the 8 it needs in a register window that slides by one, and adds h[i] times
// the window to its 8 sums.  The tap index is the same for every lane, so the taps come through scalar loads.  LDS slot k sits at
// k + k / 8: a thread stride of 8 samples would otherwise put the lanes of a read on a handful of banks.  The 8 results go back
// through the same LDS so that the stores are whole lines.  The first workgroup of a row also writes the row's next history
// (the last L - 1 samples of history | row) into the other half of a ping-pong pair.
// Arithmetic contract: plain f32, no contraction.  acc = +0; for i = 0 .. L - 1 in that order acc = acc + h[i] * x[t - i], the
// product rounded, then the sum; y = scale * acc; re and im separately.  Nothing in it depends on the call size, where a stream
// is cut, the row count or the grid.  tests/fir_restatement.py restates it exactly.
#include "../../include/csdr.h"
#include "csdr_internal.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr int FF_T = 256;               // threads per workgroup
constexpr int FF_R = 8;                 // consecutive outputs per thread
constexpr int FF_TILE = FF_T * FF_R;    // outputs per workgroup

__device__ __forceinline__ uint32_t sk(uint32_t k) { return k + (k >> 3); }
__device__ __forceinline__ float zero_of(float) { return 0.f; }
__device__ __forceinline__ float2 zero_of(float2) { return make_float2(0.f, 0.f); }
__device__ __forceinline__ float mac(float a, float h, float x) { const float p = h * x; return a + p; }
__device__ __forceinline__ float2 mac(float2 a, float h, float2 x)
{
    const float pr = h * x.x, pi = h * x.y;
    return make_float2(a.x + pr, a.y + pi);
}
__device__ __forceinline__ float scaled(float s, float a) { return s * a; }
__device__ __forceinline__ float2 scaled(float s, float2 a) { return make_float2(s * a.x, s * a.y); }

// vec: X, Y and every row start are 16-byte aligned (set by the launcher)
template <bool CPLX>
__global__ __launch_bounds__(FF_T) void k_firfilt(const void *__restrict__ Xv, void *__restrict__ Yv, const float *__restrict__ h,
                                                  const void *__restrict__ hist_in, void *__restrict__ hist_out, FirfiltLaunch l,
                                                  uint32_t tiles, uint32_t vec)
{
    using T = typename std::conditional<CPLX, float2, float>::type;
    constexpr int PV = CPLX ? 2 : 4;                                    // samples per 16 bytes
    extern __shared__ float4 lds4[];
    T *s = reinterpret_cast<T *>(lds4);
    const uint32_t L = l.L, H = L - 1, n = l.n, tid = threadIdx.x;
    const uint32_t c = blockIdx.x / tiles, T0 = (blockIdx.x - c * tiles) * FF_TILE;
    const T *row = static_cast<const T *>(Xv) + (size_t)c * n, *hin = static_cast<const T *>(hist_in) + (size_t)c * H;
    T *orow = static_cast<T *>(Yv) + (size_t)c * n;
    const bool whole = vec && T0 + FF_TILE <= n;                         // the tile lies inside the row: 16-byte loads and stores

    // LDS slot k (at sk(k)) holds x[T0 - H + k], k < H + FF_TILE; past the row's end it holds 0 (never part of a stored output)
    for (uint32_t k = tid; k < H; k += FF_T) {
        const int64_t t = (int64_t)T0 - H + k;
        s[sk(k)] = t >= 0 ? row[t] : hin[(int64_t)H + t];
    }
    if (whole) {
        const float4 *src = reinterpret_cast<const float4 *>(row + T0);
#pragma unroll
        for (int i = 0; i < FF_TILE / PV / FF_T; i++) {
            const uint32_t e = tid + FF_T * i, k = H + e * PV;
            const float4 q = src[e];
            if constexpr (CPLX) { s[sk(k)] = make_float2(q.x, q.y); s[sk(k + 1)] = make_float2(q.z, q.w); }
            else { s[sk(k)] = q.x; s[sk(k + 1)] = q.y; s[sk(k + 2)] = q.z; s[sk(k + 3)] = q.w; }
        }
    } else {
#pragma unroll
        for (int i = 0; i < FF_R; i++) {
            const uint32_t e = tid + FF_T * i, t = T0 + e;
            s[sk(H + e)] = t < n ? row[t] : zero_of(T());
        }
    }
    // the row's next history: the last H samples of (history | row), also when n < H
    if (T0 == 0) {
        T *hout = static_cast<T *>(hist_out) + (size_t)c * H;
        for (uint32_t i = tid; i < H; i += FF_T) {
            const int64_t t = (int64_t)n - H + i;
            hout[i] = t >= 0 ? row[t] : hin[(int64_t)H + t];
        }
    }
    __syncthreads();

    // output r of this thread is t = T0 + FF_R tid + r and meets, at tap i, slot base + (r - i); the window keeps slot
    // base + q in win[q mod FF_R], so that tap i = i0 + u (i0 a multiple of FF_R) overwrites the one entry it no longer needs
    const uint32_t base = H + FF_R * tid;
    T win[FF_R], acc[FF_R];
#pragma unroll
    for (int r = 0; r < FF_R; r++) { acc[r] = zero_of(T()); win[r] = s[sk(base + r)]; }
    uint32_t i0 = 0;
    for (; i0 + FF_R <= L; i0 += FF_R) {
#pragma unroll
        for (int u = 0; u < FF_R; u++) {
            const float hv = h[i0 + u];
            win[(FF_R - u) % FF_R] = s[sk(base - (i0 + u))];
#pragma unroll
            for (int r = 0; r < FF_R; r++) acc[r] = mac(acc[r], hv, win[(r + FF_R - u) % FF_R]);
        }
    }
#pragma unroll
    for (int u = 0; u < FF_R - 1; u++) {
        if (i0 + u < L) {
            const float hv = h[i0 + u];
            win[(FF_R - u) % FF_R] = s[sk(base - (i0 + u))];
#pragma unroll
            for (int r = 0; r < FF_R; r++) acc[r] = mac(acc[r], hv, win[(r + FF_R - u) % FF_R]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < FF_R; r++) s[sk(FF_R * tid + r)] = scaled(l.scale, acc[r]);
    __syncthreads();
    if (whole) {
        float4 *dst = reinterpret_cast<float4 *>(orow + T0);
#pragma unroll
        for (int i = 0; i < FF_TILE / PV / FF_T; i++) {
            const uint32_t e = tid + FF_T * i, k = e * PV;
            if constexpr (CPLX) {
                const float2 a = s[sk(k)], b = s[sk(k + 1)];
                dst[e] = make_float4(a.x, a.y, b.x, b.y);
            } else {
                dst[e] = make_float4(s[sk(k)], s[sk(k + 1)], s[sk(k + 2)], s[sk(k + 3)]);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < FF_R; i++) {
            const uint32_t e = tid + FF_T * i, t = T0 + e;
            if (t < n) orow[t] = s[sk(e)];
        }
    }
}

}  // namespace

int launch_firfilt(bool cplx, const void *x, void *y, const float *h, const void *hist_in, void *hist_out, const FirfiltLaunch &l,
                   hipStream_t s)
{
    if (!l.C || !l.n) return 0;
    const uint32_t tiles = (l.n + FF_TILE - 1) / FF_TILE;
    if ((uint64_t)tiles * l.C > 0x7fffffffull) { set_error("firfilt: %u x %u samples are more than one launch takes", l.C, l.n); return CSDR_ERR_SIZE; }
    const size_t el = cplx ? sizeof(float2) : sizeof(float);
    const uint32_t vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0 && ((size_t)l.n * el) % 16 == 0;
    const uint32_t slots = l.L - 1 + FF_TILE;
    const size_t lds = el * (slots + (slots >> 3) + 1);
    const dim3 grid(tiles * l.C);
    if (cplx) hipLaunchKernelGGL(k_firfilt<true>, grid, dim3(FF_T), lds, s, x, y, h, hist_in, hist_out, l, tiles, vec);
    else hipLaunchKernelGGL(k_firfilt<false>, grid, dim3(FF_T), lds, s, x, y, h, hist_in, hist_out, l, tiles, vec);
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr
