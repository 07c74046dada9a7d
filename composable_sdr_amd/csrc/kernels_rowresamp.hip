// rowResampler (liquid's resamp_crcf / resamp_rrrf on nchan rows, which the reference does not import; "csdr rowresamp v1",
// DESIGN.md 4.19): nchan independent rows, all CF32 or all F32, one rate r = 2^32 / delta and one clock for all of them.
//   k_rowresamp<CPLX> : 512 threads; a workgroup stages the filter bank in LDS once and walks a run of consecutive (row, tile)
//                       items (rowresamp_shape.h); a tile is TO = 1024 or 512 consecutive outputs of one row
//   k_rowresamp_hist  : the rows' next history alone, for a call that is too short to yield an output
// LDS of a workgroup (rrs_lds_bytes): the bank [P][265] float | the window [rrs_window_slots] of the sample type.
// The bank image is [j][column(b)] with an odd stride: the lanes of a wave sit on consecutive outputs, whose phases b advance by
// (delta >> 24) mod 256 and so are scattered; with tap j fixed and b varying they spread over the LDS banks, where the [b][j]
// image would put phases P floats apart; column(b) = b ^ (b >> 5) also spreads phase steps that are multiples of 32
// (rowresamp_shape.h).  Row 256 of the bank is row 0 one sample later, so b + 1 never wraps.
// A tile's input span, samples n_first - (P - 1) .. n_last of the row, goes into the linear window once, from the call or, in
// front of the call's first sample, from the row's history (zeros in front of the stream); a FIR read is one LDS read at
// window[n_k - base - j].  The workgroup that has tile 0 of a row writes that row's next history, the last P - 1 samples of
// (history | call), into the other side of the handle's pair.  No atomics, nothing waits for another workgroup.
// Arithmetic contract: f32, no contraction beyond the fmas named here.  With t_k = T + k delta, n_k = t_k >> 32,
// b = (t_k >> 24) & 255, mu = (t_k & 0xffffff) 2^-24 (exact):  s0 = s1 = +0; for j = 0, 1, .. P - 1 in this order:
// s0 = fma(bank[b][j], x[n_k - j], s0), s1 = fma(bank[b + 1][j], x[n_k - j], s1); y_k = fma(mu, s1, (1 - mu) s0), re and im apart.
// The order depends on P only; nothing depends on where an output falls in a tile, a run, a row count or a call: the output is
// bit-identical for every chunking of the stream and for a row alone against the same row among others.
#include "../../include/csdr.h"
#include "csdr_internal.h"
#include "rowresamp_shape.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

template <bool CPLX> struct RrType { typedef float2 T; };
template <> struct RrType<false> { typedef float T; };

template <class T> __device__ __forceinline__ T rr_zero();
template <> __device__ __forceinline__ float2 rr_zero<float2>() { return make_float2(0.f, 0.f); }
template <> __device__ __forceinline__ float rr_zero<float>() { return 0.f; }
__device__ __forceinline__ void rr_fma(float c, float2 v, float2 &s) { s.x = fmaf(c, v.x, s.x); s.y = fmaf(c, v.y, s.y); }
__device__ __forceinline__ void rr_fma(float c, float v, float &s) { s = fmaf(c, v, s); }
__device__ __forceinline__ float2 rr_mix(float mu, float a, float2 s0, float2 s1)
{
    return make_float2(fmaf(mu, s1.x, a * s0.x), fmaf(mu, s1.y, a * s0.y));
}
__device__ __forceinline__ float rr_mix(float mu, float a, float s0, float s1) { return fmaf(mu, s1, a * s0); }

// sample i of row `row` of the call, i in [-(P - 1), n): in front of the call the history, whose last entry is sample -1
template <class T>
__device__ __forceinline__ T rr_sample_at(const T *__restrict__ x, const T *__restrict__ hist, uint32_t row, int64_t i, uint32_t n, uint32_t H)
{
    return i >= 0 ? x[(size_t)row * n + (size_t)i] : hist[(size_t)row * H + (size_t)((int64_t)H + i)];
}

// the row's next history: the last H = P - 1 samples of (history | call); n >= 1
template <class T>
__device__ __forceinline__ void rr_write_hist(const T *__restrict__ x, const T *__restrict__ hist_in, T *__restrict__ hist_out, uint32_t row,
                                              uint32_t n, uint32_t H, uint32_t tid, uint32_t step)
{
    for (uint32_t j = tid; j < H; j += step)
        hist_out[(size_t)row * H + j] = rr_sample_at(x, hist_in, row, (int64_t)n - (int64_t)H + (int64_t)j, n, H);
}

template <bool CPLX>
__global__ __launch_bounds__(RRS_THREADS, 4) void k_rowresamp(const void *__restrict__ x_, void *__restrict__ y_,
                                                               const float *__restrict__ bank_t, const void *__restrict__ hist_in_,
                                                               void *__restrict__ hist_out_, RowResampLaunch l)
{
    typedef typename RrType<CPLX>::T T;
    const T *__restrict__ x = static_cast<const T *>(x_), *__restrict__ hist_in = static_cast<const T *>(hist_in_);
    T *__restrict__ y = static_cast<T *>(y_), *__restrict__ hist_out = static_cast<T *>(hist_out_);
    extern __shared__ float4 rr_lds4[];
    const uint32_t tid = threadIdx.x, P = rrs_P(l.delta, l.m), H = P - 1;
    float *bank = reinterpret_cast<float *>(rr_lds4);
    T *win = reinterpret_cast<T *>(bank + RRS_BANK_STRIDE * P);          // P is even: 8-byte aligned

    for (uint32_t e = tid; e < RRS_BANK_STRIDE * P; e += RRS_THREADS) bank[e] = bank_t[e];

    const uint32_t item0 = blockIdx.x * l.items_per_run;
    const uint32_t item1 = min(item0 + l.items_per_run, l.items);
    for (uint32_t item = item0; item < item1; item++) {
        const uint32_t row = item / l.tiles, tile = item - row * l.tiles;
        const RrsTile t = rrs_tile(l.T, l.delta, l.m, l.n_out, tile);
        __syncthreads();                                                  // the bank is staged; the window of the item before is read
        for (uint32_t s = tid; s < t.span; s += RRS_THREADS) win[s] = rr_sample_at(x, hist_in, row, t.base + (int64_t)s, l.n, H);
        if (tile == 0) rr_write_hist(x, hist_in, hist_out, row, l.n, H, tid, RRS_THREADS);
        __syncthreads();
        for (uint32_t o = tid; o < t.cnt; o += RRS_THREADS) {
            const uint64_t tk = rrs_time(l.T, l.delta, t.o0 + o);
            const uint32_t b = rrs_phase(tk);
            const float mu = (float)rrs_frac24(tk) * (1.0f / 16777216.0f);
            const T *wp = win + ((int64_t)rrs_sample(tk) - t.base);
            const float *bp0 = bank + rrs_bank_col(b), *bp1 = bank + rrs_bank_col(b + 1);
            T s0 = rr_zero<T>(), s1 = rr_zero<T>();
#pragma unroll 2
            for (uint32_t j = 0; j < P; j++) {
                const T v = wp[-(int)j];
                rr_fma(bp0[j * RRS_BANK_STRIDE], v, s0);
                rr_fma(bp1[j * RRS_BANK_STRIDE], v, s1);
            }
            y[(size_t)row * l.n_out + t.o0 + o] = rr_mix(mu, 1.0f - mu, s0, s1);
        }
    }
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_rowresamp_hist(const void *__restrict__ x_, const void *__restrict__ hist_in_,
                                                        void *__restrict__ hist_out_, uint32_t n, uint32_t H)
{
    typedef typename RrType<CPLX>::T T;
    rr_write_hist(static_cast<const T *>(x_), static_cast<const T *>(hist_in_), static_cast<T *>(hist_out_), blockIdx.x, n, H, threadIdx.x, 256u);
}

template <bool CPLX> hipError_t launch_one(const RrsShape &sh, hipStream_t s, const void *x, void *y, const float *bank_t, const void *hist_in,
                                           void *hist_out, const RowResampLaunch &l)
{
    if (sh.lds > 64 * 1024) {            // per device, so asked for at every such launch
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rowresamp<CPLX>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)RRS_LDS_LIMIT);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_rowresamp<CPLX>), dim3(sh.runs), dim3(RRS_THREADS), sh.lds, s, x, y, bank_t, hist_in, hist_out, l);
    return hipGetLastError();
}

}  // namespace

int launch_rowresamp(const void *x, void *y, const float *bank_t, const void *hist_in, void *hist_out, uint64_t delta, uint32_t m,
                     bool cplx, uint32_t nchan, uint32_t n, uint32_t n_out, uint64_t T, uint32_t cus, hipStream_t s)
{
    if (!n) return 0;
    if (!rrs_args_ok(delta, m) || !nchan || n_out != rrs_count(T, delta, n)) {
        set_error("rowresamp: delta = %llu, m = %u, %u rows, %u outputs of %u samples are not a launch shape", (unsigned long long)delta, m,
                  nchan, n_out, n);
        return CSDR_ERR_INVALID;
    }
    const uint32_t H = rrs_P(delta, m) - 1;
    if (!n_out) {
        if (cplx) hipLaunchKernelGGL((k_rowresamp_hist<true>), dim3(nchan), dim3(256), 0, s, x, hist_in, hist_out, n, H);
        else hipLaunchKernelGGL((k_rowresamp_hist<false>), dim3(nchan), dim3(256), 0, s, x, hist_in, hist_out, n, H);
        CSDR_HIP(hipGetLastError());
        return 0;
    }
    const RrsShape sh = rrs_shape(delta, m, cplx, n_out, nchan, cus, T);
    if (!sh.ok || sh.lds > RRS_LDS_LIMIT) {
        set_error("rowresamp: delta = %llu, m = %u need %zu bytes of LDS (limit %zu) or too many tiles", (unsigned long long)delta, m, sh.lds,
                  RRS_LDS_LIMIT);
        return CSDR_ERR_SIZE;
    }
    RowResampLaunch l;
    l.delta = delta; l.T = T; l.m = m; l.n = n; l.n_out = n_out; l.tiles = sh.tiles; l.items = sh.items; l.items_per_run = sh.items_per_run;
    CSDR_HIP(cplx ? launch_one<true>(sh, s, x, y, bank_t, hist_in, hist_out, l) : launch_one<false>(sh, s, x, y, bank_t, hist_in, hist_out, l));
    return 0;
}

}  // namespace csdr
