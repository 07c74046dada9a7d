// firpfbch2Channelizer (liquid's firpfbch2_crcf analyzer, which the reference does not import): a 2x-oversampled
// polyphase channelizer.  M channels (a power of two, 4 .. 256), a real prototype h[0 .. L - 1], L = 2 m M; every M / 2 input
// samples give one frame of M outputs, written channel-major y[k][t].
//   k_pfb2<2 m, log2 M> : 512 threads; a workgroup walks a run of consecutive tiles of F = 4096 / M frames (pfb2_shape.h)
//                         FIR + rotation + DFT + transpose in one launch, nothing in between goes through HBM
// LDS of a workgroup (pfb2_lds_bytes): the sample window | V [F][row stride] | the twiddles [M / 4].  The window holds the H = L - M/2
// samples in front of a tile and the tile's F M/2 = 2048 new ones.  A run fills it once, from the input or (before the call's first
// sample) from the handle's history; behind a tile's FIR its last H samples move to the front and the next tile's 2048 samples, fetched
// into registers ahead of the FIR, follow them: the FIR window stays in LDS for the whole run and the halo is read from HBM once per
// run.  The window is linear, so a FIR read is one ds_read at a constant offset from the item's base.  Thread tid owns branch
// i = tid mod M for every frame it meets and keeps that branch's 2 m taps in registers, loaded once per workgroup (an LDS copy of the
// taps would cost the second workgroup per CU at M = 256 and buy nothing: no other lane of a wave wants the same tap).  The DFT runs
// in place in V, two radix-2 decimation-in-frequency stages per pass (one single stage last when log2 M is odd), so that bin k ends
// at slot bitrev(k).  The FIR writes V along a frame; the DFT passes and the store pass put their lanes on consecutive frames (the
// row stride, M + 1 or M + 2, keeps a half-wave on different banks; a butterfly's twiddles are the same for all of them), and the
// store pass writes F consecutive frames of a row, F >= 16: whole 128-byte pieces, the last tile of a call masked.
// Arithmetic contract: f32, no contraction beyond the fmas named here.  v_t[i] = sum_n h[i + n M] x[n_t - i - n M],
// n_t = (t + 1) M / 2 - 1, by fma from acc = +0, oldest sample first (n = 2 m - 1 down to 0), re and im separately.
// u[(i + (t mod 2) M / 2) mod M] = v_t[i] (the rotation, an index shift).  Y = the backward DFT of u: radix-2 butterflies a + c,
// (a - c) w with w = e^{+2 pi j p / N} from one table of M / 4 twiddles (f64 on the host, rounded once; the second quarter is j
// times the first); a complex product is g_cmul of fft16_generic.h: re = fma(ai, -wi, ar wr), im = fma(ai, wr, ar wi).  The order
// of operations depends on M only.  y = Y / M, exact.  t counts frames from the start of the stream (the handle carries its
// parity).  Nothing depends on where a frame falls in a tile, a run or a call: the output is bit-identical for every chunking.
#include "../../include/csdr.h"
#include "csdr_internal.h"
#include "fft16_generic.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr int P2_T = PFB2_THREADS;
constexpr int P2_PRE = 4;                // float2 registers of a thread for the next tile's samples: F M/2 = 2048 = 4 x 512

typedef v2fg c32;                         // one CF32 sample in a register pair: the adds, products and fmas below are packed
__device__ __forceinline__ c32 mulj(c32 a) { return (c32){-a.y, a.x}; }

// sample s of the call (s < 0: the history, whose last element is sample -1)
__device__ __forceinline__ c32 sample_at(const c32 *__restrict__ x, const c32 *__restrict__ hist, int64_t s, uint32_t H)
{
    return s >= 0 ? x[s] : hist[(int64_t)H + s];
}

template <int TM, int LOGM>
__global__ __launch_bounds__(P2_T, 4) void k_pfb2(const float2 *__restrict__ x_, float2 *__restrict__ y_, const float *__restrict__ h,
                                                  const float2 *__restrict__ tw_, const float2 *__restrict__ hist_in_,
                                                  float2 *__restrict__ hist_out_, Pfb2Launch l)
{
    const c32 *__restrict__ x = reinterpret_cast<const c32 *>(x_), *__restrict__ tw = reinterpret_cast<const c32 *>(tw_);
    const c32 *__restrict__ hist_in = reinterpret_cast<const c32 *>(hist_in_);
    c32 *__restrict__ y = reinterpret_cast<c32 *>(y_), *__restrict__ hist_out = reinterpret_cast<c32 *>(hist_out_);
    extern __shared__ float4 lds4[];
    constexpr uint32_t M = 1u << LOGM, P = M >> 1, L = TM * M, H = L - P, LOGF = 12 - LOGM, F = 1u << LOGF, FP = F * P;
    constexpr uint32_t VS = pfb2_row_stride(M), Q = M >> 2;   // Q twiddles in the table; e^{2 pi j (k + Q) / M} = j e^{2 pi j k / M}
    constexpr int KEEP = (H + P2_T - 1) / P2_T, ITEMS = (F * M) / P2_T;
    static_assert(F == pfb2_tile_frames(M) && FP == P2_PRE * P2_T && H + FP == pfb2_window_slots(M, TM / 2) && P2_T % M == 0, "pfb2_shape.h");
    const uint32_t tid = threadIdx.x, frames = l.frames;
    c32 *win = reinterpret_cast<c32 *>(lds4);
    c32 *V = win + H + FP;
    c32 *twl = V + F * VS;

    for (uint32_t k = tid; k < Q; k += P2_T) twl[k] = tw[k];
    // the stream's next history: the last H samples of (history | call); the call is not empty
    if (blockIdx.x == 0) {
        const int64_t n = (int64_t)frames * P;
        for (uint32_t k = tid; k < H; k += P2_T) hist_out[k] = sample_at(x, hist_in, n - H + k, H);
    }
    const uint32_t tile0 = blockIdx.x * l.tiles_per_run;
    const uint32_t tile1 = min(tile0 + l.tiles_per_run, l.tiles);
    // window slot k holds sample f0 P - H + k of the call: H samples in front of the tile, then the tile's own
    {
        const int64_t s0 = (int64_t)tile0 * FP - H;
        const uint32_t cnt = H + min(F, frames - tile0 * F) * P;
        for (uint32_t k = tid; k < cnt; k += P2_T) win[k] = sample_at(x, hist_in, s0 + k, H);
    }
    const uint32_t i = tid & (M - 1);
    float hreg[TM];
#pragma unroll
    for (int n = 0; n < TM; n++) hreg[n] = h[i + n * M];
    const float inv_m = 1.0f / (float)M;
    __syncthreads();

    for (uint32_t tile = tile0; tile < tile1; tile++) {
        const uint32_t f0 = tile * F, nf = min(F, frames - f0);
        const bool more = tile + 1 < tile1;
        // the next tile's samples, into registers
        c32 pre[P2_PRE];
        uint32_t ncnt = 0;
        if (more) {
            ncnt = min(F, frames - (f0 + F)) * P;
            const c32 *src = x + (size_t)(f0 + F) * P;
#pragma unroll
            for (int r = 0; r < P2_PRE; r++) {
                const uint32_t e = tid + P2_T * r;
                if (e < ncnt) pre[r] = src[e];
            }
        }
        // FIR: item e = (frame fl, branch i).  The frame's newest sample is slot H + (fl + 1) P - 1, tap n meets the slot i + n M
        // below it; p points at the oldest, (2 m - 1) M further down (H - (2 m - 1) M = P)
#pragma unroll 2
        for (int r = 0; r < ITEMS; r++) {
            const uint32_t fl = (tid + P2_T * r) >> LOGM;
            if (fl < nf) {
                const c32 *p = win + ((fl + 2) * P - 1 - i);
                c32 acc = {0.f, 0.f};
#pragma unroll
                for (int n = TM - 1; n >= 0; n--) acc = __builtin_elementwise_fma((c32){hreg[n], hreg[n]}, p[(TM - 1 - n) * M], acc);
                const uint32_t par = (l.par0 + f0 + fl) & 1u;
                V[fl * VS + ((i + par * P) & (M - 1))] = acc;
            }
        }
        __syncthreads();
        // every read of the window is done: its last H samples move to the front, the next tile's samples follow them
        if (more) {
            c32 keep[KEEP];
#pragma unroll
            for (int r = 0; r < KEEP; r++) {
                const uint32_t k = tid + P2_T * r;
                if (k < H) keep[r] = win[FP + k];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < KEEP; r++) {
                const uint32_t k = tid + P2_T * r;
                if (k < H) win[k] = keep[r];
            }
#pragma unroll
            for (int r = 0; r < P2_PRE; r++) {
                const uint32_t e = tid + P2_T * r;
                if (e < ncnt) win[H + e] = pre[r];
            }
        }
        // backward DFT of every frame, in place: block length N, two stages per pass
#pragma unroll
        for (int logN = LOGM; logN >= 2; logN -= 2) {
            const uint32_t N = 1u << logN, q = N >> 2, logq = logN - 2, sh = LOGM - logN;
#pragma unroll 1
            for (int r = 0; r < (int)((F * Q + P2_T - 1) / P2_T); r++) {
                const uint32_t e = tid + P2_T * r;          // lanes run over the frames: the row stride keeps them on different banks
                const uint32_t fl = e & (F - 1), b = e >> LOGF, pos = b & (q - 1), blk = b >> logq;
                c32 *v = V + fl * VS + blk * N + pos;
                const c32 a0 = v[0], a1 = v[q], a2 = v[2 * q], a3 = v[3 * q];
                const uint32_t i2 = (2 * pos) << sh;
                const c32 w1 = twl[pos << sh], w2 = i2 < Q ? twl[i2] : mulj(twl[i2 - Q]);
                const c32 c0 = a0 + a2, c2 = g_cmul(a0 - a2, w1);
                const c32 c1 = a1 + a3, c3 = g_cmul(mulj(a1 - a3), w1);
                v[0] = c0 + c1; v[q] = g_cmul(c0 - c1, w2);
                v[2 * q] = c2 + c3; v[3 * q] = g_cmul(c2 - c3, w2);
            }
            __syncthreads();
        }
        if (LOGM & 1) {
#pragma unroll
            for (int r = 0; r < (int)((F * P) / P2_T); r++) {
                const uint32_t e = tid + P2_T * r, fl = e & (F - 1), b = e >> LOGF;
                c32 *v = V + fl * VS + 2 * b;
                const c32 a = v[0], c = v[1];
                v[0] = a + c; v[1] = a - c;
            }
            __syncthreads();
        }
        // rows: F consecutive frames of channel k, from slot bitrev(k) of every frame
#pragma unroll
        for (int r = 0; r < ITEMS; r++) {
            const uint32_t e = tid + P2_T * r, fl = e & (F - 1), g = e >> LOGF;
            // 16 frames per row piece: the two rows of a half-wave are k and k + M / 2, one slot apart in V
            const uint32_t k = F >= 32 ? g : ((g & 1u) << (LOGM - 1)) | (g >> 1);
            if (fl < nf) {
                y[(size_t)k * frames + f0 + fl] = V[fl * VS + (__brev(k) >> (32 - LOGM))] * inv_m;
            }
        }
        __syncthreads();
    }
}

using LaunchFn = hipError_t (*)(dim3, size_t, hipStream_t, const float2 *, float2 *, const float *, const float2 *, const float2 *, float2 *,
                                const Pfb2Launch &);
template <int TM, int LOGM>
hipError_t launch_one(dim3 grid, size_t lds, hipStream_t s, const float2 *x, float2 *y, const float *h, const float2 *tw,
                      const float2 *hist_in, float2 *hist_out, const Pfb2Launch &l)
{
    if (lds > 64 * 1024) {           // per device, so asked for at every such launch
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pfb2<TM, LOGM>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)PFB2_LDS_LIMIT);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_pfb2<TM, LOGM>), grid, dim3(P2_T), lds, s, x, y, h, tw, hist_in, hist_out, l);
    return hipGetLastError();
}
template <int LOGM> LaunchFn by_semi(uint32_t m)
{
    switch (m) {
    case 1: return launch_one<2, LOGM>;   case 2: return launch_one<4, LOGM>;   case 3: return launch_one<6, LOGM>;
    case 4: return launch_one<8, LOGM>;   case 5: return launch_one<10, LOGM>;  case 6: return launch_one<12, LOGM>;
    case 7: return launch_one<14, LOGM>;  case 8: return launch_one<16, LOGM>;
    }
    return nullptr;
}
LaunchFn by_shape(uint32_t M, uint32_t m)
{
    switch (M) {
    case 4: return by_semi<2>(m);    case 8: return by_semi<3>(m);    case 16: return by_semi<4>(m);   case 32: return by_semi<5>(m);
    case 64: return by_semi<6>(m);   case 128: return by_semi<7>(m);  case 256: return by_semi<8>(m);
    }
    return nullptr;
}

}  // namespace

std::vector<float2> pfb2_twiddles(uint32_t M)
{
    std::vector<float2> w(M / 4);
    for (uint32_t k = 0; k < M / 4; k++) {
        const double a = 2.0 * 3.14159265358979323846 * (double)k / (double)M;
        w[k] = make_float2((float)__builtin_cos(a), (float)__builtin_sin(a));
    }
    return w;
}

int launch_pfb2(const float2 *x, float2 *y, const float *h, const float2 *tw, const float2 *hist_in, float2 *hist_out, uint32_t M,
                uint32_t m, uint32_t frames, uint32_t parity, uint32_t cus, hipStream_t s)
{
    if (!frames) return 0;
    if (!pfb2_args_ok(M, m)) { set_error("pfbch2: M = %u, m = %u are not a launch shape", M, m); return CSDR_ERR_INVALID; }
    const Pfb2Shape sh = pfb2_shape(M, m, frames, cus);
    if (sh.lds > PFB2_LDS_LIMIT) {
        set_error("pfbch2: M = %u, m = %u need %zu bytes of LDS (limit %zu)", M, m, sh.lds, PFB2_LDS_LIMIT);
        return CSDR_ERR_SIZE;
    }
    const LaunchFn launch = by_shape(M, m);
    if (!launch) { set_error("pfbch2: no kernel for M = %u, m = %u", M, m); return CSDR_ERR_INVALID; }
    Pfb2Launch l;
    l.frames = frames; l.par0 = parity & 1u; l.tiles = sh.tiles; l.tiles_per_run = sh.tiles_per_run;
    CSDR_HIP(launch(dim3(sh.runs), sh.lds, s, x, y, h, tw, hist_in, hist_out, l));
    return 0;
}

}  // namespace csdr
