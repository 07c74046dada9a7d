// gmskDemodulator m k bw (Liquid.chs:384-429): liquid's gmskdem on C independent CF32 streams.
//   k_gmskdem : one symbol per thread, S = 256 (k <= 32) or 128 consecutive symbols of one row per workgroup     direct form, no recurrence
// phi[t] = arg(conj(x[t - 1]) x[t]) (fm_sample_rn, the library's one freqdem sample) is computed once per sample of the tile and
// once more for the L - 1 = 2 k m samples in front of it (from the row, or from the history buffer at the row's start), and kept
// in LDS.  Symbol s is d[s] = sum_i r[i] phi[s k - i]: the lanes of a wave read phi k floats apart, so phi is stored
// de-interleaved by sample phase: local position p = q k + ph (p = 0 is phi[S0 k - 2 k m]) sits at ph Q + q with Q odd.  At tap i
// every lane has the same phase and consecutive q, so the reads of a wave fall on consecutive banks for every k.  The tap index
// is the same for every lane, so the taps come through scalar loads.  The samples are loaded in pairs (16-byte loads where the
// plane's alignment allows); the sample in front of a pair comes from the neighbouring lane.  The first workgroup of a row
// also writes the row's next history (the last L samples of history | row) into the other half of a ping-pong pair.
// Arithmetic contract: phi as fm_sample_rn(x[t - 1], x[t], 1.0f) gives it; then plain f32, no contraction: acc = +0; for
// i = 0 .. L - 1 in that order acc = acc + r[i] * phi[s k - i], the product rounded, then the sum; sym = acc > 0.  Nothing in
// it depends on the call size, where a stream is cut, the row count or the grid.  tests/gmsk_restatement.py restates it in f64.
#include "../../include/csdr.h"
#include "csdr_internal.h"
#include "fm_common.h"

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr uint32_t GM_S_SMALL = 256, GM_S_LARGE = 128;      // symbols (= threads) per workgroup for k <= 32 and for k > 32
constexpr uint32_t GM_K_SMALL = 32;

// vec: X and every row start are 16-byte aligned (set by the launcher); blockDim.x = S
__global__ __launch_bounds__(GM_S_SMALL) void k_gmskdem(const float2 *__restrict__ X, uint32_t *__restrict__ SYM, float *__restrict__ SOFT,
                                                        const float *__restrict__ h, const float2 *__restrict__ hist_in,
                                                        float2 *__restrict__ hist_out, GmskdemLaunch l, uint32_t ns, uint32_t tiles,
                                                        uint32_t vec)
{
    extern __shared__ float4 lds4[];
    float *ph = reinterpret_cast<float *>(lds4);
    const uint32_t k = l.k, m2 = 2 * l.m, L = l.L, H = L - 1, n = l.n, tid = threadIdx.x, S = blockDim.x;
    const uint32_t Q = (S + m2) | 1u;                                    // rows of k phases; q <= S - 1 + 2 m
    const uint32_t c = blockIdx.x / tiles, S0 = (blockIdx.x - c * tiles) * S, nv = min(S, ns - S0);
    const float2 *row = X + (size_t)c * n, *hin = hist_in + (size_t)c * L;
    const int64_t t0 = (int64_t)S0 * k;                                  // the first sample of the tile's first symbol
    auto xat = [&](int64_t t) -> float2 { return t >= 0 ? row[t] : hin[(int64_t)L + t]; };   // t >= -L
    auto put = [&](uint32_t p, float v) {                                // p < (S - 1) k + L
        const uint32_t q = __umulhi(p, l.kinv);                          // p / k: exact for p k < 2^32
        ph[(p - q * k) * Q + q] = v;
    };

    // the 2 k m samples in front of the tile: phi[t0 - H + p], p < H
    for (uint32_t p = tid; p < H; p += S) {
        const int64_t t = t0 - H + p;
        put(p, fm_sample_rn(xat(t - 1), xat(t), 1.0f));
    }
    // the tile: phi[t0 + u], u < nb, two per thread and step; the last symbol needs its first sample only
    const uint32_t nb = (nv - 1) * k + 1, npairs = (nb + 1) / 2;
    for (uint32_t j0 = 0; j0 < npairs; j0 += S) {
        const uint32_t j = j0 + tid, jj = min(j, npairs - 1);            // lanes past the end repeat the last pair and store nothing
        const int64_t t = t0 + 2 * jj;                                   // t + 1 <= (S0 + nv - 1) k + 1 < n
        float2 a, b, pv;
        if (vec) {
            const float4 q = *reinterpret_cast<const float4 *>(row + t);
            a = make_float2(q.x, q.y); b = make_float2(q.z, q.w);
            pv.x = __shfl_up(b.x, 1); pv.y = __shfl_up(b.y, 1);          // whole waves get here: S and the step are multiples of 64
            if ((tid & 63u) == 0) pv = xat(t - 1);
        } else {
            a = row[t]; b = row[t + 1]; pv = xat(t - 1);
        }
        const float f0 = fm_sample_rn(pv, a, 1.0f), f1 = fm_sample_rn(a, b, 1.0f);
        if (j < npairs) {
            put(H + 2 * j, f0);
            if (2 * j + 1 < nb) put(H + 2 * j + 1, f1);
        }
    }
    // the row's next history: the last L samples of (history | row), also when n < L
    if (S0 == 0) {
        float2 *hout = hist_out + (size_t)c * L;
        for (uint32_t i = tid; i < L; i += S) hout[i] = xat((int64_t)n - L + i);
    }
    __syncthreads();

    // symbol tid of the tile at tap i meets position tid k + (H - i): phase (H - i) mod k, row tid + (H - i) / k
    if (tid < nv) {
        const float *base = ph + tid;
        float acc = 0.f;
        { const float p = h[0] * base[m2]; acc = acc + p; }
        uint32_t i = 1;
        for (int qo = (int)m2 - 1; qo >= 0; qo--) {
            for (int r = (int)k - 1; r >= 0; r--, i++) {
                const float p = h[i] * base[(uint32_t)r * Q + (uint32_t)qo];
                acc = acc + p;
            }
        }
        const size_t so = (size_t)c * ns + S0 + tid;
        SYM[so] = acc > 0.f ? 1u : 0u;
        if (SOFT) SOFT[so] = acc;
    }
}

}  // namespace

int launch_gmskdem(const float2 *x, uint32_t *sym, float *soft, const float *h, const float2 *hist_in, float2 *hist_out,
                   const GmskdemLaunch &l, hipStream_t s)
{
    const uint32_t ns = l.n / l.k;
    if (!l.C || !ns) return 0;
    const uint32_t S = l.k <= GM_K_SMALL ? GM_S_SMALL : GM_S_LARGE, tiles = (ns + S - 1) / S;
    if ((uint64_t)tiles * l.C > 0x7fffffffull) { set_error("gmskdem: %u x %u symbols are more than one launch takes", l.C, ns); return CSDR_ERR_SIZE; }
    const uint32_t vec = (reinterpret_cast<uintptr_t>(x) & 15u) == 0 && l.n % 2 == 0;
    const size_t lds = sizeof(float) * l.k * ((S + 2 * l.m) | 1u);      // at most 64 x 145 or 32 x 273 floats
    hipLaunchKernelGGL(k_gmskdem, dim3(tiles * l.C), dim3(S), lds, s, x, sym, soft, h, hist_in, hist_out, l, ns, tiles, vec);
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr
