// fskDemodulator m k bw (Liquid.chs:336-382): liquid's fskdem on C independent CF32 streams.
//   k_fskdem : one symbol of k samples per thread, 256 consecutive symbols of one row per workgroup     no state, no recurrence
// A symbol is the k samples zero-padded to K, and only the M mapped bins of its K-point forward DFT are wanted, so each is
// taken directly: X[b] = sum_j x[j] W[(b j) mod K] with W[t] = e^{-2 pi i t / K} from a table built at create.  The rows are
// staged through LDS in blocks of up to 16 samples per symbol (coalesced 16-byte loads where the alignment allows), the table
// sits behind them in LDS, and a thread reads its x[j] once for up to 16 tones; the table index t advances by the tone's bin
// and wraps at K.  It is the same for every lane, so the table read is a broadcast.
// Arithmetic contract: plain f32, no contraction.  Per tone the sum starts at +0 and takes j = 0 .. k - 1 in that order,
// whatever the call size, the stream count, the grid or the energy output; a complex product is four multiplies, one
// subtraction and one addition; the magnitude is sqrtf(re re + im im), correctly rounded; the symbol is the first tone with the
// largest magnitude (s == 0 || v > vmax, as liquid has it).  tests/fsk_restatement.py restates it exactly.
#include "../../include/csdr.h"
#include "csdr_internal.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace csdr {

namespace {

constexpr int FS = 256;     // symbols per workgroup, one thread each
constexpr int FJ = 16;      // samples of every symbol per LDS block
constexpr int FT = 16;      // tones per pass over the samples (two accumulator registers each)

// TG tones per pass (M for M < 16); U samples per global load (2: 16-byte loads); WL: the table fits in LDS
// LDS: xs[FS][JB | 1] float2 (JB = min(k, FJ); the odd row stride keeps the lanes' 8-byte reads on different banks) | W[K]
template <int TG, int U, bool WL>
__global__ __launch_bounds__(FS) void k_fskdem(const float2 *__restrict__ X, uint32_t *__restrict__ SYM, float *__restrict__ E,
                                               const float2 *__restrict__ gW, const uint32_t *__restrict__ gmap, FskdemLaunch l,
                                               uint32_t ns, uint32_t tiles)
{
    extern __shared__ float4 lds4[];
    using V = typename std::conditional<U == 2, float4, float2>::type;
    constexpr int NQ = FJ / U;
    const uint32_t k = l.k, K = l.K, M = l.M, tid = threadIdx.x;
    const uint32_t JB = k < (uint32_t)FJ ? k : (uint32_t)FJ, ST = JB | 1u, PER = JB / U;
    float2 *xs = reinterpret_cast<float2 *>(lds4), *sW = xs + FS * ST;
    const uint32_t c = blockIdx.x / tiles, S0 = (blockIdx.x - c * tiles) * FS, nv = min((uint32_t)FS, ns - S0);
    const size_t row0 = (size_t)c * l.n;
    if (WL) for (uint32_t i = tid; i < K; i += FS) sW[i] = gW[i];
    auto tab = [&](uint32_t t) -> float2 { if constexpr (WL) return sW[t]; else return gW[t]; };
    // element e = tid + FS i of a block: symbol e / PER, samples (e % PER) U .. + U of the block's JB
    V q[NQ];
    auto load = [&](uint32_t jb) {
        const uint32_t j0 = jb * JB, steps = min(JB, k - j0);
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            if ((uint32_t)i < PER) {
                const uint32_t e = tid + FS * i, sy = e / PER, pc = (e - sy * PER) * U;
                const bool ok = sy < nv && pc < steps;                 // otherwise: the plane's first samples, never used
                const size_t idx = ok ? row0 + (size_t)(S0 + sy) * k + j0 + pc : 0;
                q[i] = *reinterpret_cast<const V *>(X + idx);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            if ((uint32_t)i < PER) {
                const uint32_t e = tid + FS * i, sy = e / PER, pc = (e - sy * PER) * U;
                float2 *d = xs + sy * ST + pc;
                if constexpr (U == 2) { d[0] = make_float2(q[i].x, q[i].y); d[1] = make_float2(q[i].z, q[i].w); }
                else d[0] = q[i];
            }
        }
    };
    const float2 *row = xs + tid * ST;
    const bool act = tid < nv;
    const size_t so = (size_t)c * ns + S0 + tid;                       // this thread's symbol
    float ar[TG], ai[TG];
    uint32_t t[TG], b[TG];
    float vmax = 0.f;
    uint32_t best = 0;
    const uint32_t nblk = (k + JB - 1) / JB, nit = nblk * (M / TG);
    uint32_t jb = 0, g = 0;
    load(0);
    for (uint32_t it = 0; it < nit; it++) {
        __syncthreads();
        stage();
        __syncthreads();
        const uint32_t jbn = jb + 1 == nblk ? 0 : jb + 1;
        if (it + 1 < nit) load(jbn);                                   // in flight while this block is summed
        if (jb == 0) {
#pragma unroll
            for (int i = 0; i < TG; i++) { ar[i] = 0.f; ai[i] = 0.f; t[i] = 0; b[i] = gmap[g * TG + i]; }
        }
        const uint32_t steps = min(JB, k - jb * JB);
        for (uint32_t j = 0; j < steps; j++) {
            const float2 x = row[j];
#pragma unroll
            for (int i = 0; i < TG; i++) {
                const float2 w = tab(t[i]);
                const float pr = x.x * w.x - x.y * w.y;
                const float pi = x.x * w.y + x.y * w.x;
                ar[i] = ar[i] + pr;
                ai[i] = ai[i] + pi;
                t[i] += b[i];
                if (t[i] >= K) t[i] -= K;
            }
        }
        if (jb + 1 == nblk) {
            float ev[TG];
#pragma unroll
            for (int i = 0; i < TG; i++) {
                const float v = sqrtf(ar[i] * ar[i] + ai[i] * ai[i]);
                const uint32_t s = g * TG + i;
                if (s == 0 || v > vmax) { vmax = v; best = s; }
                ev[i] = v;
            }
            if (E && act) {
                float *e = E + so * M + g * TG;
#pragma unroll
                for (int i = 0; i < TG; i++) e[i] = ev[i];
            }
            g++;
        }
        jb = jbn;
    }
    if (act) SYM[so] = best;
}

template <int TG>
void launch_tg(bool vec, bool wl, dim3 grid, size_t lds, hipStream_t s, const float2 *x, uint32_t *sym, float *energy,
               const float2 *W, const uint32_t *map, const FskdemLaunch &l, uint32_t ns, uint32_t tiles)
{
    if (vec && wl) hipLaunchKernelGGL((k_fskdem<TG, 2, true>), grid, dim3(FS), lds, s, x, sym, energy, W, map, l, ns, tiles);
    else if (vec) hipLaunchKernelGGL((k_fskdem<TG, 2, false>), grid, dim3(FS), lds, s, x, sym, energy, W, map, l, ns, tiles);
    else if (wl) hipLaunchKernelGGL((k_fskdem<TG, 1, true>), grid, dim3(FS), lds, s, x, sym, energy, W, map, l, ns, tiles);
    else hipLaunchKernelGGL((k_fskdem<TG, 1, false>), grid, dim3(FS), lds, s, x, sym, energy, W, map, l, ns, tiles);
}

}  // namespace

int launch_fskdem(const float2 *x, uint32_t *sym, float *energy, const float2 *W, const uint32_t *map, const FskdemLaunch &l,
                  hipStream_t s)
{
    const uint32_t ns = l.n / l.k;
    if (!l.C || !ns) return 0;
    const uint32_t tiles = (ns + FS - 1) / FS;
    if ((uint64_t)tiles * l.C > 0x7fffffffull) { set_error("fskdem: %u x %u symbols are more than one launch takes", l.C, ns); return CSDR_ERR_SIZE; }
    // 16-byte loads: every symbol of every row has to start on an even sample of an aligned plane
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15u) == 0 && l.n % 2 == 0 && l.k % 2 == 0;
    const uint32_t JB = l.k < (uint32_t)FJ ? l.k : (uint32_t)FJ;
    const size_t tile_bytes = sizeof(float2) * FS * (JB | 1u), tab_bytes = sizeof(float2) * l.K;
    const bool wl = tile_bytes + tab_bytes <= 64 * 1024;               // a longer table is read from global memory (cached)
    const size_t lds = tile_bytes + (wl ? tab_bytes : 0);
    const dim3 grid(tiles * l.C);
    switch (l.M < (uint32_t)FT ? l.M : (uint32_t)FT) {
    case 2: launch_tg<2>(vec, wl, grid, lds, s, x, sym, energy, W, map, l, ns, tiles); break;
    case 4: launch_tg<4>(vec, wl, grid, lds, s, x, sym, energy, W, map, l, ns, tiles); break;
    case 8: launch_tg<8>(vec, wl, grid, lds, s, x, sym, energy, W, map, l, ns, tiles); break;
    default: launch_tg<FT>(vec, wl, grid, lds, s, x, sym, energy, W, map, l, ns, tiles); break;
    }
    CSDR_HIP(hipGetLastError());
    return 0;
}

}  // namespace csdr
