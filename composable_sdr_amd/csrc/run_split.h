// How a launch's tiles are split into runs, for every run kernel: the bounds of run w (host and device) -- run_range over a RunSplit
// (k_run256v2), run_range_even (k_pfb1024, k_front4096), run_range_halves (k_run64v2, k_run1024v2), run_range_blocks (k_run1024v3,
// k_shard1024) --, the host functions that size them (make_split, halves_n0) and the constants the bounds are judged against (tiles a run
// reads in front of itself, frames its dcfix kernel covers).  Included by the run kernels through fused_common.h, by kernel_choice.h and,
// on its own, by host-only programs (tests/test_run_split.py, tests/test_run_bounds_cpu.py): nothing here needs the HIP headers.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CSDR_SPLIT_HD __host__ __device__ __forceinline__
#else
#define CSDR_SPLIT_HD inline
#endif

namespace csdr {
namespace {

// Tiles (4096 samples) a run w >= 1 reads in front of its first tile: WU read-only warm-up tiles (DC state; none on a cold start) in front
// of HALO tiles it walks without output (window refill).  k_run1024v2 reads all WU + HALO without a clamp; the others clamp the warm-up.
constexpr int RUN64_WU = 6, RUN64_HALO = 1;             // k_run64v2
constexpr int RUN1024_WU = 6, RUN1024_HALO = 4;         // k_run1024v2, k_run1024v3, k_shard1024
// Output frames at a cold run's start that the dcfix kernel behind the launch corrects
constexpr int DCFIX_F = 113;                            // k_run256_dcfix: frame -1 of a run (freqdem history) + its first seven tiles of 16 frames
constexpr int RUN64_DCFIX_F = 448;                      // k_run64_dcfix: seven tiles of 64 frames (32 768 samples behind the halo tile's start)
// k_run1024_dcfix: frame -1 of a run (freqdem history) + its first eight tiles of 4 frames.  The first frame NOT corrected (32) has a
// window that reaches back to frame 35 behind the cold start: alpha |c| beta^35840 = 1.6e-8 alpha |c| of the missing state is left in it
// (with four tiles it was 5.9e-5: ~1e-5 of a unit signal at the strongest DC offset the tests use)
constexpr int RUN1024_DCFIX_F = 33;

// The plain floor split: run w of nruns gets the tiles [w nb / nruns, (w + 1) nb / nruns)
CSDR_SPLIT_HD void run_range_even(uint32_t nb, uint32_t nruns, uint32_t w, uint32_t &first, uint32_t &last)
{
    first = (uint32_t)((unsigned long long)w * nb / nruns);
    last = (uint32_t)((unsigned long long)(w + 1) * nb / nruns);
}

// Two workgroups per CU: the first half of the runs (the workgroups dispatched first, the older ones of their CUs) win the issue
// arbitration and share n0 of the nb tiles, the second half the rest (both halves then end together).  n0 = 0 or an odd nruns: even split
CSDR_SPLIT_HD void run_range_halves(uint32_t nb, uint32_t nruns, uint32_t n0, uint32_t w, uint32_t &first, uint32_t &last)
{
    if (n0 == 0 || (nruns & 1u)) return run_range_even(nb, nruns, w, first, last);
    const uint32_t half = nruns / 2, s = w / half, i = w - s * half;
    const uint32_t base = s ? n0 : 0u, tiles = s ? nb - n0 : n0;
    first = base + (uint32_t)((unsigned long long)i * tiles / half);
    last = base + (uint32_t)((unsigned long long)(i + 1) * tiles / half);
}
// n0 of run_range_halves.  weight: tile share of the older workgroup of a CU (1 = even; read between 1 and 1.5)
inline uint32_t halves_n0(uint32_t nb, uint32_t nruns, double weight)
{
    return (nruns >= 2 && !(nruns & 1u) && weight > 1.0 && weight < 1.5) ? (uint32_t)std::llround(0.5 * weight * (double)nb) : 0u;
}

// Whole blocks of TB tiles (a row's 128-byte output line), evenly; the call's last block may be a partial one (nb % TB tiles: its rows get
// the front part of a line)
CSDR_SPLIT_HD void run_range_blocks(uint32_t nb, uint32_t nruns, uint32_t w, uint32_t TB, uint32_t &first, uint32_t &last)
{
    const uint32_t nblk = (nb + TB - 1) / TB;
    first = TB * (uint32_t)((unsigned long long)w * nblk / nruns);
    last = TB * (uint32_t)((unsigned long long)(w + 1) * nblk / nruns);
    if (last > nb) last = nb;
}

// Runs are grouped in "slots": slot s holds rps consecutive runs that share tiles[s] tiles evenly, starting at tile base[s].
// One slot with rps = nruns is the plain balanced split; the run kernels use one slot per co-resident workgroup of a CU
// (blockIdx / #CUs) so that the share of a run can follow the issue priority its workgroup gets (oldest first) and all runs end together.
// shift = 1: a slot's runs share its tiles in whole PAIRS (every boundary inside the slot is base + an even number); the last run
// of a slot ends at the slot's end, so it also takes an odd last tile.  shift = 0: single tiles, the plain floor split.
struct RunSplit {
    uint32_t rps, nslots;
    uint32_t base[8], tiles[8];
    uint32_t shift;
};
CSDR_SPLIT_HD void run_range(const RunSplit &sp, uint32_t w, uint32_t &first, uint32_t &last)
{
    const uint32_t s = w / sp.rps, i = w - s * sp.rps, n = sp.tiles[s] >> sp.shift;
    first = sp.base[s] + ((uint32_t)((unsigned long long)i * n / sp.rps) << sp.shift);
    last = sp.base[s] + (i + 1 == sp.rps ? sp.tiles[s] : ((uint32_t)((unsigned long long)(i + 1) * n / sp.rps) << sp.shift));
}

// Split nb tiles into nruns runs, run w + 1 behind run w, every run >= 8 tiles.
// Weighted path -- one run per resident workgroup slot, nruns = slots x cus, 2 <= slots <= 8: a CU holds the runs c, c + cus, c + 2 cus, ...
// (class 0 = its oldest workgroup), and what decides when the launch ends is the CU with the most tiles.  So the split is made of whole tile
// pairs with the same total on every CU: q = (nb / 2) / cus pairs per CU, class k gets p_k pairs per run, sum p_k = q, the p_k chosen
// from weight[] by largest remainder (or given outright in pairs[], a diagnostics override; ignored unless it sums to q).  What does
// not divide -- (nb / 2) % cus pairs -- goes to the runs of the middle class (slots - 1) / 2, one pair each to some of them; an odd
// last tile goes to the launch's last run, the only place where it leaves every run start even (run w + 1 starts where run w ends).
// Every other run of class k has exactly 2 p_k tiles.  Fallback -- any other nruns, or a class below 8 tiles: the uniform floor split.
inline RunSplit make_split(uint32_t nb, uint32_t nruns, uint32_t cus, const float *weight, const uint32_t *pairs = nullptr)
{
    RunSplit sp{};
    const uint32_t slots = (cus && nruns && nruns % cus == 0) ? nruns / cus : 0;
    while (slots >= 2 && slots <= 8) {                  // (one pass: `break` = fall back)
        const uint32_t P = nb / 2, q = P / cus, rem = P % cus, mid = (slots - 1) / 2;
        uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sum = 0;
        if (pairs) for (uint32_t k = 0; k < slots; k++) { p[k] = pairs[k]; sum += p[k]; }
        if (!pairs || sum != q) {
            double tot = 0, frac[8];
            bool ok = true;
            for (uint32_t k = 0; k < slots; k++) { if (!(weight[k] > 0.f) || !std::isfinite(weight[k])) ok = false; tot += weight[k]; }
            if (!ok) break;
            sum = 0;
            for (uint32_t k = 0; k < slots; k++) {
                const double ideal = (double)q * weight[k] / tot;
                p[k] = (uint32_t)ideal; frac[k] = ideal - p[k]; sum += p[k];
            }
            for (; sum < q; sum++) {                    // largest remainder first, the older class on a tie
                uint32_t best = 0;
                for (uint32_t k = 1; k < slots; k++) if (frac[k] > frac[best]) best = k;
                p[best]++; frac[best] = -1.0;
            }
        }
        bool ok = sum == q;
        for (uint32_t k = 0; k < slots; k++) if (p[k] < 4) ok = false;      // 8 tiles
        if (!ok) break;
        sp.rps = cus; sp.nslots = slots; sp.shift = 1;
        uint32_t base = 0;
        for (uint32_t k = 0; k < slots; k++) {
            sp.base[k] = base;
            sp.tiles[k] = 2 * (p[k] * cus + (k == mid ? rem : 0)) + (k + 1 == slots ? (nb & 1) : 0);
            base += sp.tiles[k];
        }
        return sp;
    }
    sp = RunSplit{};
    sp.rps = nruns ? nruns : 1; sp.nslots = 1; sp.base[0] = 0; sp.tiles[0] = nb;
    return sp;
}

}  // namespace
}  // namespace csdr
