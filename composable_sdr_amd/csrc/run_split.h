// How a launch's tiles are split into runs: RunSplit, run_range (host and device) and make_split (host).  Included by the run kernels
// through fused_common.h and, on its own, by host-only programs (tests/test_run_split.py): nothing here needs the HIP headers.
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
