// Which kernel a chain call of nf frames takes, and with how many runs: KernelChoice, the run counts of the run kernels, whether their
// runs start cold, and the selection of the M = 64 and M = 1024 plans.  Pure functions of the configuration, the knobs the plan read when
// it was made, the CU count and nf.  Included by the plans through fused.h and, on its own, by host-only programs
// (tests/test_kernel_choice.py, tests/test_run_bounds_cpu.py): nothing here needs the HIP headers.
#pragma once

#include "run_split.h"
#include <cstdint>

namespace csdr {

// The kernel a call takes: an id of the plan's own (ChainPlan::kernel_name turns it into the text) and the run count of its launch
// (0: the kernel has no runs to count, or its launch sizes them itself).
struct KernelChoice {
    int id = 0;
    uint32_t runs = 0;
};

// ---- run counts.  max_runs: 0, or an upper limit of the run count below the default (CSDR_RUN1024_RUNS, CSDR_RUN1024_V3_RUNS,
// CSDR_SHARD1024_RUNS: experiments, and tests that force runs onto short inputs)

// k_run64v2.  0: not a call for the kernel; all: no size threshold (CSDR_RUN64_V2_ALL)
inline uint32_t run64_v2_runs(uint32_t nf, uint32_t cus, bool all)
{
    // two workgroups per CU; a run >= 1 reads 6 warm-up tiles and walks a halo tile: at least 16 tiles per run on average.  A call pays
    // those ~23 tile times (~60 us) whatever its size, so k_run64 keeps the calls below 3072 tiles (196 608 frames; measured by call size:
    // 4096 frames 17 us against 60 us, 131 072 frames 58 against 66, 262 144 frames 99 against 76)
    if (nf % 64u) return 0;
    const uint32_t nb = nf / 64u;
    if (nb < 3072u && !all) return 0;
    uint32_t nruns = 2 * cus;
    if (nruns > nb / 16) nruns = nb / 16;
    if (nruns > 2) nruns &= ~1u;
    return nruns;
}

// k_run1024v2.  0: call too short for the kernel
inline uint32_t run1024_v2_runs(uint32_t nf, uint32_t cus, uint32_t max_runs)
{
    // two workgroups per CU; a run >= 1 spends 6 read-only + 4 halo tiles on its start state; the shorter (younger) runs get
    // up to 1/4 less than the average: at least 24 tiles per run on average (>= 16 for every one)
    const uint32_t nb = nf / 4;
    uint32_t nruns = 2 * cus;
    if (max_runs >= 1 && max_runs < nruns) nruns = max_runs;
    if (nruns > nb / 24) nruns = nb / 24;
    if (nruns > 2) nruns &= ~1u;
    return nruns;
}

// k_run1024v3.  0: a ragged call (not whole 4-frame tiles)
inline uint32_t run1024_v3_runs(uint32_t nf, bool fm, uint32_t cus, uint32_t max_runs)
{
    // one workgroup per CU; runs are whole blocks of 8 (F32) / 4 (CF32) tiles (a row's 128-byte line), at least one (a run >= 1 walks 4
    // halo tiles in front of its first tile and folds the up to 6 tiles in front of those: short calls get as many runs as they have
    // blocks); the call's last block may be partial (nf = 0 mod 4: whole tiles)
    if (nf % 4u) return 0;
    const uint32_t TB = fm ? 8u : 4u, nblk = (nf / 4u + TB - 1) / TB;
    uint32_t nruns = cus;
    if (max_runs >= 1 && max_runs < nruns) nruns = max_runs;
    if (nruns > nblk) nruns = nblk;
    return nruns;
}

// k_shard1024.  0: the call is not for this kernel.  Whole 4-frame tiles; at least two blocks (16 / 8 tiles) per run: a run >= 1 spends
// six read-only tiles and four halo tiles on its start
inline uint32_t shard1024_runs(uint32_t nf, bool fm, uint32_t G, uint32_t cus, uint32_t max_runs)
{
    if ((G != 4 && G != 8) || (nf & 3u) || nf == 0) return 0;
    const uint32_t nb = nf / 4, TB = fm ? 8u : 4u, nblk = (nb + TB - 1) / TB;
    if ((uint64_t)(1024 / G) * nf * (fm ? 4u : 8u) >= (1ull << 31)) return 0;       // the row stores use 32-bit buffer offsets
    uint32_t nruns = cus;
    if (max_runs >= 1 && max_runs < nruns) nruns = max_runs;
    const uint32_t per = fm ? 2u : 4u;                  // >= 16 tiles per run
    if (nruns > nblk / per) nruns = nblk / per;
    return nruns;
}

// ---- cold starts: whether the runs of a launch start from DC state 0, with the kernel's dcfix launch behind them.  The shape
// half: there is a run >= 1, and every run is at least as long as what its dcfix kernel covers (run_split.h).  The capacity half is
// ColdStart::fits (fused.h): the plan's arrays were made for at least this many runs.  A plan combines the two into one flag per call.
constexpr uint32_t RUN64_COLD_TILES = 2 * (RUN64_DCFIX_F / 64);                                         // 14: the seven dcfix tiles, doubled
constexpr uint32_t RUN1024_COLD_TILES = (RUN1024_HALO + (RUN1024_DCFIX_F - 1) / 4 + 7) / 8 * 8;         // 16: 4 halo + 8 dcfix tiles, in whole blocks of 8
inline bool run64_v2_cold(uint32_t nb, uint32_t nruns) { return nruns >= 2 && nb / nruns >= RUN64_COLD_TILES; }
inline bool run1024_v3_cold(uint32_t nb, uint32_t nruns) { return nruns >= 2 && nb / nruns >= RUN1024_COLD_TILES; }
inline bool shard1024_cold(uint32_t nruns) { return nruns >= 2; }        // (shard1024_runs: at least 16 tiles per run)
inline bool run256_v2_cold(uint32_t nruns) { return nruns >= 2; }        // (make_split: at least 8 tiles per run, the seven of its dcfix among them)
// Runs the cold-start arrays are made for (ColdStart::init).  M = 1024: the plan's CU count, the most its run counts above return
constexpr uint32_t RUN64_COLD_RUNS = 1024, RUN256_COLD_RUNS = 2048;
inline bool cold_fits(uint32_t made_for, uint32_t nruns) { return nruns <= made_for; }

// k_front4096.  Frames per run: long enough that the 19 cold-start frames (about 8 frames' worth of work) stay below ~8 % of a run
inline uint32_t huge_runs(uint32_t nf, uint32_t cus, uint32_t runs_knob)
{
    uint32_t nruns = runs_knob >= 1 ? runs_knob : cus / 4;      // 4 siblings per run, one 512-thread workgroup per CU
    while (nruns > 1 && nf / nruns < 48) nruns >>= 1;    // (a run pays 20 cold-start frames: the reference chunk of 4096 frames is 64 runs of 64)
    if (nruns > 8) nruns &= ~7u;                        // the XCD-friendly workgroup -> (run, sibling) map wants a multiple of 8
    return nruns ? nruns : 1;
}

// k_dc_fold, k_dc_fold8 (kernels_dc_tile.hip).  Workgroups for nb tiles: four workgroups of four waves per CU, a tile per wave and round
inline uint32_t dc_fold_grid(uint32_t nb, uint32_t cus)
{
    const uint32_t wgs = cus * 4u;
    return wgs > (nb + 3) / 4 ? (nb + 3) / 4 : wgs;
}

// ---- M = 64 (kernels_fused_small.hip)
enum Kernel64 { K_RUN64 = 0, K_RUN64V2 };
struct Choice64 {
    bool fm, mix;
    uint32_t c0, C, cus;
    bool v1 = false;            // CSDR_RUN64_V1: k_run64 for every call
    bool v2_all = false;        // CSDR_RUN64_V2_ALL: k_run64v2 below its size threshold too
    // k_run64v2: CF32 output, whole band (the cold-start arrays are made for it)
    bool v2() const { return !fm && c0 == 0 && C == 64u && !v1; }
    KernelChoice choose(uint32_t nf) const
    {
        const uint32_t runs = (v2() && (uint64_t)C * nf * 8u < (1ull << 32)) ? run64_v2_runs(nf, cus, v2_all) : 0;
        return runs ? KernelChoice{K_RUN64V2, runs} : KernelChoice{K_RUN64, 0};     // (k_run64's runs follow its occupancy: SmallPlan::run)
    }
    // the call goes to k_run64v2 as whole 64-frame tiles, no mix inside the plan
    bool tile_major_ok(uint32_t nf) const { return !mix && choose(nf).id == K_RUN64V2; }
};

// ---- M = 1024 (kernels_pfb1024.hip)
enum Kernel1024 { K_RUN1024 = 0, K_RUN1024V2, K_RUN1024V3, K_SHARD1024 };
struct Choice1024 {
    bool fm, mix;
    uint32_t c0, C, G, cus;
    bool v1 = false;            // CSDR_RUN1024_V1: k_run1024 for every call
    bool v3_off = false;        // CSDR_RUN1024_V3=0: k_run1024 for the comparison
    bool no_shard = false;      // CSDR_NO_SHARD1024: k_run1024v2<FM, G> or whole band + gather instead
    uint32_t runs_v2 = 0, runs_v3 = 0, runs_s1 = 0;     // CSDR_RUN1024_RUNS, CSDR_RUN1024_V3_RUNS, CSDR_SHARD1024_RUNS (max_runs above)
    // k_run1024v3: whole band, calls of whole 4-frame tiles (a call that ends inside a 128-byte line stores the front part of it)
    bool v3() const { return c0 == 0 && C == 1024u && G == 1 && !v1 && !v3_off; }
    // k_run1024v2: the interleaved shards only (FM output; its whole-band instantiations are no longer built); CF32 shards: whole band + row gather
    bool v2() const { return G > 1 && fm && !v1; }
    // k_shard1024<FM | CF32, G>: every run-sized call of whole tiles
    bool shard() const { return (G == 4 || G == 8) && !v1 && !no_shard; }
    KernelChoice choose(uint32_t nf) const
    {
        uint32_t runs;
        if (shard() && (runs = shard1024_runs(nf, fm, G, cus, runs_s1))) return {K_SHARD1024, runs};
        // k_run1024v2 and k_run1024v3 index the whole-band input with 32 bits: 8 KiB per frame below 2 GiB
        const bool small = (uint64_t)nf * 8192u < (1ull << 31);
        if (small && v2() && (nf & 3u) == 0 && (runs = run1024_v2_runs(nf, cus, runs_v2))) return {K_RUN1024V2, runs};
        if (small && v3() && (runs = run1024_v3_runs(nf, fm, cus, runs_v3))) return {K_RUN1024V3, runs};
        // k_run1024: one run per CU, at least 8 tiles (of 8 frames) per run (a run >= 1 spends 3 read-only + 2 halo tiles on its start state)
        const uint32_t nb = (nf + 7) / 8;
        runs = cus < nb / 8 ? cus : nb / 8;
        return {K_RUN1024, runs ? runs : 1};
    }
    // CF32 output through k_run1024v3<CF32> (whole band) or k_shard1024<CF32, G> (interleaved shard), whole 16-frame blocks
    bool tile_major_ok(uint32_t nf) const
    {
        const int id = choose(nf).id;
        return !fm && !mix && nf % 16u == 0 && (id == K_RUN1024V3 || id == K_SHARD1024);
    }
};

}  // namespace csdr
