"""Run bounds and cold-start rules of the run kernels (csrc/run_split.h, csrc/kernel_choice.h): which tiles run w of a launch walks, and
whether the launch starts its runs cold.  No GPU needed.

A mistake here is an out-of-bounds read on the device: k_run1024v2 computes `first - 10` in unsigned arithmetic, k_run1024v3 and k_shard1024
`first - 4`, k_run64v2 `first - 1`, and a dcfix kernel corrects the first 7 (k_run64v2) or 8 (M = 1024) tiles of every cold run whatever
its length.

A small stand-alone program includes the two headers.  It is built with the host compiler, once plain and once with
-fsanitize=address,undefined; both builds must print the same.

The expected values do not come from the headers.  The program carries the bounds functions and the n0 rule as the kernel files wrote them
before the headers had them (run64_bounds, run_bounds, run3_bounds, shard_bounds, the floor split spelled out inline) as `namespace
parent` and checks equality for every run of every case.  Then, for every (configuration, nf) that Choice64 / Choice1024 send to a run
kernel, over cus in {1, 2, 8, 64, 256, 304}, run caps {0, 1, 2, 3, 7}, weights {1, 1.01, 1.1, 1.2, 1.49}, CSDR_RUN64_V2_ALL on and off and
nf = every multiple of 4 up to 4096, 2^k, 2^k +- 4, 2^k +- 64 (k = 3..22) and 3 x 2^k (k = 3..20):
  * the runs cover [0, nb) exactly once, run w + 1 behind run w, none empty;
  * a run w >= 1 starts at or beyond the tiles it reads in front of itself: 1 (k_run64v2), 10 (k_run1024v2: no clamp), 4 (k_run1024v3,
    k_shard1024);
  * where the cold rule says yes, every run is at least as long as its dcfix covers: 7 tiles (k_run64v2), 8 (k_run1024v3, k_shard1024);
  * block runs start on multiples of TB (8 for FM, 4 for CF32);
  * the plan's cold-start arrays fit every run count (cold_fits: what ColdStart::fits asks).
The literals 1, 10, 4, 7, 8 above are written out in the program, not taken from the headers' constants; the constants are checked
against them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

PROGRAM = r"""
#include "run_split.h"
#include "kernel_choice.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace parent {     // the bounds as the kernel files had them
struct Run64v2Args { uint32_t nb, nruns, n0; };
void run64_bounds(const Run64v2Args &A, unsigned w, unsigned &first, unsigned &last)      // kernels_run64_v2.hip
{
    if (A.n0 == 0 || (A.nruns & 1u)) {
        first = (unsigned)((unsigned long long)w * A.nb / A.nruns);
        last = (unsigned)((unsigned long long)(w + 1) * A.nb / A.nruns);
        return;
    }
    const unsigned half = A.nruns / 2, s = w / half, i = w - s * half;
    const unsigned base = s ? A.n0 : 0u, tiles = s ? A.nb - A.n0 : A.n0;
    first = base + (unsigned)((unsigned long long)i * tiles / half);
    last = base + (unsigned)((unsigned long long)(i + 1) * tiles / half);
}
void run_bounds(uint32_t nb, uint32_t nruns, uint32_t n0, unsigned w, unsigned &first, unsigned &last)      // kernels_run1024_v2.hip
{
    if (n0 == 0 || (nruns & 1u)) {
        first = (unsigned)((unsigned long long)w * nb / nruns);
        last = (unsigned)((unsigned long long)(w + 1) * nb / nruns);
        return;
    }
    const unsigned half = nruns / 2, s = w / half, i = w - s * half;
    const unsigned base = s ? n0 : 0u, tiles = s ? nb - n0 : n0;
    first = base + (unsigned)((unsigned long long)i * tiles / half);
    last = base + (unsigned)((unsigned long long)(i + 1) * tiles / half);
}
void run3_bounds(uint32_t nb, uint32_t nruns, unsigned w, unsigned TB, unsigned &first, unsigned &last)     // kernels_run1024_v3.hip
{
    const unsigned nblk = (nb + TB - 1) / TB;
    first = TB * (unsigned)((unsigned long long)w * nblk / nruns);
    last = TB * (unsigned)((unsigned long long)(w + 1) * nblk / nruns);
    if (last > nb) last = nb;
}
void shard_bounds(uint32_t nb, uint32_t nruns, unsigned w, unsigned TB, unsigned &first, unsigned &last)    // kernels_shard1024.hip
{
    const unsigned nblk = (nb + TB - 1) / TB;
    first = TB * (unsigned)((unsigned long long)w * nblk / nruns);
    last = TB * (unsigned)((unsigned long long)(w + 1) * nblk / nruns);
    if (last > nb) last = nb;
}
void even(uint32_t nb, uint32_t nruns, uint32_t w, uint32_t &first, uint32_t &last)       // k_pfb1024, k_pfb1024_fixup, k_front4096: inline
{
    first = (uint32_t)((uint64_t)w * nb / nruns); last = (uint32_t)((uint64_t)(w + 1) * nb / nruns);
}
uint32_t n0(uint32_t nb, uint32_t nruns, double wt)         // run64_v2_launch, run1024_v2_launch
{
    return (nruns >= 2 && !(nruns & 1u) && wt > 1.0 && wt < 1.5) ? (uint32_t)std::llround(0.5 * wt * (double)nb) : 0u;
}
}  // namespace parent

static int bad = 0;
static unsigned long long cases[5] = {0, 0, 0, 0, 0}, sum[5] = {0, 0, 0, 0, 0};
#define RULE(ok, ...) do { if (!(ok)) { if (bad < 40) { printf("RULE " __VA_ARGS__); printf("\n"); } bad++; } } while (0)

enum { EVEN = 0, R64V2, R1024V2, R1024V3, SHARD };
static const char *NAME[5] = {"even", "k_run64v2", "k_run1024v2", "k_run1024v3", "k_shard1024"};

// one launch: bounds through the header (kind says which function) against parent's, then the rules
static void launch(int kind, uint32_t nb, uint32_t nruns, uint32_t n0, uint32_t TB, uint32_t front, bool cold, uint32_t covers, const char *what, uint32_t nf)
{
    cases[kind]++;
    uint32_t pos = 0;
    for (uint32_t w = 0; w < nruns; w++) {
        uint32_t f = 0, l = 0;
        unsigned pf = 0, pl = 0;
        switch (kind) {
        case EVEN: csdr::run_range_even(nb, nruns, w, f, l); parent::even(nb, nruns, w, pf, pl); break;
        case R64V2: { csdr::run_range_halves(nb, nruns, n0, w, f, l); const parent::Run64v2Args A{nb, nruns, n0}; parent::run64_bounds(A, w, pf, pl); break; }
        case R1024V2: csdr::run_range_halves(nb, nruns, n0, w, f, l); parent::run_bounds(nb, nruns, n0, w, pf, pl); break;
        case R1024V3: csdr::run_range_blocks(nb, nruns, w, TB, f, l); parent::run3_bounds(nb, nruns, w, TB, pf, pl); break;
        default: csdr::run_range_blocks(nb, nruns, w, TB, f, l); parent::shard_bounds(nb, nruns, w, TB, pf, pl); break;
        }
        sum[kind] += (unsigned long long)f * 3u + l;
        RULE(f == pf && l == pl, "parent %s %s nf %u nb %u nruns %u n0 %u run %u: [%u, %u), parent [%u, %u)", NAME[kind], what, nf, nb, nruns, n0, w, f, l, pf, pl);
        if (kind == EVEN) { RULE(f == pos && l >= f, "cover %s %s nf %u run %u: [%u, %u) behind %u", NAME[kind], what, nf, w, f, l, pos); pos = l; continue; }    // (k_pfb1024 skips empty runs)
        RULE(f == pos && l > f, "cover %s %s nf %u nb %u nruns %u n0 %u run %u: [%u, %u) behind %u", NAME[kind], what, nf, nb, nruns, n0, w, f, l, pos);
        if (w >= 1) RULE(f >= front, "front %s %s nf %u nb %u nruns %u n0 %u run %u starts at %u, reads %u tiles in front", NAME[kind], what, nf, nb, nruns, n0, w, f, front);
        if (cold) RULE(l - f >= covers, "cold %s %s nf %u nb %u nruns %u run %u: %u tiles, the dcfix covers %u", NAME[kind], what, nf, nb, nruns, w, l - f, covers);
        if (TB) RULE(f % TB == 0, "block %s %s nf %u nb %u nruns %u run %u starts at %u (TB %u)", NAME[kind], what, nf, nb, nruns, w, f, TB);
        pos = l;
    }
    RULE(pos == nb, "cover %s %s nf %u nb %u nruns %u: ends at %u", NAME[kind], what, nf, nb, nruns, pos);
}

// argv: anchors "kind:nb:nruns:n0 or TB" (printed), then the sweep (prints nothing unless a rule fails, then the totals)
int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        unsigned kind, nb, nruns, p;
        if (sscanf(argv[a], "%u:%u:%u:%u", &kind, &nb, &nruns, &p) != 4) return 2;
        printf("case %s", argv[a]);
        for (uint32_t w = 0; w < nruns; w++) {
            uint32_t f, l;
            if (kind == 0) csdr::run_range_even(nb, nruns, w, f, l);
            else if (kind == 1) csdr::run_range_halves(nb, nruns, p, w, f, l);
            else csdr::run_range_blocks(nb, nruns, w, p, f, l);
            printf(" %u-%u", f, l);
        }
        printf("\n");
    }
    printf("const %d %d %d %d %d %d %d %u %u %u %u\n", csdr::RUN64_WU, csdr::RUN64_HALO, csdr::RUN1024_WU, csdr::RUN1024_HALO, csdr::DCFIX_F,
           csdr::RUN64_DCFIX_F, csdr::RUN1024_DCFIX_F, csdr::RUN64_COLD_TILES, csdr::RUN1024_COLD_TILES, csdr::RUN64_COLD_RUNS, csdr::RUN256_COLD_RUNS);
    printf("n0 %u %u %u %u %u\n", csdr::halves_n0(96, 4, 1.2), csdr::halves_n0(96, 3, 1.2), csdr::halves_n0(96, 4, 1.0), csdr::halves_n0(96, 4, 1.5), csdr::halves_n0(97, 2, 1.1));

    std::vector<uint32_t> nfs;
    for (uint32_t nf = 4; nf <= 4096; nf += 4) nfs.push_back(nf);
    for (uint32_t k = 3; k <= 22; k++) for (int d : {0, -4, 4, -64, 64}) if ((int64_t)(1u << k) + d > 0) nfs.push_back((uint32_t)((int64_t)(1u << k) + d));
    for (uint32_t k = 3; k <= 20; k++) nfs.push_back(3u << k);
    const uint32_t CUS[6] = {1, 2, 8, 64, 256, 304}, CAPS[5] = {0, 1, 2, 3, 7};
    const double WTS[5] = {1.0, 1.01, 1.1, 1.2, 1.49};
    char what[96];
    for (uint32_t cus : CUS) {
        // ---- M = 64: CF32, whole band
        for (int all = 0; all < 2; all++) {
            csdr::Choice64 p{};
            p.fm = false; p.mix = false; p.c0 = 0; p.C = 64; p.cus = cus; p.v2_all = all != 0;
            for (uint32_t nf : nfs) {
                const csdr::KernelChoice k = p.choose(nf);
                if (k.id != csdr::K_RUN64V2) continue;
                const uint32_t nb = nf / 64u;
                RULE(csdr::cold_fits(csdr::RUN64_COLD_RUNS, k.runs), "fits k_run64v2 cus %u nf %u: %u runs", cus, nf, k.runs);
                for (double wt : WTS) {
                    snprintf(what, sizeof what, "cus %u all %d weight %.2f", cus, all, wt);
                    const uint32_t n0 = csdr::halves_n0(nb, k.runs, wt);
                    RULE(n0 == parent::n0(nb, k.runs, wt), "parent n0 %s nf %u: %u", what, nf, n0);
                    launch(R64V2, nb, k.runs, n0, 0, 1, csdr::run64_v2_cold(nb, k.runs), 7, what, nf);
                }
            }
        }
        // ---- M = 1024: FM and CF32; whole band and the interleaved shards, with k_shard1024 and behind CSDR_NO_SHARD1024
        for (int fm = 0; fm < 2; fm++) for (uint32_t G : {1u, 2u, 4u, 8u}) for (int ns = 0; ns < 2; ns++) for (uint32_t cap : CAPS) {
            if (ns && G < 4) continue;
            csdr::Choice1024 p{};
            p.fm = fm != 0; p.mix = false; p.c0 = 0; p.C = 1024u / G; p.G = G; p.cus = cus; p.no_shard = ns != 0;
            p.runs_v2 = p.runs_v3 = p.runs_s1 = cap;
            for (uint32_t nf : nfs) {
                const csdr::KernelChoice k = p.choose(nf);
                const uint32_t nb = nf / 4u, TB = fm ? 8u : 4u;
                snprintf(what, sizeof what, "cus %u fm %d G %u no_shard %d cap %u", cus, fm, G, ns, cap);
                if (k.id == csdr::K_RUN1024) { launch(EVEN, (nf + 7) / 8, k.runs, 0, 0, 0, false, 0, what, nf); continue; }
                if (k.id == csdr::K_RUN1024V2) {                 // (two runs per CU, always warm: the plan makes no cold-start arrays for it)
                    for (double wt : WTS) {
                        const uint32_t n0 = csdr::halves_n0(nb, k.runs, wt);
                        RULE(n0 == parent::n0(nb, k.runs, wt), "parent n0 %s nf %u weight %.2f: %u", what, nf, wt, n0);
                        launch(R1024V2, nb, k.runs, n0, 0, 10, false, 0, what, nf);
                    }
                    continue;
                }
                RULE(csdr::cold_fits(cus, k.runs), "fits %s nf %u: %u runs", what, nf, k.runs);
                if (k.id == csdr::K_RUN1024V3) launch(R1024V3, nb, k.runs, 0, TB, 4, csdr::run1024_v3_cold(nb, k.runs), 8, what, nf);
                else launch(SHARD, nb, k.runs, 0, TB, 4, csdr::shard1024_cold(k.runs), 8, what, nf);
            }
        }
        // ---- k_front4096: runs of frames
        for (uint32_t knob : CAPS) for (uint32_t nf : nfs) { snprintf(what, sizeof what, "front4096 cus %u knob %u", cus, knob); launch(EVEN, nf, csdr::huge_runs(nf, cus, knob), 0, 0, 0, false, 0, what, nf); }
    }
    for (int i = 0; i < 5; i++) printf("sweep %s launches %llu checksum %llu\n", NAME[i], cases[i], sum[i]);
    printf("failures %d\n", bad);
    return bad ? 1 : 0;
}
"""

# (kind: 0 even, 1 halves, 2 blocks; nb; nruns; n0 or TB) -> the runs, worked out by hand
ANCHORS = [
    ((0, 10, 3, 0), "0-3 3-6 6-10"),
    ((0, 3, 4, 0), "0-0 0-1 1-2 2-3"),                         # an empty run: k_pfb1024 and its fix-up skip it
    ((1, 96, 4, 58), "0-29 29-58 58-77 77-96"),                # n0 = llround(0.5 * 1.2 * 96): 29 + 29 | 19 + 19
    ((1, 96, 4, 0), "0-24 24-48 48-72 72-96"),
    ((1, 97, 3, 58), "0-32 32-64 64-97"),                      # an odd run count: even split whatever n0
    ((2, 32, 2, 8), "0-16 16-32"),
    ((2, 35, 2, 8), "0-16 16-35"),                             # five blocks, the last one partial
    ((2, 35, 3, 4), "0-12 12-24 24-35"),                       # nine blocks of four
    ((2, 5, 1, 8), "0-5"),
]


def _arg(a):
    return ":".join(str(v) for v in a)


def _build(tmp, name, extra):
    src = tmp / "bounds_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    out = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "composable_sdr_amd", "csrc"),
                          str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def bounds(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("run_bounds")
    args = [_arg(a) for a, _ in ANCHORS]
    plain = subprocess.run([str(_build(tmp, "bounds_plain", [])), *args], capture_output=True, text=True, timeout=600)
    san = subprocess.run([str(_build(tmp, "bounds_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])), *args],
                         capture_output=True, text=True, timeout=600)
    return plain, san


def test_sanitized_build_prints_the_same(bounds):
    plain, san = bounds
    assert san.stderr == "" and plain.stdout == san.stdout and plain.returncode == san.returncode


def test_sweep_rules(bounds):
    """equal to the parent's bounds; cover, front tiles, cold run lengths, block starts, capacity"""
    plain, _ = bounds
    assert plain.returncode == 0, "\n".join(ln for ln in plain.stdout.splitlines() if ln.startswith(("RULE", "failures")))[:4000] + plain.stderr[-1000:]
    swept = {ln.split()[1]: int(ln.split()[3]) for ln in plain.stdout.splitlines() if ln.startswith("sweep ")}
    assert set(swept) == {"even", "k_run64v2", "k_run1024v2", "k_run1024v3", "k_shard1024"} and all(n > 1000 for n in swept.values()), swept


def test_constants_and_thresholds(bounds):
    """warm-up / halo tiles, dcfix frames, the run-length thresholds derived from them and the capacities: today's numbers"""
    got = {ln.split()[0]: ln.split()[1:] for ln in bounds[0].stdout.splitlines() if ln.startswith(("const ", "n0 "))}
    assert [int(v) for v in got["const"]] == [6, 1, 6, 4, 113, 448, 33, 14, 16, 1024, 2048]
    # llround(0.5 * 1.2 * 96) = 58; odd run count, weight 1 and weight 1.5: even split; llround(0.5 * 1.1 * 97 = 53.35) = 53
    assert [int(v) for v in got["n0"]] == [58, 0, 0, 0, 53]


@pytest.mark.parametrize("anchor", ANCHORS, ids=[_arg(a).replace(":", "-") for a, _ in ANCHORS])
def test_anchor(anchor, bounds):
    a, runs = anchor
    got = {ln.split()[1]: " ".join(ln.split()[2:]) for ln in bounds[0].stdout.splitlines() if ln.startswith("case ")}[_arg(a)]
    assert got == runs
