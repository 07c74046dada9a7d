"""Which kernel a chain call takes (csrc/kernel_choice.h): Choice64 and Choice1024, the selection of the M = 64 and M = 1024 plans.  No GPU needed.

A small stand-alone program includes the header and prints `kernel id, runs, tile-major-ok` for every command-line case.  It is built
with the host compiler, once plain and once with -fsanitize=address,undefined; both builds must print the same.

The expected values do not come from the header.  ANCHORS was worked out from the selection as the plans wrote it out before the header
existed (three run-count functions per plan, evaluated in SmallPlan::run / BigPlan::run and again in tile_major_ok), and the program
carries that selection, run-count bodies included, as `namespace parent`: over a sweep of nf (1 .. 4096, the powers of two up to 2^20
and each of those +-1) it checks for every configuration that the header's choice equals parent's, and that a call accepted for
tile-major output goes to a kernel that writes tile-major planes (k_run64v2; k_run1024v3 and k_shard1024 with CF32 output).

`parent` is the per-call selection.  It bounds k_run1024v2 and k_run1024v3 by nf * 8192 < 2^31 (2 GiB of whole-band input); the name a
handle reported before its first call was worked out without that bound, and now follows the per-call selection too."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

PROGRAM = r"""
#include "kernel_choice.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace parent {     // the selection before kernel_choice.h: run counts as the run kernels' files defined them, chosen as the plans' run() did
uint32_t run64_v2_runs(uint32_t nf, uint32_t cus, bool all)
{
    if (nf % 64u) return 0;
    const uint32_t nb = nf / 64u;
    if (nb < 3072u && !all) return 0;
    uint32_t nruns = 2 * cus;
    if (nruns > nb / 16) nruns = nb / 16;
    if (nruns > 2) nruns &= ~1u;
    return nruns;
}
uint32_t run1024_v2_runs(uint32_t nf, uint32_t cus, uint32_t max_runs)
{
    const uint32_t nb = nf / 4;
    uint32_t nruns = 2 * cus;
    if (max_runs >= 1 && max_runs < nruns) nruns = max_runs;
    if (nruns > nb / 24) nruns = nb / 24;
    if (nruns > 2) nruns &= ~1u;
    return nruns;
}
uint32_t run1024_v3_runs(uint32_t nf, bool fm, uint32_t cus, uint32_t max_runs)
{
    const uint32_t TB = fm ? 8 : 4;
    if (nf % 4) return 0;
    const uint32_t nblk = (nf / 4 + TB - 1) / TB;
    uint32_t nruns = cus;
    if (max_runs >= 1 && max_runs < nruns) nruns = max_runs;
    if (nruns > nblk) nruns = nblk;
    return nruns;
}
uint32_t shard1024_runs(uint32_t nf, bool fm, uint32_t G, uint32_t cus, uint32_t max_runs)
{
    if ((G != 4 && G != 8) || (nf & 3u) || nf == 0) return 0;
    const uint32_t nb = nf / 4, TB = fm ? 8u : 4u, nblk = (nb + TB - 1) / TB;
    if ((uint64_t)(1024 / G) * nf * (fm ? 4u : 8u) >= (1ull << 31)) return 0;
    uint32_t nruns = cus;
    if (max_runs >= 1 && max_runs < nruns) nruns = max_runs;
    const uint32_t per = fm ? 2u : 4u;
    if (nruns > nblk / per) nruns = nblk / per;
    return nruns;
}
struct Cfg { uint32_t M; bool fm, mix; uint32_t G, cus; bool v1, v3_off, no_shard; uint32_t r2, r3, rs; bool v2_all; uint32_t c0, C; };
// SmallPlan::run: k_run64v2 (1) or k_run64 (0, runs left to the launch)
void choose64(const Cfg &c, uint32_t nf, int &id, uint32_t &runs, bool &tm)
{
    const bool v2_ok = !c.fm && c.c0 == 0 && c.C == 64u && !c.v1;
    const uint32_t v2runs = (v2_ok && (uint64_t)c.C * nf * 8u < (1ull << 32)) ? run64_v2_runs(nf, c.cus, c.v2_all) : 0;
    id = v2runs ? 1 : 0; runs = v2runs;
    tm = v2_ok && !c.mix && !c.fm && (uint64_t)c.C * nf * 8u < (1ull << 32) && run64_v2_runs(nf, c.cus, c.v2_all) != 0;
}
// BigPlan::run: k_shard1024 (3), k_run1024v3 (2), k_run1024v2 (1) or k_run1024 (0)
void choose1024(const Cfg &c, uint32_t nf, int &id, uint32_t &runs, bool &tm)
{
    const bool v3_ok = c.c0 == 0 && c.C == 1024u && c.G == 1 && !c.v1 && !c.v3_off;
    const bool v2_ok = c.G > 1 && c.fm && !c.v1;
    const bool s1_ok = (c.G == 4 || c.G == 8) && !c.v1 && !c.no_shard;
    const uint32_t s1runs = s1_ok ? shard1024_runs(nf, c.fm, c.G, c.cus, c.rs) : 0;
    const uint32_t v2runs = (!s1runs && v2_ok && (nf & 3u) == 0 && (uint64_t)nf * 8192u < (1ull << 31)) ? run1024_v2_runs(nf, c.cus, c.r2) : 0;
    const uint32_t v3runs = (v3_ok && (uint64_t)nf * 8192u < (1ull << 31)) ? run1024_v3_runs(nf, c.fm, c.cus, c.r3) : 0;
    if (s1runs) { id = 3; runs = s1runs; }
    else if (v3runs) { id = 2; runs = v3runs; }
    else if (v2runs) { id = 1; runs = v2runs; }
    else {
        const uint32_t nb = (nf + 7) / 8;
        uint32_t nruns = c.cus;
        if (nruns > nb / 8) nruns = nb / 8;
        if (nruns < 1) nruns = 1;
        id = 0; runs = nruns;
    }
    if (s1_ok) tm = !c.fm && !c.mix && nf % 16u == 0 && shard1024_runs(nf, false, c.G, c.cus, c.rs) != 0;
    else tm = v3_ok && !c.fm && !c.mix && nf % 16u == 0 && (uint64_t)nf * 8192u < (1ull << 31) && run1024_v3_runs(nf, false, c.cus, c.r3) != 0;
}
}  // namespace parent

static void header_choice(const parent::Cfg &c, uint32_t nf, int &id, uint32_t &runs, bool &tm)
{
    csdr::KernelChoice k;
    if (c.M == 64) {
        csdr::Choice64 p{};
        p.fm = c.fm; p.mix = c.mix; p.c0 = c.c0; p.C = c.C; p.cus = c.cus; p.v1 = c.v1; p.v2_all = c.v2_all;
        k = p.choose(nf); tm = p.tile_major_ok(nf);
    } else {
        csdr::Choice1024 p{};
        p.fm = c.fm; p.mix = c.mix; p.c0 = c.c0; p.C = c.C; p.G = c.G; p.cus = c.cus; p.v1 = c.v1; p.v3_off = c.v3_off; p.no_shard = c.no_shard;
        p.runs_v2 = c.r2; p.runs_v3 = c.r3; p.runs_s1 = c.rs;
        k = p.choose(nf); tm = p.tile_major_ok(nf);
    }
    id = k.id; runs = k.runs;
}

// argv: one case per argument, "M:fm:mix:G:cus:v1:v3_off:no_shard:r2:r3:rs:v2_all:nf"; nf = 0: the sweep (prints nothing unless a rule fails)
int main(int argc, char **argv)
{
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        unsigned v[13];
        if (sscanf(argv[a], "%u:%u:%u:%u:%u:%u:%u:%u:%u:%u:%u:%u:%u", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11, v + 12) != 13) return 2;
        const parent::Cfg c{v[0], v[1] != 0, v[2] != 0, v[3], v[4], v[5] != 0, v[6] != 0, v[7] != 0, v[8], v[9], v[10], v[11] != 0, 0u, v[0] / v[3]};
        std::vector<uint32_t> nfs;
        if (v[12]) nfs.push_back(v[12]);
        else {
            for (uint32_t nf = 1; nf <= 4096; nf++) nfs.push_back(nf);
            for (uint32_t e = 0; e <= 20; e++) { nfs.push_back((1u << e) - 1); nfs.push_back(1u << e); nfs.push_back((1u << e) + 1); }
        }
        for (uint32_t nf : nfs) {
            if (!nf) continue;
            int id, pid; uint32_t runs, pruns; bool tm, ptm;
            header_choice(c, nf, id, runs, tm);
            if (c.M == 64) parent::choose64(c, nf, pid, pruns, ptm); else parent::choose1024(c, nf, pid, pruns, ptm);
            if (v[12]) printf("case %s %d %u %d\n", argv[a], id, runs, (int)tm);
            const bool writes_tm = c.M == 64 ? id == 1 : (!c.fm && (id == 2 || id == 3));
            if (tm && !writes_tm) { printf("RULE tile-major %s nf %u: kernel %d\n", argv[a], nf, id); bad = 1; }
            if (id != pid || runs != pruns || tm != ptm) { printf("RULE parent %s nf %u: %d %u %d, parent %d %u %d\n", argv[a], nf, id, runs, (int)tm, pid, pruns, (int)ptm); bad = 1; }
        }
    }
    return bad;
}
"""

NAMES = {64: ["k_run64", "k_run64v2"], 1024: ["k_run1024", "k_run1024v2", "k_run1024v3", "k_shard1024"]}


def _cfg(M, fm, G=1, mix=0, cus=256, v1=0, v3_off=0, no_shard=0, r2=0, r3=0, rs=0, v2_all=0):
    return (M, int(fm), mix, G, cus, v1, v3_off, no_shard, r2, r3, rs, v2_all)


def _arg(cfg, nf):
    return ":".join(str(v) for v in (*cfg, nf))


FM, CF32 = True, False
# (configuration, nf, kernel, runs or None, tile-major-ok or None): cus = 256, no caps unless noted
ANCHORS = [
    (_cfg(1024, FM), 65536, "k_run1024v3", 256, None),
    (_cfg(1024, FM), 96, "k_run1024v3", 3, None),
    (_cfg(1024, FM), 75, "k_run1024", 1, None),
    (_cfg(1024, FM, r3=8), 2048, "k_run1024v3", 8, None),
    (_cfg(1024, FM), 262144, "k_run1024", 256, None),             # the 2 GiB bound
    (_cfg(1024, CF32), 96, "k_run1024v3", 6, True),
    (_cfg(1024, CF32), 100, "k_run1024v3", None, False),
    (_cfg(1024, FM, G=8), 65536, "k_shard1024", 256, None),
    (_cfg(1024, FM, G=8, rs=4), 1024, "k_shard1024", 4, None),
    (_cfg(1024, FM, G=8), 96, "k_shard1024", 1, None),
    (_cfg(1024, FM, G=8), 8, "k_run1024", None, None),
    (_cfg(1024, FM, G=8), 5, "k_run1024", None, None),
    (_cfg(1024, CF32, G=8), 32, "k_run1024", None, None),
    (_cfg(1024, FM, G=4, no_shard=1), 1024, "k_run1024v2", None, None),
    (_cfg(1024, FM, G=2), 65536, "k_run1024v2", 512, None),
    (_cfg(1024, FM, G=2, r2=4), 1024, "k_run1024v2", 4, None),
    (_cfg(1024, FM, G=2), 96, "k_run1024v2", 1, None),
    (_cfg(1024, FM, G=2), 92, "k_run1024", None, None),
    (_cfg(1024, CF32, G=2), 65536, "k_run1024", None, None),      # CF32, G = 2: any nf
    (_cfg(1024, CF32, G=2), 96, "k_run1024", None, None),
    (_cfg(64, CF32), 1048576, "k_run64v2", 512, None),
    (_cfg(64, CF32), 196608, "k_run64v2", 192, None),
    (_cfg(64, CF32), 196544, "k_run64", None, None),
    (_cfg(64, CF32, v2_all=1), 8192, "k_run64v2", 8, None),
    (_cfg(64, CF32, v2_all=1), 6144, "k_run64v2", 6, None),
    (_cfg(64, CF32), 5, "k_run64", None, None),
    (_cfg(64, FM), 1048576, "k_run64", None, None),               # FM: any nf
    (_cfg(64, FM, v2_all=1), 8192, "k_run64", None, None),
]
# the sweep: every anchor configuration, and the knobs and shapes the anchors leave out
SWEEP = sorted({a[0] for a in ANCHORS} | {
    _cfg(1024, FM, v1=1), _cfg(1024, FM, v3_off=1), _cfg(1024, CF32, mix=1), _cfg(1024, FM, G=4), _cfg(1024, CF32, G=4), _cfg(1024, CF32, G=8, rs=4),
    _cfg(1024, FM, G=8, v1=1), _cfg(1024, CF32, G=4, no_shard=1), _cfg(1024, FM, cus=64), _cfg(1024, CF32, cus=304), _cfg(1024, FM, G=8, cus=64),
    _cfg(64, CF32, v1=1), _cfg(64, CF32, mix=1, v2_all=1), _cfg(64, CF32, cus=64), _cfg(64, CF32, G=2, v2_all=1),
})


def _build(tmp, name, extra):
    src = tmp / "choice_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    out = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "composable_sdr_amd", "csrc"),
                          str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def choices(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("kernel_choice")
    args = [_arg(c, nf) for c, nf, *_ in ANCHORS] + [_arg(c, 0) for c in SWEEP]
    plain = subprocess.run([str(_build(tmp, "choice_plain", [])), *args], capture_output=True, text=True, timeout=120)
    san = subprocess.run([str(_build(tmp, "choice_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])), *args],
                         capture_output=True, text=True, timeout=120)
    return plain, san


def test_sanitized_build_prints_the_same(choices):
    plain, san = choices
    assert san.stderr == "" and plain.stdout == san.stdout and plain.returncode == san.returncode


def test_sweep_rules(choices):
    """tile-major-ok implies a kernel that writes tile-major planes; the choice equals the parent's selection"""
    plain, _ = choices
    assert plain.returncode == 0, "\n".join(ln for ln in plain.stdout.splitlines() if ln.startswith("RULE"))[:3000] + plain.stderr[-1000:]


@pytest.mark.parametrize("anchor", ANCHORS, ids=[f"{a[2]}-{_arg(a[0], a[1]).replace(':', '-')}" for a in ANCHORS])
def test_anchor(anchor, choices):
    cfg, nf, kernel, runs, tm = anchor
    got = {ln.split()[1]: ln.split()[2:] for ln in choices[0].stdout.splitlines() if ln.startswith("case ")}[_arg(cfg, nf)]
    assert NAMES[cfg[0]][int(got[0])] == kernel, got
    if runs is not None:
        assert int(got[1]) == runs, got
    if tm is not None:
        assert bool(int(got[2])) == tm, got
