"""The launch shape of the time-parallel AGC tail (csrc/agc_tail_shape.h) and the k_dc_fold grid (csrc/kernel_choice.h).  No GPU needed.

A small stand-alone program includes the two headers and prints the shape of every command-line case.  It is built with the host
compiler, once plain and once with -fsanitize=address,undefined; both builds must print the same.

The expected values do not come from the headers.  ANCHORS was worked out by hand from the arithmetic as agc_tail_process wrote it out
before the header existed, and the program carries that arithmetic -- the knob parsing of agc_tail_create, the predicate
agc_tail_tm_supported, the segment rules and grids of agc_tail_process, the two copies of the k_dc_fold grid -- as `namespace parent`.
Over a sweep of channel counts, call sizes, CU counts and knob sets it checks that every field of the header's shape, the predicate, the
parsed knobs and the table sizes equal parent's, and that the two internal bounds of AgcTailPlan::run hold for every call a handle
accepts: nseg <= max_seg, and on the tile-major route C nseg nck <= ckpt_cap (with max_frames = nf and max_frames = 2^20).  No swept
call violates either bound.

Calls of C nf >= 2^32 samples are left out: the tail refuses them before it asks for a shape."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

PROGRAM = r"""
#include "agc_tail_shape.h"
#include "kernel_choice.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// the texts of CSDR_AGC_L, _L_TM, _W, _WGS, CSDR_CUS, CSDR_AGC_TM (null: not set)
struct Env { const char *l, *l_tm, *w, *wgs, *cus, *tm; };
static const Env ENVS[] = {
    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
    {"256", nullptr, "512", nullptr, nullptr, nullptr},
    {nullptr, "688", "512", nullptr, nullptr, nullptr},
    {nullptr, "16", nullptr, nullptr, nullptr, nullptr},
    {nullptr, "100000", nullptr, nullptr, nullptr, nullptr},
    {nullptr, nullptr, "8208", nullptr, nullptr, nullptr},
    {nullptr, nullptr, nullptr, "1", nullptr, nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr, "0"},
    {"100", "700", "1000", "2", "64", "1"},      // (not a multiple of 16 anywhere; a CU mask)
};
constexpr unsigned NENV = sizeof(ENVS) / sizeof(ENVS[0]);

namespace parent {     // kernels_agc_tail.hip and kernels_dc_tile.hip before agc_tail_shape.h
constexpr uint32_t TM_CK = 256, TM_GUARD = 512;
struct AgcTailPlan {
    uint32_t C = 0, max_nf = 0, L = 0, Lmin = 384, W = 1024, max_seg = 0;
    uint32_t L_tm = 0;
    size_t ckpt_cap = 0;
    uint32_t wg_slots = 1024;
    bool off = false;       // agc_tail_tm_supported's function-static
};
// agc_tail_create; cus: what hipDeviceGetAttribute answered
AgcTailPlan create(uint32_t C, uint32_t max_nf, int cus, const Env &env)
{
    AgcTailPlan plan, *p = &plan;
    p->C = C; p->max_nf = max_nf;
    if (const char *e = env.l) { p->L = (uint32_t)atol(e); p->L = (p->L + 15u) / 16u * 16u; if (p->L < 16) p->L = 16; }
    if (const char *e = env.l_tm) { p->L_tm = ((uint32_t)atol(e) + 15u) / 16u * 16u; if (p->L_tm < 16) p->L_tm = 16; if (p->L_tm > 8176u) p->L_tm = 8176u; }
    if (const char *e = env.w) p->W = (uint32_t)atol(e);
    p->W = (p->W + 15u) / 16u * 16u;
    {
        if (const char *e = env.cus) { if (atoi(e) > 0 && atoi(e) < cus) cus = atoi(e); }
        p->wg_slots = (uint32_t)cus * 4u;
        if (const char *e = env.wgs) p->wg_slots = (uint32_t)cus * (uint32_t)(atol(e) > 0 ? atol(e) : 1);
    }
    p->max_seg = (max_nf + 15u) / 16u + 1;
    p->ckpt_cap = (size_t)C * ((size_t)max_nf / 128u + 64u);
    p->off = env.tm && atoi(env.tm) == 0;
    return plan;
}
bool tm_supported(const AgcTailPlan *p, uint32_t nf)
{
    if (p->off || !p || !nf || nf % 16u || p->W > 8192u || p->W % 16u) return false;
    if (!(p->C % 64u == 0 || (p->C < 64u && 64u % p->C == 0))) return false;
    if (nf < 4u * p->W) return false;
    if (((uint64_t)nf / 16u + 2ull * TM_GUARD) * p->C * 128ull >= (1ull << 32)) return false;
    return true;
}
struct Shape { uint32_t L, nseg, nck; bool pairs; uint32_t ls, groups, grid, Cw, nsub, ncg, grid_tm; };
// agc_tail_process between its checks and its launches
Shape process(const AgcTailPlan *p, uint32_t nf, bool tm)
{
    const uint32_t Cw = p->C < 64u ? p->C : 64u, nsub = 64u / Cw, ncg = p->C / Cw;
    uint32_t L = tm ? p->L_tm : p->L;
    const uint32_t lmin_tm = 128u;
    if (!L && tm) {
        uint64_t nseg_t = (uint64_t)p->wg_slots * nsub * 2u / (3u * ncg);
        if (nseg_t < 2) nseg_t = 2;
        L = (uint32_t)((nf + nseg_t - 1) / nseg_t);
        L = (L + 31u) / 32u * 32u;
        if (L < lmin_tm) L = lmin_tm;
        if (L > 8160u) L = 8160u;
    }
    if (tm && L < lmin_tm) L = lmin_tm;
    if (tm && (L % 32u)) L = (L + 31u) / 32u * 32u;
    if (!L) {
        const uint64_t nseg_t = 64ull * p->wg_slots / p->C ? 64ull * p->wg_slots / p->C : 1ull;
        L = (uint32_t)((nf + nseg_t - 1) / nseg_t);
        L = (L + 15u) / 16u * 16u;
        const uint32_t lmin = ((uint64_t)p->C * nf * 8 /* sizeof(float2) */ <= (24ull << 20)) ? 16u : p->Lmin;
        if (L < lmin) L = lmin;
        if (((L / 16u) & 1u) == 0) L += 16u;
    }
    const uint32_t nseg = (nf + L - 1) / L;
    const uint32_t nck = (L + TM_CK - 1u) / TM_CK;
    const bool pairs = (nf & 1u) == 0 && (uint64_t)p->C * nf >= 2;
    uint32_t ls = 6;
    if (nseg <= 32u && pairs && (nf & 3u) == 0 && p->C >= 8u && (uint64_t)nf * 64ull < (1ull << 32)) { ls = 3; while ((1u << ls) < nseg) ls++; }
    const uint32_t spw = 1u << ls, cpw = 64u >> ls;
    const uint32_t groups = (nseg + spw - 1u) / spw;
    const uint32_t grid = ((p->C + cpw - 1u) / cpw) * groups;
    const uint32_t gtm = ncg * ((nseg + nsub - 1) / nsub);
    return {L, nseg, nck, pairs, ls, groups, grid, Cw, nsub, ncg, gtm};
}
// dctile_mix_identity
uint32_t fold_grid(uint32_t nb, uint32_t cus)
{
    uint32_t wgs = cus * 4u;
    if (wgs > (nb + 3) / 4) wgs = (nb + 3) / 4;
    return wgs;
}
// dctile_mix_identity_shard
uint32_t fold8_grid(uint32_t nb, uint32_t cus)
{
    uint32_t wgs = cus * 4u;
    if (wgs > (nb + 3) / 4) wgs = (nb + 3) / 4;
    return wgs;
}
}  // namespace parent

static int bad = 0;
#define RULE(ok, ...) do { if (!(ok)) { printf("RULE " __VA_ARGS__); printf("\n"); bad = 1; } } while (0)

static void one(uint32_t cus, unsigned e, uint32_t C, uint32_t nf, bool want_tm, bool print)
{
    const Env &env = ENVS[e];
    const csdr::AgcTailKnobs k = csdr::AgcTailKnobs::parse(cus, env.l, env.l_tm, env.w, env.wgs, env.cus, env.tm);
    for (uint32_t max_nf : {nf, 1u << 20}) {
        if (nf > max_nf) continue;
        const parent::AgcTailPlan p = parent::create(C, max_nf, (int)cus, env);
        const csdr::AgcTailSizes z = csdr::agc_tail_sizes(C, max_nf);
        RULE(k.L == p.L && k.L_tm == p.L_tm && k.W == p.W && k.Lmin == p.Lmin && k.wg_slots == p.wg_slots && k.tm_off == p.off,
             "knobs cus %u env %u: %u %u %u %u %u %d, parent %u %u %u %u %u %d", cus, e, k.L, k.L_tm, k.W, k.Lmin, k.wg_slots, (int)k.tm_off, p.L, p.L_tm,
             p.W, p.Lmin, p.wg_slots, (int)p.off);
        RULE(z.max_seg == p.max_seg && z.ckpt_cap == p.ckpt_cap, "sizes C %u max_nf %u", C, max_nf);
        const bool sup = csdr::agc_tail_tm_supported(k, C, nf);
        RULE(sup == parent::tm_supported(&p, nf), "supported cus %u env %u C %u nf %u: %d", cus, e, C, nf, (int)sup);
        RULE(csdr::agc_tail_tm_channels_ok(C) == (C % 64u == 0 || (C < 64u && 64u % C == 0)), "channels %u", C);
        RULE(csdr::agc_tail_tm_guard(C) == (size_t)parent::TM_GUARD * 16u * C, "guard %u", C);
        if (want_tm && !sup) { if (print) printf("case %u:%u:%u:%u:1 unsupported\n", cus, e, C, nf); continue; }
        const csdr::AgcTailShape h = csdr::agc_tail_shape(k, C, nf, want_tm);
        const parent::Shape q = parent::process(&p, nf, want_tm);
        RULE(h.L == q.L && h.nseg == q.nseg && h.nck == q.nck && h.pairs == q.pairs && h.ls == q.ls && h.groups == q.groups && h.grid == q.grid &&
             h.Cw == q.Cw && h.nsub == q.nsub && h.ncg == q.ncg && h.grid_tm == q.grid_tm,
             "shape cus %u env %u C %u nf %u tm %d: L %u nseg %u nck %u pairs %d ls %u groups %u grid %u Cw %u nsub %u ncg %u grid_tm %u, parent L %u nseg %u nck %u "
             "pairs %d ls %u groups %u grid %u Cw %u nsub %u ncg %u grid_tm %u", cus, e, C, nf, (int)want_tm, h.L, h.nseg, h.nck, (int)h.pairs, h.ls, h.groups,
             h.grid, h.Cw, h.nsub, h.ncg, h.grid_tm, q.L, q.nseg, q.nck, (int)q.pairs, q.ls, q.groups, q.grid, q.Cw, q.nsub, q.ncg, q.grid_tm);
        // the two internal bounds of AgcTailPlan::run, and what the tile-major kernel's guards are sized for
        RULE(h.nseg <= z.max_seg, "segment bound cus %u env %u C %u nf %u max_nf %u tm %d: %u > %u", cus, e, C, nf, max_nf, (int)want_tm, h.nseg, z.max_seg);
        if (want_tm) {
            RULE((size_t)C * h.nseg * h.nck <= z.ckpt_cap, "checkpoint bound cus %u env %u C %u nf %u max_nf %u: %zu > %zu", cus, e, C, nf, max_nf,
                 (size_t)C * h.nseg * h.nck, z.ckpt_cap);
            RULE(h.L <= csdr::TM_GUARD * 16u && k.W <= csdr::TM_GUARD * 16u && h.L % 32u == 0, "guard cus %u env %u C %u nf %u: L %u W %u", cus, e, C, nf, h.L, k.W);
        }
        if (print && max_nf == nf)
            printf("case %u:%u:%u:%u:%d %u %u %u %d %u %u %u %u %u %u %u\n", cus, e, C, nf, (int)want_tm, h.L, h.nseg, h.nck, (int)h.pairs, h.ls, h.groups, h.grid,
                   h.Cw, h.nsub, h.ncg, h.grid_tm);
    }
}

// argv: "sweep", or one case per argument "cus:env:C:nf:tm"
int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        if (strcmp(argv[a], "sweep")) {
            unsigned v[5];
            if (sscanf(argv[a], "%u:%u:%u:%u:%u", v, v + 1, v + 2, v + 3, v + 4) != 5 || v[1] >= NENV) return 2;
            one(v[0], v[1], v[2], v[3], v[4] != 0, true);
            continue;
        }
        std::vector<uint32_t> nfs;
        for (uint32_t nf = 1; nf <= 4096; nf++) nfs.push_back(nf);
        for (uint32_t nf = 4096 + 16; nf <= 8192; nf += 16) nfs.push_back(nf);
        for (uint32_t e = 0; e <= 20; e++) { nfs.push_back((1u << e) - 1); nfs.push_back(1u << e); nfs.push_back((1u << e) + 1); }
        for (uint32_t cus : {8u, 256u, 304u})
            for (unsigned e = 0; e < NENV; e++)
                for (uint32_t C : {1u, 2u, 3u, 8u, 16u, 20u, 32u, 64u, 100u, 256u, 1024u, 4096u})
                    for (uint32_t nf : nfs) {
                        if (!nf || (uint64_t)C * nf >= (1ull << 32)) continue;      // (the tail refuses the call before it asks for a shape)
                        one(cus, e, C, nf, false, false);
                        one(cus, e, C, nf, true, false);      // (where the predicate accepts the call)
                    }
        for (uint32_t cus : {8u, 256u, 304u})
            for (uint32_t nb = 1; nb <= 5000; nb++) {
                const uint32_t g = csdr::dc_fold_grid(nb, cus);
                RULE(g == parent::fold_grid(nb, cus) && g == parent::fold8_grid(nb, cus) && g >= 1, "fold grid nb %u cus %u: %u", nb, cus, g);
            }
    }
    return bad;
}
"""

KNOBS = ["none", "L=256,W=512", "W=512,L_TM=688", "L_TM=16", "L_TM=100000", "W=8208", "WGS=1", "TM=0", "ragged"]      # ENVS of the program, by index
FIELDS = ["L", "nseg", "nck", "pairs", "ls", "groups", "grid", "Cw", "nsub", "ncg", "grid_tm"]
# (cus, knob set, C, nf, tile-major, expected fields), worked by hand from the parent's text:
ANCHORS = [
    # wg_slots = 1024; 64 * 1024 / 256 = 256 segments wanted: L = 16 (8 MiB plane: lmin = 16; 16 / 16 odd); 256 > 32 segments: 64 per workgroup
    (256, 0, 256, 4096, 0, dict(L=16, nseg=256, nck=1, pairs=1, ls=6, groups=4, grid=1024)),
    # 1024 * 1 * 2 / (3 * 4) = 170 segments wanted: ceil(65536 / 170) = 386 -> 416; ceil(65536 / 416) = 158; ceil(416 / 256) = 2
    (256, 0, 256, 65536, 1, dict(Cw=64, nsub=1, ncg=4, L=416, nseg=158, nck=2, grid_tm=632)),
    # C < 64, tile-major: four segments of 16 channels per workgroup; 1024 * 4 * 2 / 3 = 2730 wanted: ceil(16384 / 2730) = 7 -> 32 -> lmin_tm = 128
    (256, 0, 16, 16384, 1, dict(Cw=16, nsub=4, ncg=1, L=128, nseg=128, nck=1, grid_tm=32)),
    # C < 64, tile-major, CSDR_AGC_L_TM = 688 -> whole block pairs: 704; ceil(32768 / 704) = 47; two segments of 32 channels per workgroup
    (256, 2, 32, 32768, 1, dict(Cw=32, nsub=2, ncg=1, L=704, nseg=47, nck=3, grid_tm=24)),
    # odd nf: no 16-byte pieces; 21845 segments wanted: L = 16; ceil(1001 / 16) = 63 segments in one group per channel
    (256, 0, 3, 1001, 0, dict(L=16, nseg=63, nck=1, pairs=0, ls=6, groups=1, grid=3)),
    # CSDR_AGC_L = 256 (a knob keeps its even L / 16): 16 segments <= 32 -> 16 segments x 4 channels per workgroup
    (256, 1, 256, 4096, 0, dict(L=256, nseg=16, nck=1, pairs=1, ls=4, groups=1, grid=64)),
]
# calls the tile-major predicate refuses: the knob, a short call, a ragged call, a channel count, a warm-up beyond the guards
REFUSED = [(256, 7, 256, 65536), (256, 0, 256, 4080), (256, 0, 256, 65544), (256, 0, 100, 65536), (256, 5, 256, 65536)]


def _arg(cus, e, C, nf, tm):
    return f"{cus}:{e}:{C}:{nf}:{tm}"


def _build(tmp, name, extra):
    src = tmp / "shape_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    out = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "composable_sdr_amd", "csrc"),
                          str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("agc_tail_shape")
    args = [_arg(*a[:5]) for a in ANCHORS] + [_arg(*r, 1) for r in REFUSED] + ["sweep"]
    plain = subprocess.run([str(_build(tmp, "shape_plain", ["-O2"])), *args], capture_output=True, text=True, timeout=600)
    san = subprocess.run([str(_build(tmp, "shape_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])), *args],
                         capture_output=True, text=True, timeout=600)
    return plain, san


def test_sanitized_build_prints_the_same(shapes):
    plain, san = shapes
    assert san.stderr == "" and plain.stdout == san.stdout and plain.returncode == san.returncode


def test_sweep_rules(shapes):
    """shape, predicate, knobs, sizes and the k_dc_fold grid equal the parent's; the segment and checkpoint bounds hold"""
    plain, _ = shapes
    assert plain.returncode == 0, "\n".join(ln for ln in plain.stdout.splitlines() if ln.startswith("RULE"))[:3000] + plain.stderr[-1000:]


def _cases(shapes):
    return {ln.split()[1]: ln.split()[2:] for ln in shapes[0].stdout.splitlines() if ln.startswith("case ")}


@pytest.mark.parametrize("anchor", ANCHORS, ids=[f"{KNOBS[a[1]]}-{_arg(*a[:5]).replace(':', '-')}" for a in ANCHORS])
def test_anchor(anchor, shapes):
    *case, want = anchor
    got = dict(zip(FIELDS, (int(v) for v in _cases(shapes)[_arg(*case)])))
    assert {k: got[k] for k in want} == want, got


@pytest.mark.parametrize("case", REFUSED, ids=[f"{KNOBS[r[1]]}-{r[2]}-{r[3]}" for r in REFUSED])
def test_tile_major_refused(case, shapes):
    assert _cases(shapes)[_arg(*case, 1)] == ["unsupported"]
