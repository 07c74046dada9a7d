"""make_split / run_range (csrc/run_split.h, which holds every run kernel's bounds: the others are in test_run_bounds_cpu.py): how a launch's tiles become the runs of k_run256v2 and k_run256_dcfix.  No GPU needed.

A small stand-alone program includes the header, makes one split per command-line case and prints every run's range twice: as
run_range gives it, and as the FM kernels use it (their pair_align rounding: starts and inner ends rounded down to even tiles).
It is built with the host compiler, once plain and once with -fsanitize=address,undefined; both builds must print the same.

What is asserted for every shape: the runs cover [0, nb) exactly once, run w + 1 behind run w; every start (as the kernels use
it) is even; every run has at least 8 tiles.  On the weighted path (nruns = slots x cus, one class per co-resident workgroup of a
CU, whole tile pairs) also: the kernels' rounding changes nothing; all runs of the oldest and of the youngest class have one
length; middle-class runs are within one pair of each other; the sums over a CU's runs (c, c + cus, c + 2 cus) are within one pair
across CUs.

An odd last tile: run w + 1 starts where run w ends (the runs hand their DC state on in that order), so a class with an odd
number of tiles in the middle of the launch would make every later start odd.  The split therefore gives the odd last tile to the
launch's last run -- the last run of the youngest class -- and the equal-length and per-CU assertions below are made on the lengths
without that one tile."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

PROGRAM = r"""
#include "run_split.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
// argv: one case per argument, "nb:nruns:cus:w0,w1,..[:p0,p1,..]"
int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        unsigned nb = 0, nruns = 0, cus = 0;
        char ws[256] = "", ps[256] = "";
        if (sscanf(argv[a], "%u:%u:%u:%255[^:]:%255s", &nb, &nruns, &cus, ws, ps) < 4) return 2;
        float w[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int k = 0;
        for (char *t = strtok(ws, ","); t && k < 8; t = strtok(nullptr, ","), k++) w[k] = (float)atof(t);
        k = 0;
        for (char *t = strtok(ps, ","); t && k < 8; t = strtok(nullptr, ","), k++) p[k] = (uint32_t)atol(t);
        const csdr::RunSplit sp = csdr::make_split(nb, nruns, cus, w, ps[0] ? p : nullptr);
        printf("case %s rps %u nslots %u shift %u\n", argv[a], sp.rps, sp.nslots, sp.shift);
        for (unsigned r = 0; r < nruns; r++) {
            uint32_t f, l;
            csdr::run_range(sp, r, f, l);
            uint32_t fa = f & ~1u, la = l != nb ? l & ~1u : l;
            printf("%u %u %u %u\n", f, l, fa, la);
        }
    }
    return 0;
}
"""

FM3 = "1.6,1,0.6"          # the shipped shares of the three workgroups of a CU (kernels_fused.hip v2_weight_fm3), two per CU below
FM2 = "1.24,0.76"
# (nb, nruns, cus, weights, pair counts or None, path expected)
CASES = [
    (16384, 768, 256, FM3, None, "weighted"),
    (16384, 512, 256, FM2, None, "weighted"),
    (16385, 768, 256, FM3, None, "weighted"),            # an odd tile
    (16384 + 2 * 37, 768, 256, FM3, None, "weighted"),   # pairs that do not divide
    (16385 + 2 * 37, 768, 256, FM3, None, "weighted"),
    (16384 + 2 * 37, 512, 256, FM2, None, "weighted"),   # two classes: the older one takes what does not divide
    (12288, 768, 256, FM3, None, "weighted"),            # (12, 8, 4) pairs: the youngest class at the floor of 8 tiles
    (11264, 768, 256, FM3, None, "weighted"),            # (11, 7, 4)
    (6144, 768, 256, FM3, None, "uniform"),              # (6, 4, 2): the youngest class would have 4 tiles
    (11264, 768, 256, "2,1,0.4", None, "uniform"),       # (13, 6, 3)
    (16384, 912, 304, FM3, None, "weighted"),            # 26 pairs per CU and 288 left over
    (16385, 912, 304, FM3, None, "weighted"),
    (16384, 192, 64, FM3, None, "weighted"),
    (2816 + 2 * 5 + 1, 192, 64, FM3, None, "weighted"),  # 22 pairs per CU: (11, 7, 4)
    (16384, 700, 256, FM3, None, "uniform"),             # nruns no multiple of cus
    (25, 3, 256, FM3, None, "uniform"),                  # [0, 8) [8, 16) [16, 25): tests/test_run256_occ3_gpu.py
    (16384, 768, 256, FM3, "16,10,6", "weighted"),       # pair counts given outright
    (16384, 768, 256, FM3, "16,10,5", "weighted"),       # ... ignored when they do not sum to the pairs of a CU
    (16384, 768, 256, "1,1,1", None, "weighted"),        # the equal split the GPU test compares with
]


def _arg(c):
    nb, nruns, cus, w, p, _ = c
    return f"{nb}:{nruns}:{cus}:{w}" + (f":{p}" if p else "")


def _build(tmp, name, extra):
    src = tmp / "split_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    out = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "composable_sdr_amd", "csrc"),
                          str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def _parse(text):
    res, cur = {}, None
    for ln in text.splitlines():
        if ln.startswith("case "):
            t = ln.split()
            cur = {"rps": int(t[3]), "nslots": int(t[5]), "shift": int(t[7]), "runs": []}
            res[t[1]] = cur
        else:
            cur["runs"].append(tuple(int(v) for v in ln.split()))
    return res


@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("run_split")
    args = [_arg(c) for c in CASES]
    plain = subprocess.run([str(_build(tmp, "split_plain", [])), *args], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr[-3000:]
    san = subprocess.run([str(_build(tmp, "split_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])), *args],
                         capture_output=True, text=True, timeout=120)
    assert san.returncode == 0, san.stderr[-3000:]
    return _parse(plain.stdout), plain.stdout, san.stdout


def test_sanitized_build_prints_the_same(splits):
    _, plain, san = splits
    assert plain == san


@pytest.mark.parametrize("case", CASES, ids=[_arg(c).replace(":", "-") for c in CASES])
def test_split(case, splits):
    nb, nruns, cus, _, pairs, path = case
    sp = splits[0][_arg(case)]
    runs = sp["runs"]
    assert len(runs) == nruns
    weighted = sp["nslots"] > 1
    assert ("weighted" if weighted else "uniform") == path, sp
    # what the kernels use: cover, even starts, >= 8 tiles
    pos = 0
    for w, (f, l, fa, la) in enumerate(runs):
        assert fa == pos and la > fa, (w, runs[w])
        assert fa % 2 == 0, (w, runs[w])
        assert la - fa >= 8, (w, runs[w])
        pos = la
    assert pos == nb
    # run_range itself: the same cover (the FM kernels' rounding moves boundaries of the uniform split only)
    pos = 0
    for w, (f, l, _, _) in enumerate(runs):
        assert f == pos and l >= f, (w, runs[w])
        pos = l
    assert pos == nb
    if not weighted:
        assert sp["shift"] == 0 and sp["rps"] == nruns
        return
    slots = nruns // cus
    assert sp["rps"] == cus and sp["nslots"] == slots and sp["shift"] == 1
    assert all((f, l) == (fa, la) for f, l, fa, la in runs), "the kernels' pair rounding must be a no-op on the weighted path"
    length = [l - f for f, l, _, _ in runs]
    length[-1] -= nb & 1                                # the odd last tile rides on the launch's last run (module docstring)
    assert all(n % 2 == 0 for n in length)
    cls = [length[k * cus:(k + 1) * cus] for k in range(slots)]
    mid = (slots - 1) // 2
    for k in range(slots):
        spread = max(cls[k]) - min(cls[k])
        assert spread <= (2 if k == mid else 0), (k, min(cls[k]), max(cls[k]))
    assert len(set(cls[-1])) == 1 and (slots == 2 or len(set(cls[0])) == 1)     # (two classes have no middle: the older one is `mid`)
    per_cu = [sum(cls[k][c] for k in range(slots)) for c in range(cus)]
    assert max(per_cu) - min(per_cu) <= 2, (min(per_cu), max(per_cu))
    assert sum(per_cu) == nb - (nb & 1)
    if (nb // 2) % cus == 0:
        assert len(set(per_cu)) == 1 and all(len(set(c)) == 1 for c in cls)
    if pairs and sum(int(v) for v in pairs.split(",")) == nb // 2 // cus:
        assert [c[0] for c in cls] == [2 * int(v) for v in pairs.split(",")]


def test_bench_shape_is_one_triple_on_every_cu(splits):
    """nb = 16384 on 256 CUs, three workgroups per CU: every CU holds the same three run lengths, 64 tiles in all"""
    runs = splits[0][_arg(CASES[0])]["runs"]
    triples = {tuple(runs[c + 256 * k][1] - runs[c + 256 * k][0] for k in range(3)) for c in range(256)}
    assert len(triples) == 1, triples
    t = triples.pop()
    assert sum(t) == 64 and t[0] > t[1] > t[2] >= 8, t
    assert t == (32, 20, 12), t
