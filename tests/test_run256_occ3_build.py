"""What k_run256v2<FM, 1> must compile to for three workgroups per CU (no GPU needed: hipcc cross-compiles).

A CU has 512 registers per lane and SIMD and 160 KiB of LDS: three workgroups of four waves need at most 168 VGPRs per wave and at most
163840 / 3 = 54613 bytes of LDS each, and the asm DMA / stores of the kernel tolerate neither SGPR spills (fused_v2_common.h) nor scratch
traffic in the tile loop.  The seven other instantiations keep the two-buffer form: two workgroups per CU, 73984 bytes of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _field(block, name):
    return int(re.search(re.escape(name) + r": (\d+)", block).group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_run256v2_fm_fits_three_workgroups_per_cu(tmp_path):
    src = os.path.join(ROOT, "composable_sdr_amd", "csrc", "kernels_fused_v2.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", str(tmp_path / "v2.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = {}
    for b in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        m = re.search(r"k_run256v2ILb([01])ELi(\d)E", b.splitlines()[0])
        if m:
            blocks[(m.group(1) == "1", int(m.group(2)))] = b
    assert sorted(blocks) == [(fm, g) for fm in (False, True) for g in (1, 2, 4, 8)]
    one = blocks.pop((True, 1))
    assert _field(one, "Occupancy [waves/SIMD]") == 3, one[:800]
    assert _field(one, "VGPRs") <= 168
    assert _field(one, "VGPRs Spill") == 0 and _field(one, "SGPRs Spill") == 0, one[:800]
    assert _field(one, "ScratchSize [bytes/lane]") == 0, one[:800]
    assert _field(one, "LDS Size [bytes/block]") <= 54613
    for key, b in blocks.items():
        assert _field(b, "Occupancy [waves/SIMD]") == 2, (key, b[:800])
        assert _field(b, "LDS Size [bytes/block]") == 73984, (key, b[:800])
        assert _field(b, "SGPRs Spill") == 0, (key, b[:800])
        assert _field(b, "VGPRs Spill") <= (0 if key[1] == 1 else 4), (key, b[:800])
