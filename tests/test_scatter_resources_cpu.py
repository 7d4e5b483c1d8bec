"""Compiler resource report of taf_fast.hip (no GPU needed): no kf_scatter_cm instance spills to scratch.

kf_scatter_cm keeps a wavefront's whole run -- MAXB batches of events in flight, then a rank and a record word per batch --
in registers across phase A.  amdgpu_waves_per_eu caps the 20-batch form at 128 VGPRs (one 1024-thread workgroup per CU)
and the 8-batch form at 64 (two), so a decode change that grows the unrolled loop does not raise the VGPR count: the
compiler spills instead.  The scratch check is what catches that; the VGPR bounds only restate the cap."""
import os
import shutil
import subprocess

import pytest

from frlw_evd_amd import _build
from test_kernel_resources_cpu import parse_resource_remarks


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return exe if os.path.exists(exe) else None


def test_scatter_cm_instances_fit_without_scratch(tmp_path):
    exe = _hipcc()
    if exe is None:
        pytest.skip("hipcc not installed")
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"] + ["-I", _build.INCLUDE, "-I", _build.CSRC, "-c",
                                                                 "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run([exe] + flags + [os.path.join(_build.CSRC, "taf_fast.hip"), "-o", str(tmp_path / "taf_fast.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    rows = parse_resource_remarks(p.stderr)
    scat = {name: r for name, r in rows.items() if "kf_scatter_cm" in name}
    # Itanium mangling of the MAXB template argument: ...ELi20E... / ...ELi8E...
    big = {name: r for name, r in scat.items() if "ELi20E" in name}
    small = {name: r for name, r in scat.items() if "ELi8E" in name}
    assert big and small, sorted(scat)
    for name, r in scat.items():
        assert r.get("ScratchSize") == "0", (name, r)
    for name, r in big.items():
        assert int(r["VGPRs"]) <= 128, (name, r["VGPRs"])
    for name, r in small.items():
        assert int(r["VGPRs"]) <= 64, (name, r["VGPRs"])
    # the form the headline encode runs (TAF, SIMPLE decode, 20 batches) is among them
    assert any("kf_scatter_cmILb0ELb0ELb1ELi20ELi0E" in name for name in big), sorted(big)
