"""Compiler resource report of the convolution translation units (no GPU needed): no kernel spills to scratch.

k_conv_mfma_sk (conv_mfma.h) reads the split partials of its tile with asm loads into "=v" outputs and waits for them in a
separate asm s_waitcnt: a spill between the two would store registers before the loads have written them.  The build
spills nothing today, but SK_ROWS, SK_OCC and the 96-register cap of that kernel are tuning knobs -- this test notices the
moment a retune makes the compiler spill, in that kernel or in any other of the two files.

A second pair of compiles with -DFRLW_DEV_BUILD checks that the developer library holds the same kernels as the product."""
import os
import re
import shutil
import subprocess

import pytest

from frlw_evd_amd import _build

FILES = ("detector.hip", "train_ops.hip")


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return exe if os.path.exists(exe) else None


def parse_resource_remarks(text):
    """{mangled kernel name: {field: value}} from -Rpass-analysis=kernel-resource-usage remarks (as tools/resusage.py reads them)."""
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass", line)
        if not m:
            continue
        s = m.group(1)
        if s.startswith("Function Name:"):
            cur = s.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur and ":" in s:
            k, v = s.split(":", 1)
            rows[cur][k.strip().split(" [")[0]] = v.strip()
    return rows


def test_parser_reads_the_remark_format():
    text = ("x.hip:1:1: remark: Function Name: _Z3fooPf [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hip:1:1: remark:     VGPRs: 12 [-Rpass-analysis=kernel-resource-usage]\n"
            "x.hip:1:1: remark:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]\n")
    assert parse_resource_remarks(text) == {"_Z3fooPf": {"VGPRs": "12", "ScratchSize": "16"}}


def _compile_with_remarks(exe, tmp_path, tag, extra):
    """Starts one hipcc per file of FILES (in parallel); {file: Popen}."""
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"] + list(extra) + ["-I", _build.INCLUDE, "-I", _build.CSRC, "-c",
                                                                               "-Rpass-analysis=kernel-resource-usage"]
    return {f: subprocess.Popen([exe] + flags + [os.path.join(_build.CSRC, f), "-o", str(tmp_path / (f + tag + ".o"))],
                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for f in FILES}


def _collect_remarks(procs):
    rows = {}
    for f, p in procs.items():
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-4000:]
        got = parse_resource_remarks(err)
        assert got, f"{f}: no resource remarks"
        rows.update(got)
    return rows


@pytest.fixture(scope="module")
def resource_rows(tmp_path_factory):
    """(product rows, developer-build rows) of the two files: four compiles side by side, once for the module."""
    exe = _hipcc()
    if exe is None:
        pytest.skip("hipcc not installed")
    tmp_path = tmp_path_factory.mktemp("resusage")
    product = _compile_with_remarks(exe, tmp_path, "", [])
    dev = _compile_with_remarks(exe, tmp_path, ".dev", ["-DFRLW_DEV_BUILD"])
    return _collect_remarks(product), _collect_remarks(dev)


def test_no_kernel_of_the_convolution_units_spills(resource_rows):
    rows, _ = resource_rows
    assert any("k_conv_mfma_sk" in name for name in rows), sorted(rows)
    assert any("k_wgrad_mfma" in name for name in rows), sorted(rows)
    missing = [name for name, r in rows.items() if "ScratchSize" not in r]
    assert not missing, missing
    spills = {name: r["ScratchSize"] for name, r in rows.items() if r["ScratchSize"] != "0"}
    assert not spills, spills


def test_developer_build_has_the_kernels_that_ship(resource_rows):
    """The developer library (-DFRLW_DEV_BUILD: environment knobs, logging, test hooks) is what GPU tests load in child processes:
    it must contain exactly the kernels of the product library -- no lab variant behind the macro -- and spill as little."""
    rows, dev = resource_rows
    assert set(dev) == set(rows), {"developer build only": sorted(set(dev) - set(rows)), "product only": sorted(set(rows) - set(dev))}
    missing = [name for name, r in dev.items() if "ScratchSize" not in r]
    assert not missing, missing
    spills = {name: r["ScratchSize"] for name, r in dev.items() if r["ScratchSize"] != "0"}
    assert not spills, spills
