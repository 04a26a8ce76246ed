"""CPU suite: the C-ABI library builds for gfx950, loads, exports every symbol include/moihgp.h declares,
and fails loudly (no fallback) without a GPU.  No compute calls here."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "moihgp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b((?:gp32|gp52|moihgp)_[a-zA-Z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_header_declares_reference_abi():
    names = _declared_symbols()
    for pfx in ("gp32", "gp52"):          # reference src/wrapper.cpp:31-326, :329-624: 13 symbols per prefix
        for n in ("new", "del", "step1", "step2", "step3", "step4", "update", "lik1", "lik2", "get_params",
                  "igp_dim", "num_param", "num_igp_param"):
            assert f"{pfx}_{n}" in names
    assert len([n for n in names if n.startswith(("gp32_", "gp52_"))]) == 26


def test_library_exports_every_declared_symbol(hip_built):
    lib = C.CDLL(hip_built)
    missing = [n for n in _declared_symbols() if not hasattr(lib, n)]
    assert not missing, missing


def test_python_loader_lists_match_header(hip_built):
    from multioutputihgp_amd import _lib
    assert sorted(_lib.REFERENCE_SYMBOLS + _lib.ADDITIVE_SYMBOLS) == _declared_symbols()
    _lib.load_library()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "multioutputihgp_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", "Makefile")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("oracle/README.md", ""), f"{f} references the oracle"


def test_fails_loudly_without_gpu(hip_built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from multioutputihgp_amd import MOIHGP, MoihgpError, load_library
    lib = load_library()
    assert lib.moihgp_device_count() == 0
    with pytest.raises(MoihgpError) as ei:
        MOIHGP(0.1, 4, 2)
    assert "no usable HIP device" in str(ei.value) and "no CPU fallback" in str(ei.value)
    from multioutputihgp_amd.streams import LatentBank
    with pytest.raises(MoihgpError):
        LatentBank(0.1, [[1.0, 1.0, 0.1]])


def test_reference_pywrapper_binds_only_symbols_we_export(hip_built):
    """Every `gpXX_*` attribute the reference's ctypes class resolves (moihgp/pywrapper.py:28-83, stored as
    tests/golden/reference_pywrapper_symbols.json) must be exported by our library."""
    import json
    names = set(json.load(open(os.path.join(ROOT, "tests", "golden", "reference_pywrapper_symbols.json")))["symbols"])
    assert len(names) == 26
    lib = C.CDLL(hip_built)
    assert all(hasattr(lib, n) for n in names)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No HIP library -> no product: the loader raises instead of falling back to anything."""
    from multioutputihgp_amd import _lib
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "_HERE", str(tmp_path))
    with pytest.raises(_lib.MoihgpError) as ei:
        _lib.load_library()
    assert "no CPU fallback" in str(ei.value)


def test_no_dpp_hazard_in_device_code(hip_built):
    """The broadcast FMAs of recursion_x.hip and grad_scan_x.hip are inline-asm DPP instructions: the compiler does not guard those
    against the GFX9 "VALU writes a VGPR, DPP reads it within two issue slots" hazard, so the built gfx950 code is scanned for it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_dpp_hazard", os.path.join(ROOT, "tools", "check_dpp_hazard.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    for obj in ("recursion_x_21.o", "recursion_x_31.o", "recursion_x_22.o", "recursion_x_23.o", "recursion_x_24.o", "recursion_x_32.o", "recursion_x_33.o", "recursion_x_34.o", "grad_scan_x.o"):
        hazards, ndpp = mod.scan(mod.disassemble(os.path.join(ROOT, "build", "obj", obj)))
        assert ndpp > 1000 and hazards == [], (obj, hazards[:5])
