"""PT_FLAG_KEEP_RENDERER -- a full pt_init that repeats the live renderer's own call with another pose moves the camera in place -- without a
GPU: the flag's value and its place among the others, the Python constant, the frozen export set, the shim's two switches in the host header,
and the comparison's answer where there is no renderer to compare with."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "pt_amd.h")


def _flags():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(PT_FLAG_[A-Z_]+)\s*=\s*(\d+)", open(HDR).read())}


def test_the_flag_is_2048():
    assert _flags()["PT_FLAG_KEEP_RENDERER"] == 2048


def test_every_flag_of_the_header_is_a_distinct_bit():
    flags = _flags()
    assert len(flags) >= 12
    for name, v in flags.items():
        assert v > 0 and v & (v - 1) == 0, name
    assert len(set(flags.values())) == len(flags)


def test_the_python_constants_equal_the_headers(pt):
    for name, v in _flags().items():
        assert getattr(pt, name) == v, name
    assert pt.PT_FLAG_KEEP_RENDERER == 2048
    assert "keep" in pt.pathtraceInit.__code__.co_varnames


def test_the_product_library_exports_exactly_the_headers_functions(pt):
    hdr = open(HDR).read()
    declared = set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    out = subprocess.run(["nm", "-D", "--defined-only", pt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared == set(pt.ABI_SYMBOLS)
    assert len(exported) == 47 and pt.PT_AMD_ABI_VERSION == 7 and "#define PT_AMD_ABI_VERSION 7\n" in hdr
    # the one entry this feature adds belongs to the test library
    assert "pt_test_keep_mismatch" in pt.TEST_ABI_SYMBOLS and "pt_test_keep_mismatch" not in exported


def test_the_host_header_declares_the_two_switches():
    h = open(os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pathtrace.h")).read()
    assert "void pathtraceKeepRenderer(bool on);" in h and "void pathtraceTemporal(bool on);" in h
    assert "HOLDS ITS DEVICE MEMORY" in h            # what a parked renderer costs, said where the host reads it
    assert "PT_AMD_KEEP_RENDERER" in h and "PT_AMD_TEMPORAL" in h
    shim = open(os.path.join(ROOT, "project3-cuda-path-tracer_amd", "host", "pathtrace_shim.cpp")).read()
    assert "PT_FLAG_KEEP_RENDERER" in shim and "pt_unpin_host" in shim


def test_a_flagged_call_that_is_refused_reports_no_move(pt):
    """no device needed: a NULL camera is refused by the full call's planning whether the flag is set or not, and the test library names
    the comparison that sent the call there"""
    import ctypes as C
    import numpy as np
    sc = pt.Scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    geoms, mats = np.ascontiguousarray(sc.geoms), np.ascontiguousarray(sc.materials)
    with pt.renderer_from_test_library():
        L = pt.lib()
        status = []
        for flags in (0, pt.PT_FLAG_KEEP_RENDERER):
            opt = pt.PtOptions(0, 1, -1, flags, 0, 0, None, None, 0.0, 0.0)
            status.append(L.pt_init(None, geoms.ctypes.data_as(C.c_void_p), len(geoms), mats.ctypes.data_as(C.c_void_p), len(mats), 4, C.byref(opt)))
        assert status[0] == status[1] == -1          # PT_ERR_INVALID
        assert pt.camera_move_info() == {"fast": None, "tables_uploaded": 0, "bytes_uploaded": 0}
        assert pt.keep_mismatch() == "no live renderer"
