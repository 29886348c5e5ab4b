"""tlab_amd/csrc/tlab_amd_conditional.h held to what tests/test_capi_symbols.py and tests/test_deferred_entry_points_host.py ask of
include/tlab_amd.h (no GPU, no compute call): the library exports every entry point the header declares, the ctypes table
tlab_amd.lib.CONDITIONAL_SIGNATURES lists exactly those, no name is also one of include/tlab_amd.h, every one is classified in
tests/conditional_entry_points.py, every one that enqueues work has a case that runs it with a record of the deferred tail pending
(tests/test_gpu_conditional.py: that GPU test is the check that a record runs first; here only the lists are held together), every one has a Fortran interface, and a C program compiles against the header alone."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import conditional_entry_points as E
import deferred_entry_points as D
import tlab_amd
from tlab_amd import lib as tl
from test_capi_symbols import declared_symbols

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "tlab_amd", "csrc", "tlab_amd_conditional.h")


def declared():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tlab_[a-z0-9_]+)\s*\(", text)))


def test_the_header_declares_the_seven_entry_points_and_none_of_the_main_header():
    assert len(declared()) == 7
    assert set(declared()) & set(declared_symbols()) == set()
    assert set(tl.CONDITIONAL_SIGNATURES) & set(tl.SIGNATURES) == set()
    assert '#include "../../include/tlab_amd.h"' in open(HEADER).read()


def test_library_exports_every_declared_symbol():
    L = ctypes.CDLL(tlab_amd.lib_path())
    assert not [n for n in declared() if not hasattr(L, n)]


def test_ctypes_table_matches_the_header_and_load_binds_it():
    assert set(declared()) == set(tl.CONDITIONAL_SIGNATURES)
    L = tlab_amd.load()
    for name, (res, args) in tl.CONDITIONAL_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_every_entry_point_is_classified_and_every_stream_one_has_a_pending_case():
    assert set(E.ENTRY_POINTS) == set(declared())
    assert set(E.ENTRY_POINTS.values()) <= {D.STREAM, D.HOST}
    assert set(E.ENTRY_POINTS) & (set(D.ENTRY_POINTS) | set(D.NOT_EXERCISED)) == set()
    src = open(os.path.join(ROOT, "tests", "test_gpu_conditional.py")).read()
    assert "def %s(" % E.PENDING_TEST in src
    cases = re.findall(r'@_entry\("(tlab_[a-z0-9_]+)"\)', src)
    assert sorted(cases) == sorted(n for n, c in E.ENTRY_POINTS.items() if c == D.STREAM), cases


def test_every_entry_point_has_a_fortran_interface():
    f90 = open(os.path.join(ROOT, "tlab_amd", "fortran", "tlab_amd_c.f90")).read()
    for name in declared():
        assert "bind(C, name='%s')" % name in f90, name


def test_a_c_program_compiles_against_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    (tmp_path / "use.c").write_text(
        '#include "tlab_amd_conditional.h"\n'
        "int use(const double *a, long long n, signed char *g) {\n"
        "    double thr[2] = {0.0, 1.0}, m[4] = {0.5, 1.0, 0.25, 2.0};\n"
        "    int rc = tlab_gate_levels(a, n, 3, thr, g);\n"
        "    return rc != TLAB_OK ? rc : tlab_raw_to_central(4, m);\n"
        "}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(tmp_path / "use.c"), "-o", str(tmp_path / "use.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
