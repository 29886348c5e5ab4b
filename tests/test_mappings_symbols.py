"""tlab_amd/csrc/tlab_amd_mappings.h held to what tests/test_capi_symbols.py and tests/test_deferred_entry_points_host.py ask of
include/tlab_amd.h (no GPU, no compute call): the library exports every entry point the header declares, the ctypes table
tlab_amd.lib.MAPPINGS_SIGNATURES lists exactly those, no name is also one of include/tlab_amd.h or of tlab_amd_conditional.h, every one is
classified in tests/mappings_entry_points.py, every one that enqueues work has a case that runs it with a record of the deferred tail pending
(tests/test_gpu_mappings.py: that GPU test is the check that a record runs first; here only the lists are held together), every one has a
Fortran interface, the header says what is refused and what is not built, and a C program compiles against the header alone."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import deferred_entry_points as D
import mappings_entry_points as E
import tlab_amd
from tlab_amd import lib as tl
from test_capi_symbols import declared_symbols

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "tlab_amd", "csrc", "tlab_amd_mappings.h")


def declared():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tlab_[a-z0-9_]+)\s*\(", text)))


def test_the_header_declares_the_five_entry_points_and_none_of_the_other_headers():
    assert len(declared()) == 5
    assert set(declared()) & set(declared_symbols()) == set()
    assert set(tl.MAPPINGS_SIGNATURES) & (set(tl.SIGNATURES) | set(tl.CONDITIONAL_SIGNATURES)) == set()
    assert '#include "../../include/tlab_amd.h"' in open(HEADER).read()


def test_library_exports_every_declared_symbol():
    L = ctypes.CDLL(tlab_amd.lib_path())
    assert not [n for n in declared() if not hasattr(L, n)]


def test_ctypes_table_matches_the_header_and_load_binds_it():
    assert set(declared()) == set(tl.MAPPINGS_SIGNATURES)
    L = tlab_amd.load()
    for name, (res, args) in tl.MAPPINGS_SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_every_entry_point_is_classified_and_every_stream_one_has_a_pending_case():
    assert set(E.ENTRY_POINTS) == set(declared())
    assert set(E.ENTRY_POINTS.values()) <= {D.STREAM, D.HOST}
    assert set(E.ENTRY_POINTS) & (set(D.ENTRY_POINTS) | set(D.NOT_EXERCISED)) == set()
    src = open(os.path.join(ROOT, "tests", "test_gpu_mappings.py")).read()
    assert "def %s(" % E.PENDING_TEST in src
    cases = re.findall(r'@_entry\("(tlab_[a-z0-9_]+)"\)', src)
    assert sorted(cases) == sorted(n for n, c in E.ENTRY_POINTS.items() if c == D.STREAM), cases


def test_every_entry_point_runs_a_pending_record_through_the_one_guard():
    """each body is flushed(...) of errors.hpp: the record first, then the one exception guard"""
    src = open(os.path.join(ROOT, "tlab_amd", "csrc", "mappings.cpp")).read()
    for name in declared():
        body = src[src.index("int %s(" % name):]
        assert re.match(r"int %s\([^)]*\)\s*\{\s*return flushed\(\[&\]" % name, body), name


def test_every_entry_point_has_a_fortran_interface():
    f90 = open(os.path.join(ROOT, "tlab_amd", "fortran", "tlab_amd_c.f90")).read()
    for name in declared():
        assert "bind(C, name='%s')" % name in f90, name


def test_the_header_states_what_is_refused_and_what_is_not_built():
    text = open(HEADER).read()
    for word in ("TLAB_EUNSUPPORTED", "staggered", "slab", "pencil", "immersed", "FI_DISSIPATION", "FI_VORTICITY_BAROCLINIC", "FI_SOLENOIDAL",
                 "FI_ISOSURFACE", "TENSOR_EIGEN", "opt_main = 9"):
        assert word in text, word


def test_a_c_program_compiles_against_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    (tmp_path / "use.c").write_text(
        '#include "tlab_amd_mappings.h"\n'
        "int use(long long n, const double *const *du9, double *const *out, tlab_dns_t d, double *const *q, double *const *w6) {\n"
        "    int maps[2] = {TLAB_MAP_Q, TLAB_MAP_CURL};\n"
        "    int rc = tlab_gradient_maps(n, du9, 0, maps, 2, out);\n"
        "    return rc != TLAB_OK ? rc : tlab_dns_fi_diffusion(d, TLAB_FI_VORTICITY_DIFFUSION, q, 0, out[0], w6);\n"
        "}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(tmp_path / "use.c"), "-o", str(tmp_path / "use.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
