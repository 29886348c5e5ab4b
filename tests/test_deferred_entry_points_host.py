"""tests/deferred_entry_points.py against the header and against the GPU cases (no GPU, no compute call): every entry point of include/tlab_amd.h
says how it relates to a pending record of the deferred tail, and every one that enqueues work or changes what a replay reads is either run with
a record pending (tests/test_gpu_deferred_entry_points.py) or listed with the reason why not."""
import deferred_entry_points as E
from test_capi_symbols import declared_symbols
from test_gpu_deferred_entry_points import CASES

CLASSES = {E.STREAM, E.SETTER, E.DEFERRED, E.LIFETIME, E.HOST, E.DECOMPOSED}
# the operator entry points of csrc/operators.cpp that used to take the stream without a flush
CAPI = ["tlab_opr_partial", "tlab_opr_partial_add", "tlab_opr_burgers", "tlab_opr_burgers_add", "tlab_opr_burgers_add_n", "tlab_opr_gradient_final",
        "tlab_boundary_bcs_neumann_y", "tlab_transpose"]
ALWAYS_EXERCISED = ["tlab_device_minmax", "tlab_time_courant", "tlab_dns_dilatation_extremes", "tlab_dns_pressure", "tlab_dns_diagnostic", "tlab_dns_filter",
                    "tlab_avg1v2d_v", "tlab_fluctuation", "tlab_cross_product", "tlab_vorticity_from_gradients"]
ALWAYS_EXERCISED_PREFIXES = ("tlab_pw_", "tlab_zslab_", "tlab_opr_filter", "tlab_fi_", "tlab_minmax")


def _of(cls):
    return sorted(n for n, c in E.ENTRY_POINTS.items() if c == cls)


def test_the_table_lists_exactly_the_symbols_of_the_header():
    decl, table = set(declared_symbols()), set(E.ENTRY_POINTS)
    assert decl - table == set(), "declared in include/tlab_amd.h but without a row in tests/deferred_entry_points.py: %s" % sorted(decl - table)
    assert table - decl == set(), "a row in tests/deferred_entry_points.py but not declared in include/tlab_amd.h: %s" % sorted(table - decl)
    bad = {n: c for n, c in E.ENTRY_POINTS.items() if c not in CLASSES}
    assert not bad, "unknown class: %s" % bad


def test_the_classes_hold_what_their_names_say():
    assert all(n.startswith("tlab_deferred_") for n in _of(E.DEFERRED))
    assert [n for n in E.ENTRY_POINTS if n.startswith("tlab_deferred_") and E.ENTRY_POINTS[n] != E.DEFERRED] == []
    assert all(n.startswith(("tlab_slab_", "tlab_pencil_dns_")) for n in _of(E.DECOMPOSED))
    for n in E.ENTRY_POINTS:
        if n.endswith(("_create", "_destroy")) or "_plan_create" in n or n in ("tlab_init", "tlab_finalize", "tlab_malloc", "tlab_free"):
            assert E.ENTRY_POINTS[n] == E.LIFETIME, n
    for n in CAPI + ALWAYS_EXERCISED:
        assert E.ENTRY_POINTS[n] == E.STREAM, n


def test_every_stream_and_setter_entry_has_a_case_or_a_reason():
    need = set(_of(E.STREAM)) | set(_of(E.SETTER))
    missing = sorted(need - set(CASES) - set(E.NOT_EXERCISED))
    assert not missing, "stream / setter entry points with neither a case in tests/test_gpu_deferred_entry_points.py nor a reason in NOT_EXERCISED: %s" % missing
    both = sorted(set(CASES) & set(E.NOT_EXERCISED))
    assert not both, "listed as not exercised but a case exists: %s" % both
    stray = sorted(set(CASES) - need)
    assert not stray, "cases for names that are neither stream nor setter: %s" % stray


def test_not_exercised_stays_small_and_away_from_what_must_be_run():
    ne = E.NOT_EXERCISED
    assert all(isinstance(r, str) and len(r.strip()) >= 20 for r in ne.values()), "every entry carries its reason"
    unknown = sorted(n for n in ne if E.ENTRY_POINTS.get(n) not in (E.STREAM, E.SETTER))
    assert not unknown, "NOT_EXERCISED holds names that are neither stream nor setter: %s" % unknown
    # only entries whose set-up needs an object the GPU file does not otherwise build -- but for the departures the table declares by name
    tag = {n: r.split(":", 1)[0] for n, r in ne.items()}
    assert sorted(n for n, t in tag.items() if t == "departure") == sorted(E.DEPARTURES), tag
    other = {n: t for n, t in tag.items() if t != "departure" and t not in E.OBJECTS}
    assert not other, "NOT_EXERCISED reasons that name none of %s: %s" % (E.OBJECTS, other)
    assert not [n for n in CAPI + ALWAYS_EXERCISED if n in ne]
    assert not [n for n in ne if n.startswith(ALWAYS_EXERCISED_PREFIXES)]
    assert 4 * len(ne) <= len(_of(E.STREAM)), (len(ne), len(_of(E.STREAM)))
