"""The ctypes binding (codonlm_amd/_lib.py) against include/codonlm_hip.h: field names, order and
kinds of every struct mirror, every prototype's argument and return kinds, every enumerator and
integer define with a twin.  A size check alone (test_abi_cpu.py) cannot see two swapped
same-width fields or a miscounted argument list."""
import pytest

from header_reader import ctypes_kind, read_header


@pytest.fixture(scope="module")
def hdr():
    return read_header()


@pytest.fixture(scope="module")
def L():
    from codonlm_amd import _lib
    return _lib


def test_struct_fields_match_the_header(hdr, L):
    assert len(hdr["structs"]) >= 25 and set(L.STRUCTS) == set(hdr["structs"])
    for name, fields in hdr["structs"].items():
        mirror = [(f, ctypes_kind(t, L.STRUCTS)) for f, t in L.STRUCTS[name]._fields_]
        assert mirror == fields, name


def test_prototypes_match_the_header(hdr, L):
    assert len(hdr["protos"]) >= 114 and set(L.SIGNATURES) == set(hdr["protos"])
    for name, (ret, args) in hdr["protos"].items():
        res, argtypes = L.SIGNATURES[name]
        assert [ctypes_kind(t, L.STRUCTS) for t in argtypes] == args, name
        assert ctypes_kind(res, L.STRUCTS) == ret, name


# every member of these groups has a twin
GROUPS = ("CG_EPI_", "CG_TILE_", "CG_P_", "CG_PROBE_", "CG_TOK_", "CG_GEN_", "CG_ATTR_", "CG_AS_", "CG_DIAG_CLS_")
# the enumerators that index L.DIAG_SLICES, under the reference's report names (four of them begin
# with CG_DIAG_CLS_ and are slices, not class codes)
SLICES = {"CG_DIAG_ALL": "all", "CG_DIAG_AFTER_SEP": "after_separator",
          "CG_DIAG_FLAG_SET": "window_with_chunk_continuation", "CG_DIAG_FLAG_CLEAR": "window_without_chunk_continuation",
          "CG_DIAG_POS_0": "segment_position_0", "CG_DIAG_POS_1_3": "segment_position_1_3",
          "CG_DIAG_POS_4_15": "segment_position_4_15", "CG_DIAG_POS_16_63": "segment_position_16_63",
          "CG_DIAG_POS_64_PLUS": "segment_position_64_plus", "CG_DIAG_CLS_SPECIAL_SLICE": "target_class_special",
          "CG_DIAG_CLS_START_SLICE": "target_class_start_codon", "CG_DIAG_CLS_STOP_SLICE": "target_class_stop_codon",
          "CG_DIAG_CLS_ORDINARY_SLICE": "target_class_ordinary_codon"}
CODES = ("CG_F32", "CG_BF16", "CG_BF16X2", "CG_OK", "CG_EINVAL", "CG_EUNSUPPORTED", "CG_ELAUNCH")


def _twin(L, name):
    """The value _lib gives a header constant: the status and dtype codes under their full name, every
    other one without the CG_ prefix; None = no twin."""
    return getattr(L, name if name in CODES else name[len("CG_"):], None)


def test_enumerators_match_the_header(hdr, L):
    enumerators = {k: v for block in hdr["enums"] for k, v in block.items()}
    assert len(enumerators) >= 100 and set(CODES) <= set(enumerators)
    seen = dict.fromkeys(GROUPS, 0)
    for name, value in enumerators.items():
        group = next((g for g in GROUPS if name.startswith(g) and name not in SLICES), None)
        if group:
            seen[group] += 1
        if group or name in CODES:
            assert _twin(L, name) is not None, f"{name} has no twin in _lib"
        if isinstance(_twin(L, name), int):
            assert _twin(L, name) == value, name
    assert all(seen.values()), seen
    # the name tuples are indexed by enumerator: same length, same order
    assert len(L.DIAG_SLICES) == enumerators["CG_DIAG_SLICES"] == len(SLICES)
    for name, report in SLICES.items():
        assert L.DIAG_SLICES[enumerators[name]] == report, name
    stats = {k: v for k, v in enumerators.items() if k.startswith("CG_AS_") and k != "CG_AS_NSTAT"}
    assert len(L.AS_STATS) == enumerators["CG_AS_NSTAT"] == L.AS_NSTAT == len(stats)
    for name, value in stats.items():
        assert L.AS_STATS[value] == name[len("CG_AS_"):].lower(), name


def test_defines_match_the_header(hdr, L):
    assert len(hdr["defines"]) >= 10
    for name, value in hdr["defines"].items():
        assert _twin(L, name) == value, name
