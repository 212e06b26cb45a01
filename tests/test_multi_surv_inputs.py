"""CPU suite for several surveillance channels per reference (blah2hip_amb_process_multi_dev): the header declares the
entry points, the cap and the new constants, the ctypes table mirrors them with the same arity, and the new option /
range-kernel values collide with none that existed."""
import os
import re

from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "blah2hip.h")).read()


def defines(prefix):
    """{name: value} of the header's integer #defines whose name starts with ``prefix``."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (%s\w*) +\(?(-?\d+)\)?" % prefix, HEADER, re.M)}


def prototype_arity(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, HEADER, re.M | re.S)
    assert m, f"{name} is not declared in include/blah2hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_the_multi_entry_points():
    assert prototype_arity("blah2hip_amb_process_multi_dev") == 10
    assert prototype_arity("blah2hip_amb_process_multi_c32") == 7
    m = re.search(r"^int blah2hip_amb_process_multi_dev\(([^;]*)\);", HEADER, re.M | re.S)
    args = " ".join(m.group(1).split())
    assert "const void *const *d_y, uint32_t n_surv, uint32_t n_cpi, uint64_t cpi_stride" in args
    assert defines("BLAH2HIP_MAX_SURV") == {"BLAH2HIP_MAX_SURV": 8}
    assert defines("BLAH2HIP_MULTI_") == {"BLAH2HIP_MULTI_AUTO": 0, "BLAH2HIP_MULTI_SHARED": 1, "BLAH2HIP_MULTI_PER_CHANNEL": 2}


def test_new_values_collide_with_no_existing_one():
    opts = defines("BLAH2HIP_OPT_")
    assert opts["BLAH2HIP_OPT_MULTI_SURV_RANGE"] == 11
    assert len(set(opts.values())) == len(opts), opts
    assert sorted(opts.values()) == list(range(1, 12))  # the next free value, no gap
    ranges = defines("BLAH2HIP_RANGE_")
    assert ranges["BLAH2HIP_RANGE_SHARED"] == 8
    assert len(set(ranges.values())) == len(ranges), ranges
    assert 4 not in ranges.values()  # the retired BLAH2HIP_RANGE_WAVE2 stays retired
    infos = defines("BLAH2HIP_INFO_")
    assert len(set(infos.values())) == len(infos), infos
    # no new sample format: the set tests/test_i8_capture.py pins
    assert sorted(defines("BLAH2HIP_FMT_").values()) == [0, 1, 2, 3, 4, 5]


def test_ctypes_table_matches_the_header(built_lib):
    import ctypes as C

    from blah2_amd import _lib
    for name in ("blah2hip_amb_process_multi_dev", "blah2hip_amb_process_multi_c32"):
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == prototype_arity(name), name
        fn = getattr(built_lib, name)  # exported by the built library
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args)
    assert _lib.OPT_MULTI_SURV_RANGE == defines("BLAH2HIP_OPT_")["BLAH2HIP_OPT_MULTI_SURV_RANGE"]
    assert _lib.RANGE_SHARED == defines("BLAH2HIP_RANGE_")["BLAH2HIP_RANGE_SHARED"]
    assert _lib.MAX_SURV == 8
    assert (_lib.MULTI_AUTO, _lib.MULTI_SHARED, _lib.MULTI_PER_CHANNEL) == (0, 1, 2)
    py_opts = [v for k, v in vars(_lib).items() if k.startswith("OPT_")]
    assert len(set(py_opts)) == len(py_opts)
    py_ranges = [v for k, v in vars(_lib).items() if k.startswith("RANGE_")]
    assert len(set(py_ranges)) == len(py_ranges)


def test_ambiguity_class_has_the_multi_methods(built_lib):
    import blah2_amd
    for name in ("process_multi_dev", "process_multi", "set_multi_surv_range"):
        assert callable(getattr(blah2_amd.Ambiguity, name))
