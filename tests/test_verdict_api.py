"""The fire-verdict section of the C-ABI as the header declares it and as
cronsun_amd._lib binds it: the eight entry points, the two constants, the two
argument structs; CG_ABI_VERSION is still 3 (additions only).  No compute call
here."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")

ENTRY_POINTS = ["cg_expand_verdicts_device", "cg_verdicts_device", "cg_verdicts_copy", "cg_verdicts_select_device",
                "cg_verdicts_selected_device", "cg_verdicts_selected_copy_offsets",
                "cg_verdicts_selected_copy_times", "cg_verdict_times"]


def header():
    return open(HEADER).read()


def code():
    return re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)


def test_header_declares_the_section():
    txt = code()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
    assert re.search(r"#define\s+CG_VERDICT_DROPPED\s+1\b", txt)
    assert re.search(r"#define\s+CG_VERDICT_SKIPPED\s+2\b", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)
    flat = re.sub(r"\s+", " ", txt)
    assert ("typedef struct { const int64_t* dur_ms; const int64_t* parallels; const int32_t* unit; } "
            "cg_admit_args;") in flat
    assert ("typedef struct { const int32_t* kind; const int64_t* avg_time_ms; const int32_t* unit; "
            "const uint8_t* contends; int64_t lock_ttl; } cg_lock_args;") in flat
    proto = re.search(r"int cg_expand_verdicts_device\((.*?)\);", flat).group(1)
    assert [a.strip() for a in proto.split(",")] == [
        "cg_ctx* ctx", "const cg_specs* specs", "const cg_zone* z", "int64_t t0", "int64_t t1",
        "const cg_admit_args* admit", "const cg_lock_args* lock", "int64_t* n_events"]


def test_every_entry_cites_the_reference():
    """Each entry of the section sits under a comment that cites job.go lines."""
    txt = header()
    sec = txt[txt.index("fire verdicts ---"):txt.index("top rules of a bucket")]
    for name in ENTRY_POINTS + ["cg_admit_args;", "cg_lock_args;"]:
        at = sec.index(name + "(") if not name.endswith(";") else sec.index(name)
        comments = [m for m in re.finditer(r"/\*.*?\*/", sec[:at], flags=re.S)]
        assert comments and re.search(r"job\.go:\d+", comments[-1].group(0)), name


def test_lib_binds_the_section():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    assert (_lib.VERDICT_DROPPED, _lib.VERDICT_SKIPPED) == (1, 2)
    vp, i64, P = C.c_void_p, C.c_int64, C.POINTER
    want = {
        "cg_expand_verdicts_device": [vp, vp, vp, i64, i64, P(_lib.cg_admit_args), P(_lib.cg_lock_args), P(i64)],
        "cg_verdicts_device": [vp, P(vp), P(i64)],
        "cg_verdicts_copy": [vp, i64, i64, vp],
        "cg_verdicts_select_device": [vp, C.c_int, C.c_int, P(i64)],
        "cg_verdicts_selected_device": [vp, P(vp), P(vp), P(i64)],
        "cg_verdicts_selected_copy_offsets": [vp, vp],
        "cg_verdicts_selected_copy_times": [vp, i64, i64, vp],
        "cg_verdict_times": [vp, P(C.c_float), C.c_int],
    }
    assert sorted(want) == sorted(ENTRY_POINTS)
    for name, args in want.items():
        assert name in _lib.SYMBOLS
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is C.c_int, name
    # the structs are laid out as the header's: pointers in order, lock_ttl last
    assert [f[0] for f in _lib.cg_admit_args._fields_] == ["dur_ms", "parallels", "unit"]
    assert [f[0] for f in _lib.cg_lock_args._fields_] == ["kind", "avg_time_ms", "unit", "contends", "lock_ttl"]
    assert C.sizeof(_lib.cg_admit_args) == 24 and C.sizeof(_lib.cg_lock_args) == 40
    assert _lib.cg_lock_args.lock_ttl.offset == 32


def test_engine_and_model_have_the_interface():
    from cronsun_amd import engine, model
    for name in ("expand_verdicts", "expand_verdicts_device", "verdicts_device", "verdicts_copy", "verdicts_select",
                 "verdict_times"):
        assert callable(getattr(engine.Engine, name)), name
    for name in ("fire_verdicts", "node_failures"):
        assert callable(getattr(model.JobSet, name)), name
