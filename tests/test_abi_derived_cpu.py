"""The Python binding of the C ABI is read from include/mcm.h (mcm_amd/abi.py).  tests/golden/abi_prototypes.json holds what the
package bound while every prototype, symbol list, struct mirror and constant was still written out by hand in engine.py, config.py
and detection.py (recorded by tests/golden/make_abi_prototypes.py at that commit): what the header gives must equal it.  And what
the parser refuses: a type it does not know, in a declaration or in a struct, and a library that lacks a declared symbol.
No test here needs a GPU; the compute entries are declared, never called."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_prototypes.json")
NOT_INT = {"mcm_destroy": None, "mcm_tokenizer_destroy": None, "mcm_last_error": "c_char_p", "mcm_tokenizer_last_error": "c_char_p"}


def type_name(t):
    """A ctypes type as the fixture writes it: None (void), c_char_p, c_void_p for every other pointer type, a scalar by its
    sized name (c_int is c_int32 here), an array as "c_int32*3"."""
    if t is None:
        return None
    if t is ctypes.c_char_p:
        return "c_char_p"
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "c_void_p"
    if issubclass(t, ctypes.Array):
        return f"{type_name(t._type_)}*{t._length_}"
    return next(n for n in ("c_int32", "c_int64", "c_uint8", "c_uint16", "c_uint32", "c_uint64", "c_float", "c_double")
                if getattr(ctypes, n) is t)


def _proto(restype, argtypes):
    return {"restype": type_name(restype), "argtypes": [type_name(t) for t in argtypes or []]}


class _Function:
    restype, argtypes = ctypes.c_int, None  # what ctypes assumes of a function nobody declared

    def __call__(self, *args):  # only mcm_abi_version is called while the library is loaded
        from mcm_amd.config import ABI_VERSION

        return ABI_VERSION


class _Library:
    """Stands where ctypes.CDLL does and keeps what is declared on it; nothing native is loaded."""

    def __init__(self, path):
        self.functions = {}

    def __getattr__(self, name):
        if not name.startswith("mcm_"):
            raise AttributeError(name)
        return self.functions.setdefault(name, _Function())


def bound():
    """What the package binds, as the fixture holds it: the prototypes engine.load_library declares on the harness library
    (every product and every harness entry), both symbol lists, the constants and the two struct mirrors."""
    from mcm_amd import config, detection, engine

    try:  # load_library imports torch first, and torch loads its own libraries with ctypes.CDLL: before the recorder stands there
        import torch  # noqa: F401
    except ImportError:
        pass
    saved = ctypes.CDLL, engine.LIB_PATH, engine.HARNESS_LIB_PATH, dict(engine._libs)
    ctypes.CDLL, engine.LIB_PATH, engine.HARNESS_LIB_PATH = _Library, __file__, __file__
    engine._libs.clear()
    try:
        declared = engine.load_library(harness=True).functions
    finally:
        ctypes.CDLL, engine.LIB_PATH, engine.HARNESS_LIB_PATH = saved[:3]
        engine._libs.clear()
        engine._libs.update(saved[3])
    assert set(declared) == set(engine.EXPORTED_SYMBOLS) | set(engine.HARNESS_ONLY_SYMBOLS)
    return {
        "prototypes": {n: _proto(f.restype, f.argtypes) for n, f in sorted(declared.items()) if n in engine.EXPORTED_SYMBOLS},
        "harness_prototypes": {n: _proto(f.restype, f.argtypes) for n, f in sorted(declared.items())
                               if n in engine.HARNESS_ONLY_SYMBOLS},
        "exported_symbols": sorted(engine.EXPORTED_SYMBOLS),
        "harness_only_symbols": sorted(engine.HARNESS_ONLY_SYMBOLS),
        "constants": {"ABI_VERSION": config.ABI_VERSION, "PREC_BF16": config.PREC_BF16, "PREC_F32": config.PREC_F32,
                      "PREC_F16": config.PREC_F16, "DT_F32": config.DT_F32, "DT_F16": config.DT_F16, "DT_BF16": config.DT_BF16,
                      "WEIGHT_OPERANDS": config.WEIGHT_OPERANDS, "HIDDEN_ACTS": config.HIDDEN_ACTS,
                      "SCORE_KINDS": config.SCORE_KINDS, "KERNEL_CLASSES": engine.KERNEL_CLASSES, "TOPK_MAX": engine.TOPK_MAX,
                      "NEG_MAX_GROUPS": detection.NEG_MAX_GROUPS},
        "structs": {s.__name__: {"fields": [[n, type_name(t)] for n, t in s._fields_], "sizeof": ctypes.sizeof(s)}
                    for s in (config.CConfig, config.JpegImage)},
    }


@pytest.fixture(scope="module")
def frozen():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_package_binds_what_it_bound_by_hand(frozen):
    assert bound() == frozen


def test_the_header_gives_the_frozen_table(frozen):
    from mcm_amd import abi

    got = {n: _proto(*p) for n, p in abi.PROTOTYPES.items()}
    got_h = {n: _proto(*p) for n, p in abi.HARNESS_PROTOTYPES.items()}
    assert got == frozen["prototypes"] and got_h == frozen["harness_prototypes"]
    assert len(got) == 58 + 1 and "mcm_abi_version" in got and len(got_h) == 28   # 86 prototypes and mcm_abi_version
    for name, (restype, _a) in {**abi.PROTOTYPES, **abi.HARNESS_PROTOTYPES}.items():
        assert type_name(restype) == NOT_INT.get(name, "c_int32") and (name in NOT_INT or restype is ctypes.c_int), name
    for py, c in (("CConfig", "mcm_config"), ("JpegImage", "mcm_jpeg_image")):
        fields = abi.struct_fields(c)
        assert [[n, type_name(t)] for n, t in fields] == frozen["structs"][py]["fields"]
        assert ctypes.sizeof(type(py, (ctypes.Structure,), {"_fields_": fields})) == frozen["structs"][py]["sizeof"]
    c, d = frozen["constants"], abi.DEFINES
    assert all(type(v) is int for v in d.values())
    assert d["MCM_ABI_VERSION"] == c["ABI_VERSION"] and d["MCM_TOPK_MAX"] == c["TOPK_MAX"]
    assert d["MCM_NEG_MAX_GROUPS"] == c["NEG_MAX_GROUPS"] and d["MCM_KC_COUNT"] == len(c["KERNEL_CLASSES"])
    assert [d["MCM_KC_" + k.upper()] for k in c["KERNEL_CLASSES"]] == list(range(len(c["KERNEL_CLASSES"])))
    assert d["MCM_EINVAL"] == -1 and d["MCM_ERANGE"] == -7   # a parenthesised negative value


HEADER = """/* a header as mcm.h is written */
#define MCM_ONE 1 /* one */
#define MCM_MINUS (-2)
typedef struct mcm_handle mcm_handle;
typedef struct mcm_pair { int32_t a, b[2]; /* two */ %s } mcm_pair;
int mcm_first(const mcm_pair* p, const char* name, const char* const* names, int64_t n, %s);
const char* mcm_text(void);
#ifdef MCM_HARNESS
void mcm_debug_second(mcm_handle** out, double x);
#endif
"""


def test_a_header_text_is_read_as_written():
    from mcm_amd import abi

    c = ctypes
    h = abi.parse(HEADER % ("float c;", "float* y"))
    assert h.prototypes == {"mcm_first": (c.c_int, [c.c_void_p, c.c_char_p, c.c_void_p, c.c_int64, c.c_void_p]),
                            "mcm_text": (c.c_char_p, [])}
    assert h.harness_prototypes == {"mcm_debug_second": (None, [c.c_void_p, c.c_double])}
    assert h.defines == {"MCM_ONE": 1, "MCM_MINUS": -2}
    assert h.structs == {"mcm_pair": [("a", c.c_int32), ("b", c.c_int32 * 2), ("c", c.c_float)]}


def test_an_unknown_type_is_refused_and_named():
    from mcm_amd import abi

    with pytest.raises(ValueError, match=r"mcm_first.*'size_t'"):
        abi.parse(HEADER % ("", "size_t y"))
    with pytest.raises(ValueError, match=r"mcm_first"):   # void is a return type only
        abi.parse(HEADER % ("", "void y"))
    with pytest.raises(ValueError, match=r"mcm_pair.*'long'"):
        abi.parse(HEADER % ("long c;", "float y"))
    with pytest.raises(ValueError, match=r"mcm_pair"):   # a struct holds scalars and arrays of them
        abi.parse(HEADER % ("float* c;", "float y"))
    with pytest.raises(ValueError, match=r"int \(\*mcm_callback\)"):   # not a declaration as mcm.h writes them
        abi.parse(HEADER % ("", "float y") + "typedef int (*mcm_callback)(int32_t x);\n")


def test_a_library_without_a_declared_symbol_is_refused_and_named():
    from mcm_amd import abi

    with pytest.raises(AttributeError, match="mcm_abi_version"):
        abi.declare(ctypes.CDLL(None))
    with pytest.raises(KeyError, match="mcm_nothing"):   # and a name the header does not declare
        abi.declare(ctypes.CDLL(None), names=["mcm_nothing"])


def test_every_symbol_of_the_built_libraries_is_declared():
    from mcm_amd import abi
    from mcm_amd.engine import HARNESS_LIB_PATH, LIB_PATH

    if not os.path.exists(LIB_PATH) or not os.path.exists(HARNESS_LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib, hlib = abi.declare(ctypes.CDLL(LIB_PATH)), abi.declare(ctypes.CDLL(HARNESS_LIB_PATH), harness=True)
    for L, table in ((lib, abi.PROTOTYPES), (hlib, {**abi.PROTOTYPES, **abi.HARNESS_PROTOTYPES})):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.mcm_abi_version() == abi.DEFINES["MCM_ABI_VERSION"] == hlib.mcm_abi_version()
