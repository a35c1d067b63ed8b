"""The Python binding of the C ABI, read from include/mcm.h: the header is the only declaration of an entry's arguments, a
struct's fields and a constant's value.  Standard library only.

    PROTOTYPES / HARNESS_PROTOTYPES   name -> (restype, argtypes): the product entries / those under #ifdef MCM_HARNESS
    EXTENSION_PROTOTYPES              the same for the product entries that the extension headers next to mcm.h declare
                                      (include/mcm_score_stream.h); declare() binds them where they are named
    EXTENSION_HARNESS_PROTOTYPES      ... and for the harness entries they declare under #ifdef MCM_HARNESS
                                      (include/mcm_debug_workspace.h)
    DEFINES                           every integer `#define MCM_*` -> int
    struct_fields(name)               the ctypes `_fields_` of a struct of the header, array members included
    declare(lib, names, harness)      sets restype and argtypes on a ctypes.CDLL

The type rule: a scalar (int, int32_t, int64_t, uint64_t, float, double, ...) is the ctypes type of the same name; `const char*` is
c_char_p, as an argument and as a return type; every other pointer — handle, struct, scalar, pointer to pointer — is c_void_p;
a `void` return is None.  Anything else raises when this module is imported and names the declaration: nothing is guessed.

This is no C parser.  It reads the header as it is written: one declaration per `;`, no function pointers, structs of scalars
and arrays of scalars.  A declaration outside that is refused: write it plainly."""
import collections
import ctypes
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcm.h")
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            **{f"{u}int{n}_t": getattr(ctypes, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}
# read by the rules of mcm.h; each includes it and adds entries, nothing else (under #ifdef MCM_HARNESS: harness entries)
EXTENSION_HEADERS = ("mcm_score_stream.h", "mcm_debug_workspace.h")
Header = collections.namedtuple("Header", "prototypes harness_prototypes defines structs")


def _ctype(ctype: str, where: str, restype: bool = False):
    words = [w for w in ctype.replace("*", " * ").split() if w != "const"]
    if words == ["char", "*"]:
        return ctypes.c_char_p
    if "*" in words:
        return ctypes.c_void_p
    if restype and words == ["void"]:
        return None
    if len(words) != 1 or words[0] not in _SCALARS:
        raise ValueError(f"include/mcm.h: {where}: no ctypes type is known for {ctype.strip()!r}")
    return _SCALARS[words[0]]


def _prototypes(text: str) -> dict:
    out = {}
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)   # the include guard, #include and the #defines
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(mcm_\w+) ?\((.*)\)", decl)
        if not m:
            raise ValueError(f"include/mcm.h: {decl!r} is not a function declaration as this module reads them")
        params = [] if m[3].strip() == "void" else [re.fullmatch(r"(.*?)(\w+)", p.strip()) for p in m[3].split(",")]
        if None in params:
            raise ValueError(f"include/mcm.h: {decl!r}: every parameter is a type and a name")
        out[m[2]] = (_ctype(m[1], decl, restype=True), [_ctype(p[1], decl) for p in params])
    return out


def parse(text: str) -> Header:
    """The declarations of a header written as include/mcm.h is."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^#define\s+(MCM_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    harness = re.search(r"#ifdef MCM_HARNESS\b(.*?)#endif", text, flags=re.S)
    if harness:
        text = text.replace(harness[0], "")
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)   # extern "C" { and its }
    structs = {}
    for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} \1;", text, flags=re.S):
        fields = structs[m[1]] = []
        for member in filter(None, (" ".join(s.split()) for s in m[2].split(";"))):
            base, _, names = member.partition(" ")
            for d in names.split(","):
                name = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", d.strip())
                if not name or base not in _SCALARS:
                    raise ValueError(f"include/mcm.h: struct {m[1]}: {member!r}: no ctypes type is known for {base!r}; "
                                     "a struct holds scalars and arrays of scalars")
                fields.append((name[1], _SCALARS[base] * int(name[2]) if name[2] else _SCALARS[base]))
        text = text.replace(m[0], "")
    text = re.sub(r"typedef struct (\w+) \1;", "", text)   # the opaque handles
    return Header(_prototypes(text), _prototypes(harness[1]) if harness else {}, defines, structs)


def _read_header(path: str = HEADER_PATH) -> Header:
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the Python binding of libmcm_hip.so is read from it "
                           "(mcm_amd runs from its source tree, next to include/)")
    with open(path) as f:
        return parse(f.read())


def read_extension(path: str, taken=()) -> Header:
    """An extension header: new entries and nothing else — product entries, and harness entries in an #ifdef MCM_HARNESS block
    of its own.  A #define, a struct or a name in `taken` (what mcm.h and the extensions before it declare) is refused."""
    ext = _read_header(path)
    again = (set(ext.prototypes) | set(ext.harness_prototypes)) & set(taken) | set(ext.prototypes) & set(ext.harness_prototypes)
    if ext.defines or ext.structs or again:
        raise ValueError(f"include/{os.path.basename(path)}: an extension header declares new entries and nothing else"
                         + (f" (declared before: {sorted(again)})" if again else ""))
    return ext


PROTOTYPES, HARNESS_PROTOTYPES, DEFINES, _STRUCTS = _read_header()
EXTENSION_PROTOTYPES, EXTENSION_HARNESS_PROTOTYPES = {}, {}
for _name in EXTENSION_HEADERS:
    _ext = read_extension(os.path.join(os.path.dirname(HEADER_PATH), _name),
                          {**PROTOTYPES, **HARNESS_PROTOTYPES, **EXTENSION_PROTOTYPES, **EXTENSION_HARNESS_PROTOTYPES})
    EXTENSION_PROTOTYPES.update(_ext.prototypes)
    EXTENSION_HARNESS_PROTOTYPES.update(_ext.harness_prototypes)


def struct_fields(name: str) -> list:
    return list(_STRUCTS[name])


def declare(lib, names=None, harness: bool = False):
    """Set restype and argtypes of `names` on `lib` (default: every product entry, and every harness entry with `harness`) and
    return it.  A symbol the library lacks is an error that names it; so is a name the header does not declare."""
    table = {**PROTOTYPES, **HARNESS_PROTOTYPES, **EXTENSION_PROTOTYPES, **EXTENSION_HARNESS_PROTOTYPES}
    if names is None:
        names = list(PROTOTYPES) + (list(HARNESS_PROTOTYPES) if harness else [])
    for name in names:
        restype, argtypes = table[name]
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AttributeError(f"{getattr(lib, '_name', lib)} does not export {name}, which include/mcm.h declares") from None
        fn.restype, fn.argtypes = restype, argtypes
    return lib
