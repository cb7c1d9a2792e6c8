"""A regex reading of include/codonlm_hip.h for the binding tests: structs, prototypes, enumerators
and integer defines.  No C parser: the header keeps to `typedef struct { ... } cg_x;`, `enum { ... };`,
`#define CG_X <integer>` and one-statement prototypes, and only /* ... */ comments are taken out."""
import ctypes as C
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "codonlm_hip.h"

# C scalar type -> kind.  ctypes has one class for `int` and `int32_t` (c_int32 is c_int), so both are "int".
SCALARS = {"int": "int", "int32_t": "int", "uint32_t": "uint32", "long long": "long long", "float": "float",
           "double": "double", "size_t": "size_t"}
CTYPES = {C.c_int: "int", C.c_uint32: "uint32", C.c_longlong: "long long", C.c_float: "float",
          C.c_double: "double", C.c_size_t: "size_t", C.c_void_p: "ptr", C.c_char_p: "ptr", None: "void"}


def c_kind(ctype: str):
    """Kind of a C type without its declarator: "ptr", a scalar kind, "void" or a cg_ struct's name."""
    ctype = " ".join(ctype.replace("const", " ").split())
    if "*" in ctype:
        return "ptr"
    return ctype if ctype.startswith("cg_") or ctype == "void" else SCALARS[ctype]


def ctypes_kind(t, structs):
    """The same kinds for a ctypes type; an array is (element kind, length)."""
    if isinstance(t, type) and issubclass(t, C.Array):
        return ctypes_kind(t._type_, structs), t._length_
    if isinstance(t, type) and issubclass(t, C.Structure):
        return {cls: name for name, cls in structs.items()}[t]
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "ptr"
    return CTYPES[t]


def _declarations(body, defines):
    """[(name, kind)] of the `type a, b[N];` declarations of a struct body."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *rest = [p.strip() for p in decl.split(",")]
        m = re.fullmatch(r"(.*?[\s*])(\w+(?:\[\w+\])?)", first, flags=re.S)
        kind = c_kind(m.group(1))
        for d in [m.group(2)] + rest:
            name, _, n = d.rstrip("]").partition("[")
            fields.append((name, (kind, int(defines.get(n, n), 0)) if n else kind))
    return fields


def read_header():
    """dict(structs={name: [(field, kind)]}, protos={name: (return kind, [argument kinds])},
    enums=[{name: value}] one per enum block, defines={name: int})."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    defines = {m.group(1): m.group(2) for m in re.finditer(r"^#define\s+(CG_\w+)\s+(-?\w+?)(?:ll)?\s*$", text, re.M)}
    structs = {}

    def take_struct(m):
        structs[m.group(2)] = _declarations(m.group(1), defines)
        return " "
    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(cg_\w+)\s*;", take_struct, text, flags=re.S)
    enums = []

    def take_enum(m):
        block, nxt = {}, 0
        for item in filter(None, (e.strip() for e in m.group(1).split(","))):
            name, _, val = (s.strip() for s in item.partition("="))
            block[name] = nxt = int(val, 0) if val else nxt
            nxt += 1
        enums.append(block)
        return " "
    text = re.sub(r"enum\s*\{(.*?)\}\s*;", take_enum, text, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"([\w ]+?[\s*]+)(cg_\w+)\s*\(([^)]*)\)\s*;", text):
        kinds = []
        for a in (a.strip() for a in args.split(",")):
            # drop the parameter's name; `void` alone is an empty list
            kinds.append(c_kind(a if a == "void" else re.fullmatch(r"(.*?[\s*])\w+", a, flags=re.S).group(1)))
        protos[name] = (c_kind(ret), [] if kinds == ["void"] else kinds)
    return dict(structs=structs, protos=protos, enums=enums, defines={k: int(v, 0) for k, v in defines.items()})
