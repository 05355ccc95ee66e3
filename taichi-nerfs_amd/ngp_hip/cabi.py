"""Reads a C ABI out of header text: the `#define`d integers, the `typedef struct` layouts and the prototypes, as ctypes.

ngp_hip/lib.py binds libngp_hip.so from what this finds in include/ngp_hip.h and include/ngp_hip_experimental.h, so the headers are the
only place where an entry point's arguments are written down.  Regular expressions over comment-free text, not a C grammar: what the
headers use is understood, and anything else raises HeaderError with the entry point's (or struct's) name and the offending text --
nothing is ever typed by default.  A header line that does not parse is to be written more plainly; this file is not to grow for it.
"""
import ctypes
import re
from collections import namedtuple

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "unsigned int": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
           "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double}
# what a pointer may point to (besides the structs): every pointer is handed over as an address, but only one whose target is understood
POINTEES = set(SCALARS) | {"void", "uint8_t", "uint16_t", "int64_t"}

Header = namedtuple("Header", "defines structs functions")
# defines: name -> int;  structs: name -> _fields_;  functions: name -> (result, [argument, ...]), each a (base type, stars, text)

_DECL = re.compile(r"([\w\s]+?)\s*((?:\*\s*(?:const\s*)?)*)\b(\w+)\s*(?:\[\s*(\w+)\s*\])?")


class HeaderError(RuntimeError):
    pass


def _declarator(text, where):
    """`const float* const* p[5]` -> ("float", 2, "p", "5")"""
    m = _DECL.fullmatch(text.strip())
    if not m:
        raise HeaderError("%s: cannot parse %r" % (where, " ".join(text.split())))
    return " ".join(w for w in m.group(1).split() if w != "const"), m.group(2).count("*"), m.group(3), m.group(4)


def ctype(base, stars, text, where, pointers):
    """The ctypes type of `stars` pointers to `base`.  pointers: struct name -> the type of a pointer to that struct."""
    if stars == 1 and base in pointers:
        return pointers[base]
    if stars and (base in POINTEES or base in pointers):
        return ctypes.c_void_p
    if not stars and base in SCALARS:
        return SCALARS[base]
    raise HeaderError("%s: no ctypes type for %r" % (where, " ".join(text.split())))


def parse(text, defines=None):
    """One header's text -> Header.  `defines` are names known from elsewhere (array lengths)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)              # first: the comments hold prototype-like text
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", " ", text, flags=re.S)        # extern "C" { and its }
    defines = dict(defines or {})
    defines.update((k, int(v)) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\d+)[uU]?[ \t]*$", text, re.M))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs = {}

    def struct(m):
        name, fields = m.group(2), []
        where = "struct " + name
        opaque = dict.fromkeys(list(structs) + [name], ctypes.c_void_p)     # a field that points to a struct is an address
        for stmt in filter(str.strip, m.group(1).split(";")):
            first, *more = stmt.split(",")
            base = _declarator(first, where)[0]
            for decl in [first] + [base + " " + d for d in more]:           # `int32_t a, b;`: the stars belong to the declarator
                _, stars, field, length = _declarator(decl, where)
                t = ctype(base, stars, decl, where, opaque)
                if length is not None:
                    if not length.isdigit() and length not in defines:
                        raise HeaderError("%s: unknown array length in %r" % (where, " ".join(decl.split())))
                    t = t * (int(length) if length.isdigit() else defines[length])
                fields.append((field, t))
        structs[name] = fields
        return " "

    text = re.sub(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    functions = {}
    for stmt in filter(str.strip, text.split(";")):                         # all that is left are prototypes
        m = re.fullmatch(r"([^()]+)\(([^()]*)\)", stmt.strip())
        if not m:
            raise HeaderError("cannot parse %r" % " ".join(stmt.split()))
        base, stars, name, length = _declarator(m.group(1), "prototype")
        args = [] if m.group(2).strip() in ("", "void") else m.group(2).split(",")
        decls = [_declarator(a, name) for a in args]
        if length is not None or any(d[3] is not None for d in decls):
            raise HeaderError("%s: array declarator in %r" % (name, " ".join(stmt.split())))
        functions[name] = ((base, stars, m.group(1)), [(d[0], d[1], a) for d, a in zip(decls, args)])
    return Header(defines, structs, functions)


def bind(functions, pointers):
    """Header.functions -> name -> (restype, argtypes)."""
    return {name: (ctype(*res, name, pointers), [ctype(*a, name, pointers) for a in args]) for name, (res, args) in functions.items()}
