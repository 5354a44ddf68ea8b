"""Reader of include/dagr_hip.h: the header is the single source of truth of the C ABI, and the ctypes binding
(``_lib.py``) is derived from it here instead of being written out a second time.

This reads the dialect that header is written in -- ``typedef struct``, ``enum``, function prototypes over the fixed
width scalars -- and nothing more: it is not a C parser.  A declaration it cannot take apart, or a type name it does not
know, raises ``ValueError`` naming the declaration; nothing is guessed and nothing is skipped.  A declaration that is
awkward to read is better re-flowed in the header than taught to the reader.
"""
import ctypes
import re

SCALARS = {"void": None, "char": ctypes.c_char, "int": ctypes.c_int, "int8_t": ctypes.c_int8, "int16_t": ctypes.c_int16,
           "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double}

_BLOCK = re.compile(r"(typedef\s+)?\b(struct|enum)\b\s*(\w*)\s*\{([^{}]*)\}\s*(\w*)\s*;")
_FIELDS = re.compile(r"(?:const\s+)?(\w+)\b\s*(.+)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*((?:\[\s*\d+\s*\]\s*)*)")
_FUNCTION = re.compile(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*\((.*)\)", re.S)
_ARGUMENT = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)?")


class Header:
    """``structs``: C name -> ``ctypes.Structure`` class (named ``dagr_pool_desc`` -> ``PoolDesc``); ``enums``:
    enumerator -> int; ``functions``: name -> ``(restype, [argtypes])`` in declaration order."""

    def __init__(self, text):
        self.structs, self.enums, self.functions = {}, {}, {}
        self._types = dict(SCALARS)
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments sit inside argument lists too
        text = re.sub(r"//[^\n]*", " ", text)
        # ``#define NAME <integer>``: the bounds the header states (DAGR_COCO_MAX_GT, DAGR_TRACK_MAX_TRACKS, ...)
        self.defines = {m.group(1): int(m.group(2), 0)
                        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M)}
        text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)     # include guard, includes, #define, #ifdef __cplusplus
        text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
        for decl in _BLOCK.sub(self._block, text).split(";"):
            if decl.strip():
                self._function(" ".join(decl.split()))

    def _ctype(self, base, pointer, decl):
        if base not in self._types:
            raise ValueError(f"dagr_hip.h reader: unknown type {base!r} in: {decl}")
        t = self._types[base]
        if pointer:
            return ctypes.POINTER(t) if base in self.structs else ctypes.c_void_p
        if t is None:
            raise ValueError(f"dagr_hip.h reader: a value of type void in: {decl}")
        return t

    def _block(self, m):
        typedef, kind, tag, body, name = m.groups()
        decl = " ".join(m.group(0).split())
        if bool(typedef) != bool(name) or (kind == "struct" and not name) or (tag and name and tag != name):
            raise ValueError(f"dagr_hip.h reader: expected `typedef {kind} [name] {{ ... }} name;`"
                             + (" or `enum [name] { ... };`" if kind == "enum" else "") + f", got: {decl}")
        if kind == "enum":
            value = -1
            for item in filter(None, (s.strip() for s in body.split(","))):
                e = re.fullmatch(r"(\w+)(?:\s*=\s*(-?\w+))?", item)
                try:
                    value = value + 1 if e.group(2) is None else int(e.group(2), 0)
                except (AttributeError, ValueError):
                    raise ValueError(f"dagr_hip.h reader: cannot read enumerator {item!r} in: {decl}") from None
                self.enums[e.group(1)] = value
            if name:
                self._types[name] = ctypes.c_int
            return " "
        fields = []
        for line in filter(None, (" ".join(s.split()) for s in body.split(";"))):
            f = _FIELDS.fullmatch(line)
            if not f:
                raise ValueError(f"dagr_hip.h reader: cannot read field declaration {line!r} of {name}")
            for item in f.group(2).split(","):
                d = _DECLARATOR.fullmatch(item.strip())
                if not d:
                    raise ValueError(f"dagr_hip.h reader: cannot read declarator {item.strip()!r} in {line!r} of {name}")
                t = self._ctype(f.group(1), d.group(1), f"{line!r} of {name}")
                for n in reversed(re.findall(r"\d+", d.group(3))):     # row-major: a[3][4] is three arrays of four
                    t = t * int(n)
                fields.append((d.group(2), t))
        cls = type("".join(p.capitalize() for p in name.split("_")[1:]), (ctypes.Structure,),
                   {"_fields_": fields, "__doc__": f"``{name}`` (include/dagr_hip.h)."})
        self.structs[name] = self._types[name] = cls
        return " "

    def _function(self, decl):
        m = _FUNCTION.fullmatch(decl)
        if not m:
            raise ValueError(f"dagr_hip.h reader: cannot read declaration: {decl}")
        const, base, pointer, name, arglist = m.groups()
        if pointer:
            self._ctype(base, pointer, decl)
            restype = ctypes.c_char_p if (const and base == "char") else ctypes.c_void_p
        else:
            restype = None if base == "void" else self._ctype(base, pointer, decl)
        argtypes = []
        if arglist.strip() != "void":
            for arg in arglist.split(","):
                a = _ARGUMENT.fullmatch(arg.strip())
                if not a:
                    raise ValueError(f"dagr_hip.h reader: cannot read argument {arg.strip()!r} of: {decl}")
                argtypes.append(self._ctype(a.group(1), a.group(2), decl))
        if name in self.functions:
            raise ValueError(f"dagr_hip.h reader: {name} is declared twice")
        self.functions[name] = (restype, argtypes)
