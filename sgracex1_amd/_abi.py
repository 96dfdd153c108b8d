"""Reads include/sgx.h into ctypes declarations, so that the header is the only statement of the C ABI.

The header is regular C99 and the reader knows exactly what it uses: `#define NAME <integer>`, `typedef enum`, `typedef
struct` (complete or opaque) and function prototypes, over the closed set of types below.  Anything else -- an unknown
type, a function pointer, a bit-field, an expression as an array extent -- raises HeaderError with the header line;
nothing is guessed.  tests/test_abi.py compares every struct and constant read here with the C compiler's.

ctypes mapping (what the call sites in ops.py rely on):
  struct field   pointer to a scalar, to void or to an opaque struct -> c_void_p (assigned from tensor.data_ptr());
                 pointer to a complete sgx struct -> POINTER(Struct); T x[n] -> T * n; a nested struct by value
  parameter      pointer to a complete sgx struct -> POINTER(Struct); T ** -> POINTER(c_void_p); any other pointer ->
                 c_void_p, which takes None, an int, a ctypes array or byref(...)
  return         a scalar, void -> None, const char * -> c_char_p
"""
import collections
import ctypes
import re

SCALARS = {
    "int": ctypes.c_int, "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "int32_t": ctypes.c_int32,
    "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
    "float": ctypes.c_float, "double": ctypes.c_double,
}
# the host arrays of sgx_node_batch: ops.py assigns ctypes arrays to them, which a c_void_p field does not take, so
# these three keep the pointee type
HOST_ARRAYS = {("sgx_node_batch", "fanouts"), ("sgx_node_batch", "hop_nodes"), ("sgx_node_batch", "hop_edges")}

# constants: {name: int} of every #define and enumerator; structs: {C name: ctypes.Structure class}, in header order;
# opaque: the names only declared; functions: {name: (restype, argtypes)}, in header order
Abi = collections.namedtuple("Abi", "constants structs opaque functions")

_TOKEN = re.compile(r"\s+|([A-Za-z_]\w*|-?\d+(?!\w)|[{}()\[\];,*=])|(.)")
_DEFINE = re.compile(r"#\s*define\s+(\w+)(?:\s+(-?\d+))?\s*")


class HeaderError(ValueError):
    pass


def class_name(c_name):
    """sgx_layer_desc -> LayerDesc: the name a struct has in _lib."""
    return "".join(part.capitalize() for part in c_name.split("_")[1:])


class _Reader:
    def __init__(self, text, name):
        self.name = name
        # comments go, their line breaks stay: every token keeps the line it has in the file
        self.lines = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S).split("\n")
        self.abi = Abi({}, {}, set(), {})
        self.tokens, self.pos = [], 0
        self._preprocess()
        while self.pos < len(self.tokens):
            self._statement()

    def fail(self, what, line):
        raise HeaderError(f"{self.name}:{line}: {what}: {self.lines[line - 1].strip()}")

    def _preprocess(self):
        """Takes the # lines (include guard, #include, the extern "C" block, #define NAME integer) and tokenises the rest."""
        guard, in_cplusplus = None, False
        for no, line in enumerate(self.lines, 1):
            s = line.strip()
            if in_cplusplus:
                in_cplusplus = s != "#endif"
            elif s == "#ifdef __cplusplus":
                in_cplusplus = True
            elif s.startswith("#"):
                define = _DEFINE.fullmatch(s)
                if define and define.group(2) is not None:
                    self._constant(define.group(1), define.group(2), no)
                elif define and define.group(1) == guard:
                    pass
                elif re.fullmatch(r"#\s*ifndef\s+\w+", s) and guard is None:
                    guard = s.split()[-1]
                elif not (s == "#endif" or re.fullmatch(r"#\s*include\s*<\w+\.h>", s)):
                    self.fail("unknown preprocessor line", no)
            else:
                for m in _TOKEN.finditer(line):
                    if m.group(2):
                        self.fail(f"unexpected character {m.group(2)!r}", no)
                    if m.group(1):
                        self.tokens.append((m.group(1), no))

    def _constant(self, name, value, line):
        if name in self.abi.constants:
            self.fail(f"{name} defined twice", line)
        if not re.fullmatch(r"-?\d+", value):
            self.fail(f"the value of {name} is not an integer literal", line)
        self.abi.constants[name] = int(value)

    # ---- tokens
    def next(self):
        if self.pos == len(self.tokens):
            self.fail("the header ends inside a declaration", len(self.lines))
        self.pos += 1
        self.line = self.tokens[self.pos - 1][1]
        return self.tokens[self.pos - 1][0]

    def peek(self, ahead=0):
        return self.tokens[self.pos + ahead][0] if self.pos + ahead < len(self.tokens) else None

    def expect(self, *wanted):
        tok = self.next()
        if tok not in wanted:
            self.fail(f"expected {' or '.join(map(repr, wanted))}, found {tok!r}", self.line)
        return tok

    def identifier(self):
        tok = self.next()
        if not re.fullmatch(r"[A-Za-z_]\w*", tok) or tok in SCALARS or tok in ("const", "void", "char", "struct", "enum"):
            self.fail(f"expected a name, found {tok!r}", self.line)
        return tok

    # ---- types
    def _base(self):
        tok = self.next()
        if tok == "const":
            tok = self.next()
        a = self.abi
        if not (tok in SCALARS or tok in ("void", "char") or tok in a.structs or tok in a.opaque):
            self.fail(f"unknown type {tok!r}", self.line)
        return tok

    def _stars(self):
        depth = 0
        while self.peek() == "*":
            self.next()
            depth += 1
        return depth

    def _ctype(self, base, depth, where, host_array=False):
        struct = self.abi.structs.get(base)
        plain = base in SCALARS or base == "void" or base in self.abi.opaque        # what a c_void_p may point to
        if depth == 0:
            if base in SCALARS:
                return SCALARS[base]
            if struct and where == "field":
                return struct
            if base == "void" and where == "return":
                return None
        elif where == "return":
            if (base, depth) == ("char", 1):
                return ctypes.c_char_p
        elif depth == 1 and struct:
            return ctypes.POINTER(struct)
        elif depth == 1 and plain:
            return ctypes.POINTER(SCALARS[base]) if host_array else ctypes.c_void_p
        elif depth == 2 and where == "param" and plain and base not in SCALARS:
            return ctypes.POINTER(ctypes.c_void_p)
        self.fail(f"no binding for {base} {'*' * depth} as a {where}", self.line)

    # ---- declarations
    def _statement(self):
        if self.peek() != "typedef":
            return self._prototype()
        self.next()
        kind, name = self.expect("enum", "struct"), self.identifier()
        if kind == "struct" and self.peek() != "{":
            self.abi.opaque.add(name)
        else:
            self.expect("{")
            if kind == "enum":
                self._enumerators()
            else:
                fields = self._fields(name)
                self.abi.structs[name] = type(class_name(name), (ctypes.Structure,), {
                    "_fields_": fields, "__doc__": f"struct {name} of include/sgx.h"})
        if self.identifier() != name:
            self.fail(f"the typedef of {kind} {name} has another name", self.line)
        self.expect(";")

    def _enumerators(self):
        while True:
            name = self.identifier()
            self.expect("=")
            self._constant(name, self.next(), self.line)
            if self.expect(",", "}") == "}":
                return

    def _fields(self, struct):
        fields = []
        while self.peek() != "}":
            base = self._base()
            while True:                                      # the declarators of one declaration: *a, *b  |  x[2], y[2]
                depth, name = self._stars(), self.identifier()
                ctype = self._ctype(base, depth, "field", (struct, name) in HOST_ARRAYS)
                if self.peek() == "[":
                    self.next()
                    extent = self.next()
                    if not re.fullmatch(r"\d+", extent) and extent not in self.abi.constants:
                        self.fail(f"array extent {extent!r} is neither a literal nor a #define seen above", self.line)
                    ctype = ctype * int(self.abi.constants.get(extent, extent))
                    self.expect("]")
                fields.append((name, ctype))
                if self.expect(",", ";") == ";":
                    break
        self.next()
        return fields

    def _prototype(self):
        base = self._base()
        restype = self._ctype(base, self._stars(), "return")
        name = self.identifier()
        self.expect("(")
        argtypes = []
        if (self.peek(), self.peek(1)) == ("void", ")"):
            self.next()
        else:
            while True:
                base = self._base()
                argtypes.append(self._ctype(base, self._stars(), "param"))
                self.identifier()
                if self.peek() == ",":
                    self.next()
                else:
                    break
        self.expect(")")
        self.expect(";")
        self.abi.functions[name] = (restype, argtypes)


def read_header(text, name="sgx.h"):
    """The Abi of a header given as text; `name` is what error messages call it."""
    return _Reader(text, name).abi


def bind(lib, abi):
    """Sets argtypes / restype of every declared function on a ctypes library (a missing symbol raises AttributeError)."""
    for name, (restype, argtypes) in abi.functions.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
