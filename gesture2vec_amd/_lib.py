"""ctypes binding of libg2v_hip.so (include/g2v.h).  No torch types cross the boundary: only raw
device pointers, sizes and a hipStream_t.  Loading FAILS LOUDLY when the library is missing; there is
no CPU or PyTorch fallback anywhere in the product path."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import re
import string

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libg2v_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "g2v.h")


class G2VLibraryError(RuntimeError):
    pass


# include/g2v.h is the ONLY description of the C ABI: the signatures, the struct classes and the constants below are read from it
# at import.  The header keeps to a small subset of C (block comments, #define NAME <integer>, typedef struct { ... } g2v_x;,
# typedef void* handles, opaque structs, prototypes); a declaration outside that subset raises here, it is never skipped.
_SCALAR = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_NAME_CHARS = string.ascii_letters + string.digits + "_"
_DECL = re.compile(r"\s*(?:typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;|([^;{}]+);)", re.S)


def parse_header(text: str):
    """-> (signatures {function: (restype, argtypes)}, structs {C name: Structure class}, constants {G2V_X: int})"""
    sigs, structs, consts, handles, opaque = {}, {}, {}, set(), set()

    def fail(decl, why):
        raise G2VLibraryError(f"include/g2v.h: cannot bind `{' '.join(decl.split())}`: {why}")

    @functools.lru_cache(None)
    def lookup(spec):
        """Device pointers, handles and pointers to pointers travel as void*; G2V_HOST marks a host array, which keeps its type
        (so that ctypes takes the array and holds it); a struct is passed by typed pointer."""
        words = spec.replace("*", " * ").split()
        host, stars = "G2V_HOST" in words, words.count("*")
        base = [w for w in words if w not in ("const", "*", "G2V_HOST")]
        base = base[0] if len(base) == 1 else None
        if host:
            if stars == 1 and base in _SCALAR:
                return C.POINTER(_SCALAR[base])
        elif stars == 0:
            if base in _SCALAR or base in handles:
                return _SCALAR.get(base, C.c_void_p)
        elif stars == 1 and base in structs:
            return C.POINTER(structs[base])
        elif base == "void" or base in _SCALAR or base in structs or base in opaque or base in handles:
            return C.c_void_p

    def ctype(spec, decl):
        return lookup(spec.strip()) or fail(decl, f"unknown type `{spec.strip()}`")

    def struct(body, cname):
        fields = []
        for stmt in filter(str.strip, body.split(";")):
            decl = f"{stmt}; (in {cname})"
            first, *more = stmt.split(",")
            m = re.fullmatch(r"\s*(.*?)(\w+\s*(?:\[.*\])?)\s*", first, re.S)
            if not m or (more and "*" in m[1]):
                fail(decl, "not a field declaration")
            ct = ctype(m[1], decl)
            for d in [m[2]] + more:
                dm = re.fullmatch(r"\s*(\w+)\s*(?:\[(.*)\])?\s*", d)
                if not dm or not (dm[2] is None or dm[2].strip().isdigit()):
                    fail(decl, "an array bound must be an integer literal")
                fields.append((dm[1], ct * int(dm[2]) if dm[2] else ct))
        name = "".join(w.capitalize() for w in cname[len("g2v_"):].split("_"))        # g2v_dec_weights -> DecWeights
        structs[cname] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": cname})

    def prototype(m, decl):
        ret, name, args = m[1].replace("*", " * ").split(), m[2], m[3]
        if name in sigs:
            fail(decl, "declared twice")
        res = None if ret == ["void"] else C.c_char_p if ret == ["const", "char", "*"] else ctype(m[1], decl)
        args = [] if args.strip() == "void" else args.split(",")
        sigs[name] = (res, [ctype(a.rstrip().rstrip(_NAME_CHARS), decl) for a in args])          # (the type is what precedes the name)

    text = re.sub(r"/\*.*?\*/|#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    for line in re.findall(r"^[ \t]*#.*$", text, re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)\s*(?:\(?\s*(-?\d+)\s*\)?)?\s*", line)
        if m and m[2]:
            consts[m[1]] = int(m[2])
        elif not m and not re.match(r"\s*#\s*(ifndef|include|endif)\b", line):      # (#define NAME alone: a guard or a marker)
            fail(line, "not a #define of an integer")
    body, pos = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M), 0
    while body[pos:].strip():
        m = _DECL.match(body, pos)
        if not m:
            fail(body[pos:].strip()[:120], "not a declaration")
        pos, decl = m.end(), m[0]
        if m[2]:
            struct(m[1], m[2])
        elif t := re.fullmatch(r"\s*typedef\s+void\s*\*\s*(\w+)\s*;", decl):
            handles.add(t[1])
        elif t := re.fullmatch(r"\s*typedef\s+struct\s+(\w+)\s+\1\s*;", decl):
            opaque.add(t[1])
        elif t := re.fullmatch(r"\s*(.*?)\b(g2v_\w+)\s*\((.*)\)\s*;", decl, re.S):
            prototype(t, decl)
        else:
            fail(decl, "neither a typedef nor a prototype")
    return sigs, structs, consts


try:
    with open(HEADER_PATH) as _f:
        _SIGS, STRUCTS, CONSTANTS = parse_header(_f.read())
except OSError as e:
    raise G2VLibraryError(f"{HEADER_PATH} cannot be read ({e}): the binding is derived from it") from None
globals().update({cls.__name__: cls for cls in STRUCTS.values()})            # DecWeights, GruDir, WgradPending, ...
globals().update({k[len("G2V_"):]: v for k, v in CONSTANTS.items()})        # OPT_PERSISTENT, WGRAD_BF16X3, VQ_BX_EXACT, ...
EXPORTS = tuple(_SIGS)

_lib = None


def load():
    """Load libg2v_hip.so once and attach the signatures.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise G2VLibraryError(
            f"{LIB_PATH} is missing: build it with `make -C gesture2vec_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`).  There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().g2v_last_error().decode()
        raise G2VLibraryError(f"g2v call failed ({rc}) {what}: {msg}")


class Context:
    """The ONE route to the library's implementation switches (include/g2v.h: G2V_OPT_*, g2v_ctx).  A Context() owns a set of
    them; `with ctx:` binds it to the calling thread for the duration of the block (re-entrant: the previous binding comes
    back) and every library call inside reads ITS switches.  An engine owns one, so that two engines in one process do not share
    switches and a residency fault in one does not switch off the fast path of the other.  Context.current() owns nothing: it
    addresses whatever the calling thread has bound at the moment of each call (the process's default context if nothing).
    scoped(name=value, ...) changes options for a block and puts back exactly what was there: no hand-written save / restore."""

    OPTIONS = {k[len("G2V_OPT_"):].lower(): v for k, v in CONSTANTS.items() if k.startswith("G2V_OPT_")}

    def __init__(self):
        self._lib = load()
        self._h = self._lib.g2v_ctx_create()
        if not self._h:
            raise MemoryError("g2v_ctx_create failed")
        self._stack = []

    @classmethod
    def current(cls) -> "Context":
        """a non-owning handle: the calling thread's bound context, else the default one (g2v_ctx_set_option(NULL, ...))"""
        self = object.__new__(cls)
        self._lib, self._h = load(), None
        return self

    def set(self, option: int, value: int) -> int:
        """-> the previous value"""
        prev = int(self._lib.g2v_ctx_set_option(self._h, int(option), int(value)))
        if prev < 0:
            check(prev, f"(g2v_ctx_set_option {option})")
        return prev

    def get(self, option: int) -> int:
        value = int(self._lib.g2v_ctx_get_option(self._h, int(option)))
        if value < 0:
            check(value, f"(g2v_ctx_get_option {option})")
        return value

    @contextlib.contextmanager
    def scoped(self, **options):
        """ctx.scoped(persistent=0, gru_cluster=0): set each option in order; on the way out -- also behind an exception --
        restore, in reverse order, the values the sets returned."""
        unknown = [k for k in options if k not in self.OPTIONS]
        if unknown:
            raise TypeError(f"scoped(): unknown option(s) {unknown}; the header has {sorted(self.OPTIONS)}")
        with contextlib.ExitStack() as undo:
            for name, value in options.items():
                undo.callback(self.set, self.OPTIONS[name], self.set(self.OPTIONS[name], value))
            yield self

    def __enter__(self):
        if self._h is None:
            raise G2VLibraryError("Context.current() is a handle on whatever is bound: it cannot be bound itself")
        self._stack.append(self._lib.g2v_ctx_bind(self._h))
        return self

    def __exit__(self, *exc):
        self._lib.g2v_ctx_bind(self._stack.pop())
        return False

    def __del__(self):
        try:
            if self._h:
                self._lib.g2v_ctx_destroy(self._h)
                self._h = None
        except Exception:
            pass
