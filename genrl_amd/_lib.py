"""ctypes binding of libgenrl_hip.so — the C-ABI declared in include/genrl_hip.h.

The header is the one definition of the boundary: function argtypes AND the argument structs the launch loops take by pointer
(`struct(name)`) are derived from its text, so the binding cannot drift from it.  The grammar the structs may use is stated in the
header next to the first of them; a declaration outside it raises here, it is never skipped.  The product path has no CPU
fallback: importing ops without the built library raises."""
import ctypes, functools, os, re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'genrl_hip.h')
SO = os.environ.get('GENRL_HIP_SO', os.path.join(HERE, 'libgenrl_hip.so'))   # override: kernel experiments

_CT = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float, 'unsigned': ctypes.c_uint, 'uint16_t': ctypes.c_uint16}
_NAME = r'\w+(?:\s*\[\d+\])?'
_DECL = re.compile(r'(?:const\s+)?(\w+)\s*(\*?)\s*(%s(?:\s*,\s*%s)*)' % (_NAME, _NAME))


def _parse_structs(src):
    """-> {name: ctypes.Structure subclass} for every `typedef struct { ... } genrl_NAME;`, in header order.  Every pointer field is a
    c_void_p (filled from tensor addresses); a genrl_* struct by value is the class built before it."""
    out = {}
    blocks = list(re.finditer(r'\btypedef\s+struct\s*\{([^{}]*)\}\s*(genrl_\w+)\s*;', src))
    if len(blocks) != len(re.findall(r'\b(?:struct|union)\b', src)):
        raise ValueError('a struct / union outside `typedef struct { ... } genrl_NAME;` (tagged, nested or anonymous)')
    for blk in blocks:
        fields = []
        for decl in [d.strip() for d in blk.group(1).split(';') if d.strip()]:
            m = _DECL.fullmatch(decl)
            if not m:
                raise ValueError(f'{blk.group(2)}: declaration outside the binding grammar: {decl!r}')
            base, star, names = m.group(1), m.group(2), [n.strip() for n in m.group(3).split(',')]
            if star:
                if len(names) > 1 or not (base == 'void' or base in _CT or base in out):
                    raise ValueError(f'{blk.group(2)}: pointer declaration outside the binding grammar: {decl!r}')
                ct = ctypes.c_void_p
            elif base in _CT or base in out:
                ct = _CT.get(base) or out[base]
            else:
                raise ValueError(f'{blk.group(2)}: unknown type {base!r} in {decl!r}')
            for n in names:
                n, _, dim = n.partition('[')
                fields.append((n.strip(), ct * int(dim.rstrip(' ]')) if dim else ct))
        # (no instance __dict__: assigning a name that is not a field raises instead of setting nothing)
        out[blk.group(2)] = type(blk.group(2), (ctypes.Structure,), {'_fields_': fields, '__slots__': ()})
    return out


@functools.lru_cache(None)             # (once per header: the struct classes are the identity the argtypes check against)
def _parse(path):
    src = open(path).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    structs = _parse_structs(src)
    out = {}
    for m in re.finditer(r'\b(int|long)\s+(genrl_\w+)\s*\(([^)]*)\)\s*;', src):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        al = []
        for a in [x.strip() for x in args.split(',') if x.strip() and x.strip() != 'void']:
            if '*' in a:
                base = a.split('*')[0].replace('const', '').strip()
                al.append((ctypes.POINTER(structs[base]) if base in structs else ctypes.c_void_p, a.split('*')[-1].strip()))
            else:
                t, n = a.rsplit(' ', 1)
                al.append((_CT[t.replace('const', '').strip()], n))
        out[name] = (_CT[ret], al)
    return structs, out


def parse_header(path=HEADER):
    """-> {name: (restype, [(ctype, argname), ...])}; a `genrl_NAME*` parameter is POINTER(struct('genrl_NAME')): ctypes takes the
    struct, an array of it, byref() of it or None there, and refuses every other struct, c_void_p and plain integers"""
    return _parse(path)[1]


def structs(path=HEADER):
    """-> {name: ctypes.Structure subclass} of the header's argument structs"""
    return _parse(path)[0]


def struct(name):
    return structs()[name]


class GenrlHipError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise GenrlHipError(f'{SO} is missing: build it with `python -m genrl_amd.build` '
                                '(there is no CPU fallback for the hot path)')
        # torch bundles its own libamdhip64; it must be resident BEFORE this library is dlopen'ed so
        # that both share ONE HIP runtime (two runtimes in a process -> "no ROCm-capable device").
        import torch  # noqa: F401
        L = ctypes.CDLL(SO)
        for name, (ret, args) in parse_header().items():
            fn = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = ret
            fn.argtypes = [t for t, _ in args]
        _lib = L
    return _lib


def check(code, what):
    if code != 0:
        detail = ''
        if code == 2:
            try:
                fn = _lib.genrl_last_error
                fn.restype = ctypes.c_char_p
                detail = ': ' + fn().decode()
            except Exception:
                pass
        raise GenrlHipError(f'{what} failed with status {code}{detail}')
