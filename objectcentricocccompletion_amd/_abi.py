"""Reader of ``include/ococc_hip.h``: the header is the one place a signature or a descriptor struct is written.

``functions``: name -> (restype, [(ctype, parameter name), ...]) in header order; ``structs``: name -> [(field name,
ctype), ...]; ``types``: name -> the ctypes.Structure built from those fields.  A parameter is one of six shapes: a
fixed-width scalar, an array ``T x[k]`` (host memory, bound as ``T * k``), a device pointer or stream (``c_void_p``: call
sites pass ``tensor.data_ptr()``), a host pointer ``T* host_x`` (``POINTER(T)``), a host table of pointers ``T* const*
host_x`` (``POINTER(c_void_p)``) or a descriptor ``const <struct>* x`` (``POINTER(struct)``).  Anything else raises:
a declaration that is skipped silently is a signature nobody checks.
"""
import ctypes
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ococc_hip.h')

_SCALARS = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
            'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float, 'double': ctypes.c_double}
_POINTEES = set(_SCALARS) | {'void', 'uint8_t', 'uint16_t'}
_RESTYPES = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p}
_DECL = re.compile(r'(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?')
_STRUCT = re.compile(r'typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;')
_PROTO = re.compile(r'(.*?)\b(ococc_\w+)\s*\((.*)\)', re.S)


class AbiError(ValueError):
    pass


def _ctype(decl, where, types, field=False):
    """(ctype, name) of one parameter (or, with ``field``, struct member) declaration"""
    m = _DECL.fullmatch(decl.strip())
    if not m:
        raise AbiError(f'{where}: cannot read the declaration "{decl.strip()}"')
    base, stars, name, count = m.group(1), m.group(2).count('*'), m.group(3), m.group(4)
    if base not in _POINTEES and base not in types and not (base == 'ococc_stream_t' and not stars):
        raise AbiError(f'{where}: unknown type "{base}" of "{name}"')
    if field and stars:                        # pointer members are plain addresses, as call sites fill them
        ct = ctypes.c_void_p
    elif not stars:
        ct = ctypes.c_void_p if base == 'ococc_stream_t' else _SCALARS.get(base)
    elif count:
        ct = None                              # an array of pointers is a struct member's shape only
    elif base in types:
        ct = ctypes.POINTER(types[base]) if stars == 1 and not name.startswith('host_') else None
    elif not name.startswith('host_'):
        ct = ctypes.c_void_p
    elif stars == 1:
        ct = ctypes.POINTER(_SCALARS[base]) if base in _SCALARS else None
    else:
        ct = ctypes.POINTER(ctypes.c_void_p) if stars == 2 else None
    if ct is None:
        raise AbiError(f'{where}: "{decl.strip()}" is none of the parameter shapes of the C ABI')
    return (ct * int(count) if count else ct), name


def parse(text):
    """(functions, structs, types) of a header's text"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    declared = set(re.findall(r'\b(ococc_\w+)\s*\(', text))
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{|typedef\s+void\s*\*\s*ococc_stream_t\s*;', ' ', text, flags=re.M)
    functions, structs, types = {}, {}, {}
    for body, name in _STRUCT.findall(text):
        fields = []
        for line in filter(None, (s.strip() for s in body.split(';'))):
            first, *more = line.split(',')         # "int32_t a, b": the later names repeat the first one's type
            ct, fname = _ctype(first, f'struct {name}', types, field=True)
            if more and not (ct in _SCALARS.values() and all(re.fullmatch(r'\w+', s.strip()) for s in more)):
                raise AbiError(f'struct {name}: cannot read the declaration "{line}"')
            fields += [(fname, ct)] + [(s.strip(), ct) for s in more]
        structs[name] = fields
        types[name] = type(name, (ctypes.Structure,), {'_fields_': fields, '__doc__': f'{name} of include/ococc_hip.h'})
    for stmt in (s.strip() for s in _STRUCT.sub(' ', text).split(';')):
        if stmt in ('', '}'):                      # (the brace that closes extern "C")
            continue
        m = _PROTO.fullmatch(stmt)
        if not m:
            raise AbiError(f'not a prototype of the C ABI: "{" ".join(stmt.split())[:120]}"')
        res, name, params = re.sub(r'\s*\*', '*', ' '.join(m.group(1).split())), m.group(2), m.group(3).strip()
        if res not in _RESTYPES:
            raise AbiError(f'{name}: unknown return type "{res}"')
        functions[name] = (_RESTYPES[res], [] if params == 'void' else [_ctype(p, name, types) for p in params.split(',')])
    if declared - set(functions):
        raise AbiError(f'declared but not read as prototypes: {sorted(declared - set(functions))}')
    return functions, structs, types


if not os.path.exists(HEADER_PATH):
    raise ImportError(f'{HEADER_PATH} is missing: the ctypes signatures of libococc_hip.so are read from the C header, '
                      'which ships next to the package (include/ococc_hip.h).')
with open(HEADER_PATH) as _f:
    functions, structs, types = parse(_f.read())
