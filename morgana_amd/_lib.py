"""ctypes binding of ``libmorgana_hip.so``, derived from ``include/morgana_hip.h`` at import.

This is the stub a maintainer of the reference would add: the reference has no FFI of its own, its
hot path is PyTorch eager.  The header is the single definition of the C ABI: ``parse_header`` turns its text into the
``MG_*`` constants, one ``ctypes.Structure`` per ``typedef struct`` (named as in the header: ``mg_cast_desc``) and the
``SIGNATURES`` table, and this module exposes all three under the header's own names.  Nothing is restated by hand.
There is NO fallback: if the shared library is missing or a call fails, an exception is raised.  Nothing here imports
the oracle.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmorgana_hip.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'morgana_hip.h'))


class MorganaHipError(RuntimeError):
    pass


# The whole type mapping.  Every pointer and every array parameter, whatever it points to, is a c_void_p: call sites pass
# c_void_p, None, integers (tensor.data_ptr()) and cast ctypes arrays.  Anything else in the header is refused, not guessed.
_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float,
            'double': ctypes.c_double, 'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64}
_DIRECTIVE = re.compile(r'#\s*(include\s*<\w+\.h>|ifndef\s+\w+_H|define\s+\w+_H|ifdef\s+__cplusplus|endif)\s*$')
_DEFINE = re.compile(r'#\s*define\s+(MG_\w+)\s+(\(\s*-?\s*\w+\s*\)|-?\s*\w+)\s*$')
_STRUCT = re.compile(r'typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;')
_DECLARATOR = re.compile(r'(.*?[\s*])(\w+)\s*(?:\[\s*(\w+)\s*\])?$', re.S)      # type, name, array length
_PROTOTYPE = re.compile(r'(.*?[\s*])(\w+)\s*\(([^()]*)\)$', re.S)                  # return type, name, parameters


def _refuse(text):
    raise MorganaHipError('morgana_hip.h: no ctypes binding for %r' % ' '.join(text.split()))


def _integer(word, constants, text):
    try:
        return constants[word] if word in constants else int(word.replace(' ', ''), 0)
    except ValueError:
        _refuse(text)


def _ctype(spec, structs, text):
    """'const float* const*' -> c_void_p, 'int64_t' -> c_int64, 'mg_adam_tail' -> that Structure; anything else is refused."""
    words = [w for w in spec.replace('*', ' * ').split() if w != 'const']
    if not words or not re.fullmatch(r'\w+', words[0]) or any(w != '*' for w in words[1:]):
        _refuse(text)
    if len(words) > 1:
        return ctypes.c_void_p
    ctype = _SCALARS.get(words[0], structs.get(words[0]))
    return ctype if ctype is not None else _refuse(text)


def _fields(body, constants, structs):
    fields = []
    for statement in filter(None, (s.strip() for s in body.split(';'))):
        base = ''
        for declarator in statement.split(','):      # `int rows, cols;`: later declarators share the type up to its first `*`
            spec, name, length = (_DECLARATOR.match(base + declarator.strip()) or _refuse(statement)).groups()
            base = base or spec.split('*')[0].strip() + ' '
            ctype = _ctype(spec, structs, statement)
            fields.append((name, ctype if length is None else ctype * _integer(length, constants, statement)))
    return fields


def _signature(statement):
    returns, name, params = (_PROTOTYPE.match(statement) or _refuse(statement)).groups()
    if returns.split() == ['void']:
        restype = None
    elif returns.replace('*', ' * ').split() == ['const', 'char', '*']:
        restype = ctypes.c_char_p
    else:
        restype = _ctype(returns, {}, statement)
        if restype is ctypes.c_void_p:
            _refuse(statement)
    argtypes = []
    for param in ([] if params.split() in ([], ['void']) else params.split(',')):
        spec, _, length = (_DECLARATOR.match(param.strip()) or _refuse(statement)).groups()
        ctype = _ctype(spec, {}, statement)      # scalars and pointers only: no entry point takes a struct by value
        argtypes.append(ctype if length is None else ctypes.c_void_p)      # `const uint32_t counter[4]` is a pointer
    return name, (restype, argtypes)


def parse_header(text):
    """The C ABI of include/morgana_hip.h as (constants, structs, signatures): {'MG_X': int}, {'mg_x_desc': ctypes.Structure
    subclass} and {'mg_x': (restype, argtypes)}.  Raises MorganaHipError, quoting the text, on anything it has no mapping for."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    constants, structs, signatures, code = {}, {}, {}, []
    for line in text.split('\n'):
        if not line.lstrip().startswith('#'):
            code.append(line)
        elif _DEFINE.match(line.strip()):
            name, value = _DEFINE.match(line.strip()).groups()
            constants[name] = _integer(value.strip('() '), constants, line)
        elif not _DIRECTIVE.match(line.strip()):
            _refuse(line)
    code = re.sub(r'extern\s+"C"\s*\{(.*)\}', r'\1', '\n'.join(code), flags=re.S)

    def struct(match):      # in the header's order: a struct may hold an earlier one by value
        body, name = match.groups()
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': _fields(body, constants, structs),
                                                         '__doc__': '%s of include/morgana_hip.h.' % name})
        return ''

    for statement in filter(None, (s.strip() for s in _STRUCT.sub(struct, code).split(';'))):
        name, signature = _signature(statement)
        signatures[name] = signature
    return constants, structs, signatures


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise MorganaHipError('the C ABI header is missing (%s): %s.  The binding is derived from it.' % (HEADER_PATH, e))


# MG_* constants, mg_* descriptor structs and SIGNATURES = name -> (restype, argtypes) of every entry point: include/morgana_hip.h
# parsed under the mapping above (tests/test_abi.py holds it against the C compiler's layouts and the library's exports).
CONSTANTS, STRUCTS, SIGNATURES = parse_header(_read_header())
globals().update(CONSTANTS)      # _lib.MG_CAST_MAX, ...
globals().update(STRUCTS)        # _lib.mg_cast_desc, ...
_lib = None


def load():
    """dlopen the HIP library once and attach the signatures.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get('MORGANA_HIP_LIB', LIB_PATH)      # the diagnostic build (make diag) for scripts/stamps.py
    if not os.path.exists(path):
        raise MorganaHipError(
            'libmorgana_hip.so is missing (%s): build it with `python -c "import __graft_entry__ as g; g.build()"` '
            'or `make -C morgana_amd/csrc`.  There is no CPU fallback.' % path)
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    for item in filter(None, os.environ.get('MG_TUNE', '').split(',')):      # experiments: MG_TUNE=key:value[,key:value]
        key, value = item.split(':')
        lib.mg_set_tuning(int(key), int(value))
    _lib = lib
    return lib


def last_error():
    return load().mg_last_error().decode('utf-8', 'replace')


CALL_LOG = None      # debugging aid: set to a list and every C-ABI call that went through check() appends its entry-point name


def check(rc, what):
    if CALL_LOG is not None:
        CALL_LOG.append(what)
    if rc != 0:
        msg = last_error()
        if rc == MG_EINVAL:
            raise ValueError('%s: %s' % (what, msg))
        raise MorganaHipError('%s failed (code %d): %s' % (what, rc, msg))
