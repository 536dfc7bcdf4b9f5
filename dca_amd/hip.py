"""ctypes binding of libdcahip.so (include/dcahip.h) -- the only door to the HIP kernels.

There is NO fallback: if the shared library is missing, or a kernel is asked to run on anything
but device memory of an AMD GPU, this module raises.  PyTorch is used for what it is good at
here -- owning device buffers and streams; tensors cross the boundary as raw device pointers.
"""
import ctypes
import os
import re

import torch

from . import build as _build

_c = ctypes

NLL_HAS_PI = 1
NLL_CONST_DISP = 2
NLL_POISSON = 4
NLL_MSE = 8

REG_MAX_SEGS = 16


class SmallLayer(_c.Structure):
    """dcahip_small_layer (include/dcahip.h)."""
    _fields_ = [('W', _c.c_void_p), ('ldw', _c.c_long), ('bias', _c.c_void_p), ('K', _c.c_int), ('H', _c.c_int),
                ('beta', _c.c_void_p), ('moving_mean', _c.c_void_p), ('moving_var', _c.c_void_p),
                ('Z', _c.c_void_p), ('ldz', _c.c_long), ('xhat', _c.c_void_p), ('ldx', _c.c_long),
                ('Hout', _c.c_void_p), ('ldh', _c.c_long), ('inv_std', _c.c_void_p)]


class StackBwdLayer(_c.Structure):
    """dcahip_stack_bwd_layer (include/dcahip.h)."""
    _fields_ = [('W', _c.c_void_p), ('ldw', _c.c_long), ('K', _c.c_int), ('H', _c.c_int),
                ('Hact', _c.c_void_p), ('ldh', _c.c_long), ('xhat', _c.c_void_p), ('ldx', _c.c_long),
                ('inv_std', _c.c_void_p), ('Hprev', _c.c_void_p), ('ldp', _c.c_long),
                ('gW', _c.c_void_p), ('ldg', _c.c_long), ('dbeta', _c.c_void_p), ('dH', _c.c_void_p), ('lddh', _c.c_long),
                ('beta', _c.c_void_p)]


class RegDesc(_c.Structure):
    """dcahip_reg_desc (include/dcahip.h)."""
    _fields_ = [('nseg', _c.c_int), ('start', _c.c_long * REG_MAX_SEGS), ('end', _c.c_long * REG_MAX_SEGS),
                ('l1', _c.c_float * REG_MAX_SEGS), ('l2', _c.c_float * REG_MAX_SEGS)]


ACT_CODES = {'linear': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3, 'elu': 4, 'selu': 5, 'softplus': 6,
             'softsign': 7, 'LeakyReLU': 8, 'hard_sigmoid': 10, 'exponential': 11, 'swish': 12, 'gelu': 13}
ACT_PRE = 12        # codes from here up take their slope from the pre-activation (include/dcahip.h, conventions)

OPT_KINDS = {'sgd': 0, 'rmsprop': 1, 'adagrad': 2, 'adadelta': 3, 'adam': 4, 'adamax': 5}

_SCALARS = {'int': _c.c_int, 'long': _c.c_long, 'long long': _c.c_long, 'unsigned long long': _c.c_ulonglong,
            'float': _c.c_float, 'double': _c.c_double}
_STRUCTS = {'dcahip_small_layer': SmallLayer, 'dcahip_stack_bwd_layer': StackBwdLayer, 'dcahip_reg_desc': RegDesc}
_POINTEES = set(_SCALARS) | {'void', 'unsigned', 'unsigned char'}


def _ctype(param):
    """ctypes type of one parameter of a declaration ('long ldh', 'const float* beta', 'unsigned* const* flags',
    'int out[8]': an array parameter is a pointer)."""
    param = re.sub(r'^(.*\S)\s+(\w+)\s*\[\s*\d*\s*\]$', r'\1* \2', param)
    words = param.replace('*', ' * ').split()
    if '*' in words:
        base = ' '.join(w for w in words[:words.index('*')] if w != 'const')
        if base in _STRUCTS:
            return _c.POINTER(_STRUCTS[base])
        if base in _POINTEES:
            return _c.c_void_p
    elif ' '.join(words[:-1]) in _SCALARS:               # the last word is the parameter's name
        return _SCALARS[' '.join(words[:-1])]
    raise ValueError('dca_amd.hip: include/dcahip.h: cannot bind the parameter %r' % param)


def _parse_header(text):
    """{name: (restype, argtypes)} of every `int|long dcahip_*(...)` declaration of the header text.  A declaration that
    does not have that form, or a parameter type without a ctypes counterpart, raises: an entry point is never skipped."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    sigs = {}
    for res, name, params in re.findall(r'\b(int|long)\s+(dcahip_\w+)\s*\(([^()]*)\)\s*;', text):
        params = [q.strip() for q in params.split(',')]
        sigs[name] = (_SCALARS[res], [] if params in ([''], ['void']) else [_ctype(q) for q in params])
    missed = set(re.findall(r'\b(dcahip_\w+)\s*\(', text)) - set(sigs)
    if missed:
        raise ValueError('dca_amd.hip: include/dcahip.h: cannot split the declaration of %s' % ', '.join(sorted(missed)))
    return sigs


# the header the library is compiled against (build.py fingerprints it) is the one table of argument types
with open(os.path.join(_build.ROOT, 'include', 'dcahip.h')) as _f:
    _SIGNATURES = _parse_header(_f.read())

_lib = None


class HipExtensionMissing(RuntimeError):
    pass


def lib():
    """Loads libdcahip.so once (building it with hipcc first if it is absent or stale)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if _build.needs_build():
        try:
            _build.build_hip(verbose=False)
        except Exception as e:  # noqa: BLE001
            if not os.path.exists(path):
                raise HipExtensionMissing(
                    'dca_amd: libdcahip.so is missing and could not be built (%s). The HIP '
                    'extension is mandatory; there is no CPU fallback.' % e) from e
    try:
        L = ctypes.CDLL(path)
    except OSError as e:
        raise HipExtensionMissing('dca_amd: cannot load %s: %s' % (path, e)) from e
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)          # AttributeError => header / library mismatch: loud
        fn.restype, fn.argtypes = res, args
    assert L.dcahip_version() == 2
    _lib = L
    return L


def exported_symbols():
    return sorted(_SIGNATURES)


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError('dca_amd: no AMD GPU visible (torch.cuda.is_available() is False); the '
                           'training path runs on MI355X only -- there is no CPU fallback.')


def ptr(t):
    """Device pointer of a tensor (None -> NULL). Refuses host memory."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('dca_amd.hip: host tensor passed to a HIP kernel')
    return t.data_ptr()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream():
    """Raw handle of torch's current stream on the current device (every kernel is launched on it).  The
    private fast getter saves ~8 us per launch over torch.cuda.current_stream() (two dozen launches per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def check(rc, what):
    if rc != 0:
        raise RuntimeError('dca_amd.hip: %s failed with code %d' % (what, rc))
