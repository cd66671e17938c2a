"""ctypes binding of ``libococc_hip.so``.  The C ABI is declared in ``include/ococc_hip.h`` and nowhere else: the
signatures and descriptor structs below are read from the header when this module is imported (``_abi.py``).

The library is the product: there is no CPU or PyTorch fallback behind these
calls.  Importing this module without the built library raises, and every op
refuses tensors that do not live on a ROCm device.
"""
import ctypes
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('OCOCC_LIB_PATH') or os.path.join(_HERE, 'libococc_hip.so')   # (the override: diagnostic builds, tools/probe)

F32, BF16 = 0, 1
REDUCE = {'sum': 0, 'mean': 1, 'avg': 1, 'max': 2}

c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

# ococc_conv_ln: the LayerNorm epilogue of the three convolution exports (pass None for a plain convolution)
ConvLn = _abi.types['ococc_conv_ln']

# name -> (restype, argtypes) of every function include/ococc_hip.h declares, derived from its prototypes (_abi.py)
SIGNATURES = {name: (res, [ct for ct, _ in params]) for name, (res, params) in _abi.functions.items()}


class Timer(object):
    """One HIP event behind the C ABI (ococc_timer_*), recorded on torch's current stream."""

    def __init__(self):
        h = c_vp()
        check(lib.ococc_timer_create(ctypes.byref(h)), 'timer_create')
        self.h = h

    def record(self, in_graph=False):
        check(lib.ococc_timer_record(self.h, int(in_graph), stream()), 'timer_record')

    def elapsed_ms(self, stop):
        ms = c_f32()
        check(lib.ococc_timer_elapsed_ms(self.h, stop.h, ctypes.byref(ms)), 'timer_elapsed')
        return float(ms.value)

    def __del__(self):
        try:
            lib.ococc_timer_destroy(self.h)
        except Exception:  # interpreter shutdown
            pass


class OcoccError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} is missing: build the HIP kernels first '
            '(python -c "import __graft_entry__ as g; g.build()" or '
            '`make -C objectcentricocccompletion_amd/csrc`). There is no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc, what=''):
    if rc != 0:
        msg = lib.ococc_last_error().decode(errors='replace')
        raise OcoccError(f'{what} failed with code {rc}: {msg}')


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise OcoccError('ococc ops run on a ROCm device only; got a CPU tensor '
                             '(there is no CPU fallback)')


def ptr(t):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def stream():
    """hipStream_t of torch's current stream on the current device (the raw accessor: building a torch.cuda.Stream
    object per kernel launch cost ~11 us of host time, 1.4 ms per OcOccNet step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def f3(v):
    return (c_f32 * 3)(*[float(x) for x in v])


def f6(v):
    return (c_f32 * 6)(*[float(x) for x in v])


def i3(v):
    return (c_i32 * 3)(*[int(x) for x in v])


def i4(v):
    v = list(v) + [1] * (4 - len(v))
    return (c_i32 * 4)(*[int(x) for x in v])


def dtype_code(dt):
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    raise OcoccError(f'unsupported dtype {dt}; the kernels take float32 or bfloat16')


_CONSTS = {}


def const_tensor(values, device, dtype=torch.float32):
    """A small read-only constant on `device`, uploaded once per (values, device, dtype): building it per call
    (torch.tensor(list, device=...)) is a pageable host-to-device copy, i.e. a host synchronisation, every time."""
    key = (tuple(float(v) for v in values), str(device), dtype)
    t = _CONSTS.get(key)
    if t is None:
        t = _CONSTS[key] = torch.tensor(key[0], dtype=dtype, device=device)
    return t


_plan = None  # the BufferPlan in force (None: plain torch.empty)


def empty(shape, dtype, device):
    """torch.empty, or the next buffer of the BufferPlan in force."""
    if _plan is not None:
        return _plan.take(tuple(int(v) for v in shape), dtype, device)
    return torch.empty(shape, dtype=dtype, device=device)


class BufferPlan(object):
    """Caller-owned output memory for a chain of ops whose wrappers allocate through L.empty / L.workspace.

    The first ``with plan:`` block records every buffer the wrapped calls allocate; every later block hands the same
    tensors back in the same order (the calls must repeat with the same shapes and dtypes -- checked).  With two plans
    a captured HIP graph can write the geometry of the NEXT batch into one set of buffers while the training kernels
    of the same graph read the other set (graph.PipelinedStep)."""

    def __init__(self):
        self.bufs, self.pos, self.recorded = [], 0, False

    def take(self, shape, dtype, device):
        if not self.recorded:
            t = torch.empty(shape, dtype=dtype, device=device)
            self.bufs.append(t)
            return t
        if self.pos >= len(self.bufs):
            raise OcoccError('BufferPlan: more allocations than in the recorded run')
        t = self.bufs[self.pos]
        self.pos += 1
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != torch.device(device):
            raise OcoccError(f'BufferPlan: allocation {self.pos - 1} was {tuple(t.shape)} {t.dtype}, now {shape} {dtype}')
        return t

    def __enter__(self):
        global _plan
        if _plan is not None:
            raise OcoccError('BufferPlan: plans do not nest')
        self.pos = 0
        _plan = self
        return self

    def __exit__(self, *exc):
        global _plan
        _plan = None
        if exc[0] is None and self.recorded and self.pos != len(self.bufs):
            raise OcoccError('BufferPlan: fewer allocations than in the recorded run')
        self.recorded = True
        return False


def workspace(nbytes, device):
    """Caller-owned scratch buffer (the C ABI never allocates)."""
    return empty((max(int(nbytes), 1),), torch.uint8, device)


def count_scan_fill(tiles, groups, cols, device, count, fill):
    """The host side of an ordered compaction in two launches (csrc/wave_compact.hpp): ``count(tile_counts,
    group_counts)`` launches the count pass, the exclusive scan of tile_counts [tiles] says where each tile's survivors
    start, the counts per group [groups] are the ONE read-back, and ``fill(scan, out, n)`` launches the fill pass into
    out [n, cols] f32.  Returns (out, the counts per group as a list of int, what ``fill`` returned)."""
    tile_counts = empty((tiles,), torch.int32, device)
    group_counts = empty((groups,), torch.int64, device)
    count(tile_counts, group_counts)
    scan = torch.cumsum(tile_counts, 0, dtype=torch.int64) - tile_counts
    counts = [int(v) for v in group_counts.tolist()]
    out = empty((sum(counts), cols), torch.float32, device)
    return out, counts, fill(scan, out, out.size(0))


_logged = set()


def log_once(key, msg, level='warning'):
    """one line on the package logger the first time ``key`` is seen: a fused kernel that does not cover a module's shape
    falls back to the operator-by-operator path -- correct, several times slower, and otherwise silent"""
    if key not in _logged:
        _logged.add(key)
        import logging
        getattr(logging.getLogger('objectcentricocccompletion_amd'), level)(msg)
