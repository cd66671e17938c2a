"""CPU suite: the ctypes binding is derived from include/ococc_hip.h (objectcentricocccompletion_amd/_abi.py).  The reader on
literal snippets, its strictness, and the real header against hand-written pins: signatures in literal ctypes, the three
descriptor structs' sizes and offsets, and the host_ naming rule."""
import ctypes
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p

import pytest

from objectcentricocccompletion_amd import _abi
from test_abi_cpu import _declared

SNIPPET = '''
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define OCOCC_OK 0
typedef void* ococc_stream_t; /* hipStream_t */
typedef struct ococc_desc {
  int32_t a, b;       /* two in one declaration */
  float eps[8];
  const float* w_frag[8];
  int64_t partial_rows;
  uint16_t* y;
} ococc_desc;
typedef struct {
  double d;
} ococc_anon;
/* ococc_in_a_comment(int x); is not a declaration */
const char* ococc_name(void);
int64_t ococc_bytes(int64_t n, const float host_size[3],
                    const int32_t host_shape[4],
                    uint32_t t, uint64_t seed);
int ococc_run(const float* x, /* device */ float* host_ms, const int64_t* host_rows, void* const* host_tbl,
              const void* const* host_src, void** host_out, float* const* host_f, const ococc_desc* d, double lr,
              int flag, const ococc_anon* e, const uint16_t* const* table, ococc_stream_t stream);
int32_t ococc_rows(int64_t n);
#ifdef __cplusplus
}
#endif
'''


def test_reader_on_a_literal_header():
    functions, structs, types = _abi.parse(SNIPPET)
    assert list(functions) == ['ococc_name', 'ococc_bytes', 'ococc_run', 'ococc_rows']      # header order
    assert functions['ococc_name'] == (c_char_p, [])
    assert functions['ococc_rows'] == (c_int32, [(c_int64, 'n')])
    assert functions['ococc_bytes'] == (c_int64, [(c_int64, 'n'), (c_float * 3, 'host_size'), (c_int32 * 4, 'host_shape'),
                                                  (c_uint32, 't'), (c_uint64, 'seed')])
    res, params = functions['ococc_run']
    assert res is c_int32
    assert params == [(c_void_p, 'x'), (POINTER(c_float), 'host_ms'), (POINTER(c_int64), 'host_rows'),
                      (POINTER(c_void_p), 'host_tbl'), (POINTER(c_void_p), 'host_src'), (POINTER(c_void_p), 'host_out'),
                      (POINTER(c_void_p), 'host_f'), (POINTER(types['ococc_desc']), 'd'), (c_double, 'lr'), (c_int32, 'flag'),
                      (POINTER(types['ococc_anon']), 'e'), (c_void_p, 'table'), (c_void_p, 'stream')]
    assert structs['ococc_desc'] == [('a', c_int32), ('b', c_int32), ('eps', c_float * 8), ('w_frag', c_void_p * 8),
                                     ('partial_rows', c_int64), ('y', c_void_p)]
    assert structs['ococc_anon'] == [('d', c_double)]
    assert issubclass(types['ococc_desc'], ctypes.Structure) and types['ococc_desc']._fields_ == structs['ococc_desc']
    assert ctypes.sizeof(types['ococc_desc']) == 8 + 32 + 64 + 8 + 8


@pytest.mark.parametrize('decl, names', [
    ('int ococc_f(size_t n);', ['ococc_f', 'size_t']),
    ('int ococc_f(int32_t n, unsigned flags);', ['ococc_f', 'unsigned']),
    ('int ococc_f(int32_t n, void (*done)(int32_t));', ['ococc_f']),
    ('int ococc_f(const char* fmt, ...);', ['ococc_f']),
    ('int ococc_f(const ococc_unknown* p);', ['ococc_f', 'ococc_unknown']),
    ('typedef struct { int32_t a; } ococc_s;\nint ococc_f(const ococc_s* host_p);', ['ococc_f', 'host_p']),
    ('int ococc_f(void* host_p);', ['ococc_f', 'host_p']),
    ('int ococc_f(long n);', ['ococc_f', 'long']),
    ('size_t ococc_f(int32_t n);', ['ococc_f', 'size_t']),
    ('typedef struct { int32_t a; size_t b; } ococc_s;', ['ococc_s', 'size_t']),
    ('#define ococc_macro(x) (x)\nint ococc_f(int32_t n);', ['ococc_macro']),
    ('static inline int ococc_f(int32_t n) { return n; }', ['ococc_f']),
])
def test_reader_refuses_what_it_does_not_know(decl, names):
    with pytest.raises(_abi.AbiError) as err:
        _abi.parse(decl)
    for name in names:
        assert name in str(err.value)


def test_real_header_is_the_table_the_library_is_bound_with():
    from objectcentricocccompletion_amd import _lib
    assert sorted(_abi.functions) == _declared() and len(_abi.functions) >= 147
    assert set(_abi.functions) == set(_lib.SIGNATURES)
    for name, (res, params) in _abi.functions.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and _lib.SIGNATURES[name][0] is res, name
        assert len(fn.argtypes) == len(params) == len(_lib.SIGNATURES[name][1]), name
        for got, listed, (ct, _) in zip(fn.argtypes, _lib.SIGNATURES[name][1], params):
            assert got is ct and listed is ct, name


def test_signatures_pinned_by_hand():
    """one export per parameter shape, written out in literal ctypes (from the table this binding had when it was typed in by
    hand), so that the derived table is not checked against itself alone"""
    from objectcentricocccompletion_amd import _lib
    from objectcentricocccompletion_amd.sir import _RelChainDesc
    vp, i32, i64, f32 = c_void_p, c_int32, c_int64, c_float
    pins = {
        'ococc_last_error': (c_char_p, []),
        'ococc_hard_voxelize_workspace_bytes': (i64, [i64, f32 * 3, f32 * 6]),
        'ococc_dynamic_voxelize_f32': (i32, [vp, i64, i32, f32 * 3, f32 * 6, vp, vp]),
        'ococc_frame_match_f32': (i32, [vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, i32, i32, i64, i64, i32, f32 * 5, vp, vp,
                                        vp, i64, vp]),
        'ococc_latent_ln_adam_f32': (i32, [vp, vp, vp, vp, i64, i32, vp, f32, i32, c_double, c_double, c_double, c_double,
                                           i32, vp, vp]),
        'ococc_layernorm_act_dropout_fwd_bf16': (i32, [vp, i64, i32, vp, vp, f32, i32, c_uint32, c_uint64, vp, vp, vp]),
        'ococc_adamw_operands_f32': (i32, [i32, POINTER(vp), POINTER(vp), POINTER(vp), POINTER(vp), POINTER(i64), f32, vp,
                                           f32, f32, f32, f32, vp, i32, i32, POINTER(i32), POINTER(i32), POINTER(i32),
                                           POINTER(i32), POINTER(i32), POINTER(vp), vp]),
        'ococc_sparse_conv_tile_bf16': (i32, [vp, i64, i32, vp, i32, i32, vp, i32, i64, vp, vp, i32, POINTER(_lib.ConvLn),
                                              vp]),
        'ococc_timer_create': (i32, [POINTER(vp)]),
        # the descriptor array and the two host tables of device pointers were untyped addresses in that table
        'ococc_sir_rel_chains_fwd_f32': (i32, [i32, POINTER(_RelChainDesc), vp, i64, POINTER(vp), POINTER(vp), vp]),
    }
    for name, (res, args) in pins.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res, name
        assert len(got_args) == len(args) and all(a is b for a, b in zip(got_args, args)), name


LAYOUTS = {   # sizeof, [(field, offset, size)]: what the hand-written ctypes.Structure mirrors reported
    'ococc_conv_ln': (72, [('backward', 0, 4), ('act', 4, 4), ('eps', 8, 4), ('gamma', 16, 8), ('beta', 24, 8), ('y', 32, 8),
                           ('mean_rstd', 40, 8), ('block_conv_out', 48, 8), ('partials', 56, 8), ('partial_rows', 64, 8)]),
    'ococc_sir_layer': (416, [('n_rel', 0, 4), ('n_vfe', 4, 4), ('feat_cols', 8, 4), ('cluster_cols', 12, 4),
                              ('with_cluster_center', 16, 4), ('shortcut', 20, 4), ('bscale', 24, 4), ('inference', 28, 4),
                              ('rel_colscale', 32, 8), ('colscale', 40, 8), ('n', 48, 32), ('act', 80, 32), ('eps', 112, 32),
                              ('w_frag', 144, 64), ('wt_frag', 208, 64), ('ln_weight', 272, 64), ('ln_bias', 336, 64),
                              ('gate', 400, 8), ('dgate', 408, 8)]),
    'ococc_sir_rel_chain': (192, [('n_blocks', 0, 4), ('cluster_cols', 4, 4), ('rel_colscale', 8, 8), ('n', 16, 16),
                                  ('act', 32, 16), ('eps', 48, 16), ('w_frag', 64, 32), ('wt_frag', 96, 32),
                                  ('ln_weight', 128, 32), ('ln_bias', 160, 32)]),
}


def test_descriptor_struct_layouts():
    from objectcentricocccompletion_amd import _lib, sir
    assert set(_abi.structs) == set(LAYOUTS)
    assert _lib.ConvLn is _abi.types['ococc_conv_ln'] and sir._SirLayerDesc is _abi.types['ococc_sir_layer'] \
        and sir._RelChainDesc is _abi.types['ococc_sir_rel_chain']
    for name, (size, fields) in LAYOUTS.items():
        cls = _abi.types[name]
        assert ctypes.sizeof(cls) == size, name
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields, name
    assert [t for _, t in _abi.structs['ococc_conv_ln']] == [c_int32, c_int32, c_float] + [c_void_p] * 6 + [c_int64]
    d = sir._SirLayerDesc()
    d.eps[7], d.w_frag[7], d.dgate = 0.5, 1 << 40, 3       # float[8], pointer[8] and pointer members take what call sites store
    assert (d.eps[7], d.w_frag[7], d.dgate) == (0.5, 1 << 40, 3)


def test_host_pointers_are_named_host():
    """typed pointers (which refuse a tensor.data_ptr() int) are exactly the host_* pointers; arrays are passed by value of
    their ctypes array type; everything else a prototype calls a pointer is an untyped device address"""
    typed = array = 0
    for name, (_, params) in _abi.functions.items():
        for ct, pname in params:
            if issubclass(ct, ctypes.Array):
                array += 1
                assert pname.startswith('host_') and ct._type_ in (c_float, c_int32), (name, pname)
            elif issubclass(ct, ctypes._Pointer) and not issubclass(ct._type_, ctypes.Structure):
                typed += 1
                assert pname.startswith('host_'), (name, pname)
                assert ct._type_ in (c_void_p, c_int32, c_int64, c_uint64, c_float), (name, pname)
            else:
                assert not pname.startswith('host_'), (name, pname)
    assert typed >= 137 and array >= 37      # today's header: the rule is not vacuous
