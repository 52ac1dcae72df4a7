"""The whole C ABI in one place: every declaration of include/var_hip.h against the symbols libvar_hip.so exports and the ctypes binding
var_amd/abi.py derives from that header, argument by argument; the partition of the declarations into the signature tables; the oracle's
twins; the constants; and the parser's strictness on synthetic headers.  The header is read here a second time by a loose reading of its
own (a '*' makes a pointer, otherwise the first word is the type), so a mistake of abi.parse_header does not agree with itself."""
import ctypes
import os
import re

import pytest

from tests import util
from var_amd import abi, hip

HDR = open(os.path.join(util.ROOT, 'include', 'var_hip.h')).read()
KIND = {'int': abi.I, 'int64_t': abi.L, 'float': abi.F, 'double': abi.D}
RET = {'int': abi.I, 'int64_t': abi.L, 'const char*': ctypes.c_char_p}


def _declared():
    """{name: (return type text, [parameter texts])} of every `varhip_<name>(...);` outside the comments"""
    txt = re.sub(r'/\*.*?\*/', ' ', HDR, flags=re.S)
    out = {}
    for m in re.finditer(r'(const char\*|\bint64_t|\bint)\s+varhip_(\w+)\s*\(([^;]*?)\)\s*;', txt, re.S):
        params = [' '.join(p.split()) for p in m.group(3).split(',')]
        out.setdefault(m.group(2), (m.group(1), [] if params == ['void'] else params))
    assert set(out) == {n[len('varhip_'):] for n in re.findall(r'\b(varhip_\w+)\s*\(', txt)}, 'a declaration this reading does not take in'
    return out


def _kind(p):
    return abi.P if '*' in p or p.endswith(']') else KIND[p.split()[0]]


DECLARED = _declared()
LAUNCHERS = {**abi.SIGNATURES, **abi.SIGNATURES_F16, **abi.SIGNATURES_BF16, **abi.SIGNATURES_HIP_ONLY}


def test_every_declaration_is_exported_and_bound_as_declared():
    assert set(DECLARED) == set(abi.DECLS) and len(DECLARED) >= 124
    raw = ctypes.CDLL(hip.LIB_PATH)
    lib = hip.lib()
    for name, (ret, params) in DECLARED.items():
        assert hasattr(raw, 'varhip_' + name), f'{name}: declared and not exported'
        fn = (lib.host if name in abi.SIGNATURES_HOST else lib.fn).get(name)
        assert fn is not None and fn is getattr(lib.so, 'varhip_' + name), f'{name}: not bound in hip.lib()'
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        stream = bool(params) and params[-1] == 'varhip_stream_t stream'
        assert not any('varhip_stream_t' in p for p in params[:-1]), name
        for p, ct in zip(params[:-1] if stream else params, fn.argtypes):
            assert ct is _kind(p), (name, p, ct)
        assert stream == (name in LAUNCHERS), f'{name}: the stream is last exactly for the launchers'
        assert not stream or fn.argtypes[-1] is abi.P, name
        assert fn.restype is RET[ret], (name, ret, fn.restype)
    assert 'gfx950' in lib.version()


def test_the_tables_partition_the_declarations():
    tables = (abi.SIGNATURES, abi.SIGNATURES_F16, abi.SIGNATURES_BF16, abi.SIGNATURES_HIP_ONLY, abi.SIGNATURES_HOST)
    keys = [k for t in tables for k in t]
    assert len(keys) == len(set(keys)), 'an entry point in two tables'
    assert set(keys) <= set(DECLARED), f'in a table and not in the header: {sorted(set(keys) - set(DECLARED))}'
    for t in tables:                                         # name -> the declared classes without the stream
        for name, sig in t.items():
            params = DECLARED[name][1]
            assert sig == [_kind(p) for p in params if p != 'varhip_stream_t stream'], name
    assert set(abi.SIGNATURES) == set(abi.TWINNED) and set(abi.SIGNATURES_F16) == set(abi.BASE_F16)
    with_stream = {n for n, (_, ps) in DECLARED.items() if ps and ps[-1] == 'varhip_stream_t stream'}
    assert set(LAUNCHERS) == with_stream
    assert set(abi.SIGNATURES_HIP_ONLY) == with_stream - set(abi.TWINNED) - set(abi.SIGNATURES_F16) - set(abi.SIGNATURES_BF16)
    # the plain host functions: no stream, host pointers, an int return code; the rest without a stream are hooks, helpers and reports
    assert all(abi.P in sig and DECLARED[n][0] == 'int' and (n.endswith('_host') or '_host_' in n) for n, sig in abi.SIGNATURES_HOST.items())
    rest = set(DECLARED) - with_stream - set(abi.SIGNATURES_HOST)
    assert not any('host' in n for n in rest) and [n for n in rest if any('*' in p for p in DECLARED[n][1])] == ['timing_read']
    assert set(hip.lib().fn) == set(LAUNCHERS) | rest and set(hip.lib().host) == set(abi.SIGNATURES_HOST)


def test_every_twin_is_exported_by_the_oracle_with_the_same_list_minus_the_stream():
    util.ensure_oracle_built()
    so = ctypes.CDLL(os.path.join(util.ROOT, 'oracle', 'libvar_oracle.so'))
    twins = abi.bind(so, 'varref_', with_stream=False)
    assert set(twins) == set(abi.SIGNATURES) | set(abi.TWIN_HELPERS)
    for name in twins:
        assert hasattr(so, 'varref_' + name), name
        mine = hip.lib().fn[name]
        assert list(twins[name].argtypes) == list(mine.argtypes)[:len(mine.argtypes) - (name in abi.SIGNATURES)], name
        assert twins[name].restype is mine.restype, name
    for name, sig in abi.SIGNATURES.items():
        assert list(twins[name].argtypes) == sig, name


def test_the_bf16_table_is_the_f16_table_name_for_name():
    ren = lambda k: k.replace('_f16out', '_bf16out').replace('_to_f16', '_to_bf16').replace('cast_f16_', 'cast_bf16_').replace('_f16', '_bf16')
    assert list(abi.SIGNATURES_BF16) == [ren(k) for k in abi.SIGNATURES_F16] and not set(abi.SIGNATURES_BF16) & set(abi.SIGNATURES_F16)
    for k, sig in abi.SIGNATURES_F16.items():
        assert 'f16' in k and 'bf16' in ren(k) and abi.SIGNATURES_BF16[ren(k)] == sig, k
        assert DECLARED[ren(k)] == DECLARED[k], k                          # the same parameter text, names included


def test_the_constants_are_the_headers_defines():
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define VARHIP_(\w+) \(?(-?\d+)\)?$', HDR, re.M)}
    assert defs == abi.CONSTANTS and set(defs) == {'EINVAL', 'EPI_NONE', 'EPI_GELU', 'EPI_RESID', 'VQ_STATS_MAX_BLOCKS', 'NFAM'}
    assert (abi.EINVAL, abi.EPI_NONE, abi.EPI_GELU, abi.EPI_RESID) == (defs['EINVAL'], defs['EPI_NONE'], defs['EPI_GELU'], defs['EPI_RESID']) == (-1, 0, 1, 2)
    assert hip.VQ_STATS_MAX_BLOCKS == defs['VQ_STATS_MAX_BLOCKS'] and hip.NFAM == defs['NFAM']
    name = hip.lib().so.varhip_timing_name                            # a family past the table is answered with "?"
    names = [name(i) for i in range(-2, hip.NFAM + 16)]
    assert sum(n is not None and n != b'?' for n in names) == hip.NFAM and len(set(names[2:2 + hip.NFAM])) == hip.NFAM


# ---- the parser refuses what it cannot classify ------------------------------------------------------------------------------------------
def test_parser_reads_a_small_header():
    decls, consts = abi.parse_header('''
        /* a comment; with a semicolon */
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define VARHIP_EINVAL (-1)
        #define VARHIP_NFAM 3   /* families */
        typedef void* varhip_stream_t;
        const char* varhip_version(void);
        // a line comment; too
        int64_t varhip_elems(int B, int64_t n);
        int varhip_block(const uint32_t ctr[4], const void* const* src, void * const *dst, float eps, double t,
                         int64_t ld, const int* pn, varhip_stream_t stream);
        int varhip_hook(int on);
        int varhip_hook(int tile);
        #ifdef __cplusplus
        }
        #endif
        #endif /* X_H */
    ''')
    P, I, L, F, D = abi.P, abi.I, abi.L, abi.F, abi.D
    assert consts == {'EINVAL': -1, 'NFAM': 3}
    assert decls == {'version': (ctypes.c_char_p, [], False), 'elems': (L, [I, L], False),
                     'block': (I, [P, P, P, F, D, L, P], True), 'hook': (I, [I], False)}
    assert abi.parse_header('int varhip_f(const uint32_t key[2]);')[0]['f'] == (I, [P], False)      # `const T name[n]` is a pointer


@pytest.mark.parametrize('what, text', [
    ('an unknown parameter type', 'int varhip_f(size_t n);'),
    ('a pointer to an unknown type', 'int varhip_f(const foo_t* p);'),
    ('a parameter with no type', 'int varhip_f(int a, b);'),
    ('a type with no parameter name', 'int varhip_f(int);'),
    ('a declaration split by a comment containing ;', 'int varhip_f(int a, /* rows; then */ int b);'),
    ('a comment between the type and the name', 'int /* rc */ varhip_f(int a);'),
    ('a struct returned by value', 'struct pair varhip_f(int a);'),
    ('an unknown return type', 'float varhip_f(int a);'),
    ('a struct passed by value', 'int varhip_f(struct pair p);'),
    ('a function pointer', 'int varhip_f(int (*cb)(int), int n);'),
    ('a varargs list', 'int varhip_f(const char* fmt, ...);'),
    ('a stream that is not last', 'int varhip_f(varhip_stream_t stream, int n);'),
    ('a stream under another name', 'int varhip_f(int n, varhip_stream_t s);'),
    ('a 16-bit scalar by value', 'int varhip_f(uint8_t flag);'),
    ('two different declarations of one name', 'int varhip_f(int a);\nint varhip_f(int64_t a);'),
    ('a statement that is no declaration', 'int varhip_f(int a);\nstatic int x = 3;'),
    ('a constant that is no integer', '#define VARHIP_SCALE 1.5f\nint varhip_f(int a);'),
])
def test_parser_refuses(what, text):
    with pytest.raises(ValueError, match='varhip_f|VARHIP_SCALE|static int x'):
        abi.parse_header(text)
