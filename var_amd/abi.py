"""ctypes bindings of the C ABI, derived from include/var_hip.h.

The header is the one description of libvar_hip.so: parse_header() reads every `varhip_<name>(...)` declaration and every integer
`#define VARHIP_*`, and the signature tables below are built from that parse.  Two consumers: var_amd/hip.py binds `varhip_<name>(..., stream)`
in libvar_hip.so (the product), the CPU checker under oracle/ binds `varref_<name>(...)` in its own shared library.  One source for the
argument lists is what lets the parity tests drive both libraries with identical arguments.
"""
import ctypes as C
import os
import re

P = C.c_void_p
I = C.c_int
L = C.c_int64
F = C.c_float
D = C.c_double

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'var_hip.h')

_SCALAR = {'int': I, 'int64_t': L, 'float': F, 'double': D}
_POINTEE = set(_SCALAR) | {'void', 'char', 'int32_t', 'uint8_t', 'uint32_t'}
_RETURN = {'int': I, 'int64_t': L, 'const char*': C.c_char_p}
_PARAM = re.compile(r'(?:const\s+)?(\w+)\b\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(\[\d*\])?')      # type, stars, name, [n]
_DECL = re.compile(r'([\w\s*]*?)\bvarhip_(\w+)\s*\(([^()]*)\)')


def parse_header(text: str):
    """-> ({name: (restype, [argument ctypes], has_stream)}, {NAME: int of `#define VARHIP_NAME`}) of a header in the form of include/var_hip.h.

    Strict: once comments and preprocessor lines are gone, every statement must be the stream typedef or one declaration whose return type
    and parameters are all of a known class (pointer or `name[n]`: P; int: I; int64_t: L; float: F; double: D; `varhip_stream_t stream`,
    last).  Anything else raises ValueError naming the statement: a wrong guess here is a truncated stride or a shifted pointer in a
    kernel's arguments.  A comment inside a declaration is refused too (nothing in the header needs one)."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', '@', text, flags=re.S)
    consts = {}
    for line in re.findall(r'^[ \t]*#[^\n]*', text, re.M):
        m = re.fullmatch(r'\s*#\s*define\s+VARHIP_(\w+)\s+\(?(-?\d+)\)?[\s@]*', line)
        if m:
            consts[m.group(1)] = int(m.group(2))
        elif re.match(r'\s*#\s*define\s+VARHIP_', line):
            raise ValueError(f'include/var_hip.h: cannot read the constant `{line.strip()}`')
    text = re.sub(r'^[ \t]*#[^\n]*', '', text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', '', text)
    decls = {}
    for stmt in text.split(';'):
        stmt = stmt.strip('@} \t\n')
        if not stmt or re.fullmatch(r'typedef\s+void\s*\*\s*varhip_stream_t', stmt):
            continue
        m = _DECL.fullmatch(stmt)
        ret = re.sub(r'\s*\*', '*', ' '.join(m.group(1).split())) if m else None
        if ret not in _RETURN:
            raise ValueError(f'include/var_hip.h: cannot classify `{" ".join(stmt.split())}`')
        name, params = m.group(2), [p.strip() for p in m.group(3).split(',')]
        args = []
        stream = params[-1] == 'varhip_stream_t stream'
        for p in ([] if params == ['void'] else params[:-1] if stream else params):
            pm = _PARAM.fullmatch(p)
            if pm and (pm.group(2) or pm.group(4)) and pm.group(1) in _POINTEE:
                args.append(P)
            elif pm and not (pm.group(2) or pm.group(4)) and pm.group(1) in _SCALAR:
                args.append(_SCALAR[pm.group(1)])
            else:
                raise ValueError(f'include/var_hip.h: varhip_{name}: cannot classify the parameter `{p}`')
        decl = (_RETURN[ret], args, stream)
        if decls.setdefault(name, decl) != decl:
            raise ValueError(f'include/var_hip.h: varhip_{name} is declared twice with different signatures')
    return decls, consts


if not os.path.exists(HEADER):
    raise ImportError(f'{HEADER} not found: the ctypes bindings are derived from it, so var_amd is used from the repository tree')
with open(HEADER) as _f:
    DECLS, CONSTANTS = parse_header(_f.read())

# Two partitions no declaration shows.  The entry points with a CPU twin `varref_<name>` in oracle/var_oracle.c:
TWINNED = ('gemm_nt_f32', 'silu_f32', 'add_bcast_f32', 'ln_modulate_f32', 'qkv_prep_f32', 'attn_cached_f32', 'cfg_sample_f32', 'quant_accum_f32',
           'next_map_f32', 'lvl_pos_f32', 'first_map_f32', 'conv3x3_nhwc_f32', 'gn_stats_f32', 'gn_apply_f32', 'softmax_rows_f32', 'nchw_to_nhwc_f32',
           'nhwc_to_nchw_f32', 'nearest_code_f32', 'nearest_code_cos_f32', 'token_select_i64', 'conv3x3_s2_nhwc_f32', 'nchw_to_nhwc_pad_f32',
           'area_pool_f32', 'word_embed_f32', 'quant_residual_f32', 'upconv_pack_f32', 'upconv_phase_f32', 'quant_accum_h_f32', 'gumbel_softmax_f32',
           'gemm_qkv_f32', 'conv3x3_gn_nhwc_f32', 'upconv_phase_gn_f32', 'gn_stats_part_f32', 'adaln_block_f32', 'neighbor_table_f32',
           'smooth_select_f32')
TWIN_HELPERS = ('gn_scratch_elems', 'conv_gn_blocks', 'version')      # ... and what the oracle exports beside them (no stream on either side)
# the 16-bit throughput mode (its CPU twin is oracle/var_oracle.py with f16=True: the fp32 functions + rounding points), and one bfloat16
# entry point per _f16 entry point with the same arguments (include/var_hip.h, "bf16")
BASE_F16 = ('gemm_nt_f16', 'gemm_qkv_f16', 'attn_cached_f16', 'ln_modulate_f16out', 'adaln_block_f16', 'conv3x3_nhwc_f16', 'upconv_phase_f16',
            'gnconv3x3_nhwc_f16', 'gn_stats_f16', 'gn_apply_f16', 'gn_silu_conv_out_f16', 'cast_f32_to_f16', 'cast_f16_to_f32')
BASE_BF16 = tuple(k.replace('_f16out', '_bf16out').replace('_to_f16', '_to_bf16').replace('cast_f16_', 'cast_bf16_').replace('_f16', '_bf16')
                  for k in BASE_F16)

# name -> argument ctypes without the trailing stream.  Launchers (the declarations that end in a stream): twinned, the two 16-bit flavours,
# and the rest, which have no oracle twin of their own (the header says beside each what it is pinned against).
SIGNATURES = {k: DECLS[k][1] for k in TWINNED}
SIGNATURES_F16 = {k: DECLS[k][1] for k in BASE_F16}
SIGNATURES_BF16 = {k: DECLS[k][1] for k in BASE_BF16}
SIGNATURES_HIP_ONLY = {k: d[1] for k, d in DECLS.items() if d[2] and k not in TWINNED + BASE_F16 + BASE_BF16}
# No stream: the plain host functions (host pointers, no GPU needed; hip.call_host) are those that take a pointer, the timing table's reader
# aside; everything else is a hook, a size helper or a report (hip.lib().so.varhip_<name>).
SIGNATURES_HOST = {k: d[1] for k, d in DECLS.items() if not d[2] and P in d[1] and not k.startswith('timing_')}

EPI_NONE, EPI_GELU, EPI_RESID = CONSTANTS['EPI_NONE'], CONSTANTS['EPI_GELU'], CONSTANTS['EPI_RESID']
EINVAL = CONSTANTS['EINVAL']
with open(HEADER) as _f:
    CODEC_PB = int(re.search(r'^#define VARCODEC_PB (\d+)$', _f.read(), re.M).group(1))      # precision bits of the coding tables (codec.hip)


def bind(lib, prefix: str, with_stream: bool):
    """Attach argtypes/restype to the ABI functions of `lib` -> {name: function}; raises AttributeError naming a missing symbol.
    with_stream (libvar_hip.so): every declaration of the header; the plain host functions are bound on `lib` like the rest and left out
    of the result (var_amd/hip.py keeps them apart, in .host).  Without (the oracle): the twins and their helpers, no stream argument."""
    fns = {}
    for name in (DECLS if with_stream else TWINNED + TWIN_HELPERS):
        ret, args, stream = DECLS[name]
        fn = getattr(lib, prefix + name)
        fn.argtypes = args + [P] if stream and with_stream else list(args)
        fn.restype = ret
        if name not in SIGNATURES_HOST:
            fns[name] = fn
    return fns
