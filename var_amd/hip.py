"""ctypes binding of libvar_hip.so (include/var_hip.h).  The product path has no fallback: a missing or unloadable
library raises here, and every non-zero return code of a kernel launcher raises VarHipError."""
import ctypes
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VARHIP_LIB') or os.path.join(_HERE, 'libvar_hip.so')      # (VARHIP_LIB: A/B experiments against another build of the library)


class VarHipError(RuntimeError):
    pass


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise VarHipError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                              f'(or `make -C var_amd/csrc`). There is no CPU/PyTorch fallback for the sampling path.')
        self.so = ctypes.CDLL(LIB_PATH)
        self.fn = abi.bind(self.so, 'varhip_', with_stream=True)
        self.host = {name: getattr(self.so, 'varhip_' + name) for name in abi.SIGNATURES_HOST}      # bound by abi.bind with the rest

    def version(self) -> str:
        return self.fn['version']().decode()


_LIB = None


def lib() -> _Lib:
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB


def _arg(a):
    if a is None:
        return None
    if hasattr(a, 'data_ptr'):
        return ctypes.c_void_p(a.data_ptr())
    return a


def current_stream() -> ctypes.c_void_p:
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name: str, *args, stream=None):
    """Launch `varhip_<name>` on torch's current stream (tensors are passed by data_ptr); raises on a non-zero code."""
    L = lib()
    st = current_stream() if stream is None else stream
    rc = L.fn[name](*[_arg(a) for a in args], st)
    if rc != 0:
        raise VarHipError(f'varhip_{name} returned {rc}' + (' (VARHIP_EINVAL: unsupported shape/argument)' if rc == abi.EINVAL else ' (HIP launch error %d)' % (-rc - 1000)))


def call_host(name: str, *args):
    """Run the plain host function `varhip_<name>` (abi.SIGNATURES_HOST: no stream, no GPU; CPU tensors and numpy arrays are passed by
    address); raises on a non-zero code."""
    def arg(a):
        if hasattr(a, 'ctypes'):
            return ctypes.c_void_p(a.ctypes.data)
        return _arg(a)
    if name not in abi.SIGNATURES_HOST:
        raise VarHipError(f'varhip_{name} is not a host function')
    rc = lib().host[name](*[arg(a) for a in args])
    if rc != 0:
        raise VarHipError(f'varhip_{name} returned {rc}' + (' (VARHIP_EINVAL: unsupported shape/argument)' if rc == abi.EINVAL else ''))


def gn_scratch_elems(B, HW, C, G) -> int:
    return int(lib().fn['gn_scratch_elems'](B, HW, C, G))


def conv_gn_blocks(H, W, Cout, phase=False) -> int:
    """blocks per sample of the GroupNorm partials a conv can leave behind (0: unsupported shape)"""
    return int(lib().fn['conv_gn_blocks'](H, W, Cout, 1 if phase else 0))


def upconv_winograd(on: bool):
    """the library's switch for varhip_upconv_phase[_gn]_f32 (vh_g_upconv_wino, winograd.hip; off by default): on, a launch whose output tiles
    into 16 x 16 patches with channels in multiples of 32 runs as position-sparse Winograd.  DecoderEngine.upsample sets it around its launch."""
    ctypes.c_int.in_dll(lib().so, 'vh_g_upconv_wino').value = 1 if on else 0


def _wino_hook(name, nargs):
    """the workgroup-shape hooks of varhip_conv3x3_wino_nhwc_f32 (winograd.hip): exported beside the header's entry points, ints in and out"""
    fn = getattr(lib().so, 'varhip_wino_' + name)
    fn.argtypes, fn.restype = [ctypes.c_int] * nargs, ctypes.c_int
    return fn


def wino_force_shape(shape: int):
    """-1: the library's own rule; 0: 64 tiles x 32 channels per workgroup; 1: the wide shape, 32 tiles x 80 channels, where Cout % 80 == 0
    (elsewhere shape 0 still runs).  Both shapes give the same bits.  Tests and experiments: reset to -1 in a `finally`."""
    _wino_hook('force_shape', 1)(int(shape))


def wino_last_shape() -> int:
    """the shape the latest accepted varhip_conv3x3_wino_nhwc_f32 launch took (-1 before the first)"""
    return int(_wino_hook('last_shape', 0)())


def wino_auto_shape(H, W, Cin, Cout) -> int:
    """the shape the library's own rule gives this level (host arithmetic: no GPU, no launch)"""
    return int(_wino_hook('auto_shape', 4)(H, W, Cin, Cout))


def conv16_gn_fusable(B, H, W, Cin, Cout) -> bool:
    """can the 16-bit conv apply the GroupNorm + SiLU in front of it to its own input patch (varhip_gnconv3x3_nhwc_*)?"""
    return bool(lib().fn['conv16_gn_fusable'](B, H, W, Cin, Cout))


VQ_STATS_MAX_BLOCKS = abi.CONSTANTS['VQ_STATS_MAX_BLOCKS']      # VARHIP_VQ_STATS_MAX_BLOCKS of include/var_hip.h: doubles of scratch varhip_vq_scale_stats_f32 takes


def vq_stats_blocks(n: int) -> int:
    """workgroup partials of varhip_vq_scale_stats_f32's float64 sum over n elements (its summation order depends on n through this alone)"""
    return int(lib().so.varhip_vq_stats_blocks(n))


# ---- timing table --------------------------------------------------------------------------------------------------
NFAM = abi.CONSTANTS['NFAM']            # VARHIP_NFAM of include/var_hip.h


def timing_enable(on: bool, families=None):
    """families: names of the kernel families to time (None = all); each timed launch records two events on the stream"""
    so = lib().so
    mask = -1
    if families is not None:
        names = [so.varhip_timing_name(i).decode() for i in range(NFAM)]
        mask = sum(1 << names.index(f) for f in families)
    so.varhip_timing_select(mask)
    so.varhip_timing_enable(1 if on else 0)


def timing_reset():
    lib().so.varhip_timing_reset()


def timing_read():
    """-> {family: dict(ms, flops, bytes, launches)} (synchronises the recorded events)"""
    n = abi_nfam = NFAM
    ms = (ctypes.c_double * n)(); fl = (ctypes.c_double * n)(); by = (ctypes.c_double * n)(); ln = (ctypes.c_int64 * n)()
    lib().so.varhip_timing_read(ms, fl, by, ln)
    return {lib().so.varhip_timing_name(i).decode(): dict(ms=ms[i], flops=fl[i], bytes=by[i], launches=int(ln[i])) for i in range(abi_nfam)}
