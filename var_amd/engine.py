"""Host side of the MI355X sampling path: drives the HIP kernels of libvar_hip.so for one (VAR, VQVAE) pair.

This is what `VAR.autoregressive_infer_cfg` (reference models/var.py:126-190) and `VQVAE.fhat_to_img`
(models/vqvae.py:62-63) run on a GPU.  PyTorch supplies device memory, the RNG stream and the current HIP stream;
every floating-point operation of the path happens in a kernel reached through `hip.call` (include/var_hip.h).
There is no CPU / eager fallback here: without the library `hip.lib()` raises.

Differences from the reference's schedule (results unchanged):
  * the per-block AdaLN projection `ada_lin(cond)` is computed once per call instead of once per scale
    (it only depends on the class embedding: basic_var.py:156, var.py:165-169);
  * the KV cache is pre-allocated [2B, H, L, 64] per block and appended in place (no torch.cat, basic_var.py:107-109);
  * activations of the decoder are channels-last; f_hat is kept [B, P, P, Cvae] and only transposed at the API edge.
"""
from __future__ import annotations

import math
import os
import weakref
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch

from . import hip
from .abi import EPI_GELU, EPI_NONE, EPI_RESID
from .workspace import Dims, allocate, cached, keep_precision, sampler_rows, workspace_spec


def bicubic_taps(pn: int, P: int):
    """4-tap index/weight table of F.interpolate(mode='bicubic', align_corners=False) for pn -> P (reference quant.py:190).
    Follows ATen's upsample_bicubic2d in fp32: src = (pn/P)*(dst+0.5)-0.5, taps floor(src)-1..+2 clamped, Keys kernel A=-0.75."""
    f = np.float32
    A = f(-0.75)
    scale = f(pn) / f(P)
    src = scale * (np.arange(P, dtype=np.float32) + f(0.5)) - f(0.5)
    i0 = np.floor(src)
    t = (src - i0).astype(np.float32)

    def near(x):
        return ((A + f(2)) * x - (A + f(3))) * x * x + f(1)

    def far(x):
        return ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A
    w = np.stack([far(t + f(1)), near(t), near(f(1) - t), far((f(1) - t) + f(1))], axis=1).astype(np.float32)
    idx = np.clip(i0.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, pn - 1).astype(np.int32)
    return idx, w


def per_image_tables(cfg, top_k, top_p, S: int, V: int) -> dict:
    """the host tables of a per-image call: t [S, B] float64 with t[si][b] = cfg[b] * (si / (S - 1)) formed as the plain call forms its scalar (one
    fp64 division, one fp64 multiplication), top_k [B] int32, top_p [B] float64, and cap = the largest top_k (V if any image has none)"""
    B = len(cfg)
    c = np.asarray([float(x) for x in cfg], dtype=np.float64)
    t = np.stack([c * (si / (S - 1)) if S > 1 else np.zeros(B) for si in range(S)])
    k = np.asarray([int(x) for x in top_k], dtype=np.int32)
    return dict(t=t, top_k=k, top_p=np.asarray([float(x) for x in top_p], dtype=np.float64), cap=int(V if (k == 0).any() else k.max()))


def control_tables(cfg, top_k, top_p, temperature, min_p, logit_bias, S: int, V: int, B: int, cfg_ramp: bool = True) -> dict:
    """the host tables of a controlled call (VAR.sample_controlled).  Every knob is a scalar, (B,) or (S, B), a size-1 B axis broadcasting ((S, 1)
    is a pure per-scale schedule); logit_bias is None, (V,), (B, V) or (S, B, V), again with a size-1 B (models/args.py: control_args checks
    them) -> dict(t [S, B] float64, top_k [S, B] int32, top_p [S, B] float64, tau [S, B] float32, min_p [S, B] float32, cap [S] int: per scale
    the largest top_k (V if any image has none), bias [R, V] float32: the distinct bias rows in order of first use (None without a bias),
    bias_row [S, B] int32: each (scale, image)'s row of it, -1 = none).  cfg_ramp: t[s][b] = cfg[s][b] * (s / (S - 1)), formed exactly as
    per_image_tables forms it (the reference's ramp); without it t[s][b] = cfg[s][b], the schedule is the caller's."""
    from .models.args import control_args
    a = control_args(V, S, B, cfg, top_k, top_p, temperature, min_p, logit_bias)
    c = a['cfg']
    t = np.stack([c[si] * (si / (S - 1)) if S > 1 else np.zeros(B) for si in range(S)]) if cfg_ramp else c.copy()
    k = a['top_k'].astype(np.int32)
    cap = [int(V if (k[si] == 0).any() else k[si].max()) for si in range(S)]
    bias, bias_row = None, np.full((S, B), -1, dtype=np.int32)
    if a['bias'] is not None:
        src = a['bias'].reshape(-1, V)                                # the rows as given: a shared row is looked at once
        seen, rows, which = {}, [], np.empty(len(src), dtype=np.int32)
        for i, row in enumerate(src):
            which[i] = seen.setdefault(row.tobytes(), len(rows))
            if which[i] == len(rows):
                rows.append(row)
        bias = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
        bias_row = np.ascontiguousarray(np.broadcast_to(which.reshape(a['bias'].shape[:-1] or (1,)), (S, B)), dtype=np.int32)
    return dict(t=t, top_k=k, top_p=a['top_p'], tau=a['tau'], min_p=a['min_p'], cap=cap, bias=bias, bias_row=bias_row)


def compose_tables(cfg, weights, S: int) -> np.ndarray:
    """the coefficient table of a composed call (VAR.sample_composed): coef [S, B, K + 1] float32 from cfg (B values) and weights (S, B, K).
    With t = per_image_tables' t[si][b] and W = sum_k w_k, added in float64 in index order:
        a_k = fl32((1 + t) * w_k)  for the K class rows,    a_u = fl32(t + (1 + t) * (W - 1))  for the unconditional row, the last entry
    — u + (1 + t) * sum_k w_k (c_k - u) with the u terms collected — every entry evaluated in float64 and rounded once.  K = 1, w = 1 gives
    ((float)(1 + t), (float)t): the two scalars varhip_cfg_sample_rows_f32 derives from t."""
    w = np.asarray(weights, dtype=np.float64)
    Sw, B, K = w.shape
    if Sw != S or B != len(cfg):
        raise ValueError(f'weights must be ({S}, {len(cfg)}, K), got {tuple(w.shape)}')
    t = per_image_tables(cfg, [0] * B, [0.0] * B, S, 1)['t']
    W = np.zeros((S, B), dtype=np.float64)
    for k in range(K):                                            # index order
        W = W + w[:, :, k]
    one_t = 1.0 + t
    return np.concatenate((one_t[:, :, None] * w, (t + one_t * (W - 1.0))[:, :, None]), axis=2).astype(np.float32)


# the per-token outputs of varhip_sample_stats_f32 in the order of its arguments (the keys of SamplingEngine.sample's `stats`)
STATS_FIELDS = ('logp_cond', 'logp_guided', 'logp_drawn', 'kept', 'entropy')


def _stats_dtype(key: str) -> torch.dtype:
    return torch.int32 if key == 'kept' else torch.float32


def stats_record(shape: tuple, dev, fill: Optional[tuple] = None, fields: tuple = STATS_FIELDS) -> dict:
    """{field: tensor of `shape`} for the sampler's statistics; fill: (the value of `kept`, the value of the others), default uninitialised"""
    if fill is None:
        return {key: torch.empty(shape, dtype=_stats_dtype(key), device=dev) for key in fields}
    return {key: torch.full(shape, fill[0] if key == 'kept' else fill[1], dtype=_stats_dtype(key), device=dev) for key in fields}


def pointer_table(tensors) -> torch.Tensor:
    """the addresses of a list of device tensors as a host int64 array (the launcher that takes it copies it)"""
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64)


def phi_index(si: int, S: int, K: int) -> int:
    """which shared Phi conv serves scale si (reference quant.py:218-226)"""
    ticks = np.linspace(1 / 3 / K, 1 - 1 / 3 / K, K) if K == 4 else np.linspace(1 / 2 / K, 1 - 1 / 2 / K, K)
    return int(np.argmin(np.abs(ticks - si / (S - 1)))) if S > 1 else 0


PRECISIONS = ('f32', 'f16', 'bf16')
DT16 = {'f16': torch.float16, 'bf16': torch.bfloat16}      # storage type of the two 16-bit flavours (include/var_hip.h "f16" / "bf16")


def gemm_nt(prec: str, A, W, bias, out, M: int, N: int, K: int, *, lda: int, ldw: int, ldo: int, epi: int = EPI_NONE, resid=None, ldr: int = 0,
            gamma=None, ldg: int = 0, rpg: int = 1, bias_per_row: int = 0, batch: int = 1, sA: int = 0, sW: int = 0, sO: int = 0):
    """out[M, N] = epi(A[M, K] . W[N, K]^T + bias), `batch` of them at element strides sA / sW / sO, on varhip_gemm_nt_<prec>: the one place that
    knows the two argument orders.  The 16-bit entry points take A and W in `prec`, are told whether out and resid are 16-bit or fp32 (read
    off the tensors here) and have no per-row bias"""
    if prec == 'f32':
        hip.call('gemm_nt_f32', A, lda, W, ldw, bias, out, ldo, M, N, K, epi, resid, ldr, gamma, ldg, rpg, bias_per_row, batch, sA, sW, sO)
        return
    if bias_per_row:
        raise ValueError(f'varhip_gemm_nt_{prec} has no per-row bias')
    hip.call('gemm_nt_' + prec, A, lda, W, ldw, bias, out, ldo, int(out.dtype != torch.float32), M, N, K, epi, resid, ldr,
             int(resid is not None and resid.dtype != torch.float32), gamma, ldg, rpg, batch, sA, sW, sO)


def _ver(p: torch.Tensor) -> int:
    """version counter of a parameter; tensors created under torch.inference_mode() have none"""
    try:
        return p._version
    except RuntimeError:
        return -1


class _Signature:
    """what the engines key their re-laid weight copies on: the parameter OBJECTS (by weak reference), with the storage address and version
    counter of each.  Address and counter alone prove nothing: where an engine keeps only a packed copy of a parameter (ada_w_all, qkv_b,
    the Phi and decoder kernels) nothing holds the parameter's storage, and a replacement parameter comes out of the freed block with the
    old address and, filled the same way, the old version counter.  The weak reference to a parameter that was dropped is dead and equals
    nothing, and a parameter that is still alive somewhere keeps its address to itself.
    In-place writes through `.data` (p.data.mul_(), p.data.copy_()) bump no counter: after such surgery call `engine.invalidate()` (VAR /
    VQVAE do it from load_state_dict and init_weights)."""

    def __init__(self, params, extra: tuple = ()):
        params = list(params)
        self.refs = [weakref.ref(p) for p in params]
        self.key = tuple((p.data_ptr(), _ver(p)) for p in params) + tuple(extra)

    def __eq__(self, other):
        if not isinstance(other, _Signature) or self.key != other.key or len(self.refs) != len(other.refs):
            return False
        return all(a() is not None and a() is b() for a, b in zip(self.refs, other.refs))

    __hash__ = None


def _signature(params, extra: tuple = ()) -> _Signature:
    return _Signature(params, extra)


def _chk(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_cuda:
        raise hip.VarHipError(f'{name}: the MI355X sampling path needs fp32 CUDA parameters, got {t.dtype} on {t.device}')
    return t if t.is_contiguous() else t.contiguous()


class _Engine:
    """what every engine does with its packed weight copies (`w`, keyed on `_sig`): announce them to other streams, retire them, drop them"""

    def __init__(self):
        self._sig = None
        self.w: dict = {}
        self._ready = None              # event recorded behind the kernels that built the packed copies (they run on whichever stream called first)

    def _built(self):
        """packed copies were just (re)built on the current stream: calls arriving on OTHER streams wait for this event before they read them"""
        self._ready = torch.cuda.Event()
        self._ready.record()

    def _wait_ready(self):
        if self._ready is not None:
            torch.cuda.current_stream().wait_event(self._ready)

    def _retire(self):
        """weights changed: before the old packed copies go back to the allocator, every stream that may still read them has to finish (a weight
        change is rare — checkpoint load, EMA swap — so a device-wide wait is the simple safe form)"""
        if self.w and torch.cuda.is_available():
            torch.cuda.synchronize()

    def invalidate(self):
        """drop the packed weight copies: the next call re-reads the module's parameters"""
        self._sig = None


# ---- the quantizer's tables, as QuantizerEngine and SamplingEngine both keep them (each its own copy, under its own signature) ----------
def _pack_quantizer(quant):
    """(codebook [V][Cvae], [(Phi kernel [Cout][3][3][Cin], bias, resi_ratio), ...]) of a VectorQuantizer2"""
    return (_chk(quant.embedding.weight.detach(), 'codebook'),
            [(_chk(p.weight.detach(), 'phi').permute(0, 2, 3, 1).contiguous(), _chk(p.bias.detach(), 'phi'), float(p.resi_ratio))
             for p in quant.quant_resi.phis()])


def _tap_tables(cache: dict, pn: int, P: int, dev):
    """the bicubic tap tables pn -> P on the device, built once per pn in `cache` (one cache per P); (None, None) at pn == P: nothing to resample"""
    if pn == P:
        return None, None
    if pn not in cache:
        ti, tw = bicubic_taps(pn, P)
        cache[pn] = (torch.from_numpy(ti).to(dev), torch.from_numpy(tw).to(dev))
    return cache[pn]


def bilinear_axis(pn: int, size: int):
    """(i0, i1, l1): the axis table of F.interpolate(mode='bilinear', align_corners=False) for pn -> size, rows and columns alike (also for
    size < pn: the same formula, no antialiasing).  Follows ATen's upsample_bilinear2d in fp32: src = max((dst + 0.5) * (pn / size) - 0.5, 0) with
    the ratio and the product in fp32, i0 = int(src), i1 = min(i0 + 1, pn - 1), l1 = src - i0 (the weight of i1; i0 weighs 1 - l1)."""
    f = np.float32
    scale = f(pn) / f(size)
    src = np.maximum((np.arange(size, dtype=np.float32) + f(0.5)) * scale - f(0.5), f(0))
    i0 = src.astype(np.int32)
    i1 = np.minimum(i0 + 1, pn - 1).astype(np.int32)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def evidence_scales(patch_nums, scales):
    """(pn, begin, w) of the selected scales as varhip_evidence_* take them: int32, int32 (first token of the scale) and fp32
    w_s = float32(pn_s^2 / sum of the selected pn^2), numpy arrays"""
    begins = np.concatenate([[0], np.cumsum([p * p for p in patch_nums])])
    pn = np.asarray([patch_nums[s] for s in scales], dtype=np.int32)
    total = int((pn.astype(np.int64) ** 2).sum())
    w = np.asarray([np.float32(int(p) * int(p) / total) for p in pn], dtype=np.float32)
    return pn, np.asarray([begins[s] for s in scales], dtype=np.int32), w


# the limits of varhip_evidence_reduce_f32 / varhip_evidence_overlay_u8 (include/var_hip.h)
EVIDENCE_MAX_SCALES, EVIDENCE_MAX_STAGE, EVIDENCE_MAX_PN, EVIDENCE_MAX_SIZE, EVIDENCE_MAX_IMAGES = 16, 4096, 64, 4096, 65535
_AXIS_HOST: dict = {}              # (pn, size) -> bilinear_axis(pn, size)
_AXIS_DEVICE: dict = {}            # (selected pn, size, device) -> (ax_i [ns][size][2] int32, ax_l [ns][size] fp32) on the device


def evidence_axis_tables(pns: tuple, size: int, dev):
    """the axis tables of the selected scales on the device, built on the host once per (pn, size) and uploaded once per (scales, size, device)"""
    key = (tuple(int(p) for p in pns), int(size), str(dev))
    if key not in _AXIS_DEVICE:
        ai = np.empty((len(pns), size, 2), np.int32)
        al = np.empty((len(pns), size), np.float32)
        for s, pn in enumerate(key[0]):
            if (pn, size) not in _AXIS_HOST:
                _AXIS_HOST[(pn, size)] = bilinear_axis(pn, size)
            ai[s, :, 0], ai[s, :, 1], al[s] = _AXIS_HOST[(pn, size)]
        if len(_AXIS_DEVICE) >= 64:
            _AXIS_DEVICE.clear()
        _AXIS_DEVICE[key] = (torch.from_numpy(ai).to(dev), torch.from_numpy(al).to(dev))
    return _AXIS_DEVICE[key]


@torch.no_grad()
def evidence_maps_hip(scores: torch.Tensor, patch_nums, scales, size: int, image, image_pm1: bool, alpha: float, return_maps: bool) -> dict:
    """VAR.evidence_maps on the HIP path: scores (N, K, L) fp32 contiguous on the GPU, arguments already validated by the caller
    -> dict(lo, hi, pred, margin, area, maps | None, overlays | None).  Two entry points, no (N, K, size, size) tensor unless asked for."""
    N, K, L = scores.shape
    dev = scores.device
    pn, begin, w = evidence_scales(patch_nums, scales)
    stage = int(begin[-1]) + int(pn[-1]) ** 2 - int(begin[0])
    if len(pn) > EVIDENCE_MAX_SCALES or stage > EVIDENCE_MAX_STAGE or int(pn.max()) > EVIDENCE_MAX_PN or N > EVIDENCE_MAX_IMAGES or N * K >= 2 ** 31:
        raise ValueError(f'evidence_maps on the GPU takes at most {EVIDENCE_MAX_SCALES} scales of side <= {EVIDENCE_MAX_PN} spanning at most '
                         f'{EVIDENCE_MAX_STAGE} tokens, and at most {EVIDENCE_MAX_IMAGES} images')
    ax_i, ax_l = evidence_axis_tables(tuple(pn.tolist()), size, dev)
    host = (torch.from_numpy(pn), torch.from_numpy(begin), torch.from_numpy(w))
    with torch.cuda.device(dev):
        out = dict(lo=torch.empty(N, dtype=torch.float32, device=dev), hi=torch.empty(N, dtype=torch.float32, device=dev),
                   pred=torch.empty(N, size, size, dtype=torch.int32, device=dev), margin=torch.empty(N, size, size, dtype=torch.float32, device=dev),
                   area=torch.empty(N, K, dtype=torch.int32, device=dev),
                   maps=torch.empty(N, K, size, size, dtype=torch.float32, device=dev) if return_maps else None, overlays=None)
        hip.call('evidence_reduce_f32', scores, K * L, L, N, K, len(pn), *host, ax_i, ax_l, size,
                 out['lo'], out['hi'], out['pred'], out['margin'], out['area'], out['maps'])
        if image is not None:
            out['overlays'] = torch.empty(N, K, size, size, 3, dtype=torch.uint8, device=dev)
            hip.call('evidence_overlay_u8', scores, K * L, L, N, K, len(pn), *host, ax_i, ax_l, size,
                     out['lo'], out['hi'], image, 1 if image_pm1 else 0, float(alpha), out['overlays'])
    return out


def _scale_tables(taps: dict, phi: list, si: int, S: int, pn: int, P: int, dev):
    """(ti, tw, pw, pb, ratio): what the quantizer step of scale si (pn x pn of S scales, the last P x P) takes besides its tokens"""
    return _tap_tables(taps, pn, P, dev) + phi[phi_index(si, S, len(phi))]


# ---- the two VAE graphs: (kind, key) steps, read by the walk that runs them (_VaeOps._run) and by the decoder's FLOP counters --------------
def _decoder_graph(w: dict, nlev: int):
    """post_quant_conv, then Decoder.forward (reference basic_vae.py:163-226); attention blocks where the weight table `w` has them"""
    yield 'conv', 'post_quant_conv'
    yield 'conv', 'decoder.conv_in'
    yield 'res', 'decoder.mid.block_1'
    yield 'attn', 'decoder.mid.attn_1'
    yield 'res', 'decoder.mid.block_2'
    for lev in reversed(range(nlev)):
        for ib in range(3):
            yield 'res', f'decoder.up.{lev}.block.{ib}'
            if f'decoder.up.{lev}.attn.{ib}.norm.weight' in w:
                yield 'attn', f'decoder.up.{lev}.attn.{ib}'
        if lev != 0:
            yield 'up', f'decoder.up.{lev}.upsample.conv'
    yield 'tail', 'decoder'                                      # norm_out -> swish -> conv_out -> clamp


def _encoder_graph(w: dict, nlev: int):
    """Encoder.forward (reference basic_vae.py:99-160); quant_conv follows it in EncoderEngine.encode"""
    yield 'conv', 'encoder.conv_in'
    for lev in range(nlev):
        for ib in range(2):
            yield 'res', f'encoder.down.{lev}.block.{ib}'
            if f'encoder.down.{lev}.attn.{ib}.norm.weight' in w:
                yield 'attn', f'encoder.down.{lev}.attn.{ib}'
        if lev != nlev - 1:
            yield 'down', f'encoder.down.{lev}.downsample.conv'
    yield 'res', 'encoder.mid.block_1'
    yield 'attn', 'encoder.mid.attn_1'
    yield 'res', 'encoder.mid.block_2'
    yield 'norm_conv', 'encoder'                                 # norm_out -> swish -> conv_out


_NORM_FIRST = ('res', 'norm_conv', 'tail')                      # the steps that open with a GroupNorm of their input


class _VaeOps(_Engine):
    """What the decoder and encoder engines share: the packed weights, the walk over a VAE graph, and the fp32 set of channels-last building
    blocks (reference basic_vae.py:18-92).  `_Ops16` is the same set of blocks in 16-bit arithmetic; a call picks one of the two and walks."""

    PREFIXES = ()
    LEVELS = ''                     # prefix of the per-level weights: the highest index under it gives nlev
    # convs whose result a GroupNorm reads next but which run without the partial-sum epilogue in fp32: the encoder's conv_in has always run on
    # the plain kernel (the 16-bit one does leave partials), and its first ResnetBlock takes a statistics pass
    PLAIN_CONVS = ('encoder.conv_in',)
    fuse_gn = os.environ.get('VARHIP_FUSE_GN', '1') != '0'      # 16-bit blocks; False (tests, A/B runs): every GroupNorm + SiLU as its own pass in front of the conv (the same bits)

    def __init__(self, vae):
        super().__init__()
        self.vae = vae
        self._gn_part = None            # (tensor, partial sums, blocks per sample) left by the last conv for the GroupNorm after it

    def _signature(self):
        return _signature(self.vae.parameters())

    def refresh(self):
        sig = self._signature()
        if sig == self._sig:
            return
        self._retire()
        self.w = self._derive(self._pack())
        self.w16s = {}                       # {'f16' | 'bf16': 16-bit copies}: made by ops16() the first time such a call runs on these weights
        self.nlev = 1 + max(int(k.split('.')[2]) for k in self.w if k.startswith(self.LEVELS))
        self._sig = sig
        self._built()

    def _pack(self):
        """our copies of the weights this engine uses: 3x3 kernels re-laid [Cout][3][3][Cin] (Cin zero-padded to a multiple of 32),
        1x1 kernels as [Cout][Cin] matrices"""
        w = {}
        for k, v in self.vae.state_dict().items():
            if not k.startswith(self.PREFIXES) or not torch.is_floating_point(v):
                continue
            v = _chk(v.detach(), k)
            if v.dim() == 4 and v.shape[-1] == 3:
                v = v.permute(0, 2, 3, 1).contiguous()               # [Cout][Cin][3][3] -> [Cout][3][3][Cin]
                if v.shape[3] % 32:
                    pad = torch.zeros(v.shape[0], 3, 3, (v.shape[3] + 31) // 32 * 32, dtype=v.dtype, device=v.device)
                    pad[..., :v.shape[3]] = v
                    v = pad
                w[k] = v
            elif v.dim() == 4:
                w[k] = v.reshape(v.shape[0], v.shape[1])            # 1x1 conv == linear
            else:
                w[k] = v
        return w

    def _derive(self, w):
        """kernels derived from the packed ones (the decoder has some)"""
        return w

    def ops16(self, prec):
        """the 16-bit blocks for ONE call in flavour `prec`, over 16-bit copies of every conv kernel (3x3, phase, 1x1 shortcut, attention
        projections) made the first time the flavour runs on these weights; biases and GroupNorm affine stay fp32"""
        if prec not in self.w16s:
            self._wait_ready()
            self.w16s[prec] = {k: v.to(DT16[prec]).contiguous() for k, v in self.w.items()
                               if (k.endswith('.weight') or k.endswith('.phase')) and v.dim() >= 2 and '.norm' not in k}
            self._built()
        return _Ops16(self, prec, self.w16s[prec])

    def _run(self, ops, graph, h, B, Hh, Ww, **tail):
        """execute a VAE graph on the blocks of `ops` (this engine: fp32; an _Ops16: 16 bits).  A conv is asked for GroupNorm partials when the
        step behind it opens with a GroupNorm; none outlive the walk."""
        steps = list(graph)
        self._gn_part = None
        for (kind, key), (nxt, _) in zip(steps, steps[1:] + [(None, None)]):
            if kind == 'conv':
                h = ops.conv3(h, key, B, Hh, Ww, stats=nxt in _NORM_FIRST)
            elif kind == 'res':
                h = ops.resblock(h, key, B, Hh, Ww)
            elif kind == 'attn':
                h = ops.attnblock(h, key, B, Hh, Ww)
            elif kind == 'up':
                Hh, Ww = 2 * Hh, 2 * Ww
                h = ops.upsample(h, key, B, Hh, Ww)
            elif kind == 'down':
                Hh, Ww = Hh // 2, Ww // 2
                h = ops.downsample(h, key, B, Hh, Ww)
            elif kind == 'norm_conv':
                h = ops.norm_conv(h, key + '.norm_out', key + '.conv_out', B, Hh, Ww)
            else:
                h = ops.tail(h, key, B, Hh, Ww, **tail)
        self._gn_part = None
        return h

    # -- GroupNorm statistics handed from a conv to the norm behind it ------------------------------------------------------------------
    def _leave_partials(self, out, B, nblk):
        """`out` is about to be written by a conv whose epilogue also emits per-block channel sums, nblk blocks per sample (0: not for this
        shape) -> the buffer they go to (None at 0), remembered together with the tensor they describe for the GroupNorm that reads it next.
        Holding `out` keeps its address from being recycled before then."""
        self._gn_part = None
        if not nblk:
            return None
        part = torch.empty((B, nblk, out.shape[-1], 2), dtype=torch.float64, device=out.device)
        self._gn_part = (out, part, nblk)
        return part

    def _stats_from(self, x, B, HW, fn_full):
        """(mean, rstd) per (sample, group) of a channels-last map: folded from the producing conv's per-block partial sums when it left them for
        exactly this tensor, else by a statistics pass (`fn_full`) over x"""
        Cc = x.shape[-1]
        stats = torch.empty((B, 32, 2), dtype=torch.float32, device=x.device)
        pend, self._gn_part = self._gn_part, None
        if pend is not None and pend[0].data_ptr() == x.data_ptr() and pend[0].numel() == x.numel() and tuple(pend[1].shape) == (B, pend[2], Cc, 2):
            hip.call('gn_stats_part_f32', pend[1], stats, B, pend[2], HW, Cc, 32, 1e-6)
        else:
            scratch = torch.empty(hip.gn_scratch_elems(B, HW, Cc, 32), dtype=torch.float64, device=x.device)
            hip.call(fn_full, x, stats, scratch, B, HW, Cc, 32, 1e-6)
        return stats

    # -- the fp32 building blocks --------------------------------------------------------------------------------------------------------
    def _wino(self, key, Hh, Ww, Cin, Cout):
        """the Winograd-transformed kernel of conv `key` where that path takes this shape, else None (only the decoder engine keeps any)"""
        return None

    def conv3(self, x, key, B, Hh, Ww, resid=None, out_mode=0, stats=False):
        """stats=True: the result feeds a GroupNorm next — the conv epilogue also emits per-block channel sums (when the shape
        allows), which gn() then uses instead of a statistics pass over the tensor."""
        wt = self.w[key + '.weight']
        Cout, Cin = wt.shape[0], wt.shape[3]
        out = torch.empty((B, Cout, Hh, Ww) if out_mode else (B, Hh, Ww, Cout), dtype=torch.float32, device=x.device)
        nblk = hip.conv_gn_blocks(Hh, Ww, Cout) if (stats and out_mode == 0 and key not in self.PLAIN_CONVS) else 0
        wino = self._wino(key, Hh, Ww, Cin, Cout) if out_mode == 0 else None
        part = self._leave_partials(out, B, nblk)
        if wino is not None:
            hip.call('conv3x3_wino_nhwc_f32', x, wino, self.w[key + '.bias'], resid, out, part, B, Hh, Ww, Cin, Cout)
        elif nblk:
            hip.call('conv3x3_gn_nhwc_f32', x, wt, self.w[key + '.bias'], resid, out, part, B, Hh, Ww, Cin, Cout, 0)      # (0: no nearest-2x in front)
        else:
            hip.call('conv3x3_nhwc_f32', x, wt, self.w[key + '.bias'], resid, out, B, Hh, Ww, Cin, Cout, 0, out_mode)
        return out

    def gn_stats(self, x, B, HW):
        return self._stats_from(x, B, HW, 'gn_stats_f32')

    def gn(self, x, key, B, HW, silu):
        stats = self.gn_stats(x, B, HW)
        out = torch.empty_like(x)
        hip.call('gn_apply_f32', x, stats, self.w[key + '.weight'], self.w[key + '.bias'], out, B, HW, x.shape[-1], 32, int(silu))
        return out

    def norm_conv(self, x, nkey, ckey, B, Hh, Ww):
        """conv(swish(norm(x))) (basic_vae.py:57-60) as two passes; no partials: what follows it (the encoder's conv_out) is no GroupNorm"""
        return self.conv3(self.gn(x, nkey, B, Hh * Ww, True), ckey, B, Hh, Ww)

    def lin(self, x2d, key, resid=None):
        wt = self.w[key + '.weight']
        N, K = wt.shape
        M = x2d.shape[0]
        out = torch.empty((M, N), dtype=torch.float32, device=x2d.device)
        gemm_nt('f32', x2d, wt, self.w[key + '.bias'], out, M, N, K, lda=K, ldw=K, ldo=N, epi=EPI_RESID if resid is not None else EPI_NONE, resid=resid, ldr=N)
        return out

    def resblock(self, x, pre, B, Hh, Ww):
        HW = Hh * Ww
        h = self.conv3(self.gn(x, pre + '.norm1', B, HW, True), pre + '.conv1', B, Hh, Ww, stats=True)        # -> norm2
        hn = self.gn(h, pre + '.norm2', B, HW, True)
        sc = self.lin(x.view(B * HW, -1), pre + '.nin_shortcut').view(B, Hh, Ww, -1) if (pre + '.nin_shortcut.weight') in self.w else x
        return self.conv3(hn, pre + '.conv2', B, Hh, Ww, resid=sc, stats=True)                                  # -> the next block's norm

    def attnblock(self, x, pre, B, Hh, Ww):
        HW, Cc = Hh * Ww, x.shape[-1]
        dev = x.device
        xn = self.gn(x, pre + '.norm', B, HW, False).view(B * HW, Cc)
        wqkv, bqkv = self.w[pre + '.qkv.weight'], self.w[pre + '.qkv.bias']
        qk = torch.empty((B * HW, 2 * Cc), dtype=torch.float32, device=dev)
        gemm_nt('f32', xn, wqkv, bqkv, qk, B * HW, 2 * Cc, Cc, lda=Cc, ldw=Cc, ldo=2 * Cc)
        vt = torch.empty((B, Cc, HW), dtype=torch.float32, device=dev)                   # V^T[b][c][j], bias per row (c)
        gemm_nt('f32', wqkv[2 * Cc:], xn, bqkv[2 * Cc:], vt, Cc, HW, Cc, lda=Cc, ldw=Cc, ldo=HW, bias_per_row=1, batch=B, sA=0, sW=HW * Cc, sO=Cc * HW)
        s = torch.empty((B, HW, HW), dtype=torch.float32, device=dev)
        gemm_nt('f32', qk, qk[:, Cc:], None, s, HW, HW, Cc, lda=2 * Cc, ldw=2 * Cc, ldo=HW, batch=B, sA=HW * 2 * Cc, sW=HW * 2 * Cc, sO=HW * HW)
        p = torch.empty_like(s)
        hip.call('softmax_rows_f32', s, p, B * HW, HW, float(np.float32(int(Cc) ** (-0.5))))
        o = torch.empty((B * HW, Cc), dtype=torch.float32, device=dev)
        gemm_nt('f32', p, vt, None, o, HW, Cc, HW, lda=HW, ldw=HW, ldo=Cc, batch=B, sA=HW * HW, sW=Cc * HW, sO=HW * Cc)
        return self.lin(o, pre + '.proj_out', resid=x.view(B * HW, Cc)).view(B, Hh, Ww, Cc)


def _tail_mode(denorm, clamp):
    """out_mode of the decoder's last conv: 1 clamp and (x + 1) / 2, 2 clamp to [-1, 1], 3 the value as it is"""
    return 3 if not clamp else (1 if denorm else 2)


class _Ops16:
    """The building blocks of _VaeOps on 16-bit activations and conv weights with fp32 accumulation (conv16.hip, rowops16.hip, conv16s2.hip):
    the same methods, for the same walk.  One object per call, made by `_VaeOps.ops16` from a flavour and the engine's weight copies of that
    flavour, so a call's precision is nobody's state but its own.  `fl` ('f16' | 'bf16') is the flavour and the suffix of its entry points, `dt`
    its storage type, `w16` the 16-bit kernels; biases and GroupNorm affine are the engine's fp32 ones (`w`), and GroupNorm partials are handed
    over through the engine like the fp32 ones."""

    def __init__(self, eng: _VaeOps, fl: str, w16: dict):
        self.eng, self.w, self.w16, self.fl, self.dt = eng, eng.w, w16, fl, DT16[fl]

    def _to16(self, x32, shape=None):
        y = torch.empty(x32.shape if shape is None else shape, dtype=self.dt, device=x32.device)
        hip.call('cast_f32_to_' + self.fl, x32, y, y.numel())
        return y

    def _to32(self, x16):
        y = torch.empty(x16.shape, dtype=torch.float32, device=x16.device)
        hip.call(f'cast_{self.fl}_to_f32', x16, y, y.numel())
        return y

    def conv3(self, x, key, B, Hh, Ww, resid=None, out_mode=0, stats=False):
        wt = self.w16[key + '.weight']
        Cout, Cin = wt.shape[0], wt.shape[3]
        out = torch.empty((B, Cout, Hh, Ww), dtype=torch.float32, device=x.device) if out_mode else torch.empty((B, Hh, Ww, Cout), dtype=self.dt, device=x.device)
        nblk = hip.conv_gn_blocks(Hh, Ww, Cout) if (stats and out_mode == 0 and Cout % 4 == 0) else 0
        part = self.eng._leave_partials(out, B, nblk)
        hip.call('conv3x3_nhwc_' + self.fl, x, wt, self.w[key + '.bias'], resid, out, part, B, Hh, Ww, Cin, Cout, out_mode)
        return out

    def gn_stats(self, x, B, HW):
        return self.eng._stats_from(x, B, HW, 'gn_stats_' + self.fl)

    def gn(self, x, key, B, HW, silu):
        stats = self.gn_stats(x, B, HW)
        out = torch.empty_like(x)
        hip.call('gn_apply_' + self.fl, x, stats, self.w[key + '.weight'], self.w[key + '.bias'], out, B, HW, x.shape[-1], 32, int(silu))
        return out

    def norm_conv(self, x, nkey, ckey, B, Hh, Ww, resid=None):
        """conv(swish(norm(x))) (basic_vae.py:57-60): one launch where the halo-patch conv can normalise its own input patch, else apply pass + conv.
        Always leaves partials: its callers are ResnetBlocks (after the encoder's conv_out nobody reads them, and the walk drops them)"""
        wt = self.w16[ckey + '.weight']
        Cout, Cin = wt.shape[0], wt.shape[3]
        if not (self.eng.fuse_gn and hip.conv16_gn_fusable(B, Hh, Ww, Cin, Cout)):
            return self.conv3(self.gn(x, nkey, B, Hh * Ww, True), ckey, B, Hh, Ww, resid=resid, stats=True)
        stats = self.gn_stats(x, B, Hh * Ww)
        out = torch.empty((B, Hh, Ww, Cout), dtype=self.dt, device=x.device)
        part = self.eng._leave_partials(out, B, hip.conv_gn_blocks(Hh, Ww, Cout) if Cout % 4 == 0 else 0)
        table = torch.empty((B, 2, Cin), dtype=torch.float32, device=x.device)
        hip.call('gn_scale_shift_f32', stats, self.w[nkey + '.weight'], self.w[nkey + '.bias'], table, B, Cin, 32)
        hip.call('gnconv3x3_nhwc_' + self.fl, x, table, 1, wt, self.w[ckey + '.bias'], resid, out, part, B, Hh, Ww, Cin, Cout)
        return out

    def resblock(self, x, pre, B, Hh, Ww):
        HW = Hh * Ww
        h = self.norm_conv(x, pre + '.norm1', pre + '.conv1', B, Hh, Ww)
        sc = x
        if (pre + '.nin_shortcut.weight') in self.w16 and self.w16[pre + '.nin_shortcut.weight'].shape[1] % 64:
            # (the encoder's 160 -> 320 shortcut: the 16-bit GEMM contracts 64 at a time) the fp32 GEMM between two casts
            sc32 = self.eng.lin(self._to32(x).view(B * HW, -1), pre + '.nin_shortcut')
            sc = self._to16(sc32, (B, Hh, Ww, sc32.shape[1]))
        elif (pre + '.nin_shortcut.weight') in self.w16:              # 1x1 conv == fp16 GEMM over the pixels
            wt = self.w16[pre + '.nin_shortcut.weight']
            N, K = wt.shape
            sc = torch.empty((B, Hh, Ww, N), dtype=self.dt, device=x.device)
            gemm_nt(self.fl, x, wt, self.w[pre + '.nin_shortcut.bias'], sc, B * HW, N, K, lda=K, ldw=K, ldo=N)
        return self.norm_conv(h, pre + '.norm2', pre + '.conv2', B, Hh, Ww, resid=sc)

    def attnblock(self, x, pre, B, Hh, Ww):
        """AttnBlock (basic_vae.py:73-92) on fp16 activations: the five products (q/k projection, V^T projection, q.k^T, p.v, proj_out + residual)
        on the f16 MFMA GEMM with fp32 accumulation; scores and softmax in fp32, the probabilities rounded to fp16 for p.v"""
        HW, Cc = Hh * Ww, x.shape[-1]
        dev = x.device
        f16 = self.dt
        if Cc % 64 or HW % 64:                     # (tiny test configurations: the f16 GEMM contracts 64 at a time) fp32 attention between two casts
            x32 = self._to32(x)
            self.eng._gn_part = None
            return self._to16(self.eng.attnblock(x32, pre, B, Hh, Ww))
        xn = self.gn(x, pre + '.norm', B, HW, False).view(B * HW, Cc)
        wqkv, bqkv = self.w16[pre + '.qkv.weight'], self.w[pre + '.qkv.bias']
        qk = torch.empty((B * HW, 2 * Cc), dtype=f16, device=dev)
        gemm_nt(self.fl, xn, wqkv, bqkv, qk, B * HW, 2 * Cc, Cc, lda=Cc, ldw=Cc, ldo=2 * Cc)
        # V^T[b][c][j] WITHOUT its bias: the GEMM's bias is per column and here c is the row.  The rows of p sum to one, so the bias is added
        # to p.v instead (column c of that product) — equal up to the fp16 rounding of p (|sum p - 1| <= 1e-3, bias ~1e-2: 1e-5)
        vt = torch.empty((B, Cc, HW), dtype=f16, device=dev)
        gemm_nt(self.fl, wqkv[2 * Cc:], xn, None, vt, Cc, HW, Cc, lda=Cc, ldw=Cc, ldo=HW, batch=B, sA=0, sW=HW * Cc, sO=Cc * HW)
        s = torch.empty((B, HW, HW), dtype=torch.float32, device=dev)
        gemm_nt(self.fl, qk, qk[:, Cc:], None, s, HW, HW, Cc, lda=2 * Cc, ldw=2 * Cc, ldo=HW, batch=B, sA=HW * 2 * Cc, sW=HW * 2 * Cc, sO=HW * HW)
        p32 = torch.empty_like(s)
        hip.call('softmax_rows_f32', s, p32, B * HW, HW, float(np.float32(int(Cc) ** (-0.5))))
        p = self._to16(p32)
        o = torch.empty((B * HW, Cc), dtype=f16, device=dev)
        gemm_nt(self.fl, p, vt, bqkv[2 * Cc:], o, HW, Cc, HW, lda=HW, ldw=HW, ldo=Cc, batch=B, sA=HW * HW, sW=Cc * HW, sO=HW * Cc)
        y = torch.empty((B, Hh, Ww, Cc), dtype=f16, device=dev)
        gemm_nt(self.fl, o, self.w16[pre + '.proj_out.weight'], self.w[pre + '.proj_out.bias'], y, B * HW, Cc, Cc, lda=Cc, ldw=Cc, ldo=Cc,
                epi=EPI_RESID, resid=x, ldr=Cc)
        return y

    def upsample(self, h, key, B, Hh, Ww):
        """Upsample2x onto an Hh x Ww map, as DecoderEngine.upsample; one entry point with or without partials"""
        wp = self.w16[key + '.phase']
        up = torch.empty((B, Hh, Ww, wp.shape[1]), dtype=self.dt, device=h.device)
        part = self.eng._leave_partials(up, B, hip.conv_gn_blocks(Hh, Ww, wp.shape[1], phase=True))
        hip.call('upconv_phase_' + self.fl, h, wp, self.w[key + '.bias'], up, part, B, Hh, Ww, wp.shape[4], wp.shape[1])
        return up

    def downsample(self, h, key, B, Hh, Ww):
        """Downsample2x onto an Hh x Ww map (conv16s2.hip)"""
        wt = self.w16[key + '.weight']
        out = torch.empty((B, Hh, Ww, wt.shape[0]), dtype=self.dt, device=h.device)
        self.eng._leave_partials(out, B, 0)
        hip.call('conv3x3_s2_nhwc_' + self.fl, h, wt, self.w[key + '.bias'], out, B, Hh, Ww, wt.shape[3], wt.shape[0])
        return out

    def tail(self, h, key, B, Hh, Ww, denorm, clamp=True):
        """DecoderEngine.tail on a 16-bit map (varhip_gn_silu_conv_out_*); there is no unclamped form (decode_nhwc refuses it)"""
        wt = self.w16[key + '.conv_out.weight']
        Cout, Cin = wt.shape[0], wt.shape[3]
        mode = _tail_mode(denorm, True)
        if Hh % 8 == 0 and Ww % 32 == 0 and Cin % 32 == 0 and Cout <= 16 and (2 * 22 * 1024 + Cout * 9 * Cin * 2 + 16 + 8 * Cin) <= 64 * 1024 and not self.eng.unfused_tail:
            stats = self.gn_stats(h, B, Hh * Ww)
            out = torch.empty((B, Cout, Hh, Ww), dtype=torch.float32, device=h.device)
            hip.call('gn_silu_conv_out_' + self.fl, h, stats, self.w[key + '.norm_out.weight'], self.w[key + '.norm_out.bias'], wt,
                     self.w[key + '.conv_out.bias'], out, B, Hh, Ww, Cin, Cout, 32, mode)
            return out
        h = self.gn(h, key + '.norm_out', B, Hh * Ww, True)
        return self.conv3(h, key + '.conv_out', B, Hh, Ww, out_mode=mode)


# Winograd F(2x2,3x3) filter transform (Lavin & Gray 2016): U = G g G^T per (output, input) channel pair
_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def wino_filter(w: torch.Tensor) -> torch.Tensor:
    """[Cout][3][3][Cin] fp32 kernel -> U = G g G^T in float64, rounded once to fp32 and laid out [16][Cin/16][Cout][16] (xi = 4 i + j
    of the 4x4 transform, input-channel tile, output channel, input channel in the tile) for varhip_conv3x3_wino_nhwc_f32"""
    co, _, _, ci = w.shape
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    u = torch.einsum('ik,jl,oklc->ijoc', G, G, w.double()).float()                      # [4][4][Cout][Cin]
    return u.reshape(16, co, ci // 16, 16).permute(0, 2, 1, 3).contiguous()


class DecoderEngine(_VaeOps):
    """VQVAE.fhat_to_img on HIP kernels (reference vqvae.py:62-63, basic_vae.py:163-226)."""

    PREFIXES = ('decoder.', 'post_quant_conv.')
    LEVELS = 'decoder.up.'
    # default precision of the VQVAE's own entry points (fhat_to_img, idxBl_to_img, ...): 'f32' unless the VQVAE's owner asks for 'f16'
    # here.  The sampling loop does NOT change it: SamplingEngine passes its own precision with every decode_nhwc call, so two VARs
    # sharing one VQVAE, or a VAR in the 16-bit mode next to direct VQVAE calls, never fight over a mode flag.
    precision = 'f32'
    unfused_tail = False         # tests: run norm_out / conv_out of the decoder as two launches
    # The ResnetBlock convolutions (stride 1, 3x3) as fused Winograd F(2x2,3x3) where wino_ok() holds, and the Upsample2x convolutions as its
    # position-sparse form where the library's shape rule holds (winograd.hip); False (tests, A/B runs): every conv on the direct implicit-GEMM kernel.  VARHIP_WINOGRAD=0 sets the default for a whole process.
    winograd = os.environ.get('VARHIP_WINOGRAD', '1') != '0'
    WINO_MIN_HW = 16 * 16        # smallest map that takes it (1.63-1.72x faster than the direct kernel at every decoder level)
    # the precision flops_per_image_executed counts when not given one: that of the last decode_nhwc, or the one the owning SamplingEngine was
    # last set to (SamplingEngine.set_precision), whichever came later; None: `precision`.  Only an f32 decode runs the Winograd kernel.
    flops_precision = None

    def set_precision(self, precision: str):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}")
        self.precision = precision

    def _derive(self, w):
        for k in [k for k in w if k.endswith('.upsample.conv.weight')]:        # Upsample2x convs: pre-summed 2x2 phase weights
            cout, _, _, cin = w[k].shape
            wp = torch.empty(4, cout, 2, 2, cin, dtype=torch.float32, device=w[k].device)
            hip.call('upconv_pack_f32', w[k], wp, cin, cout)
            w[k[:-len('weight')] + 'phase'] = wp
        for k in [k for k in w if k.endswith(('.conv1.weight', '.conv2.weight'))]:   # ResnetBlock convs: Winograd filter transforms
            w[k[:-len('weight')] + 'wino'] = wino_filter(w[k])
        return w

    # -- the fp32 blocks only a decoder has ------------------------------------------------------------------------------------------
    def wino_ok(self, Hh, Ww, Cin, Cout):
        """the shape rule of the Winograd path: maps of at least WINO_MIN_HW pixels in whole 16 x 16 patches, channels in multiples of 32"""
        return Hh * Ww >= self.WINO_MIN_HW and Hh % 16 == 0 and Ww % 16 == 0 and Cin % 32 == 0 and Cout % 32 == 0

    def _wino(self, key, Hh, Ww, Cin, Cout):
        return self.w.get(key + '.wino') if self.winograd and self.wino_ok(Hh, Ww, Cin, Cout) else None

    def upsample(self, h, key, B, Hh, Ww):
        """Upsample2x onto an Hh x Ww map: nearest 2x + conv3x3, from the pre-summed phase weights on the low-res map.  With `winograd` on, the
        library runs the launch as position-sparse Winograd (9 multiplies per 2x2 output tile instead of the 16 of the four phase convs;
        DESIGN.md §13.2) where the output tiles into 16 x 16 patches and the channels are multiples of 32 — the same entry points, the same
        arguments.  Its result is normalised by the next level's first ResnetBlock: the partials where the shape has them"""
        wp = self.w[key + '.phase']
        up = torch.empty((B, Hh, Ww, wp.shape[1]), dtype=torch.float32, device=h.device)
        part = self._leave_partials(up, B, hip.conv_gn_blocks(Hh, Ww, wp.shape[1], phase=True))
        hip.upconv_winograd(self.winograd)
        try:
            if part is not None:
                hip.call('upconv_phase_gn_f32', h, wp, self.w[key + '.bias'], up, part, B, Hh, Ww, wp.shape[4], wp.shape[1])
            else:
                hip.call('upconv_phase_f32', h, wp, self.w[key + '.bias'], up, B, Hh, Ww, wp.shape[4], wp.shape[1])
        finally:
            hip.upconv_winograd(False)
        return up

    def tail(self, h, key, B, Hh, Ww, denorm, clamp=True):
        """norm_out -> swish -> conv_out -> clamp (-> (x + 1) / 2) (basic_vae.py:224-226, vqvae.py:63, var.py:190): one pass over the map
        (varhip_gn_silu_conv_out_f32) where it tiles into 8 x 32 patches, else GroupNorm apply + conv — the same bits either way.
        clamp=False: conv_out's value as it is (out_mode 3; vqvae.py:59, VQVAE.forward)"""
        wt = self.w[key + '.conv_out.weight']
        Cout, Cin = wt.shape[0], wt.shape[3]
        mode = _tail_mode(denorm, clamp)
        if Hh % 8 == 0 and Ww % 32 == 0 and Cin % 32 == 0 and Cout <= 4 and (10 * 34 * 36 + 4 * Cin) * 4 <= 64 * 1024 and not self.unfused_tail:
            stats = self.gn_stats(h, B, Hh * Ww)
            out = torch.empty((B, Cout, Hh, Ww), dtype=torch.float32, device=h.device)
            hip.call('gn_silu_conv_out_f32', h, stats, self.w[key + '.norm_out.weight'], self.w[key + '.norm_out.bias'], wt,
                     self.w[key + '.conv_out.bias'], out, B, Hh, Ww, Cin, Cout, 32, mode)
            return out
        h = self.gn(h, key + '.norm_out', B, Hh * Ww, True)
        return self.conv3(h, key + '.conv_out', B, Hh, Ww, out_mode=mode)

    # -- model arithmetic (for bench.py's roofline) ------------------------------------------------------------------------------------
    def _flops(self, P: int, prec: Optional[str]) -> float:
        """2 FLOPs per MAC summed over the decoder graph at a P x P f_hat.  prec None: every 3x3 conv at its 9 taps; else what a decode in
        `prec` executes (see flops_per_image_executed)"""
        self.refresh()
        w, f, hw, side = self.w, 0.0, P * P, P
        def c3(key, taps=9): co, _, _, ci = w[key + '.weight'].shape; return 2.0 * hw * co * taps * ci
        def c1(key): co, ci = w[key + '.weight'].shape; return 2.0 * hw * co * ci
        def res_taps(key): co, _, _, ci = w[key + '.weight'].shape; return 4 if prec == 'f32' and self.winograd and self.wino_ok(side, side, ci, co) else 9
        for kind, key in _decoder_graph(w, self.nlev):
            if kind == 'conv':
                f += c3(key)
            elif kind == 'res':
                f += c3(key + '.conv1', res_taps(key + '.conv1')) + c3(key + '.conv2', res_taps(key + '.conv2'))
                if (key + '.nin_shortcut.weight') in w: f += c1(key + '.nin_shortcut')
            elif kind == 'attn':
                f += c1(key + '.qkv') + c1(key + '.proj_out') + 2.0 * 2 * hw * hw * w[key + '.proj_out.weight'].shape[0]
            elif kind == 'up':
                hw *= 4; side *= 2
                f += c3(key, 9 if prec is None else 4)
            else:
                f += c3(key + '.conv_out')
        return f

    def flops_per_image_reference(self, P: int) -> float:
        """FLOPs (2/MAC) of one decode as the REFERENCE computes it (9-tap upsample convs; SURVEY.md §8d: 393.7 G at P=16, ch=160)"""
        return self._flops(P, None)

    def flops_per_image_executed(self, P: int, precision: Optional[str] = None) -> float:
        """FLOPs the kernels execute for one decode in `precision` (None: `flops_precision`): as flops_per_image_reference, with the Upsample2x
        convolutions in their folded four-phase form (4 taps per output pixel instead of 9) and, in an f32 decode, the ResnetBlock convolutions
        that take the Winograd path at 16 multiplies per 2x2 output tile (4 per output pixel instead of 9; the 16-bit decode has no such path).
        The Upsample2x convolutions are counted in the four-phase form in every precision, also where the f32 decode runs them at 9 multiplies
        per tile (tests/test_winograd_cpu.py pins this count)"""
        return self._flops(P, precision or self.flops_precision or self.precision)

    def decode_nhwc(self, f_hat: torch.Tensor, denorm: bool = True, precision: Optional[str] = None, clamp: bool = True) -> torch.Tensor:
        """[B,P,P,Cvae] channels-last -> [B,3,16P,16P]; denorm=True: in [0,1] (clamp and (x+1)/2 fused into the last conv, what
        autoregressive_infer_cfg returns); denorm=False: clamped to [-1,1] (VQVAE.fhat_to_img's contract); clamp=False: the decoder's
        output as it is (VQVAE.forward, vqvae.py:59; fp32 only, denorm is ignored).
        precision: 'f32' / 'f16' / 'bf16' for THIS call (None: the engine's default, `self.precision`)"""
        self.refresh()
        prec = precision or self.precision
        if not clamp and prec != 'f32':
            raise hip.VarHipError('decode_nhwc(clamp=False) is the fp32 decoder only')
        self.flops_precision = prec
        ops = self if prec == 'f32' else self.ops16(prec)
        self._wait_ready()
        B, P = f_hat.shape[0], f_hat.shape[1]
        h = f_hat if prec == 'f32' else ops._to16(f_hat.contiguous())
        return self._run(ops, _decoder_graph(self.w, self.nlev), h, B, P, P, denorm=denorm, clamp=clamp)


class QuantizerEngine(_Engine):
    """Encode-side methods of VectorQuantizer2 on HIP: f_to_idxBl_or_fhat (quant.py:135-166) and idxBl_to_var_input (quant.py:169-184)"""

    def __init__(self, quant):
        super().__init__()
        self.quant = quant

    def refresh(self):
        sig = _signature(self.quant.parameters())
        if sig == self._sig:
            return
        self.codebook, self.phi = _pack_quantizer(self.quant)
        self._taps = {}                      # {P: {pn: tap tables}}: the scales are the caller's, call by call
        self._sig = sig

    def tables(self, si, S, pn, P, dev):
        return _scale_tables(self._taps.setdefault(P, {}), self.phi, si, S, pn, P, dev)

    @torch.no_grad()
    def quantize(self, f_nhwc: torch.Tensor, to_fhat: bool, patch_nums, last_fhat: bool = False, stats: Optional[dict] = None):
        """residual quantisation scale by scale (quant.py:147-164): idx lists (B, pn^2) int64, or the cumulative f_hat's (NCHW).
        last_fhat=True (with to_fhat False): (idx lists, the last f_hat (B, Cvae, P, P)) from the one pass.
        stats (a dict, with to_fhat False): one varhip_vq_scale_stats_f32 launch behind every scale fills it with hits_SV (S, V) int64,
        mse_S (S,) fp32, sum_S (S,) fp64, bad (1,) int32 and f_hat_nhwc, the final channels-last f_hat (quant.py:77,95)"""
        self.refresh()
        B, P, _, Cv = f_nhwc.shape
        dev = f_nhwc.device
        f_rest = f_nhwc.clone()
        f_hat = torch.zeros_like(f_rest)
        up = torch.empty_like(f_rest)
        S, out = len(patch_nums), []
        if stats is not None:
            V = self.codebook.shape[0]
            stats.update(hits_SV=torch.zeros((S, V), dtype=torch.int64, device=dev), mse_S=torch.empty(S, dtype=torch.float32, device=dev),
                         sum_S=torch.empty(S, dtype=torch.float64, device=dev), bad=torch.zeros(1, dtype=torch.int32, device=dev), f_hat_nhwc=f_hat)
            scratch = torch.empty(hip.VQ_STATS_MAX_BLOCKS, dtype=torch.float64, device=dev)
        for si, pn in enumerate(patch_nums):
            if si != S - 1:
                z = torch.empty((B, pn * pn, Cv), dtype=torch.float32, device=dev)
                hip.call('area_pool_f32', f_rest, z, B, P, pn, Cv)
            else:
                z = f_rest
            idx = torch.empty(B * pn * pn, dtype=torch.int64, device=dev)
            # argmin |z - e|^2, or argmax cos(z, e) when using_znorm (quant.py:151-157)
            hip.call('nearest_code_cos_f32' if self.quant.using_znorm else 'nearest_code_f32', z, self.codebook, idx, B * pn * pn, self.codebook.shape[0], Cv)
            ti, tw, pw, pb, ratio = self.tables(si, S, pn, P, dev)
            hip.call('quant_residual_f32', idx, self.codebook, ti, tw, pw, pb, ratio, up, f_hat, f_rest, B, pn, P, Cv)
            if stats is not None:
                hip.call('vq_scale_stats_f32', f_hat, f_nhwc, f_hat.numel(), idx, B * pn * pn, V, stats['hits_SV'][si], scratch,
                         stats['sum_S'][si:], stats['mse_S'][si:], stats['bad'])
            out.append(f_hat.permute(0, 3, 1, 2).contiguous() if to_fhat else idx.view(B, pn * pn))
        if last_fhat and not to_fhat:
            return out, f_hat.permute(0, 3, 1, 2).contiguous()
        return out

    @torch.no_grad()
    def quantize_stats(self, f_nhwc: torch.Tensor, patch_nums, beta: float, nchw: bool = True) -> dict:
        """VectorQuantizer2.forward on HIP (quant.py:52-104): quantize() with its per-scale statistics, the loss combine (quant.py:95,97) and the
        straight-through value (quant.py:98).  -> dict(idx_Bl, hits_SV, mse_S, sum_S, bad, vq_loss (0-dim fp32), f_hat_raw (B, P, P, Cvae) the
        accumulated f_hat, f_hat_st_nhwc (f_hat - f) + f channels-last for the decoder, f_hat_st (B, Cvae, P, P) when nchw).  No host sync."""
        f_nhwc = f_nhwc.contiguous()
        st = {}
        st['idx_Bl'] = self.quantize(f_nhwc, False, patch_nums, stats=st)
        B, P, _, Cv = f_nhwc.shape
        loss = torch.empty(1, dtype=torch.float32, device=f_nhwc.device)
        hip.call('vq_loss_combine_f32', st['mse_S'], len(patch_nums), float(beta), loss)
        st['vq_loss'] = loss[0]
        st['f_hat_raw'] = st.pop('f_hat_nhwc')
        st['f_hat_st_nhwc'] = torch.empty_like(f_nhwc)
        st['f_hat_st'] = torch.empty((B, Cv, P, P), dtype=torch.float32, device=f_nhwc.device) if nchw else None
        hip.call('vq_straight_through_f32', st['f_hat_raw'], f_nhwc, st['f_hat_st_nhwc'], st['f_hat_st'], B, P * P, Cv)
        return st

    @torch.no_grad()
    def fhat_from_scales(self, items, patch_nums, from_tokens: bool, last_one: bool):
        """f_hat (B, Cvae, P, P) accumulated over all scales (quant.py:107-133 embed_to_fhat with all_to_max_scale=True; with
        from_tokens=True the codebook lookup of vqvae.py:77-84 idxBl_to_img is fused in).  items[si]: (B, pn*pn) token ids, or the
        embedding maps (B, Cvae, pn, pn).  Same kernels, same order of operations as the sampling loop's incremental f_hat."""
        self.refresh()
        B, P, Cv, S = items[0].shape[0], patch_nums[-1], self.codebook.shape[1], len(patch_nums)
        dev = self.codebook.device
        f_hat = torch.zeros((B, P, P, Cv), dtype=torch.float32, device=dev)
        up = torch.empty_like(f_hat)
        outs = []
        for si, pn in enumerate(patch_nums):
            ti, tw, pw, pb, ratio = self.tables(si, S, pn, P, dev)
            if from_tokens:
                hip.call('quant_accum_f32', items[si].to(dev, torch.int64).contiguous(), self.codebook, ti, tw, pw, pb, ratio, up, f_hat, B, pn, P, Cv)
            else:
                h = torch.empty((B, pn * pn, Cv), dtype=torch.float32, device=dev)
                hip.call('nchw_to_nhwc_f32', items[si].to(dev, torch.float32).contiguous(), h, B, Cv, pn * pn)
                hip.call('quant_accum_h_f32', h, ti, tw, pw, pb, ratio, up, f_hat, B, pn, P, Cv)
            if not last_one or si == S - 1:
                o = torch.empty((B, Cv, P, P), dtype=torch.float32, device=dev)
                hip.call('nhwc_to_nchw_f32', f_hat, o, B, Cv, P * P)
                outs.append(o)
        return outs[-1] if last_one else outs

    @torch.no_grad()
    def var_input(self, idx_list, patch_nums) -> torch.Tensor:
        """teacher-forcing input (B, L - first_l, Cvae) of VAR.forward from ground-truth token maps (quant.py:169-184)"""
        self.refresh()
        B, P, Cv, S = idx_list[0].shape[0], patch_nums[-1], self.codebook.shape[1], len(patch_nums)
        dev = idx_list[0].device
        f_hat = torch.zeros((B, P, P, Cv), dtype=torch.float32, device=dev)
        up = torch.empty_like(f_hat)
        L = sum(p * p for p in patch_nums)
        out = torch.empty((B, L - patch_nums[0] ** 2, Cv), dtype=torch.float32, device=dev)
        cur = 0
        for si in range(S - 1):
            pn, pq = patch_nums[si], patch_nums[si + 1]
            ti, tw, pw, pb, ratio = self.tables(si, S, pn, P, dev)
            hip.call('quant_accum_f32', idx_list[si].to(torch.int64).contiguous(), self.codebook, ti, tw, pw, pb, ratio, up, f_hat, B, pn, P, Cv)
            pooled = torch.empty((B, pq * pq, Cv), dtype=torch.float32, device=dev)
            hip.call('area_pool_f32', f_hat, pooled, B, P, pq, Cv)
            out[:, cur:cur + pq * pq] = pooled
            cur += pq * pq
        return out



class EncoderEngine(_VaeOps):
    """Encoder + quant_conv on HIP (reference vqvae.py:65-75 img_to_*: basic_vae.py:99-160)."""

    PREFIXES = ('encoder.', 'quant_conv.')
    LEVELS = 'encoder.down.'
    precision = 'f32'            # what encode() runs in when not told: there is no mode to set, a 16-bit encode is asked for per call
    last_precision = None        # the precision the last encode() ran in ('f32' | 'f16' | 'bf16')

    def downsample(self, x, key, B, Hh, Ww):
        """Downsample2x onto an Hh x Ww map: the stride-2 conv over the map padded right and below (basic_vae.py:41-42)"""
        wt = self.w[key + '.weight']
        Cout, Cin = wt.shape[0], wt.shape[3]
        out = torch.empty((B, Hh, Ww, Cout), dtype=torch.float32, device=x.device)
        hip.call('conv3x3_s2_nhwc_f32', x, wt, self.w[key + '.bias'], out, B, Hh, Ww, Cin, Cout)
        return out

    @torch.no_grad()
    def encode(self, img: torch.Tensor, precision: Optional[str] = None) -> torch.Tensor:
        """img (B,3,H,W) fp32 in [-1,1] -> f (B, H/16, W/16, Cvae) fp32 channels-last == quant_conv(encoder(img)).
        precision: None or 'f32' — the fp32 encoder; 'f16' / 'bf16' — for THIS call the encoder on 16-bit activations and conv weights with
        fp32 accumulation: the image is rounded to 16 bits once, after its channels are zero-padded to conv_in's 32.  quant_conv runs in fp32
        on the cast conv_out map either way, so f (what the quantizer and the feature distance read) is fp32."""
        if precision not in (None,) + PRECISIONS:
            raise ValueError(f"precision must be None or one of {PRECISIONS}")
        self.refresh()
        prec = self.last_precision = precision or self.precision
        ops = self if prec == 'f32' else self.ops16(prec)
        self._wait_ready()
        B, Ci, Hh, Ww = img.shape
        cin_pad = self.w['encoder.conv_in.weight'].shape[3]
        x = torch.empty((B, Hh, Ww, cin_pad), dtype=torch.float32, device=img.device)
        hip.call('nchw_to_nhwc_pad_f32', img.contiguous(), x, B, Ci, Hh * Ww, cin_pad)
        h = self._run(ops, _encoder_graph(self.w, self.nlev), x if prec == 'f32' else ops._to16(x), B, Hh, Ww)
        return self.conv3(h if prec == 'f32' else ops._to32(h), 'quant_conv', B, h.shape[1], h.shape[2])


AUTOCAST_PRECISION = {torch.float16: 'f16', torch.bfloat16: 'bf16'}


_SCORE_MODES = {'group_smoothed': 1, 'neighbor_max': 2, 'expected_distance': 3}     # score -> mode of varhip_token_score_f32 ('log_prob' has its own kernel)
_DIST_SCORES = ('neighbor_max', 'expected_distance')                                # the scores that read the code distance table


class _Exp1:
    """One stream of Exp(1) fills [B * l, V] fp32, the one place where the sampling loop gets its noise.  src None: every fill is drawn with
    `exponential_(generator=rng)` exactly as torch.multinomial (helpers.py:19) would; a callable (si, l) -> tensor (the Philox fill of
    sample_per_image; var_amd.multi hands each rank its rows; tests inject the CPU generator's stream); a list: one tensor per draw, indexed by
    the draw count, so a scale that draws nothing (fully kept under inpainting) takes no entry."""

    def __init__(self, src, rng: Optional[torch.Generator], V: int, dev):
        self.src, self.rng, self.V, self.dev, self.draws = src, rng, V, dev, 0

    def draw(self, B: int, si: int, l: int, use: bool = True) -> Optional[torch.Tensor]:
        """scale si's fill.  use=False: the draw is spent and not read — the generator advances, a list skips its entry, a callable is not called"""
        if self.src is None:
            return torch.empty(B * l, self.V, dtype=torch.float32, device=self.dev).exponential_(1, generator=self.rng)
        k, self.draws = self.draws, self.draws + 1
        if not use:
            return None
        return (self.src(si, l) if callable(self.src) else self.src[k]).to(self.dev, torch.float32).contiguous()


class SamplingEngine(_Engine):
    """The AR loop of VAR.autoregressive_infer_cfg on HIP kernels.  One engine per VAR module; calls on different HIP streams may be in flight
    together (per-stream workspaces), the host side is not thread-safe."""

    MAX_WORKSPACES = 6          # buffer sets kept alive per engine (workspace(): one per (batch size, stream, precision) in use)
    # all blocks' ada_lin weights are packed into one GEMM operand up to this many bytes; beyond it (the weight rows would leave the GEMM's 32-bit
    # request offsets) every block projects its own
    ADA_PACKED_MAX_BYTES = 3.5e9

    def __init__(self, var):
        super().__init__()
        self.var = var
        self._ws: Dict[tuple, dict] = {}            # (batch size, HIP stream, precision) -> buffers of a call; (..., G): of a pass of sample_composed
        self._ws_tf: Dict[tuple, dict] = {}         # the same for teacher_forced_logits
        self._ws_bop: Dict[tuple, dict] = {}        # (capacity, HIP stream, precision, stage) -> buffers of a stage of sample_best_of_pruned
        self._labels_ok = None                      # (the last label tensor whose range was checked, its version counter, address, length): one host sync saved per repeated call

        self.policy = 'auto' if os.environ.get('VARHIP_FOLLOW_AUTOCAST', '0') not in ('', '0') else 'f32'      # what set_precision() was given: 'f32' | 'f16' | 'bf16' | 'auto' (follow the caller's torch.autocast)
        self.precision = 'f32'              # the arithmetic of the call in progress (the policy, resolved): 'f16' / 'bf16' = the 16-bit throughput mode (include/var_hip.h)
        self.dec = var.vae_proxy[0]._decoder_engine()       # the VQVAE's own engine: one packed copy of the decoder weights, one place to invalidate
        self.last_trace: Optional[dict] = None

    # -- weights -----------------------------------------------------------------------------------------------------
    def refresh(self):
        var = self.var
        quant = var.vae_quant_proxy[0]
        sig = _signature(list(var.parameters()) + list(quant.parameters()), (getattr(var.vae_proxy[0], '_hip_generation', 0),))
        if sig == self._sig:
            self._ensure16()
            return
        if var.C != 64 * var.num_heads:
            raise hip.VarHipError(f'the HIP attention kernels are built for head_dim 64, got embed_dim {var.C} / {var.num_heads} heads')
        self._retire()
        dev = var.pos_start.device
        w = {}
        g = lambda t, n: _chk(t.detach(), n)
        C = var.C
        w['class_emb'] = g(var.class_emb.weight, 'class_emb')
        w['pos_start'] = g(var.pos_start, 'pos_start').view(var.first_l, C)
        w['pos_1LC'] = g(var.pos_1LC, 'pos_1LC').view(var.L, C)
        w['lvl_embed'] = g(var.lvl_embed.weight, 'lvl_embed')
        w['lvl_1L'] = var.lvl_1L.view(-1).to(torch.int64).contiguous()
        w['word_w'], w['word_b'] = g(var.word_embed.weight, 'word_embed.weight'), g(var.word_embed.bias, 'word_embed.bias')
        w['head_w'], w['head_b'] = g(var.head.weight, 'head.weight'), g(var.head.bias, 'head.bias')
        w['hn_w'], w['hn_b'] = g(var.head_nm.ada_lin[1].weight, 'head_nm'), g(var.head_nm.ada_lin[1].bias, 'head_nm')
        if var.shared_aln:
            w['sal_w'], w['sal_b'] = g(var.shared_ada_lin[1].weight, 'shared_ada_lin'), g(var.shared_ada_lin[1].bias, 'shared_ada_lin')
        blocks = []
        for b in var.blocks:
            a = b.attn
            d = dict(
                qkv_w=g(a.mat_qkv.weight, 'mat_qkv'), qkv_b=torch.cat((a.q_bias.detach(), a.zero_k_bias, a.v_bias.detach())).float().contiguous(),
                proj_w=g(a.proj.weight, 'proj'), proj_b=g(a.proj.bias, 'proj'),
                fc1_w=g(b.ffn.fc1.weight, 'fc1'), fc1_b=g(b.ffn.fc1.bias, 'fc1'), fc2_w=g(b.ffn.fc2.weight, 'fc2'), fc2_b=g(b.ffn.fc2.bias, 'fc2'),
                smul=g(a.scale_mul_1H11, 'scale_mul').view(-1) if a.attn_l2_norm else None, l2=bool(a.attn_l2_norm), plain_scale=float(a.scale))
            if var.shared_aln:
                d['gss'] = g(b.ada_gss, 'ada_gss').view(-1)
            blocks.append(d)
        w['blocks'] = blocks
        w['b16'], w['head_w16'] = {}, {}     # {'f16' | 'bf16': ...} 16-bit copies of the GEMM weights, made by _ensure16() when such a call first needs them
        if not var.shared_aln and var.depth * 6 * C * C * 4 < self.ADA_PACKED_MAX_BYTES:
            # all blocks' ada_lin projections as ONE GEMM per call (N = depth * 6C): sixteen launches of 192 workgroups each were bound by one
            # workgroup's K loop (29 us each at d16).  The packed copy (0.4 GB fp32 at d16, 2.65 GB at d30; rebuilt when weights change) is the only
            # copy the engine holds: the per-block path is not used beside it
            w['ada_w_all'] = torch.cat([g(b.ada_lin[1].weight, 'ada_lin') for b in var.blocks], dim=0)
            w['ada_b_all'] = torch.cat([g(b.ada_lin[1].bias, 'ada_lin') for b in var.blocks], dim=0)
        elif not var.shared_aln:
            for d, b in zip(blocks, var.blocks):
                d['ada_w'], d['ada_b'] = g(b.ada_lin[1].weight, 'ada_lin'), g(b.ada_lin[1].bias, 'ada_lin')
        w['codebook'], w['phi'] = _pack_quantizer(quant)
        w['codebook_T'] = w['codebook'].t().contiguous()          # [Cvae][V]: "probabilities @ codebook" as an NT GEMM (more_smooth)
        w['taps'] = {}                                            # {pn: tap tables} of every scale, uploaded here: behind the event of _built()
        for pn in var.patch_nums:
            _tap_tables(w['taps'], pn, var.patch_nums[-1], dev)
        self.w = w
        self._sig = sig
        self._labels_ok = None
        self._built()
        self._ensure16()

    def _ensure16(self):
        """16-bit copies of the four GEMM weights of every block and of the head (round-to-nearest-even, once per weight change and flavour), kept
        per flavour so that calls alternating between precisions ('auto' inside and outside an autocast region) convert nothing twice"""
        prec = self.precision
        if prec == 'f32' or prec in self.w['b16']:
            return
        self._wait_ready()
        dt = DT16[prec]
        self.w['b16'][prec] = [{k: d[k].to(dt).contiguous() for k in ('qkv_w', 'proj_w', 'fc1_w', 'fc2_w')} for d in self.w['blocks']]
        self.w['head_w16'][prec] = self.w['head_w'].to(dt).contiguous()
        self._built()

    def resolve_precision(self) -> str:
        """the arithmetic of the call that starts now: the policy itself, or under 'auto' what the caller's torch.autocast('cuda', dtype=...) asks for
        (reference basic_var.py:97 branches on the dtype autocast hands it; demo_sample.py:66-68 is the caller)"""
        if self.policy == 'auto':
            self.precision = AUTOCAST_PRECISION.get(torch.get_autocast_dtype('cuda'), 'f32') if torch.is_autocast_enabled('cuda') else 'f32'
        else:
            self.precision = self.policy
        return self.precision

    def set_precision(self, precision: str):
        """'f32' (default; the parity contract: token ids bit-identical to the CPU oracle), 'f16' or 'bf16': 16-bit weights / GEMM operands / KV
        cache with fp32 accumulation on the f16 MFMAs — what the reference's harness asks for with torch.autocast(fp16)
        (demo_sample.py:66-68), and the decoder call that ends the loop runs on fp16 activations / conv weights too (conv16.hip).  LayerNorm /
        GroupNorm statistics, AdaLN parameters, the residual stream, softmax, logits, sampler and quantizer stay fp32.  The VQVAE's own entry
        points (fhat_to_img, idxBl_to_img, ...) are NOT switched: the shared DecoderEngine is told the precision per call."""
        if precision not in PRECISIONS + ('auto',):
            raise ValueError(f"precision must be one of {PRECISIONS + ('auto',)}")
        self.policy = precision
        if precision != 'auto':
            self.dec.flops_precision = precision                    # what the decoder's FLOP count describes from now on (bench.py prices each mode)
        if precision != 'auto' and precision != self.precision:
            self.precision = precision
            for cache in ('_ws', '_ws_tf', '_ws_bop'):                                   # an explicit switch releases the other modes' buffers (6-11 GB each at d16 / B=64)
                keep_precision(getattr(self, cache, {}), precision)

    def invalidate(self):
        """forget the packed weight copies of the sampling loop and of the decoder (call after editing parameters through `.data`)"""
        super().invalidate()
        self.dec.invalidate()

    # -- workspaces --------------------------------------------------------------------------------------------------
    def _dims(self) -> Dims:
        var = self.var
        return Dims(C=var.C, H=var.num_heads, V=var.V, Cvae=var.Cvae, P=var.patch_nums[-1], depth=var.depth, hidden=var.blocks[0].ffn.fc1.weight.shape[0],
                    shared_aln=bool(var.shared_aln), L=var.L)

    def _workspace(self, cache: dict, bound: int, size: int, slot: tuple, R: int, lmax: Optional[int] = None, Lkv: Optional[int] = None, **on_top) -> dict:
        """the buffer set cache[(size, HIP stream, precision, *slot)] in the call's precision: R transformer rows of up to lmax tokens a scale
        (default: the widest scale) over caches of Lkv tokens (default: all L), plus what `on_top` names (workspace.workspace_spec), held by
        the one cache rule (workspace.cached)"""
        var = self.var
        dev = var.pos_start.device
        lmax = max(p * p for p in var.patch_nums) if lmax is None else lmax
        spec = lambda: workspace_spec(self._dims(), DT16.get(self.precision, torch.float32), R, lmax, var.L if Lkv is None else Lkv, **on_top)
        return cached(cache, size, (int(torch.cuda.current_stream().cuda_stream), self.precision) + slot, bound, dev, lambda: allocate(spec(), dev))

    def workspace(self, B: int) -> dict:
        """buffers of one call of B images, the 2B rows of its CFG pairs (residual stream, GEMM operands, KV caches ...), cached per (batch size,
        HIP stream, precision): calls issued on DIFFERENT streams may be in flight together — each owns its buffers, everything else a call
        allocates comes from torch's stream-ordered allocator — and a call's latency-bound small scales then run beside another call's decoder"""
        return self._workspace(self._ws, self.MAX_WORKSPACES, B, (), 2 * B, B=B)

    def _mix_workspace(self, B: int, G: int) -> dict:
        """the buffer set of a pass of sample_composed: B images of G row groups.  It lives in the plain calls' cache under a key of its own,
        (B, HIP stream, precision, G) — one B resident per (stream, precision, G), the same bound on the number of sets, the same poisoning in
        the tests — and adds what the composed sampler writes, `masked` and `mixed`.  The prologue gets the G * B labels themselves (twin)"""
        return self._workspace(self._ws, self.MAX_WORKSPACES, B, (G,), G * B, B=B, twin=True, masked=True, mixed=True)

    def _bop_workspace(self, cap: int, stage: int) -> dict:
        """the buffer set of stage `stage` of sample_best_of_pruned, for up to `cap` candidates (a chunk of fewer uses a prefix of every buffer:
        all of them are row-major in the candidate).  A cache of its own, keyed (capacity, HIP stream, precision, stage): one capacity resident per
        (stream, precision, stage), so the stages evict neither one another nor the plain calls' workspace, and a repeated call allocates nothing."""
        return self._workspace(self._ws_bop, 4 * len(self.var.patch_nums), cap, (stage,), 2 * cap, B=cap, masked=True)

    def _check_labels(self, label_B: torch.Tensor):
        """labels index class_emb: out-of-range ones must not reach the kernel.  One device-side reduction and ONE host sync (a sync drains the
        stream, so back-to-back calls would otherwise never overlap their host side with the previous call's kernels); the tensor OBJECT that was
        checked last is not checked again while its version counter stands.  The engine keeps a reference to that object, so its storage cannot
        go back to the allocator and come out again under another tensor: an address alone proves nothing (a fresh tensor in a recycled block
        has the same address, the same length and version 0).  Tensors made under torch.inference_mode() have no counter and are checked every
        time.  What stays the caller's business: writes to that same object that bump no counter — through `.data`, or through memory the tensor
        only wraps (a numpy array under torch.from_numpy, DLPack, another view of its storage made with `.data`)."""
        ver = _ver(label_B)
        ok = self._labels_ok
        if ok is not None and ok[0] is label_B and ver >= 0 and ok[1:] == (ver, label_B.data_ptr(), label_B.numel()):
            return
        self._labels_ok = None
        lo, hi = torch.aminmax(label_B)
        lo, hi = torch.stack((lo, hi)).tolist()
        if lo < 0 or hi > self.var.num_classes:
            raise ValueError(f'labels must lie in [0, {self.var.num_classes}]')
        self._labels_ok = (label_B, ver, label_B.data_ptr(), label_B.numel())

    def gemm(self, A, W, bias, out, M, epi=EPI_NONE, resid=None, gamma=None, ldg=0, rpg=1):
        N, K = W.shape
        gemm_nt('f32', A, W, bias, out, M, N, K, lda=K, ldw=K, ldo=N, epi=epi, resid=resid, ldr=N, gamma=gamma, ldg=ldg, rpg=rpg)

    def neighbor_table(self, n: int):
        """(idx int32 [V, n], dist float32 [V, n]) nearest codes of every code (var.py:459-462); cached until the codebook changes."""
        self.refresh()
        tabs = self.w.setdefault('nbr', {})
        if n not in tabs:
            cb = self.w['codebook']
            V, D = cb.shape
            idx = torch.empty(V, n, dtype=torch.int32, device=cb.device)
            dist = torch.empty(V, n, dtype=torch.float32, device=cb.device)
            self._wait_ready()
            hip.call('neighbor_table_f32', cb, V, D, n, idx, dist)
            tabs.clear()                                        # one n resident at a time
            tabs[n] = (idx, dist)
            self._built()
        return tabs[n]

    def block(self, blk, ws, bi, x, x2, rows, l, cur, Lmax: Optional[int] = None):
        """one AdaLNSelfAttn block (basic_var.py:152-159): seven launches behind one library call; the result is left in x.  Lmax: the token
        length of the KV caches in ws (default var.L)"""
        var = self.var
        C = var.C
        Lmax = var.L if Lmax is None else Lmax
        prec = self.precision
        gw = blk if prec == 'f32' else self.w['b16'][prec][bi]          # the four GEMM weights in the call's arithmetic; everything else is fp32
        hip.call('adaln_block_' + prec, x, x2, ws['xn'], ws['q'], ws['att'], ws['hid'], ws['ada_view'][bi][0], ws['ada_view'][bi][1],
                 gw['qkv_w'], blk['qkv_b'], blk['smul'], blk['plain_scale'], int(blk['l2']), gw['proj_w'], blk['proj_b'],
                 gw['fc1_w'], blk['fc1_b'], gw['fc2_w'], blk['fc2_b'], ws['kc'][bi], ws['vc'][bi],
                 rows, l, C, var.num_heads, blk['fc1_w'].shape[0], cur, Lmax, var.norm_eps)

    def block_patched(self, blk, ws, bi, x, x2, rows, l, cur, Lmax: int, dir_att, n_att: int, dir_hid, n_hid: int):
        """block() in f32 with interventions (varhip_adaln_block_patched_f32): dir_att / dir_hid, device tables of n_att / n_hid directives
        (row, c0, c1, src) on the attention output in front of proj and on the MLP hidden activation behind the GELU"""
        var = self.var
        hip.call('adaln_block_patched_f32', x, x2, ws['xn'], ws['q'], ws['att'], ws['hid'], ws['ada_view'][bi][0], ws['ada_view'][bi][1],
                 blk['qkv_w'], blk['qkv_b'], blk['smul'], blk['plain_scale'], int(blk['l2']), blk['proj_w'], blk['proj_b'],
                 blk['fc1_w'], blk['fc1_b'], blk['fc2_w'], blk['fc2_b'], ws['kc'][bi], ws['vc'][bi],
                 rows, l, var.C, var.num_heads, blk['fc1_w'].shape[0], cur, Lmax, var.norm_eps, dir_att, n_att, dir_hid, n_hid)

    def block_keysel(self, blk, ws, bi, x, x2, rows, l, cur, Lmax: int, ends, S1: int, keymask):
        """block() in f32 with edges of the block-causal graph cut (varhip_adaln_block_keysel_f32): ends, a host int32 array of the S1 key
        scales' ends (the last one cur + l), keymask, a device int32 table [rows * H] whose bit i says that the row's head sees key scale i"""
        var = self.var
        hip.call('adaln_block_keysel_f32', x, x2, ws['xn'], ws['q'], ws['att'], ws['hid'], ws['ada_view'][bi][0], ws['ada_view'][bi][1],
                 blk['qkv_w'], blk['qkv_b'], blk['smul'], blk['plain_scale'], int(blk['l2']), blk['proj_w'], blk['proj_b'],
                 blk['fc1_w'], blk['fc1_b'], blk['fc2_w'], blk['fc2_b'], ws['kc'][bi], ws['vc'][bi],
                 rows, l, var.C, var.num_heads, blk['fc1_w'].shape[0], cur, Lmax, var.norm_eps, ends, S1, keymask)

    def head(self, x, hn, xn, logits, M, l):
        """get_logits (var.py:118-124): AdaLNBeforeHead (LayerNorm + scale/shift) then the vocabulary projection -> fp32 logits"""
        var, w = self.var, self.w
        C, V = var.C, var.V
        prec = self.precision
        hip.call('ln_modulate_f32' if prec == 'f32' else f'ln_modulate_{prec}out', x, hn, 2 * C, hn[:, C:], 2 * C, xn, M, C, l, var.norm_eps)
        if prec == 'f32':
            self.gemm(xn, w['head_w'], w['head_b'], logits, M)
        else:
            gemm_nt(prec, xn, w['head_w16'][prec], w['head_b'], logits, M, V, C, lda=C, ldw=C, ldo=V)

    def _prologue(self, ws, labels, rows):
        """what a pass computes once, before its scales (var.py:151-157): the level + position embedding, the first map and the condition of
        every label (first_map_f32 also writes each label's unconditional twin), and from SiLU(condition) the AdaLN parameters of every
        block and of the head, for `rows` rows (sampling: the 2B rows of the CFG pairs; teacher forcing: the labels' own R).  Leaves
        ws['ada_view'][block] = (that block's 6C parameters per row, their row stride)"""
        var, w = self.var, self.w
        C, D6 = var.C, var.depth * 6 * var.C
        hip.call('lvl_pos_f32', w['lvl_embed'], w['lvl_1L'], w['pos_1LC'], ws['lvl_pos'], var.L, C)
        hip.call('first_map_f32', w['class_emb'], labels, var.num_classes, w['pos_start'], ws['lvl_pos'], ws['cond'], ws['x'], labels.numel(), C, var.first_l)
        hip.call('silu_f32', ws['cond'], ws['cond_silu'], rows * C)
        if var.shared_aln:
            self.gemm(ws['cond_silu'], w['sal_w'], w['sal_b'], ws['shared'], rows)
            for bi, blk in enumerate(w['blocks']):
                hip.call('add_bcast_f32', blk['gss'], ws['shared'], ws['ada'][bi], rows, 6 * C)
            ws['ada_view'] = [(ws['ada'][bi], 6 * C) for bi in range(var.depth)]
        else:
            ws['ada_view'] = [(ws['ada'][:, bi * 6 * C:], D6) for bi in range(var.depth)]          # row b: [block 0: 6C | block 1: 6C | ...]
            if 'ada_w_all' in w:
                self.gemm(ws['cond_silu'], w['ada_w_all'], w['ada_b_all'], ws['ada'], rows)
            else:
                for (view, _), blk in zip(ws['ada_view'], w['blocks']):
                    gemm_nt('f32', ws['cond_silu'], blk['ada_w'], blk['ada_b'], view, rows, 6 * C, C, lda=C, ldw=C, ldo=D6)
        self.gemm(ws['cond_silu'], w['hn_w'], w['hn_b'], ws['hn'], rows)

    def qkv(self, xn, blk, ws, bi, rows, l, cur):
        """mat_qkv + q/k normalisation + KV-cache append in one launch (basic_var.py:93-109)."""
        C, H = self.var.C, self.var.num_heads
        hip.call('gemm_qkv_f32', xn, C, blk['qkv_w'], C, blk['qkv_b'], rows * l, C, C, blk['smul'], blk['plain_scale'], int(blk['l2']),
                 ws['q'], ws['kc'][bi], ws['vc'][bi], rows, l, H, cur, self.var.L)

    # -- the sampling walk -------------------------------------------------------------------------------------------
    def _scales(self, ws: dict, B: int, first: int, last: int, tr: Optional[dict] = None, ev: Optional[list] = None, G: int = 2):
        """the sampling loop over scales first .. last for the B images whose state sits in the first rows of ws (its prologue run, ws['x'] holding
        scale `first`'s input, the caches the scales below it).  Per scale: the blocks; the scale is yielded (si, pn, l = pn * pn, cur = its first
        token, r = the stage ratio) and the caller's loop body sets .idx, the int64 [B * l] tokens it chose, and where they apply .soft and .ed;
        then the quantizer step (_quant_step) and, between the walk's own scales, next_map_f32.  Ends behind the quantizer step of `last`: what
        follows is the caller's (a prune or resampling boundary, the decoder).  tr: sample()'s trace; ev: its profile_scales events.
        G: the row groups of ws (sample_composed: K + 1), group-major, each of B rows; every group gets the same next-scale input: next_map_f32
        writes a pair of groups per launch, so it runs once per pair (an odd G: the last launch writes group G - 2 a second time, with the
        same bits), and the groups hold identical bits because one kernel computed them from one f_hat."""
        var, w = self.var, self.w
        C, Cv, P = var.C, var.Cvae, var.patch_nums[-1]
        x, x2 = ws['x'], ws['x2']
        for si in range(first, last + 1):                                 # var.py:160
            pn = var.patch_nums[si]
            r = si / var.num_stages_minus_1 if var.num_stages_minus_1 > 0 else 0.0                  # the stage ratio (var.py:166)
            sc = SimpleNamespace(si=si, pn=pn, l=pn * pn, cur=var.begin_ends[si][0], r=r, idx=None, soft=None, ed=None)
            if ev: ev[si].record()
            for bi, blk in enumerate(w['blocks']):                        # AdaLNSelfAttn.forward, basic_var.py:152-159
                self.block(blk, ws, bi, x, x2, G * B, sc.l, sc.cur)
            yield sc
            self._quant_step(ws, B, sc)
            if tr is not None: tr['f_hat'].append(ws['f_hat'].permute(0, 3, 1, 2).clone())
            if si != last:
                pq = var.patch_nums[si + 1]
                for g0 in list(range(0, G - 1, 2)) + ([G - 2] if G % 2 else []):          # groups (g0, g0 + 1); G = 2: one launch on x itself
                    hip.call('next_map_f32', ws['f_hat'], w['word_w'], w['word_b'], ws['lvl_pos'][sc.cur + sc.l:], x[g0 * B * pq * pq:] if g0 else x,
                             ws['pooled'], B, P, pq, C, Cv)
                if tr is not None: tr['pooled'].append(ws['pooled'][:B * pq * pq].view(B, pq, pq, Cv).permute(0, 3, 1, 2).clone())

    def _quant_step(self, ws: dict, B: int, sc):
        """the quantizer step of a scale (var.py:177-183): f_hat += phi(upsample(h)), h = codebook[sc.idx].  sc.soft, an Exp(1) fill [B * l, V]
        (more_smooth): h = gumbel_softmax(filtered logits * (1 + ratio), tau) @ codebook instead, from the logits the sampler left in
        ws['masked'] (var.py:178-180).  sc.ed = (tokens, keep, ...) [B, L] of an edit: kept positions take codebook[token] (replace_embedding)."""
        var, w = self.var, self.w
        V, Cv, P = var.V, var.Cvae, var.patch_nums[-1]
        l, cur = sc.l, sc.cur
        tail = (*_scale_tables(w['taps'], w['phi'], sc.si, len(var.patch_nums), sc.pn, P, ws['dev']), ws['up'], ws['f_hat'], B, sc.pn, P, Cv)
        kept = () if sc.ed is None else (sc.ed[1][:, cur:], sc.ed[0][:, cur:], var.L, w['codebook'])
        if sc.soft is not None:
            hip.call('gumbel_softmax_f32', ws['masked'], sc.soft, ws['probs'], B * l, V, float(1 + sc.r), float(max(0.27 * (1 - sc.r * 0.95), 0.005)))
            self.gemm(ws['probs'], w['codebook_T'], None, ws['h'], B * l)
            hip.call('quant_accum_h_edit_f32' if kept else 'quant_accum_h_f32', ws['h'], *kept, *tail)
        elif kept:                                                        # codebook[keep ? token : sampled]
            hip.call('quant_accum_edit_f32', sc.idx, *kept, *tail)
        else:
            hip.call('quant_accum_f32', sc.idx, w['codebook'], *tail)

    # -- the choosers: each leaves a scale's tokens, int64 [B * l] -------------------------------------------------------------------
    def _logits(self, ws: dict, B: int, sc, tr: Optional[dict], G: int = 2):
        """get_logits (var.py:118-124): AdaLNBeforeHead + head over the scale's G * B * l rows (G = 2: the CFG pair), into ws['logits']"""
        self.head(ws['x'], ws['hn'], ws['xn'], ws['logits'], G * B * sc.l, sc.l)
        if tr is not None: tr['logits'].append(ws['logits'][:2 * B * sc.l].view(2 * B, sc.l, self.var.V).clone())

    def _sampled(self, ws: dict, B: int, sc, noise: '_Exp1', masked: Optional[torch.Tensor], t: float = 0.0, top_k: int = 0, top_p: float = 0.0,
                 per: Optional[dict] = None, stats: Optional[dict] = None, tr: Optional[dict] = None) -> torch.Tensor:
        """CFG + top-k/top-p + multinomial (var.py:172-175) with one fill of `noise`.  per = dict(t=[S, B] float64, top_k=[B] int32, top_p=[B] float64
        on the device, cap=int): every image samples with its own parameters (varhip_cfg_sample_rows_f32), and t, top_k and top_p are not read.
        A per that holds 'tau' is _controlled_upload's: top_k, top_p, tau, min_p, bias_row [S, B] and cap [S] indexed by the scale, bias [R, V] or
        None (varhip_ctl_sample_rows_f32).  masked: None, or [>= B * l, V] fp32 that receives the filtered logits.  stats: the (B, L) tensors of STATS_FIELDS; varhip_sample_stats_f32
        runs behind the sampler into this scale's slice of them (the drawn tokens' log-probabilities, kept counts and entropies)."""
        var = self.var
        l, cur, V = sc.l, sc.cur, var.V
        self._logits(ws, B, sc, tr)
        idx = ws['idx'][:B * l]
        fill = noise.draw(B, sc.si, l)
        if per is not None and 'tau' in per:                              # sample_controlled: every table is indexed by the scale
            si, bias = sc.si, per['bias']
            hip.call('ctl_sample_rows_f32', ws['logits'], fill, idx, masked, B, l, V, per['t'][si], per['top_k'][si], per['top_p'][si], per['tau'][si],
                     per['min_p'][si], bias, per['bias_row'][si] if bias is not None else None, 0 if bias is None else bias.shape[0], V,
                     int(per['cap'][si]))
        elif per is not None:
            hip.call('cfg_sample_rows_f32', ws['logits'], fill, idx, masked, B, l, V, per['t'][sc.si], per['top_k'], per['top_p'], int(per['cap']))
        else:
            hip.call('cfg_sample_f32', ws['logits'], fill, idx, masked, B, l, V, float(t), int(top_k), float(top_p))
        if stats is not None:
            hip.call('sample_stats_f32', ws['logits'], masked, idx, B, l, V, float(t), per['t'][sc.si] if per is not None else None,
                     *[stats[key][:, cur:] for key in STATS_FIELDS], var.L)
            if tr is not None: tr.setdefault('masked', []).append(masked[:B * l].clone())
        return idx

    def _greedy(self, ws: dict, B: int, sc, t: float, inp: Optional[tuple], tr: Optional[dict]) -> torch.Tensor:
        """CFG + argmax: the lowest index of the CFG logits' maximum (varhip_cfg_argmax_f32) — cfg_sample_f32 with top_k=1 on every row without an
        exact tie at its maximum; no sampler, no Exp(1) draw.  inp = (tokens, keep, ...) [B, L] of inpainting: the keep mask is fused in."""
        l, cur = sc.l, sc.cur
        self._logits(ws, B, sc, tr)
        idx = ws['idx'][:B * l]
        mask = (None, None, 0) if inp is None else (inp[1][:, cur:], inp[0][:, cur:], self.var.L)
        hip.call('cfg_argmax_f32', ws['logits'], *mask, idx, B, l, self.var.V, float(t))
        return idx

    def _smooth_select(self, ws: dict, B: int, sc, sm: dict, t: float, masked: Optional[torch.Tensor], tr: Optional[dict]) -> torch.Tensor:
        """neighbour-candidate selection instead of sampling (var.py:484-537, fork): no sampler, no Exp(1) draw, every position takes the most
        likely of the nearest codebook neighbours of its ground-truth token (sm: _smooth_setup); `masked` receives the CFG logits.  The two
        log-likelihoods accumulate in sm['ll'] and sm['dl']."""
        l, cur, r, n, thr = sc.l, sc.cur, sc.r, sm['n'], sm['thr']
        self._logits(ws, B, sc, tr)
        idx = ws['idx'][:B * l]
        hip.call('smooth_select_f32', ws['logits'], sm['gt'][:, cur:cur + l].contiguous(), sm['nbr_idx'], sm['nbr_dist'], n, 1 + int((n - 1) * r),
                 int(thr is not None), float(thr if thr is not None else 0.0), float(r), B, l, self.var.V, float(t),
                 idx, sm['val'], sm['dlp'], masked)
        # var.py:537: new_tensor(max_vals) has the tokens' dtype, so every value is truncated to an integer before the sum
        sm['ll'] = sm['ll'] + sm['val'][:B * l].to(torch.int64).sum()
        sm['dl'] = sm['dl'] + sm['dlp'][:B * l].sum()
        return idx

    def _edit_kept(self, B: int, sc, tokens: torch.Tensor, noise: '_Exp1', gumbel: Optional['_Exp1']) -> torch.Tensor:
        """an edit's scale whose tokens are all kept: no head, no sampler, no gumbel softmax, but the scale's fills are drawn as the notebook's
        loop draws them (it samples, then replaces), so the RNG stream stays that of a plain call; its tokens go to the plain quantizer step"""
        noise.draw(B, sc.si, sc.l, use=False)
        if gumbel is not None:
            gumbel.draw(B, sc.si, sc.l, use=False)
        return tokens[:, sc.cur:sc.cur + sc.l].contiguous().view(-1)

    def _publish(self, B: int, sc, idx: torch.Tensor, kept: bool, inp: Optional[tuple], ed: Optional[tuple], force_idx: Optional[torch.Tensor],
                 tokens_out: Optional[torch.Tensor], tr: Optional[dict]) -> torch.Tensor:
        """what happens to a scale's chosen tokens `idx` before the quantizer step -> the tokens that step takes.  kept: every token of the scale
        was kept (nothing was chosen).  inp = (tokens, keep, ...) of inpainting whose chooser did not apply the mask itself:
        torch.where(mask, gt_tokens, sampled) (var.py:326-328), in place.  force_idx (B, L): teacher forcing, replaces the tokens.  ed = (tokens,
        keep, ...) of an edit: the replacement happens inside the quantizer step, the final tokens are only materialised for the caller
        (tokens_out, trace).  The trace's 'idx' holds the final tokens, under edit its 'sampled' the chooser's (None on fully kept scales)."""
        l, cur = sc.l, sc.cur
        if inp is not None and not kept:
            hip.call('token_select_i64', inp[1][:, cur:cur + l].contiguous(), inp[0][:, cur:cur + l].contiguous(), idx, idx, B * l)
        if tr is not None:
            if kept: tr['logits'].append(None)
            if ed is not None: tr['sampled'].append(None if kept else idx.view(B, l).clone())
            if ed is None or kept: tr['idx'].append(idx.view(B, l).clone())
        if force_idx is not None:
            idx = force_idx[:, cur:cur + l].to(idx.device, torch.int64).contiguous().view(-1)
        fin = idx.view(B, l)
        if ed is not None and not kept and (tokens_out is not None or tr is not None):
            fin = torch.empty(B, l, dtype=torch.int64, device=idx.device)
            hip.call('token_select_i64', ed[1][:, cur:cur + l].contiguous(), ed[0][:, cur:cur + l].contiguous(), idx, fin, B * l)
            if tr is not None: tr['idx'].append(fin.clone())
        if tokens_out is not None:
            tokens_out[:, cur:cur + l].copy_(fin)
        return idx

    # -- the modes of sample(): argument checks and device preparation, each run only when its argument is given --------------------
    def _masked(self, ws: dict, B: int, soft: bool) -> torch.Tensor:
        """the workspace's buffer for the sampler's filtered logits (B * l_max * V * 4 bytes: more_smooth and stats share it), made on first use;
        soft: with it the gumbel-softmax probabilities and their embedding of more_smooth"""
        rows = sampler_rows(self._dims(), B, max(p * p for p in self.var.patch_nums))
        for key in ('masked', 'probs', 'h') if soft else ('masked',):
            shape, dt, _ = rows[key]
            if key not in ws:
                ws[key] = torch.empty(shape, dtype=dt, device=ws['dev'])
        return ws['masked']

    def _stats_setup(self, B: int, stats: dict, dev):
        """stats: the (B, L) tensors of STATS_FIELDS, allocated here unless the caller put contiguous ones there"""
        var = self.var
        for key in STATS_FIELDS:
            dt = _stats_dtype(key)
            if key not in stats:
                stats[key] = torch.empty(B, var.L, dtype=dt, device=dev)
            sv = stats[key]
            if sv.dtype != dt or tuple(sv.shape) != (B, var.L) or not sv.is_contiguous() or sv.device != dev:
                raise ValueError(f"stats['{key}'] must be a contiguous {dt} ({B}, {var.L}) tensor on the model's device")

    def _inpaint_setup(self, B: int, gt_tokens: torch.Tensor, keep_mask: Optional[torch.Tensor], more_smooth: bool, dev) -> tuple:
        """VAR.inpainting (var.py:236-364, fork): kept positions take the given token, the others are chosen; a scale whose tokens are all kept
        skips the head, the sampler and the RNG draw, as the reference does -> (tokens int64, keep uint8, both [B, L] on the device; per scale:
        is every token kept)"""
        var = self.var
        if keep_mask is None or tuple(keep_mask.shape) != tuple(gt_tokens.shape) or tuple(gt_tokens.shape) != (B, var.L):
            raise ValueError('Mask shape must match the latent token shape obtained from vae.img_to_idxBl')
        gt = gt_tokens.to(dev, torch.int64).contiguous()
        if int(gt.min()) < 0 or int(gt.max()) >= var.V:
            raise ValueError(f'gt_tokens must lie in [0, {var.V})')
        keep = keep_mask.to(dev).bool()
        skip = torch.stack([keep[:, b0:e0].all() for b0, e0 in var.begin_ends]).tolist()      # one host sync for all scales
        if more_smooth and any(skip):
            # var.py:312-341 (fork): on a fully kept scale the reference feeds the gumbel softmax the PREVIOUS scale's logits
            # (a NameError on the first scale, a shape error afterwards) — there is no behaviour to reproduce
            raise NotImplementedError('inpainting(more_smooth=True) with a fully kept scale: undefined in the reference (it reads logits it did not compute)')
        return gt, keep.to(torch.uint8).contiguous(), skip

    def _edit_setup(self, B: int, edit: dict, dev) -> tuple:
        """VAR.autoregressive_infer_cfg_with_mask (demo_zero_shot_edit.ipynb cell 2): the mask is resized to every scale on the device
        (varhip_edit_keep_u8); kept positions take codebook[token] in the quantizer step (varhip_quant_accum[_h]_edit_f32).  Unlike inpainting
        every scale draws its Exp(1) fill, and with more_smooth its gumbel fill (_edit_kept) -> (tokens int64, keep uint8, both [B, L] on the
        device; per scale: is every token kept)"""
        var = self.var
        tokens, mask = edit['tokens'], edit['mask']
        if tokens.dtype != torch.int64 or tuple(tokens.shape) != (B, var.L):
            raise ValueError(f'edit tokens must be an int64 ({B}, {var.L}) tensor')
        if mask.dtype != torch.float32 or mask.dim() != 3 or mask.shape[0] not in (1, B) or min(mask.shape[1:]) < 1:
            raise ValueError(f'edit mask must be a float32 (1 or {B}, h, w) tensor')
        tokens = tokens.to(dev).contiguous()
        if int(tokens.min()) < 0 or int(tokens.max()) >= var.V:
            raise ValueError(f'edit tokens must lie in [0, {var.V})')
        mask = mask.to(dev).contiguous()
        keep = torch.empty(B, var.L, dtype=torch.uint8, device=dev)
        pns = torch.tensor(var.patch_nums, dtype=torch.int32)               # a host array: the launcher copies it into the kernel's arguments
        hip.call('edit_keep_u8', mask, mask.shape[0], mask.shape[1], mask.shape[2], pns, len(var.patch_nums), B, keep)
        skip = torch.stack([keep[:, b0:e0].all() for b0, e0 in var.begin_ends]).tolist()      # one host sync for all scales
        return tokens, keep, skip

    def _smooth_setup(self, B: int, smooth: dict, dev) -> dict:
        """VAR.smooth_sampling (var.py:367-572, fork): the ground-truth tokens, the table of every code's n nearest codes, the per-position
        outputs of varhip_smooth_select_f32 and the two accumulated log-likelihoods (_smooth_select adds every scale's)"""
        var = self.var
        gt = smooth['gt'].to(dev, torch.int64).contiguous()
        n = int(smooth['n'])
        if tuple(gt.shape) != (B, var.L) or int(gt.min()) < 0 or int(gt.max()) >= var.V:
            raise ValueError(f'gt_tokens must be (B, L) token ids in [0, {var.V})')
        if not 1 <= n <= var.V:
            raise ValueError(f'n must lie in [1, {var.V}]')
        nbr_idx, nbr_dist = self.neighbor_table(n)
        rows = B * max(p * p for p in var.patch_nums)
        return dict(gt=gt, n=n, thr=smooth.get('thr'), nbr_idx=nbr_idx, nbr_dist=nbr_dist,
                    val=torch.empty(rows, dtype=torch.float32, device=dev), dlp=torch.empty(rows, dtype=torch.float32, device=dev),
                    ll=torch.zeros((), dtype=torch.float32, device=dev), dl=torch.zeros((), dtype=torch.float32, device=dev))

    # -- the loop ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, B: int, label_B: torch.Tensor, rng: Optional[torch.Generator], cfg: float, top_k: int, top_p: float,
               noises=None, force_idx: Optional[torch.Tensor] = None, trace: bool = False,
               decode: bool = True, gt_tokens: Optional[torch.Tensor] = None, keep_mask: Optional[torch.Tensor] = None,
               more_smooth: bool = False, gumbel_noises=None, smooth: Optional[dict] = None, greedy: bool = False,
               tokens_out: Optional[torch.Tensor] = None, edit: Optional[dict] = None, per_image: Optional[dict] = None,
               stats: Optional[dict] = None, kept_scales: Optional[tuple] = None) -> torch.Tensor:
        """label_B: int64 [B] on the device.  noises: optional per-scale Exp(1) tensors [B*l, V] — a list, or a callable
        (si, l) -> tensor (tests inject the CPU generator's stream; var_amd.multi hands each rank its rows); by default they
        are drawn with `exponential_(generator=rng)` exactly as torch.multinomial (helpers.py:19) would (_Exp1).  gumbel_noises: the same for
        the second fill per scale that more_smooth draws.
        gt_tokens/keep_mask [B, L]: VAR.inpainting (_inpaint_setup).  edit = dict(tokens=[B, L] int64, mask=[Bm, h, w] fp32, Bm in {1, B}):
        VAR.autoregressive_infer_cfg_with_mask (_edit_setup).  smooth = dict(gt=[B, L] tokens, n=int, thr=float|None): VAR.smooth_sampling
        (_smooth_setup); the two accumulated log-likelihoods are left in self.last_smooth.
        greedy=True: every chosen position takes the argmax of the CFG logits (_greedy); rng, noises, top_k and top_p are not read.
        tokens_out: optional int64 [B, L] on the device, receives every scale's tokens (kept and chosen).
        per_image = dict(t=[S, B] float64, top_k=[B] int32, top_p=[B] float64 on the device, cap=int): every image samples with its own
        parameters (sample_per_image builds the tables); cfg, top_k and top_p are not read.
        stats: a dict (VAR.autoregressive_infer_cfg_scored), receives the (B, L) tensors stats['logp_cond' | 'logp_guided' | 'logp_drawn' |
        'entropy'] (fp32) and stats['kept'] (int32).  One launch per scale and nothing else (_sampled): the RNG draws, the other kernels and
        their order are those of the call without it.  Combines with more_smooth and per_image; not with smooth, greedy, gt_tokens /
        keep_mask or edit, whose kept positions have no drawn distribution.
        kept_scales = (tokens int64 [B, L] on the device, first): every scale below `first` takes the given tokens by the route of a fully kept
        scale of inpainting — no head, no sampler, no draw (a callable noise source is not called for it), the plain quantizer step — and the
        scales from `first` on sample as without it (counterfactual).  With stats the kept scales' slices are left as the caller filled them.
        Not with gt_tokens / keep_mask, edit, smooth sampling, greedy selection or more_smooth.
        force_idx/trace are test hooks (teacher forcing; keep per-scale logits/tokens/f_hat, with stats also the filtered logits 'masked')."""
        var = self.var
        self.resolve_precision()
        self.refresh()
        self._wait_ready()
        ws = self.workspace(B)
        dev, S = ws['dev'], len(var.patch_nums)
        if label_B.dtype != torch.int64 or label_B.numel() != B:
            raise ValueError('label_B must be an int64 tensor of B labels')
        self._check_labels(label_B)
        label_B = label_B.to(dev).contiguous()
        if greedy and (more_smooth or smooth is not None):
            raise ValueError('greedy selection replaces the sampler: it does not combine with more_smooth or smooth sampling')
        if edit is not None and (gt_tokens is not None or keep_mask is not None or smooth is not None or greedy):
            raise ValueError('edit does not combine with gt_tokens / keep_mask, smooth sampling or greedy selection')
        if per_image is not None and (greedy or smooth is not None):
            raise ValueError('per-image parameters belong to the sampler: they do not combine with greedy selection or smooth sampling')
        if stats is not None and (smooth is not None or greedy or gt_tokens is not None or keep_mask is not None or edit is not None):
            raise ValueError('stats describe sampled tokens: they do not combine with smooth sampling, greedy selection, gt_tokens / keep_mask or edit')
        if kept_scales is not None and (gt_tokens is not None or keep_mask is not None or edit is not None or smooth is not None or greedy or more_smooth):
            raise ValueError('kept_scales does not combine with gt_tokens / keep_mask, edit, smooth sampling, greedy selection or more_smooth')
        if tokens_out is not None and (tokens_out.dtype != torch.int64 or tuple(tokens_out.shape) != (B, var.L) or not tokens_out.is_contiguous()):
            raise ValueError(f'tokens_out must be a contiguous int64 ({B}, {var.L}) tensor')
        tr = dict(logits=[], idx=[], f_hat=[], pooled=[]) if trace else None
        masked = self._masked(ws, B, more_smooth) if more_smooth or stats is not None else None
        if stats is not None:
            self._stats_setup(B, stats, dev)
        inp = self._inpaint_setup(B, gt_tokens, keep_mask, more_smooth, dev) if gt_tokens is not None else None
        ed = self._edit_setup(B, edit, dev) if edit is not None else None
        if ed is not None and trace: tr['sampled'] = []
        if smooth is not None and gt_tokens is not None:
            raise ValueError('smooth sampling and inpainting are separate entry points')
        sm = self._smooth_setup(B, smooth, dev) if smooth is not None else None
        skip = (inp or ed or (None, None, None))[2]
        forced = None
        if kept_scales is not None:
            forced, first = kept_scales
            if forced.dtype != torch.int64 or tuple(forced.shape) != (B, var.L) or forced.device != dev:
                raise ValueError(f'kept_scales tokens must be an int64 ({B}, {var.L}) tensor on the model\'s device')
            skip = [si < first for si in range(S)]
        noise = _Exp1(noises, rng, var.V, dev)
        gumbel = _Exp1(gumbel_noises, rng, var.V, dev) if more_smooth else None

        ws['f_hat'].zero_()
        self._prologue(ws, label_B, 2 * B)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(S + 2)] if getattr(self, 'profile_scales', False) else None
        for sc in self._scales(ws, B, 0, S - 1, tr, ev):
            t = cfg * sc.r if S > 1 else 0.0
            kept = skip is not None and skip[sc.si]
            if kept and ed is not None:
                idx = self._edit_kept(B, sc, ed[0], noise, gumbel)
            elif kept:        # inpainting, every token of this scale is kept: no head, no sampling, no RNG draw (var.py:312-313, fork)
                idx = (forced if inp is None else inp[0])[:, sc.cur:sc.cur + sc.l].contiguous().view(-1)
            elif sm is not None:
                idx = self._smooth_select(ws, B, sc, sm, t, masked, tr)
            elif greedy:
                idx = self._greedy(ws, B, sc, t, inp, tr)
            else:
                idx = self._sampled(ws, B, sc, noise, masked, t, top_k, top_p, per_image, stats, tr)
            sc.idx = self._publish(B, sc, idx, kept, None if greedy else inp, ed, force_idx, tokens_out, tr)
            if not kept:              # (a fully kept scale takes the plain quantizer step: under more_smooth it is an edit's, _inpaint_setup refuses its own)
                sc.ed = ed
                if more_smooth:
                    sc.soft = gumbel.draw(B, sc.si, sc.l)
        self.last_trace = tr
        self.last_smooth = (sm['ll'], sm['dl']) if sm is not None else None
        if not decode:
            return ws['f_hat'].permute(0, 3, 1, 2).contiguous()
        if ev: ev[S].record()
        img = self.dec.decode_nhwc(ws['f_hat'], precision=self.precision)     # var.py:190
        if ev:                                                            # tools/per_scale.py: ms per scale (blocks + head + sampler + quantizer step), then the decoder
            ev[S + 1].record(); torch.cuda.synchronize()
            self.last_scale_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(S + 1)]
        return img

    # -- per-image parameters and seeds (VAR.autoregressive_infer_cfg_per_image) --------------------------------------------
    @torch.no_grad()
    def sample_per_image(self, label_B: torch.Tensor, seeds, cfg, top_k, top_p, more_smooth: bool = False,
                         tokens_out: Optional[torch.Tensor] = None, trace: bool = False, decode: bool = True,
                         stats: Optional[dict] = None) -> torch.Tensor:
        """sample() on a batch of unrelated requests: image b uses seeds[b], cfg[b], top_k[b], top_p[b] (host sequences of length B, already
        validated: VAR.autoregressive_infer_cfg_per_image).  The noise is the project's counter-based stream (varhip_exp1_philox_f32): image
        b's rows depend on (seeds[b], scale, row, column, draw) only, the sampler reads image b's parameters from device tables
        (varhip_cfg_sample_rows_f32) — so a request's tokens do not depend on what it is batched with.  The tables are built and uploaded once,
        outside the scale loop; per scale: one fill launch, one sampler launch (and the draw-1 fill under more_smooth)."""
        per, seeds_d = self._per_image_upload(cfg, top_k, top_p, seeds)
        return self.sample(len(seeds), label_B, None, 0.0, 0, 0.0, noises=self._philox(seeds_d, 0), gumbel_noises=self._philox(seeds_d, 1) if more_smooth else None,
                           more_smooth=more_smooth, tokens_out=tokens_out, trace=trace, per_image=per, decode=decode, stats=stats)

    def _per_image_upload(self, cfg, top_k, top_p, seeds=None) -> tuple:
        """the device side of per-row sampler parameters (host sequences of one length R) -> (sample()'s `per_image` dict, the int64 [R] seeds on
        the device or None)"""
        var = self.var
        R, S, dev = len(cfg), len(var.patch_nums), var.pos_start.device
        tab = per_image_tables(cfg, top_k, top_p, S, var.V)
        # one upload: [S*R t | R top_p] float64, then the two integer tables
        f64 = torch.from_numpy(np.concatenate((tab['t'].reshape(-1), tab['top_p']))).to(dev)
        per = dict(t=f64[:S * R].view(S, R), top_p=f64[S * R:], top_k=torch.from_numpy(tab['top_k']).to(dev), cap=tab['cap'])
        return per, None if seeds is None else torch.from_numpy(np.asarray(seeds, dtype=np.int64)).to(dev)

    # -- temperature, min-p, logit bias and per-scale schedules (VAR.sample_controlled) ----------------------------------------------
    @torch.no_grad()
    def sample_controlled(self, label_B: torch.Tensor, seeds, tab: dict, tokens_out: Optional[torch.Tensor] = None, decode: bool = True,
                          stats: Optional[dict] = None, trace: bool = False) -> torch.Tensor:
        """sample_per_image(stats=...) with the sampler's whole parameter set per image and scale: tab is control_tables' result (validated
        there), seeds a host sequence of length B.  The walk, the Philox noise, the stats kernel, the quantizer step and the decode are those
        of sample_per_image; the one difference is the sampler's entry (_sampled: varhip_ctl_sample_rows_f32 reads the scale's rows of the
        tables).  logp_cond, logp_guided and entropy are the stats kernel's on the logits and t, so they describe the row before bias and
        temperature; logp_drawn and kept come from the filtered row the sampler left, so they describe the controlled distribution."""
        per, seeds_d = self._controlled_upload(tab, seeds)
        return self.sample(len(seeds), label_B, None, 0.0, 0, 0.0, noises=self._philox(seeds_d, 0), tokens_out=tokens_out, per_image=per,
                           decode=decode, stats=stats, trace=trace)

    def _controlled_upload(self, tab: dict, seeds=None) -> tuple:
        """the device side of control_tables' result, uploaded once, outside the scale loop -> (sample()'s `per_image` dict in its controlled form,
        the int64 [B] seeds on the device or None).  Three transfers, one per element type: [t | top_p] float64, [bias | tau | min_p] float32
        (the bias table first: its rows are read 16 bytes per lane and V % 256 == 0 keeps them aligned), [top_k | bias_row] int32."""
        dev = self.var.pos_start.device
        S, R = tab['t'].shape
        bias = tab['bias']
        nb = 0 if bias is None else bias.size
        f64 = torch.from_numpy(np.concatenate((tab['t'].reshape(-1), tab['top_p'].reshape(-1)))).to(dev)
        f32 = torch.from_numpy(np.concatenate(([] if bias is None else [bias.reshape(-1)]) + [tab['tau'].reshape(-1), tab['min_p'].reshape(-1)])
                               .astype(np.float32)).to(dev)
        i32 = torch.from_numpy(np.concatenate((tab['top_k'].reshape(-1), tab['bias_row'].reshape(-1))).astype(np.int32)).to(dev)
        n = S * R
        per = dict(t=f64[:n].view(S, R), top_p=f64[n:].view(S, R), tau=f32[nb:nb + n].view(S, R), min_p=f32[nb + n:].view(S, R),
                   top_k=i32[:n].view(S, R), bias_row=i32[n:].view(S, R), bias=None if bias is None else f32[:nb].view(-1, self.var.V),
                   cap=list(tab['cap']))
        return per, None if seeds is None else torch.from_numpy(np.asarray(seeds, dtype=np.int64)).to(dev)

    def _philox(self, seeds_d: torch.Tensor, draw: int):
        """the project's counter-based Exp(1) stream as a noise source of _Exp1: (si, l) -> the fill [R * l, V] of draw `draw` (0: the sampler's,
        1: the gumbel softmax's) of scale si, row r keyed by seeds_d[r] (varhip_exp1_philox_f32)"""
        R, V = seeds_d.numel(), self.var.V

        def fill(si, l):
            out = torch.empty(R * l, V, dtype=torch.float32, device=seeds_d.device)
            hip.call('exp1_philox_f32', seeds_d, R, l, V, si, draw, out)
            return out
        return fill

    # -- the noise behind given tokens, and its replay (VAR.abduct_noise / VAR.counterfactual) ---------------------------------------------
    @torch.no_grad()
    def abduct(self, gt_tokens: torch.Tensor, label_B: torch.Tensor, seeds, cfg, first: int) -> dict:
        """code_tokens' walk — the tokens are given, sc.idx = gt — with varhip_exp1_posterior_f32 behind the head of every scale >= first: the
        Exp(1) noise under which the unfiltered guided sampler of image b (guidance t[si][b] = cfg[b] * si / (S - 1), per_image_tables' roundings:
        those of varhip_cfg_sample_rows_f32's table) draws exactly these tokens, sampled from its law given that outcome with fresh values of
        the Philox stream keyed by seeds[b] (draws 2 and 3).  gt_tokens (B, L) int64 in [0, V) on the device, label_B (B,) int64, seeds and
        cfg host sequences of B values.  The logits are fp32 in every precision, so the call runs in f32, f16 and bf16 alike.
        -> dict(noise (B, L, V) fp32 — below `first` the stream's draw-2 fill, which nothing reads —, logp (B, L) fp32: log p(gt token) under
        the guided row, NaN below `first`; flags (B, L) int32: 1 where no noise explains the token (probability 0 or a NaN row: the row
        holds the prior fill, logp -inf); precision, sig: the arithmetic and the weights the logits came from).  Nothing is kept by the engine."""
        var = self.var
        B = gt_tokens.shape[0]
        self.resolve_precision()
        self.refresh()
        self._wait_ready()
        ws = self.workspace(B)
        dev, S, V, L = ws['dev'], len(var.patch_nums), var.V, var.L
        if label_B.dtype != torch.int64 or label_B.numel() != B:
            raise ValueError('label_B must be an int64 tensor of B labels')
        self._check_labels(label_B)
        label_B = label_B.to(dev).contiguous()
        gt = gt_tokens.to(dev, torch.int64).contiguous()
        per, seeds_d = self._per_image_upload(cfg, [0] * B, [0.0] * B, seeds)
        noise = torch.empty(B, L, V, dtype=torch.float32, device=dev)
        logp = torch.full((B, L), float('nan'), dtype=torch.float32, device=dev)
        flags = torch.zeros(B, L, dtype=torch.int32, device=dev)
        prior = self._philox(seeds_d, 2)
        for si in range(min(first, S)):
            b0, e0 = var.begin_ends[si]
            noise[:, b0:e0].copy_(prior(si, e0 - b0).view(B, e0 - b0, V))
        if first < S:
            ws['f_hat'].zero_()
            self._prologue(ws, label_B, 2 * B)
            for sc in self._scales(ws, B, 0, S - 1):
                if sc.si >= first:
                    self._logits(ws, B, sc, None)
                    hip.call('exp1_posterior_f32', ws['logits'], per['t'][sc.si], gt[:, sc.cur:], L, seeds_d, B, sc.l, V, sc.si,
                             noise[:, sc.cur:], logp[:, sc.cur:], flags[:, sc.cur:], L)
                sc.idx = gt[:, sc.cur:sc.cur + sc.l].contiguous().view(-1)
        return dict(noise=noise, logp=logp, flags=flags, precision=self.precision, sig=self._sig)

    @torch.no_grad()
    def counterfactual(self, noise: torch.Tensor, rows: torch.Tensor, gt_tokens: torch.Tensor, label_R: torch.Tensor, cfg, top_k, top_p, first: int,
                       tokens_out: torch.Tensor, stats: dict, decode: bool) -> Optional[torch.Tensor]:
        """sample() for R requests whose noise is stored: request r reads noise[rows[r]] ((B, L, V) fp32 of abduct, rows int64 [R] on the
        device), scale si its slice [cur, cur + l) — gathered per scale, (R, l, V), never the whole record — and samples under label_R[r]
        with its own cfg / top_k / top_p (host sequences of R values: sample_per_image's tables).  Scales below `first` are forced to
        gt_tokens ((R, L) int64 on the device) through sample()'s kept-scale route.  stats: the (R, L) tensors of STATS_FIELDS, filled by the
        caller; the kept scales' slices stay as they are.  No new sampler: varhip_cfg_sample_rows_f32 reads the stored noise.
        -> the images, or None (decode=False)"""
        var = self.var
        R = rows.numel()
        per, _ = self._per_image_upload(cfg, top_k, top_p)

        def stored(si, l):
            cur = var.begin_ends[si][0]
            return noise[:, cur:cur + l].index_select(0, rows).view(R * l, var.V)
        img = self.sample(R, label_R, None, 0.0, 0, 0.0, noises=stored, tokens_out=tokens_out, per_image=per, decode=decode, stats=stats,
                          kept_scales=(gt_tokens, first) if first > 0 else None)
        return img if decode else None

    def _begin_rows(self, who: str, what: str, label_N: torch.Tensor, N: int, n: int, most: int, max_images: int):
        """how a call over N = B * n rows, n `what` per image, opens: its limits, the call's precision and weights, the labels' check -> the device"""
        if n > most:
            raise ValueError(f'{who} takes at most {most} {what} per image, got {n}')
        if n > max_images:
            raise ValueError(f'max_images = {max_images} holds no whole image of n = {n} {what}')
        self.resolve_precision()
        self.refresh()
        self._wait_ready()
        if label_N.dtype != torch.int64 or label_N.numel() != N:
            raise ValueError('label_N must be an int64 tensor of B * n labels')
        self._check_labels(label_N)
        return self.var.pos_start.device

    def _scored_scales(self, ws: dict, R: int, first: int, last: int, per: dict, seeds_d: torch.Tensor, stats: dict, tokens: torch.Tensor):
        """scales first .. last of sample_per_image(stats=..., decode=False, tokens_out=tokens) for the R rows whose state sits in ws (_scales): the
        stages of sample_best_of_pruned and sample_smc.  ws['masked'] takes the filtered logits."""
        noise = _Exp1(self._philox(seeds_d, 0), None, self.var.V, ws['dev'])
        for sc in self._scales(ws, R, first, last):
            sc.idx = self._sampled(ws, R, sc, noise, ws['masked'], per=per, stats=stats)
            tokens[:, sc.cur:sc.cur + sc.l].copy_(sc.idx.view(R, sc.l))

    # -- weighted multi-class guidance (VAR.sample_composed) ------------------------------------------------------------------------
    @torch.no_grad()
    def sample_composed(self, labels: torch.Tensor, coef: np.ndarray, seeds, cfg, top_k, top_p, max_rows: int, decode: bool) -> dict:
        """sample_per_image with K classes per image mixed inside the sampler.  labels (B, K) int64, coef [S, B, K + 1] float32 (compose_tables),
        seeds / cfg / top_k / top_p host sequences of length B, all validated by the caller (cfg is only there for the tables' sake: the
        sampler reads coef).  G = K + 1 row groups run through the sampling walk, group-major with the unconditional group last: class k of
        image b is transformer row k * B + b.  Per scale: the head over the G * B * l rows, the Philox fill of sample_per_image (draw 0),
        varhip_mix_sample_rows_f32 (tokens, the filtered rows, the guided rows), varhip_sample_stats_f32 on (guided rows | zero rows) with
        t = 0 — 1 * m - 0 * 0 is m exactly, so its `guided` outputs describe the mixed row — and varhip_token_loglik_f32 on the G * B rows
        against the drawn tokens.  Passes of max_rows // G images; a pass is the per-image walk on its own images, so the split changes no bit
        of the tokens, and the decoder runs once on all B maps.
        -> dict(tokens (B, L) int64, logp_class (B, G, L), logp_guided, logp_drawn, entropy (B, L) fp32, kept (B, L) int32, images or None)"""
        var = self.var
        self.resolve_precision()
        self.refresh()
        self._wait_ready()
        dev = var.pos_start.device
        (B, K), G = labels.shape, labels.shape[1] + 1
        S, L, V, P, Cv = len(var.patch_nums), var.L, var.V, var.patch_nums[-1], var.Cvae
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
        out = dict(tokens=e(B, L, dt=torch.int64), logp_class=e(B, G, L), images=None)
        out.update(stats_record((B, L), dev, fields=STATS_FIELDS[1:]))
        f_all = e(B, P, P, Cv)
        ipp = max(1, int(max_rows) // G)
        for b0 in range(0, B, ipp):
            n = min(ipp, B - b0)
            ws = self._mix_workspace(n, G)
            per, seeds_d = self._per_image_upload(cfg[b0:b0 + n], top_k[b0:b0 + n], top_p[b0:b0 + n], seeds[b0:b0 + n])
            coef_d = torch.from_numpy(np.ascontiguousarray(coef[:, b0:b0 + n])).to(dev)
            lab = torch.cat((labels[b0:b0 + n].t().reshape(-1), torch.full((n,), var.num_classes, dtype=torch.int64, device=dev))).contiguous()
            lp_g, lp_own = e(G, n, L), e(n, L)                    # (lp_own: the stats kernel's `lp_cond` of the pair it is handed = logp_guided)
            noise = _Exp1(self._philox(seeds_d, 0), None, V, dev)
            ws['f_hat'].zero_()
            self._prologue(ws, lab, G * n)
            for sc in self._scales(ws, n, 0, S - 1, G=G):
                l, cur = sc.l, sc.cur
                self._logits(ws, n, sc, None, G)
                idx, mixed = ws['idx'][:n * l], ws['mixed'][:2 * n * l]
                mixed[n * l:].zero_()
                hip.call('mix_sample_rows_f32', ws['logits'], noise.draw(n, sc.si, l), idx, ws['masked'], mixed, n, l, V, G, coef_d[sc.si],
                         per['top_k'], per['top_p'], int(per['cap']))
                hip.call('sample_stats_f32', mixed, ws['masked'], idx, n, l, V, 0.0, None, lp_own[:, cur:],
                         *[out[key][b0:, cur:] for key in STATS_FIELDS[1:]], L)
                hip.call('token_loglik_f32', ws['logits'], idx.repeat(G), l, G * n, 1, l, V, 0, 1.0, 0.0, lp_g[:, :, cur:], L, L)
                out['tokens'][b0:b0 + n, cur:cur + l].copy_(idx.view(n, l))
                sc.idx = idx
            out['logp_class'][b0:b0 + n].copy_(lp_g.permute(1, 0, 2))
            f_all[b0:b0 + n].copy_(ws['f_hat'])
        if decode:
            out['images'] = self.dec.decode_nhwc(f_all, precision=self.precision)
        return out

    # -- best-of-n (VAR.sample_best_of) ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_best_of(self, label_N: torch.Tensor, seeds, cfg, top_k, top_p, n: int, by: str, max_images: int):
        """N = B * n candidates, candidate c of image b at position b * n + c (labels, seeds and parameters already spread and validated: host
        sequences of length N).  They run through sample_per_image with decode=False and stats in chunks of at most max_images; every chunk
        writes its rows of the (N, L) token / stats tensors and its f_hat maps.  varhip_class_select_f32 then adds stats[by] to float64 totals
        in token order and keeps each image's best candidate (higher total first, NaN below everything, ties by lower index).
        -> (dict of the B winners' tokens and stats (B, L), their f_hat (B, Cvae, P, P), totals (B, n) float64, choice (B,) int64)."""
        var = self.var
        dev = var.pos_start.device
        N, L, P, Cv = len(seeds), var.L, var.patch_nums[-1], var.Cvae
        B = N // n
        if n > self.CLASSIFY_MAX_CAND:
            raise ValueError(f'sample_best_of takes at most {self.CLASSIFY_MAX_CAND} candidates per image, got {n}')
        rec = stats_record((N, L), dev)
        rec['tokens'] = torch.empty(N, L, dtype=torch.int64, device=dev)
        f_all = torch.empty(N, Cv, P, P, dtype=torch.float32, device=dev)
        for c0 in range(0, N, max_images):
            c1 = min(N, c0 + max_images)
            f_all[c0:c1] = self.sample_per_image(label_N[c0:c1], seeds[c0:c1], cfg[c0:c1], top_k[c0:c1], top_p[c0:c1], tokens_out=rec['tokens'][c0:c1],
                                                 decode=False, stats={key: rec[key][c0:c1] for key in STATS_FIELDS})
        totals = torch.full((B, n), -0.0, dtype=torch.float64, device=dev)      # (-0.0 + x == x for every x)
        kept = torch.empty(B, 1, dtype=torch.int32, device=dev)
        hip.call('class_select_f32', rec[by], n * L, L, B, n, 0, L, totals, 1, kept)
        choice = kept[:, 0].long()
        win = torch.arange(B, device=dev) * n + choice
        return {key: v.index_select(0, win) for key, v in rec.items()}, f_all.index_select(0, win), totals, choice

    # -- best-of-n with per-scale pruning (VAR.sample_best_of_pruned) -------------------------------------------------------------------
    @torch.no_grad()
    def sample_best_of_pruned(self, label_N: torch.Tensor, seeds, cfg, top_k, top_p, n: int, by: str, schedule: list, max_images: int):
        """sample_best_of that stops sampling a candidate at the scale where it is dropped.  N = B * n candidates, candidate c of image b at
        position b * n + c (host sequences of length N, already spread and validated; an image's candidates share its label, cfg, top_k and
        top_p: candidate 0's are read).  schedule: [(scale, m), ...] ascending, each m below the survivor count before it (validated by the caller).
        One stage per boundary and a final one through the last scale; a stage runs its scales on a workspace of its own batch (_scored_scales).
        At a boundary behind scale s, after the quantizer step: varhip_class_select_f32 adds stats[by] of the stage's scales to the float64 running
        totals and keeps each image's best m (sample_best_of's rule); the survivors' seeds and f_hat rows are gathered, varhip_kv_compact moves
        their conditional and unconditional rows of every block's K and V cache (tokens 0 .. end(s) - 1) into the next stage's workspace in one
        launch, _prologue rebuilds the condition and AdaLN tables there, and next_map_f32 recomputes scale s + 1's input from the gathered f_hat.
        Survivor positions stay on the device: the stage batches follow from the schedule alone, and every host table of a chunk is uploaded
        before its first stage, so nothing waits for the host at a boundary.  Chunks hold max_images // n whole images.
        -> (dict of every candidate's tokens (int64, -1 past its depth) and stats (NaN / -1 past its depth), each (B, n, L); the winners' f_hat
        (B, Cvae, P, P); totals (B, n) float64 at each candidate's depth; depth (B, n) int64; choice (B,) int64).
        self.best_of_work: [(last scale of the stage, candidates per image, candidate row-tokens the transformer ran in it), ...]."""
        var = self.var
        N, L, S, V, H = len(seeds), var.L, len(var.patch_nums), var.V, var.num_heads
        B = N // n
        dev = self._begin_rows('sample_best_of_pruned', 'candidates', label_N, N, n, self.CLASSIFY_MAX_CAND, max_images)
        lab_img = label_N.to(dev).view(B, n)[:, 0].contiguous()
        stages, first, m = [], 0, n                                 # (first scale, last scale, candidates per image, kept behind it)
        for s, k in list(schedule) + [(S - 1, 1)]:
            stages.append((first, s, m, k))
            first, m = s + 1, k
        per_chunk = min(B, max_images // n)
        esz = 4 if self.precision == 'f32' else 2
        rec = stats_record((B, n, L), dev, fill=(-1, float('nan')))
        rec['tokens'] = torch.full((B, n, L), -1, dtype=torch.int64, device=dev)
        totals = torch.empty(B, n, dtype=torch.float64, device=dev)
        depth = torch.empty(B, n, dtype=torch.int64, device=dev)
        choice = torch.empty(B, dtype=torch.int64, device=dev)
        f_win = torch.empty(B, var.patch_nums[-1], var.patch_nums[-1], var.Cvae, dtype=torch.float32, device=dev)
        work = [[last, m, 0] for _, last, m, _ in stages]
        for b0 in range(0, B, per_chunk):
            b1 = min(B, b0 + per_chunk)
            nb = b1 - b0
            # every host table of the chunk, uploaded before its first stage: per stage the per-image sampler tables of its nb * m rows
            pers = [self._per_image_upload(*[[v for v in x[b0 * n:b1 * n:n] for _ in range(m)] for x in (cfg, top_k, top_p)])[0] for _, _, m, _ in stages]
            seeds_d = torch.from_numpy(np.asarray(seeds[b0 * n:b1 * n], dtype=np.int64)).to(dev)
            img = torch.arange(nb, device=dev).view(nb, 1)
            pos = torch.arange(n, device=dev).expand(nb, n).contiguous()        # the stage's candidates, ascending positions per image
            tot = torch.full((nb, n), -0.0, dtype=torch.float64, device=dev)     # their running totals (-0.0 + x == x for every x)
            prev = rows = None
            for j, (first, last, m, keep) in enumerate(stages):
                R = nb * m
                ws = self._bop_workspace(per_chunk * m, j)
                self._prologue(ws, lab_img[b0:b1].repeat_interleave(m), 2 * R)
                if j == 0:
                    ws['f_hat'][:R].zero_()
                else:
                    # the boundary's data movement: seeds and f_hat rows by torch gathers, the caches by one varhip_kv_compact launch
                    # (conditional rows 0 .. R-1 and their unconditional twins behind them, in the old batch and in the new one)
                    R0 = nb * stages[j - 1][2]
                    seeds_d = seeds_d.index_select(0, rows)
                    ws['f_hat'][:R].copy_(prev['f_hat'][:R0].index_select(0, rows))
                    rows2 = torch.cat((rows, rows + R0)).to(torch.int32)
                    hip.call('kv_compact', pointer_table(prev['kc'] + prev['vc']), pointer_table(ws['kc'] + ws['vc']), 2 * var.depth, rows2, 2 * R0, ws['kc'][0].shape[0],
                             2 * R, H, L, var.begin_ends[first][0], esz)
                    hip.call('next_map_f32', ws['f_hat'], self.w['word_w'], self.w['word_b'], ws['lvl_pos'][var.begin_ends[first][0]:], ws['x'], ws['pooled'],
                             R, var.patch_nums[-1], var.patch_nums[first], var.C, var.Cvae)
                st = stats_record((R, L), dev)
                tok = torch.empty(R, L, dtype=torch.int64, device=dev)
                self._scored_scales(ws, R, first, last, pers[j], seeds_d, st, tok)
                t0, t1 = var.begin_ends[first][0], var.begin_ends[last][1]
                rec['tokens'][b0:b1][img, pos, t0:t1] = tok.view(nb, m, L)[:, :, t0:t1]
                for key in STATS_FIELDS:
                    rec[key][b0:b1][img, pos, t0:t1] = st[key].view(nb, m, L)[:, :, t0:t1]
                kept = torch.empty(nb, min(keep, m), dtype=torch.int32, device=dev)
                hip.call('class_select_f32', st[by], m * L, L, nb, m, t0, t1, tot, keep, kept)
                totals[b0:b1][img, pos] = tot
                depth[b0:b1][img, pos] = last
                work[j][2] += R * (t1 - t0)
                kept = kept.long()
                rows = (img * m + kept).view(-1)                                # the survivors' rows in this stage's batch, ascending per image
                pos, tot, prev = pos.gather(1, kept), tot.gather(1, kept).contiguous(), ws
            choice[b0:b1] = pos[:, 0]
            f_win[b0:b1] = prev['f_hat'][:R].index_select(0, rows)
        self.best_of_work = [tuple(x) for x in work]
        return rec, f_win.permute(0, 3, 1, 2).contiguous(), totals, depth, choice

    # -- particle resampling at scale boundaries (VAR.sample_smc) -----------------------------------------------------------------------
    SMC_MAX_PARTICLES = 2048    # varhip_smc_resample_f32 stages an image's weights in LDS
    smc_reference = False       # test switch: the slow route of sample_smc (ancestors from the host twin, caches gathered out of place by torch)

    @torch.no_grad()
    def sample_smc(self, label_N: torch.Tensor, seeds, cfg, top_k, top_p, n: int, by: str, resample: list, beta: float, ess_frac: float,
                   rs_seeds, max_images: int):
        """n particles per image with resampling behind the scales of `resample` (ascending, below the last scale; validated by the caller).
        N = B * n particles, particle c of image b at position b * n + c (host sequences of length N, already spread and validated; an image's
        particles share its label, cfg, top_k and top_p).  rs_seeds: B integers, the key of each image's resampling uniform.
        One workspace of nb * n rows serves all stages of a chunk (sample_best_of_pruned's first-stage set: no second cache set), _prologue runs
        once.  A stage runs _scored_scales from the scale after the previous boundary through the next one; behind a boundary scale s, after its
        quantizer step: (a) varhip_smc_resample_f32 adds beta * (the stage's stats[by]) to the float64 log-weights, decides by the effective
        sample size and leaves the ancestor table, survivors in place; (b) the table plus the image's row offset, and its copy shifted by R for
        the unconditional twins, is the row index; (c) ONE varhip_kv_resample launch overwrites the dead rows of every block's K and V cache,
        tokens 0 .. end(s) - 1, in place; (d) the f_hat rows, the tokens and the statistic rows [:, :end(s)] are gathered by the table, so every
        slot's record is its lineage's; (e) next_map_f32 recomputes scale s + 1's input from f_hat.  A slot keeps its own seed: a copy diverges
        from its parent from scale s + 1 on.  Behind the last scale the weights take in the last stage without resampling.  did, anc and the
        count of refused rows stay on the device until the call ends; a non-zero count raises.  Chunks hold max_images // n whole images.
        -> dict(tokens, the STATS_FIELDS (each (B * n, L)), f_hat (B * n, Cvae, P, P), log_weights (B, n) f64, ancestors (B, K, n) int64,
        resampled (B, K) bool, ess (B, K) f64, log_weights_seen (B, K, n) f64).  Under smc_reference self.smc_pre_tokens holds, per boundary,
        the (B, n, end(s)) tokens before its gather (None otherwise).  self.smc_work: [(last scale of the stage, particle row-tokens the transformer ran), ...]."""
        var = self.var
        N, L, S, V, H = len(seeds), var.L, len(var.patch_nums), var.V, var.num_heads
        B, K = N // n, len(resample)
        dev = self._begin_rows('sample_smc', 'particles', label_N, N, n, self.SMC_MAX_PARTICLES, max_images)
        lab = label_N.to(dev)
        P, Cv = var.patch_nums[-1], var.Cvae
        stages, first = [], 0
        for s in list(resample) + [S - 1]:
            stages.append((first, s))
            first = s + 1
        per_chunk = min(B, max_images // n)
        esz = 4 if self.precision == 'f32' else 2
        ref = bool(self.smc_reference)
        rec = stats_record((N, L), dev)
        rec['tokens'] = torch.empty(N, L, dtype=torch.int64, device=dev)
        f_all = torch.empty(N, P, P, Cv, dtype=torch.float32, device=dev)
        logw = torch.zeros(B, n, dtype=torch.float64, device=dev)
        # per boundary (and one more set for the weight update behind the last scale), boundary-major so that a chunk's part is contiguous
        anc = torch.empty(K + 1, B, n, dtype=torch.int32, device=dev)
        did = torch.empty(K + 1, B, dtype=torch.int32, device=dev)
        ess = torch.empty(K + 1, B, dtype=torch.float64, device=dev)
        seen = torch.empty(K + 1, B, n, dtype=torch.float64, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        rs_np = np.asarray(rs_seeds, dtype=np.int64)
        rs_d = torch.from_numpy(rs_np).to(dev)
        pre =[[] for _ in range(K)]
        work = [[last, 0] for _, last in stages]
        for b0 in range(0, B, per_chunk):
            b1 = min(B, b0 + per_chunk)
            nb = b1 - b0
            R = nb * n
            per, seeds_d = self._per_image_upload(*[x[b0 * n:b1 * n] for x in (cfg, top_k, top_p, seeds)])
            ws = self._bop_workspace(per_chunk * n, 0)
            caches = ws['kc'] + ws['vc']
            ptrs = pointer_table(caches)
            off = (torch.arange(nb, device=dev, dtype=torch.int32) * n).view(nb, 1)
            self._prologue(ws, lab[b0 * n:b1 * n], 2 * R)
            ws['f_hat'][:R].zero_()
            st = {key: rec[key][b0 * n:b1 * n] for key in STATS_FIELDS}
            tok = rec['tokens'][b0 * n:b1 * n]
            lw = logw[b0:b1]
            for j, (first, last) in enumerate(stages):
                self._scored_scales(ws, R, first, last, per, seeds_d, st, tok)
                t0, t1 = var.begin_ends[first][0], var.begin_ends[last][1]
                work[j][1] += R * (t1 - t0)
                frac = ess_frac if j < K else 0.0               # (behind the last scale: ess >= 1 > 0 * n, the weights are updated and nothing moves)
                out = (lw, anc[j, b0:b1], did[j, b0:b1], ess[j, b0:b1], seen[j, b0:b1])             # (a)
                if not ref:
                    hip.call('smc_resample_f32', st[by], n * L, L, nb, n, t0, t1, float(beta), lw, rs_d[b0:b1], last, frac, *out[1:])
                else:
                    h = [x.cpu().numpy() for x in out]
                    hip.call_host('smc_resample_host_f32', st[by].cpu().numpy(), n * L, L, nb, n, t0, t1, float(beta), h[0], rs_np[b0:b1], last, frac,
                                  *h[1:])
                    for x, v in zip(out, h):
                        x.copy_(torch.from_numpy(v))
                if j == K:
                    break
                rows = (anc[j, b0:b1] + off).view(-1)                                   # (b) the slots' ancestors as rows of the chunk
                idx = torch.cat((rows, rows + R))
                if not ref:
                    hip.call('kv_resample', ptrs, len(caches), idx, 2 * R, H, L, t1, esz, bad)       # (c)
                else:
                    pre[j].append(tok[:, :t1].clone().view(nb, n, t1))
                    for t in caches:
                        t[:2 * R, :, :t1] = t[:2 * R, :, :t1].clone().index_select(0, idx.long())
                rows = rows.long()
                ws['f_hat'][:R].copy_(ws['f_hat'][:R].index_select(0, rows))            # (d)
                tok[:, :t1] = tok[:, :t1].index_select(0, rows)
                for key in STATS_FIELDS:
                    st[key][:, :t1] = st[key][:, :t1].index_select(0, rows)
                hip.call('next_map_f32', ws['f_hat'], self.w['word_w'], self.w['word_b'], ws['lvl_pos'][t1:], ws['x'], ws['pooled'],
                         R, P, var.patch_nums[last + 1], var.C, Cv)                      # (e)
            f_all[b0 * n:b1 * n] = ws['f_hat'][:R]
        if int(bad.item()) != 0:
            raise hip.VarHipError(f'sample_smc: varhip_kv_resample refused {int(bad.item())} rows (an ancestor table that is no table of fixed points)')
        self.smc_work = [tuple(x) for x in work]
        res = dict(rec, f_hat=f_all.permute(0, 3, 1, 2).contiguous(), log_weights=logw, ancestors=anc[:K].permute(1, 0, 2).long().contiguous(),
                   resampled=did[:K].t().ne(0).contiguous(), ess=ess[:K].t().contiguous(), log_weights_seen=seen[:K].permute(1, 0, 2).contiguous())
        self.smc_pre_tokens = [torch.cat(p, 0) for p in pre] if ref else None
        return res

    # -- lossless token coding (VAR.compress / VAR.decompress) -----------------------------------------------------------------
    def _codec_begin(self, who: str, B: int, label_B: torch.Tensor) -> tuple:
        """what code_tokens and decode_tokens share in front of the walk: f32 or ValueError (a stream written in one arithmetic cannot be read
        in another), the call's workspace, the checked labels -> (ws, labels on the device)"""
        if self.resolve_precision() != 'f32':
            raise ValueError(f'{who} runs in f32: a stream coded with {self.precision} tables could not be read in any other arithmetic '
                             f'(set_hip_precision(\'f32\'), no 16-bit autocast)')
        self.refresh()
        self._wait_ready()
        ws = self.workspace(B)
        if label_B.dtype != torch.int64 or label_B.numel() != B:
            raise ValueError('label_B must be an int64 tensor of B labels')
        self._check_labels(label_B)
        return ws, label_B.to(ws['dev']).contiguous()

    @torch.no_grad()
    def code_tokens(self, gt_tokens: torch.Tensor, label_B: torch.Tensor, cfg: float, last: int) -> tuple:
        """the encoder's half of VAR.compress: sample()'s walk over scales 0 .. last on 2B rows with the tokens given, and behind every scale's
        head varhip_code_table_f32 with gt: the (C, F) of every token under the table of its row, guidance t = cfg * si / (S - 1) as sample()
        forms it.  gt_tokens (B, L) int64 in [0, V) on the device, label_B (B,) int64.  One device-to-host copy after the walk
        -> (pairs (B, L, 2) uint32, flags (B, L) int32: varhip_code_table_f32's, both numpy; rows past scale `last` are zero)."""
        var = self.var
        B = gt_tokens.shape[0]
        ws, label_B = self._codec_begin('compress', B, label_B)
        dev, S = ws['dev'], len(var.patch_nums)
        gt = gt_tokens.to(dev, torch.int64).contiguous()
        out = torch.zeros(B, var.L, 3, dtype=torch.int32, device=dev)          # (C, F, flag) per token: one copy back
        pairs, flags = torch.zeros(B, var.L, 2, dtype=torch.int32, device=dev), torch.zeros(B, var.L, dtype=torch.int32, device=dev)
        ws['f_hat'].zero_()
        self._prologue(ws, label_B, 2 * B)
        for sc in self._scales(ws, B, 0, last):
            t = cfg * sc.r if S > 1 else 0.0
            self._logits(ws, B, sc, None)
            hip.call('code_table_f32', ws['logits'], B, sc.l, var.V, float(t), None, gt[:, sc.cur:], var.L, None, pairs[:, sc.cur:], flags[:, sc.cur:])
            sc.idx = gt[:, sc.cur:sc.cur + sc.l].contiguous().view(-1)
        out[:, :, :2] = pairs
        out[:, :, 2] = flags
        host = out.cpu().numpy()
        return np.ascontiguousarray(host[:, :, :2]).view(np.uint32), np.ascontiguousarray(host[:, :, 2])

    @torch.no_grad()
    def decode_tokens(self, words: np.ndarray, word_off: np.ndarray, nwords: np.ndarray, label_B: torch.Tensor, cfg: float, last: int,
                      fill: Optional[float], decode: bool) -> tuple:
        """the decoder's half of VAR.decompress: the same walk with the bitstream as the chooser.  Per coded scale: the head,
        varhip_code_table_f32 with cum_out = ws['masked'] (the buffer _masked provides), varhip_rans_decode_u32 into ws['idx']; the quantizer
        step and next_map as in sampling.  words: uint32, all images' streams back to back, image b's at word_off[b] with nwords[b] words
        (int64); uploaded once before the walk.  Scales past `last`: not run (fill None; their tokens stay -1), or chosen by _greedy with
        guidance fill * si / (S - 1).  No host synchronisation inside the walk: the coder's state, err and the tables' flags come back in one
        copy when it ends.  A token of -1 (an image in error) reaches the quantizer step as code 0; the caller raises for that image.
        -> (tokens (B, L) int64 on the device, images or None, state (B, 4) uint32, err (B,) int32, refused (B,) int32: rows of the image
        whose table was refused; the last three numpy)"""
        var = self.var
        B = int(nwords.shape[0])
        ws, label_B = self._codec_begin('decompress', B, label_B)
        dev, S, V = ws['dev'], len(var.patch_nums), var.V
        cum = self._masked(ws, B, False)
        words_d = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev) if words.size else torch.zeros(1, dtype=torch.int32, device=dev)
        off_d = torch.from_numpy(np.ascontiguousarray(word_off, np.int64)).to(dev)
        nw_d = torch.from_numpy(np.ascontiguousarray(nwords, np.int64)).to(dev)
        st = torch.zeros(B, 6, dtype=torch.int32, device=dev)                  # the coder's state (4 words), err, refused rows: one copy back
        state, err = st[:, :4].contiguous(), st[:, 4].contiguous()
        flags = torch.zeros(B, var.L, dtype=torch.int32, device=dev)
        tokens = torch.full((B, var.L), -1, dtype=torch.int64, device=dev)
        ws['f_hat'].zero_()
        self._prologue(ws, label_B, 2 * B)
        for sc in self._scales(ws, B, 0, last if fill is None else S - 1):
            if sc.si <= last:
                t = cfg * sc.r if S > 1 else 0.0
                self._logits(ws, B, sc, None)
                idx = ws['idx'][:B * sc.l]
                hip.call('code_table_f32', ws['logits'], B, sc.l, V, float(t), None, None, var.L, cum, None, flags[:, sc.cur:])
                hip.call('rans_decode_u32', cum, sc.l, V, words_d, int(words.size), off_d, nw_d, state, idx, err, B)
                tokens[:, sc.cur:sc.cur + sc.l].copy_(idx.view(B, sc.l))
                idx.clamp_(min=0)
            else:
                idx = self._greedy(ws, B, sc, fill * sc.r if S > 1 else 0.0, None, None)
                tokens[:, sc.cur:sc.cur + sc.l].copy_(idx.view(B, sc.l))
            sc.idx = idx
        img = self.dec.decode_nhwc(ws['f_hat'], precision=self.precision) if decode else None
        st[:, :4] = state
        st[:, 4] = err
        st[:, 5] = flags.ne(0).sum(1)
        host = st.cpu().numpy()
        return tokens, img, np.ascontiguousarray(host[:, :4]).view(np.uint32), np.ascontiguousarray(host[:, 4]), np.ascontiguousarray(host[:, 5])

    @torch.no_grad()
    def decode_f_hat(self, f_hat: torch.Tensor) -> torch.Tensor:
        """(B, Cvae, P, P) fp32 as sample(decode=False) returns it -> the images (B, 3, H, W) in [0, 1], by the call's own decoder step"""
        self.resolve_precision()
        return self.dec.decode_nhwc(f_hat.permute(0, 2, 3, 1).contiguous(), precision=self.precision)

    # -- teacher-forced logits (VAR.forward without autograd) ------------------------------------------------------------
    @torch.no_grad()
    def teacher_forced_logits(self, label_B: torch.Tensor, x_BLCv_wo_first_l: Optional[torch.Tensor]) -> torch.Tensor:
        """logits (B, L, V) of VAR.forward (reference var.py:192-234) for given next-scale inputs, computed scale by scale over the
        KV cache instead of one masked pass: the cache holds exactly the scales <= the current one, which is what the block-causal
        mask `attn_bias_for_masking` allows (SURVEY.md §4 identity (i): identical to 3e-8 in the reference itself).
        No CFG doubling: B rows.  label_B may contain num_classes (dropped condition)."""
        tf = self._tf_begin(label_B)
        R = int(label_B.numel())                               # rows: one per image, no CFG pair
        V = self.var.V
        self._check_labels(label_B)
        xin = None if x_BLCv_wo_first_l is None else x_BLCv_wo_first_l.to(tf.dev, torch.float32).contiguous()

        def head(p, si, cur, l):
            out[:, cur:cur + l] = p.ws['lg'][:R * l].view(R, l, V)
        for p in self._tf_rows(tf.lab.view(-1), xin, R):         # a single pass
            # (behind the workspace: a call with another row count frees the resident set before the logits are allocated)
            out = torch.empty(R, self.var.L, V, dtype=torch.float32, device=tf.dev)
            self._tf_pass(p, head=head)
        return out

    def _tf_begin(self, labels: torch.Tensor, gt_tokens: Optional[torch.Tensor] = None, f32_only: Optional[str] = None, before_tokens=None):
        """what every teacher-forced call does first: the call's precision (f32_only: the sentence, with {} for the precision, that refuses any
        other), the weights and the stream handshake; the labels on the device as int64; before_tokens(tf), the caller's own refusals and
        tables, which come before the tokens are touched; then the tokens (N, L) on the device as int64, and from them the teacher-forcing
        input of every image (eval_prob.py:437), one encode-side call for all of them -> (dev, lab, gt, xin); without tokens gt and xin are None"""
        var = self.var
        if self.resolve_precision() != 'f32' and f32_only:
            raise ValueError(f32_only.format(self.precision) + ' (set_hip_precision(\'f32\'), no 16-bit autocast)')
        self.refresh()
        self._wait_ready()
        tf = SimpleNamespace(dev=var.pos_start.device, dist=None, gt=None, xin=None)
        tf.lab = labels.to(tf.dev, torch.int64).contiguous()
        if before_tokens is not None:
            before_tokens(tf)
        if gt_tokens is not None:
            tf.gt = gt_tokens.to(tf.dev, torch.int64).contiguous()
            tf.xin = var.vae_proxy[0].quantize.idxBl_to_var_input([tf.gt[:, b:e] for b, e in var.begin_ends]).to(tf.dev, torch.float32)
        return tf

    def _tf_workspace(self, R: int, last: Optional[int] = None) -> dict:
        """buffers of a teacher-forced pass of up to R rows through scale `last` (default: the last scale): KV caches of L_e = end of that scale
        tokens, activations of its l_e = pn^2 rows per row; cached per (rows, HIP stream, precision, L_e), one R resident per L_e; a pass of fewer
        rows uses a prefix"""
        var = self.var
        last = len(var.patch_nums) - 1 if last is None else last
        Le = var.begin_ends[last][1]
        return self._workspace(self._ws_tf, self.MAX_WORKSPACES, R, (Le,), R, var.patch_nums[last] ** 2, Le, twin=True, logits='lg', Lmax=True)

    def _tf_rows(self, lab: torch.Tensor, xin: Optional[torch.Tensor], max_rows: int):
        """the pass loop of the calls that run one row per image: the N images of lab (N,) and xin (N, L - first_l, Cvae), in order, as passes p
        of at most max_rows rows over one workspace (sized once: a shorter last pass uses a prefix); p.i0: the pass's first image.  The loop
        body runs the pass (_tf_pass) between whatever it keeps per pass"""
        N = lab.shape[0]
        rpp = min(int(max_rows), N)
        ws = self._tf_workspace(rpp)
        for i0 in range(0, N, rpp):
            R = min(rpp, N - i0)
            yield SimpleNamespace(ws=ws, i0=i0, R=R, lab=lab[i0:i0 + R].contiguous(), xin=None if xin is None else xin[i0:i0 + R].contiguous())

    def _tf_pass(self, p, last: Optional[int] = None, done: int = -1, head=None, after_block=None, block=None):
        """one teacher-forced pass: the p.R rows of labels p.lab and next-scale inputs p.xin (R, >= L_e - first_l, Cvae) through scale `last`
        (default: the last; p.ws must reach it).  head(p, si, cur, l) runs after the head of each scale si > done has left that scale's fp32
        logits in p.ws['lg'][:R * l] (row r, token t at r * l + t); the scales up to `done` only fill the KV caches, and without `head` no
        scale runs a head.  after_block(p, bi, si, cur, l), if given, runs right behind every block: p.ws['q'] then holds that block's queries
        [R * l][C], normalised and scaled, p.ws['kc'][bi] the keys 0 .. cur + l - 1.  block(p, blk, bi, si, cur, l), if given, runs every block in
        place of self.block (patch_effects: the block with its interventions)"""
        var, w, ws, R = self.var, self.w, p.ws, p.R
        C, Cv = var.C, var.Cvae
        self._prologue(ws, p.lab, R)
        x, x2 = ws['x'], ws['x2']
        cur = 0
        for si, pn in enumerate(var.patch_nums[:(len(var.patch_nums) if last is None else last + 1)]):
            l = pn * pn
            if si > 0:                                           # word_embed(teacher-forcing input) + lvl_pos  (var.py:206-207)
                seg = p.xin[:, cur - var.first_l:cur - var.first_l + l].contiguous()
                hip.call('word_embed_f32', seg, w['word_w'], w['word_b'], ws['lvl_pos'][cur:], x, R, l, C, Cv)
            for bi, blk in enumerate(w['blocks']):
                if block is None:
                    self.block(blk, ws, bi, x, x2, R, l, cur, ws['Lmax'])
                else:
                    block(p, blk, bi, si, cur, l)
                if after_block is not None:
                    after_block(p, bi, si, cur, l)
            if head is not None and si > done:
                self.head(x, ws['hn'], ws['xn'], ws['lg'], R * l, l)
                head(p, si, cur, l)
            cur += l

    # -- teacher-forced class scoring (VAR.token_log_likelihood, VAR.token_scores) --------------------------------------------------
    @torch.no_grad()
    def token_log_likelihood(self, gt_tokens: torch.Tensor, labels: torch.Tensor, cfg: float, max_rows: int) -> torch.Tensor:
        """(N, K, L) fp32 log p(gt token) of every image under every candidate class (fork eval_prob.py:437-463; cfg > 0: the guided
        likelihood of var_analysis.py:322-349).  gt_tokens (N, L) int64 and labels (N, K) int64 on the device, already validated by the caller.
        The N x K rows are packed into passes of at most max_rows rows: images_in_pass x (classes_in_pass + [cfg > 0]), the unconditional
        row of every image of a pass (label num_classes) after its class rows.  Each scale's logits are reduced to one value per row by
        varhip_token_loglik_f32 right after the head: no (rows, L, V) tensor exists at any time."""
        return self.token_scores(gt_tokens, labels, cfg, max_rows, ('log_prob',))

    @torch.no_grad()
    def token_scores(self, gt_tokens: torch.Tensor, labels: torch.Tensor, cfg: float, max_rows: int, score: tuple) -> torch.Tensor:
        """(N, K, L) fp32 per-token scores of VAR.token_scores: as token_log_likelihood, with each scale's logits reduced by
        varhip_token_score_f32.  score: ('group_smoothed', group) | ('neighbor_max', threshold) | ('expected_distance', top_k or 0),
        already validated by the caller; ('log_prob',) is token_log_likelihood.  One stage through the last scale over every candidate."""
        sc = self._score_setup(gt_tokens, labels, cfg, dist=score[0] in _DIST_SCORES)
        N, K = labels.shape
        out = torch.empty(N, K, self.var.L, dtype=torch.float32, device=sc.dev)
        self._score_stage(sc, sc.lab, len(self.var.patch_nums) - 1, -1, max_rows, self._token_reducer(sc, score, out))
        return out

    @torch.no_grad()
    def distance_profile(self, gt_tokens: torch.Tensor, labels: torch.Tensor, cfg: float, max_rows: int, edges: torch.Tensor, min_prob: float):
        """VAR.distance_profile on the HIP path -> (mass_q, count), two (N, K, S, B) int64 arrays: as token_scores, with each scale's logits
        reduced behind the head by varhip_dist_profile_f32 into that scale's histograms (zeroed here, once per call).  edges: (B + 1,) fp32,
        min_prob: an fp32 value, both already validated by the caller."""
        sc = self._score_setup(gt_tokens, labels, cfg, dist=True)
        edges = edges.to(sc.dev, torch.float32).contiguous()
        N, K = labels.shape
        V, S, B = self.var.V, len(self.var.patch_nums), edges.numel() - 1
        mass, count = torch.zeros(N, K, S, B, dtype=torch.int64, device=sc.dev), torch.zeros(N, K, S, B, dtype=torch.int64, device=sc.dev)

        def reduce(p, si, cur, l):
            hip.call('dist_profile_f32', *p.args, sc.dist, V, edges, B, float(min_prob), mass[p.i0:, p.k0:, si], count[p.i0:, p.k0:, si], K * S * B, S * B)
        self._score_stage(sc, sc.lab, S - 1, -1, max_rows, reduce)
        return mass, count

    CLASS_MIX_LDS_V = 4096             # varhip_class_mix_f32 holds a token's mixture on the chip up to this V

    @torch.no_grad()
    def class_information(self, gt_tokens: torch.Tensor, labels: torch.Tensor, cfg: float, max_rows: int, prior: torch.Tensor) -> dict:
        """VAR.class_information on the HIP path -> dict(entropy (N, K, L), h_mix, h_cond, mi, logp_mix (N, L)) fp32: as token_scores, with
        each scale's logits reduced behind the head by varhip_class_mix_f32.  A pass that holds all K classes of its images finalises in that
        kernel; otherwise the chunks of an image add into an (L, V) int64 accumulator of the teacher-forced workspace (zeroed once per image)
        and varhip_class_mix_finish_f32 runs per scale after the last chunk.  prior: (N, K) fp32, already validated by the caller."""
        sc = self._score_setup(gt_tokens, labels, cfg)
        dev = sc.dev
        N, K = labels.shape
        L, V = self.var.L, self.var.V
        prior = prior.to(dev, torch.float32).contiguous()
        out = dict(entropy=torch.empty(N, K, L, dtype=torch.float32, device=dev))
        for k in ('h_mix', 'h_cond', 'mi', 'logp_mix'):
            out[k] = torch.empty(N, L, dtype=torch.float32, device=dev)

        def reduce(p, si, cur, l):
            i0, k0 = p.i0, p.k0
            mix = (*p.args, prior[i0:, k0:], K, out['entropy'][i0:, k0:, cur:], K * L, L)
            res = [out[k][i0:, cur:] for k in ('h_mix', 'h_cond', 'mi', 'logp_mix')]
            if p.nk == K and V <= self.CLASS_MIX_LDS_V:              # all classes of the pass's images: the mixture stays on the chip
                hip.call('class_mix_f32', *mix, None, None, None, 0, *res, L)
                return
            if k0 == 0 and si == 0:                                  # the chunked route: the sums of a full pass's images, zeroed once per image
                if 'class_mix' not in p.ws or p.ws['class_mix'][1].shape[0] < p.ipp:
                    p.ws['class_mix'] = (torch.empty(p.ipp, L, V, dtype=torch.int64, device=dev), torch.empty(p.ipp, L, dtype=torch.int64, device=dev),
                                         torch.empty(p.ipp, L, dtype=torch.int32, device=dev))
                for a in p.ws['class_mix']:
                    a[:p.ni].zero_()
            acc = [a[:, cur:] for a in p.ws['class_mix']]
            hip.call('class_mix_f32', *mix, *acc, L, None, None, None, None, 0)
            if k0 + p.nk == K:                                       # an image's last chunk
                hip.call('class_mix_finish_f32', *acc, L, sc.gt[i0:, cur:], L, p.ni, l, V, *res, L)
        self._score_stage(sc, sc.lab, len(self.var.patch_nums) - 1, -1, max_rows, reduce)
        return out

    def _token_reducer(self, sc, score: tuple, out: torch.Tensor):
        """the reducer of token_log_likelihood, token_scores and classify: one value per row and token into out (N, K, >= L_e), by
        varhip_token_loglik_f32 (score ('log_prob',)) or varhip_token_score_f32 in the mode score names, with its parameter"""
        K, Lo = out.shape[1:]
        if score[0] != 'log_prob':
            mode = _SCORE_MODES[score[0]]
            param, thr = (0, float(score[1])) if score[0] == 'neighbor_max' else (int(score[1]), 0.0)

        def reduce(p, si, cur, l):
            dst = out[p.i0:, p.k0:, cur:]
            if score[0] == 'log_prob':
                hip.call('token_loglik_f32', *p.args, dst, K * Lo, Lo)
            else:
                hip.call('token_score_f32', *p.args, mode, param, thr, sc.dist, self.var.V, dst, K * Lo, Lo)
        return reduce

    def _score_setup(self, gt_tokens: torch.Tensor, labels: torch.Tensor, cfg: float, dist: bool = False):
        """what every stage of a scoring call shares: _tf_begin's tokens, labels and teacher-forcing inputs, the code distance table (dist) or
        None, and the guidance factors"""
        def table(tf):
            tf.dist = self.code_distance_table()
            self._wait_ready()
        sc = self._tf_begin(labels, gt_tokens, before_tokens=table if dist else None)
        S = len(self.var.patch_nums)
        sc.u = 1 if cfg > 0 else 0
        # guidance factors per scale, rounded where var_analysis.py:333-344 rounds them (a float32 ratio tensor times the Python cfg)
        sc.t32 = [np.float32(np.float32(cfg) * np.float32(si / (S - 1) if S > 1 else 0.0)) for si in range(S)]
        return sc

    def _score_stage(self, sc, lab_all: torch.Tensor, last: int, done: int, max_rows: int, reduce):
        """one stage: the rows of labels lab_all (N, K) through scale `last`, packed into passes of at most max_rows rows:
        images_in_pass x (classes_in_pass + [cfg > 0]), the unconditional row of every image of a pass (label num_classes) after its class rows.
        Scales <= `done` only rebuild the KV caches; behind the head of each later scale runs reduce(p, si, cur, l), the caller's scoring
        kernel over the pass p: images p.i0 .. + p.ni, classes p.k0 .. + p.nk of lab_all (p.ipp: the images of a full pass), p.args the ten
        arguments every scoring kernel begins with (logits, the scale's tokens of the pass's images, the row geometry, the guidance factors)"""
        var = self.var
        dev = lab_all.device
        N, K = lab_all.shape
        L, V, u = var.L, var.V, sc.u
        if K + u <= max_rows:
            ipp, kpp = max(1, max_rows // (K + u)), K            # whole images per pass
        else:
            ipp, kpp = 1, max_rows - u                           # one image per pass, its classes in chunks (each pass with its own uncond row)
        passes = [(i0, min(ipp, N - i0), k0, min(kpp, K - k0)) for i0 in range(0, N, ipp) for k0 in range(0, K, kpp)]
        ws = self._tf_workspace(max(ni * (nk + u) for _, ni, _, nk in passes), last)   # sized once: a shorter pass uses a prefix
        xin_img = sc.xin[:, :var.begin_ends[last][1] - var.first_l]

        def head(p, si, cur, l):
            t = sc.t32[si]
            p.args = (ws['lg'], sc.gt[p.i0:, cur:], L, p.ni, p.nk, l, V, u, float(np.float32(1) + t), float(t))
            reduce(p, si, cur, l)
        for i0, ni, k0, nk in passes:
            rows_img = torch.arange(i0, i0 + ni, device=dev)
            lab = lab_all[i0:i0 + ni, k0:k0 + nk].reshape(-1)
            src = rows_img.repeat_interleave(nk)
            if u:
                lab = torch.cat((lab, torch.full((ni,), var.num_classes, dtype=torch.int64, device=dev)))
                src = torch.cat((src, rows_img))
            # the pass and the inputs gathered for it end with _tf_pass: a call holds one pass's copy however many passes it runs
            self._tf_pass(SimpleNamespace(ws=ws, R=ni * (nk + u), lab=lab.contiguous(), i0=i0, ni=ni, k0=k0, nk=nk, ipp=ipp, args=None,
                                          xin=xin_img.index_select(0, src).contiguous()),     # each image's input broadcast to its rows
                          last, done, head)

    # -- validation metrics (VAR.evaluate) -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate(self, gt_tokens: torch.Tensor, label_B: torch.Tensor, max_rows: int) -> dict:
        """the trainer's validation pass (reference trainer.py:54-84, :126-156) -> dict(nll_BL, smooth_BL (N, L) fp32, pred_BL int64, rank_BL
        int32, nll_S, smooth_S (S,) float64, correct_S (S,) int64, pred_hist_V (V,) int64).  gt_tokens (N, L) int64 and label_B (N,) int64,
        already validated by the caller; the labels are used as given.  The images are packed into passes of at most max_rows rows, one row per
        image; varhip_token_eval_f32 reduces each scale's logits right behind the head, varhip_eval_reduce_f32 the per-token arrays at the
        end: no (rows, L, V) tensor exists at any time."""
        var = self.var
        tf = self._tf_begin(label_B, gt_tokens)
        dev, gt = tf.dev, tf.gt
        L, V, S = var.L, var.V, len(var.patch_nums)
        N = gt.shape[0]
        out = dict(nll_BL=torch.empty(N, L, dtype=torch.float32, device=dev), smooth_BL=torch.empty(N, L, dtype=torch.float32, device=dev),
                   pred_BL=torch.empty(N, L, dtype=torch.int64, device=dev), rank_BL=torch.empty(N, L, dtype=torch.int32, device=dev),
                   nll_S=torch.empty(S, dtype=torch.float64, device=dev), smooth_S=torch.empty(S, dtype=torch.float64, device=dev),
                   correct_S=torch.empty(S, dtype=torch.int64, device=dev), pred_hist_V=torch.zeros(V, dtype=torch.int64, device=dev))

        def head(p, si, cur, l):
            hip.call('token_eval_f32', p.ws['lg'], gt[p.i0:, cur:], L, p.R, l, V, *[out[k][p.i0:, cur:] for k in ('nll_BL', 'smooth_BL', 'pred_BL', 'rank_BL')], L)
        for p in self._tf_rows(tf.lab, tf.xin, max_rows):
            self._tf_pass(p, head=head)
        begins = torch.tensor([0] + [e for _, e in var.begin_ends], dtype=torch.int32)      # a host array: the launcher copies it into the kernel's arguments
        hip.call('eval_reduce_f32', out['nll_BL'], out['smooth_BL'], out['pred_BL'], out['rank_BL'], L, N, begins, S, V,
                 out['nll_S'], out['smooth_S'], out['correct_S'], out['pred_hist_V'])
        return out

    # -- attention mass by key scale (VAR.attention_profile) ----------------------------------------------------------------------------
    ATTN_PROFILE_MAX_L, ATTN_PROFILE_MAX_S = 4096, 16          # the limits of varhip_attn_profile_f32 (include/var_hip.h)

    @torch.no_grad()
    def attention_profile(self, gt_tokens: torch.Tensor, label_N: torch.Tensor, radius: int, layers: tuple, max_rows: int,
                          return_tokens: bool = False, _tap=None) -> dict:
        """VAR.attention_profile on the HIP path -> dict(share_q (N, D', H, S, S + 1) int64, nan_queries (N, D', H, S) int32, tokens (N, D', H, L,
        S + 1) int32 or None).  gt_tokens (N, L) int64, label_N (N,) int64, layers: the selected block indices, ascending; all validated by the
        caller.  The images run teacher-forced in passes of at most max_rows rows, one row per image (no CFG rows); the head is skipped (no
        logits are needed); behind every selected block of every scale varhip_attn_profile_f32 reduces that block's queries (ws['q']) against
        its key cache into the (layer, query scale) slice of the outputs, zeroed here once.  The kernel keeps a scale's near bin behind its
        last key bin (index si + 1); it is moved to index S at the end.  _tap (tests): called after a stream sync with clones of the queries
        and of the keys 0 .. cur + l - 1 and (bi, si, cur, l) for every launch."""
        var = self.var
        L, S, H = var.L, len(var.patch_nums), var.num_heads

        def refusals(tf):
            if L > self.ATTN_PROFILE_MAX_L or S > self.ATTN_PROFILE_MAX_S:
                raise ValueError(f'attention_profile takes at most {self.ATTN_PROFILE_MAX_L} tokens and {self.ATTN_PROFILE_MAX_S} scales, got {L} and {S}')
            self._check_labels(tf.lab)
        tf = self._tf_begin(label_N, gt_tokens, 'attention_profile runs in f32: the {} workspaces hold 16-bit queries and keys', refusals)
        dev = tf.dev
        N, Dn = tf.gt.shape[0], len(layers)
        slot = {bi: d for d, bi in enumerate(layers)}
        share = torch.zeros(N, Dn, H, S, S + 1, dtype=torch.int64, device=dev)
        nanq = torch.zeros(N, Dn, H, S, dtype=torch.int32, device=dev)
        tokens = torch.zeros(N, Dn, H, L, S + 1, dtype=torch.int32, device=dev) if return_tokens else None
        ends = [torch.tensor([e for _, e in var.begin_ends[:si + 1]], dtype=torch.int32) for si in range(S)]      # host arrays: the launcher copies them

        def tap(p, bi, si, cur, l):
            d = slot.get(bi)
            if d is None:
                return
            ws, i0, R = p.ws, p.i0, p.R
            S1, pn = si + 1, var.patch_nums[si]
            tok = torch.empty(R, H, l, S1 + 1, dtype=torch.int32, device=dev) if return_tokens else None
            hip.call('attn_profile_f32', ws['q'], ws['kc'][bi], R, l, H, cur + l, ws['Lmax'], ends[si], S1, pn, int(radius),
                     share[i0:, d, :, si], Dn * H * S * (S + 1), S * (S + 1), p.nan[d, si], tok, H * l * (S1 + 1), l * (S1 + 1))
            if return_tokens:
                dst = tokens[i0:i0 + R, d, :, cur:cur + l]
                dst[..., :S1] = tok[..., :S1]
                dst[..., S] = tok[..., S1]
                if S1 < S:
                    dst[..., S1:S] = -(tok[..., :1] < 0).to(torch.int32)           # a NaN query: -1 in every entry
            if _tap is not None:
                torch.cuda.current_stream().synchronize()
                _tap(ws['q'][:R * l].clone(), ws['kc'][bi][:R, :, :cur + l].clone(), (bi, si, cur, l))
        for p in self._tf_rows(tf.lab, tf.xin, max_rows):
            p.nan = torch.zeros(Dn, S, p.R, H, dtype=torch.int32, device=dev)      # the kernel's nan_count is dense [row][head]
            self._tf_pass(p, after_block=tap)                             # no head: no logits are needed
            nanq[p.i0:p.i0 + p.R] = p.nan.permute(2, 0, 3, 1)
        for si in range(S - 1):                                       # near bin: from behind the scale's last key bin to index S
            share[..., si, S] = share[..., si, si + 1]
            share[..., si, si + 1] = 0
        return dict(share_q=share, nan_queries=nanq, tokens=tokens)

    # -- where a token looks (VAR.attention_maps, VAR.attention_rollout) ----------------------------------------------------------------
    @torch.no_grad()
    def attention_flow(self, gt_tokens: torch.Tensor, label_N: torch.Tensor, targets: tuple, layers: tuple, max_rows: int,
                       alpha: Optional[float] = None) -> dict:
        """VAR.attention_maps (alpha None) and VAR.attention_rollout (alpha in [0, 1]) on the HIP path -> dict(rows (N, D', H, T, L) fp32 or flow
        (N, T, L) fp32, nan_queries (N, D', H) int32).  gt_tokens (N, L) int64, label_N (N,) int64, targets: at most 32 flat token indices,
        layers: the selected block indices, ascending; all validated by the caller.  The images run teacher-forced in passes of at most
        max_rows rows, one row per image (no CFG rows, no head).  Behind every selected block of every scale its queries (ws['q']) go into a
        stash (D', R, L, C) that lives for this call only; after the pass ws['kc'][bi] holds every block's keys, and per selected layer
        varhip_attn_rowstats_f32 and varhip_attn_flow_f32 run once over all L queries: for the maps with a one-hot r and per_head = 1, for the
        rollout from the last selected layer to the first with per_head = 0, each layer's output the next one's r."""
        var = self.var
        L, S, H, C = var.L, len(var.patch_nums), var.num_heads, var.C

        def refusals(tf):
            if L > self.ATTN_PROFILE_MAX_L or S > self.ATTN_PROFILE_MAX_S:
                raise ValueError(f'attention maps and rollout take at most {self.ATTN_PROFILE_MAX_L} tokens and {self.ATTN_PROFILE_MAX_S} scales, '
                                 f'got {L} and {S}')
            self._check_labels(tf.lab)
        tf = self._tf_begin(label_N, gt_tokens, 'attention maps and rollout run in f32: the {} workspaces hold 16-bit queries and keys', refusals)
        dev = tf.dev
        N, Dn, T = tf.gt.shape[0], len(layers), len(targets)
        slot = {bi: d for d, bi in enumerate(layers)}
        ends = torch.tensor([e for _, e in var.begin_ends], dtype=torch.int32)            # a host array: the launcher copies it
        rpp = min(int(max_rows), N)
        onehot = torch.zeros(rpp, T, L, dtype=torch.float32, device=dev)
        onehot[:, torch.arange(T, device=dev), torch.tensor(targets, dtype=torch.int64, device=dev)] = 1.0
        stash = torch.empty(Dn, rpp, L, C, dtype=torch.float32, device=dev)
        m, rinv = (torch.empty(rpp, H, L, dtype=torch.float32, device=dev) for _ in range(2))
        nanq = torch.zeros(N, Dn, H, dtype=torch.int32, device=dev)
        if alpha is None:
            out = torch.empty(N, Dn, H, T, L, dtype=torch.float32, device=dev)
            rows = torch.empty(rpp, H, T, L, dtype=torch.float32, device=dev)
        else:
            out = torch.empty(N, T, L, dtype=torch.float32, device=dev)
            ping = [torch.empty(rpp, T, L, dtype=torch.float32, device=dev) for _ in range(2)]

        def tap(p, bi, si, cur, l):
            d = slot.get(bi)
            if d is not None:
                stash[d, :p.R, cur:cur + l] = p.ws['q'][:p.R * l].view(p.R, l, C)
        for p in self._tf_rows(tf.lab, tf.xin, max_rows):
            ws, i0, R = p.ws, p.i0, p.R
            self._tf_pass(p, after_block=tap)                             # no head: no logits are needed
            r = onehot
            for d in (range(Dn) if alpha is None else reversed(range(Dn))):
                bi = layers[d]
                cnt = torch.zeros(R, H, dtype=torch.int32, device=dev)
                hip.call('attn_rowstats_f32', stash[d], ws['kc'][bi], R, L, H, ws['Lmax'], ends, S, m, rinv, cnt)
                nanq[i0:i0 + R, d] = cnt
                if alpha is None:
                    hip.call('attn_flow_f32', stash[d], ws['kc'][bi], m, rinv, onehot, rows, R, L, H, ws['Lmax'], ends, S, T, 1, 0.0)
                    out[i0:i0 + R, d] = rows[:R]
                else:
                    dst = ping[0] if r is not ping[0] else ping[1]
                    hip.call('attn_flow_f32', stash[d], ws['kc'][bi], m, rinv, r, dst, R, L, H, ws['Lmax'], ends, S, T, 0, float(alpha))
                    r = dst
            if alpha is not None:
                out[i0:i0 + R] = r[:R]
        return {'rows' if alpha is None else 'flow': out, 'nan_queries': nanq}

    # -- every block's prediction against the final one (VAR.logit_lens) ----------------------------------------------------------------
    @torch.no_grad()
    def logit_lens(self, gt_tokens: torch.Tensor, label_N: torch.Tensor, layers: tuple, max_rows: int, _tap=None) -> dict:
        """VAR.logit_lens on the HIP path -> dict(nll, entropy, kl (N, D', L) fp32, pred int64, rank int32).  gt_tokens (N, L) int64, label_N
        (N,) int64, layers: the selected block indices, ascending; all validated by the caller.  The images run teacher-forced in passes of at
        most max_rows rows, one row per image, as in evaluate.  Per scale, the residual stream behind every selected block but the model's last
        (ws['x'][:R * l]) is copied into its stash slot; behind the head, which has left the final logits in ws['lg'], the head runs once more
        per stashed layer into a second logits buffer lg2 and varhip_token_lens_f32 reduces (lg2, ws['lg']) into the (layer, scale) slice of
        the outputs.  The model's last block is reduced with logits = final_logits = ws['lg'] (no second GEMM).  No per-layer (rows, L, V)
        tensor exists at any time; the stash (D' x R lmax x C fp32) and lg2 (R lmax x V) live for the call only.  _tap (tests): called after a
        stream sync with clones of the layer's logits, of ws['lg'] and (bi, si, cur, l) for every launch."""
        var = self.var
        tf = self._tf_begin(label_N, gt_tokens)
        dev, gt = tf.dev, tf.gt
        L, V, C = var.L, var.V, var.C
        N, Dn = gt.shape[0], len(layers)
        final = var.depth - 1
        slot = {bi: d for d, bi in enumerate(layers)}
        e = lambda dt: torch.empty(N, Dn, L, dtype=dt, device=dev)
        out = dict(nll=e(torch.float32), entropy=e(torch.float32), kl=e(torch.float32), pred=e(torch.int64), rank=e(torch.int32))
        keys = ('nll', 'entropy', 'kl', 'pred', 'rank')
        stash = lg2 = None

        def keep(p, bi, si, cur, l):
            if bi in slot and bi != final:
                stash[slot[bi], :p.R * l].copy_(p.ws['x'][:p.R * l])

        def head(p, si, cur, l):
            ws, R = p.ws, p.R
            for bi in layers:
                d = slot[bi]
                lg = ws['lg']
                if bi != final:
                    lg = lg2
                    self.head(stash[d], ws['hn'], ws['xn'], lg2, R * l, l)
                hip.call('token_lens_f32', lg, ws['lg'], gt[p.i0:, cur:], L, R, l, V, *[out[k][p.i0:, d, cur:] for k in keys], Dn * L)
                if _tap is not None:
                    torch.cuda.current_stream().synchronize()
                    _tap(lg[:R * l].clone(), ws['lg'][:R * l].clone(), (bi, si, cur, l))
        for p in self._tf_rows(tf.lab, tf.xin, max_rows):
            if stash is None:                                         # (behind the workspace, sized by the passes' row count)
                M = p.R * var.patch_nums[-1] ** 2
                stash = torch.empty(max(Dn - (final in slot), 1), M, C, dtype=torch.float32, device=dev)
                lg2 = torch.empty(M, V, dtype=torch.float32, device=dev)
            self._tf_pass(p, head=head, after_block=keep)
        return out

    # -- the final logit as a sum over heads and MLPs (VAR.logit_attribution) ------------------------------------------------------------
    DLA_MODE = dict(gt=0, margin=1, against=2)         # the `mode` of varhip_dla_target_f32

    @torch.no_grad()
    def logit_attribution(self, gt_tokens: torch.Tensor, label_N: torch.Tensor, mode: str, against: Optional[torch.Tensor], layers: tuple,
                          max_rows: int, _tap=None) -> dict:
        """VAR.logit_attribution on the HIP path -> dict(value, konst, embed, rest, residual (N, L) fp32, attn, mlp, attn_bias (N, D', L) fp32,
        head (N, D', H, L) fp32, rival (N, L) int64).  gt_tokens (N, L) int64, label_N (N,) int64; mode 'gt' | 'margin' | 'against' with
        against (N, L) int64; layers: the selected block indices, ascending; all validated by the caller (against is NOT range-checked: the
        kernels answer an out-of-range rival with NaN).  The images run teacher-forced in passes of at most max_rows rows, one row per image, as
        in evaluate.  Per scale the residual stream in front of every selected block and behind it (shared where two selected blocks follow one
        another), the stream behind its attention residual (ws['x2'] when the block returns) and its proj input (ws['att']) are copied into the
        call's stash.  Behind the scale's head varhip_dla_target_f32 reads the target off ws['lg'], varhip_dla_direction_f32 makes ghat, konst and
        ghat . x from the final stream, and per selected block the product ghat * gamma1 (one torch multiply: one fp32 rounding per element),
        u = (ghat * gamma1) proj.weight (varhip_gemm_nt_f32 on a transposed copy of proj.weight, made at the start of the call) and
        varhip_rowdot_seg_f64 on (ghat, every kept stream), (u, att) per head and (ghat * gamma1, proj.bias) give float64 dots.  The terms are
        their differences in float64 (torch, element-wise), rounded to fp32 once.  The stash (at most 3 D' + 1 buffers of R lmax x C fp32), the
        transposed weights and the dots live for the call only.  _tap (tests): called after a stream sync with a dict of clones of everything
        the reductions of a scale read, and of u, and (si, cur, l)."""
        var = self.var
        tf = self._tf_begin(label_N, gt_tokens, 'logit_attribution runs in f32: the {} workspaces hold 16-bit activations',
                            lambda tf: self._check_labels(tf.lab))
        w = self.w                                                    # (behind _tf_begin: it refreshes the weight table)
        dev, gt = tf.dev, tf.gt
        L, V, C, H, depth = var.L, var.V, var.C, var.num_heads, var.depth
        N, Dn = gt.shape[0], len(layers)
        kmode = self.DLA_MODE[mode]
        against = None if against is None else against.to(dev, torch.int64).contiguous()
        slot = {bi: d for d, bi in enumerate(layers)}
        # stream point k: the stream in front of block k (= behind block k - 1); point `depth` is ws['x'] at the head and needs no copy
        pt = {k: i for i, k in enumerate(sorted(({0} | set(layers) | {bi + 1 for bi in layers}) - {depth}))}
        f = lambda *s: torch.empty(N, *s, dtype=torch.float32, device=dev)
        out = dict(value=f(L), konst=f(L), embed=f(L), rest=f(L), residual=f(L), attn=f(Dn, L), mlp=f(Dn, L), attn_bias=f(Dn, L), head=f(Dn, H, L),
                   rival=torch.empty(N, L, dtype=torch.int64, device=dev))
        projT = {bi: w['blocks'][bi]['proj_w'].t().contiguous() for bi in layers}          # u = gg projT^T on the NT GEMM; freed with the call
        st = None

        def block(p, blk, bi, si, cur, l):
            n = p.R * l
            if bi in pt:
                st.pts[pt[bi], :n].copy_(p.ws['x'][:n])
            self.block(blk, p.ws, bi, p.ws['x'], p.ws['x2'], p.R, l, cur, p.ws['Lmax'])
            if bi in slot:
                st.mid[slot[bi], :n].copy_(p.ws['x2'][:n])
                st.att[slot[bi], :n].copy_(p.ws['att'][:n])

        def head(p, si, cur, l):
            ws, R, i0 = p.ws, p.R, p.i0
            n = R * l
            hn = ws['hn']
            g_, riv = gt[i0:, cur:], out['rival'][i0:, cur:]
            hip.call('dla_target_f32', ws['lg'], g_, None if against is None else against[i0:, cur:], L, kmode, R, l, V, riv, out['value'][i0:, cur:], L)
            hip.call('dla_direction_f32', ws['x'], hn, hn[:, C:], 2 * C, w['head_w'], w['head_b'], g_, None if kmode == 0 else riv, L, R, l, C, V,
                     var.norm_eps, st.ghat, st.konst, st.dpt[-1], l)
            for k, i in pt.items():
                hip.call('rowdot_seg_f64', st.ghat, C, st.pts[i], C, n, C, 1, st.dpt[i])
            g1 = {}
            for bi in layers:
                d, blk = slot[bi], w['blocks'][bi]
                hip.call('rowdot_seg_f64', st.ghat, C, st.mid[d], C, n, C, 1, st.dmid[d])
                ada, ld = ws['ada_view'][bi]
                g1[bi] = torch.as_strided(ada, (R, 1, C), (ld, 0, 1), ada.storage_offset())          # gamma1 of every row
                torch.mul(st.ghat[:n].view(R, l, C), g1[bi], out=st.gg[:n].view(R, l, C))
                self.gemm(st.gg, projT[bi], None, st.u, n)
                hip.call('rowdot_seg_f64', st.u, C, st.att[d], C, n, C, H, st.dhead[d])
                hip.call('rowdot_seg_f64', st.gg, C, blk['proj_b'], 0, n, C, 1, st.dbias[d])
                if _tap is not None:
                    torch.cuda.current_stream().synchronize()
                    _tap(dict(block=bi, u=st.u[:n].clone(), gg=st.gg[:n].clone(), g1=g1[bi].reshape(R, C).clone(), mid=st.mid[d, :n].clone(),
                              att=st.att[d, :n].clone()), (si, cur, l))
            xf = st.dpt[-1][:n]
            at = lambda k: xf if k == depth else st.dpt[pt[k]][:n]
            embed = at(0)
            rest = xf - embed
            img = lambda t: t.view(R, l).to(torch.float32)
            for bi in layers:
                d = slot[bi]
                attn, mlp = st.dmid[d][:n] - at(bi), at(bi + 1) - st.dmid[d][:n]
                rest = rest - (attn + mlp)
                out['attn'][i0:i0 + R, d, cur:cur + l] = img(attn)
                out['mlp'][i0:i0 + R, d, cur:cur + l] = img(mlp)
                out['attn_bias'][i0:i0 + R, d, cur:cur + l] = img(st.dbias[d][:n])
                out['head'][i0:i0 + R, d, :, cur:cur + l] = st.dhead[d][:n * H].view(R, l, H).permute(0, 2, 1).to(torch.float32)
            out['embed'][i0:i0 + R, cur:cur + l] = img(embed)
            out['rest'][i0:i0 + R, cur:cur + l] = img(rest)
            out['konst'][i0:i0 + R, cur:cur + l] = img(st.konst[:n])
            out['residual'][i0:i0 + R, cur:cur + l] = img(out['value'][i0:i0 + R, cur:cur + l].double().reshape(-1) - (st.konst[:n] + xf))
            if _tap is not None:
                torch.cuda.current_stream().synchronize()
                _tap(dict(block=None, lg=ws['lg'][:n].clone(), x=ws['x'][:n].clone(), hn=hn[:R].clone(), ghat=st.ghat[:n].clone(),
                          pts={k: st.pts[i, :n].clone() for k, i in pt.items()}, i0=i0, R=R), (si, cur, l))
        for p in self._tf_rows(tf.lab, tf.xin, max_rows):
            if st is None:                                            # (behind the workspace, sized by the passes' row count)
                M = p.R * var.patch_nums[-1] ** 2
                e32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
                e64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
                st = SimpleNamespace(pts=e32(len(pt), M, C), mid=e32(Dn, M, C), att=e32(Dn, M, C), ghat=e32(M, C), gg=e32(M, C), u=e32(M, C),
                                     dpt=e64(len(pt) + 1, M), dmid=e64(Dn, M), dbias=e64(Dn, M), dhead=e64(Dn, M * H), konst=e64(M))
            self._tf_pass(p, head=head, block=block)
        return out

    # -- head / MLP ablation and activation patching (VAR.patch_effects) ----------------------------------------------------------------
    PATCH_SRC = dict(zero=-1, mean=-2)                 # the `src` of varhip_act_patch_f32's directives; 'donor': the donor row's index

    @torch.no_grad()
    def patch_effects(self, gt_tokens: torch.Tensor, label_N: torch.Tensor, sites: tuple, mode: str, donor_N: Optional[torch.Tensor], scales: tuple,
                      max_rows: int, _tap=None) -> dict:
        """VAR.patch_effects on the HIP path -> dict(nll, entropy, kl (N, P + 1, L) fp32, pred int64, rank int32), index 0 the clean row.
        gt_tokens (N, L) int64, label_N (N,) int64; sites: P entries, each a tuple of elementary sites ('att' | 'hid', block, c0, c1); mode
        'zero' | 'mean' | 'donor' with donor_N (N,) int64 labels; scales: the scale indices at which the interventions apply, ascending; all
        validated by the caller.  The rows of a pass are image-major: per image the donor row (mode 'donor': the image's tokens under its
        donor label), the clean row, then one row per site.  Images whose rows fit max_rows share passes; otherwise an image's sites are chunked
        over passes, each with its own clean (and donor) row, as token_scores chunks classes.  The directives of every block are built on the
        host and uploaded once per pass layout (image count, site chunk); a block with directives at an active scale runs
        varhip_adaln_block_patched_f32, every other block self.block.  Behind each scale's head the clean row of every row's image is
        gathered into a second logits buffer and varhip_token_lens_f32 reduces (row, its clean row): no (rows, L, V) tensor exists at any
        time, and the tables, the second buffer and the per-pass outputs live for the call only.  _tap (tests): called after a stream sync
        with clones of the scale's logits, of the gathered clean rows, the pass's (image, slot) per row (slot -1: the donor row, 0: the clean
        row, j + 1: site j) and (si, cur, l)."""
        var = self.var
        tf = self._tf_begin(torch.stack((label_N, label_N if donor_N is None else donor_N), 1), gt_tokens,
                            'patch_effects runs in f32: the {} workspaces hold 16-bit activations', lambda tf: self._check_labels(tf.lab))
        dev, gt = tf.dev, tf.gt
        L, V, C, S = var.L, var.V, var.C, len(var.patch_nums)
        N, P = gt.shape[0], len(sites)
        d = 1 if mode == 'donor' else 0
        keys = ('nll', 'entropy', 'kl', 'pred', 'rank')
        dts = (torch.float32, torch.float32, torch.float32, torch.int64, torch.int32)
        out = {k: torch.empty(N, P + 1, L, dtype=dt, device=dev) for k, dt in zip(keys, dts)}
        if d + 1 + P <= max_rows:
            ipp, spp = max(1, max_rows // (d + 1 + P)), P                # whole images per pass
        else:
            ipp, spp = 1, max_rows - d - 1                               # one image per pass, its sites in chunks
        passes = [(i0, min(ipp, N - i0), j0, min(spp, P - j0)) for i0 in range(0, N, ipp) for j0 in range(0, P, spp)]
        Rmax = max(ni * (d + 1 + nj) for _, ni, _, nj in passes)
        ws = self._tf_workspace(Rmax)                                    # sized once: a shorter pass uses a prefix
        lg2 = torch.empty(Rmax * var.patch_nums[-1] ** 2, V, dtype=torch.float32, device=dev)
        res = [torch.empty(Rmax, L, dtype=dt, device=dev) for dt in dts]
        active = set(scales)
        layouts = {}

        def layout(ni, j0, nj):
            """the rows of a pass of ni images with the sites j0 .. j0 + nj: (image, slot) per row, each row's clean row, and per block the
            device tables of the attention and the hidden directives; built once, one upload"""
            if (ni, j0, nj) not in layouts:
                per = d + 1 + nj
                rows = [(i, s) for i in range(ni) for s in ([-1] * d + [0] + list(range(j0 + 1, j0 + nj + 1)))]
                tabs = {}
                for i in range(ni):
                    src = i * per if d else self.PATCH_SRC[mode]
                    for j in range(nj):
                        for kind, bi, c0, c1 in sites[j0 + j]:
                            tabs.setdefault((bi, kind), []).extend((i * per + d + 1 + j, c0, c1, src))
                flat, where = [], {}
                for key, t in tabs.items():
                    where[key] = (len(flat), len(t) // 4)
                    flat.extend(t)
                table = torch.tensor(flat or [0], dtype=torch.int32).to(dev)
                views = {key: (table[o:], n) for key, (o, n) in where.items()}
                layouts[(ni, j0, nj)] = SimpleNamespace(rows=rows, views=views, blocks={bi for bi, _ in tabs},
                                                        clean=torch.tensor([i * per + d for i, _ in rows], dtype=torch.int64).to(dev))
            return layouts[(ni, j0, nj)]

        def block(p, blk, bi, si, cur, l):
            if si not in active or bi not in p.lay.blocks:
                return self.block(blk, p.ws, bi, p.ws['x'], p.ws['x2'], p.R, l, cur, p.ws['Lmax'])
            a, h = p.lay.views.get((bi, 'att'), (None, 0)), p.lay.views.get((bi, 'hid'), (None, 0))
            self.block_patched(blk, p.ws, bi, p.ws['x'], p.ws['x2'], p.R, l, cur, p.ws['Lmax'], a[0], a[1], h[0], h[1])

        def head(p, si, cur, l):
            R = p.R
            torch.index_select(ws['lg'][:R * l].view(R, l * V), 0, p.lay.clean, out=lg2[:R * l].view(R, l * V))
            hip.call('token_lens_f32', ws['lg'], lg2, p.gt[:, cur:], L, R, l, V, *[r[:, cur:] for r in res], L)
            if _tap is not None:
                torch.cuda.current_stream().synchronize()
                _tap(ws['lg'][:R * l].clone(), lg2[:R * l].clone(), [(p.i0 + i, s) for i, s in p.lay.rows], (si, cur, l))
        for i0, ni, j0, nj in passes:
            lay = layout(ni, j0, nj)
            img = torch.tensor([i0 + i for i, _ in lay.rows], dtype=torch.int64).to(dev)
            slot = torch.tensor([s for _, s in lay.rows], dtype=torch.int64).to(dev)
            lab = tf.lab[img, (slot < 0).to(torch.int64)].contiguous()            # the donor rows under the donor labels
            self._tf_pass(SimpleNamespace(ws=ws, R=len(lay.rows), lab=lab, i0=i0, lay=lay, gt=gt.index_select(0, img),
                                          xin=tf.xin.index_select(0, img).contiguous()), head=head, block=block)
            keep = slot >= 0
            for k, r in zip(keys, res):
                out[k][img[keep], slot[keep]] = r[:len(lay.rows)][keep]
        return out

    # -- cutting scale-to-scale attention (VAR.attention_knockout) -------------------------------------------------------------------------
    ATTN_KEYSEL_MAX_S = 16             # varhip_attn_keysel_f32 takes at most 16 key scales (include/var_hip.h)

    @torch.no_grad()
    def attention_knockout(self, gt_tokens: torch.Tensor, label_N: torch.Tensor, cuts: tuple, max_rows: int, _tap=None) -> dict:
        """VAR.attention_knockout on the HIP path -> dict(nll, entropy, kl (N, P + 1, L) fp32, pred int64, rank int32), index 0 the clean row.
        gt_tokens (N, L) int64, label_N (N,) int64; cuts: P entries, each {(query scale, block): the H key-scale masks of that block's heads
        while that scale is the query scale} (args.knockout_masks; bit i set = key scale i is visible); all validated by the caller.  The rows
        of a pass are image-major: per image the clean row, then one row per entry.  Images whose rows fit max_rows share passes; otherwise
        an image's entries are chunked over passes, each with its own clean row, as in patch_effects.  Per pass layout (image count, entry
        chunk) one int32 table is built on the host and uploaded: per (scale, block) some row of the layout touches, the [R * H] masks (the
        full mask for the rows that do not).  Those (scale, block) pairs run varhip_adaln_block_keysel_f32, every other one self.block.
        Behind each scale's head the clean row of every row's image is gathered into a second logits buffer and varhip_token_lens_f32
        reduces (row, its clean row): no (rows, L, V) tensor exists at any time, and the tables, the second buffer and the per-pass outputs
        live for the call only.  _tap (tests): called after a stream sync with clones of the scale's logits, of the gathered clean rows, the
        pass's (image, slot) per row (slot 0: the clean row, j + 1: entry j) and (si, cur, l)."""
        var = self.var
        S, H = len(var.patch_nums), var.num_heads

        def refusals(tf):
            if S > self.ATTN_KEYSEL_MAX_S:
                raise ValueError(f'attention_knockout takes at most {self.ATTN_KEYSEL_MAX_S} scales, got {S}')
            self._check_labels(tf.lab)
        tf = self._tf_begin(label_N, gt_tokens, 'attention_knockout runs in f32: the {} workspaces hold 16-bit queries and keys', refusals)
        dev, gt = tf.dev, tf.gt
        L, V = var.L, var.V
        N, P = gt.shape[0], len(cuts)
        keys = ('nll', 'entropy', 'kl', 'pred', 'rank')
        dts = (torch.float32, torch.float32, torch.float32, torch.int64, torch.int32)
        out = {k: torch.empty(N, P + 1, L, dtype=dt, device=dev) for k, dt in zip(keys, dts)}
        if 1 + P <= max_rows:
            ipp, spp = max(1, max_rows // (1 + P)), P                    # whole images per pass
        else:
            ipp, spp = 1, max_rows - 1                                   # one image per pass, its entries in chunks
        passes = [(i0, min(ipp, N - i0), j0, min(spp, P - j0)) for i0 in range(0, N, ipp) for j0 in range(0, P, spp)]
        Rmax = max(ni * (1 + nj) for _, ni, _, nj in passes)
        ws = self._tf_workspace(Rmax)                                    # sized once: a shorter pass uses a prefix
        lg2 = torch.empty(Rmax * var.patch_nums[-1] ** 2, V, dtype=torch.float32, device=dev)
        res = [torch.empty(Rmax, L, dtype=dt, device=dev) for dt in dts]
        ends = [torch.tensor([e for _, e in var.begin_ends[:si + 1]], dtype=torch.int32) for si in range(S)]      # host arrays: the launcher copies them
        layouts = {}

        def layout(ni, j0, nj):
            """the rows of a pass of ni images with the entries j0 .. j0 + nj: (image, slot) per row, each row's clean row, and per touched
            (scale, block) the device view of its [R * H] mask table; built once, one upload"""
            if (ni, j0, nj) not in layouts:
                per = 1 + nj
                rows = [(i, s) for i in range(ni) for s in [0] + list(range(j0 + 1, j0 + nj + 1))]
                tabs = {}
                for j in range(nj):
                    for (si, bi), masks in cuts[j0 + j].items():
                        t = tabs.setdefault((si, bi), [(2 << si) - 1] * (len(rows) * H))
                        for i in range(ni):
                            r = i * per + 1 + j
                            t[r * H:(r + 1) * H] = masks
                flat, where = [], {}
                for key, t in tabs.items():
                    where[key] = len(flat)
                    flat.extend(t)
                table = torch.tensor(flat or [0], dtype=torch.int32).to(dev)
                layouts[(ni, j0, nj)] = SimpleNamespace(rows=rows, views={key: table[o:] for key, o in where.items()},
                                                        clean=torch.tensor([i * per for i, _ in rows], dtype=torch.int64).to(dev))
            return layouts[(ni, j0, nj)]

        def block(p, blk, bi, si, cur, l):
            mask = p.lay.views.get((si, bi))
            if mask is None:
                return self.block(blk, p.ws, bi, p.ws['x'], p.ws['x2'], p.R, l, cur, p.ws['Lmax'])
            self.block_keysel(blk, p.ws, bi, p.ws['x'], p.ws['x2'], p.R, l, cur, p.ws['Lmax'], ends[si], si + 1, mask)

        def head(p, si, cur, l):
            R = p.R
            torch.index_select(ws['lg'][:R * l].view(R, l * V), 0, p.lay.clean, out=lg2[:R * l].view(R, l * V))
            hip.call('token_lens_f32', ws['lg'], lg2, p.gt[:, cur:], L, R, l, V, *[r[:, cur:] for r in res], L)
            if _tap is not None:
                torch.cuda.current_stream().synchronize()
                _tap(ws['lg'][:R * l].clone(), lg2[:R * l].clone(), [(p.i0 + i, s) for i, s in p.lay.rows], (si, cur, l))
        for i0, ni, j0, nj in passes:
            lay = layout(ni, j0, nj)
            img = torch.tensor([i0 + i for i, _ in lay.rows], dtype=torch.int64).to(dev)
            slot = torch.tensor([s for _, s in lay.rows], dtype=torch.int64).to(dev)
            self._tf_pass(SimpleNamespace(ws=ws, R=len(lay.rows), lab=tf.lab[img].contiguous(), i0=i0, lay=lay, gt=gt.index_select(0, img),
                                          xin=tf.xin.index_select(0, img).contiguous()), head=head, block=block)
            for k, r in zip(keys, res):
                out[k][img, slot] = r[:len(lay.rows)]
        return out

    # -- zero-shot classification with per-scale pruning (VAR.classify) -------------------------------------------------------------
    CLASSIFY_MAX_CAND = 16384          # varhip_class_select_f32 stages a stage's totals in LDS

    @torch.no_grad()
    def classify(self, gt_tokens: torch.Tensor, labels: torch.Tensor, cfg: float, max_rows: int, score: tuple, schedule: list):
        """VAR.classify on the HIP path -> (pred (N,) int64, total (N, K) float64, depth (N, K) int64, tokens (N, K, L) fp32).
        schedule: [(scale, m), ...] ascending, each m below the survivor count before it (validated by the caller).  One stage per boundary and a
        final stage through the last scale.  A stage rebuilds its rows' KV caches from scale 0 (the caches of the previous stage are not kept
        or compacted), scores only the scales no earlier stage scored into a compact (N, m_j, L_e) buffer, which is scattered into `tokens`;
        varhip_class_select_f32 then adds those tokens to the survivors' float64 totals and keeps each image's best m (keep 1 after the final
        stage: pred).  Survivor positions stay on the device: the pass counts follow from the schedule alone, nothing waits for the host.
        A stage ending at scale e packs max_rows * min(L // L_e, l_max // l_e) rows per pass, so no buffer outgrows a full pass's.
        self.classify_work: [(e_j, m_j, N * m_j * L_e_j), ...] the class row-tokens the transformer ran per stage (unconditional rows excluded)."""
        var = self.var
        N, K = labels.shape
        if K > self.CLASSIFY_MAX_CAND:
            raise ValueError(f'classify takes at most {self.CLASSIFY_MAX_CAND} candidates per image on the HIP path, got {K}')
        sc = self._score_setup(gt_tokens, labels, cfg, dist=score[0] in _DIST_SCORES)
        dev = sc.dev
        L, S = var.L, len(var.patch_nums)
        lmax = max(p * p for p in var.patch_nums)
        ends = [e for _, e in var.begin_ends]
        img = torch.arange(N, device=dev).view(N, 1)
        tokens = torch.full((N, K, L), float('nan'), dtype=torch.float32, device=dev)
        total = torch.empty(N, K, dtype=torch.float64, device=dev)
        depth = torch.empty(N, K, dtype=torch.int64, device=dev)
        pos = torch.arange(K, device=dev).expand(N, K).contiguous()         # the stage's candidates, ascending positions per image
        tot = torch.full((N, K), -0.0, dtype=torch.float64, device=dev)      # their running totals (-0.0 + x == x for every x)
        work, done, m = [], -1, K
        for last, keep in list(schedule) + [(S - 1, 1)]:
            Le, t0 = ends[last], ends[done] if done >= 0 else 0
            rows = max_rows * min(L // Le, lmax // var.patch_nums[last] ** 2)
            buf = torch.empty(N, m, Le, dtype=torch.float32, device=dev)
            self._score_stage(sc, sc.lab.gather(1, pos), last, done, rows, self._token_reducer(sc, score, buf))
            tokens[img, pos, t0:Le] = buf[:, :, t0:]
            nk = min(keep, m)
            kept = torch.empty(N, nk, dtype=torch.int32, device=dev)
            hip.call('class_select_f32', buf, m * Le, Le, N, m, t0, Le, tot, keep, kept)
            total[img, pos] = tot
            depth[img, pos] = last
            work.append((last, m, N * m * Le))
            kept = kept.long()
            pos, tot, done, m = pos.gather(1, kept), tot.gather(1, kept), last, nk
        self.classify_work = work
        return pos[:, 0], total, depth, tokens

    @torch.no_grad()
    def classify_generative(self, img: torch.Tensor, labels: torch.Tensor, last_kept: int, feature, cfg: float, max_rows: int,
                            match_input_range: bool):
        """VAR.classify_generative on the HIP path (eval_prob.py:466-516, `--mode gen`): -> (score (N, K) fp32, tokens (N, K, L) int64).
        The image side runs once per image: encode -> quantize -> tokens, and the image's feature.  The N * K (image, class) rows then run in
        passes of at most max_rows rows, packed across images in row-major (image, position) order; per pass:
          sample(greedy=True, the image's tokens kept through scale last_kept, decode=False) -> decode_nhwc -> the feature -> feature_l1_f32.
        Every stage is row-independent, so the results do not depend on the packing.  self.generative_ms: per-stage milliseconds of the last
        call when self.profile_generative is set (a synchronising event pair around each stage)."""
        var = self.var
        vae = var.vae_proxy[0]
        prec = self.resolve_precision()
        enc, qe = vae._encoder_engine(), var.vae_quant_proxy[0].hip_engine()
        eprec = prec if prec != 'f32' else None
        pns = tuple(var.patch_nums)
        N, K = labels.shape
        dev = var.lvl_1L.device
        prof = getattr(self, 'profile_generative', False)
        ms = dict(image=0.0, ar=0.0, decode=0.0, encode=0.0, quantize=0.0, distance=0.0)

        def stage(name, fn):
            if not prof:
                return fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); out = fn(); e1.record(); e1.synchronize()
            ms[name] += e0.elapsed_time(e1)
            return out

        def feat_of(x):                            # (rows, D) fp32 view of the feature of images x, and its token ids when wanted
            if callable(feature):
                f = feature(x)
                return f.reshape(f.shape[0], -1).float().contiguous(), None
            f = stage('encode', lambda: enc.encode(x, precision=eprec))
            if feature == 'vae_fhat':
                f = stage('quantize', lambda: qe.quantize(f, True, pns)[-1])
            return f.reshape(f.shape[0], -1), f

        def image_side(i0, i1):
            img_d = img[i0:i1].to(dev, torch.float32).contiguous()
            f_img = enc.encode(img_d, precision=eprec)
            idx, fh = qe.quantize(f_img, False, pns, last_fhat=True)              # tokens (vae.img_to_idxBl) and img_to_fhat(...)[-1]
            if callable(feature):
                fin = feature(img_d)
                fin = fin.reshape(i1 - i0, -1).float().contiguous()
            elif feature == 'vae_fhat':
                fin = fh.reshape(i1 - i0, -1)
            else:
                fin = f_img.reshape(i1 - i0, -1)
            return torch.cat(idx, dim=1), fin

        # the image side in chunks of at most max_rows images: its activations are bounded like a pass's
        parts = [stage('image', lambda i0=i0: image_side(i0, min(i0 + max_rows, N))) for i0 in range(0, N, max_rows)]
        gt = torch.cat([p[0] for p in parts]) if len(parts) > 1 else parts[0][0]
        fin = torch.cat([p[1] for p in parts]) if len(parts) > 1 else parts[0][1]
        del parts
        lab = labels.to(dev, torch.int64).reshape(-1)
        keep_n = var.begin_ends[last_kept][1]                                     # cumsum(pn^2)[c]: the kept prefix
        score = torch.empty(N * K, dtype=torch.float32, device=dev)
        tokens = torch.empty(N * K, var.L, dtype=torch.int64, device=dev)
        row_img = torch.arange(N, device=dev).repeat_interleave(K)
        # every pass runs the AR loop on RP rows, so all passes share one workspace; a shorter last pass is padded with copies of its last row
        # (rows are independent: the copies change nothing and are dropped)
        RP = min(max_rows, N * K)
        keep = torch.zeros(RP, var.L, dtype=torch.bool, device=dev)
        keep[:, :keep_n] = True
        tok_pass = torch.empty(RP, var.L, dtype=torch.int64, device=dev)
        for q0 in range(0, N * K, max_rows):
            q1 = min(q0 + max_rows, N * K)
            R = q1 - q0
            ri = row_img[q0:q1]
            rows = torch.arange(q0, q0 + RP, device=dev).clamp_(max=q1 - 1)
            stage('ar', lambda: self.sample(RP, lab[rows], None, cfg, 1, 0.0, decode=False, gt_tokens=gt[row_img[rows]], keep_mask=keep,
                                            greedy=True, tokens_out=tok_pass))
            tokens[q0:q1] = tok_pass[:R]
            f_hat = self.workspace(RP)['f_hat'][:R]
            rec = stage('decode', lambda: self.dec.decode_nhwc(f_hat, denorm=not match_input_range, precision=prec))
            frec, _ = feat_of(rec)
            if frec.shape[1] != fin.shape[1]:
                raise ValueError(f'the feature of the reconstructions has {frec.shape[1]} elements per image, that of the input {fin.shape[1]}')
            stage('distance', lambda: hip.call('feature_l1_f32', fin, frec, ri.contiguous(), R, fin.shape[1], score[q0:q1]))
        self.generative_ms = ms if prof else None
        return score.view(N, K), tokens.view(N, K, var.L)

    def code_distance_table(self) -> torch.Tensor:
        """(V, V) fp32 L2 distances between codebook vectors in the direct form of neighbor_table (one fma chain over the channels, then
        sqrt; not cdist's |a|^2 + |b|^2 - 2ab): entry (v, u) equals neighbor_table's distance for the pair bit for bit.  64 MiB at V = 4096;
        cached next to the neighbour tables until the codebook changes."""
        self.refresh()
        if 'code_dist' not in self.w:
            cb = self.w['codebook']
            V, D = cb.shape
            dist = torch.empty(V, V, dtype=torch.float32, device=cb.device)
            self._wait_ready()
            hip.call('code_dist_f32', cb, V, D, dist)
            self.w['code_dist'] = dist
            self._built()
        return self.w['code_dist']

    # -- model arithmetic (for bench.py's roofline) -------------------------------------------------------------------
    def flops_per_image(self) -> float:
        """Algorithmic FLOPs of one image (2 per MAC, both CFG branches), SURVEY.md §8(d) formula; ada_lin hoisted."""
        var = self.var
        C, depth, V = var.C, var.depth, var.V
        L = var.L
        T = 2 * L
        sig = 0; cur = 0
        for pn in var.patch_nums:
            cur += pn * pn; sig += pn * pn * cur
        lin = 2 * 12 * C * C * depth * T
        att = 2 * 2 * sig * C * depth * 2
        head = 2 * C * V * T
        ada = 2 * 2 * depth * 6 * C * C
        return float(lin + att + head + ada)
