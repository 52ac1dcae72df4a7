"""The host side of the engines, pinned launch by launch without a GPU.

var_amd/engine.py decides which `hip.call` runs with which arguments; the kernels decide everything else.  So two versions of engine.py
compute the same thing if every entry point issues the same launches, with the same scalar arguments, over the same dataflow between
buffers.  This module records exactly that on CPU tensors and compares it with tests/golden/launch_trace.json.

What is patched (and nothing else): `hip.call` records instead of launching; `engine._chk` keeps its dtype test and drops `is_cuda`; the
`_built` / `_wait_ready` stream handshake is a no-op (tests/test_call_order_gpu.py pins it on the GPU); `torch.cuda.current_stream()` is
stream 0.  The shape helpers of the library (`hip.conv_gn_blocks`, `hip.conv16_gn_fusable`, `hip.gn_scratch_elems`) are the real host
functions: they choose the paths.

Per launch the record holds the entry point's name and every argument in order: None, ints, floats as `float.hex`, host arrays by content,
tensors as (dtype, shape, stride, storage offset, buffer number).  A buffer number is the order in which that storage first appeared in the
case; the recorder keeps every tensor it saw alive until the case ends, so no address comes back under another tensor and the numbers are
the dataflow.  The host arrays of device pointers that `kv_compact` and `kv_resample` take are recorded as the buffer numbers of the storages
they point to (the workspaces that own them live in the engine's caches), so the dataflow across a prune or resampling boundary is part of
the record.  What the entry point returns is recorded the same way.  The tensors are real CPU tensors: `_stats_from` compares
`data_ptr()`s, and that comparison runs for real.

The one place where the host branches on a kernel's output is `edit_keep_u8` -> `skip`: the recorder fills that output (the first
KEEP_PREFIX tokens of every row kept), and two cases cover a fully kept first scale and no kept token.  Two more outputs become indices
on the host, and the recorder fills them as well: `class_select_f32` leaves kept[i] = 0 .. keep-1 (every image keeps its first candidates),
`smc_resample_f32` leaves the identity ancestor table and did = 0 (nothing is resampled; `kv_resample` still runs, and its count of refused
rows stays 0).  The `smc_reference` route of sample_smc goes through `hip.call_host` and real NumPy: tests/test_smc_gpu.py holds it.

The fixture stores, per case, one line per launch ("name digest-of-its-arguments") and the SHA-256 of the whole record: a failure names the
first launch that differs.  `python tests/test_launch_trace_cpu.py --write PATH` writes it.  It only drives entry points that keep their
signature (decode_nhwc, encode, the SamplingEngine and QuantizerEngine methods), so the same file records any revision of engine.py;
every case of tests/golden/launch_trace.json is the record of the revision that first had it: the revision before the engines' fp32 /
16-bit paths were folded into one walk each, for the stats, best-of and particle cases the one before the samplers shared one scale walk, and for the token_scores, distance_profile,
class_information, attention_profile, classify, code_tokens and decode_tokens cases the one before the teacher-forced calls shared one pass
walk (2f8fb50)."""
import contextlib
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from var_amd import engine, hip                                             # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'launch_trace.json')
HOST_ARRAYS = {('edit_keep_u8', 4), ('eval_reduce_f32', 6), ('attn_profile_f32', 7)}    # tensor arguments the launcher reads on the host: recorded by content
POINTER_ARRAYS = {('kv_compact', 0), ('kv_compact', 1), ('kv_resample', 0)}    # host arrays of device addresses: recorded as the buffers they point to
ADA_ATTR = 'ADA_PACKED_MAX_BYTES'                                           # SamplingEngine: above it the per-block AdaLN projections replace the packed one

# every entry point named in a hip.call of _VaeOps, DecoderEngine, EncoderEngine, of SamplingEngine's prologue, block() and head(), and of
# the per-image, stats, best-of and particle routes of its sampling walk, of its teacher-forced calls and of the token coder: the cases
# below must reach all of them
MUST_REACH = {
    'word_embed_f32', 'token_loglik_f32', 'token_score_f32', 'token_eval_f32', 'eval_reduce_f32', 'code_dist_f32', 'dist_profile_f32', 'class_mix_f32',
    'class_mix_finish_f32', 'attn_profile_f32', 'code_table_f32', 'rans_decode_u32',
    'conv3x3_nhwc_f32', 'conv3x3_gn_nhwc_f32', 'conv3x3_wino_nhwc_f32', 'conv3x3_s2_nhwc_f32', 'gn_stats_f32', 'gn_stats_part_f32', 'gn_apply_f32',
    'gn_silu_conv_out_f32', 'gemm_nt_f32', 'softmax_rows_f32', 'upconv_phase_f32', 'upconv_phase_gn_f32', 'nchw_to_nhwc_pad_f32', 'gn_scale_shift_f32',
    'lvl_pos_f32', 'first_map_f32', 'silu_f32', 'add_bcast_f32', 'adaln_block_f32', 'ln_modulate_f32',
    'exp1_philox_f32', 'cfg_sample_rows_f32', 'sample_stats_f32', 'class_select_f32', 'kv_compact', 'kv_resample', 'smc_resample_f32', 'quant_accum_f32',
    'next_map_f32',
} | {n + s for s in ('f16', 'bf16') for n in ('conv3x3_nhwc_', 'gn_stats_', 'gn_apply_', 'gn_silu_conv_out_', 'gnconv3x3_nhwc_', 'gemm_nt_', 'upconv_phase_',
                                                'conv3x3_s2_nhwc_', 'cast_f32_to_', 'adaln_block_')} \
  | {'cast_f16_to_f32', 'cast_bf16_to_f32', 'ln_modulate_f16out', 'ln_modulate_bf16out'}


class Recorder:
    KEEP_PREFIX = 0          # edit_keep_u8's stand-in: this many leading tokens of every row are kept

    def __init__(self):
        self.alive, self.bufs, self.log = [], {}, []

    def tensor(self, t):
        self.alive.append(t)
        n = self.bufs.setdefault(t.untyped_storage().data_ptr(), len(self.bufs))
        return ['T', str(t.dtype), list(t.shape), list(t.stride()), int(t.storage_offset()), n]

    def value(self, a, host=False, pointers=False):
        if a is None or isinstance(a, str):
            return a
        if pointers:
            return ['pointers', [self.bufs.setdefault(p, len(self.bufs)) for p in a.tolist()]]
        if isinstance(a, torch.Tensor):
            return ['host', str(a.dtype), a.tolist()] if host else self.tensor(a)
        if isinstance(a, np.ndarray):
            return ['host', str(a.dtype), a.tolist()]
        if isinstance(a, (bool, int, np.integer)):
            return int(a)
        if isinstance(a, (float, np.floating)):
            return float(a).hex()
        if isinstance(a, dict):
            return {k: self.value(v) for k, v in a.items()}
        if isinstance(a, (list, tuple)):
            return [self.value(v) for v in a]
        raise TypeError(f'launch argument of type {type(a)}')

    def call(self, name, *args, stream=None):
        assert stream is None
        self.log.append([name] + [self.value(a, (name, i) in HOST_ARRAYS, (name, i) in POINTER_ARRAYS) for i, a in enumerate(args)])
        if name == 'edit_keep_u8':
            args[-1].zero_()
            args[-1][:, :self.KEEP_PREFIX] = 1
        if name == 'class_select_f32':                           # kept (images, keep)
            args[-1][:] = torch.arange(args[-1].shape[1], dtype=args[-1].dtype)
        if name == 'smc_resample_f32':                           # ..., anc (images, n), did (images,), ess, seen
            args[-4][:] = torch.arange(args[-4].shape[1], dtype=args[-4].dtype)
            args[-3].zero_()

    def returned(self, out):
        self.log.append(['return', self.value(out)])


@contextlib.contextmanager
def patched(rec):
    nop = lambda self: None
    def chk(t, name):
        if t.dtype != torch.float32:
            raise hip.VarHipError(f'{name}: fp32 parameters only')
        return t if t.is_contiguous() else t.contiguous()
    todo = [(hip, 'call', rec.call), (engine, '_chk', chk), (torch.cuda, 'current_stream', lambda *a: SimpleNamespace(cuda_stream=0))]
    for cls in vars(engine).values():
        if isinstance(cls, type):
            todo += [(cls, m, nop) for m in ('_built', '_wait_ready') if m in vars(cls)]
    saved = [(o, n, getattr(o, n)) for o, n, _ in todo]
    try:
        for o, n, v in todo:
            setattr(o, n, v)
        yield
    finally:
        for o, n, v in saved:
            setattr(o, n, v)


def record(fn, keep_prefix=0):
    rec = Recorder()
    rec.KEEP_PREFIX = keep_prefix
    with patched(rec), torch.no_grad():
        rec.returned(fn())
    return rec.log


def summarise(log):
    lines = [f'{e[0]} {hashlib.sha256(json.dumps(e[1:], sort_keys=True).encode()).hexdigest()[:8]}' for e in log]
    return dict(launches=lines, sha256=hashlib.sha256(json.dumps(log, sort_keys=True).encode()).hexdigest())


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _vae(ch, pns):
    from var_amd.models.vqvae import VQVAE
    return VQVAE(vocab_size=64, z_channels=32, ch=ch, v_patch_nums=pns)


def _switched(eng, name, value, fn):
    old = getattr(eng, name)
    setattr(eng, name, value)
    try:
        return fn()
    finally:
        setattr(eng, name, old)


def smallest_fused_shape(ch=160):
    """the smallest (B, P) at which the 16-bit decoder runs at least one ResnetBlock conv with its GroupNorm fused in (gnconv3x3_nhwc_*):
    asked of the library's own host function, level by level (a decode at P has maps of side P, 2P, .. 16P with 4ch, 4ch, 2ch, 2ch, ch, ch
    channels around its ResnetBlock convs)"""
    widths = [(1, 4 * ch, 4 * ch), (2, 4 * ch, 4 * ch), (4, 4 * ch, 2 * ch), (4, 2 * ch, 2 * ch), (8, 2 * ch, 2 * ch), (16, 2 * ch, ch), (16, ch, ch)]
    for P in (1, 2, 3, 4, 6, 8, 12, 16):
        for B in (1, 2):
            if any(hip.conv16_gn_fusable(B, m * P, m * P, ci, co) for m, ci, co in widths):
                return B, P
    return 1, 16


def vae_cases():
    out = {}
    vae = _vae(32, (1, 2, 4))
    dec, enc, qe = vae._decoder_engine(), vae._encoder_engine(), vae.quantize.hip_engine()
    f = lambda B, P: torch.zeros(B, P, P, 32)
    for prec in ('f32', 'f16', 'bf16'):
        for P in (4, 2):
            for denorm in (True, False):
                out[f'ch32 decode {prec} P{P} denorm{int(denorm)}'] = record(lambda: dec.decode_nhwc(f(2, P), denorm=denorm, precision=prec))
        out[f'ch32 decode {prec} P4 unfused_tail'] = record(lambda: _switched(dec, 'unfused_tail', True, lambda: dec.decode_nhwc(f(2, 4), precision=prec)))
        out[f'ch32 decode {prec} P4 no winograd'] = record(lambda: _switched(dec, 'winograd', False, lambda: dec.decode_nhwc(f(2, 4), precision=prec)))
        out[f'ch32 decode {prec} P4 no fuse_gn'] = record(lambda: _switched(dec, 'fuse_gn', False, lambda: dec.decode_nhwc(f(2, 4), precision=prec)))
        out[f'ch32 encode {prec}'] = record(lambda: enc.encode(torch.zeros(2, 3, 64, 64), precision=prec))
    out['ch32 decode f32 P4 no clamp'] = record(lambda: dec.decode_nhwc(f(2, 4), precision='f32', clamp=False))
    out['ch32 decode default precision'] = record(lambda: dec.decode_nhwc(f(2, 4)))
    out['ch32 encode default precision'] = record(lambda: enc.encode(torch.zeros(2, 3, 64, 64)))

    # the quantizer engine's own entry points (their tables are built by the code the sampling engine shares)
    pns = (1, 2, 4)
    toks = [torch.zeros(2, pn * pn, dtype=torch.int64) for pn in pns]
    out['quantize idx'] = record(lambda: qe.quantize(f(2, 4), False, pns))
    out['quantize fhat'] = record(lambda: qe.quantize(f(2, 4), True, pns))
    out['quantize last_fhat'] = record(lambda: qe.quantize(f(2, 4), False, pns, last_fhat=True))
    out['quantize_stats'] = record(lambda: qe.quantize_stats(f(2, 4), pns, 0.25))
    out['fhat_from_scales tokens'] = record(lambda: qe.fhat_from_scales(toks, pns, True, True))
    out['fhat_from_scales maps'] = record(lambda: qe.fhat_from_scales([torch.zeros(2, 32, pn, pn) for pn in pns], pns, False, False))
    out['var_input'] = record(lambda: qe.var_input(toks, pns))

    vae = _vae(160, (1, 2, 8))
    dec, enc = vae._decoder_engine(), vae._encoder_engine()
    for prec in ('f32', 'f16'):
        for P in (1, 2, 8):
            out[f'ch160 decode {prec} P{P}'] = record(lambda: dec.decode_nhwc(f(1, P), precision=prec))
        for side in (32, 64):
            out[f'ch160 encode {prec} {side}'] = record(lambda: enc.encode(torch.zeros(1, 3, side, side), precision=prec))
    B, P = smallest_fused_shape()
    for prec in ('f16', 'bf16'):
        out[f'ch160 decode {prec} fused GroupNorm'] = record(lambda: dec.decode_nhwc(f(B, P), precision=prec))
    return out


def _per_block_adaln(eng):
    """a revision of SamplingEngine without the named threshold: the same weight table the threshold at 0 gives (every block's own ada_lin
    parameters, no packed copy)"""
    with patched(Recorder()):
        eng.refresh()
    if 'ada_w_all' in eng.w:
        del eng.w['ada_w_all'], eng.w['ada_b_all']
        for d, b in zip(eng.w['blocks'], eng.var.blocks):
            d['ada_w'], d['ada_b'] = b.ada_lin[1].weight.detach(), b.ada_lin[1].bias.detach()


def sampling_cases():
    import contextlib as cl
    import io
    from var_amd.models import build_vae_var
    out = {}
    pns = (1, 2, 3)
    L = sum(p * p for p in pns)
    lab = torch.tensor([3, 7])
    gt = (torch.arange(2 * L).view(2, L) * 37) % 4096
    rng = lambda: torch.Generator().manual_seed(0)

    def build(**kw):
        with cl.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=pns, depth=2, ch=32, **kw)
        return var.eval()

    var = build()
    eng = var.engine()
    plain = lambda **kw: eng.sample(2, lab, rng(), 1.5, 900, 0.96, **kw)
    for prec in ('f32', 'bf16', 'f16'):
        eng.set_precision(prec)
        out[f'sample {prec}'] = record(plain)
        out[f'teacher_forced_logits {prec}'] = record(lambda: eng.teacher_forced_logits(lab, torch.zeros(2, L - 1, 32)))
    eng.set_precision('f32')
    out['sample more_smooth'] = record(lambda: plain(more_smooth=True))
    out['sample trace'] = record(lambda: (plain(trace=True), eng.last_trace))
    keep = torch.zeros(2, L, dtype=torch.bool)
    keep[:, :1] = True
    keep[0, 2] = True
    out['sample greedy inpainting'] = record(lambda: plain(greedy=True, gt_tokens=gt, keep_mask=keep, tokens_out=torch.empty(2, L, dtype=torch.int64)))
    out['sample inpainting'] = record(lambda: plain(gt_tokens=gt, keep_mask=keep))
    edit = dict(tokens=gt, mask=torch.zeros(1, 6, 6))
    out['sample edit first scale kept'] = record(lambda: plain(edit=edit, tokens_out=torch.empty(2, L, dtype=torch.int64)), keep_prefix=1)
    out['sample edit nothing kept'] = record(lambda: plain(edit=edit), keep_prefix=0)
    out['sample edit more_smooth first scale kept'] = record(lambda: plain(edit=edit, more_smooth=True), keep_prefix=1)
    out['sample_per_image'] = record(lambda: eng.sample_per_image(lab, [1, 2], [1.5, 2.0], [900, 0], [0.96, 0.0]))
    out['sample_per_image more_smooth'] = record(lambda: eng.sample_per_image(lab, [1, 2], [1.5, 2.0], [900, 0], [0.96, 0.0], more_smooth=True))
    out['sample smooth'] = record(lambda: (plain(smooth=dict(gt=gt, n=4, thr=None)), eng.last_smooth))
    out['sample decode=False'] = record(lambda: plain(decode=False))
    def scored(fn, **kw):                                        # the call's result and what it left in the caller's stats dict and tensors
        kw['stats'] = {}
        return fn(**kw), kw
    out['sample stats'] = record(lambda: scored(plain))
    out['sample stats more_smooth'] = record(lambda: scored(plain, more_smooth=True))
    out['sample_per_image stats decode=False'] = record(lambda: scored(
        lambda **kw: eng.sample_per_image(lab, [1, 2], [1.5, 2.0], [900, 0], [0.96, 0.0], **kw), decode=False, tokens_out=torch.empty(2, L, dtype=torch.int64)))
    # two candidates / particles per image: labels, seeds and parameters spread to N = 4 rows as the VAR methods hand them over
    lab4 = lab.repeat_interleave(2)
    cand = ([11, 12, 21, 22], [1.5, 1.5, 2.0, 2.0], [900, 900, 0, 0], [0.96, 0.96, 0.0, 0.0])
    out['sample_best_of two chunks'] = record(lambda: eng.sample_best_of(lab4, *cand, 2, 'logp_cond', 2))
    for name, max_images in (('one chunk', 4), ('two chunks', 2)):
        out[f'sample_best_of_pruned {name}'] = record(
            lambda: (eng.sample_best_of_pruned(lab4, *cand, 2, 'logp_cond', [(0, 1)], max_images), eng.best_of_work))
        out[f'sample_smc {name}'] = record(lambda: (eng.sample_smc(lab4, *cand, 2, 'logp_cond', [0, 1], 1.0, 0.5, [5, 6], max_images), eng.smc_work))
    labels = torch.tensor([[1, 2, 3], [4, 5, 6]])
    out['token_log_likelihood cfg'] = record(lambda: eng.token_log_likelihood(gt, labels, 1.5, 4))
    out['token_log_likelihood no cfg'] = record(lambda: eng.token_log_likelihood(gt, labels, 0.0, 8))
    out['token_scores neighbor_max'] = record(lambda: eng.token_scores(gt, labels, 1.5, 4, ('neighbor_max', 0.5)))
    out['evaluate'] = record(lambda: eng.evaluate(gt, lab, 2))
    out['evaluate one row per pass'] = record(lambda: eng.evaluate(gt, lab, 1))
    # the rest of the teacher-forced family, on both packings (whole images per pass | one image per pass, its classes in chunks)
    S = len(pns)
    out['token_scores group_smoothed'] = record(lambda: eng.token_scores(gt, labels, 0.0, 4, ('group_smoothed', 50)))
    out['token_scores expected_distance chunked'] = record(lambda: eng.token_scores(gt, labels, 1.5, 2, ('expected_distance', 8)))
    edges = torch.tensor([0.0, 0.5, 1.0, float('inf')])
    out['distance_profile cfg chunked'] = record(lambda: eng.distance_profile(gt, labels, 1.5, 3, edges, 1e-4))
    out['distance_profile no cfg'] = record(lambda: eng.distance_profile(gt, labels, 0.0, 8, edges, 1e-4))
    prior = torch.full((2, 3), 1 / 3)
    out['class_information'] = record(lambda: eng.class_information(gt, labels, 1.5, 8, prior))
    out['class_information chunked'] = record(lambda: eng.class_information(gt, labels, 1.5, 3, prior))
    out['class_information V above the LDS limit'] = record(
        lambda: _switched(eng, 'CLASS_MIX_LDS_V', 1024, lambda: eng.class_information(gt, labels, 1.5, 8, prior)))
    out['attention_profile tokens'] = record(lambda: eng.attention_profile(gt, lab, 1, (0, 1), 1, return_tokens=True))
    out['attention_profile'] = record(lambda: eng.attention_profile(gt, lab, 0, (1,), 2))
    out['classify pruned'] = record(lambda: (eng.classify(gt, labels, 1.5, 2, ('log_prob',), [(0, 2)]), eng.classify_work))
    out['classify neighbor_max'] = record(lambda: eng.classify(gt, labels, 0.0, 4, ('neighbor_max', 0.5), []))
    # the sampling walk's two newest users
    out['code_tokens'] = record(lambda: eng.code_tokens(gt, lab, 1.5, S - 1))
    out['code_tokens last=1'] = record(lambda: eng.code_tokens(gt, lab, 1.5, 1))
    coded = (np.zeros(8, np.uint32), np.array([0, 4], np.int64), np.array([4, 4], np.int64))
    out['decode_tokens'] = record(lambda: eng.decode_tokens(*coded, lab, 1.5, 1, None, False))
    out['decode_tokens fill decode'] = record(lambda: eng.decode_tokens(*coded, lab, 1.5, 1, 1.5, True))

    # the per-block AdaLN projections: a fresh model whose engine packs nothing
    var = build()
    eng = var.engine()
    if hasattr(type(eng), ADA_ATTR):
        setattr(eng, ADA_ATTR, 0)
    else:
        _per_block_adaln(eng)
    out['sample per-block adaln'] = record(plain)
    out['teacher_forced_logits per-block adaln'] = record(lambda: eng.teacher_forced_logits(lab, torch.zeros(2, L - 1, 32)))
    assert 'ada_w' in eng.w['blocks'][0] and 'ada_w_all' not in eng.w

    var = build(shared_aln=True)
    eng = var.engine()
    out['sample shared_aln'] = record(plain)
    out['teacher_forced_logits shared_aln'] = record(lambda: eng.teacher_forced_logits(lab, torch.zeros(2, L - 1, 32)))
    return out


def all_cases():
    out = vae_cases()
    out.update(sampling_cases())
    return {k: summarise(v) for k, v in out.items()}


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def traces():
    return all_cases()


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_same_cases(traces, golden):
    assert sorted(traces) == sorted(golden)


def test_every_engine_entry_point_is_reached(traces):
    seen = {line.split()[0] for t in traces.values() for line in t['launches']}
    assert not MUST_REACH - seen, f'no case launches {sorted(MUST_REACH - seen)}'


def test_edit_cases_take_both_branches(traces):
    """a fully kept scale runs no head: fewer ln_modulate launches than the case that keeps nothing"""
    heads = lambda k: sum(line.startswith('ln_modulate_f32 ') for line in traces[k]['launches'])
    assert heads('sample edit first scale kept') == heads('sample edit nothing kept') - 1 == 2


def test_launches_identical(traces, golden):
    bad = []
    for case in sorted(golden):
        got, want = traces[case]['launches'], golden[case]['launches']
        if got == want and traces[case]['sha256'] == golden[case]['sha256']:
            continue
        i = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        bad.append(f'{case}: launch {i} of {len(want)} (now {len(got)}): recorded {want[i] if i < len(want) else "<end>"!r}, '
                   f'now {got[i] if i < len(got) else "<end>"!r}; before it: {want[max(0, i - 3):i]}')
    assert not bad, '\n'.join(bad)


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--write', 'usage: test_launch_trace_cpu.py --write PATH'
    res = all_cases()
    seen = {line.split()[0] for t in res.values() for line in t['launches']}
    assert not MUST_REACH - seen, f'no case launches {sorted(MUST_REACH - seen)}'
    with open(sys.argv[2], 'w') as fh:
        json.dump(res, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print(len(res), 'cases,', sum(len(t['launches']) for t in res.values()), 'launches,', len(sorted(seen)), 'entry points')
