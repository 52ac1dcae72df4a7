"""The argument handling of VAR's public calls, pinned case by case: one case table and one recorder, shared by tests/test_front_end_cpu.py (a
CPU model) and tests/test_front_end_gpu.py (a GPU model; no kernel is launched).

A case is a public call with its arguments.  The engine is replaced per case by `var.engine = lambda: stub` (an instance attribute); every
method of the stub records (name, args, kwargs) and raises Reached.  Nothing else is patched, so the record is what the front end alone
decides: either it refuses the arguments, or it hands them to the engine, or (a CPU model, the scoring family) it runs the PyTorch path to
the end.  The outcome of a case is one of
  ["raise", exception type name, str(exception)]
  ["engine", method, args, kwargs]
  ["return", value]
with values recorded as: None, bools, ints and strs as they are (numpy scalars as their Python value), floats as float.hex, lists / tuples /
dicts recursively, numpy arrays and tensors as [dtype, shape, device type, content as a list] (above 256 elements the SHA-256 of the bytes), a torch.Generator as ["rng", initial_seed()],
result objects as [class name, {field: value}].  The content of the `tokens_out` buffer (torch.empty) is not recorded.  What a call returns is
recorded the same way; a returned tensor above 64 elements by its SHA-256 if it is an exact integer result and by its float64 sum otherwise.
Returned floats, and the fixed-point fields named in FIXED_POINT, are compared within RTOL / ATOL (see there); everything else exactly.  torch's global
generators are seeded before every case, so a label drawn "unseeded" is a recorded value too: with label None the record shows which
generator the labels came from and whether self.rng was seeded before the draw.

tests/golden/front_end.json holds the outcomes of the revision before the checkers moved to var_amd/models/args.py, for a CPU model and
for a model on an MI355X, per call one line per outcome: [where ("cpu", "gpu" or "both"), outcome, the arguments that end in it].  `python tests/frontcases.py --write PATH` writes the section of the device it finds (and keeps the other);
it also prints the `raise` lines of the argument handling in var_amd/models/var.py and args.py that no case reached.
`python tests/frontcases.py --check-parent`, run on that revision, compares it with the fixture and UNIFIED's first column.

UNIFIED (tests/golden/front_end_unified.json) lists every case whose outcome differs from that revision, per section {case: (outcome then,
outcome now)}; such a case is not in the fixture.
Three rules cover all of them: (1) an exception of a stray type or with an interpreter's message (int('a'), float(None), .to on a numpy scalar)
became ValueError with the argument's own message; (2) a Python bool is refused as a count or parameter; (3) a numpy integer is a label
wherever a Python int is."""
import ast
import contextlib
import hashlib
import io
import json
import os
import re
import sys
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'front_end.json')
PNS, DEPTH, V, NUM_CLASSES = (1, 2, 3), 2, 4096, 1000
L, S = sum(p * p for p in PNS), len(PNS)
SEED = 20240                       # torch's global generators, before every case
MODULE_FUNCTIONS = ('normalize_keep', 'normalize_resample')
# What a CPU call returns through the PyTorch path is fp32 arithmetic whose last bits depend on the host's BLAS and vector units.  Returned
# floats are compared within RTOL of the larger magnitude plus ATOL: a depth-2 model with reductions over at most 512 terms loses a few hundred
# units of 2^-24 (3e-5 of the logits' magnitude, which is O(1)); 1e-4 / 1e-5 holds that and is four orders below what a dropped or altered cfg,
# max_rows, group, threshold, top_k or label does to a result.  Every returned integer is compared exactly, except the result fields that are
# fixed-point images of such floats, {(class, field): the integer that stands for 1.0}: those are compared as floats after division by it
# (and the ranks, below).
RTOL, ATOL = 1e-4, 1e-5
# EvalResult.rank_BL counts the codes whose logit lies above the token's: it moves by the number of codes whose logit is within that tolerance
# of the token's.  The deck's logits rows have a standard deviation of about 3 over V = 4096 codes, at most V / (3 sqrt(2 pi)) = 545 codes per
# unit; the tolerance at the largest logit (13) is 1.3e-3 either way: 1.4 codes expected, 6 with four standard deviations of that count.
RANK_SLACK = 6
_ZEROS = re.compile(r'0+p')
FIXED_POINT = {('DistanceProfile', 'mass_q_NKSB'): 2.0 ** 48, ('AttentionProfile', 'share_q'): 2.0 ** 21, ('AttentionProfile', 'tokens'): 2.0 ** 21,
               ('EvidenceMaps', 'overlays'): 255.0, ('EvalResult', 'rank_BL'): 'rank'}

def pack(sections):
    """{section: {'call: arguments': outcome}} -> {call: [[where, outcome, [arguments, ...]], ...]}: the cases of a call that share an outcome stand
    together, where = 'both' if the CPU and the GPU model agree on it"""
    out = {}
    for name in sorted(set().union(*sections.values())):
        call, tag = name.split(': ', 1)
        have = [(sec, sections[sec][name]) for sec in sorted(sections) if name in sections[sec]]
        if len(have) == 2 and have[0][1] == have[1][1]:
            have = [('both', have[0][1])]
        for where, outcome in have:
            groups = out.setdefault(call, [])
            hit = next((g for g in groups if g[0] == where and g[1] == outcome), None)
            if hit is None:
                groups.append([where, outcome, [tag]])
            else:
                hit[2].append(tag)
    return out


def unpack(packed):
    out = {'cpu': {}, 'gpu': {}}
    for call, groups in packed.items():
        for where, outcome, tags in groups:
            for sec in ('cpu', 'gpu') if where == 'both' else (where,):
                out[sec].update({f'{call}: {tag}': outcome for tag in tags})
    return out


def dump_packed(packed, path):
    dump = lambda x: json.dumps(x, separators=(',', ':'))
    with open(path, 'w') as fh:                               # one outcome per line
        fh.write('{\n' + ',\n'.join(f'{dump(call)}:[\n' + ',\n'.join(dump(g) for g in groups) + '\n]' for call, groups in sorted(packed.items())) + '\n}\n')


def _load(name):
    with open(os.path.join(ROOT, 'tests', 'golden', name)) as fh:
        return unpack(json.load(fh))


UNIFIED = _load('front_end_unified.json')          # {section: {case: [outcome then, outcome now]}}, a table too long to spell out here


class Reached(Exception):
    pass


class StubEngine:
    def __getattr__(self, name):
        def method(*args, **kwargs):
            raise Reached(name, args, kwargs)
        return method


def build(device):
    from var_amd.detinit import fill_module_
    from var_amd.models import build_vae_var
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=device, patch_nums=PNS, depth=DEPTH, ch=32)
    fill_module_(var, DEPTH, 0, 'var.')
    fill_module_(vae, DEPTH, 0, 'vae.')
    return var.eval()


def value(a, content=True, result=False):
    if a is None or isinstance(a, (bool, str)):
        return a
    if isinstance(a, (np.bool_, np.integer)):
        return a.item()
    if isinstance(a, int):
        return a
    if isinstance(a, (float, np.floating)):
        return _ZEROS.sub('p', float(a).hex())                  # (float.hex without the mantissa's trailing zeros: the same number)
    if isinstance(a, torch.Generator):
        return ['rng', a.initial_seed()]
    if isinstance(a, torch.Tensor):
        if content and a.numel() > (64 if result else 256):
            if result and (a.is_floating_point() or result == 'fixed point'):     # compared within a tolerance: the sum stands for the content
                return [str(a.dtype), list(a.shape), a.device.type, {'sum': value(float(a.detach().double().sum()))}]
            # an input handed through whole (an image) or an exact integer result: its bytes, hashed
            return [str(a.dtype), list(a.shape), a.device.type, {'sha256': hashlib.sha256(a.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}]
        return [str(a.dtype), list(a.shape), a.device.type, value(a.detach().cpu().tolist()) if content else None]
    if isinstance(a, np.ndarray):
        return [str(a.dtype), list(a.shape), 'numpy', value(a.tolist())]
    if isinstance(a, (bytes, bytearray)):
        return ['bytes', bytes(a).hex()]
    if isinstance(a, dict):
        return {str(k): value(v, content and k != 'tokens_out', result) for k, v in a.items()}
    if hasattr(a, '_asdict'):
        return [type(a).__name__, value(a._asdict(), content, result)]
    if isinstance(a, (list, tuple)):
        return [value(v, content, result) for v in a]
    if callable(a):
        return ['callable', getattr(a, '__name__', type(a).__name__)]
    names = [n for n in getattr(a, '__slots__', None) or vars(a) if not n.startswith('_')]
    return [type(a).__name__, {n: value(getattr(a, n), content, 'fixed point' if result and (type(a).__name__, n) in FIXED_POINT else result) for n in names}]


def run_case(var, case):
    """-> (outcome, the (file, line) of var_amd/models/var.py or args.py that raised, or None)"""
    from var_amd.models import var as var_module
    name, kw = case
    fn = getattr(var_module, name) if name in MODULE_FUNCTIONS else getattr(var, name)
    torch.manual_seed(SEED)
    var.engine = lambda: StubEngine()
    try:
        out = fn(**kw)
    except Reached as e:
        method, args, kwargs = e.args
        return ['engine', method, value(list(args)), value(kwargs)], None
    except Exception as e:                                   # noqa: BLE001  (every refusal is an outcome)
        here = os.path.join('var_amd', 'models')
        lines = [(os.path.basename(f.filename), f.lineno) for f in traceback.extract_tb(e.__traceback__)
                 if here in f.filename and os.path.basename(f.filename) in ('var.py', 'args.py')]
        return ['raise', type(e).__name__, str(e)], (lines[-1] if lines else None)
    finally:
        del var.engine
    return ['return', value(out, result=True)], None


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _short(v):
    if isinstance(v, torch.Tensor):
        return f'tensor({str(v.dtype)[6:]}, {tuple(v.shape)}, {v.device.type})'
    if isinstance(v, np.ndarray):
        return f'ndarray({v.dtype}, {v.shape})'
    if isinstance(v, np.generic):
        return f'np.{type(v).__name__}({v.item()!r})'
    if hasattr(v, '__next__'):
        return 'iterator'
    if isinstance(v, (list, tuple)) and any(isinstance(x, (torch.Tensor, np.ndarray, list, tuple)) for x in v):
        r = '[' + ', '.join(_short(x) for x in v) + ']'
    else:
        r = repr(v)
    return r if len(r) <= 60 else r[:57] + '...'


def cases(dev):
    """{name: (method or module function, keyword arguments)}; dev: where the model lives, and where the 'on the model's device' inputs go"""
    out = {}
    t = torch.tensor

    def add(prefix, method, base, **changed):
        tag = ', '.join(f'{k}={_short(v)}' for k, v in changed.items()) or 'valid'
        name, i = f'{prefix}: {tag}', 1
        while name in out:                                   # (two tensors of one dtype and shape)
            i += 1
            name = f'{prefix}: {tag} ({i})'
        out[name] = (method, {**base, **changed})

    def sweep(prefix, method, base, table):
        for arg, values in table.items():
            for v in values:
                add(prefix, method, base, **{arg: v})

    gt = (torch.arange(2 * L).view(2, L) * 37) % V
    gt_list = [gt[:, b:b + p * p] for b, p in zip((0, 1, 5), PNS)]
    lab = t([3, 7])
    nan, inf = float('nan'), float('inf')

    # the reference-style samplers: B, label_B, g_seed
    labels = [None, 3, -1, 0, NUM_CLASSES, True, np.int64(3), np.int32(-1), t([3, 7]), t([3, 7], device=dev), t([3, 7], dtype=torch.int32), np.array([3, 7]), [3, 7],
              t([[3], [7]]), t([3.0, 7.0]), t([True, False]), t([3, 7, 9]), 'a', 3.0]
    for m in ('autoregressive_infer_cfg', 'autoregressive_infer_cfg_scored'):
        base = dict(B=2, label_B=3, g_seed=11, cfg=1.5, top_k=900, top_p=0.96)
        add(m, m, base)
        sweep(m, m, base, dict(label_B=labels, g_seed=[None, 0, np.int64(5), 'a', 1.5, -1], B=[1, np.int64(2), 2.0, 'a'], cfg=[t(2.0), np.float32(3.0), [1.0, 2.0]],
                               top_k=[0, np.int64(5)], top_p=[0.0, np.float64(0.5)], more_smooth=[True, 1, None]))
        add(m, m, base, label_B=None, g_seed=None)
        add(m, m, base, label_B=None, g_seed=12)
    add('autoregressive_infer_cfg_scored', 'autoregressive_infer_cfg_scored', dict(B=2, label_B=3, g_seed=11), decode=False)

    m = 'autoregressive_infer_cfg_with_mask'
    mask = torch.zeros(6, 6)
    base = dict(B=2, label_B=3, g_seed=11, cfg=1.5, top_k=900, top_p=0.96, input_img_tokens=gt, edit_mask=mask)
    add(m, m, base)
    add(m, m, base, input_img_tokens=None, edit_mask=None)
    add(m, m, base, input_img_tokens=None)
    add(m, m, base, edit_mask=None)
    add(m, m, base, label_B=None, g_seed=None)
    add(m, m, base, label_B=None, g_seed=12)
    sweep(m, m, base, dict(
        B=[True, 0, -1, 2.0, np.int64(2), 'a', None, 1, 3],
        label_B=labels, g_seed=[None, 'a'],
        input_img_tokens=[gt_list, tuple(gt_list), gt[:1], [x[:1] for x in gt_list], gt.to(dev), gt.int(), gt[:, :-1], torch.cat([gt, gt[:1]]), gt.float(), gt.bool(),
                          gt.to(torch.complex64), gt - 1, gt + (V - 500), gt_list[:2], [gt_list[0], gt_list[1], [1] * 9], [gt_list[0], gt_list[1], gt_list[2][:, :8]],
                          [gt_list[0], gt_list[1][:1], gt_list[2]], [gt_list[0][0], gt_list[1][0], gt_list[2][0]], [gt_list[0].to(dev), gt_list[1], gt_list[2].to(dev)],
                          gt.tolist(), gt.numpy(), gt[0], 5, torch.zeros(2, 0, dtype=torch.int64)],
        edit_mask=[torch.zeros(2, 6, 6), torch.zeros(1, 5, 7), torch.zeros(6, 6, dtype=torch.bool), torch.zeros(6, 6, dtype=torch.int32), torch.ones(6, 6, device=dev),
                   torch.zeros(6, 6, dtype=torch.float64), torch.zeros(3, 6, 6), torch.zeros(1, 1, 6, 6), torch.zeros(6), torch.zeros(6, 6, dtype=torch.complex64),
                   torch.zeros(0, 6), torch.zeros(2, 6, 0), mask.numpy(), mask.tolist(), 1],
        more_smooth=[True, 1]))

    m = 'inpainting'
    keep = torch.zeros(2, L, dtype=torch.bool)
    keep[:, :5] = True
    base = dict(gt_tokens=gt, mask=keep, label=3, g_seed=11, cfg=1.5, top_k=900, top_p=0.96)
    add(m, m, base)
    add(m, m, base, label=None, g_seed=None)
    add(m, m, base, label=None, g_seed=12)
    sweep(m, m, base, dict(label=labels, g_seed=[None, 'a'], mask=[keep[:1], keep[:, :5], keep.to(dev), keep.float()], gt_tokens=[gt.to(dev), gt[:1], gt.tolist()],
                           cfg=[np.float32(2.0)], top_k=[np.int64(3)], top_p=[0.5], more_smooth=[True, 1]))

    m = 'smooth_sampling'
    base = dict(gt_tokens=gt, n=4, label=3, g_seed=11, cfg=1.5)
    add(m, m, base)
    add(m, m, base, label=None, g_seed=None)
    add(m, m, base, label=None, g_seed=12)
    sweep(m, m, base, dict(label=labels, g_seed=[None, 'a'], gt_tokens=[gt.to(dev), gt.tolist()], n=[np.int64(3), 0, 'a'],
                           neighbor_threshold=[None, 0.5, np.float32(0.25), 1, 'a', t(0.5)], more_smooth=[True, 1]))

    # the per-image samplers
    seeds = [1, 2]
    per_image = dict(
        label_B=[[3, 7], (3, 7), np.array([3, 7]), t([3, 7], device=dev), t([3, 7], dtype=torch.uint8), [NUM_CLASSES, 0], [-1, 3], [3, NUM_CLASSES + 1], 3, np.int64(3), t(3),
                 t([[3, 7]]), [], t([3.0, 7.0]), [3.0, 7.0], t([True, False]), [True, False], t([3, 7], dtype=torch.complex64), None, 'a'],
        g_seeds=[(1, 2), t([1, 2]), t([1, 2], device=dev), np.array([1, 2]), [np.int64(1), np.int32(2)], [1.0, 2.0], [0, (1 << 63) - 1], 1, np.int64(1), t(1), t([1]),
                 [1, 2, 3], [], [-1, 2], [1, 1 << 63], [1.5, 2], [True, 2], ['a', 2], [None, 2], None, 'ab', [inf, 1], [nan, 1], [[1, 2]], t([1.0, 2.0]),
                 np.array([1.5, 2.0]), 1.0],
        cfg=[0, 2, np.float32(2.5), np.int64(2), t(2.5), [1.0, 2.0], (1.0, 2.0), t([1.0, 2.0]), np.array([1.0, 2.0]), t([1, 2]), -1.0, True, '1.5', [1.0], [1.0, 2.0, 3.0], nan,
             inf, [1.0, nan], 'a', None, [1.0, None], [1.0, 'a'], [[1.0, 2.0]], 1 << 2000],
        top_k=[0, V, np.int64(5), 5.0, t(5), [0, 5], t([0, 5]), np.array([0, 5]), [5.0, np.int32(6)], -1, V + 1, [0, -1], 1.5, True, [True, 1], 'a', None, [1], nan, inf,
               t([0.5, 1.0]), np.float32(5.0)],
        top_p=[0, 1, 1.0, np.float32(0.5), t(0.5), [0.0, 1.0], t([0.0, 1.0]), np.array([0.5, 0.25]), True, -0.1, 1.1, nan, [0.5, nan], 'a', None, [0.5], [0.5, 'a']])
    for m in ('autoregressive_infer_cfg_per_image', 'autoregressive_infer_cfg_per_image_scored'):
        base = dict(label_B=lab, g_seeds=seeds, cfg=1.5, top_k=900, top_p=0.96)
        add(m, m, base)
        sweep(m, m, base, per_image)
        sweep(m, m, base, dict(more_smooth=[True, 1]))
    add('autoregressive_infer_cfg_per_image', 'autoregressive_infer_cfg_per_image', dict(label_B=lab, g_seeds=seeds), return_tokens=True)
    add('autoregressive_infer_cfg_per_image_scored', 'autoregressive_infer_cfg_per_image_scored', dict(label_B=lab, g_seeds=seeds), decode=False)

    # candidates and particles
    sd2 = [[11, 12], [21, 22]]
    cand = dict(
        label_B=[[3, 7], np.array([3, 7]), t([3, 7], device=dev), 3, [3], [3, 7, 9], t([[3, 7]]), t([[3], [7]]), t([3.0, 7.0]), t([True, False]), [-1, 3], [3, NUM_CLASSES + 1],
                 [], 'a'],
        g_seeds=[t(sd2), t(sd2, device=dev), np.array(sd2), ((11, 12), (21, 22)), [[11], [21]], [[11, 12, 13], [21, 22, 23]], [11, 21], t([11, 21]), [[11, 12], [21]],
                 [[11, 12]], [[], []], [], 11, None, [[11, 12], [21, -1]], [[11, 12], [21, 1 << 63]], [[11, 12], [21, 1.5]], [[11, 12], [21, 2.0]], [[11, 12], [21, True]],
                 [[11, 12], [21, 'a']], t(sd2).float(), [[[11, 12]], [[21, 22]]], 'ab', ['ab', 'cd']],
        n=[None, 2, np.int64(2), 2.0, 3, 1, True, 'a', 2.5, '2'],
        by=['logp_guided', 'logp_drawn', 'logp', None, 1, ('logp_cond',)],
        cfg=[[1.0, 2.0], t([1.0, 2.0]), np.array([1.0, 2.0]), (1.0, 2.0), [1.0], [1.0, 2.0, 3.0, 4.0], t(2.0), np.float32(2.0), nan, [1.0, inf], 'a', None],
        top_k=[[0, 5], t([0, 5]), np.array([0, 5]), np.int64(5), 5.0, [1], -1, V + 1, 1.5, True, 'a'],
        top_p=[[0.0, 1.0], t([0.0, 1.0]), np.array([0.5, 0.25]), np.float32(0.5), [0.5], -0.1, 1.1, nan, 'a'],
        max_images=[1, 2, 4, np.int64(8), 4.0, 0, -1, True, False, 2.5, 'a', None, nan, inf, [4], t(4)])
    keeps = [None, {}, {0: 1}, {1: 1}, {0: 2}, {np.int64(0): np.int64(1)}, {0: 5, 1: 1}, {1: 1, 0: 1}, [(0, 1)], 'a', 1, {True: 1}, {0.0: 1}, {-1: 1}, {2: 1}, {'a': 1},
             {0: True}, {0: 0}, {0: 1.0}, {0: 'a'}, {0: None}]
    m = 'sample_best_of'
    base = dict(label_B=lab, g_seeds=sd2, n=2, by='logp_cond', cfg=1.5, top_k=900, top_p=0.96, max_images=64)
    add(m, m, base)
    sweep(m, m, base, cand)
    m = 'sample_best_of_pruned'
    base = dict(base, keep={0: 1})
    add(m, m, base)
    sweep(m, m, base, cand)
    sweep(m, m, base, dict(keep=keeps, decode=[False, 0]))
    m = 'sample_smc'
    base = dict(label_B=lab, g_seeds=sd2, resample=(0, 1), n=2, by='logp_cond', beta=1.0, ess=0.5, cfg=1.5, top_k=900, top_p=0.96, max_images=64)
    add(m, m, base)
    sweep(m, m, base, cand)
    resamples = [(), [], [0], (1,), [np.int64(0), np.int32(1)], t([0, 1]), np.array([0]), range(2), None, 'ab', b'ab', {0: 1}, 1, [True], [0.0], [-1], [2], [1, 0], [0, 0],
                 ['a'], [None]]
    sweep(m, m, base, dict(
        resample=resamples,
        beta=[0, 0.0, -2.5, np.float32(0.5), np.int64(2), True, nan, inf, -inf, 'a', None, '1.0', t(1.0), [1.0], 1 << 2000],
        ess=[None, 1, 1.0, 1e-9, np.float32(0.25), np.int64(1), 0, 0.0, -0.5, 1.5, True, nan, inf, 'a', '0.5', t(0.5), [0.5]],
        resample_seeds=[None, [5, 6], (5, 6), t([5, 6]), np.array([5, 6]), [5.0, 6.0], 5, np.int64(5), t(5), [5], [5, 6, 7], [-1, 6], [5, 1 << 63], [5.5, 6], [True, 6], ['a', 6],
                        'ab'],
        decode=[False, 0]))
    for v in resamples:
        add('normalize_resample', 'normalize_resample', dict(resample=(0,), S=S), resample=v)
    add('normalize_resample', 'normalize_resample', dict(resample=(0, 1, 2), S=5))
    add('normalize_resample', 'normalize_resample', dict(resample=(0,), S=1))
    add('normalize_resample', 'normalize_resample', dict(resample=(), S=1))
    for v in keeps:
        add('normalize_keep', 'normalize_keep', dict(keep={0: 1}, S=S, alive=3), keep=v)
    add('normalize_keep', 'normalize_keep', dict(keep={0: 4, 1: 3, 2: 3, 3: 1}, S=5, alive=4))
    add('normalize_keep', 'normalize_keep', dict(keep={0: 1}, S=S, alive=1))

    # the scoring family
    lab_k, lab_nk = [1, 2, 3], [[1, 2, 3], [4, 5, 6]]
    tokens = [gt.tolist(), gt.numpy(), gt.int(), gt.to(torch.uint8) if V <= 256 else gt.to(torch.int16), gt.to(dev), gt[:1], gt[0], gt[:, :-1], gt[:0], gt.float(), gt.bool(),
              gt.to(torch.complex64), gt - 1, gt + (V - 500), gt.view(2, 1, L), 5, None, 'a', gt.double().numpy()]
    score_labels = [lab_k, lab_nk, t(lab_k), t(lab_nk), np.array(lab_nk), t(lab_nk, device=dev), t(lab_nk, dtype=torch.int32), tuple(lab_k), [0, NUM_CLASSES], [7],
                    3, np.int64(3), [], [[], []], [[1, 2, 3]], [[1, 2], [3, 4], [5, 6]], t(lab_nk).view(2, 3, 1), t([1.0, 2.0]), [1.5, 2.0], t([True, False]), [True], [-1, 2],
                    [1, NUM_CLASSES + 1], None, 'a']
    cfgs = [0, 0.0, 1.5, np.float32(1.5), np.int64(2), t(1.5), '1.5', True, -1.0, -1e-9, nan, inf, 'a', None, [1.5], t([1.0, 2.0]), 1 << 2000]
    rows = [1, 2, 64, np.int64(4), 4.0, np.float32(4.0), 0, -1, True, False, 2.5, nan, inf, 'a', '4', None, [4], t(4), t(4.0)]
    scoring = dict(gt_tokens=tokens, label=score_labels, cfg=cfgs, max_rows=rows)
    base = dict(gt_tokens=gt, label=lab_k, cfg=0.0, max_rows=4)
    m = 'token_log_likelihood'
    add(m, m, base)
    sweep(m, m, base, scoring)
    sweep(m + ' with cfg', m, dict(base, cfg=1.5), dict(max_rows=[1, 2, True, 1.0, 2.0]))
    m = 'token_scores'
    for sc, kw in (('log_prob', {}), ('group_smoothed', {}), ('group_smoothed', dict(group=7)), ('neighbor_max', dict(threshold=0.5)), ('expected_distance', {}),
                   ('expected_distance', dict(top_k=5))):
        add(f'{m} {sc}', m, dict(base, score=sc), **kw)
    sweep(m, m, dict(base, score='group_smoothed', group=7), dict(gt_tokens=tokens[-6:], label=score_labels[-6:], cfg=cfgs[-8:], max_rows=rows[-12:]))
    sweep(m, m, dict(base, score='log_prob'), dict(score=['logprob', None, 1, ('log_prob',)], group=[7], threshold=[0.5], top_k=[5], cfg=['a'], max_rows=[0]))
    sweep(m + ' group_smoothed', m, dict(base, score='group_smoothed'),
          dict(group=[1, V + 5, np.int64(7), 7.0, 0, -1, True, 2.5, nan, inf, 'a', '7', [7], t(7)], threshold=[0.5], top_k=[5]))
    sweep(m + ' neighbor_max', m, dict(base, score='neighbor_max', threshold=0.5),
          dict(threshold=[0, 0.0, np.float32(0.5), np.int64(1), t(0.5), '0.5', None, True, -0.5, nan, inf, 'a', [0.5], 1 << 2000], group=[7], top_k=[5]))
    sweep(m + ' expected_distance', m, dict(base, score='expected_distance'),
          dict(top_k=[1, V, np.int64(5), 5.0, 0, V + 1, -1, True, 2.5, nan, inf, 'a', '5', [5], t(5)], group=[7], threshold=[0.5]))
    m = 'distance_profile'
    edges = [0.0, 0.5, 1.0, inf]
    base_dp = dict(base, edges=edges)
    add(m, m, base_dp)
    add(m, m, base_dp, min_prob=1e-10)
    sweep(m, m, base_dp, dict(
        edges=[t(edges), np.array(edges), tuple(edges), [0, 1], t([0, 1]), t(edges, dtype=torch.float64), t(edges[:3], device=dev), [0.0], [], 1.0, None, 'a', ['a', 'b'],
               [[0.0, 1.0]], list(range(258)), list(range(257)), [0.0, nan, 1.0], [nan, 1.0], [-0.5, 1.0], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, inf, inf], [inf, inf],
               [1.0, 1.0 + 2.0 ** -30], t([1 + 2j, 2])],
        min_prob=[0, 0.5, np.float32(0.25), np.int64(0), 1 - 2.0 ** -30, True, 1, 1.0, -0.1, -1e-60, nan, inf, 'a', '0.5', None, t(0.5), [0.5]],
        gt_tokens=tokens[-6:], label=score_labels[-6:], cfg=cfgs[-8:], max_rows=rows[-12:]))
    m = 'class_information'
    add(m, m, base)
    third = [1 / 3, 1 / 3, 1 / 3]
    sweep(m, m, base, dict(
        prior=[[0.5, 0.25, 0.25], t([0.5, 0.25, 0.25]), np.array([0.5, 0.25, 0.25]), [[0.5, 0.25, 0.25], [0.25, 0.25, 0.5]], [1, 0, 0], t([1, 0, 0]), third,
               t(third, dtype=torch.float64), t([0.5, 0.25, 0.25], device=dev), [0.5, 0.5], [[0.5, 0.25, 0.25]], [[[0.5, 0.25, 0.25]]], 0.5, t([True, False, False]),
               t([1 + 0j, 0, 0]), 'a', ['a', 'b', 'c'], [0.5, 0.25, nan], [0.5, 0.25, inf], [1.5, -0.25, -0.25], [0.5, 0.25, 0.2], [0.5, 0.25, 0.25 + 1e-5], [0.0, 0.0, 0.0],
               [[0.5, 0.25, 0.25], [0.5, 0.25, 0.3]]],
        gt_tokens=tokens[-6:], label=score_labels[-6:] + [[0] * 16385], cfg=cfgs[-8:], max_rows=rows[-12:]))
    m = 'classify'
    add(m, m, base)
    add(m, m, base, score='neighbor_max', threshold=0.5, keep={0: 2})
    sweep(m, m, base, dict(keep=keeps, score=['logprob'], group=[7], gt_tokens=tokens[-6:], label=score_labels[-6:], cfg=cfgs[-8:], max_rows=rows[-12:]))
    m = 'class_heatmaps'
    base_hm = dict(base, image=torch.zeros(2, 3, 8, 8), size=8)
    add(m, m, base_hm)
    sweep(m, m, base_hm, dict(score=['group_smoothed', 'logprob'], group=[7], gt_tokens=[gt[:1]], label=[[-1]], cfg=[nan], max_rows=[0, True]))
    add(m, m, base_hm, score='group_smoothed', group=0)

    m = 'attention_profile'
    base = dict(gt_tokens=gt, label=lab, radius=1, layers=None, max_rows=4)
    add(m, m, base)
    add(m, m, base, return_tokens=True)
    sweep(m, m, base, dict(
        gt_tokens=tokens,
        label=[3, NUM_CLASSES, np.int64(3), [3, 7], np.array([3, 7]), t([3, 7], device=dev), t([3, 7], dtype=torch.int32), True, 3.0, t(3), [3], [3, 7, 9], [[3, 7]], t([3.0, 7.0]),
               t([True, False]), -1, NUM_CLASSES + 1, [-1, 3], [3, NUM_CLASSES + 1], None, 'a'],
        radius=[0, 3, 100, np.int64(2), -1, True, 1.0, 1.5, nan, 'a', None, [1], t(1)],
        layers=[(0,), [1], [0, 1], (np.int64(0), np.int32(1)), t([0, 1]), np.array([1]), range(2), [], (), [1, 0], [0, 0], [-1], [DEPTH], [True], [0.0], ['a'], [None], 1, 'ab',
                {0: 1}],
        max_rows=[1, np.int64(4), 0, -1, True, 4.0, 2.5, nan, 'a', None, [4], t(4)]))

    m = 'evaluate'
    base = dict(gt_tokens=gt, label_B=lab, label_smooth=0.0, max_rows=4)
    add(m, m, base)
    sweep(m, m, base, dict(
        gt_tokens=tokens + [gt_list, tuple(gt_list), [x.to(dev) for x in gt_list], gt_list[:2], gt_list + gt_list[:1], [gt_list[0], gt_list[1], gt_list[2][:, :8]],
                            [gt_list[0], gt_list[1][:1], gt_list[2]], [gt_list[0][0], gt_list[1][0], gt_list[2][0]], [gt_list[0].to(dev), gt_list[1], gt_list[2].to(dev)],
                            [gt_list[0], gt_list[1], gt_list[2].tolist()], [], [x.float() for x in gt_list], [x - 1 for x in gt_list]],
        label_B=[[3, 7], (3, 7), np.array([3, 7]), t([3, 7], device=dev), t([3, 7], dtype=torch.int32), [0, NUM_CLASSES], 3, np.int64(3), t(3), [3], [3, 7, 9], [[3, 7]],
                 t([3.0, 7.0]), [3.0, 7.0], t([True, False]), [-1, 3], [3, NUM_CLASSES + 1], None, 'a'],
        label_smooth=[0, 0.1, np.float32(0.1), np.int64(0), 1 - 2.0 ** -30, True, 1, 1.0, -0.1, nan, inf, 'a', '0.1', None, t(0.1), [0.1]],
        max_rows=[1, np.int64(4), 0, -1, True, 4.0, 2.5, nan, 'a', None, [4], t(4)]))

    m = 'classify_generative'
    img = torch.zeros(2, 3, 48, 48)
    base = dict(img=img, label=lab_k, last_kept_scale=0, feature='vae_post', cfg=0.0, max_rows=4)
    add(m, m, base)
    add(m, m, dict(base, img=img.to(dev)))
    sweep(m, m, base, dict(
        img=[img[:1], img[0], img[:0], img[:, :2], img[:, :, :47], img[:, :, :, :47], img.double(), img.half(), img.numpy(), img.tolist(), None],
        label=score_labels,
        last_kept_scale=[1, np.int64(1), -1, S - 1, True, 0.0, 1.5, nan, 'a', None, [0], t(0)],
        feature=['vae_fhat', len, 'vae', None, 1, ('vae_post',)],
        cfg=cfgs, max_rows=rows, match_input_range=[True, 1, 0, None, 'a', np.bool_(True)]))
    sweep(m + ' with cfg', m, dict(base, cfg=4.0), dict(max_rows=[1, 2, True, 1.0, 2.0]))

    # the token codec
    m = 'compress'
    base = dict(gt_tokens=gt, label_B=lab, cfg=0.0, scales=None)
    add(m, m, base)
    sweep(m, m, base, dict(
        gt_tokens=tokens + [gt_list, tuple(gt_list), gt_list[:2], [x.float() for x in gt_list], [gt_list[0], gt_list[1], gt_list[2][:1]], [], [x - 1 for x in gt_list]],
        label_B=[3, NUM_CLASSES, np.int64(3), [3, 7], np.array([3, 7]), t([3, 7], device=dev), True, 3.0, t(3), [3], [3, 7, 9], [[3, 7]], t([3.0, 7.0]), t([True, False]), -1,
                 NUM_CLASSES + 1, [-1, 3], [3, NUM_CLASSES + 1], None, 'a'],
        cfg=cfgs,
        scales=[0, 1, S - 1, np.int64(1), 1.0, S, -1, True, False, 1.5, nan, inf, 'a', '1', [1], t(1)]))
    m = 'decompress'
    from var_amd.models.var import codec_pack
    words = np.array([1, 2, 3], np.uint32)

    def blob(label=3, cfg=0.0, v=V, pns=PNS, coded=S, pb=None):
        from var_amd import abi
        return codec_pack(words, label, cfg, v, pns, coded, 77, abi.CODEC_PB if pb is None else pb)
    base = dict(blobs=[blob(), blob(label=7)], complete=None, fill_cfg=1.5, decode=True)
    add(m, m, base)
    add(m, m, dict(base, blobs=[blob(coded=2)], complete='greedy'))
    add(m, m, dict(base, blobs=[blob(coded=2)]))
    sweep(m, m, base, dict(
        blobs=[(blob(),), iter([blob()]), [bytearray(blob())], [], [blob(), blob(cfg=1.0)], [blob(), blob(coded=2)], [blob(), blob(pns=(1, 2, 4))], [blob(), blob(pb=11)],
               [blob(v=V // 2)], [blob(), blob(v=V // 2)], [blob(pns=(1, 2))], [blob(pb=11)], [blob(coded=0)], [blob(coded=S + 1)], [blob(cfg=-1.0)], [blob(cfg=nan)],
               [blob(label=-1)], [blob(label=NUM_CLASSES + 1)], [blob(label=NUM_CLASSES)], [blob()[:-1]], [blob()[:10]], [b'x' * len(blob())], ['a'], [None], None, 5],
        complete=['greedy', 'argmax', 1, True],
        fill_cfg=cfgs, decode=[False, 0]))
    return out


# ---- recording and comparing ------------------------------------------------------------------------------------------------------------
def record(device):
    """-> ({case: outcome}, {case: line that raised})"""
    var = build(device)
    dev = next(var.parameters()).device
    outcomes, lines = {}, {}
    with torch.no_grad():
        for name, case in cases(dev).items():
            outcomes[name], line = run_case(var, case)
            if line is not None:
                lines[name] = line
    return outcomes, lines


def golden(section):
    return _load('front_end.json')[section]


def _number(x):
    return float.fromhex(x) if isinstance(x, str) else float(x)


def close(want, got, one=None) -> bool:
    """a returned value against its record: floats (float.hex strings) within RTOL / ATOL, ints exactly; below a FIXED_POINT field (one: its
    unit) ints as floats / one"""
    if isinstance(want, list) and len(want) == 2 and isinstance(want[1], dict) and isinstance(got, list) and len(got) == 2 and isinstance(got[1], dict) \
            and isinstance(want[0], str) and want[0] == got[0] and sorted(want[1]) == sorted(got[1]):                     # a result object
        return all(close(want[1][k], got[1][k], FIXED_POINT.get((want[0], k), one)) for k in want[1])
    if isinstance(want, dict) and isinstance(got, dict):
        return sorted(want) == sorted(got) and all(close(want[k], got[k], one) for k in want)
    if isinstance(want, list) and isinstance(got, list):
        return len(want) == len(got) and all(close(a, b, one) for a, b in zip(want, got))
    is_hex = lambda x: isinstance(x, str) and (x.lstrip('-').startswith('0x') or x in ('nan', 'inf', '-inf'))
    if (is_hex(want) and is_hex(got)) or (one is not None and all(type(x) is int or is_hex(x) for x in (want, got))):
        if one == 'rank':
            return abs(want - got) <= RANK_SLACK
        a, b = _number(want) / (one or 1.0), _number(got) / (one or 1.0)
        return (a == b) or (a != a and b != b) or abs(a - b) <= RTOL * max(abs(a), abs(b)) + ATOL
    return type(want) is type(got) and want == got


def same(want, got) -> bool:
    return close(want[1], got[1]) if want[0] == got[0] == 'return' else want == got


def compare(section, got, column=1):
    """the fixture's section against the outcomes of this tree: same cases, same outcomes, but for UNIFIED (column 1: its outcome now; column 0:
    its outcome then, which makes this the check of the revision the fixture was recorded on)"""
    want = golden(section)
    moved = UNIFIED[section]
    assert not set(moved) & set(want), f'in UNIFIED and in the fixture: {sorted(set(moved) & set(want))}'
    assert sorted(got) == sorted(set(want) | set(moved)), (sorted(set(got) - set(want) - set(moved)), sorted(set(want) - set(got)))
    got = json.loads(json.dumps(got))
    want.update({k: v[column] for k, v in moved.items()})
    bad = [f'{k}{" (UNIFIED)" if k in moved else ""}:\n  recorded {want[k]!r}\n  now      {got[k]!r}' for k in sorted(want) if not same(want[k], got[k])]
    assert not bad, f'{len(bad)} of {len(got)} cases differ\n' + '\n'.join(bad[:20])
    return len(want) - len(moved), len(moved)


HANDLERS = ('autoregressive_infer_cfg', 'autoregressive_infer_cfg_scored', 'autoregressive_infer_cfg_per_image', 'autoregressive_infer_cfg_per_image_scored',
            'autoregressive_infer_cfg_with_mask', 'sample_best_of', 'sample_best_of_pruned', 'sample_smc', 'inpainting', 'smooth_sampling', 'token_log_likelihood',
            'token_scores', 'distance_profile', 'class_information', 'attention_profile', 'class_heatmaps', 'classify', 'classify_generative', 'evaluate', 'compress',
            'decompress', '_scored_device', '_hip_only', '_rng_and_labels', '_prior_arg', '_profile_args', '_score_desc', '_token_shape', '_token_label_range') + MODULE_FUNCTIONS


def raise_lines():
    """{(file, line): function} of every `raise` in the argument handling of var_amd/models/var.py and in var_amd/models/args.py (if it exists)"""
    from var_amd.models import var as var_module
    out = {}
    for name in ('var.py', 'args.py'):
        path = os.path.join(os.path.dirname(var_module.__file__), name)
        if not os.path.exists(path):
            continue
        with open(path) as fh:
            tree = ast.parse(fh.read())
        for fn in ast.walk(tree):
            if isinstance(fn, ast.FunctionDef) and (name == 'args.py' or fn.name in HANDLERS or fn.name.endswith('_args') or fn.name.startswith('_edit_')):
                out.update({(name, n.lineno): fn.name for n in ast.walk(fn) if isinstance(n, ast.Raise)})
    return out


if __name__ == '__main__':
    if sys.argv[1:] == ['--check-parent']:                   # on the revision the fixture was recorded on: the fixture and UNIFIED's first column
        for section, device in (('cpu', 'cpu'),) + ((('gpu', 'cuda'),) if torch.cuda.is_available() else ()):
            print(section, compare(section, record(device)[0], column=0), 'cases as recorded / in UNIFIED with their outcome then')
        sys.exit(0)
    assert len(sys.argv) == 3 and sys.argv[1] == '--write', 'usage: frontcases.py --write PATH | --check-parent'
    res = {}
    if os.path.exists(sys.argv[2]):
        with open(sys.argv[2]) as fh:
            res = unpack(json.load(fh))
    reached = set()
    for section, device in (('cpu', 'cpu'),) + ((('gpu', 'cuda'),) if torch.cuda.is_available() else ()):
        outcomes, lines = record(device)
        res[section] = {k: v for k, v in outcomes.items() if k not in UNIFIED[section]}
        reached |= set(lines.values())
        kinds = [v[0] for v in outcomes.values()]
        print(section, len(outcomes), 'cases:', {k: kinds.count(k) for k in ('raise', 'engine', 'return')})
    dump_packed(pack(res), sys.argv[2])
    left = {at: fn for at, fn in raise_lines().items() if at not in reached}
    print(len(left), 'raise lines of the argument handling not reached', '(a multi-line raise counts at its first line)')
    for (name, ln), fn in sorted(left.items()):
        print(f'  {name}:{ln} in {fn}')
