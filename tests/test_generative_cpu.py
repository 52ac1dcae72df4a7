"""VAR.classify_generative without a GPU: argument checks (ValueError), the CPU model's RuntimeError after them, the reference fixture's
self-consistency (tests/golden/generative_t_pn12345.npz, tools/gen_golden_generative.py), and the new C ABI entries."""
import contextlib
import ctypes
import io
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from models import build_vae_var
from models.var import GenerativeResult
from var_amd.detinit import fill_module_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_M = {}


def cpu_model():
    """the tiny t_pn12345 model of the fixture (depth 2, ch 32, patch_nums 1..5, 80 x 80 images) on CPU"""
    if 'm' not in _M:
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=(1, 2, 3, 4, 5), depth=2, ch=32)
        fill_module_(var, 2, 0, 'var.'); fill_module_(vae, 2, 0, 'vae.')
        var.eval(); vae.eval()
        _M['m'] = (vae, var)
    return _M['m']


def img80(n=2):
    g = torch.Generator(); g.manual_seed(5)
    return torch.rand(n, 3, 80, 80, generator=g) * 2 - 1


BAD = [
    (dict(img=torch.zeros(2, 3, 80)), 'img'),
    (dict(img=torch.zeros(2, 1, 80, 80)), 'img'),
    (dict(img=torch.zeros(2, 3, 64, 64)), 'img'),
    (dict(img=torch.zeros(2, 3, 80, 80, dtype=torch.float64)), 'img'),
    (dict(img=torch.zeros(2, 3, 80, 80, dtype=torch.float16)), 'img'),
    (dict(img=np.zeros((2, 3, 80, 80), np.float32)), 'img'),
    (dict(last_kept_scale=-1), 'last_kept_scale'),
    (dict(last_kept_scale=4), 'last_kept_scale'),
    (dict(last_kept_scale=True), 'last_kept_scale'),
    (dict(last_kept_scale=1.0), 'last_kept_scale'),
    (dict(feature='dinov2'), 'feature'),
    (dict(label=[3, 1001]), 'labels'),
    (dict(label=[-1, 3]), 'labels'),
    (dict(label=torch.tensor([[1, 2], [3, 4], [5, 6]])), 'label'),
    (dict(label=[1.5, 2.0]), 'label'),
    (dict(cfg=-1.0), 'cfg'),
    (dict(cfg=math.nan), 'cfg'),
    (dict(cfg=math.inf), 'cfg'),
    (dict(max_rows=0), 'max_rows'),
    (dict(cfg=4.0, max_rows=1), 'max_rows'),
    (dict(max_rows=2.5), 'max_rows'),
    (dict(match_input_range=1), 'match_input_range'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_validation_raises_value_error(kw, word):
    _, var = cpu_model()
    args = dict(img=img80(), label=[3, 1000], last_kept_scale=1, feature='vae_post', cfg=0.0, max_rows=64)
    args.update(kw)
    mir = args.pop('match_input_range', False)
    with pytest.raises(ValueError, match=word):
        var.classify_generative(args['img'], args['label'], args['last_kept_scale'], args['feature'], args['cfg'], args['max_rows'],
                                match_input_range=mir)


@pytest.mark.parametrize('feature', ['vae_post', 'vae_fhat', lambda x: x.flatten(1)])
def test_cpu_model_raises_runtime_error_after_validation(feature):
    _, var = cpu_model()
    with pytest.raises(RuntimeError, match='HIP'):
        var.classify_generative(img80(), [3, 1000, 3], 0, feature, cfg=4.0, max_rows=2)
    with pytest.raises(ValueError):                       # validation still comes first
        var.classify_generative(img80(), [3, 1000, 3], 4, feature)


def test_training_mode_raises_runtime_error():
    _, var = cpu_model()
    var.train()
    try:
        with pytest.raises(RuntimeError):
            var.classify_generative(img80(), [3], 1)
    finally:
        var.eval()


def test_result_type_is_exported():
    import models.var as mv
    assert mv.GenerativeResult is GenerativeResult and GenerativeResult._fields == ('pred', 'score', 'tokens')


def test_fixture_is_self_consistent(golden_dir):
    z = np.load(f'{golden_dir}/generative_t_pn12345.npz')
    meta = json.loads(str(z['meta']))
    assert meta['ties'] == 0, 'the reference run met an exact tie at a greedy position'
    N, K = z['img'].shape[0], z['labels'].shape[0]
    assert 1000 in z['labels'].tolist() and z['img'].shape == (2, 3, 80, 80)
    ends = np.cumsum([p * p for p in meta['patch_nums']])
    L = int(ends[-1])
    for feat in meta['features']:
        for cfg in meta['cfgs']:
            for c in meta['clayers']:
                key = f'{feat}_cfg{int(cfg)}_c{c}'
                f_in, f_rec, score, pred, tok = (z[f'{key}_{s}'] for s in ('f_in', 'f_rec', 'score', 'pred', 'tokens'))
                assert f_rec.shape[:2] == (N, K) and tok.shape == (N, K, L) and score.dtype == np.float32
                # -mean |f_in - f_rec| (eval_prob.py:509-513), in float64 here: within a few fp32 ulps of the reference's fp32 mean
                s64 = -np.abs(f_in[:, None].astype(np.float64) - f_rec.astype(np.float64)).reshape(N, K, -1).mean(-1)
                assert np.allclose(score, s64, rtol=1e-6, atol=0), key
                # the tie rule: highest score, lowest position among equals (np.argmax returns the first maximum)
                assert np.array_equal(pred, np.argmax(score, axis=-1)), key
                assert all(score[n, pred[n]] >= score[n].max() for n in range(N))
                # the kept prefix is the image's own tokens
                assert np.array_equal(tok[:, :, :ends[c]], np.broadcast_to(z['gt'][:, None, :ends[c]], (N, K, int(ends[c])))), key


def test_new_abi_entries_declared_and_exported():
    new = {'varhip_cfg_argmax_f32', 'varhip_feature_l1_f32'}
    from var_amd import abi
    assert {n[len('varhip_'):] for n in new} <= set(abi.SIGNATURES_HIP_ONLY) <= set(abi.DECLS)     # (the tables against the header: tests/test_abi_cpu.py)
    so_path = os.path.join(ROOT, 'var_amd', 'libvar_hip.so')
    if not os.path.exists(so_path):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'var_amd', 'csrc'), '-j8'], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    so = ctypes.CDLL(so_path)
    assert all(hasattr(so, n) for n in new)
