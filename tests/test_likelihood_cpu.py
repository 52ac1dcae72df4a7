"""VAR.token_log_likelihood on CPU (the PyTorch branch): the reference's teacher-forced class scoring (fork eval_prob.py:437-463,
var_analysis.py:322-349) against the reference's own logits, the guided formula, the label spellings and the argument checks."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from models import build_vae_var
from var_amd.detinit import fill_module_

_M = {}


def fixture_model(golden_dir):
    """the d2 model of tests/golden/encode_t_pn12345.npz on CPU, its tokens and the reference's teacher-forced logits"""
    if 'm' not in _M:
        z = np.load(f'{golden_dir}/encode_t_pn12345.npz')
        meta = json.loads(str(z['meta']))
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'])
        fill_module_(var, meta['depth'], 0, 'var.'); fill_module_(vae, meta['depth'], 0, 'vae.')
        var.eval(); vae.eval()
        gt = torch.from_numpy(np.concatenate([z[f'idx_s{si}'] for si in range(len(meta['patch_nums']))], 1).astype(np.int64))
        _M['m'] = (vae, var, meta, gt, torch.from_numpy(z['logits']))
    return _M['m']


def gather64(logits, gt):
    return logits.double().log_softmax(-1).gather(-1, gt.unsqueeze(-1)).squeeze(-1)


def test_matches_reference_logits(golden_dir):
    """(N, 1) labels: the fixture's own labels, against the float64 log-softmax-gather of the reference's logits at its tokens"""
    vae, var, meta, gt, ref_logits = fixture_model(golden_dir)
    var.cond_drop_rate = 0.1                        # ignored: labels are used as given
    lp = var.token_log_likelihood(gt, torch.tensor(meta['labels']).view(-1, 1))
    assert lp.shape == (2, 1, var.L) and lp.dtype == torch.float32
    ref = gather64(ref_logits, gt)
    err = float((lp[:, 0].double() - ref).abs().max())
    assert err <= 7e-4, f'log p(gt) vs reference logits: max |diff| {err:.3e}'


def test_cfg_matches_the_guided_formula(golden_dir):
    """cfg > 0 against var_analysis.py:322-344 evaluated explicitly from two forward calls per image"""
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    var.cond_drop_rate = 0.0
    classes, cfg = [5, meta['labels'][0], 999, 0], 2.5
    lp = var.token_log_likelihood(gt, classes, cfg=cfg, max_rows=3)
    pns = meta['patch_nums']
    ratio = torch.tensor([si / (len(pns) - 1) for si, pn in enumerate(pns) for _ in range(pn * pn)])
    t = cfg * ratio.unsqueeze(0).unsqueeze(-1)
    x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
    for i in range(gt.shape[0]):
        with torch.no_grad():
            cond = var(torch.tensor(classes), x[i:i + 1].expand(len(classes), -1, -1))
            uncond = var(torch.tensor([var.num_classes]), x[i:i + 1])
        z = (1 + t) * cond - t * uncond
        want = torch.log_softmax(z, dim=-1).gather(-1, gt[i:i + 1].expand(len(classes), -1).unsqueeze(-1)).squeeze(-1)
        err = float(((lp[i] - want).abs() / (want.abs() + 1)).max())
        assert err <= 2e-6, f'image {i}: guided log p(gt) vs the explicit formula: relative error {err:.3e}'   # (CPU GEMMs of 3 vs 4 rows round differently)
    # without guidance every class row is its plain log-softmax-gather; guidance changes scales > 0 only
    lp0 = var.token_log_likelihood(gt, classes)
    assert torch.allclose(lp0[..., :1], lp[..., :1], atol=1e-6) and not torch.allclose(lp0[..., 1:], lp[..., 1:])


def test_label_spellings_agree(golden_dir):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    classes = [3, 980, 1000]
    a = var.token_log_likelihood(gt, torch.tensor(classes))
    b = var.token_log_likelihood(gt, torch.tensor([classes, classes]))
    c = var.token_log_likelihood(gt.tolist(), classes)
    assert a.shape == (2, 3, var.L)
    assert torch.equal(a, b) and torch.equal(a, c)
    # the classifier's decision and eval_prob --Clayer are reductions of the same tensor
    assert a.sum(-1).argmax(-1).shape == (2,)


def test_argument_checks(golden_dir):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    ok = torch.tensor([1, 2])
    bad = [
        dict(gt_tokens=gt[:, :-1], label=ok),                                   # token shape
        dict(gt_tokens=gt[0], label=ok),
        dict(gt_tokens=gt.float(), label=ok),
        dict(gt_tokens=torch.where(gt == gt[0, 3], -1, gt), label=ok),          # token range
        dict(gt_tokens=torch.where(gt == gt[1, 7], var.V, gt), label=ok),
        dict(gt_tokens=gt, label=torch.tensor([1, -1])),                        # label range
        dict(gt_tokens=gt, label=torch.tensor([1, var.num_classes + 1])),
        dict(gt_tokens=gt, label=torch.zeros(0, dtype=torch.int64)),            # K >= 1
        dict(gt_tokens=gt, label=torch.zeros(3, 2, dtype=torch.int64)),         # (N, K) with the wrong N
        dict(gt_tokens=gt, label=torch.tensor([1.0, 2.0])),
        dict(gt_tokens=gt, label=ok, cfg=-0.5),                                 # cfg
        dict(gt_tokens=gt, label=ok, cfg=float('nan')),
        dict(gt_tokens=gt, label=ok, cfg=float('inf')),
        dict(gt_tokens=gt, label=ok, max_rows=0),                               # max_rows
        dict(gt_tokens=gt, label=ok, cfg=1.0, max_rows=1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            var.token_log_likelihood(**kw)
    # the boundaries themselves are accepted
    lp = var.token_log_likelihood(torch.where(gt == gt[0, 3], var.V - 1, gt), torch.tensor([0, var.num_classes]), cfg=1.0, max_rows=2)
    assert torch.isfinite(lp).all()
