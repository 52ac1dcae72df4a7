"""VAR.attention_maps and VAR.attention_rollout on the GPU, on the tiny test model: the HIP route against the PyTorch twins on a CPU copy, its
invariances (max_rows, batch neighbours, a subset of the layers), the rows' per-scale sums against VAR.attention_profile, and the refusals."""
import numpy as np
import pytest
import torch

from tests import attnflowref as R
from tests.test_attention_profile_gpu import tiny

pytestmark = pytest.mark.gpu

TARGETS = (0, 3, (2, 1, 1), 29, (4, 4, 4))
_BASE = {}


def base():
    if not _BASE:
        var, _, gt, lab = tiny()
        _BASE['maps'] = var.attention_maps(gt.cuda(), lab.cuda(), TARGETS)
        _BASE['roll'] = var.attention_rollout(gt.cuda(), lab.cuda(), TARGETS)
    return _BASE['maps'], _BASE['roll']


def test_hip_route_against_the_torch_twins():
    """within 8x the twins' own f32-against-f64 deviation (attnflowref.TORCH_F32_VS_F64_*, measured on the CPU without the library)"""
    var, cvar, gt, lab = tiny()
    m, r = base()
    D, H, L = var.depth, var.num_heads, var.L
    assert m.rows.shape == (3, D, H, 5, L) and m.rows.dtype == torch.float32 and m.nan_queries.shape == (3, D, H) and not m.nan_queries.any()
    assert r.flow.shape == (3, 5, L) and r.flow.dtype == torch.float32 and not r.nan_queries.any() and m.targets == (0, 3, 9, 29, 54)
    cm, cr = cvar.attention_maps(gt, lab, TARGETS), cvar.attention_rollout(gt, lab, TARGETS)
    for name, a, b, rec in (('rows', m.rows, cm.rows, R.TORCH_F32_VS_F64_ROWS), ('flow', r.flow, cr.flow, R.TORCH_F32_VS_F64_FLOW)):
        err, tol = float((a.cpu() - b).abs().max()), R.HIP_VS_TORCH_FACTOR * rec
        print(f'HIP route against the torch twin, {name}: {err:.3e} (allowed {tol:.3e})')
        assert err <= tol
    assert float((m.rows.double().sum(-1) - 1).abs().max()) <= 1e-3 and float((r.flow.double().sum(-1) - 1).abs().max()) <= 1e-3
    assert bool((r.flow >= 0).all()) and bool((m.rows[:, :, :, 0, 0] == 1).all()) and bool((r.flow[:, 0, 0] == 1).all())
    lim = [1, 5, 14, 30, 55]
    for s, e in enumerate(lim):                                                                # +0 beyond the target's own scale
        assert not m.rows[..., s, e:].any() and not r.flow[:, s, e:].any()
    # a one-layer rollout at alpha = 1 is the head mean of that layer's rows
    one = var.attention_rollout(gt.cuda(), lab.cuda(), TARGETS, layers=(1,), alpha=1.0)
    assert float((one.flow.double() - m.rows[:, 1].double().mean(1)).abs().max()) <= 4 * R.U
    assert torch.equal(var.attention_rollout(gt.cuda(), lab.cuda(), TARGETS, alpha=0.0).flow.cpu(),
                       torch.nn.functional.one_hot(torch.tensor(m.targets), L).float().expand(3, -1, -1))


def test_bit_equal_across_max_rows_neighbours_and_layer_subsets():
    var, _, gt, lab = tiny()
    gt, lab = gt.cuda(), lab.cuda()
    m, r = base()
    for mr in (1, 2):
        assert torch.equal(var.attention_maps(gt, lab, TARGETS, max_rows=mr).rows, m.rows), mr
        assert torch.equal(var.attention_rollout(gt, lab, TARGETS, max_rows=mr).flow, r.flow), mr
    one = var.attention_maps(gt[1:2], lab[1:2], TARGETS)
    assert torch.equal(one.rows[0], m.rows[1]) and torch.equal(var.attention_rollout(gt[1:2], lab[1:2], TARGETS).flow[0], r.flow[1])
    for d in range(var.depth):                                                                 # a subset's maps: the matching slices of the full call
        sub = var.attention_maps(gt, lab, TARGETS, layers=(d,))
        assert sub.layers == (d,) and torch.equal(sub.rows[:, 0], m.rows[:, d]) and torch.equal(sub.nan_queries[:, 0], m.nan_queries[:, d])
    few = var.attention_maps(gt, lab, TARGETS[3:])                                             # ... and a subset of the targets
    assert torch.equal(few.rows, m.rows[:, :, :, 3:])
    assert torch.equal(var.attention_rollout(gt, lab, TARGETS[3:]).flow, r.flow[:, 3:])
    var.autoregressive_infer_cfg(2, torch.tensor([1, 2], device='cuda'), g_seed=0)
    var.token_log_likelihood(gt, [1, 2, 3], cfg=1.5)
    assert torch.equal(var.attention_maps(gt, lab, TARGETS).rows, m.rows) and torch.equal(var.attention_rollout(gt, lab, TARGETS).flow, r.flow)


def test_scale_sums_against_attention_profile():
    """per-scale sums of the rows against attention_profile's tokens / 2^21 for the same queries: that call's bar (attnprofref: (F - 1) + L 2^-30 +
    2^-21, F from |q| <= 100 and unit keys) plus this one's ((a) of attnflowref with the same F: the L1 bar of a row bounds every partial sum)"""
    var, _, gt, lab = tiny()
    m, _ = base()
    L, S = var.L, len(var.patch_nums)
    prof = var.attention_profile(gt.cuda(), lab.cuda(), return_tokens=True)
    mass = m.scale_mass()                                                                      # (3, D, H, 5, S)
    want = prof.tokens[:, :, :, list(m.targets), :S].double() / 2 ** 21
    Dq = R.gamma(64) * 100.0 + 87 * R.U
    F = np.exp(2 * Dq) * (1 + R.EXP_EPS) / (1 - R.EXP_EPS)
    tol = (F - 1) + L * 2.0 ** -30 + 2.0 ** -21 + (F * (1 + (L + 3) * R.U) / (1 - (L + 3) * R.U) - 1)
    err = float((mass - want).abs().max())
    print(f'scale sums of attention_maps against attention_profile: {err:.3e} (allowed {tol:.3e})')
    assert err <= tol


@pytest.mark.parametrize('prec', ['f16', 'bf16'])
def test_16_bit_precisions_are_refused(prec):
    var, _, gt, lab = tiny()
    m, r = base()
    var.set_hip_precision(prec)
    try:
        with pytest.raises(ValueError, match='attention maps and rollout run in f32'):
            var.attention_maps(gt.cuda(), lab.cuda(), TARGETS)
        with pytest.raises(ValueError, match='attention maps and rollout run in f32'):
            var.attention_rollout(gt.cuda(), lab.cuda(), TARGETS)
        assert var.engine().policy == prec                                     # the refusal changes nothing
    finally:
        var.set_hip_precision('f32')
    assert torch.equal(var.attention_maps(gt.cuda(), lab.cuda(), TARGETS).rows, m.rows)
