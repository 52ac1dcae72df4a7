"""VAR.classify on the MI355X: the staged, pruned route against the classification rule applied in numpy to the full token_scores of the same
precision (every scored entry bit for bit, every pruned one NaN), bitwise invariance under packing, per-image calls and class order, the work
counter, varhip_class_select_f32 against a lexsort of the rule, and the peak allocation."""
import contextlib

import numpy as np
import pytest
import torch

from tests import util
from tests.test_classify_cpu import expect, same
from tests.test_token_scores_gpu import d16, tokens
from var_amd import abi, hip

pytestmark = pytest.mark.gpu

SCHEDULES = [{2: 16, 5: 4}, {0: 1}, {6: 40}, None]
SCORES = [('log_prob', {}), ('expected_distance', dict(top_k=100))]


def precision(var, prec):
    var.set_hip_precision(prec)
    return torch.autocast('cuda', dtype=torch.bfloat16) if prec == 'auto' else contextlib.nullcontext()


def tied_labels(full, labels, ends, s, m):
    """labels (N, K) with, per image, the lowest-ranked candidate at scale s other than label 1000 replaced by a copy of the one ranked m-1 (the
    last kept): the two have bit-identical scores, so a cut to m after scale s falls between them.  -> (labels, (lower, higher position) per image)"""
    cum = np.add.accumulate(full.astype(np.float64), axis=-1)[..., ends[s] - 1]
    out, pairs = labels.clone(), []
    for n in range(labels.shape[0]):
        order = np.lexsort((np.arange(labels.shape[1]), -cum[n]))
        a = int(order[m - 1])
        b = int([c for c in order[m:] if int(labels[n, c]) != 1000][-1])
        out[n, b] = labels[n, a]
        pairs.append((min(a, b), max(a, b)))
    return out, pairs


def check_against_rule(var, r, full, schedule, what):
    ends = [e for _, e in var.begin_ends]
    pred, total, depth, masked = expect(full, ends, schedule or {})
    assert np.array_equal(r.depth.cpu().numpy(), depth), f'{what}: depths'
    assert same(r.total.cpu().numpy(), total), f'{what}: totals'
    assert np.array_equal(r.pred.cpu().numpy(), pred), f'{what}: pred'
    assert same(r.tokens.cpu().numpy(), masked), f'{what}: tokens (scored entries bitwise, the others NaN)'


@pytest.mark.parametrize('prec', ['f32', 'f16', 'bf16', 'auto'])
def test_d16_matches_the_rule_on_token_scores(prec):
    vae, var = d16()
    gt = tokens(var, 3, 21)
    g = torch.Generator().manual_seed(5)
    base = torch.stack([torch.cat((torch.tensor([1000]), torch.randperm(1000, generator=g)[:39])) for _ in range(3)]).cuda()
    ends = [e for _, e in var.begin_ends]
    try:
        for score, kw in SCORES:
            for cfg in (0.0, 1.5):
                what = f'{prec} {score} cfg={cfg}'
                with torch.no_grad(), precision(var, prec):
                    probe = var.token_scores(gt, base, score, cfg=cfg, **kw).cpu().numpy()
                    labels, pairs = tied_labels(probe, base, ends, 2, 16)
                    full = var.token_scores(gt, labels, score, cfg=cfg, **kw).cpu().numpy()
                    res = {str(k): var.classify(gt, labels, score, cfg=cfg, keep=k, **kw) for k in SCHEDULES}
                for n, (a, b) in enumerate(pairs):
                    assert same(full[n, a], full[n, b]), f'{what}: duplicate rows differ'
                for keep in SCHEDULES:
                    check_against_rule(var, res[str(keep)], full, keep, f'{what} keep={keep}')
                r = res[str(SCHEDULES[0])]
                for n, (a, b) in enumerate(pairs):
                    assert int(r.depth[n, a]) > 2 and int(r.depth[n, b]) == 2, f'{what}: of two tied duplicates the lower position survives'
    finally:
        var.set_hip_precision('f32')


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_packing_calls_and_class_order_are_invisible(prec):
    vae, var = d16()
    gt = tokens(var, 3, 23)
    classes = torch.tensor([[4, 90, 1000, 17, 5, 6, 7, 8, 999, 0, 31, 300],
                            [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16],
                            [999, 0, 4, 31, 500, 501, 502, 1000, 2, 3, 700, 800]], device='cuda')
    perm = torch.randperm(12, generator=torch.Generator().manual_seed(1)).cuda()
    keep = {2: 6, 5: 3}
    var.set_hip_precision(prec)
    try:
        for score, kw in SCORES:
            for cfg in (0.0, 1.5):
                what = f'{prec} {score} cfg={cfg}'
                base = var.classify(gt, classes, score, cfg=cfg, keep=keep, **kw)
                for mr in (2, 7, 64, 300):
                    r = var.classify(gt, classes, score, cfg=cfg, max_rows=mr, keep=keep, **kw)
                    assert all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(r, base)), f'{what} max_rows={mr}'
                single = [var.classify(gt[i:i + 1], classes[i:i + 1], score, cfg=cfg, keep=keep, **kw) for i in range(3)]
                for f in range(4):
                    assert same(torch.cat([s[f] for s in single]).cpu().numpy(), base[f].cpu().numpy()), f'{what}: per-image calls, field {f}'
                p = var.classify(gt, classes[:, perm], score, cfg=cfg, keep=keep, **kw)
                assert torch.equal(perm[p.pred], base.pred), f'{what}: permuted classes, pred'
                for f in (1, 2, 3):
                    assert same(p[f].cpu().numpy(), base[f][:, perm].cpu().numpy()), f'{what}: permuted classes, field {f}'
    finally:
        var.set_hip_precision('f32')


def test_work_counter_counts_rows_run():
    vae, var = d16()
    gt = tokens(var, 2, 29)
    K, N = 30, 2
    ends = [e for _, e in var.begin_ends]
    S = len(ends)
    eng = var.engine()
    for keep, stages in (({2: 16, 5: 4}, [(2, 30), (5, 16), (S - 1, 4)]), ({6: 40, 3: 12}, [(3, 30), (S - 1, 12)]), (None, [(S - 1, 30)])):
        var.classify(gt, list(range(K)), keep=keep)
        assert eng.classify_work == [(e, m, N * m * ends[e]) for e, m in stages], keep
        done = sum(w for _, _, w in eng.classify_work)
        assert keep is None or done < N * K * var.L, keep


def rule_lexsort(tot):
    nan = np.isnan(tot)
    return np.lexsort((np.arange(tot.shape[0]), np.where(nan, 0.0, -tot), nan))


@pytest.mark.parametrize('cand', [1, 7, 1000, 16384])
def test_select_kernel_vs_lexsort(cand):
    """synthetic totals with exact ties (+0 / -0 among them), NaN and +-inf; keep below, at and above cand; with and without tokens to add"""
    rng = np.random.default_rng(cand)
    images = 3
    tot = np.round(rng.standard_normal((images, cand)) * 4) / 2
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -np.inf])
    idx = rng.integers(0, cand, (images, max(1, cand // 5)))
    tot[np.arange(images)[:, None], idx] = special[rng.integers(0, len(special), idx.shape)]
    T, t0 = 6, 2
    toks = (np.round(rng.standard_normal((images, cand, T)) * 8) / 8).astype(np.float32)
    toks[0, :: 3, 4] = np.float32(1e-9)                   # additions that round
    for keep in sorted({1, 3, max(1, cand // 2), cand, cand + 5}):
        for with_tokens in (False, True):
            t1 = T if with_tokens else t0
            want = tot.copy()
            for t in range(t0, t1):
                want = want + toks[:, :, t].astype(np.float64)
            dev_tot = torch.from_numpy(tot).cuda()
            kept = torch.full((images, min(keep, cand)), -7, dtype=torch.int32, device='cuda')
            util.guarded_call('class_select_f32', torch.from_numpy(toks).cuda(), cand * T, T, images, cand, t0, t1, dev_tot, keep, kept)
            torch.cuda.synchronize()
            assert same(dev_tot.cpu().numpy(), want), (cand, keep, with_tokens)
            for n in range(images):
                exp = np.sort(rule_lexsort(want[n])[:keep])
                assert np.array_equal(kept[n].cpu().numpy(), exp), (cand, keep, with_tokens, n)


def test_select_kernel_rejects_bad_arguments():
    tot = torch.zeros(2, 16385, dtype=torch.float64, device='cuda')
    toks = torch.zeros(2, 16385, 4, device='cuda')
    kept = torch.zeros(2, 16385, dtype=torch.int32, device='cuda')
    f = hip.lib().fn['class_select_f32']
    st = hip.current_stream()
    good = [toks.data_ptr(), 16384 * 4, 4, 2, 16384, 0, 4, tot.data_ptr(), 5, kept.data_ptr()]
    assert f(*good, st) == 0
    torch.cuda.synchronize()
    for pos, val in [(4, 16385), (4, 0), (3, 0), (8, 0), (5, -1), (6, -1), (6, 5), (2, 3), (1, 16384 * 4 - 1), (7, None), (9, None), (0, None)]:
        a = list(good); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)
    with pytest.raises(ValueError):
        vae, var = d16()
        var.classify(tokens(var, 1, 3), torch.zeros(16385, dtype=torch.int64), keep={0: 10})


def test_peak_allocation():
    """K = 200, 2 images: after a warm-up call, the peak allocation increase stays below a quarter of one full pass's R * L * V * 4 bytes"""
    vae, var = d16()
    gt = tokens(var, 2, 31)
    classes = list(range(200))
    full = 64 * var.L * var.V * 4
    keep = {4: 50, 7: 10}
    var.classify(gt, classes, cfg=1.5, keep=keep)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = var.classify(gt, classes, cfg=1.5, keep=keep)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert r.tokens.shape == (2, 200, var.L) and r.pred.shape == (2,)
    assert rise < full / 4, f'peak allocation rose by {rise / 1e6:.1f} MB (a full logits tensor is {full / 1e6:.0f} MB)'
