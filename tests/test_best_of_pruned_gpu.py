"""VAR.sample_best_of_pruned on the MI355X on the fixtures e2e_t_pn12345 (depth 2, 5 scales, L = 55) and d16_pn123 (3 scales,
L = 14), B = 2, n = 4.  No tolerances: every candidate, through its depth, must be bit for bit the request
autoregressive_infer_cfg_per_image_scored(label, seed, ...) run alone, and depth / totals / choice must be what the numpy rule
(tests/test_best_of_pruned_cpu.py: classify's rule on per-token statistics) gives on those eight records.  A wrong cache row, a stale f_hat, a
wrong seed gather or a wrong condition row at a prune boundary changes a survivor's later tokens and fails here."""
import numpy as np
import pytest
import torch

from tests import test_e2e_gpu, util
from tests.test_best_of_pruned_cpu import best_of_rule
from tests.test_e2e_gpu import build_models
from var_amd.models.var import BestOfResult, SampleRecord

pytestmark = pytest.mark.gpu

KW = dict(cfg=1.5, top_k=900, top_p=0.96)
REC = ('tokens',) + SampleRecord.FIELDS
# seeds for which no boundary of KEEP (nor the final choice) hangs on an exact tie; d16_pn123 prunes behind scale 0, a single token: two candidates
# that draw the same first token tie there (seeds 11 and 14 of label 3 do), so its seeds are ones whose first tokens differ
SEEDS_OF = {'t_pn12345': [[11, 12, 13, 14], [21, 22, 23, 24]], 'd16_pn123': [[1, 2, 3, 4], [1, 2, 5, 6]]}
SEEDS = SEEDS_OF['t_pn12345']
KEEP = {'t_pn12345': {1: 3, 3: 1}, 'd16_pn123': {0: 2}}


def _model(name='t_pn12345', fresh=False):
    z, meta = util.load_case(name)
    if fresh:
        test_e2e_gpu._MODELS.clear()
    vae, var = build_models(meta)
    return var, torch.tensor(meta['labels'], dtype=torch.int64, device='cuda')[:2]


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x


def _same_record(a: SampleRecord, b: SampleRecord, rows_a=slice(None), rows_b=slice(None)):
    for k in REC:
        assert torch.equal(_bits(getattr(a, k)[rows_a]), _bits(getattr(b, k)[rows_b])), k


def _same_result(a: BestOfResult, b: BestOfResult):
    assert (a.images is None) == (b.images is None) and (a.images is None or torch.equal(a.images, b.images))
    _same_record(a.winners, b.winners)
    for k in ('totals', 'depth', 'choice', 'tokens'):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k


@pytest.mark.parametrize('name', ['t_pn12345', 'd16_pn123'])
def test_no_pruning_is_sample_best_of(name):
    var, lab = _model(name)
    S, L = len(var.patch_nums), var.L
    img, win, totals, choice = var.sample_best_of(lab, SEEDS, by='logp_cond', **KW)
    full = var.autoregressive_infer_cfg_per_image_scored(lab.repeat_interleave(4), [s for r in SEEDS for s in r], decode=False, **KW)
    for keep in (None, {}, {0: 4, S - 2: 7}):
        res = var.sample_best_of_pruned(lab, SEEDS, keep, n=4, by='logp_cond', **KW)
        assert isinstance(res, BestOfResult)
        assert torch.equal(res.images, img) and torch.equal(_bits(res.totals), _bits(totals)) and torch.equal(res.choice, choice)
        _same_record(res.winners, win)
        assert torch.equal(res.winners.images, res.images)
        assert res.depth.dtype == torch.int64 and bool((res.depth == S - 1).all()) and res.depth.shape == (2, 4)
        assert res.tokens.dtype == torch.int64 and torch.equal(res.tokens.view(8, L), full.tokens)


CASES = [('t_pn12345', 'f32', 'logp_cond'), ('t_pn12345', 'f32', 'logp_drawn'), ('t_pn12345', 'bf16', 'logp_cond'), ('t_pn12345', 'bf16', 'logp_drawn'),
         ('d16_pn123', 'f32', 'logp_cond'), ('d16_pn123', 'f32', 'logp_drawn')]


@pytest.mark.parametrize('name, prec, by', CASES)
def test_pruned_candidates_are_their_own_per_image_requests(name, prec, by):
    var, lab = _model(name)
    SEEDS = SEEDS_OF[name]
    var.set_hip_precision(prec)
    try:
        ends = [e for _, e in var.begin_ends]
        L, schedule = var.L, sorted(KEEP[name].items())
        ones = [[var.autoregressive_infer_cfg_per_image_scored(lab[b:b + 1], [SEEDS[b][c]], decode=False, **KW) for c in range(4)] for b in range(2)]
        stats = np.stack([np.stack([getattr(ones[b][c], by)[0].cpu().numpy() for c in range(4)]) for b in range(2)])       # (2, 4, L) fp32
        # no boundary (nor the final choice) may hang on an exact tie between different candidates: the seeds are chosen so; were one
        # unavoidable, the rule's lower-index order would still define the answer below
        cum = np.add.accumulate(stats.astype(np.float64), axis=-1)
        for s in [s for s, _ in schedule] + [len(ends) - 1]:
            for b in range(2):
                t = cum[b, :, ends[s] - 1]
                assert len(set(t.tolist())) == 4 and not np.isnan(t).any(), f'tie or NaN at scale {s}, image {b}: {t}'
        choice, totals, depth = best_of_rule(stats, ends, schedule)
        res = var.sample_best_of_pruned(lab, SEEDS, KEEP[name], by=by, **KW)
        print(f'{name} {prec} {by}: depth {res.depth.tolist()} (expected {depth.tolist()}), choice {res.choice.tolist()} (expected {choice.tolist()})')
        assert res.depth.tolist() == depth.tolist()
        assert res.choice.tolist() == choice.tolist()
        assert np.array_equal(res.totals.cpu().numpy().view(np.int64), totals.view(np.int64)) and res.totals.dtype == torch.float64
        assert sorted(set(depth.reshape(-1).tolist())) == sorted(set(s for s, _ in schedule) | {len(ends) - 1}), 'the schedule did not prune at every boundary'
        for b in range(2):
            for c in range(4):
                e = ends[depth[b, c]]
                assert torch.equal(res.tokens[b, c, :e], ones[b][c].tokens[0, :e]), (b, c)
                assert bool((res.tokens[b, c, e:] == -1).all()), (b, c)
            w = int(choice[b])
            _same_record(res.winners, ones[b][w], slice(b, b + 1))
            own = var.autoregressive_infer_cfg_per_image_scored(lab[b:b + 1], [SEEDS[b][w]], decode=True, **KW)
            assert torch.equal(res.images[b], own.images[0]), f'image {b}: the winner differs from its own per-image call'
        nod = var.sample_best_of_pruned(lab, SEEDS, KEEP[name], by=by, decode=False, **KW)
        assert nod.images is None and nod.winners.images is None and torch.equal(nod.tokens, res.tokens)
    finally:
        var.set_hip_precision('f32')


def test_chunking_changes_nothing():
    var, lab = _model()
    keep = KEEP['t_pn12345']
    a = var.sample_best_of_pruned(lab, SEEDS, keep, max_images=4, **KW)           # one image per chunk
    b = var.sample_best_of_pruned(lab, torch.tensor(SEEDS), keep, max_images=8, **KW)
    c = var.sample_best_of_pruned(lab, SEEDS, keep, max_images=7, **KW)           # 7 // 4 = 1 image per chunk
    _same_result(a, b)
    _same_result(a, c)
    with pytest.raises(ValueError, match='max_images'):
        var.sample_best_of_pruned(lab, SEEDS, keep, max_images=3, **KW)
    for bad in (dict(by='entropy'), dict(n=2), dict(max_images=0)):
        with pytest.raises(ValueError):
            var.sample_best_of_pruned(lab, SEEDS, keep, **bad)
    for bad in ({4: 2}, {1: 0}, [1, 2]):
        with pytest.raises(ValueError, match='keep'):
            var.sample_best_of_pruned(lab, SEEDS, bad, **KW)


def test_no_trace_left():
    keep = KEEP['t_pn12345']
    var, lab = _model(fresh=True)
    plain0 = var.autoregressive_infer_cfg(2, lab, g_seed=5, **KW).clone()
    best0 = var.sample_best_of(lab, SEEDS, **KW)
    var, lab = _model(fresh=True)
    state = var.rng.get_state().clone()
    first = var.sample_best_of_pruned(lab, SEEDS, keep, **KW)
    assert torch.equal(var.rng.get_state(), state), 'var.rng was read or advanced'
    plain1 = var.autoregressive_infer_cfg(2, lab, g_seed=5, **KW).clone()
    best1 = var.sample_best_of(lab, SEEDS, **KW)
    assert torch.equal(plain1, plain0), 'a plain call differs after a pruned call'
    assert torch.equal(best1[0], best0[0]) and torch.equal(_bits(best1[2]), _bits(best0[2])) and torch.equal(best1[3], best0[3])
    _same_record(best1[1], best0[1])
    eng = var.engine()
    sets = {k: v['kc'][0].data_ptr() for k, v in eng._ws_bop.items()}
    _same_result(var.sample_best_of_pruned(lab, SEEDS, keep, **KW), first)
    assert {k: v['kc'][0].data_ptr() for k, v in eng._ws_bop.items()} == sets, 'a repeated call allocated cache memory'
    # the workspace slots: the plain call's workspace at another batch size neither disturbs the stages' nor is disturbed by them
    lab3 = torch.cat((lab, lab[:1]))
    plain3 = var.autoregressive_infer_cfg(3, lab3, g_seed=6, **KW).clone()
    ws3 = eng._ws[next(k for k in eng._ws if k[0] == 3)]
    _same_result(var.sample_best_of_pruned(lab, SEEDS, keep, **KW), first)
    assert any(v is ws3 for v in eng._ws.values()), "the pruned call evicted the plain call's workspace"
    assert {k: v['kc'][0].data_ptr() for k, v in eng._ws_bop.items()} == sets
    assert torch.equal(var.autoregressive_infer_cfg(3, lab3, g_seed=6, **KW), plain3)


@pytest.mark.parametrize('keep, max_images', [({1: 3, 3: 1}, 8), ({1: 3, 3: 1}, 4), ({}, 8), ({0: 2}, 64)])
def test_best_of_work_is_what_the_schedule_implies(keep, max_images):
    var, lab = _model()
    var.sample_best_of_pruned(lab, SEEDS, keep, decode=False, max_images=max_images, **KW)
    be, S = var.begin_ends, len(var.patch_nums)
    want, first, m = [], 0, 4
    for s, k in sorted(keep.items()) + [(S - 1, 1)]:
        want.append((s, m, 2 * m * (be[s][1] - be[first][0])))
        first, m = s + 1, k
    assert var.engine().best_of_work == want
