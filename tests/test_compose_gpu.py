"""VAR.sample_composed on the MI355X, on the tiny model of tests/test_per_image_gpu.py (patch_nums (1, 2, 3, 4), depth 2, ch 32):
one class of weight one is the per-image scored call bit for bit in f32, f16 and bf16; a request does not depend on its batch or on max_rows;
the tokens are rebuilt scale by scale from teacher-forced logits, the numpy twin of the mix, the host Philox fill and the pinned sampler; a
schedule over the scales; the record's statistics against float64; no trace in the engine's state; the refusals."""
import contextlib
import io

import numpy as np
import pytest

from tests import samplestatsref as R
from tests import util
from tests.test_compose_cpu import REFUSED, mix_rows
from tests.test_per_image_cpu import host_fill

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

PNS, DEPTH, CH = (1, 2, 3, 4), 2, 32
S = len(PNS)
NC = 1000
_MODELS = {}
FIELDS = ('tokens', 'logp_class', 'logp_guided', 'logp_drawn', 'kept', 'entropy')


def _model():
    """this file's own model (VAR.forward drops labels at random unless cond_drop_rate is 0: set here, on a model no other file sees)"""
    if 'm' not in _MODELS:
        from models import build_vae_var
        from var_amd.detinit import fill_module_device_
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=DEPTH, ch=CH)
        fill_module_device_(var, DEPTH, 0, 'var.'); fill_module_device_(vae, DEPTH, 0, 'vae.')
        var.cond_drop_rate = 0.0
        _MODELS['m'] = (vae.eval(), var.eval())
    return _MODELS['m']


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, rows_a=slice(None), rows_b=slice(None), fields=FIELDS, what=''):
    for k in fields:
        assert torch.equal(_bits(getattr(a, k)[rows_a]), _bits(getattr(b, k)[rows_b])), f'{what}{k} differs'


# ---- reduction to the per-image call -----------------------------------------------------------------------------------------------------
PER = dict(labels=[3, 980, 1000, 417], seeds=[17, 3, (1 << 62) + 5, 0], cfg=[4.0, 1.5, 0.0, 2.5], top_k=[0, 900, 1, 600], top_p=[0.96, 0.0, 0.0, 0.5])


@pytest.mark.parametrize('prec', ['f32', 'f16', 'bf16'])
def test_one_class_of_weight_one_is_the_per_image_scored_call(prec):
    vae, var = _model()
    var.set_hip_precision(prec)
    try:
        d = PER
        ref = var.autoregressive_infer_cfg_per_image_scored(d['labels'], d['seeds'], cfg=d['cfg'], top_k=d['top_k'], top_p=d['top_p'])
        ref_img = ref.images.clone()
        rec = var.sample_composed([[x] for x in d['labels']], np.ones((4, 1)), d['seeds'], cfg=d['cfg'], top_k=d['top_k'], top_p=d['top_p'])
        assert torch.equal(rec.tokens, ref.tokens), f'{prec}: tokens differ from the per-image call'
        assert torch.equal(_bits(rec.images), _bits(ref_img)), f'{prec}: images differ from the per-image call'
        _same(rec, ref, fields=('logp_guided', 'logp_drawn', 'kept', 'entropy'), what=prec + ': ')
        assert torch.equal(_bits(rec.logp_class[:, 0]), _bits(ref.logp_cond)), f'{prec}: logp_class[:, 0] is not logp_cond'
        assert rec.logp_class.shape == (4, 2, var.L) and rec.coef.shape == (S, 4, 2) and rec.coef.dtype == np.float32 and rec.patch_nums == PNS
        for si in range(S):
            for b in range(4):
                t = d['cfg'][b] * (si / (S - 1))
                assert rec.coef[si, b].tobytes() == np.asarray([1 + t, t], np.float32).tobytes()
        nod = var.sample_composed([[x] for x in d['labels']], torch.ones(S, 4, 1), d['seeds'], cfg=d['cfg'], top_k=d['top_k'], top_p=d['top_p'], decode=False)
        assert nod.images is None and 'ComposedRecord(B=4, K=1' in repr(nod)
        _same(nod, rec)
    finally:
        var.set_hip_precision('f32')


# ---- batch invariance ----------------------------------------------------------------------------------------------------------------------
def _deck():
    """five unrelated requests of K = 3 (one uses two classes: a zero weight), per-scale weights on one of them"""
    labels = [[3, 980, 22], [1000, 417, 5], [207, 207, 1], [9, 8, 7], [500, 3, 980]]
    w = np.zeros((S, 5, 3))
    w[:, 0] = [0.5, 0.5, 0.0]
    w[:, 1] = [1.0, 1.0, -1.0]
    w[:, 2] = [0.25, 0.25, 0.5]
    w[:, 3] = [2.0, -0.5, -0.5]
    w[:2, 4] = [1.0, 0.0, 0.0]; w[2:, 4] = [0.0, 0.7, 0.3]
    return dict(labels=labels, w=w, seeds=[17, 3, (1 << 62) + 5, 0, 99991], cfg=[4.0, 1.5, 0.0, 2.5, 1.5], top_k=[0, 900, 1, 600, 0],
                top_p=[0.96, 0.0, 0.0, 0.5, 0.0])


def _call(var, ids, max_rows=128, decode=True):
    d = _deck()
    return var.sample_composed([d['labels'][i] for i in ids], d['w'][:, ids], [d['seeds'][i] for i in ids], cfg=[d['cfg'][i] for i in ids],
                               top_k=[d['top_k'][i] for i in ids], top_p=[d['top_p'][i] for i in ids], max_rows=max_rows, decode=decode)


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_a_request_does_not_depend_on_its_batch_or_on_max_rows(prec):
    vae, var = _model()
    var.set_hip_precision(prec)
    try:
        full = _call(var, [0, 1, 2, 3, 4])
        img = full.images.clone()
        assert img.shape == (5, 3, 64, 64) and bool(torch.isfinite(img).all()) and len({tuple(t.tolist()) for t in full.tokens}) == 5
        perm = [4, 0, 3, 1, 2]
        moved = _call(var, perm)
        for j, i in enumerate(perm):
            _same(moved, full, slice(j, j + 1), slice(i, i + 1), what=f'{prec} request {i} at position {j}: ')
            assert torch.equal(_bits(moved.images[j]), _bits(img[i])), f'{prec}: the image of request {i} changed with its position'
        for mr in (8, 4, 11):                                   # passes of 2 + 2 + 1, of 1 image each, of 2 + 2 + 1 (11 // 4 = 2)
            split = _call(var, [0, 1, 2, 3, 4], max_rows=mr)
            _same(split, full, what=f'{prec} max_rows {mr}: ')
            assert torch.equal(_bits(split.images), _bits(img)), f'{prec}: max_rows = {mr} changed the images'
        for i in range(5):
            one = _call(var, [i])
            _same(one, full, slice(0, 1), slice(i, i + 1), what=f'{prec} request {i} alone: ')
            assert torch.equal(_bits(one.images[0]), _bits(img[i])), f'{prec}: the image of request {i} alone differs from its image in the batch'
    finally:
        var.set_hip_precision('f32')


# ---- independent reconstruction, and the statistics against float64 ----------------------------------------------------------------------
def _class_logits(vae, var, tokens, labels):
    """(G, B, L, V) fp32: every class row's logits (the unconditional row last) from the teacher-forced VAR.forward on the returned tokens —
    equal to the sampling logits bit for bit"""
    B = tokens.shape[0]
    labs = [labels[:, k] for k in range(labels.shape[1])] + [torch.full((B,), NC, dtype=torch.int64)]
    with torch.no_grad():                          # (with autograd on, both calls take their PyTorch paths, which round differently)
        xin = vae.quantize.idxBl_to_var_input([tokens[:, b0:e0] for b0, e0 in var.begin_ends])
        return torch.stack([var(lab.cuda(), xin).float() for lab in labs]).cpu().numpy()


def _rebuild(vae, var, rec, seeds, ks, ps):
    """-> per scale (mixed rows, filtered rows, tokens) from the class logits, the numpy twin, the host fill and the pinned rows entry"""
    B, V = rec.tokens.shape[0], var.V
    lg = _class_logits(vae, var, rec.tokens, rec.labels)
    cap = V if 0 in ks else max(ks)
    out = []
    for si, ((b0, e0), pn) in enumerate(zip(var.begin_ends, PNS)):
        l = pn * pn
        mixed = mix_rows(lg[:, :, b0:e0], rec.coef[si])
        noise = torch.from_numpy(host_fill(seeds, l, V, si, 0)).cuda()
        pair = torch.from_numpy(np.concatenate((mixed, np.zeros_like(mixed)))).cuda()
        idx = torch.full((B * l,), -7, dtype=torch.int64, device='cuda')
        masked = torch.full((B * l, V), float('nan'), device='cuda')
        util.guarded_call('cfg_sample_rows_f32', pair, noise, idx, masked, B, l, V, torch.zeros(B, dtype=torch.float64, device='cuda'),
                          torch.tensor(ks, dtype=torch.int32, device='cuda'), torch.tensor(ps, dtype=torch.float64, device='cuda'), cap)
        out.append((mixed, masked.cpu().numpy(), idx.view(B, l).cpu()))
    return out


CASES = {
    'hybrid': dict(labels=[[3, 980], [417, 22]], weights=[[0.5, 0.5], [0.5, 0.5]], cfg=[0.0, 1.5]),
    'negative': dict(labels=[[3, 980, 22], [1000, 417, 5]], weights=[[1.0, 0.5, -0.5], [0.7, -1.0, 0.8]], cfg=[1.5, 0.0]),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_tokens_and_statistics_are_rebuilt_from_teacher_forced_logits(case):
    vae, var = _model()
    c = CASES[case]
    seeds, ks, ps = [11, 12], [900, 0], [0.96, 0.0]
    rec = var.sample_composed(c['labels'], c['weights'], seeds, cfg=c['cfg'], top_k=ks, top_p=ps)
    V = var.V
    for si, (mixed, masked, idx) in enumerate(_rebuild(vae, var, rec, seeds, ks, ps)):
        b0, e0 = var.begin_ends[si]
        assert torch.equal(idx, rec.tokens[:, b0:e0].cpu()), f'{case}: scale {si}: the rebuilt tokens differ\n{idx}\n{rec.tokens[:, b0:e0]}'
        B, l = idx.shape
        ref = R.reference(np.concatenate((mixed, np.zeros_like(mixed))), masked, idx.numpy(), B, l, 0.0)
        got = dict(lp_cond=rec.logp_guided[:, b0:e0].cpu().numpy(), lp_guided=rec.logp_guided[:, b0:e0].cpu().numpy(),
                   lp_drawn=rec.logp_drawn[:, b0:e0].cpu().numpy(), kept=rec.kept[:, b0:e0].cpu().numpy(), entropy=rec.entropy[:, b0:e0].cpu().numpy())
        R.check_against_reference(got, ref, V, f'{case} scale {si}: ')
        assert (got['kept'][0] <= 900).all() and (got['kept'][1] == V).all()
        assert np.array_equal(got['lp_drawn'][1].view(np.uint32), got['lp_guided'][1].view(np.uint32))          # nothing filtered on image 1


# ---- a schedule over the scales ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [1, 2, 3])
def test_schedule_follows_class_a_below_the_switch_and_scores_every_class(s):
    vae, var = _model()
    a, b, seed, kw = 3, 980, 77, dict(cfg=1.5, top_k=900, top_p=0.96)
    w = np.zeros((S, 1, 2))
    w[:s, 0, 0] = 1.0
    w[s:, 0, 1] = 1.0
    rec = var.sample_composed([[a, b]], w, [seed], **kw)
    only_a = var.autoregressive_infer_cfg_per_image_scored([a], [seed], **kw)
    cut = var.begin_ends[s][0]
    assert torch.equal(rec.tokens[:, :cut], only_a.tokens[:, :cut]), f'switch at {s}: the scales below it are not the plain request for class a'
    for k in ('logp_guided', 'logp_drawn', 'kept', 'entropy'):
        assert torch.equal(_bits(getattr(rec, k)[:, :cut]), _bits(getattr(only_a, k)[:, :cut])), k
    for si in range(S):                                          # class a's coefficient below the switch, class b's from it on
        t = 1.5 * (si / (S - 1))
        one_t = np.float32(1 + t)
        assert rec.coef[si, 0].tolist() == ([one_t, 0.0, np.float32(t)] if si < s else [0.0, one_t, np.float32(t)]), (si, rec.coef[si, 0])
    tail = var.token_log_likelihood(rec.tokens, torch.tensor([[b]]), cfg=1.5)[:, 0, cut:]
    assert torch.equal(_bits(tail), _bits(rec.logp_guided[:, cut:])), f'switch at {s}: from the switch on the guided row is not class b\'s'
    lp = var.token_log_likelihood(rec.tokens, torch.tensor([[a, b, NC]]), cfg=0.0)
    assert torch.equal(_bits(lp), _bits(rec.logp_class)), f'switch at {s}: logp_class is not token_log_likelihood bit for bit'


# ---- no state ------------------------------------------------------------------------------------------------------------------------------
def test_no_trace_in_the_engine_and_poisoned_workspaces_change_nothing():
    from tests import test_call_order_gpu as co
    vae, var = _model()
    labels = torch.tensor([3, 7, 980], device='cuda')
    plain = lambda: var.autoregressive_infer_cfg(3, labels, g_seed=0, cfg=1.5, top_k=900, top_p=0.96).clone()
    per = lambda: [x.clone() for x in var.autoregressive_infer_cfg_per_image([3, 980], [5, 6], cfg=[1.5, 4.0], top_k=900, top_p=0.96, return_tokens=True)]
    comp = lambda: _call(var, [0, 1, 4], max_rows=8)
    a, p = plain(), per()
    state = var.rng.get_state().clone()
    c1 = comp()
    c1_img = c1.images.clone()
    assert torch.equal(var.rng.get_state(), state), 'sample_composed must not touch the model generator'
    assert torch.equal(_bits(plain()), _bits(a)), 'the plain call changed after a composed call'
    p2 = per()
    assert torch.equal(p2[1], p[1]) and torch.equal(_bits(p2[0]), _bits(p[0])), 'the per-image call changed after a composed call'
    c2 = comp()
    _same(c2, c1, what='repeated after other calls: ')
    assert torch.equal(_bits(c2.images), _bits(c1_img))
    eng = var.engine()
    assert any(len(k) == 4 for k in eng._ws), 'the composed call keeps its buffer sets where the poisoning reaches them'
    assert len(eng._ws) <= eng.MAX_WORKSPACES
    written = 0
    for fn, want in ((plain, a), (comp, None), (per, p), (comp, None), (plain, a)):
        torch.cuda.synchronize()
        written += co.poison_engines(vae, var)
        co.poison_allocator()
        torch.cuda.synchronize()
        got = fn()
        if want is None:
            _same(got, c1, what='poisoned: ')
            assert torch.equal(_bits(got.images), _bits(c1_img)), 'poisoned: the composed images changed'
        elif isinstance(want, list):
            assert torch.equal(got[1], want[1]) and torch.equal(_bits(got[0]), _bits(want[0])), 'poisoned: the per-image call changed'
        else:
            assert torch.equal(_bits(got), _bits(want)), 'poisoned: the plain call changed'
    assert written >= 100, written
    assert co.unlisted_kept_tensors(vae, var)[0] == [], 'a composed call parked a tensor outside the poisoned and the derived attributes'


# ---- validation ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_surface_as_value_errors_before_any_launch():
    from var_amd import hip
    vae, var = _model()
    good = dict(labels=[[1, 2], [3, 1000]], weights=[[0.5, 0.5], [2.0, -1.0]], g_seeds=[5, 6], cfg=1.5, top_k=0, top_p=0.0, max_rows=128)
    var.sample_composed(**good)
    hip.timing_reset(); hip.timing_enable(True)
    try:
        for what, over in sorted(REFUSED.items()):
            with pytest.raises(ValueError):
                var.sample_composed(**{**good, **over})
        with pytest.raises(ValueError):
            var.sample_composed(**{**good, 'weights': np.ones((S + 1, 2, 2))})
        launches = sum(v['launches'] for v in hip.timing_read().values())
    finally:
        hip.timing_enable(False); hip.timing_reset()
    assert launches == 0, f'{launches} kernels were launched by refused calls'
    var.train()
    try:
        with pytest.raises(RuntimeError, match='HIP kernels only'):
            var.sample_composed(**good)
    finally:
        var.eval()
